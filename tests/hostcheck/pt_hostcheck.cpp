// pt_hostcheck.cpp — TEST INFRASTRUCTURE.  Compiles the render kernel's own
// per-lane code (pathtracerpython_amd/csrc/pt_path.h, pt_core.h, pt_prepare.h)
// for the host with g++, so the CPU test suite can check the kernel logic —
// in particular the f32 filter's "certain" verdicts — against the oracle and
// against its own FORCE_F64 mode without a GPU.  Never used by the product.
#define __host__
#define __device__
#define __forceinline__ inline
#include <cstddef>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <random>
#include <type_traits>
#include <vector>

#include "../../pathtracerpython_amd/csrc/pt_path.h"
#include "../../pathtracerpython_amd/csrc/pt_wavefront.h"
#include "../../pathtracerpython_amd/csrc/pt_prepare.h"
#include "../../pathtracerpython_amd/csrc/pt_plan.h"
#include "../devcheck/filter_eval.h"

using namespace pt;

// The launch record of the rows first, first + row_step, ... (n_rows of them)
// of p's frame with `split` slots per pixel, as pt_render_device fills it:
// plan_frame's, on a BVH scene (no tail rows), with lanes_per_pixel = split.
static const PlanScene kHostBvhScene{true, true, 256, false, 0.0};
static RenderK host_frame(const pt_render_params* p, int32_t first, int32_t row_step, int32_t n_rows,
                          uint32_t split) {
    pt_render_params q = *p;
    q.row_step = row_step;
    q.lanes_per_pixel = (int32_t)split;
    RenderK R;
    LaunchPlan L;
    (void)plan_frame(&q, kHostBvhScene, first, n_rows, &R, &L);
    return R;
}

// ---- the lane driver: what every hc_* entry that runs lane code shares ----

// prepare_scene and bind_host; false: the scene (with its lens, its box) is refused
static inline bool open_scene(const pt_scene_desc* d, HostScene* H, const pt_lens* L = nullptr,
                              const double* box = nullptr) {
    if (!prepare_scene(d, H, L, box).empty()) return false;
    bind_host(H);
    return true;
}
// An opened scene with one lane's spill home and the counters the lanes bump
struct Host {
    HostScene H;
    Counters c = {};
    double spill_mem[kSpillSlots];
    const Spill sp{spill_mem, 1};
    bool open(const pt_scene_desc* d, const pt_lens* L = nullptr, const double* box = nullptr) {
        return open_scene(d, &H, L, box);
    }
};

// A runtime choice as a template argument: f(std::true_type{}) or f(std::false_type{})
template <class F>
auto with_bool(bool b, F&& f) {
    return b ? f(std::true_type{}) : f(std::false_type{});
}

static inline uint32_t pixel_key(const pt_render_params* p, int ix, int iy) {
    return (uint32_t)ix * (uint32_t)p->height + (uint32_t)iy;
}
static inline size_t image_index(const pt_render_params* p, int ix, int iy) {
    return (size_t)(p->height - 1 - iy) * p->width + ix;
}
static inline void st3(double* o, D3 v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }
static inline void add3(double* o, D3 v) { o[0] += v.x; o[1] += v.y; o[2] += v.z; }

// The job of n_samples samples from sample0 on under p (pt_radiance's launches
// clamp rr_depth at 0: their callers pass a p that has it)
static inline LaneJob lane_job(const pt_render_params* p, uint32_t pixel, int32_t sample0, int32_t stride,
                               int32_t n_samples) {
    return LaneJob{p->seed, pixel, sample0, stride, n_samples, p->bounces,
                   (p->flags & PT_FLAG_RR) ? p->rr_depth : -1};
}
// lane l of `lanes` emulated lanes: samples sample_begin + l, + lanes, ...
static inline LaneJob lane_of(const pt_render_params* p, uint32_t pixel, int l, int lanes) {
    return lane_job(p, pixel, p->sample_begin + l, lanes, l < p->spp ? (p->spp - l + lanes - 1) / lanes : 0);
}
// the xor butterfly of store_pixel over a power of two of values; lane 0's result
static inline D3 xor_reduce(std::vector<D3> v) {
    const size_t n = v.size();
    for (size_t m = 1; m < n; m <<= 1) {
        std::vector<D3> w(n);
        for (size_t i = 0; i < n; ++i) w[i] = v[i] + v[i ^ m];
        v = w;
    }
    return v[0];
}

// One lane through the prologue its primary source takes (P0: a cached hit's
// point; COUNT: FrameHit's counting form)
template <bool F64, bool COUNT, class Primary, class Sink>
auto run_lane(Host& h, const LaneJob& J, const Primary& prim, D3 P0, Sink sink) {
    if constexpr (Primary::kCached) return render_lane_cached<F64, COUNT, true>(h.H.k, J, prim, P0, h.sp, &h.c, sink);
    else return render_lane_sampled<F64, true>(h.H.k, J, prim, h.sp, &h.c, sink);
}
// ... with both sinks: the sum of SumSink, then the moments of MomentSink
struct LaneSums {
    D3 a, s, q;
};
template <bool F64, class Primary>
LaneSums both_sinks(Host& h, const LaneJob& J, const Primary& prim, D3 P0) {
    MomentRegs M;
    M.clear();
    const D3 a = run_lane<F64, false>(h, J, prim, P0, SumSink{});
    run_lane<F64, false>(h, J, prim, P0, MomentSink<MomentRegs>{M});
    return LaneSums{a, M.sum(), M.sumsq()};
}
// One element (a pixel, a ray record): lane(J) of each of its `lanes` (a power
// of two) emulated lanes, reduced in store_pixel's xor order into row e of
// sum, S and Q
template <class Lane>
void store_lanes(const pt_render_params* p, uint32_t pixel, int lanes, size_t e, double* sum, double* S, double* Q,
                 Lane&& lane) {
    std::vector<D3> a(lanes), s(lanes), q(lanes);
    for (int l = 0; l < lanes; ++l) {
        const LaneSums r = lane(lane_of(p, pixel, l, lanes));
        a[l] = r.a; s[l] = r.s; q[l] = r.q;
    }
    st3(sum + 3 * e, xor_reduce(a));
    st3(S + 3 * e, xor_reduce(s));
    st3(Q + 3 * e, xor_reduce(q));
}

// Pixel (ix, iy)'s centre ray and its hit, which every sample restarts from (main.py:191)
struct CentreHit {
    FrameHit hit;
    D3 P0;
};
template <bool F64>
CentreHit centre_hit(Host& h, const pt_render_params* p, int ix, int iy) {
    const SceneK& K = h.H.k;
    const D3 eye = ld3(K.eye);
    const double x = linspace_at(K.ortho[0], K.ortho[2], p->width, ix);
    const double y = linspace_at(K.ortho[1], K.ortho[3], p->height, iy);
    CentreHit r{{-1, d3(x - eye.x, y - eye.y, 0.0 - eye.z)}, d3(0, 0, 0)};
    if (p->bounces > 0) r.hit.tri0 = closest<F64, false>(K, eye, r.hit.d0, -1, h.sp, &r.P0, &h.c, true);
    return r;
}
// The ladder over (force64, PT_FLAG_LENS, PT_FLAG_AA), once: f(F64, prim, P0)
// with the primary source of pixel (ix, iy) they select — a ray per sample from
// LensRay or AaRay, or with neither flag the centre ray's cached hit
static const AaEye kNoEye{nullptr, 0};   // (the device's per-wave table of the eye's origin terms: none here)
template <class F>
void with_primary(Host& h, const pt_render_params* p, bool force64, bool lens, bool aa, int ix, int iy, F&& f) {
    const AaPixel X{p->width, p->height, ix, iy};
    const D3 none = d3(0, 0, 0);
    with_bool(force64, [&](auto F64) {
        constexpr bool k64 = decltype(F64)::value;
        if (lens && aa) return f(F64, LensRay<k64, true, true>{X}, none);
        if (lens) return f(F64, LensRay<k64, true, false>{X}, none);
        if (aa) return f(F64, AaRay<k64, true>{X, kNoEye}, none);
        const CentreHit c = centre_hit<k64>(h, p, ix, iy);
        return f(F64, c.hit, c.P0);
    });
}

// ---- the wavefront walks, to completion (k_wf_shadow's and k_wf_closest's) ----

// A walk's observer: visit(ref, top) before a QNode (ref >= 0) or a leaf
// (ref < 0) is entered, false gives the walk up; visited(top) after a QNode.
struct NoWatch {
    bool visit(int, int) { return true; }
    void visited(int) {}
};
template <class V, class A>
struct Watcher {
    V v;
    A a;
    bool visit(int ref, int top) { return v(ref, top); }
    void visited(int top) { a(top); }
};
template <class V, class A>
Watcher<V, A> watcher(V v, A a) {
    return {v, a};
}
// the node visits' peak of a walk on the walk kernels' stacks: pk[0] the
// largest T.top after a node visit, pk[1] the visits that left T.top above
// their shared-memory part (16 entries)
static inline auto peak_watch(int64_t* pk) {
    return watcher([](int, int) { return true; },
                   [pk](int top) {
                       pk[0] = std::max<int64_t>(pk[0], top);
                       if (top > 16) ++pk[1];
                   });
}

// shadow ray k of a query, on the stack view St; false: the observer gave up
template <class Watch = NoWatch>
bool walk_shadow(const SceneK& K, WfShadowQ* q, int k, const Spill& sp, const ShadowStack& St, Watch&& w = Watch{}) {
    Shadow1 r;
    F3 o32;
    int ogrp;
    wf_get_shadow1(*q, k, &o32, &ogrp, &r);
    ShadowTrav1 T;
    s1_init(T, K, o32, ogrp, r, K.qroot);
    while (T.ref != kNoRef) {
        while (T.ref >= 0) {
            if (!w.visit(T.ref, T.top)) return false;
            s1_qnode(T, St, K, r);
            w.visited(T.top);
        }
        if (T.ref != kNoRef) {
            if (!w.visit(T.ref, T.top)) return false;
            if (K.bunitc) s1_units<true, PT_WF_LRNG != 0>(T, K, &r, sp, T.ref);
            else s1_units<false, PT_WF_LRNG != 0>(T, K, &r, sp, T.ref);
            T.ref = s1_pop(T, St, K, r);
        }
    }
    wf_put_shadow1(q, r);
    return true;
}
// a closest query likewise
template <class Watch = NoWatch>
bool walk_closest(const SceneK& K, WfClosestQ* q, const Spill& sp, const ClosestStack& St, Watch&& w = Watch{}) {
    ClosestAcc ca = wf_get_acc(*q);
    ClosestTrav T;
    ctrav_init(T, K, F3{q->o[0], q->o[1], q->o[2]}, q->ogrp, F3{q->d[0], q->d[1], q->d[2]}, ca.b1, K.qroot);
    while (T.ref != kNoRef) {
        while (T.ref >= 0) {
            if (!w.visit(T.ref, T.top)) return false;
            ctrav_qnode(T, St, K, &ca);
            w.visited(T.top);
        }
        if (T.ref != kNoRef) {
            if (!w.visit(T.ref, T.top)) return false;
            if (K.bunitc) ctrav_leaf<false, true>(T, St, K, &ca, sp, nullptr);   // as k_wf_closest
            else ctrav_leaf<false>(T, St, K, &ca, sp, nullptr);
        }
    }
    q->a1 = ca.a1; q->a2 = ca.a2; q->b1 = ca.b1; q->i1 = ca.i1;
    return true;
}
// Every walk the slots' shade steps asked for (want[t]), on per-lane local stacks
static inline void run_walks(const SceneK& K, const std::vector<uint32_t>& want, WfPath* W, WfShadowQ* SQ,
                             WfClosestQ* CQ) {
    for (size_t t = 0; t < want.size(); ++t) {
        const Spill sp{W[t].sp, 1};
        int buf[kBvhStackLocal];
        ClosestStackLocal L;
        for (int k = 0; k < kLightSamples; ++k)
            if ((want[t] >> k) & 1u) walk_shadow(K, &SQ[t], k, sp, ShadowStack{buf, 1});
        if (want[t] & kWfWantClosest) walk_closest(K, &CQ[t], sp, L.view());
    }
}
// a prepared scene the wavefront kernels take: a BVH whose walks fit their stacks
static inline bool wf_walkable(const SceneK& K) { return K.n_bnode != 0 && K.n_qnode != 0 && K.qstack <= kBvhStack; }
// a slot count per pixel, entry or record: a power of two up to 64
static inline bool split_ok(uint32_t split) { return split != 0 && split <= 64 && (split & (split - 1)) == 0; }

extern "C" {

// sizes and field offsets of the C-ABI structs as the C++ compiler lays
// them out (the ctypes mirror in _abi.py must agree)
int hc_abi_layout(int64_t* out) {
    out[0] = (int64_t)sizeof(pt_scene_desc);
    out[1] = (int64_t)sizeof(pt_render_params);
    out[2] = (int64_t)sizeof(pt_stats);
    out[3] = (int64_t)offsetof(pt_stats, shadow_queries);
    out[4] = (int64_t)offsetof(pt_stats, shade_ms);
    out[5] = (int64_t)offsetof(pt_stats, closest_launches);
    out[6] = (int64_t)offsetof(pt_scene_desc, light_rgb);
    out[7] = (int64_t)offsetof(pt_render_params, sample_begin);
    return 0;
}

// Render the band of p on the host with the kernel's lane code (split = 1).
// out: rows*W*3 float64 in image orientation.  counters[8] (optional).
int hc_render(const pt_scene_desc* d, const pt_render_params* p, int force64,
              double* out, uint64_t* counters) {
    Host h;
    if (!h.open(d)) return -1;
    int32_t first, rows;
    if (!band_layout(p, &first, &rows)) return -2;
    for (int r = 0; r < rows; ++r) {
        const int iy = first + r * p->row_step;
        for (int ix = 0; ix < p->width; ++ix) {
            // counters requested: the count-mode lane code (exact first
            // occluders); else the render kernel's own (object-level) one
            const D3 acc = with_bool(force64 != 0, [&](auto F64) {
                return with_bool(counters != nullptr, [&](auto COUNT) {
                    const CentreHit c = centre_hit<decltype(F64)::value>(h, p, ix, iy);
                    return run_lane<decltype(F64)::value, decltype(COUNT)::value>(
                        h, lane_of(p, pixel_key(p, ix, iy), 0, 1), c.hit, c.P0, SumSink{});
                });
            });
            double* o = out + ((size_t)(rows - 1 - r) * p->width + ix) * 3;
            o[0] = acc.x / p->spp; o[1] = acc.y / p->spp; o[2] = acc.z / p->spp;
        }
    }
    if (counters) {
        const Counters& c = h.c;
        uint32_t v[8] = {c.closest_tests, c.shadow_tests, c.ray_bounces, c.shading_points,
                         c.light_hits, c.escapes, c.fallbacks, c.rescans};
        for (int i = 0; i < 8; ++i) counters[i] = v[i];
    }
    return 0;
}

// The wavefront form of the render (pt_wavefront.h) run on the host: every
// shade step over all slots, then every pending shadow and closest walk to
// completion, as the GPU's shade / walk kernels do (split = 1, one slot per
// pixel).  Must equal hc_render (force64 = 0, no counters) bit for bit.
// steps_out (optional): shade steps that found work.
// walk_stats (optional, int64[8]): shadow rays walked, node visits, leaves,
// leaf units; the same for the closest walks.
// depth_hist (optional, int64[2][32]): node visits of the shadow / closest
// walks by QNode depth (root = 0)
// lds_entries: 0 runs the walks on per-lane local arrays (whose views never
// leave their first part); n in 1 .. kBvhStack runs them on the split views
// of the walk kernels (pt_hip.hip k_wf_shadow / k_wf_closest): entries below
// n in one heap block of exactly n elements, entries n .. kBvhStack - 1 in
// another of exactly kBvhStack - n, so an index outside either part is a heap
// overrun (the sanitize build reports it).  The framebuffer must not depend
// on it.  The GPU's split is n = 16 (PT_WALK_STACK_LDS).
// peak (optional, int64[4]): the largest T.top after a node visit of the
// shadow / closest walks, and their node visits that left T.top > 16.
int hc_render_wavefront3(const pt_scene_desc* d, const pt_render_params* p, double* out,
                         int32_t* steps_out, int64_t* walk_stats, int64_t* depth_hist,
                         int32_t lds_entries, int64_t* peak);
int hc_render_wavefront2(const pt_scene_desc* d, const pt_render_params* p, double* out,
                         int32_t* steps_out, int64_t* walk_stats, int64_t* depth_hist) {
    return hc_render_wavefront3(d, p, out, steps_out, walk_stats, depth_hist, 0, nullptr);
}
int hc_render_wavefront(const pt_scene_desc* d, const pt_render_params* p, double* out,
                        int32_t* steps_out, int64_t* walk_stats) {
    return hc_render_wavefront2(d, p, out, steps_out, walk_stats, nullptr);
}
int hc_render_wavefront3(const pt_scene_desc* d, const pt_render_params* p, double* out,
                         int32_t* steps_out, int64_t* walk_stats, int64_t* depth_hist,
                         int32_t lds_entries, int64_t* peak) {
    int64_t ws[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t pk[4] = {0, 0, 0, 0};
    if (lds_entries < 0 || lds_entries > kBvhStack) return -4;
    // the split stacks' two parts (stale entries stay between walks, as in
    // the kernels' shared and global memory)
    const int nl = lds_entries, ng = kBvhStack - lds_entries;
    std::unique_ptr<int[]> s_lds, s_glob, c_ref, c_gref;
    std::unique_ptr<uint16_t[]> c_dist, c_gdist;
    if (nl > 0) {
        s_lds.reset(new int[nl]);
        s_glob.reset(new int[ng]);
        c_ref.reset(new int[nl]);
        c_gref.reset(new int[ng]);
        c_dist.reset(new uint16_t[nl]);
        c_gdist.reset(new uint16_t[ng]);
        std::fill_n(s_lds.get(), nl, kNoRef);
        std::fill_n(s_glob.get(), ng, kNoRef);
        std::fill_n(c_ref.get(), nl, kNoRef);
        std::fill_n(c_gref.get(), ng, kNoRef);
        // (distances start as +inf: an entry whose store was lost is dropped on
        // its pop instead of passing every bound)
        std::fill_n(c_dist.get(), nl, (uint16_t)0x7f80);
        std::fill_n(c_gdist.get(), ng, (uint16_t)0x7f80);
    }
    // a walk visits a QNode or a leaf at most once and holds at most kBvhStack
    // entries: anything else is a corrupted stack (-5 instead of a walk that
    // never ends or leaves the tree)
    HostScene H;
    if (!open_scene(d, &H)) return -1;
    auto sane = [&](int ref, int top, int64_t work) {
        return ref < (int)H.qnode.size() && top >= 0 && top <= kBvhStack &&
               work <= 5 * (int64_t)H.qnode.size() + 1;
    };
    auto seen = [&](int kind, int top) {
        pk[kind] = std::max<int64_t>(pk[kind], top);
        if (top > 16) ++pk[2 + kind];
    };
    std::vector<int> qdepth(H.qnode.size(), 0);
    if (depth_hist && H.k.qroot >= 0) {   // depth of every QNode (refs point deeper)
        std::vector<int> st{H.k.qroot};
        while (!st.empty()) {
            const int q = st.back();
            st.pop_back();
            for (int c = 0; c < 4; ++c) {
                const int r = H.qnode[q].ref[c];
                if (r >= 0) { qdepth[r] = qdepth[q] + 1; st.push_back(r); }
            }
        }
    }
    auto hist = [&](int kind, int ref) {
        if (depth_hist && ref >= 0) ++depth_hist[kind * 32 + std::min(qdepth[ref], 31)];
    };
    // a walk's observer: the sanity check, the depth histogram, the counts and the peak
    auto watch = [&](int kind, int64_t& work) {
        return watcher(
            [&, kind](int ref, int top) {
                if (!sane(ref, top, ++work)) return false;
                hist(kind, ref);
                if (ref < 0) {
                    ++ws[4 * kind + 2];
                    ws[4 * kind + 3] += (~ref) & 7;
                }
                return true;
            },
            [&, kind](int top) {
                ++ws[4 * kind + 1];
                seen(kind, top);
            });
    };
    if (!wf_walkable(H.k)) return -3;
    int32_t first, rows;
    if (!band_layout(p, &first, &rows)) return -2;
    const size_t n = (size_t)rows * p->width;
    const RenderK R = host_frame(p, first, p->row_step, rows, 1);
    const WfFrame src{R};
    // (split = 1: a pixel's primary query is its one slot's own, CQP = CQ)
    std::vector<WfPath> W(n);
    std::vector<WfShadowQ> SQ(n);
    std::vector<WfClosestQ> CQ(n);
    std::vector<uint32_t> want(n);
    int32_t busy = 0;
    for (int step = 0;; ++step) {
        bool any = false;
        for (size_t i = 0; i < n; ++i) {   // the shade kernel's step, then (step 0) the primary kernel's
            any |= step > 0 && W[i].state() != kWfDone;
            want[i] = wf_slot_step<false>(H.k, src, step, (uint32_t)i, W.data(), SQ.data(), CQ.data(), CQ.data(),
                                          WfSum{}) & 0xffffu;
            if (step == 0) want[i] = wf_primary_step(H.k, src, (uint32_t)i, W.data(), CQ.data());
        }
        if (step > 0 && !any) break;
        ++busy;
        for (size_t i = 0; i < n; ++i) {
            const Spill sp{W[i].sp, 1};
            for (int k = 0; k < kLightSamples; ++k) {   // one walk per open shadow ray, as k_wf_shadow
                if (!((want[i] >> k) & 1u)) continue;
                ++ws[0];
                int buf[kBvhStackLocal];
                const ShadowStack K = nl > 0 ? ShadowStack{s_lds.get(), 1, s_glob.get(), 1, nl}
                                             : ShadowStack{buf, 1};
                int64_t work = 0;
                if (!walk_shadow(H.k, &SQ[i], k, sp, K, watch(0, work))) return -5;
            }
            if (want[i] & kWfWantClosest) {
                ClosestStackLocal L;
                const ClosestStack K =
                    nl > 0 ? ClosestStack{c_ref.get(), c_dist.get(), 1, c_gref.get(), c_gdist.get(), 1, nl}
                           : L.view();
                ++ws[4];
                int64_t work = 0;
                if (!walk_closest(H.k, &CQ[i], sp, K, watch(1, work))) return -5;
            }
        }
    }
    for (int r = 0; r < rows; ++r)
        for (int ix = 0; ix < p->width; ++ix) {
            const size_t i = (size_t)r * p->width + ix;
            double* o = out + ((size_t)(rows - 1 - r) * p->width + ix) * 3;
            o[0] = W[i].acc[0] / p->spp; o[1] = W[i].acc[1] / p->spp; o[2] = W[i].acc[2] / p->spp;
        }
    if (steps_out) *steps_out = busy;
    if (walk_stats) memcpy(walk_stats, ws, sizeof(ws));
    if (peak) memcpy(peak, pk, sizeof(pk));
    return 0;
}

// BVH shape: out[6] = {n_bnode, bvh_depth, n_qnode, qstack, n_bunitc, bvh_obj1}
int hc_bvh_info(const pt_scene_desc* d, int32_t* out) {
    HostScene H;
    if (!prepare_scene(d, &H).empty()) return -1;
    out[0] = H.k.n_bnode;
    out[1] = H.k.bvh_depth;
    out[2] = H.k.n_qnode;
    out[3] = H.k.qstack;
    out[4] = (int32_t)H.bunitc.size();   // the walks' 64-B unit form (0: not used)
    out[5] = H.k.bvh_obj1;
    return 0;
}

}   // extern "C"
struct FilterArrays {   // hc_filter_cases' arrays: [n] lines, results as ptcheck::FilterOut
    double* o; double* dn; double* lim;
    float* hlo; float* hhi;
    int32_t* at_eye;
    ptcheck::FilterOut out;
    int8_t* near;   // [n][nu][2] eval64_near, or null
};
// eval64's decisions of this line and triangle within `rel` (relative) of
// their thresholds: |n.d| against 1e-5, the two weight products against 0
// (relative to their factors' lengths), sqd against 1e-5 and against lim —
// a build whose reciprocal differs in the last place may decide these the
// other way, so the device check compares its eval64 on the others.
static bool eval64_near(const TriD& T, D3 o, D3 dn, double lim, double rel) {
    const D3 vp = ld3(T.vp);
    const double den = fabs(dot(dn, vp));
    if (fabs(den - kZero) <= rel * kZero) return true;
    if (!(den > kZero)) return false;
    const D3 p = plane_point(T, o, dn);
    const D3 c1 = cross(ld3(T.e12), p - ld3(T.v2));
    const D3 c2 = cross(ld3(T.e23), p - ld3(T.v3));
    const D3 c3 = cross(ld3(T.e31), p - ld3(T.v1));
    const double n1 = sqrt(dot(c1, c1)), n2 = sqrt(dot(c2, c2)), n3 = sqrt(dot(c3, c3));
    if (fabs(dot(c1, c2)) <= rel * n1 * n2 || fabs(dot(c1, c3)) <= rel * n1 * n3) return true;
    const double sqd = squared_dist(p, o);
    return fabs(sqd - kZero) <= rel * kZero || fabs(sqd - lim) <= rel * lim;
}
// the self-test's loop: the lines, filter_line on each, the tally (X: hc_filter_cases' arrays, or null)
static int filter_run(const pt_scene_desc* d, int64_t n_rays, uint64_t seed, int64_t* out,
                      const FilterArrays* X) {
    HostScene H;
    if (!prepare_scene(d, &H).empty()) return -1;
    bind_host(&H);
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::normal_distribution<double> N(0.0, 1.0);
    int64_t wrong = 0, amb = 0, tests = 0, cand = 0, mdiff = 0;
    const int nu = H.k.n_unit + H.k.n_bunit;
    const int kKinds = ptcheck::kKinds;
    // without arrays from the caller: one line's worth, reused
    std::vector<double> s_d(7), s_sqd((size_t)nu * 2);
    std::vector<float> s_f(2), s_atdt((size_t)nu * 4), s_sum((size_t)H.k.n_obj_unit * ptcheck::kSumN + 1);
    std::vector<int8_t> s_code((size_t)nu * 2 * kKinds), s_hit((size_t)nu * 2), s_mflag(nu);
    int32_t s_eye = 0;
    FilterArrays L = X ? *X : FilterArrays{s_d.data(), s_d.data() + 3, s_d.data() + 6, s_f.data(),
                                           s_f.data() + 1, &s_eye,
                                           {s_code.data(), s_hit.data(), s_sqd.data(), s_atdt.data(),
                                            s_mflag.data(), s_sum.data()}, nullptr};
    const ptcheck::FilterLines LC = {L.o, L.dn, L.lim, L.hlo, L.hhi, L.at_eye};
    const ptcheck::FilterOut& F = L.out;
    for (int64_t i = 0; i < n_rays; ++i) {
        D3 o;
        if (i % 4 == 0) {
            o = ld3(H.k.eye);
        } else {   // a point on a random triangle (as hit points are)
            const TriD& T = H.trid[rng() % H.trid.size()];
            double a = U(rng), b = U(rng);
            if (a + b > 1) { a = 1 - a; b = 1 - b; }
            o = ld3(T.v1) + (ld3(T.v2) - ld3(T.v1)) * a + (ld3(T.v3) - ld3(T.v1)) * b;
        }
        D3 dir = d3(N(rng), N(rng), N(rng));
        if (i % 3 == 0) {   // aim near a random vertex: many near-edge lines
            const TriD& T = H.trid[rng() % H.trid.size()];
            dir = ld3(T.v1) + d3(N(rng), N(rng), N(rng)) * 1e-3 - o;
        } else if (i % 3 == 1 && (i / 3) % 2 == 0) {
            // aim at a point of a random edge, off by 1e-2 .. 1e-9: lines
            // grazing edges (e.g. from the ceiling across a wall's top edge)
            const TriD& T = H.trid[rng() % H.trid.size()];
            const D3 vv[3] = {ld3(T.v1), ld3(T.v2), ld3(T.v3)};
            const int e = (int)(rng() % 3);
            const double a = U(rng), sc = pow(10.0, -2.0 - 7.0 * U(rng));
            dir = vv[e] + (vv[(e + 1) % 3] - vv[e]) * a + d3(N(rng), N(rng), N(rng)) * sc - o;
        }
        const D3 dn = unit(dir);
        const bool at_eye = i % 4 == 0;
        const double lim = 0.5 + 40.0 * U(rng);   // a shadow range
        const float hlo = (float)(sqrt(lim) * (1 - 1e-6)), hhi = (float)(sqrt(lim) * (1 + 1e-6));
        // the line's slots: the caller's arrays, or one line's scratch
        const int64_t at = X ? i : 0;
        const double od[3] = {o.x, o.y, o.z}, dd[3] = {dn.x, dn.y, dn.z};
        memcpy(L.o + 3 * at, od, sizeof od);
        memcpy(L.dn + 3 * at, dd, sizeof dd);
        L.lim[at] = lim;
        L.hlo[at] = hlo;
        L.hhi[at] = hhi;
        L.at_eye[at] = at_eye ? 1 : 0;
        // frames: the eye's origins test unit_eye, surface origins `unit`
        // (surface frame); the BVH units are in the frame with the eye
        ptcheck::filter_line(H.k, LC, at, F, true);
        if (X && X->near)   // which f64 decisions another arithmetic may take the other way
            for (int u = 0; u < nu; ++u) {
                const bool uni = u < H.k.n_unit;
                const UnitF& Un = uni ? H.unit[u] : H.bunit[u - H.k.n_unit];
                for (int m = 0; m < 2; ++m)
                    X->near[(at * nu + u) * 2 + m] =
                        m < Un.count && eval64_near(H.trid[Un.t[m]], o, dn, lim, 1e-12) ? 1 : 0;
            }
        // the tally: this build's verdicts against its own eval64
        for (int u = 0; u < nu; ++u) {
            const bool uni = u < H.k.n_unit;
            const int64_t lu = at * nu + u;
            for (int m = 0; m < 2; ++m) {
                const int8_t* c = F.code + (lu * 2 + m) * kKinds;
                const bool h = F.hit[lu * 2 + m] != 0;
                const double sqd = F.sqd[lu * 2 + m];
                const bool ref_c = h && sqd > kZero;                       // closest semantics
                const bool ref_s = h && !(sqd < kZero) && sqd < lim;      // shadow semantics
                if (c[ptcheck::kClosest] >= 0) {   // a member triangle: the single-triangle forms
                    int st = c[ptcheck::kClosest];
                    ++tests;
                    if (st == kAmb) ++amb;
                    else if ((st == kCand) != ref_c) ++wrong;
                    else if (st == kCand) {
                        ++cand;
                        const double sq = sqrt(sqd);   // the |t| interval must cover the truth
                        const float pat = F.atdt[lu * 4], pdt = F.atdt[lu * 4 + 1];
                        if (sq < (double)pat - pdt || sq > (double)pat + pdt) ++wrong;
                    }
                    st = c[ptcheck::kShadow];
                    ++tests;
                    if (st == kAmb) ++amb;
                    else if ((st == kCand) != ref_s) ++wrong;
                    // the render loop's margin form (shadow_unit_m) of the same test
                    const int ms = c[ptcheck::kMarginF];
                    if (ms != kAmb && (ms == kCand) != ref_s) ++wrong;
                    if (ms != st && !(st == kMiss && ms == kAmb)) ++mdiff;
                }
                if (uni) {   // the render loop's unit form (quad_m): both members' tests
                    const int ms = c[ptcheck::kQuadShadow];
                    ++tests;
                    if (ms == kAmb) ++amb;
                    else if ((ms == kCand) != ref_s) ++wrong;
                    const int vc = c[ptcheck::kQuadClosest];
                    ++tests;
                    if (vc == kAmb) ++amb;
                    else if ((vc == kCand) != ref_c) ++wrong;
                    // the render loop's lean closest range (PT_CLOSEST_LEAN): no wrong certain verdict
                    const int vl = c[ptcheck::kLean];
                    if (vl != kAmb && (vl == kCand) != ref_c) ++wrong;
                    if (vl != vc && !(vc == kMiss && vl == kAmb)) ++mdiff;
                }
            }
            // the merged unit margins (PT_MMERGE, margin_unit) against the members'
            if (F.mflag[lu] & ptcheck::kMfOcc) ++mdiff;
            if (F.mflag[lu] & ptcheck::kMfLost) ++mdiff;
        }
    }
    out[0] = wrong; out[1] = amb; out[2] = tests; out[3] = cand; out[4] = mdiff;
    return 0;
}

extern "C" {
// Filter self-test: random lines (origins at the eye or on triangles,
// directions random) against every triangle; compares classify() with the
// f64 evaluation.  out[0] = wrong certain verdicts (must be 0), out[1] =
// ambiguous verdicts, out[2] = tests, out[3] = certain candidates, out[4] =
// shadow tests where the margin form (margin_plane/margin_tri) differs from
// classify_tri other than by "ambiguous" for a certain miss (must be 0).
// The tests of a line are filter_eval.h's filter_line (the code the device
// check compiles for gfx950), tallied here; hc_filter_cases also hands out
// the lines and the per-test results.
int hc_filter_selftest(const pt_scene_desc* d, int64_t n_rays, uint64_t seed, int64_t* out) {
    return filter_run(d, n_rays, seed, out, nullptr);
}

// The self-test's lines and this build's results of them, for the device
// check (tests/devcheck dc_filter runs the same lines on the GPU; the host's
// eval64 here is the truth both builds' verdicts are judged by).  The lines
// and the tally are hc_filter_selftest's own (one generator, one loop): out[5]
// as there.  Arrays as in filter_eval.h, n = n_rays, nu = n_unit + n_bunit
// (hc_filter_dims); near[n][nu][2] = eval64_near at 1e-12.
int hc_filter_cases(const pt_scene_desc* d, int64_t n_rays, uint64_t seed, double* o, double* dn,
                    double* lim, float* hlo, float* hhi, int32_t* at_eye, int8_t* code, int8_t* hit,
                    double* sqd, float* atdt, int8_t* mflag, float* sum, int8_t* near, int64_t* out) {
    FilterArrays X = {o, dn, lim, hlo, hhi, at_eye, {code, hit, sqd, atdt, mflag, sum}, near};
    return filter_run(d, n_rays, seed, out, &X);
}

// out[4] = {n_unit, n_bunit, n_obj_unit, 1 if the BVH units have the 64-B form}
int hc_filter_dims(const pt_scene_desc* d, int32_t* out) {
    HostScene H;
    if (!prepare_scene(d, &H).empty()) return -1;
    out[0] = H.k.n_unit;
    out[1] = H.k.n_bunit;
    out[2] = H.k.n_obj_unit;
    out[3] = H.bunitc.empty() ? 0 : 1;
    return 0;
}

// The host twins of the min / max family (pt_path.h, pt_core.h), raw bits
// out: out[i][6] = nan_min(a,b), nan_min3(a,b,c), fmax_q(a,b), min3f(a,b,c),
// med3_q(a,b,c), pt_canon(a) — the layout of devcheck's dc_minmax.
int hc_minmax(const float* a, const float* b, const float* c, int64_t n, uint32_t* out) {
    for (int64_t i = 0; i < n; ++i) {
        const float r[6] = {nan_min(a[i], b[i]), nan_min3(a[i], b[i], c[i]), fmax_q(a[i], b[i]),
                            min3f(a[i], b[i], c[i]), med3_q(a[i], b[i], c[i]), pt_canon(a[i])};
        memcpy(out + 6 * i, r, sizeof r);
    }
    return 0;
}

// BVH check.  Structure: every BVH unit in exactly one leaf, child boxes
// inside their parent's, every triangle vertex inside its leaf's box, skip
// links consistent with the depth-first layout.  Conservativeness: random
// lines (as in the filter self-test); for every BVH triangle the f64
// reference says the line meets at sqd, a traversal with the kernel's f32
// line and range sqrt(sqd) (1 + 1e-6) must reach that triangle's leaf.
// out: [0] structural errors, [1] missed hits, [2] hits checked, [3] nodes.
int hc_bvh_check(const pt_scene_desc* d, int64_t n_rays, uint64_t seed, int64_t* out) {
    HostScene H;
    if (!prepare_scene(d, &H).empty()) return -1;
    bind_host(&H);
    const SceneK& K = H.k;
    int64_t bad = 0, missed = 0, checked = 0;
    const int N = K.n_bnode;
    std::vector<int> seen(K.n_bunit, 0), leaf_of(K.n_bunit, -1);
    // structure: parent of node i+1 is i when i is internal; check via a stack walk
    std::vector<int> st;
    for (int i = 0; i < N; ++i) {
        const BNode& B = H.bnode[i];
        for (int a = 0; a < 3; ++a)
            if (!(B.lo[a] <= B.hi[a])) ++bad;
        if (B.leaf >= 0) {
            const int u0 = B.leaf >> 3, nu = B.leaf & 7;
            if (nu < 1 || u0 + nu > K.n_bunit) { ++bad; continue; }
            if (B.skip != (i + 1 < N ? i + 1 : -1)) ++bad;
            for (int q = u0; q < u0 + nu; ++q) {
                seen[q]++;
                leaf_of[q] = i;
                const UnitF& U = H.bunit[q];
                for (int m = 0; m < U.count; ++m) {
                    const TriD& T = H.trid[U.t[m]];
                    const double* vs[3] = {T.v1, T.v2, T.v3};
                    for (int v = 0; v < 3; ++v)
                        for (int a = 0; a < 3; ++a) {
                            const double x = vs[v][a] - K.center[a];
                            if (!(B.lo[a] <= x && x <= B.hi[a])) ++bad;
                        }
                }
            }
        } else {
            if (i + 1 >= N) { ++bad; continue; }
            const BNode& C = H.bnode[i + 1];   // first child
            for (int a = 0; a < 3; ++a)
                if (!(B.lo[a] <= C.lo[a] && C.hi[a] <= B.hi[a])) ++bad;
            if (!(B.skip == -1 || (B.skip > i + 1 && B.skip <= N))) ++bad;
        }
    }
    for (int q = 0; q < K.n_bunit; ++q)
        if (seen[q] != 1) ++bad;
    // conservativeness
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> U01(0.0, 1.0);
    std::vector<char> visited(N);
    for (int64_t r = 0; r < n_rays && K.n_bunit > 0; ++r) {
        // origin: a point on a random BVH triangle or at the eye; random direction
        D3 o;
        if (r % 4 == 0) {
            o = ld3(K.eye);
        } else {
            const UnitF& U = H.bunit[(size_t)(U01(rng) * K.n_bunit) % K.n_bunit];
            const TriD& T = H.trid[U.t[0]];
            double a = U01(rng), b = U01(rng);
            if (a + b > 1) { a = 1 - a; b = 1 - b; }
            o = ld3(T.v1) * (1 - a - b) + ld3(T.v2) * a + ld3(T.v3) * b;
        }
        D3 dir = d3(U01(rng) - 0.5, U01(rng) - 0.5, U01(rng) - 0.5);
        const D3 dn = unit(dir);
        const F3 o32 = to_f3(o - ld3(K.center)), inv = rcp_dir(to_f3(dn));
        for (int q = 0; q < K.n_bunit; ++q) {
            const UnitF& U = H.bunit[q];
            for (int m = 0; m < U.count; ++m) {
                D3 Q; double sqd;
                if (!eval64(H.trid[U.t[m]], o, dn, &Q, &sqd)) continue;
                const float R = (float)(sqrt(sqd) * (1 + 1e-6));
                ++checked;
                std::fill(visited.begin(), visited.end(), 0);
                int node = 0;
                while (node >= 0) {
                    const BNode& B = H.bnode[node];
                    const F3 l = {B.lo[0] - o32.x, B.lo[1] - o32.y, B.lo[2] - o32.z};
                    const F3 h = {B.hi[0] - o32.x, B.hi[1] - o32.y, B.hi[2] - o32.z};
                    const bool hit = box_hit(l, h, inv, R);
                    if (hit) visited[node] = 1;
                    node = (hit && B.leaf < 0) ? node + 1 : B.skip;
                }
                if (!visited[leaf_of[q]]) ++missed;
            }
        }
    }
    out[0] = bad; out[1] = missed; out[2] = checked; out[3] = N;
    return 0;
}

// 4-wide walk check (QNode, the wavefront walks' child test): random lines as
// in hc_bvh_check; for every BVH triangle the f64 line meets at sqd, a walk
// of the QNode tree that enters every child whose test (the kernels'
// q_child_dist / box_dist) passes within |t| <= sqrt(sqd)(1 + 1e-6) must
// reach that triangle's leaf; the sign-ordered child test the walks use
// (q_child_dist_s, on q_line_ex's slab parameters) must equal q_child_dist
// bit for bit on every child tested, and reject every absent child.
// out: [0] missed hits, [1] hits checked, [2] QNodes, [3] child tests whose
// two forms differ, [4] child tests compared.
int hc_qbvh_check(const pt_scene_desc* d, int64_t n_rays, uint64_t seed, int64_t* out) {
    HostScene H;
    if (!prepare_scene(d, &H).empty()) return -1;
    bind_host(&H);
    const SceneK& K = H.k;
    int64_t missed = 0, checked = 0, slab_diff = 0, slab_n = 0;
    if (K.n_qnode == 0) { out[0] = out[1] = out[2] = out[3] = out[4] = 0; return 0; }
    // leaf of every BVH unit: the leaf codes in the QNode refs
    std::vector<int> leaf_of(K.n_bunit, 0);
    for (int q = 0; q < K.n_qnode; ++q)
        for (int c = 0; c < 4; ++c) {
            const int r = H.qnode[q].ref[c];
            if (r <= -2) {
                const int code = ~r, u0 = code >> 3, nu = code & 7;
                for (int i = 0; i < nu; ++i) leaf_of[u0 + i] = r;
            }
        }
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> U01(0.0, 1.0);
    std::vector<int> reached;
    for (int64_t r = 0; r < n_rays; ++r) {
        D3 o;
        if (r % 4 == 0) {
            o = ld3(K.eye);
        } else {
            const UnitF& U = H.bunit[(size_t)(U01(rng) * K.n_bunit) % K.n_bunit];
            const TriD& T = H.trid[U.t[0]];
            double a = U01(rng), b = U01(rng);
            if (a + b > 1) { a = 1 - a; b = 1 - b; }
            o = ld3(T.v1) * (1 - a - b) + ld3(T.v2) * a + ld3(T.v3) * b;
        }
        const D3 dn = unit(d3(U01(rng) - 0.5, U01(rng) - 0.5, U01(rng) - 0.5));
        const F3 o32 = to_f3(o - ld3(K.center)), inv = rcp_dir(to_f3(dn));
        for (int q = 0; q < K.n_bunit; ++q) {
            const UnitF& U = H.bunit[q];
            for (int m = 0; m < U.count; ++m) {
                D3 Q; double sqd;
                if (!eval64(H.trid[U.t[m]], o, dn, &Q, &sqd)) continue;
                const float R = (float)(sqrt(sqd) * (1 + 1e-6));
                ++checked;
                reached.clear();
                std::vector<int> st{K.qroot};
                while (!st.empty()) {
                    const int n = st.back();
                    st.pop_back();
                    if (n <= -2) { reached.push_back(n); continue; }
                    const QNode& N = H.qnode[n];
                    const float step[3] = {q_step(N.ex, 0), q_step(N.ex, 1), q_step(N.ex, 2)};
#if PT_QLINE
                    const QLine L = q_line(N, step, o32, inv);
                    const QSlabs SL = q_slabs(N, L);
#endif
                    const QLine LX = q_line_ex(N, o32, inv);
                    if (memcmp(&LX, &L, sizeof L) != 0) ++slab_diff;   // the walks' ldexp form
                    for (int c = 0; c < 4; ++c) {
                        if (N.ref[c] == kNoRef) {   // an empty box: no line meets it
                            ++slab_n;
                            if (q_child_dist_s(SL, c, L, INFINITY) != INFINITY) ++slab_diff;
                            continue;
                        }
#if PT_QLINE
                        const float e = q_child_dist(N, c, L, R);
                        const float es = q_child_dist_s(SL, c, L, R);
                        ++slab_n;
                        if (memcmp(&e, &es, sizeof e) != 0) ++slab_diff;
#else
                        F3 l, h;
                        q_box(N, c, step, o32, &l, &h);
                        const float e = box_dist(l, h, inv, R);
#endif
                        if (e < INFINITY) st.push_back(N.ref[c]);
                    }
                }
                if (std::find(reached.begin(), reached.end(), leaf_of[q]) == reached.end()) ++missed;
            }
        }
    }
    out[0] = missed; out[1] = checked; out[2] = K.n_qnode; out[3] = slab_diff; out[4] = slab_n;
    return 0;
}

// The kernel's RNG (rng_blocks4): the 16 words of one (pixel, sample, bounce).
void hc_rng4(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t bounce, uint32_t* out) {
    rng_blocks4(seed, pixel, sample, bounce, out);
}

// Bounce-loop iterations of every lane of a single-kernel launch with `split`
// lanes per pixel (lane c of a pixel runs samples c, c + split, ...), the
// pixels of the selected rows in launch order: out[pixel * split + c] (dev
// tool: the lane-utilisation bound of a wave is sum / (64 max) over its 64).
int hc_lane_iters(const pt_scene_desc* d, const pt_render_params* p, int32_t split,
                  int32_t* out) {
    Host h;
    if (!h.open(d)) return -1;
    int32_t first, rows;
    if (!band_layout(p, &first, &rows)) return -2;
    for (int r = 0; r < rows; ++r) {
        const int iy = first + r * p->row_step;
        for (int ix = 0; ix < p->width; ++ix) {
            const CentreHit c0 = centre_hit<false>(h, p, ix, iy);
            for (int c = 0; c < split; ++c) {
                h.c = {};
                run_lane<false, true>(h, lane_of(p, pixel_key(p, ix, iy), c, split), c0.hit, c0.P0, SumSink{});
                out[((size_t)r * p->width + ix) * split + c] = (int32_t)h.c.shading_points;
            }
        }
    }
    return 0;
}

}  // extern "C"

// ---- the launch rules (pt_plan.h), for tests/test_plan_host.py ----
// scene[4]: bvh, walkable, n_cu, has_lens.  acc[6]: W, H, the band's fixed
// lanes per pixel, rays, aa, lens.  A check's message goes to msg[cap]; the
// functions return 0, or -1 with the message.
static PlanScene plan_scene_of(const int32_t* sc) { return PlanScene{sc[0] != 0, sc[1] != 0, sc[2], sc[3] != 0, 2.5}; }
static PlanAccum plan_accum_of(const int32_t* a) {
    return PlanAccum{a[0], a[1], (uint32_t)a[0] * (uint32_t)a[1], (uint32_t)a[2], a[3] != 0, a[4], a[5]};
}
static int plan_ret(const std::string& m, char* msg, int cap) {
    if (msg && cap > 0) snprintf(msg, (size_t)cap, "%s", m.c_str());
    return m.empty() ? 0 : -1;
}

extern "C" {

uint32_t hc_plan_lane_cap(int32_t spp) { return lane_cap(spp); }

// pt_render_device up to its first HIP call.  out[12]: split, split_log2,
// npix, tail_pix, tail_lane, tail_log2, work-items, wavefront, rr_depth,
// out_stride, first_row, n_rows.  Returns 1 for a band without rows.
int hc_plan_frame(const pt_render_params* p, const int32_t* scene, int64_t* out, char* msg, int cap) {
    std::string m = validate(p);
    const PlanScene sc = plan_scene_of(scene);
    if (m.empty()) m = check_scene(p->flags, sc);
    if (!m.empty()) return plan_ret(m, msg, cap);
    int32_t first = 0, rows = 0;
    band_layout(p, &first, &rows);
    if (rows == 0) return 1;
    RenderK R;
    LaunchPlan L{};
    m = plan_frame(p, sc, first, rows, &R, &L);
    if (!m.empty()) return plan_ret(m, msg, cap);
    const int64_t v[12] = {R.split, R.split_log2, R.npix, R.tail_pix, R.tail_lane, R.tail_log2, (int64_t)L.work_items,
                           L.wavefront, R.rr_depth, R.out_stride, R.first_row, R.n_rows};
    memcpy(out, v, sizeof(v));
    return plan_ret(m, msg, cap);
}

// pt_radiance_device likewise, n_rays > 0.  out[4]: split, split_log2, work-items, wavefront.
int hc_plan_rays(const pt_render_params* p, int64_t n_rays, int has_S, int has_Q, const int32_t* scene, int64_t* out,
                 char* msg, int cap) {
    std::string m = check_rays(p, true, n_rays, has_S != 0, has_Q != 0);
    RaysK R;
    LaunchPlan L{};
    if (m.empty()) m = plan_rays(p, n_rays, plan_scene_of(scene), &R, &L);
    if (m.empty()) {
        const int64_t v[4] = {R.split, R.split_log2, (int64_t)L.work_items, L.wavefront};
        memcpy(out, v, sizeof(v));
    }
    return plan_ret(m, msg, cap);
}

// An accumulator pass before the select (acc: may be null) ...
int hc_plan_check_pass(const pt_render_params* p, const pt_adapt_params* ap, const int32_t* acc, const int32_t* scene,
                       char* msg, int cap) {
    PlanAccum pa{};
    if (acc) pa = plan_accum_of(acc);
    const PlanScene sc = plan_scene_of(scene);
    AdaptK A;
    return plan_ret(check_pass(p, ap, acc ? &pa : nullptr, &sc, &A), msg, cap);
}
// ... and after it: count list entries of at least kmin samples.  out[5]:
// split, work-items, the single kernel's blocks, the wavefront's, wavefront.
int hc_plan_pass(const int32_t* acc, const int32_t* scene, uint32_t flags, uint32_t count, uint32_t kmin, int64_t* out,
                 char* msg, int cap) {
    uint32_t split = 0;
    LaunchPlan L{};
    const std::string m = plan_pass(plan_accum_of(acc), plan_scene_of(scene), flags, count, kmin, &split, &L);
    if (m.empty()) {
        const int64_t v[5] = {split, (int64_t)L.work_items, (int64_t)L.blocks, (int64_t)L.wf_blocks, L.wavefront};
        memcpy(out, v, sizeof(v));
    }
    return plan_ret(m, msg, cap);
}

}  // extern "C"
