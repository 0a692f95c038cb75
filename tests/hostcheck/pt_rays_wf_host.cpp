// pt_rays_wf_host.cpp — TEST INFRASTRUCTURE.  The ray form of the wavefront
// state machine (pt_wavefront.h wf_slot_step over a WfRays source,
// wf_rays_primary_step: the text k_wf_shade_rays and k_wf_primary_rays run;
// pt_shade_rays.hip k_wf_final_rays) run on the host, on pt_aa_wf_host.cpp's
// buffers and walk primitives — a ray run finds what an antialiased or a lens
// run left, and the other way round — so the CPU suite can check it against
// the single kernel's lane code (pt_rays_host.cpp hc_radiance) and the
// oracle's per-sample colours without a GPU.  Built by
// tests/test_rays_wavefront_host.py into a temporary directory with the
// hostcheck Makefile's g++ flags.
#include "pt_lens_wf_host.cpp"

namespace {

std::vector<WfClosestQ> g_rays_cqp;   // the records' primary queries (stale between calls, as g_aa)

// walk_closest for a record's primary query, its stack watched: pk[0] the
// largest T.top after a node visit, pk[1] the node visits that left T.top
// above the walk kernels' shared-memory part (16 entries)
void walk_primary(const SceneK& K, WfClosestQ* q, const Spill& sp, int64_t* pk) {
    ClosestAcc ca = wf_get_acc(*q);
    ClosestTrav T;
    ClosestStackLocal L;
    const ClosestStack St = L.view();
    ctrav_init(T, K, F3{q->o[0], q->o[1], q->o[2]}, q->ogrp, F3{q->d[0], q->d[1], q->d[2]}, ca.b1, K.qroot);
    while (T.ref != kNoRef) {
        while (T.ref >= 0) {
            ctrav_qnode(T, St, K, &ca);
            pk[0] = std::max<int64_t>(pk[0], T.top);
            if (T.top > 16) ++pk[1];
        }
        if (T.ref != kNoRef) {
            if (K.bunitc) ctrav_leaf<false, true>(T, St, K, &ca, sp, nullptr);
            else ctrav_leaf<false>(T, St, K, &ca, sp, nullptr);
        }
    }
    q->a1 = ca.a1; q->a2 = ca.a2; q->b1 = ca.b1; q->i1 = ca.i1;
}

// The shade / primary / walk loop over `slots` slots (a multiple of 256, as
// the kernels' grid: the slots past the batch are stepped too) until a shade
// step finds no work.  home_stride > 0: the moments' home.  queried[e]: 1 when
// record e's primary step issued a closest query, else 0; pk: walk_primary's.
// Returns the shade steps that found work.
int32_t rays_wf_loop(const SceneK& K, const WfRays& src, size_t slots, size_t home_stride, int fresh,
                     int32_t* queried, int64_t* pk) {
    const uint32_t n = src.R.n_rays, slog = src.R.split_log2;
    if (g_aa.W.size() < slots) {
        g_aa.W.resize(slots);
        g_aa.SQ.resize(slots);
        g_aa.CQ.resize(slots);
    }
    if (g_rays_cqp.size() < n) g_rays_cqp.resize(n);
    if (g_aa.home.size() < 6 * home_stride) g_aa.home.resize(6 * home_stride, -1.0);
    if (fresh) {
        memset((void*)g_aa.W.data(), 0x55, g_aa.W.size() * sizeof(WfPath));
        memset((void*)g_aa.SQ.data(), 0x55, g_aa.SQ.size() * sizeof(WfShadowQ));
        memset((void*)g_aa.CQ.data(), 0x55, g_aa.CQ.size() * sizeof(WfClosestQ));
        memset((void*)g_rays_cqp.data(), 0x55, g_rays_cqp.size() * sizeof(WfClosestQ));
        std::fill(g_aa.home.begin(), g_aa.home.end(), -1.0);
    }
    WfPath* W = g_aa.W.data();
    WfShadowQ* SQ = g_aa.SQ.data();
    WfClosestQ* CQ = g_aa.CQ.data();
    WfClosestQ* CQP = g_rays_cqp.data();
    std::vector<uint32_t> want(slots);
    int32_t worked = 0;
    for (int32_t step = 0;; ++step) {
        bool any = step == 0 && slots > 0;
        for (size_t t = 0; t < slots; ++t) {
            any |= W[t].state() != kWfDone;
            const uint32_t w =
                home_stride ? wf_slot_step<false>(K, src, step, (uint32_t)t, W, SQ, CQ, CQP,
                                                  WfMoments{{&g_aa.home[t], home_stride}})
                            : wf_slot_step<false>(K, src, step, (uint32_t)t, W, SQ, CQ, CQP, WfSum{});
            want[t] = w & 0xffffu;
        }
        if (!any) break;
        ++worked;
        if (step == 0) {   // k_wf_primary_rays and the primary walks (home: the record's first slot)
            for (uint32_t e = 0; e < n; ++e) {
                const bool q = (wf_rays_primary_step(K, src, e, W, CQP) & kWfWantClosest) != 0;
                if (queried) queried[e] = q ? 1 : 0;
                if (q) walk_primary(K, &CQP[e], Spill{W[(size_t)e << slog].sp, 1}, pk);
            }
        }
        run_walks(K, want, W, SQ, CQ);
    }
    return worked;
}

}  // namespace

extern "C" {

// pt_radiance through the wavefront kernels' text: the n records, `split` (a
// power of two <= 64) slots each.  sum: the records' colour sums of the form
// without moments (WfSum; k_wf_final_rays<false> before its division by spp);
// S, Q: the moments' (WfMoments), all [n][3] f64, a record's slots reduced in
// k_render_rays' xor order.  queried[n]: 1 for a record whose primary step
// issued a closest query (an origin inside the frame), 0 for one decided in
// f64.  steps[2]: the shade steps that found work in the two runs.  peak[2]
// (optional): walk_primary's figures over the records' primary walks.  fresh = 0:
// the buffers keep what the last run of any form left.  box (may be null):
// pt_scene_create_rays' box.  -3: a scene the wavefront kernels do not take
// (wf_scene_ok).
int hc_rays_wf(const pt_scene_desc* d, const double* box, const RayK* rays, int64_t n, const pt_render_params* p,
               uint32_t split, int fresh, double* sum, double* S, double* Q, int32_t* queried, int32_t* steps,
               int64_t* peak) {
    if (split == 0 || split > 64 || (split & (split - 1)) != 0) return -4;
    HostScene H;
    if (!prepare_scene(d, &H, nullptr, box).empty()) return -1;
    bind_host(&H);
    if (H.k.n_bnode == 0 || H.k.n_qnode == 0 || H.k.qstack > kBvhStack) return -3;
    pt_render_params q = *p;   // the launch record as pt_radiance_device fills it, f64 out
    q.lanes_per_pixel = (int32_t)split;
    q.flags |= PT_FLAG_OUT_F64;
    RaysK R;
    LaunchPlan L;
    (void)plan_rays(&q, n, PlanScene{true, true, 256, false, H.frame_x}, &R, &L);
    const WfRays src{R, rays};
    const size_t slots = ((((size_t)n << R.split_log2) + 255) / 256) * 256;
    int64_t pk[2] = {0, 0};
    for (int mom = 0; mom < 2; ++mom) {
        const int32_t worked = rays_wf_loop(H.k, src, slots, mom ? slots : 0, fresh, queried, pk);
        if (steps) steps[mom] = worked;
        for (int64_t e = 0; e < n; ++e) {   // k_wf_final_rays
            D3 s[64], q[64];
            for (uint32_t c = 0; c < split; ++c) {
                const size_t t = ((size_t)e << R.split_log2) + c;
                const double* h = mom ? &g_aa.home[t] : nullptr;
                s[c] = mom ? d3(h[0], h[slots], h[2 * slots]) : ld3(g_aa.W[t].acc);
                q[c] = mom ? d3(h[3 * slots], h[4 * slots], h[5 * slots]) : d3(0, 0, 0);
            }
            for (uint32_t m = 1; m < split; m <<= 1) {   // the kernel's xor order
                D3 ns[64], nq[64];
                for (uint32_t c = 0; c < split; ++c) { ns[c] = s[c] + s[c ^ m]; nq[c] = q[c] + q[c ^ m]; }
                memcpy(s, ns, split * sizeof(D3));
                memcpy(q, nq, split * sizeof(D3));
            }
            const D3 rs = s[0], rq = q[0];
            if (mom) {
                S[3 * e] = rs.x; S[3 * e + 1] = rs.y; S[3 * e + 2] = rs.z;
                Q[3 * e] = rq.x; Q[3 * e + 1] = rq.y; Q[3 * e + 2] = rq.z;
            } else {
                sum[3 * e] = rs.x; sum[3 * e + 1] = rs.y; sum[3 * e + 2] = rs.z;
            }
        }
    }
    if (peak) memcpy(peak, pk, sizeof(pk));
    return 0;
}

// the C ABI's additive record of this change (tests: the sizes are pinned)
int hc_ray_size() { return (int)sizeof(pt_ray); }
uint32_t hc_flag_rays_single() { return PT_FLAG_RAYS_SINGLE; }

}  // extern "C"
