// pt_plan.h — what a launch looks like, decided on the host: the argument
// checks, the lanes per pixel, the launch records (pt_job.h), the work-items
// and the route (wavefront kernels or the single kernel) of pt_render_device,
// pt_radiance_device and the accumulator passes.  Pure arithmetic on
// pt_render_params, pt_adapt_params and a few facts about the scene and the
// accumulator, without the HIP runtime: pt_hip.hip and the host checks
// (tests/hostcheck, tests/test_plan_host.py) compile the same text.
// A check returns its message, empty for success; every message is a
// PT_EINVAL.  pt_hip.hip wraps it in fail().
#pragma once
#include <algorithm>
#include <string>

#include "../../include/pt_capi.h"
#include "pt_job.h"   // RenderK, ListK, RaysK, RaysListK, log2_ceil, kRenderBlock

// What the rules read of a scene handle: n_bnode > 0; the walk kernels can take
// it (n_qnode > 0 and the tree fits their stack); created with a lens;
// rays_in_frame's extent (HostScene::frame_x).
struct PlanScene {
    bool bvh, walkable;
    int n_cu;
    bool has_lens;
    double frame_x;
};
// ... and of an accumulator: the band's fixed lanes per pixel (0: choose_split),
// a ray accumulator, PT_FLAG_AA / PT_FLAG_LENS of the passes so far (-1: none yet).
struct PlanAccum {
    int32_t W, H;
    uint32_t npix, lanes_per_pixel;
    bool rays;
    int aa, lens;
};
// A planned launch: its work-items, the single kernel's blocks (kRenderBlock
// work-items each), the wavefront's (256 slots each) and the route.
struct LaunchPlan {
    uint64_t work_items, blocks, wf_blocks;
    bool wavefront;
};

constexpr uint32_t kKnownFlags = PT_FLAG_RR | PT_FLAG_FORCE_F64 | PT_FLAG_COUNT | PT_FLAG_OUT_F64 |
                                 PT_FLAG_MEGAKERNEL | PT_FLAG_WALK_COUNT | PT_FLAG_KERNEL_TIMES |
                                 PT_FLAG_AA | PT_FLAG_LENS;
static const char kLensNoCount[] = "PT_FLAG_LENS does not combine with PT_FLAG_COUNT, PT_FLAG_WALK_COUNT or "
                                   "PT_FLAG_KERNEL_TIMES: the lens kernels do not count";
static const char kLensNoScene[] = "PT_FLAG_LENS needs a scene created with a lens (pt_scene_create_lens)";
static const char kAaNoCount[] = "PT_FLAG_AA does not combine with PT_FLAG_COUNT, PT_FLAG_WALK_COUNT or "
                                 "PT_FLAG_KERNEL_TIMES: the antialiasing kernels do not count";
static const char kTooManyItems[] = "launch needs 2^32 or more work-items (32-bit lane index)";

// The most lanes a pixel of spp samples takes: the largest power of two <= min(64, spp).
inline uint32_t lane_cap(int32_t spp) {
    uint32_t cap = 64;
    while (cap > 1 && (int32_t)cap > spp) cap >>= 1;
    return cap;
}
// A caller's lanes per pixel: 0 (the rule chooses) or a power of two <= cap.
inline bool lanes_ok(int32_t l, uint32_t cap) { return l >= 0 && (l & (l - 1)) == 0 && l <= (int32_t)cap; }
inline std::string check_lanes(const pt_render_params* p) {
    if (p->lanes_per_pixel != 0 && !lanes_ok(p->lanes_per_pixel, lane_cap(p->spp)))
        return "lanes_per_pixel must be 0 or a power of two <= min(64, spp)";
    return {};
}
inline int32_t rr_depth_of(const pt_render_params* p) {   // -1: off
    return (p->flags & PT_FLAG_RR) ? std::max(0, p->rr_depth) : -1;
}

// An antialiased launch that takes the single kernel (pt_aa.hip) has nothing
// to fill pt_stats with; through the wavefront kernels the walk counts and the
// kernel times are a centre-ray launch's.
inline bool aa_stats_refused(uint32_t flags) {
    return (flags & PT_FLAG_AA) && (flags & (PT_FLAG_WALK_COUNT | PT_FLAG_KERNEL_TIMES));
}
// What the scene and the flags alone say about the path: false — the launch
// takes the single kernel whatever its size (wf_route's condition without the
// slot count).
inline bool wf_scene_ok(const PlanScene& s, uint32_t flags) {
    return s.bvh && !(flags & (PT_FLAG_COUNT | PT_FLAG_FORCE_F64 | PT_FLAG_MEGAKERNEL)) && s.walkable;
}
// (PT_FLAG_LENS does not decide it: the lens has its wavefront form,
// pt_shade_lens.hip.)
// This launch takes the wavefront kernels: BVH scenes, unless the caller asks
// for the single kernel, or for counting / forced f64, which only the single
// kernel implements (wf_scene_ok), or the launch has 2^29 or more path slots,
// beyond the shadow lists' (slot << 2) | ray entries.  The single kernel's
// result is the same bit for bit.
inline bool wf_route(const PlanScene& s, uint32_t flags, uint64_t slots) {
    return wf_scene_ok(s, flags) && slots < ((uint64_t)1 << 29);
}
// What a frame's flags ask of the scene (pt_render_device, a frame accumulator's pass).
inline std::string check_scene(uint32_t flags, const PlanScene& s) {
    if ((flags & PT_FLAG_LENS) && !s.has_lens) return kLensNoScene;
    if (aa_stats_refused(flags) && !wf_scene_ok(s, flags)) return kAaNoCount;
    return {};
}

inline std::string validate(const pt_render_params* p) {
    if (!p) return "null params";
    if (p->width <= 0 || p->height <= 0) return "width/height must be > 0";
    // pixel keys k = ix*H + iy and the launch's pixel counts are 32-bit
    if ((int64_t)p->width * p->height >= (int64_t)1 << 32) return "image too large for 32-bit pixel keys";
    if (p->spp <= 0) return "spp must be > 0";
    if (p->bounces < 0) return "bounces must be >= 0";
    if (p->sample_begin < 0) return "sample_begin must be >= 0";
    if (p->row_step <= 0 || p->row_phase < 0 || p->row_phase >= p->row_step)
        return "need row_step > 0 and 0 <= row_phase < row_step";
    if (p->flags & ~kKnownFlags) return "unknown flag bits (bit 7, v4's PT_FLAG_TREE_WALK, is retired)";
    // (with PT_FLAG_WALK_COUNT / PT_FLAG_KERNEL_TIMES: aa_stats_refused, once the launch's path is known)
    if ((p->flags & PT_FLAG_LENS) && (p->flags & (PT_FLAG_COUNT | PT_FLAG_WALK_COUNT | PT_FLAG_KERNEL_TIMES)))
        return kLensNoCount;
    if ((p->flags & PT_FLAG_AA) && (p->flags & PT_FLAG_COUNT)) return kAaNoCount;
    if (p->out_row_stride != 0 && (int64_t)p->out_row_stride < (int64_t)p->width * 3)
        return "out_row_stride must be 0 or >= width*3";
    return check_lanes(p);
}

// Lanes (wavefront: path slots) per pixel: a power of two <= min(64, spp).
//
// Single kernel (scenes without a BVH): >= 8 samples per lane where the
// launch is large (K2 512^2 x 64 spp: 8 lanes per pixel; K3 and K4: 64), at
// most 2^30 lanes over the full image — but at least `min_lanes` lanes in the
// launch, i.e. ~4 dispatch rounds of the device's resident waves (n_cu x 4
// SIMDs x 4 waves x 64 lanes x 4 rounds = 2^20 on MI355X).  A launch of one
// round is as long as its slowest wave (~0.7 ms at K2) however little work
// the band holds: one rank's band of an N-GPU strong-scaling split of the K2
// frame, per-band kernel ms at 8 / 16 / 32 / 64 lanes per
// pixel: N=4 1.592 / 1.450 / 1.480 / 1.566, N=8 0.882 / 0.816 / 0.767 / 0.809
// (N=1 5.584 / 5.674 / 5.792 / 6.136: each lane traces its pixel's primary
// ray once).  A pixel's samples are summed in an order that depends on its
// lane count, so bands of different sizes round differently in the last
// bits (all within 1e-12 of the oracle); bands of equal launch size agree bit
// for bit.
// Wavefront (BVH scenes): path slots hold ~420 B of state each, so at most
// 64M slots (28 GB) over the full image (K5 512^2 x 64 spp: 2M slots 161.6
// ms, 4M 147.1, 8M 140.5, 16M 139.3 (round 1); 1024^2 x 256 spp with the
// one-ray walks: 16M 1419 ms, 32M 1392, 64M 1378 — fewer shade / walk steps,
// each with its drain); an N-way band gets 1/N of them.  The single kernel
// uses the same split on BVH scenes (min_lanes does not apply), so its
// framebuffer stays bitwise equal to the wavefront one.
//
// PT_SPLIT_FIXED (compile-time, tuning builds only) pins the split.
// PT_MIN_SPL: samples per lane the whole-image split keeps at least (round 6:
// 4, i.e. 16 lanes per pixel at K2 — 4.669-4.693 vs 4.741-4.744 ms at 8 samples
// per lane; round 5's kernel was flat between 8 and 16 lanes)
#ifndef PT_MIN_SPL
#define PT_MIN_SPL 4
#endif
inline uint32_t choose_split(uint64_t image_pixels, uint64_t launch_pixels, int32_t spp, bool bvh,
                             uint64_t min_lanes) {
    const uint32_t cap = lane_cap(spp);
#ifdef PT_SPLIT_FIXED
    uint32_t f = 1;
    while (f * 2 <= (uint32_t)PT_SPLIT_FIXED && f * 2 <= cap) f *= 2;
    (void)image_pixels; (void)launch_pixels; (void)bvh; (void)min_lanes;
    return f;
#else
    uint32_t s = 1;
    const uint64_t target = (uint64_t)1 << (bvh ? 26 : 30);
    while (s < cap && image_pixels * s * 2 <= target && (bvh || spp / (int32_t)(s * 2) >= PT_MIN_SPL)) s *= 2;
    if (!bvh)
        while (s < cap && launch_pixels * s < min_lanes) s *= 2;
    return s;
#endif
}
// lanes of a single-kernel launch below which it gets more lanes per pixel:
// PT_MIN_ROUNDS dispatch rounds of the device's resident waves (4 per SIMD,
// k_render's __launch_bounds__)
#ifndef PT_MIN_ROUNDS
#define PT_MIN_ROUNDS 4
#endif
inline uint64_t min_lanes_of(int n_cu) {
    return (uint64_t)n_cu * 4u * (uint64_t)PT_RENDER_WAVES * 64u * (uint64_t)PT_MIN_ROUNDS;
}

// A planned launch of `items` < 2^32 work-items on scene s: the blocks of
// both paths and the route.
inline std::string plan_launch(uint64_t items, bool may_wavefront, const PlanScene& s, uint32_t flags,
                               LaunchPlan* L) {
    L->work_items = items;
    L->blocks = (items + kRenderBlock - 1) / kRenderBlock;
    L->wf_blocks = (items + 255) / 256;
    L->wavefront = may_wavefront && wf_route(s, flags, L->wf_blocks * 256u);
    if (!L->wavefront && aa_stats_refused(flags)) return kAaNoCount;
    return {};
}

// pt_render_device's launch of the band's rows first, first + row_step, ...
// (rows > 0 of them; band_layout) of a frame that passed validate and
// check_scene: the whole RenderK, the work-items and the route.
inline std::string plan_frame(const pt_render_params* p, const PlanScene& s, int32_t first, int32_t rows,
                              RenderK* out, LaunchPlan* L) {
    RenderK& R = *out;
    R.W = p->width; R.H = p->height; R.spp = p->spp; R.bounces = p->bounces;
    R.seed = p->seed;
    R.rr_depth = rr_depth_of(p);
    R.first_row = first; R.row_step = p->row_step; R.n_rows = rows;
    R.sample_begin = p->sample_begin;
    R.out_f64 = (p->flags & PT_FLAG_OUT_F64) ? 1 : 0;
    R.npix = (uint32_t)rows * (uint32_t)p->width;
    R.out_stride = p->out_row_stride ? (uint32_t)p->out_row_stride : (uint32_t)p->width * 3u;
    R.split = p->lanes_per_pixel > 0
                  ? (uint32_t)p->lanes_per_pixel
                  : choose_split((uint64_t)p->width * (uint64_t)p->height, (uint64_t)R.npix, p->spp, s.bvh,
                                 min_lanes_of(s.n_cu));
    R.split_log2 = log2_ceil(R.split);
    R.tail_pix = R.npix;
    R.tail_lane = R.npix * R.split;
    R.tail_log2 = R.split_log2;
    if (!s.bvh) {
        // The launch drains for about one wave lifetime (~1 ms at K2: 7% of
        // its wave-slots idle).  The image's top sixteenth of
        // rows (iy >= H - ceil(H/16), dispatched last, also in every
        // interleaved band) gets 8x the lanes per pixel, so the last dispatch
        // round is short waves.  K2 6.70 -> 6.49 ms; sixteenth / eighth /
        // quarter of the rows at 2x / 4x / 8x lanes all land within 6.49-6.54.
#ifndef PT_TAIL_FRAC
#define PT_TAIL_FRAC 16
#endif
#ifndef PT_TAIL_MUL
#define PT_TAIL_MUL 3
#endif
        constexpr int kTailFrac = PT_TAIL_FRAC;
        constexpr uint32_t kTailMul = PT_TAIL_MUL;   // log2 of the lane multiplier
        const uint32_t tl = std::min(R.split_log2 + kTailMul, (uint32_t)__builtin_ctz(lane_cap(p->spp)));
        const int32_t thresh = p->height - (p->height + kTailFrac - 1) / kTailFrac;
        int32_t ra = 0;   // band rows below the threshold (a prefix: rows ascend)
        while (ra < rows && first + ra * p->row_step < thresh) ++ra;
        // (no tail when this launch's lanes would overflow the 32-bit lane index)
        const uint64_t lanes = (uint64_t)ra * p->width * R.split + 64 +
                               (((uint64_t)(rows - ra) * (uint64_t)p->width) << tl);
        if (tl > R.split_log2 && ra < rows && lanes < ((uint64_t)1 << 32)) {
            R.tail_pix = (uint32_t)ra * (uint32_t)p->width;
            R.tail_lane = (R.tail_pix * R.split + 63u) & ~63u;
            R.tail_log2 = tl;
        }
    }
    const uint64_t threads = (uint64_t)R.tail_lane + ((uint64_t)(R.npix - R.tail_pix) << R.tail_log2);
    if ((uint64_t)R.npix * R.split >= ((uint64_t)1 << 32) || threads >= ((uint64_t)1 << 32)) return kTooManyItems;
    return plan_launch(threads, true, s, p->flags, L);
}

// pt_radiance_device's arguments, up to the batch's size
inline std::string check_rays(const pt_render_params* p, bool has_scene, int64_t n_rays, bool has_S, bool has_Q) {
    if (!p) return "null params";
    if (!has_scene) return "null scene";
    if (p->flags & ~(uint32_t)(PT_FLAG_RR | PT_FLAG_FORCE_F64 | PT_FLAG_OUT_F64 | PT_FLAG_RAYS_SINGLE))
        return "unsupported flag bits: pt_radiance takes PT_FLAG_RR, PT_FLAG_FORCE_F64, "
               "PT_FLAG_OUT_F64 and PT_FLAG_RAYS_SINGLE only (the ray kernels do not count, jitter "
               "or draw a lens point)";
    if (p->spp <= 0) return "spp must be > 0";
    if (p->bounces < 0) return "bounces must be >= 0";
    if (p->sample_begin < 0) return "sample_begin must be >= 0";
    std::string m = check_lanes(p);
    if (!m.empty()) return m;
    if (n_rays < 0 || n_rays >= ((int64_t)1 << 30)) return "need 0 <= n_rays < 2^30";
    if (has_S != has_Q) return "out_S and out_Q: both or neither";
    return {};
}
// Its launch of n_rays > 0 records: the whole RaysK, the work-items and the
// route.  The lanes per record are chosen before the route, so both paths
// deal a record's samples alike and agree bit for bit.
inline std::string plan_rays(const pt_render_params* p, int64_t n_rays, const PlanScene& s, RaysK* out,
                             LaunchPlan* L) {
    RaysK& R = *out;
    R.spp = p->spp; R.bounces = p->bounces;
    R.seed = p->seed;
    R.rr_depth = rr_depth_of(p);
    R.sample_begin = p->sample_begin;
    R.n_rays = (uint32_t)n_rays;
    R.out_f64 = (p->flags & PT_FLAG_OUT_F64) ? 1 : 0;
    R.frame_x = s.frame_x;
    // lanes per record: the rule of a launch of n_rays pixels
    R.split = p->lanes_per_pixel > 0 ? (uint32_t)p->lanes_per_pixel
                                     : choose_split((uint64_t)n_rays, (uint64_t)n_rays, p->spp, s.bvh,
                                                    min_lanes_of(s.n_cu));
    R.split_log2 = log2_ceil(R.split);
    const uint64_t threads = (uint64_t)n_rays << R.split_log2;
    if (threads >= ((uint64_t)1 << 32)) return kTooManyItems;
    return plan_launch(threads, !(p->flags & PT_FLAG_RAYS_SINGLE), s, p->flags, L);
}

// ------------------------------------------------- accumulator passes --
inline std::string check_adapt(const pt_adapt_params* a, AdaptK* A) {
    if (!a) return "null adapt params";
    if (a->min_spp < 2 || a->max_spp < a->min_spp) return "need 2 <= min_spp <= max_spp";
    if (a->step_spp < 1) return "step_spp must be >= 1";
    if (!(a->tol >= 0.0)) return "tol must be >= 0";
    if (!(a->floor > 0.0)) return "floor must be > 0";
    A->tol = a->tol; A->floor = a->floor;
    A->min_spp = (uint32_t)a->min_spp; A->max_spp = (uint32_t)a->max_spp;
    A->step_spp = (uint32_t)a->step_spp;
    return {};
}
// pt_accum_render(_stats), before the select: the arguments of a pass of a
// frame accumulator, or of a ray accumulator (acc->rays: one launch of the
// list kernel over ray records on every scene, pt_rays_list.hip).  acc, s:
// null for a null accumulator.
inline std::string check_pass(const pt_render_params* p, const pt_adapt_params* ap, const PlanAccum* acc,
                              const PlanScene* s, AdaptK* A) {
    const bool rays = acc && acc->rays;
    pt_render_params q;
    if (rays) {
        if (!p) return "null params";
        const uint32_t ok_flags = PT_FLAG_RR | PT_FLAG_FORCE_F64 | PT_FLAG_RAYS_SINGLE;
        if (p->flags & ~ok_flags) {
            static const struct { uint32_t bit; const char* name; } kNames[] = {
                {PT_FLAG_COUNT, "PT_FLAG_COUNT"}, {PT_FLAG_OUT_F64, "PT_FLAG_OUT_F64"},
                {PT_FLAG_MEGAKERNEL, "PT_FLAG_MEGAKERNEL"}, {PT_FLAG_WALK_COUNT, "PT_FLAG_WALK_COUNT"},
                {PT_FLAG_KERNEL_TIMES, "PT_FLAG_KERNEL_TIMES"}, {PT_FLAG_AA, "PT_FLAG_AA"}, {PT_FLAG_LENS, "PT_FLAG_LENS"}};
            std::string bad;
            uint32_t rest = p->flags & ~ok_flags;
            for (const auto& f : kNames)
                if (rest & f.bit) {
                    bad += std::string(bad.empty() ? "" : ", ") + f.name;
                    rest &= ~f.bit;
                }
            if (rest) bad += std::string(bad.empty() ? "" : ", ") + "unknown bits";
            return "unsupported flag bits (" + bad + "): a pass of a ray accumulator takes PT_FLAG_RR, "
                   "PT_FLAG_FORCE_F64 and PT_FLAG_RAYS_SINGLE only (the ray list kernel does not count, "
                   "jitter or draw a lens point, and is the single kernel already)";
        }
        q = *p;
        q.flags &= ~(uint32_t)PT_FLAG_RAYS_SINGLE;   // (accepted, no effect yet: reserved for the wavefront form)
    }
    std::string m = validate(rays ? &q : p);
    if (!m.empty()) return m;
    if (!acc) return "null accumulator";
    m = check_adapt(ap, A);
    if (!m.empty()) return m;
    if (p->width != acc->W || p->height != acc->H) return "width/height are not the accumulator's";
    if (p->row_begin != 0 || p->row_end != p->height || p->row_step != 1 || p->row_phase != 0 ||
        p->sample_begin != 0 || p->out_row_stride != 0 || p->lanes_per_pixel != 0)
        return "an accumulator pass renders the whole frame: row_begin 0, row_end height, "
               "row_step 1, sample_begin 0, out_row_stride 0, lanes_per_pixel 0";
    if (!rays && (p->flags & ~(uint32_t)(PT_FLAG_RR | PT_FLAG_FORCE_F64 | PT_FLAG_MEGAKERNEL | PT_FLAG_WALK_COUNT |
                                         PT_FLAG_KERNEL_TIMES | PT_FLAG_AA | PT_FLAG_LENS)))
        return "unsupported flag bits: an accumulator pass takes PT_FLAG_RR, PT_FLAG_FORCE_F64, "
               "PT_FLAG_MEGAKERNEL, PT_FLAG_WALK_COUNT, PT_FLAG_KERNEL_TIMES, PT_FLAG_AA and "
               "PT_FLAG_LENS only";
    if (p->spp != ap->max_spp) return "spp must be the budget max_spp";
    if (rays) return {};
    const bool aa = (p->flags & PT_FLAG_AA) != 0;
    if (acc->aa >= 0 && acc->aa != (aa ? 1 : 0))
        return "this accumulator's passes so far were made with the other value of PT_FLAG_AA: "
               "sample s would have two definitions (pt_accum_reset first)";
    const bool lens = (p->flags & PT_FLAG_LENS) != 0;
    if (acc->lens >= 0 && acc->lens != (lens ? 1 : 0))
        return "this accumulator's passes so far were made with the other value of PT_FLAG_LENS: "
               "sample s would have two definitions (pt_accum_reset first)";
    return check_scene(p->flags, *s);
}
// After the select: the pass over `count` > 0 list entries whose pixels take
// at least kmin >= 1 samples.  Lanes per entry: choose_split's rule for a
// launch of the list's pixels, or the band's fixed count capped at the
// pass's samples (pt_accum_band); then the work-items and the route.  A frame
// accumulator's pass on a BVH scene takes the wavefront kernels under
// pt_render_device's condition with the same split, so S, Q and n are the
// single kernel's bit for bit; a ray accumulator's is the single kernel.
inline std::string plan_pass(const PlanAccum& acc, const PlanScene& s, uint32_t flags, uint32_t count,
                             uint32_t kmin, uint32_t* split, LaunchPlan* L) {
    const int32_t k = (int32_t)std::min(kmin, 64u);
    *split = acc.lanes_per_pixel == 0
                 ? choose_split((uint64_t)acc.npix, (uint64_t)count, k, s.bvh, min_lanes_of(s.n_cu))
                 : std::min(acc.lanes_per_pixel, lane_cap(k));
    const uint64_t threads = (uint64_t)count << log2_ceil(*split);
    if ((threads + kRenderBlock - 1) / kRenderBlock * kRenderBlock >= ((uint64_t)1 << 32)) return kTooManyItems;
    return plan_launch(threads, !acc.rays, s, flags, L);
}
// The pass's launch records (L.lanes: the single kernel's work-items; the
// wavefront form takes its slots instead).
inline ListK list_record(const pt_render_params* p, const PlanAccum& acc, const AdaptK& A, uint32_t count,
                         uint32_t split, const LaunchPlan& L) {
    ListK R;
    R.W = acc.W; R.H = acc.H; R.bounces = p->bounces;
    R.rr_depth = rr_depth_of(p);
    R.seed = p->seed;
    R.split = split;
    R.split_log2 = log2_ceil(split);
    R.n_list = count;
    R.npix = acc.npix;
    R.lanes = (L.wavefront ? L.wf_blocks * 256u : L.blocks * kRenderBlock);
    R.A = A;
    return R;
}
inline RaysListK rays_list_record(const pt_render_params* p, const PlanAccum& acc, const PlanScene& s,
                                  const AdaptK& A, uint32_t count, uint32_t split) {
    RaysListK R;
    R.bounces = p->bounces;
    R.rr_depth = rr_depth_of(p);
    R.seed = p->seed;
    R.split = split;
    R.split_log2 = log2_ceil(split);
    R.n_list = count;
    R.n_rays = acc.npix;
    R.frame_x = s.frame_x;
    R.A = A;
    return R;
}
