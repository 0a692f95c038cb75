// pt_rays_wf_host.cpp — TEST INFRASTRUCTURE.  The ray form of the wavefront
// state machine (pt_wavefront.h wf_slot_step over a WfRays source,
// wf_rays_primary_step: the text k_wf_shade_rays and k_wf_primary_rays run;
// pt_shade_rays.hip k_wf_final_rays) run on the host, on pt_aa_wf_host.cpp's
// buffers and loop (wf_loop with a step-0 primary pass) — a ray run finds what
// an antialiased or a lens run left, and the other way round — so the CPU
// suite can check it against
// the single kernel's lane code (pt_rays_host.cpp hc_radiance) and the
// oracle's per-sample colours without a GPU.  Built by
// tests/test_rays_wavefront_host.py into a temporary directory by the
// hostcheck Makefile's pattern rule (tests/hostlib.py).
#include "pt_lens_wf_host.cpp"

extern "C" {

// pt_radiance through the wavefront kernels' text: the n records, `split` (a
// power of two <= 64) slots each.  sum: the records' colour sums of the form
// without moments (WfSum; k_wf_final_rays<false> before its division by spp);
// S, Q: the moments' (WfMoments), all [n][3] f64, a record's slots reduced in
// k_render_rays' xor order.  queried[n]: 1 for a record whose primary step
// issued a closest query (an origin inside the frame), 0 for one decided in
// f64.  steps[2]: the shade steps that found work in the two runs.  peak[2]
// (optional): peak_watch's figures over the records' primary walks.  fresh = 0:
// the buffers keep what the last run of any form left.  box (may be null):
// pt_scene_create_rays' box.  -3: a scene the wavefront kernels do not take
// (wf_walkable).
int hc_rays_wf(const pt_scene_desc* d, const double* box, const RayK* rays, int64_t n, const pt_render_params* p,
               uint32_t split, int fresh, double* sum, double* S, double* Q, int32_t* queried, int32_t* steps,
               int64_t* peak) {
    if (!split_ok(split)) return -4;
    HostScene H;
    if (!open_scene(d, &H, nullptr, box)) return -1;
    if (!wf_walkable(H.k)) return -3;
    pt_render_params q = *p;   // the launch record as pt_radiance_device fills it, f64 out
    q.lanes_per_pixel = (int32_t)split;
    q.flags |= PT_FLAG_OUT_F64;
    RaysK R;
    LaunchPlan L;
    (void)plan_rays(&q, n, PlanScene{true, true, 256, false, H.frame_x}, &R, &L);
    const WfRays src{R, rays};
    const size_t slots = ((((size_t)n << R.split_log2) + 255) / 256) * 256;
    const uint32_t slog = R.split_log2;
    int64_t pk[2] = {0, 0};
    // k_wf_primary_rays and the records' primary walks, their stacks watched
    // (home: the record's first slot)
    auto primary0 = [&](WfClosestQ* CQP) {
        ClosestStackLocal St;
        for (int64_t e = 0; e < n; ++e) {
            const bool asked = (wf_rays_primary_step(H.k, src, (uint32_t)e, g_wf.W.data(), CQP) & kWfWantClosest) != 0;
            if (queried) queried[e] = asked ? 1 : 0;
            if (asked)
                walk_closest(H.k, &CQP[e], Spill{g_wf.W[(size_t)e << slog].sp, 1}, St.view(), peak_watch(pk));
        }
    };
    for (int mom = 0; mom < 2; ++mom) {
        // (the slots past the batch are stepped too, as the kernels' grid does)
        const int32_t worked = wf_loop(H.k, slots, mom ? slots : 0, fresh, nullptr, 0, slot_step<false, false>(H.k, src),
                                       (size_t)n, primary0);
        if (steps) steps[mom] = worked;
        for (int64_t e = 0; e < n; ++e) {   // k_wf_final_rays
            const size_t t0 = (size_t)e << slog;
            const double* home = g_wf.home.data();
            if (mom) {
                st3(S + 3 * e, reduce_slots(t0, split, [&](size_t t) { return home_at(home, slots, t, 0); }));
                st3(Q + 3 * e, reduce_slots(t0, split, [&](size_t t) { return home_at(home, slots, t, 1); }));
            } else {
                st3(sum + 3 * e, reduce_slots(t0, split, acc_at));
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
