// pt_accum_host.cpp — TEST INFRASTRUCTURE.  The adaptive sampler's lane code
// (pt_path.h render_lane_cached over FrameHit and MomentSink, moment_err,
// adapt_active, adapt_k) compiled for the host on top of pt_hostcheck.cpp, so the CPU suite
// can check the per-pixel moments against the oracle's per-sample colours and
// the stop rule against numpy without a GPU.  Built by tests/test_adaptive.py
// into a temporary directory by the hostcheck Makefile's pattern rule (tests/hostlib.py).
#include "pt_hostcheck.cpp"

extern "C" {

// The whole frame of p on the host, p->spp samples per pixel from sample
// p->sample_begin on (split = 1): S, Q [H*W][3] f64 and n [H*W] u32 in image
// orientation, e = (H-1-iy)*W + ix.  home: 0 the register home (MomentRegs),
// 1 the memory home (MomentMem, stride 1).
int hc_render_moments(const pt_scene_desc* d, const pt_render_params* p, int force64, int home,
                      double* S, double* Q, uint32_t* n) {
    Host h;
    if (!h.open(d)) return -1;
    for (int iy = 0; iy < p->height; ++iy) {
        for (int ix = 0; ix < p->width; ++ix) {
            const size_t e = image_index(p, ix, iy);
            auto lane = [&](auto& M) {   // the pixel's one lane into the home M
                M.clear();
                with_bool(force64 != 0, [&](auto F64) {
                    const CentreHit c = centre_hit<decltype(F64)::value>(h, p, ix, iy);
                    run_lane<decltype(F64)::value, false>(h, lane_of(p, pixel_key(p, ix, iy), 0, 1), c.hit, c.P0,
                                                          MomentSink<std::decay_t<decltype(M)>>{M});
                });
                st3(S + 3 * e, M.sum());
                st3(Q + 3 * e, M.sumsq());
            };
            double mem[6];
            MomentMem Mm{mem, 1};
            MomentRegs Mr;
            if (home) lane(Mm);
            else lane(Mr);
            n[e] = (uint32_t)p->spp;
        }
    }
    return 0;
}

// The stop rule on npix pixels: err, the active flags and each pixel's k.
int hc_adapt_rule(const double* S, const double* Q, const uint32_t* n, int64_t npix, double tol,
                  double floor, uint32_t min_spp, uint32_t max_spp, uint32_t step_spp, double* err,
                  uint8_t* active, uint32_t* k) {
    const AdaptK A{tol, floor, min_spp, max_spp, step_spp};
    for (int64_t e = 0; e < npix; ++e) {
        err[e] = moment_err(S + 3 * e, Q + 3 * e, n[e], floor);
        active[e] = adapt_active(n[e], err[e], A) ? 1 : 0;
        k[e] = adapt_k(n[e], A);
    }
    return 0;
}

}  // extern "C"
