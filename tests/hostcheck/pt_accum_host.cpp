// pt_accum_host.cpp — TEST INFRASTRUCTURE.  The adaptive sampler's lane code
// (pt_path.h MomentSink / render_lane_moments, moment_err, adapt_active,
// adapt_k) compiled for the host on top of pt_hostcheck.cpp, so the CPU suite
// can check the per-pixel moments against the oracle's per-sample colours and
// the stop rule against numpy without a GPU.  Built by tests/test_adaptive.py
// into a temporary directory with the hostcheck Makefile's g++ flags.
#include "pt_hostcheck.cpp"

extern "C" {

// The whole frame of p on the host, p->spp samples per pixel from sample
// p->sample_begin on (split = 1): S, Q [H*W][3] f64 and n [H*W] u32 in image
// orientation, e = (H-1-iy)*W + ix.  home: 0 the register home (MomentRegs),
// 1 the memory home (MomentMem, stride 1).
int hc_render_moments(const pt_scene_desc* d, const pt_render_params* p, int force64, int home,
                      double* S, double* Q, uint32_t* n) {
    HostScene H;
    if (!prepare_scene(d, &H).empty()) return -1;
    bind_host(&H);
    Counters c = {};
    double spill_mem[kSpillSlots];
    const Spill sp{spill_mem, 1};
    const D3 eye = ld3(H.k.eye);
    for (int iy = 0; iy < p->height; ++iy) {
        for (int ix = 0; ix < p->width; ++ix) {
            const double x = linspace_at(H.k.ortho[0], H.k.ortho[2], p->width, ix);
            const double y = linspace_at(H.k.ortho[1], H.k.ortho[3], p->height, iy);
            const D3 d0 = d3(x - eye.x, y - eye.y, 0.0 - eye.z);
            LaneJob J;
            J.seed = p->seed;
            J.pixel = (uint32_t)ix * (uint32_t)p->height + (uint32_t)iy;
            J.sample0 = p->sample_begin;
            J.sample_stride = 1;
            J.n_samples = p->spp;
            J.bounces = p->bounces;
            J.rr_depth = (p->flags & PT_FLAG_RR) ? p->rr_depth : -1;
            D3 P0 = d3(0, 0, 0);
            int tri0 = -1;
            double mem[6];
            MomentMem Mm{mem, 1};
            MomentRegs Mr;
            Mm.clear();
            Mr.clear();
            if (force64) {
                if (p->bounces > 0) tri0 = closest<true, false>(H.k, eye, d0, -1, sp, &P0, &c, true);
                if (home) render_lane_moments<true, false, true>(H.k, J, d0, tri0, P0, sp, &c, Mm);
                else render_lane_moments<true, false, true>(H.k, J, d0, tri0, P0, sp, &c, Mr);
            } else {
                if (p->bounces > 0) tri0 = closest<false, false>(H.k, eye, d0, -1, sp, &P0, &c, true);
                if (home) render_lane_moments<false, false, true>(H.k, J, d0, tri0, P0, sp, &c, Mm);
                else render_lane_moments<false, false, true>(H.k, J, d0, tri0, P0, sp, &c, Mr);
            }
            const D3 s = home ? Mm.sum() : Mr.sum(), q = home ? Mm.sumsq() : Mr.sumsq();
            const size_t e = (size_t)(p->height - 1 - iy) * p->width + ix;
            S[3 * e] = s.x; S[3 * e + 1] = s.y; S[3 * e + 2] = s.z;
            Q[3 * e] = q.x; Q[3 * e + 1] = q.y; Q[3 * e + 2] = q.z;
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
