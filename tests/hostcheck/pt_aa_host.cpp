// pt_aa_host.cpp — TEST INFRASTRUCTURE.  The antialiasing lane code (pt_path.h
// aa_jitter / aa_dir, AaRay with either sink through render_loop) compiled
// for the host on top of pt_hostcheck.cpp, so the CPU suite can check the rule
// of PT_FLAG_AA (include/pt_capi.h) against its numpy restatement and the
// oracle without a GPU.  Built by tests/test_aa_host.py into a temporary
// directory by the hostcheck Makefile's pattern rule (tests/hostlib.py).
#include "pt_hostcheck.cpp"

extern "C" {

void hc_aa_jitter(uint64_t seed, uint32_t pixel, uint32_t sample, double* out) {
    aa_jitter(seed, pixel, sample, &out[0], &out[1]);
}

// The shifted window (4 doubles) and d0 (3 doubles) of offsets (jx, jy).
int hc_aa_dir(const pt_scene_desc* d, int32_t W, int32_t H, int32_t ix, int32_t iy, double jx,
              double jy, double* ortho, double* d0) {
    HostScene Hs;
    if (!open_scene(d, &Hs)) return -1;
    aa_window(Hs.k, W, H, jx, jy, ortho);
    const D3 v = aa_dir(Hs.k, W, H, ix, iy, jx, jy);
    d0[0] = v.x; d0[1] = v.y; d0[2] = v.z;
    return 0;
}

}  // extern "C"
namespace {
// The whole frame of p, `lanes` (a power of two) emulated lanes per pixel with
// both sinks.  primary(ix, iy, f): calls f(F64, prim, P0) with the pixel's
// primary source, as with_primary does.
template <class Primary>
void render_frame(Host& h, const pt_render_params* p, int32_t lanes, double* sum, double* S, double* Q,
                  Primary&& primary) {
    for (int iy = 0; iy < p->height; ++iy)
        for (int ix = 0; ix < p->width; ++ix)
            primary(ix, iy, [&](auto F64, const auto& prim, D3 P0) {
                store_lanes(p, pixel_key(p, ix, iy), lanes, image_index(p, ix, iy), sum, S, Q,
                            [&](const LaneJob& J) { return both_sinks<decltype(F64)::value>(h, J, prim, P0); });
            });
}
// An adaptive run on the host: the accumulator's pass loop (select by
// moment_err / adapt_active, adapt_k more samples from sample n[e] on for each
// listed pixel, one lane per pixel, its primary source as render_frame's) until
// no pixel is active.  S, Q [H*W][3], n [H*W] in image orientation; returns the
// passes made, or -3.
template <class Primary>
int accum_passes(Host& h, const pt_render_params* p, const AdaptK& A, double* S, double* Q, uint32_t* n,
                 Primary&& primary) {
    const size_t np = (size_t)p->width * p->height;
    for (size_t i = 0; i < 3 * np; ++i) S[i] = Q[i] = 0.0;
    for (size_t i = 0; i < np; ++i) n[i] = 0;
    for (int pass = 0; pass <= (int)A.max_spp + 1; ++pass) {
        bool any = false;
        for (size_t e = 0; e < np; ++e) {
            const double err = moment_err(S + 3 * e, Q + 3 * e, n[e], A.floor);
            if (!adapt_active(n[e], err, A)) continue;
            const uint32_t k = adapt_k(n[e], A);
            if (k == 0) continue;
            any = true;
            const int row = (int)(e / p->width), ix = (int)(e % p->width), iy = p->height - 1 - row;
            const LaneJob J = lane_job(p, pixel_key(p, ix, iy), (int32_t)n[e], 1, (int32_t)k);
            MomentRegs M;
            M.clear();
            primary(ix, iy, [&](auto F64, const auto& prim, D3 P0) {
                run_lane<decltype(F64)::value, false>(h, J, prim, P0, MomentSink<MomentRegs>{M});
            });
            add3(S + 3 * e, M.sum());
            add3(Q + 3 * e, M.sumsq());
            n[e] += k;
        }
        if (!any) return pass;
    }
    return -3;
}
// the jittered source of pixel (ix, iy) alone, as f(F64, prim, P0)
template <bool F64, class F>
void aa_primary(const pt_render_params* p, int ix, int iy, F&& f) {
    f(std::bool_constant<F64>{}, AaRay<F64, true>{AaPixel{p->width, p->height, ix, iy}, kNoEye}, d3(0, 0, 0));
}
}  // namespace
extern "C" {

// The whole frame of p with PT_FLAG_AA's lane code, `lanes` (a power of two)
// emulated lanes per pixel: lane c takes samples sample_begin + c, + lanes,
// ... and the lanes reduce in store_pixel's xor order.  sum: the colour sums
// of the uniform form (SumSink); S, Q: the moments of the list form
// (MomentSink), all [H*W][3] f64 in image orientation.
int hc_render_aa(const pt_scene_desc* d, const pt_render_params* p, int force64, int32_t lanes,
                 double* sum, double* S, double* Q) {
    Host h;
    if (!h.open(d)) return -1;
    if (lanes < 1 || (lanes & (lanes - 1))) return -2;
    render_frame(h, p, lanes, sum, S, Q, [&](int ix, int iy, auto&& f) {
        if (force64) aa_primary<true>(p, ix, iy, f);
        else aa_primary<false>(p, ix, iy, f);
    });
    return 0;
}

// accum_passes with antialiased samples
int hc_accum_aa(const pt_scene_desc* d, const pt_render_params* p, double tol, double floor,
                uint32_t min_spp, uint32_t max_spp, uint32_t step_spp, double* S, double* Q,
                uint32_t* n) {
    Host h;
    if (!h.open(d)) return -1;
    return accum_passes(h, p, AdaptK{tol, floor, min_spp, max_spp, step_spp}, S, Q, n,
                        [&](int ix, int iy, auto&& f) { aa_primary<false>(p, ix, iy, f); });
}

// Dev tool (scripts/aa_restart_stats.py): how often a wave of k_render_aa runs
// the restart's closest query.  The frame's lanes in launch order (`lanes` per
// pixel, 64 / lanes pixels per wave, no tail rows); a lane's trace is, per
// loop iteration, the primary rays its restart traces there.  A wave runs
// max-over-lanes queries in an iteration (the divergent loop's trip count) and
// as many iterations as its longest lane.  out: [0] waves, [1] loop
// iterations summed over waves, [2] restart queries summed over waves
// (the start before the loop included), [3] iterations with a restart,
// [4] samples per lane summed over waves (the lockstep floor of [2]),
// [5] lane-iterations (utilisation = [5] / (64 [1])).
}  // extern "C"
namespace {
template <bool FORCE64, bool BVH>
using AaSumSched = Sched<AaRay<FORCE64, BVH>, SumSink>;   // the sum form's scheduler of render_lane_sampled
template <bool FORCE64, bool BVH>
struct AaTraceSched : AaSumSched<FORCE64, BVH> {
    std::vector<int>* trace;   // queries at iteration i (index 0: before the loop)
    template <bool COUNT>
    bool advance(const SceneK& S, bool done, const Spill& sp, int* tri, D3* acc, Counters* cnt) {
        const int before = this->si;
        const bool r = AaSumSched<FORCE64, BVH>::template advance<COUNT>(S, done, sp, tri, acc, cnt);
        // start() traced samples before+1 .. si (the one that landed included)
        int q = 0;
        if (done) q = (r ? this->si : this->J.n_samples - 1) - before;
        trace->push_back(q);
        return r;
    }
};
}  // namespace
extern "C" {
int hc_aa_restart_stats(const pt_scene_desc* d, const pt_render_params* p, int32_t lanes, int64_t* out) {
    Host h;
    if (!h.open(d)) return -1;
    if (lanes < 1 || lanes > 64 || (lanes & (lanes - 1))) return -2;
    const SceneK& K = h.H.k;
    const Spill& sp = h.sp;
    Counters& c = h.c;
    for (int i = 0; i < 6; ++i) out[i] = 0;
    std::vector<std::vector<int>> wave;
    auto flush = [&]() {
        if (wave.empty()) return;
        size_t len = 0;
        for (auto& t : wave) len = std::max(len, t.size());
        out[0] += 1;
        out[1] += (int64_t)len - 1;
        for (size_t i = 0; i < len; ++i) {
            int q = 0;
            for (auto& t : wave) q = std::max(q, i < t.size() ? t[i] : 0);
            out[2] += q;
            if (i > 0 && q > 0) out[3] += 1;
        }
        for (auto& t : wave) out[5] += (int64_t)t.size() - 1;
        wave.clear();
    };
    // launch order: pixel pl = row_local * W + ix, rows from iy = 0
    for (int iy = 0; iy < p->height; ++iy) {
        for (int ix = 0; ix < p->width; ++ix) {
            for (int l = 0; l < lanes; ++l) {
                const LaneJob J = lane_of(p, pixel_key(p, ix, iy), l, lanes);
                const int32_t ns = J.n_samples;
                std::vector<int> t;
                AaTraceSched<false, true> q{{J, AaPixel{p->width, p->height, ix, iy}, kNoEye, 0}, &t};
                int tri = -1;
                D3 acc = d3(0, 0, 0);
                bool go = false;
                if (ns > 0 && p->bounces > 0) {
                    go = q.start(K, sp, &tri, &acc, &c);
                    t.push_back((go ? q.si : ns - 1) + 1);
                } else {
                    t.push_back(0);
                }
                if (go) render_loop<false, false, true>(K, J, tri, sp, &c, q, &acc);
                if (wave.empty()) out[4] += (p->spp + lanes - 1) / lanes;
                wave.push_back(t);
                if ((int)wave.size() == 64) flush();
            }
        }
    }
    flush();
    return 0;
}

}  // extern "C"
