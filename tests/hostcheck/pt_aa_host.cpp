// pt_aa_host.cpp — TEST INFRASTRUCTURE.  The antialiasing lane code (pt_path.h
// aa_jitter / aa_dir, AaRay with either sink through render_loop) compiled
// for the host on top of pt_hostcheck.cpp, so the CPU suite can check the rule
// of PT_FLAG_AA (include/pt_capi.h) against its numpy restatement and the
// oracle without a GPU.  Built by tests/test_aa_host.py into a temporary
// directory with the hostcheck Makefile's g++ flags.
#include "pt_hostcheck.cpp"

#include <vector>

extern "C" {

void hc_aa_jitter(uint64_t seed, uint32_t pixel, uint32_t sample, double* out) {
    aa_jitter(seed, pixel, sample, &out[0], &out[1]);
}

// The shifted window (4 doubles) and d0 (3 doubles) of offsets (jx, jy).
int hc_aa_dir(const pt_scene_desc* d, int32_t W, int32_t H, int32_t ix, int32_t iy, double jx,
              double jy, double* ortho, double* d0) {
    HostScene Hs;
    if (!prepare_scene(d, &Hs).empty()) return -1;
    bind_host(&Hs);
    aa_window(Hs.k, W, H, jx, jy, ortho);
    const D3 v = aa_dir(Hs.k, W, H, ix, iy, jx, jy);
    d0[0] = v.x; d0[1] = v.y; d0[2] = v.z;
    return 0;
}

namespace {
const AaEye kNoEye{nullptr, 0};   // (the device's per-wave table of the eye's origin terms: none here)
LaneJob lane_job(const pt_render_params* p, int ix, int iy, int32_t sample0, int32_t stride,
                 int32_t n_samples) {
    LaneJob J;
    J.seed = p->seed;
    J.pixel = (uint32_t)ix * (uint32_t)p->height + (uint32_t)iy;
    J.sample0 = sample0;
    J.sample_stride = stride;
    J.n_samples = n_samples;
    J.bounces = p->bounces;
    J.rr_depth = (p->flags & PT_FLAG_RR) ? p->rr_depth : -1;
    return J;
}
// the xor butterfly of store_pixel over `lanes` values; lane 0's result
D3 xor_reduce(std::vector<D3> v) {
    const size_t n = v.size();
    for (size_t m = 1; m < n; m <<= 1) {
        std::vector<D3> w(n);
        for (size_t i = 0; i < n; ++i) w[i] = v[i] + v[i ^ m];
        v = w;
    }
    return v[0];
}
}  // namespace

// The whole frame of p with PT_FLAG_AA's lane code, `lanes` (a power of two)
// emulated lanes per pixel: lane c takes samples sample_begin + c, + lanes,
// ... and the lanes reduce in store_pixel's xor order.  sum: the colour sums
// of the uniform form (SumSink); S, Q: the moments of the list form
// (MomentSink), all [H*W][3] f64 in image orientation.
int hc_render_aa(const pt_scene_desc* d, const pt_render_params* p, int force64, int32_t lanes,
                 double* sum, double* S, double* Q) {
    HostScene H;
    if (!prepare_scene(d, &H).empty()) return -1;
    bind_host(&H);
    if (lanes < 1 || (lanes & (lanes - 1))) return -2;
    Counters c = {};
    double spill_mem[kSpillSlots];
    const Spill sp{spill_mem, 1};
    for (int iy = 0; iy < p->height; ++iy) {
        for (int ix = 0; ix < p->width; ++ix) {
            std::vector<D3> a(lanes), s(lanes), q(lanes);
            for (int l = 0; l < lanes; ++l) {
                const int32_t ns = l < p->spp ? (p->spp - l + lanes - 1) / lanes : 0;
                const LaneJob J = lane_job(p, ix, iy, p->sample_begin + l, lanes, ns);
                const AaPixel X{p->width, p->height, ix, iy};
                MomentRegs M;
                M.clear();
                if (force64) {
                    a[l] = render_lane_aa<true, true>(H.k, J, X, kNoEye, sp, &c);
                    render_lane_moments_aa<true, true>(H.k, J, X, kNoEye, sp, &c, M);
                } else {
                    a[l] = render_lane_aa<false, true>(H.k, J, X, kNoEye, sp, &c);
                    render_lane_moments_aa<false, true>(H.k, J, X, kNoEye, sp, &c, M);
                }
                s[l] = M.sum();
                q[l] = M.sumsq();
            }
            const D3 ra = xor_reduce(a), rs = xor_reduce(s), rq = xor_reduce(q);
            const size_t e = (size_t)(p->height - 1 - iy) * p->width + ix;
            sum[3 * e] = ra.x; sum[3 * e + 1] = ra.y; sum[3 * e + 2] = ra.z;
            S[3 * e] = rs.x; S[3 * e + 1] = rs.y; S[3 * e + 2] = rs.z;
            Q[3 * e] = rq.x; Q[3 * e + 1] = rq.y; Q[3 * e + 2] = rq.z;
        }
    }
    return 0;
}

// An adaptive run on the host with antialiased samples: the accumulator's
// pass loop (select by moment_err / adapt_active, adapt_k more samples from
// sample n[e] on for each listed pixel, one lane per pixel) until no pixel is
// active.  S, Q [H*W][3], n [H*W] in image orientation; returns the passes
// made, or < 0.
int hc_accum_aa(const pt_scene_desc* d, const pt_render_params* p, double tol, double floor,
                uint32_t min_spp, uint32_t max_spp, uint32_t step_spp, double* S, double* Q,
                uint32_t* n) {
    HostScene H;
    if (!prepare_scene(d, &H).empty()) return -1;
    bind_host(&H);
    const AdaptK A{tol, floor, min_spp, max_spp, step_spp};
    Counters c = {};
    double spill_mem[kSpillSlots];
    const Spill sp{spill_mem, 1};
    const size_t np = (size_t)p->width * p->height;
    for (size_t i = 0; i < 3 * np; ++i) S[i] = Q[i] = 0.0;
    for (size_t i = 0; i < np; ++i) n[i] = 0;
    for (int pass = 0; pass <= (int)max_spp + 1; ++pass) {
        bool any = false;
        for (size_t e = 0; e < np; ++e) {
            const double err = moment_err(S + 3 * e, Q + 3 * e, n[e], floor);
            if (!adapt_active(n[e], err, A)) continue;
            const uint32_t k = adapt_k(n[e], A);
            if (k == 0) continue;
            any = true;
            const int row = (int)(e / p->width), ix = (int)(e % p->width), iy = p->height - 1 - row;
            const LaneJob J = lane_job(p, ix, iy, (int32_t)n[e], 1, (int32_t)k);
            MomentRegs M;
            M.clear();
            render_lane_moments_aa<false, true>(H.k, J, AaPixel{p->width, p->height, ix, iy}, kNoEye, sp, &c, M);
            const D3 s = M.sum(), q = M.sumsq();
            S[3 * e] += s.x; S[3 * e + 1] += s.y; S[3 * e + 2] += s.z;
            Q[3 * e] += q.x; Q[3 * e + 1] += q.y; Q[3 * e + 2] += q.z;
            n[e] += k;
        }
        if (!any) return pass;
    }
    return -3;
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
struct AaTraceSched : AaSched<FORCE64, BVH> {
    std::vector<int>* trace;   // queries at iteration i (index 0: before the loop)
    template <bool COUNT>
    bool advance(const SceneK& S, bool done, const Spill& sp, int* tri, D3* acc, Counters* cnt) {
        const int before = this->si;
        const bool r = AaSched<FORCE64, BVH>::template advance<COUNT>(S, done, sp, tri, acc, cnt);
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
    HostScene H;
    if (!prepare_scene(d, &H).empty()) return -1;
    bind_host(&H);
    if (lanes < 1 || lanes > 64 || (lanes & (lanes - 1))) return -2;
    Counters c = {};
    double spill_mem[kSpillSlots];
    const Spill sp{spill_mem, 1};
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
                const int32_t ns = l < p->spp ? (p->spp - l + lanes - 1) / lanes : 0;
                const LaneJob J = lane_job(p, ix, iy, p->sample_begin + l, lanes, ns);
                std::vector<int> t;
                AaTraceSched<false, true> q{{J, AaPixel{p->width, p->height, ix, iy}, kNoEye, 0}, &t};
                int tri = -1;
                D3 acc = d3(0, 0, 0);
                bool go = false;
                if (ns > 0 && p->bounces > 0) {
                    go = q.start(H.k, sp, &tri, &acc, &c);
                    t.push_back((go ? q.si : ns - 1) + 1);
                } else {
                    t.push_back(0);
                }
                if (go) render_loop<false, false, true>(H.k, J, tri, sp, &c, q, &acc);
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
