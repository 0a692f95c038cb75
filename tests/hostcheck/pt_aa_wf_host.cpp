// pt_aa_wf_host.cpp — TEST INFRASTRUCTURE.  The antialiased wavefront state
// machine (pt_wavefront.h wf_aa_start / wf_shade_aa; pt_shade.h k_wf_shade_aa,
// k_wf_shade_list_aa) run on the host, in its uniform form (a whole frame,
// `split` slots per pixel) and its list form (one accumulator pass), with the
// walk primitives of hc_accum_wf_pass (pt_accum_wf_host.cpp), so the CPU suite
// can check it against the single kernel's lane code (pt_aa_host.cpp
// hc_render_aa) and the oracle's antialiased per-sample colours without a GPU.
// Built by tests/test_aa_wavefront_host.py into a temporary directory with the
// hostcheck Makefile's g++ flags.
#include "pt_accum_wf_host.cpp"

namespace {

// The buffers live on between calls, as the scene handle's on the device do:
// a run finds the state an earlier run left (fresh: a fill pattern instead).
struct AaWfBuffers {
    std::vector<WfPath> W;
    std::vector<WfShadowQ> SQ;
    std::vector<WfClosestQ> CQ;
    std::vector<double> home;
};
AaWfBuffers g_aa;

// The shade / walk loop over `slots` slots until a shade step finds no work.
// home_stride > 0: the list form (the slots' six sums in g_aa.home
// [6][home_stride]).  busy[s] (s < busy_cap): the slots that are not kWfDone
// after shade step s.  Returns the shade steps that found work.
int32_t aa_wf_loop(const SceneK& K, const std::vector<LaneJob>& J, const std::vector<AaPixel>& X,
                   const std::vector<char>& valid, size_t home_stride, int fresh, int32_t* busy,
                   int32_t busy_cap) {
    const size_t slots = J.size();
    if (g_aa.W.size() < slots) {
        g_aa.W.resize(slots);
        g_aa.SQ.resize(slots);
        g_aa.CQ.resize(slots);
    }
    if (g_aa.home.size() < 6 * home_stride) g_aa.home.resize(6 * home_stride, -1.0);
    if (fresh) {
        memset((void*)g_aa.W.data(), 0x55, g_aa.W.size() * sizeof(WfPath));
        memset((void*)g_aa.SQ.data(), 0x55, g_aa.SQ.size() * sizeof(WfShadowQ));
        memset((void*)g_aa.CQ.data(), 0x55, g_aa.CQ.size() * sizeof(WfClosestQ));
        std::fill(g_aa.home.begin(), g_aa.home.end(), -1.0);
    }
    WfPath* W = g_aa.W.data();
    WfShadowQ* SQ = g_aa.SQ.data();
    WfClosestQ* CQ = g_aa.CQ.data();
    std::vector<uint32_t> want(slots);
    int32_t worked = 0;
    for (int32_t step = 0;; ++step) {
        bool any = false;
        std::fill(want.begin(), want.end(), 0u);
        for (size_t t = 0; t < slots; ++t) {
            WfMoments M{{home_stride ? &g_aa.home[t] : nullptr, home_stride}};
            if (step == 0) {   // k_wf_shade_aa's step 0: the slot, then its first sample's query
                if (home_stride) M.clear();
                W[t].acc[0] = W[t].acc[1] = W[t].acc[2] = 0.0;
                W[t].put_rkey(J[t]);
                W[t].si = 0;
                W[t].set(kWfDone, false, 0);
                if (valid[t] && J[t].n_samples > 0 && J[t].bounces > 0)
                    want[t] = wf_aa_start(K, J[t], X[t], &W[t], &CQ[t]);
                any = true;
            } else if (W[t].state() != kWfDone) {
                want[t] = home_stride ? wf_shade_aa<false>(K, J[t], X[t], &W[t], &SQ[t], &CQ[t], M)
                                      : wf_shade_aa<false>(K, J[t], X[t], &W[t], &SQ[t], &CQ[t]);
                any = true;
            }
        }
        if (!any) break;
        ++worked;
        for (size_t t = 0; t < slots; ++t) {
            const Spill sp{W[t].sp, 1};
            for (int k = 0; k < kLightSamples; ++k)
                if ((want[t] >> k) & 1u) walk_shadow(K, &SQ[t], k, sp);
            if (want[t] & kWfWantClosest) walk_closest(K, &CQ[t], sp);
        }
        if (step < busy_cap) {
            int32_t b = 0;
            for (size_t t = 0; t < slots; ++t) b += W[t].state() != kWfDone;
            busy[step] = b;
        }
    }
    return worked;
}

int32_t rr_of(const pt_render_params* p) { return (p->flags & PT_FLAG_RR) ? std::max(0, p->rr_depth) : -1; }

}  // namespace

extern "C" {

// The whole frame of p (spp samples from sample_begin on), `split` slots per
// pixel by slot_job's mapping; sum [H*W][3] f64 in image orientation: the
// pixel's slots reduced in store_pixel's xor order, not divided by spp.
int hc_aa_wf_render(const pt_scene_desc* d, const pt_render_params* p, uint32_t split, int fresh,
                    double* sum, int32_t* steps_out, int32_t* busy, int32_t busy_cap) {
    if (split == 0 || split > 64 || (split & (split - 1)) != 0) return -4;
    HostScene H;
    if (!prepare_scene(d, &H).empty()) return -1;
    bind_host(&H);
    if (H.k.n_bnode == 0 || H.k.n_qnode == 0 || H.k.qstack > kBvhStack) return -3;
    uint32_t slog = 0;
    while ((1u << slog) < split) ++slog;
    const uint32_t npix = (uint32_t)p->width * (uint32_t)p->height;
    const size_t slots = (size_t)npix << slog;
    std::vector<LaneJob> J(slots);
    std::vector<AaPixel> X(slots);
    std::vector<char> valid(slots, 1);
    for (size_t t = 0; t < slots; ++t) {   // slot_job
        const uint32_t pl = (uint32_t)(t >> slog);
        const int32_t c = (int32_t)(t & (split - 1u)), sp = (int32_t)split;
        const int32_t iy = (int32_t)(pl / (uint32_t)p->width), ix = (int32_t)pl - iy * p->width;
        X[t] = AaPixel{p->width, p->height, ix, iy};
        J[t] = LaneJob{};
        J[t].seed = p->seed;
        J[t].pixel = (uint32_t)ix * (uint32_t)p->height + (uint32_t)iy;
        J[t].sample0 = p->sample_begin + c;
        J[t].sample_stride = sp;
        J[t].n_samples = c < p->spp ? (p->spp - c + sp - 1) / sp : 0;
        J[t].bounces = p->bounces;
        J[t].rr_depth = rr_of(p);
    }
    const int32_t worked = aa_wf_loop(H.k, J, X, valid, 0, fresh, busy, busy_cap);
    for (uint32_t pl = 0; pl < npix; ++pl) {   // k_wf_final
        D3 v[64];
        for (uint32_t c = 0; c < split; ++c) v[c] = ld3(g_aa.W[((size_t)pl << slog) + c].acc);
        for (uint32_t m = 1; m < split; m <<= 1) {
            D3 nv[64];
            for (uint32_t c = 0; c < split; ++c) nv[c] = v[c] + v[c ^ m];
            memcpy(v, nv, split * sizeof(D3));
        }
        const int32_t iy = (int32_t)(pl / (uint32_t)p->width), ix = (int32_t)pl - iy * p->width;
        const size_t e = (size_t)(p->height - 1 - iy) * p->width + ix;
        sum[3 * e] = v[0].x; sum[3 * e + 1] = v[0].y; sum[3 * e + 2] = v[0].z;
    }
    if (steps_out) *steps_out = worked;
    return 0;
}

// hc_accum_wf_pass with antialiased samples (k_wf_shade_list_aa, list_job's
// mapping, k_wf_final_list): one pass over list[0..n_list) under the rule,
// `split` slots per entry; S, Q, n read and updated in place.
int hc_aa_wf_pass(const pt_scene_desc* d, const pt_render_params* p, const uint32_t* list, uint32_t n_list,
                  uint32_t min_spp, uint32_t max_spp, uint32_t step_spp, uint32_t split, int fresh,
                  double* accS, double* accQ, uint32_t* accN, int32_t* steps_out, int32_t* busy,
                  int32_t busy_cap) {
    if (split == 0 || split > 64 || (split & (split - 1)) != 0) return -4;
    HostScene H;
    if (!prepare_scene(d, &H).empty()) return -1;
    bind_host(&H);
    if (H.k.n_bnode == 0 || H.k.n_qnode == 0 || H.k.qstack > kBvhStack) return -3;
    const AdaptK A{0.0, 1.0, min_spp, max_spp, step_spp};
    uint32_t slog = 0;
    while ((1u << slog) < split) ++slog;
    const uint32_t npix = (uint32_t)p->width * (uint32_t)p->height;
    const size_t slots = (size_t)n_list << slog;
    std::vector<LaneJob> J(slots);
    std::vector<AaPixel> X(slots, AaPixel{p->width, p->height, 0, 0});
    std::vector<char> valid(slots, 0);
    std::vector<uint32_t> kk(n_list, 0);
    for (size_t t = 0; t < slots; ++t) {   // list_job
        const uint32_t entry = (uint32_t)(t >> slog), c = (uint32_t)t & (split - 1u);
        const uint32_t e = list[entry];
        J[t] = LaneJob{};
        J[t].seed = p->seed;
        J[t].sample_stride = (int32_t)split;
        J[t].bounces = p->bounces;
        J[t].rr_depth = rr_of(p);
        if (e >= npix) continue;
        valid[t] = 1;
        const uint32_t n0 = accN[e], k = adapt_k(n0, A);
        kk[entry] = k;
        const int32_t row = (int32_t)(e / (uint32_t)p->width);
        const int32_t ix = (int32_t)e - row * p->width, iy = p->height - 1 - row;
        X[t].ix = ix;
        X[t].iy = iy;
        J[t].pixel = (uint32_t)ix * (uint32_t)p->height + (uint32_t)iy;
        J[t].sample0 = (int32_t)(n0 + c);
        J[t].n_samples = c < k ? (int32_t)((k - c + split - 1u) >> slog) : 0;
    }
    const int32_t worked = aa_wf_loop(H.k, J, X, valid, slots, fresh, busy, busy_cap);
    const std::vector<double>& home = g_aa.home;
    for (uint32_t en = 0; en < n_list; ++en) {   // k_wf_final_list
        const uint32_t e = list[en];
        if (e >= npix) continue;
        double v[6][64];
        for (uint32_t c = 0; c < split; ++c)
            for (int i = 0; i < 6; ++i) v[i][c] = home[(size_t)i * slots + ((size_t)en << slog) + c];
        for (uint32_t m = 1; m < split; m <<= 1)
            for (int i = 0; i < 6; ++i) {
                double nv[64];
                for (uint32_t c = 0; c < split; ++c) nv[c] = v[i][c] + v[i][c ^ m];
                memcpy(v[i], nv, split * sizeof(double));
            }
        if (kk[en] == 0) continue;
        for (int i = 0; i < 3; ++i) {
            accS[3 * (size_t)e + i] += v[i][0];
            accQ[3 * (size_t)e + i] += v[3 + i][0];
        }
        accN[e] += kk[en];
    }
    if (steps_out) *steps_out = worked;
    return 0;
}

}  // extern "C"
