// pt_aa_wf_host.cpp — TEST INFRASTRUCTURE.  The antialiased wavefront state
// machine (pt_wavefront.h wf_slot_step<true>, the text k_wf_shade_aa and
// k_wf_shade_list_aa run) run on the host, in its uniform form (a whole frame,
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

// The shade / walk loop over the `slots` slots of src (a WfFrame or a
// WfActive: the antialiased shade kernels' step, pt_wavefront.h wf_slot_step)
// until a shade step finds no work.  home_stride > 0: the list form (the
// slots' six sums in g_aa.home [6][home_stride]).  busy[s] (s < busy_cap): the
// slots that are not kWfDone after shade step s.  Returns the shade steps that
// found work.
template <class Src>
int32_t aa_wf_loop(const SceneK& K, const Src& src, size_t slots, size_t home_stride, int fresh, int32_t* busy,
                   int32_t busy_cap) {
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
        bool any = step == 0 && slots > 0;
        for (size_t t = 0; t < slots; ++t) {
            any |= W[t].state() != kWfDone;
            const uint32_t w =
                home_stride ? wf_slot_step<true>(K, src, step, (uint32_t)t, W, SQ, CQ, nullptr,
                                                 WfMoments{{&g_aa.home[t], home_stride}})
                            : wf_slot_step<true>(K, src, step, (uint32_t)t, W, SQ, CQ, nullptr, WfSum{});
            want[t] = w & 0xffffu;
        }
        if (!any) break;
        ++worked;
        run_walks(K, want, W, SQ, CQ);
        if (step < busy_cap) {
            int32_t b = 0;
            for (size_t t = 0; t < slots; ++t) b += W[t].state() != kWfDone;
            busy[step] = b;
        }
    }
    return worked;
}

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
    const RenderK R = host_frame(p, 0, 1, p->height, split);
    const uint32_t npix = R.npix, slog = R.split_log2;
    const int32_t worked = aa_wf_loop(H.k, WfFrame{R}, (size_t)npix << slog, 0, fresh, busy, busy_cap);
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

// hc_accum_wf_pass with antialiased samples (k_wf_shade_list_aa's step over
// the active list, k_wf_final_list): one pass over list[0..n_list) under the
// rule, `split` slots per entry; S, Q, n read and updated in place.
int hc_aa_wf_pass(const pt_scene_desc* d, const pt_render_params* p, const uint32_t* list, uint32_t n_list,
                  uint32_t min_spp, uint32_t max_spp, uint32_t step_spp, uint32_t split, int fresh,
                  double* accS, double* accQ, uint32_t* accN, int32_t* steps_out, int32_t* busy,
                  int32_t busy_cap) {
    if (split == 0 || split > 64 || (split & (split - 1)) != 0) return -4;
    HostScene H;
    if (!prepare_scene(d, &H).empty()) return -1;
    bind_host(&H);
    if (H.k.n_bnode == 0 || H.k.n_qnode == 0 || H.k.qstack > kBvhStack) return -3;
    const ListK R = host_list(p, n_list, AdaptK{0.0, 1.0, min_spp, max_spp, step_spp}, split);
    const WfActive src{R, list, accN};
    const size_t slots = (size_t)R.lanes;
    const int32_t worked = aa_wf_loop(H.k, src, slots, slots, fresh, busy, busy_cap);
    final_list(H.k, src, g_aa.home.data(), accS, accQ, accN);
    if (steps_out) *steps_out = worked;
    return 0;
}

}  // extern "C"
