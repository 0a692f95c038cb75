// pt_lens_wf_host.cpp — TEST INFRASTRUCTURE.  The thin-lens wavefront state
// machine (pt_wavefront.h wf_slot_step<AA, true>, the text k_wf_shade_lens and
// k_wf_shade_list_lens run) run on the host, in its uniform form (a whole
// frame, `split` slots per pixel) and its list form (one accumulator pass),
// on pt_aa_wf_host.cpp's buffers and walk primitives — a lens run finds what
// an antialiased run left, and the other way round — so the CPU suite can
// check it against the single kernel's lane code (pt_lens_host.cpp
// hc_render_lens) and the oracle's per-sample colours through the lens without
// a GPU.  Built by tests/test_lens_wavefront_host.py into a temporary
// directory with the hostcheck Makefile's g++ flags.
#include "pt_aa_wf_host.cpp"

namespace {

// aa_wf_loop with the lens step; aa: PT_FLAG_AA beside the lens (a template
// parameter of the step, as in the kernels).
template <bool AA, class Src>
int32_t lens_wf_loop(const SceneK& K, const Src& src, size_t slots, size_t home_stride, int fresh, int32_t* busy,
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
                home_stride ? wf_slot_step<AA, true>(K, src, step, (uint32_t)t, W, SQ, CQ, nullptr,
                                                     WfMoments{{&g_aa.home[t], home_stride}})
                            : wf_slot_step<AA, true>(K, src, step, (uint32_t)t, W, SQ, CQ, nullptr, WfSum{});
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

// hc_aa_wf_render through the lens L: the whole frame of p (PT_FLAG_AA in
// p->flags: jittered as well), `split` slots per pixel; sum [H*W][3] f64 in
// image orientation, the pixel's slots reduced in store_pixel's xor order.
int hc_lens_wf_render(const pt_scene_desc* d, const pt_lens* L, const pt_render_params* p, uint32_t split,
                      int fresh, double* sum, int32_t* steps_out, int32_t* busy, int32_t busy_cap) {
    if (split == 0 || split > 64 || (split & (split - 1)) != 0) return -4;
    HostScene H;
    if (!L || !prepare_scene(d, &H, L).empty()) return -1;
    bind_host(&H);
    if (H.k.n_bnode == 0 || H.k.n_qnode == 0 || H.k.qstack > kBvhStack) return -3;
    const RenderK R = host_frame(p, 0, 1, p->height, split);
    const uint32_t npix = R.npix, slog = R.split_log2;
    const size_t slots = (size_t)npix << slog;
    const int32_t worked = (p->flags & PT_FLAG_AA)
                               ? lens_wf_loop<true>(H.k, WfFrame{R}, slots, 0, fresh, busy, busy_cap)
                               : lens_wf_loop<false>(H.k, WfFrame{R}, slots, 0, fresh, busy, busy_cap);
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

// hc_aa_wf_pass through the lens L (k_wf_shade_list_lens's step over the
// active list, k_wf_final_list): one pass over list[0..n_list) under the rule,
// `split` slots per entry; S, Q, n read and updated in place.
int hc_lens_wf_pass(const pt_scene_desc* d, const pt_lens* L, const pt_render_params* p, const uint32_t* list,
                    uint32_t n_list, uint32_t min_spp, uint32_t max_spp, uint32_t step_spp, uint32_t split,
                    int fresh, double* accS, double* accQ, uint32_t* accN, int32_t* steps_out, int32_t* busy,
                    int32_t busy_cap) {
    if (split == 0 || split > 64 || (split & (split - 1)) != 0) return -4;
    HostScene H;
    if (!L || !prepare_scene(d, &H, L).empty()) return -1;
    bind_host(&H);
    if (H.k.n_bnode == 0 || H.k.n_qnode == 0 || H.k.qstack > kBvhStack) return -3;
    const ListK R = host_list(p, n_list, AdaptK{0.0, 1.0, min_spp, max_spp, step_spp}, split);
    const WfActive src{R, list, accN};
    const size_t slots = (size_t)R.lanes;
    const int32_t worked = (p->flags & PT_FLAG_AA) ? lens_wf_loop<true>(H.k, src, slots, slots, fresh, busy, busy_cap)
                                                   : lens_wf_loop<false>(H.k, src, slots, slots, fresh, busy, busy_cap);
    final_list(H.k, src, g_aa.home.data(), accS, accQ, accN);
    if (steps_out) *steps_out = worked;
    return 0;
}

// the C ABI's additive record of this change (tests: its size is pinned)
int hc_launch_info_size() { return (int)sizeof(pt_launch_info); }
int hc_api_version() { return PT_API_VERSION; }

}  // extern "C"
