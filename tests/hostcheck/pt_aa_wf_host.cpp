// pt_aa_wf_host.cpp — TEST INFRASTRUCTURE.  The antialiased wavefront state
// machine (pt_wavefront.h wf_slot_step<true>, the text k_wf_shade_aa and
// k_wf_shade_list_aa run) run on the host, in its uniform form (a whole frame,
// `split` slots per pixel) and its list form (one accumulator pass), with the
// walks of hc_accum_wf_pass (pt_accum_wf_host.cpp), so the CPU suite can check
// it against the single kernel's lane code (pt_aa_host.cpp hc_render_aa) and
// the oracle's antialiased per-sample colours without a GPU.  The buffers, the
// loop and the finals here serve the lens and the ray form as well
// (pt_lens_wf_host.cpp, pt_rays_wf_host.cpp).  Built by the hostcheck
// Makefile's pattern rule (tests/hostlib.py).
#include "pt_accum_wf_host.cpp"

namespace {

// The buffers live on between calls, as the scene handle's on the device do:
// a run of any form finds the state an earlier run left (fresh: a fill
// pattern instead).  CQP: the ray form's primary queries, one per record.
struct WfBuffers {
    std::vector<WfPath> W;
    std::vector<WfShadowQ> SQ;
    std::vector<WfClosestQ> CQ, CQP;
    std::vector<double> home;
};
WfBuffers g_wf;

// The shade / walk loop over `slots` slots until a shade step finds no work.
// step(s, t, CQP, sink): the form's wf_slot_step instantiation for slot t at
// shade step s.  home_stride > 0: the list form (the slots' six sums in
// g_wf.home [6][home_stride]).  n_cqp > 0: CQP holds that many primary queries,
// which primary0(CQP) issues and walks after shade step 0 (the ray form).
// busy[s] (s < busy_cap): the slots that are not kWfDone after shade step s.
// Returns the shade steps that found work.
template <class Step, class Primary0>
int32_t wf_loop(const SceneK& K, size_t slots, size_t home_stride, int fresh, int32_t* busy, int32_t busy_cap,
                Step&& step, size_t n_cqp, Primary0&& primary0) {
    WfBuffers& B = g_wf;
    if (B.W.size() < slots) {
        B.W.resize(slots);
        B.SQ.resize(slots);
        B.CQ.resize(slots);
    }
    if (B.CQP.size() < n_cqp) B.CQP.resize(n_cqp);
    if (B.home.size() < 6 * home_stride) B.home.resize(6 * home_stride, -1.0);
    if (fresh) {
        memset((void*)B.W.data(), 0x55, B.W.size() * sizeof(WfPath));
        memset((void*)B.SQ.data(), 0x55, B.SQ.size() * sizeof(WfShadowQ));
        memset((void*)B.CQ.data(), 0x55, B.CQ.size() * sizeof(WfClosestQ));
        if (n_cqp) memset((void*)B.CQP.data(), 0x55, B.CQP.size() * sizeof(WfClosestQ));
        std::fill(B.home.begin(), B.home.end(), -1.0);
    }
    WfClosestQ* CQP = n_cqp ? B.CQP.data() : nullptr;
    std::vector<uint32_t> want(slots);
    int32_t worked = 0;
    for (int32_t s = 0;; ++s) {
        bool any = s == 0 && slots > 0;
        for (size_t t = 0; t < slots; ++t) {
            any |= B.W[t].state() != kWfDone;
            const uint32_t w = home_stride ? step(s, (uint32_t)t, CQP, WfMoments{{&B.home[t], home_stride}})
                                           : step(s, (uint32_t)t, CQP, WfSum{});
            want[t] = w & 0xffffu;
        }
        if (!any) break;
        ++worked;
        if (s == 0 && n_cqp) primary0(CQP);
        run_walks(K, want, B.W.data(), B.SQ.data(), B.CQ.data());
        if (s < busy_cap) {
            int32_t b = 0;
            for (size_t t = 0; t < slots; ++t) b += B.W[t].state() != kWfDone;
            busy[s] = b;
        }
    }
    return worked;
}
// ... without primary queries of its own (the frame and the list forms)
template <class Step>
int32_t wf_loop(const SceneK& K, size_t slots, size_t home_stride, int fresh, int32_t* busy, int32_t busy_cap,
                Step&& step) {
    return wf_loop(K, slots, home_stride, fresh, busy, busy_cap, step, 0, [](WfClosestQ*) {});
}
// The step of a form over src (a WfFrame, a WfActive, a WfRays): <true, false>
// the antialiased one, <AA, true> the lens's (AA: PT_FLAG_AA beside it, a
// template parameter as in the kernels), <false, false> the ray form's
template <bool AA, bool LENS, class Src>
auto slot_step(const SceneK& K, const Src& src) {
    return [&K, &src](int32_t s, uint32_t t, WfClosestQ* CQP, auto sink) {
        WfBuffers& B = g_wf;
        return wf_slot_step<AA, LENS>(K, src, s, t, B.W.data(), B.SQ.data(), B.CQ.data(), CQP, sink);
    };
}
// slot_step by the flags of a frame or a list launch, as f(step)
template <class Src, class F>
int32_t with_step(const SceneK& K, const Src& src, bool lens, bool aa, F&& f) {
    if (!lens) return f(slot_step<true, false>(K, src));
    return aa ? f(slot_step<true, true>(K, src)) : f(slot_step<false, true>(K, src));
}

// slot t's running sum (the form without moments)
D3 acc_at(size_t t) { return ld3(g_wf.W[t].acc); }
// k_wf_final: every pixel's slots' sums reduced into sum [H*W][3] in image orientation
void final_frame(const pt_render_params* p, const RenderK& R, double* sum) {
    for (uint32_t pl = 0; pl < R.npix; ++pl) {
        const int32_t iy = (int32_t)(pl / (uint32_t)p->width), ix = (int32_t)pl - iy * p->width;
        st3(sum + 3 * image_index(p, ix, iy),
            reduce_slots((size_t)pl << R.split_log2, R.split, acc_at));
    }
}

// The whole frame of p through the form the flags select (lens, aa), `split`
// slots per pixel by slot_job's mapping: hc_aa_wf_render and hc_lens_wf_render
int wf_render(const SceneK& K, const pt_render_params* p, bool lens, bool aa, uint32_t split, int fresh, double* sum,
              int32_t* steps_out, int32_t* busy, int32_t busy_cap) {
    if (!wf_walkable(K)) return -3;
    const RenderK R = host_frame(p, 0, 1, p->height, split);
    const WfFrame src{R};
    const size_t slots = (size_t)R.npix << R.split_log2;
    const int32_t worked =
        with_step(K, src, lens, aa, [&](auto step) { return wf_loop(K, slots, 0, fresh, busy, busy_cap, step); });
    final_frame(p, R, sum);
    if (steps_out) *steps_out = worked;
    return 0;
}
// One accumulator pass likewise (k_wf_final_list): list[0..n_list) under the
// rule, `split` slots per entry; S, Q, n read and updated in place
int wf_pass(const SceneK& K, const pt_render_params* p, bool lens, bool aa, const uint32_t* list, uint32_t n_list,
            const AdaptK& A, uint32_t split, int fresh, double* accS, double* accQ, uint32_t* accN, int32_t* steps_out,
            int32_t* busy, int32_t busy_cap) {
    if (!wf_walkable(K)) return -3;
    const ListK R = host_list(p, n_list, A, split);
    const WfActive src{R, list, accN};
    const size_t slots = (size_t)R.lanes;
    const int32_t worked =
        with_step(K, src, lens, aa, [&](auto step) { return wf_loop(K, slots, slots, fresh, busy, busy_cap, step); });
    final_list(K, src, g_wf.home.data(), accS, accQ, accN);
    if (steps_out) *steps_out = worked;
    return 0;
}

}  // namespace

extern "C" {

// The whole frame of p (spp samples from sample_begin on), `split` slots per
// pixel by slot_job's mapping; sum [H*W][3] f64 in image orientation: the
// pixel's slots reduced in store_pixel's xor order, not divided by spp.
int hc_aa_wf_render(const pt_scene_desc* d, const pt_render_params* p, uint32_t split, int fresh,
                    double* sum, int32_t* steps_out, int32_t* busy, int32_t busy_cap) {
    if (!split_ok(split)) return -4;
    HostScene H;
    if (!open_scene(d, &H)) return -1;
    return wf_render(H.k, p, false, true, split, fresh, sum, steps_out, busy, busy_cap);
}

// hc_accum_wf_pass with antialiased samples (k_wf_shade_list_aa's step over
// the active list, k_wf_final_list): one pass over list[0..n_list) under the
// rule, `split` slots per entry; S, Q, n read and updated in place.
int hc_aa_wf_pass(const pt_scene_desc* d, const pt_render_params* p, const uint32_t* list, uint32_t n_list,
                  uint32_t min_spp, uint32_t max_spp, uint32_t step_spp, uint32_t split, int fresh,
                  double* accS, double* accQ, uint32_t* accN, int32_t* steps_out, int32_t* busy,
                  int32_t busy_cap) {
    if (!split_ok(split)) return -4;
    HostScene H;
    if (!open_scene(d, &H)) return -1;
    return wf_pass(H.k, p, false, true, list, n_list, AdaptK{0.0, 1.0, min_spp, max_spp, step_spp}, split, fresh, accS,
                   accQ, accN, steps_out, busy, busy_cap);
}

}  // extern "C"
