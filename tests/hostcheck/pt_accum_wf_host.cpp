// pt_accum_wf_host.cpp — TEST INFRASTRUCTURE.  One accumulator pass through
// the list form of the wavefront state machine (pt_wavefront.h wf_start /
// wf_shade with the WfMoments home; pt_shade.h k_wf_shade_list, pt_hip.hip
// k_wf_primary_list / k_wf_final_list) run on the host on top of
// pt_hostcheck.cpp, with the walk primitives hc_render_wavefront3 uses, so
// the CPU suite can check the pass against the single-kernel lane code
// (hc_render_moments) and the oracle's per-sample colours without a GPU.
// Built by tests/test_adaptive_wavefront_host.py into a temporary directory
// with the hostcheck Makefile's g++ flags.
#include "pt_hostcheck.cpp"

namespace {

// k_wf_shadow's walk of shadow ray k of a query, to completion
void walk_shadow(const SceneK& K, WfShadowQ* q, int k, const Spill& sp) {
    Shadow1 r;
    F3 o32;
    int ogrp;
    wf_get_shadow1(*q, k, &o32, &ogrp, &r);
    ShadowTrav1 T;
    int buf[kBvhStackLocal];
    const ShadowStack St{buf, 1};
    s1_init(T, K, o32, ogrp, r, K.qroot);
    while (T.ref != kNoRef) {
        while (T.ref >= 0) s1_qnode(T, St, K, r);
        if (T.ref != kNoRef) {
            if (K.bunitc) s1_units<true, PT_WF_LRNG != 0>(T, K, &r, sp, T.ref);
            else s1_units<false, PT_WF_LRNG != 0>(T, K, &r, sp, T.ref);
            T.ref = s1_pop(T, St, K, r);
        }
    }
    wf_put_shadow1(q, r);
}

// k_wf_closest's walk of a query, to completion
void walk_closest(const SceneK& K, WfClosestQ* q, const Spill& sp) {
    ClosestAcc ca = wf_get_acc(*q);
    ClosestTrav T;
    ClosestStackLocal L;
    const ClosestStack St = L.view();
    ctrav_init(T, K, F3{q->o[0], q->o[1], q->o[2]}, q->ogrp, F3{q->d[0], q->d[1], q->d[2]}, ca.b1, K.qroot);
    while (T.ref != kNoRef) {
        while (T.ref >= 0) ctrav_qnode(T, St, K, &ca);
        if (T.ref != kNoRef) {
            if (K.bunitc) ctrav_leaf<false, true>(T, St, K, &ca, sp, nullptr);
            else ctrav_leaf<false>(T, St, K, &ca, sp, nullptr);
        }
    }
    q->a1 = ca.a1; q->a2 = ca.a2; q->b1 = ca.b1; q->i1 = ca.i1;
}

}  // namespace

extern "C" {

// One pass over list[0..n_list) of the frame of p (S, Q [H*W][3] f64 and
// n [H*W] u32 in image orientation, read and updated in place) under the rule
// (min_spp, max_spp, step_spp) with `split` (a power of two <= 64) slots per
// entry: slot -> (entry, sample slice) as list_job (pt_render.h), the primary
// ray once per entry with its spill home in the entry's first slot, the
// slots' six sums in a [6][slots] home, the entry's slots reduced in
// store_pixel's xor order.  Entries >= H*W are skipped.  steps_out
// (optional): shade steps that found work.
int hc_accum_wf_pass(const pt_scene_desc* d, const pt_render_params* p, const uint32_t* list,
                     uint32_t n_list, uint32_t min_spp, uint32_t max_spp, uint32_t step_spp,
                     uint32_t split, double* accS, double* accQ, uint32_t* accN, int32_t* steps_out) {
    if (split == 0 || split > 64 || (split & (split - 1)) != 0) return -4;
    HostScene H;
    if (!prepare_scene(d, &H).empty()) return -1;
    bind_host(&H);
    if (H.k.n_bnode == 0 || H.k.n_qnode == 0 || H.k.qstack > kBvhStack) return -3;
    const SceneK& K = H.k;
    const AdaptK A{0.0, 1.0, min_spp, max_spp, step_spp};
    uint32_t slog = 0;
    while ((1u << slog) < split) ++slog;
    const uint32_t npix = (uint32_t)p->width * (uint32_t)p->height;
    const size_t slots = (size_t)n_list << slog;
    std::vector<WfPath> W(slots);
    std::vector<WfShadowQ> SQ(slots);
    std::vector<WfClosestQ> CQ(slots), CQP(n_list);
    std::vector<LaneJob> J(slots);
    std::vector<D3> D0(slots);
    std::vector<double> home(6 * slots, -1.0);   // (stale: step 0 clears it)
    std::vector<uint32_t> kk(n_list, 0);
    memset((void*)W.data(), 0x55, slots * sizeof(WfPath));   // (stale state of an earlier pass)
    const D3 eye = ld3(K.eye);
    for (size_t t = 0; t < slots; ++t) {   // list_job
        const uint32_t entry = (uint32_t)(t >> slog), c = (uint32_t)t & (split - 1u);
        const uint32_t e = list[entry];
        J[t] = LaneJob{};
        J[t].seed = p->seed;
        J[t].sample_stride = (int32_t)split;
        J[t].bounces = p->bounces;
        J[t].rr_depth = (p->flags & PT_FLAG_RR) ? std::max(0, p->rr_depth) : -1;
        D0[t] = d3(0, 0, 0);
        if (e >= npix) continue;
        const uint32_t n0 = accN[e], k = adapt_k(n0, A);
        kk[entry] = k;
        const int32_t row = (int32_t)(e / (uint32_t)p->width);
        const int32_t ix = (int32_t)e - row * p->width, iy = p->height - 1 - row;
        const double x = linspace_at(K.ortho[0], K.ortho[2], p->width, ix);
        const double y = linspace_at(K.ortho[1], K.ortho[3], p->height, iy);
        D0[t] = d3(x - eye.x, y - eye.y, 0.0 - eye.z);
        J[t].pixel = (uint32_t)ix * (uint32_t)p->height + (uint32_t)iy;
        J[t].sample0 = (int32_t)(n0 + c);
        J[t].n_samples = c < k ? (int32_t)((k - c + split - 1u) >> slog) : 0;
    }
    std::vector<uint32_t> want(slots);
    int32_t busy = 0;
    for (int step = 0;; ++step) {
        bool any = false;
        std::fill(want.begin(), want.end(), 0u);
        if (step == 0) {
            for (size_t t = 0; t < slots; ++t) {   // k_wf_shade_list's step 0
                const bool valid = list[t >> slog] < npix;
                WfMoments M{{&home[t], slots}};
                M.clear();
                W[t].acc[0] = W[t].acc[1] = W[t].acc[2] = 0.0;
                W[t].put_rkey(J[t]);
                W[t].set(valid && J[t].n_samples > 0 && J[t].bounces > 0 ? kWfPrimary : kWfDone, false, 0);
            }
            for (uint32_t en = 0; en < n_list; ++en) {   // k_wf_primary_list, then the primary walks
                const size_t t = (size_t)en << slog;
                if (list[en] >= npix) continue;
                if (wf_start(K, J[t], D0[t], &W[t], &CQP[en]) & kWfWantClosest)
                    walk_closest(K, &CQP[en], Spill{W[t].sp, 1});
            }
        } else {
            for (size_t t = 0; t < slots; ++t) {
                if (W[t].state() == kWfDone) continue;
                WfMoments M{{&home[t], slots}};
                want[t] = wf_shade<false>(K, J[t], D0[t], &W[t], &SQ[t], &CQ[t], &CQP[t >> slog], M);
                any = true;
            }
            if (!any) break;
            for (size_t t = 0; t < slots; ++t) {
                const Spill sp{W[t].sp, 1};
                for (int k = 0; k < kLightSamples; ++k)
                    if ((want[t] >> k) & 1u) walk_shadow(K, &SQ[t], k, sp);
                if (want[t] & kWfWantClosest) walk_closest(K, &CQ[t], sp);
            }
        }
        ++busy;
    }
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
    if (steps_out) *steps_out = busy;
    return 0;
}

}  // extern "C"
