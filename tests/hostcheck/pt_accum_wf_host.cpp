// pt_accum_wf_host.cpp — TEST INFRASTRUCTURE.  One accumulator pass through
// the list form of the wavefront state machine (pt_wavefront.h wf_slot_step /
// wf_primary_step over a WfActive with the WfMoments home: the text
// k_wf_shade_list and k_wf_primary_list run; pt_hip.hip k_wf_final_list) run
// on the host on top of pt_hostcheck.cpp, with the walk primitives
// hc_render_wavefront3 uses, so the CPU suite can check the pass against the
// single-kernel lane code (hc_render_moments) and the oracle's per-sample
// colours without a GPU.
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

// Every walk the slots' shade steps asked for (want[t]), to completion
void run_walks(const SceneK& K, const std::vector<uint32_t>& want, WfPath* W, WfShadowQ* SQ, WfClosestQ* CQ) {
    for (size_t t = 0; t < want.size(); ++t) {
        const Spill sp{W[t].sp, 1};
        for (int k = 0; k < kLightSamples; ++k)
            if ((want[t] >> k) & 1u) walk_shadow(K, &SQ[t], k, sp);
        if (want[t] & kWfWantClosest) walk_closest(K, &CQ[t], sp);
    }
}

// The launch record of a pass over n_list entries of p's frame under the rule
// A with `split` slots per entry, as pt_accum_render fills it (list_record);
// lanes: the host loop's slots, with no blocks to round up to.
ListK host_list(const pt_render_params* p, uint32_t n_list, const AdaptK& A, uint32_t split) {
    const PlanAccum acc{p->width, p->height, (uint32_t)p->width * (uint32_t)p->height, split, false, -1, -1};
    ListK R = list_record(p, acc, A, n_list, split, LaunchPlan{});
    R.lanes = (uint64_t)n_list << R.split_log2;
    return R;
}

// k_wf_final_list: an entry's slots' six sums (home[6][slots]) reduced in
// store_pixel's xor order and added to the accumulator with the entry's k
void final_list(const SceneK& K, const WfActive& src, const double* home, double* accS, double* accQ,
                uint32_t* accN) {
    const ListK& R = src.R;
    const size_t slots = (size_t)R.lanes;
    for (uint32_t en = 0; en < R.n_list; ++en) {
        const ListJob j = src.job(K, en << R.split_log2);
        if (!j.valid) continue;
        double v[6][64];
        for (uint32_t c = 0; c < R.split; ++c)
            for (int i = 0; i < 6; ++i) v[i][c] = home[(size_t)i * slots + ((size_t)en << R.split_log2) + c];
        for (uint32_t m = 1; m < R.split; m <<= 1)
            for (int i = 0; i < 6; ++i) {
                double nv[64];
                for (uint32_t c = 0; c < R.split; ++c) nv[c] = v[i][c] + v[i][c ^ m];
                memcpy(v[i], nv, R.split * sizeof(double));
            }
        if (j.k == 0) continue;
        for (int i = 0; i < 3; ++i) {
            accS[3 * (size_t)j.e + i] += v[i][0];
            accQ[3 * (size_t)j.e + i] += v[3 + i][0];
        }
        accN[j.e] += j.k;
    }
}

}  // namespace

extern "C" {

// One pass over list[0..n_list) of the frame of p (S, Q [H*W][3] f64 and
// n [H*W] u32 in image orientation, read and updated in place) under the rule
// (min_spp, max_spp, step_spp) with `split` (a power of two <= 64) slots per
// entry: the shade and primary kernels' steps (pt_wavefront.h wf_slot_step,
// wf_primary_step over a WfActive: list_job's mapping, the primary ray once
// per entry with its spill home in the entry's first slot), the slots' six
// sums in a [6][slots] home.  Entries >= H*W are skipped.  steps_out
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
    const ListK R = host_list(p, n_list, AdaptK{0.0, 1.0, min_spp, max_spp, step_spp}, split);
    const WfActive src{R, list, accN};
    const size_t slots = (size_t)R.lanes;
    std::vector<WfPath> W(slots);
    std::vector<WfShadowQ> SQ(slots);
    std::vector<WfClosestQ> CQ(slots), CQP(n_list);
    std::vector<double> home(6 * slots, -1.0);   // (stale: step 0 clears it)
    memset((void*)W.data(), 0x55, slots * sizeof(WfPath));   // (stale state of an earlier pass)
    std::vector<uint32_t> want(slots), wantp(n_list);
    int32_t busy = 0;
    for (int step = 0;; ++step) {
        bool any = step == 0;
        for (size_t t = 0; t < slots; ++t) {
            any |= W[t].state() != kWfDone;
            want[t] = wf_slot_step<false>(K, src, step, (uint32_t)t, W.data(), SQ.data(), CQ.data(), CQP.data(),
                                          WfMoments{{&home[t], slots}}) & 0xffffu;
        }
        if (!any) break;
        ++busy;
        if (step == 0) {   // the primary queries and their walks (home: the entry's first slot)
            for (uint32_t en = 0; en < n_list; ++en)
                if (wf_primary_step(K, src, en, W.data(), CQP.data()) & kWfWantClosest)
                    walk_closest(K, &CQP[en], Spill{W[(size_t)en << R.split_log2].sp, 1});
        }
        run_walks(K, want, W.data(), SQ.data(), CQ.data());
    }
    final_list(K, src, home.data(), accS, accQ, accN);
    if (steps_out) *steps_out = busy;
    return 0;
}

}  // extern "C"
