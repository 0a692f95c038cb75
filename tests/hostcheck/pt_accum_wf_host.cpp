// pt_accum_wf_host.cpp — TEST INFRASTRUCTURE.  One accumulator pass through
// the list form of the wavefront state machine (pt_wavefront.h wf_slot_step /
// wf_primary_step over a WfActive with the WfMoments home: the text
// k_wf_shade_list and k_wf_primary_list run; pt_hip.hip k_wf_final_list) run
// on the host on top of pt_hostcheck.cpp, with the walks hc_render_wavefront3
// runs (walk_shadow, walk_closest), so the CPU suite can check the pass against
// the single-kernel lane code (hc_render_moments) and the oracle's per-sample
// colours without a GPU.
// Built by tests/test_adaptive_wavefront_host.py into a temporary directory
// by the hostcheck Makefile's pattern rule (tests/hostlib.py).
#include "pt_hostcheck.cpp"

namespace {

// The launch record of a pass over n_list entries of p's frame under the rule
// A with `split` slots per entry, as pt_accum_render fills it (list_record);
// lanes: the host loop's slots, with no blocks to round up to.
ListK host_list(const pt_render_params* p, uint32_t n_list, const AdaptK& A, uint32_t split) {
    const PlanAccum acc{p->width, p->height, (uint32_t)p->width * (uint32_t)p->height, split, false, -1, -1};
    ListK R = list_record(p, acc, A, n_list, split, LaunchPlan{});
    R.lanes = (uint64_t)n_list << R.split_log2;
    return R;
}

// Slots t0 .. t0 + split - 1 reduced in store_pixel's xor order, slot t's value get(t)
template <class Get>
D3 reduce_slots(size_t t0, uint32_t split, Get&& get) {
    std::vector<D3> v(split);
    for (uint32_t c = 0; c < split; ++c) v[c] = get(t0 + c);
    return xor_reduce(v);
}
// slot t's sums (which = 0) or sums of squares (1) in a moment home [6][slots]
D3 home_at(const double* home, size_t slots, size_t t, int which) {
    const double* h = home + (size_t)(3 * which) * slots + t;
    return d3(h[0], h[slots], h[2 * slots]);
}

// k_wf_final_list: an entry's slots' six sums (home[6][slots]) reduced and
// added to the accumulator with the entry's k
void final_list(const SceneK& K, const WfActive& src, const double* home, double* accS, double* accQ,
                uint32_t* accN) {
    const ListK& R = src.R;
    const size_t slots = (size_t)R.lanes;
    for (uint32_t en = 0; en < R.n_list; ++en) {
        const ListJob j = src.job(K, en << R.split_log2);
        if (!j.valid || j.k == 0) continue;
        const size_t t0 = (size_t)en << R.split_log2;
        add3(accS + 3 * (size_t)j.e, reduce_slots(t0, R.split, [&](size_t t) { return home_at(home, slots, t, 0); }));
        add3(accQ + 3 * (size_t)j.e, reduce_slots(t0, R.split, [&](size_t t) { return home_at(home, slots, t, 1); }));
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
    if (!split_ok(split)) return -4;
    HostScene H;
    if (!open_scene(d, &H)) return -1;
    if (!wf_walkable(H.k)) return -3;
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
            ClosestStackLocal L;
            for (uint32_t en = 0; en < n_list; ++en)
                if (wf_primary_step(K, src, en, W.data(), CQP.data()) & kWfWantClosest)
                    walk_closest(K, &CQP[en], Spill{W[(size_t)en << R.split_log2].sp, 1}, L.view());
        }
        run_walks(K, want, W.data(), SQ.data(), CQ.data());
    }
    final_list(K, src, home.data(), accS, accQ, accN);
    if (steps_out) *steps_out = busy;
    return 0;
}

}  // extern "C"
