// pt_shade.hip — the wavefront path's shade step: one body (pt_shade_block.h:
// pt_wavefront.h wf_slot_step, then the block's list appends) behind the four kernels
// k_wf_shade, k_wf_shade_list, k_wf_shade_aa and k_wf_shade_list_aa
// (pt_shade.h), in a translation unit of its own: build.py compiles it with
// LLVM's iterative ILP scheduler (its unit pass is the K2 kernel's), while the
// walk kernels of pt_hip.hip keep the default scheduler (DESIGN.md §11,
// round 6).
#include "pt_shade_block.h"

__global__ __launch_bounds__(kShadeBlock) void k_wf_shade(SceneK S, RenderK R, int32_t step,
                                                  WfPath* __restrict__ W, WfShadowQ* __restrict__ SQ,
                                                  WfClosestQ* __restrict__ CQ, const WfClosestQ* __restrict__ CQP,
                                                  int32_t* __restrict__ lists, int32_t* counters,
                                                  uint32_t slots, uint16_t* __restrict__ keys) {
    shade_block<false, WfSum>(S, WfFrame{R}, step, W, SQ, CQ, CQP, lists, counters, slots, keys, nullptr);
}
__global__ __launch_bounds__(kShadeBlock) void k_wf_shade_list(
    SceneK S, ListK R, int32_t step, const uint32_t* __restrict__ list, const uint32_t* __restrict__ accN,
    WfPath* __restrict__ W, WfShadowQ* __restrict__ SQ, WfClosestQ* __restrict__ CQ,
    const WfClosestQ* __restrict__ CQP, int32_t* __restrict__ lists, int32_t* counters, uint32_t slots,
    uint16_t* __restrict__ keys, double* __restrict__ home) {
    shade_block<false, WfMoments>(S, WfActive{R, list, accN}, step, W, SQ, CQ, CQP, lists, counters, slots, keys,
                                  home);
}
__global__ __launch_bounds__(kShadeBlock) void k_wf_shade_aa(SceneK S, RenderK R, int32_t step,
                                                     WfPath* __restrict__ W, WfShadowQ* __restrict__ SQ,
                                                     WfClosestQ* __restrict__ CQ,
                                                     int32_t* __restrict__ lists, int32_t* counters,
                                                     uint32_t slots, uint16_t* __restrict__ keys) {
    shade_block<true, WfSum>(S, WfFrame{R}, step, W, SQ, CQ, nullptr, lists, counters, slots, keys, nullptr);
}
__global__ __launch_bounds__(kShadeBlock) void k_wf_shade_list_aa(
    SceneK S, ListK R, int32_t step, const uint32_t* __restrict__ list, const uint32_t* __restrict__ accN,
    WfPath* __restrict__ W, WfShadowQ* __restrict__ SQ, WfClosestQ* __restrict__ CQ,
    int32_t* __restrict__ lists, int32_t* counters, uint32_t slots, uint16_t* __restrict__ keys,
    double* __restrict__ home) {
    shade_block<true, WfMoments>(S, WfActive{R, list, accN}, step, W, SQ, CQ, nullptr, lists, counters, slots,
                                 keys, home);
}
