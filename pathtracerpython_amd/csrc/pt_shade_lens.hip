// pt_shade_lens.hip — the wavefront path's shade step through the thin lens
// (PT_FLAG_LENS on a BVH scene): k_wf_shade_aa's and
// k_wf_shade_list_aa's body (pt_shade_block.h) with a lens point per sample
// (pt_wavefront.h wf_lens_start, wf_shade_lens).  AA (PT_FLAG_AA beside the
// lens) is a template parameter, not an argument (pt_path.h lens_point).  A
// translation unit of its own, so that the four kernels of pt_shade.hip stay
// as they were; build.py gives it the same flags.  pt_hip.hip launches them
// through pt_wf_shade_lens / pt_wf_shade_list_lens (pt_shade.h).
#include "pt_shade_block.h"

template <bool AA>
__global__ __launch_bounds__(kShadeBlock) void k_wf_shade_lens(SceneK S, RenderK R, int32_t step,
                                                       WfPath* __restrict__ W, WfShadowQ* __restrict__ SQ,
                                                       WfClosestQ* __restrict__ CQ,
                                                       int32_t* __restrict__ lists, int32_t* counters,
                                                       uint32_t slots, uint16_t* __restrict__ keys) {
    shade_block<AA, WfSum, true>(S, WfFrame{R}, step, W, SQ, CQ, nullptr, lists, counters, slots, keys, nullptr);
}
template <bool AA>
__global__ __launch_bounds__(kShadeBlock) void k_wf_shade_list_lens(
    SceneK S, ListK R, int32_t step, const uint32_t* __restrict__ list, const uint32_t* __restrict__ accN,
    WfPath* __restrict__ W, WfShadowQ* __restrict__ SQ, WfClosestQ* __restrict__ CQ,
    int32_t* __restrict__ lists, int32_t* counters, uint32_t slots, uint16_t* __restrict__ keys,
    double* __restrict__ home) {
    shade_block<AA, WfMoments, true>(S, WfActive{R, list, accN}, step, W, SQ, CQ, nullptr, lists, counters, slots,
                                     keys, home);
}

void pt_wf_shade_lens(bool aa, dim3 grid, hipStream_t st, const SceneK& S, const RenderK& R, int32_t step,
                      WfPath* W, WfShadowQ* SQ, WfClosestQ* CQ, int32_t* lists, int32_t* counters, uint32_t slots,
                      uint16_t* keys) {
    const dim3 block(kShadeBlock);
    if (aa) hipLaunchKernelGGL(k_wf_shade_lens<true>, grid, block, 0, st, S, R, step, W, SQ, CQ, lists, counters, slots, keys);
    else hipLaunchKernelGGL(k_wf_shade_lens<false>, grid, block, 0, st, S, R, step, W, SQ, CQ, lists, counters, slots, keys);
}
void pt_wf_shade_list_lens(bool aa, dim3 grid, hipStream_t st, const SceneK& S, const ListK& R, int32_t step,
                           const uint32_t* list, const uint32_t* accN, WfPath* W, WfShadowQ* SQ, WfClosestQ* CQ,
                           int32_t* lists, int32_t* counters, uint32_t slots, uint16_t* keys, double* home) {
    const dim3 block(kShadeBlock);
    if (aa)
        hipLaunchKernelGGL(k_wf_shade_list_lens<true>, grid, block, 0, st, S, R, step, list, accN, W, SQ, CQ, lists,
                           counters, slots, keys, home);
    else
        hipLaunchKernelGGL(k_wf_shade_list_lens<false>, grid, block, 0, st, S, R, step, list, accN, W, SQ, CQ, lists,
                           counters, slots, keys, home);
}
