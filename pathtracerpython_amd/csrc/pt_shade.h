// pt_shade.h — what pt_hip.hip and pt_shade.hip share of the wavefront path's
// shade step: the wave-level helpers of the list appends and the declarations
// of the four shade kernels.  The kernels are defined in pt_shade.hip, a
// translation unit of their own so that they get their own code-generation
// flags (build.py UNITS), as the K2 kernel does (pt_k2.hip).
#pragma once
#include "pt_render.h"
#include "pt_wavefront.h"

// ------------------------------------------------- wavefront (BVH scenes) --
// pt_wavefront.h.  Queue counters: [0] shadow count, [1] shadow head,
// [2] closest count, [3] closest head; lists[0..3 slots) the shadow rays
// ((slot << 2) | ray), then [3 slots, 4 slots) closest.
// A walk kernel gets its list and its [count, head] pair.
__device__ __forceinline__ uint32_t lane_id() {
    return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}
__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {   // set bits of m below this lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// wave-aggregated append: one atomic per wave (the primary kernels' closest
// queries; the shade kernels append per block, pt_shade.hip wf_append_block)
__device__ __forceinline__ void wf_append(bool want, int32_t* counter, int32_t* list, int32_t v) {
    const uint64_t m = __ballot(want);
    if (m == 0) return;
    const uint32_t leader = (uint32_t)__ffsll((unsigned long long)m) - 1u;
    int32_t base = 0;
    if (lane_id() == leader) base = atomicAdd(counter, (int32_t)__popcll(m));
    base = __shfl(base, (int)leader);
    if (want) list[base + (int32_t)lanes_below(m)] = v;
}

// work-items per shade block (one append atomic per list and block): 256 /
// 512 / 1024 -> K5 1248 / 1255 / 1284 ms (512: two waves/SIMD at 135 VGPRs;
// 1024: 127 VGPRs with a spill)
#ifndef PT_SHADE_BLOCK
#define PT_SHADE_BLOCK 256
#endif
constexpr int kShadeBlock = PT_SHADE_BLOCK;
// (>= 128: wf_append_block issues its two list atomics from waves 0 and 1)
static_assert(kShadeBlock % 64 == 0 && kShadeBlock >= 128 && kShadeBlock <= 1024, "whole waves, >= 2");

// The shade step, one work-item per path slot (pt_wavefront.h wf_slot_step):
// a frame's slots (slot_job), and the list form of an accumulator pass
// (pt_accum_render: list_job, a path's colour to the slot's six sums
// home[6][slots] when the path ends); the antialiased forms (PT_FLAG_AA) start
// a primary query per sample and take no shared one (CQP).
__global__ __launch_bounds__(kShadeBlock) void k_wf_shade(SceneK S, RenderK R, int32_t step,
                                                  WfPath* __restrict__ W, WfShadowQ* __restrict__ SQ,
                                                  WfClosestQ* __restrict__ CQ, const WfClosestQ* __restrict__ CQP,
                                                  int32_t* __restrict__ lists, int32_t* counters,
                                                  uint32_t slots, uint16_t* __restrict__ keys);
__global__ __launch_bounds__(kShadeBlock) void k_wf_shade_list(
    SceneK S, ListK R, int32_t step, const uint32_t* __restrict__ list, const uint32_t* __restrict__ accN,
    WfPath* __restrict__ W, WfShadowQ* __restrict__ SQ, WfClosestQ* __restrict__ CQ,
    const WfClosestQ* __restrict__ CQP, int32_t* __restrict__ lists, int32_t* counters, uint32_t slots,
    uint16_t* __restrict__ keys, double* __restrict__ home);
__global__ __launch_bounds__(kShadeBlock) void k_wf_shade_aa(SceneK S, RenderK R, int32_t step,
                                                     WfPath* __restrict__ W, WfShadowQ* __restrict__ SQ,
                                                     WfClosestQ* __restrict__ CQ,
                                                     int32_t* __restrict__ lists, int32_t* counters,
                                                     uint32_t slots, uint16_t* __restrict__ keys);
__global__ __launch_bounds__(kShadeBlock) void k_wf_shade_list_aa(
    SceneK S, ListK R, int32_t step, const uint32_t* __restrict__ list, const uint32_t* __restrict__ accN,
    WfPath* __restrict__ W, WfShadowQ* __restrict__ SQ, WfClosestQ* __restrict__ CQ,
    int32_t* __restrict__ lists, int32_t* counters, uint32_t slots, uint16_t* __restrict__ keys,
    double* __restrict__ home);

// The thin-lens forms (PT_FLAG_LENS on a BVH scene; pt_shade_lens.hip): the
// launchers of k_wf_shade_lens<AA> / k_wf_shade_list_lens<AA> on grid x
// kShadeBlock work-items, aa: PT_FLAG_AA beside the lens.
void pt_wf_shade_lens(bool aa, dim3 grid, hipStream_t st, const SceneK& S, const RenderK& R, int32_t step,
                      WfPath* W, WfShadowQ* SQ, WfClosestQ* CQ, int32_t* lists, int32_t* counters, uint32_t slots,
                      uint16_t* keys);
// The ray forms (pt_radiance on a BVH scene; pt_shade_rays.hip): the launchers
// of k_wf_shade_rays<MOM>, k_wf_primary_rays and k_wf_final_rays<MOM>; home
// (the moment home [6][slots]) non-null: MOM, the moments S, Q as well.
void pt_wf_shade_rays(dim3 grid, hipStream_t st, const SceneK& S, const RaysK& R, int32_t step, const RayK* rays,
                      WfPath* W, WfShadowQ* SQ, WfClosestQ* CQ, const WfClosestQ* CQP, int32_t* lists,
                      int32_t* counters, uint32_t slots, uint16_t* keys, double* home);
void pt_wf_primary_rays(dim3 grid, hipStream_t st, const SceneK& S, const RaysK& R, const RayK* rays, WfPath* W,
                        WfClosestQ* CQP, int32_t* qlist, int32_t* counters);
void pt_wf_final_rays(dim3 grid, hipStream_t st, const RaysK& R, const WfPath* W, const double* home,
                      uint32_t slots, void* out, double* outS, double* outQ);
void pt_wf_shade_list_lens(bool aa, dim3 grid, hipStream_t st, const SceneK& S, const ListK& R, int32_t step,
                           const uint32_t* list, const uint32_t* accN, WfPath* W, WfShadowQ* SQ, WfClosestQ* CQ,
                           int32_t* lists, int32_t* counters, uint32_t slots, uint16_t* keys, double* home);
