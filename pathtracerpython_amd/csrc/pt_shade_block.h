// pt_shade_block.h — the body of the wavefront shade kernels (pt_shade.hip,
// pt_shade_lens.hip): the slot's step (pt_wavefront.h wf_slot_step), then the
// block's appends to the two query lists.
#pragma once
#include "pt_shade.h"

// Both lists' appends of a kShadeBlock-work-item block with one atomic per
// list and block: every block's appends land on the same two counters, whose
// atomics serialise (~10 ns each: three per wave on one counter made the shade
// step 6 -> 11.6 ms at 262k waves).  Shadow entries (slot << 2) | ray for the
// rays in bits 0..2 of want, a slot's rays next to each other (they share the
// query record and the origin: 94.1 vs 96.5 ms ray-major on K5 512^2 x 64),
// the block's waves in order; skeys: each shadow entry's sort key (the
// origin's cell, render_wavefront's counting sort).
__device__ __forceinline__ void wf_append_block(uint32_t want, int32_t* counters, int32_t* shadow_list,
                                                int32_t* closest_list, int32_t slot, uint16_t* skeys,
                                                uint32_t skey) {
    constexpr int kWaves = kShadeBlock / 64;
    __shared__ int32_t cnt[2][kWaves], base[2];
    uint64_t m[kLightSamples];
    int32_t n = 0;
#pragma unroll
    for (int k = 0; k < kLightSamples; ++k) {
        m[k] = __ballot(((want >> k) & 1u) != 0);
        n += (int32_t)__popcll(m[k]);
    }
    const uint64_t mc = __ballot((want & kWfWantClosest) != 0);
    const int wv = (int)(threadIdx.x >> 6);
    if ((threadIdx.x & 63u) == 0) {
        cnt[0][wv] = n;
        cnt[1][wv] = (int32_t)__popcll(mc);
    }
    __syncthreads();
    if (threadIdx.x == 0 || threadIdx.x == 64) {   // the two atomics from two waves
        const int l = threadIdx.x == 0 ? 0 : 1;
        int32_t tot = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) tot += cnt[l][w];
        base[l] = tot ? atomicAdd(&counters[2 * l], tot) : 0;
    }
    __syncthreads();
    int32_t bs = base[0], bc = base[1];
    for (int w = 0; w < wv; ++w) {
        bs += cnt[0][w];
        bc += cnt[1][w];
    }
#pragma unroll
    for (int k = 0; k < kLightSamples; ++k) bs += (int32_t)lanes_below(m[k]);
#pragma unroll
    for (int k = 0; k < kLightSamples; ++k)
        if ((want >> k) & 1u) {
            if (skeys) skeys[bs] = (uint16_t)skey;
            shadow_list[bs++] = wf_shadow_entry(slot, k);
        }
    if (want & kWfWantClosest) closest_list[bc + (int32_t)lanes_below(mc)] = slot;
}

// The shade kernels' body: the slot's step, then the block's appends (every
// work-item of the block takes part in them: the last block of a kShadeBlock
// grid over 256-slot blocks has work-items past the slots).
// LENS: the thin-lens step (pt_shade_lens.hip).
template <bool AA, class Home, bool LENS = false, class Src>
__device__ __forceinline__ void shade_block(const SceneK& S, const Src& src, int32_t step, WfPath* W,
                                            WfShadowQ* SQ, WfClosestQ* CQ, const WfClosestQ* CQP, int32_t* lists,
                                            int32_t* counters, uint32_t slots, uint16_t* keys, double* home) {
    const uint32_t tid = blockIdx.x * (uint32_t)kShadeBlock + threadIdx.x;
    Home h{};
    if constexpr (Home::kMoments) h = Home{{home + tid, (size_t)slots}};
    uint32_t want = 0;
    if (tid < slots) want = wf_slot_step<AA, LENS>(S, src, step, tid, W, SQ, CQ, CQP, h);
    wf_append_block(want & 0xffffu, counters, lists, lists + 3 * (size_t)slots, (int32_t)tid, keys, want >> 16);
}
