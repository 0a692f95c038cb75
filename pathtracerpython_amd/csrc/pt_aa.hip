// pt_aa.hip — the antialiasing kernels (PT_FLAG_AA, include/pt_capi.h;
// DESIGN.md §4.3): k_render and k_render_list with a jittered primary ray per
// sample (pt_path.h AaRay; SumSink / MomentSink) instead of the pixel's cached
// one.  A translation unit of its own (build.py AA_UNITS): the kernels get
// their own code-generation flags and the other units' code does not move.
// pt_hip.hip launches them through pt_aa_render / pt_aa_render_list.
#include "pt_render.h"
#include "pt_aa.h"

// The wave's table of the eye's origin terms (pt_path.h AaEye) in the spill
// rows from kSpD0 on, which no antialiased path uses: lane l computes units l,
// l + 64, ... (a per-lane unit index: vector loads of the records).  One wave
// per block, so the barrier is the wave's own.  PT_AA_EYE_LDS 0: no table.
#ifndef PT_AA_EYE_LDS
#define PT_AA_EYE_LDS 1
#endif
static_assert(kRenderBlock == 64, "aa_eye_fill: one wave per block");
static_assert((kSpillSlots - kSpD0) * kRenderBlock * sizeof(double) >= kAaEyeCap * 8 * sizeof(float),
              "the eye table fits the free spill rows");
template <bool FORCE64>
__device__ __forceinline__ AaEye aa_eye_fill(const SceneK& S, double (*spill)[kRenderBlock]) {
    if (FORCE64 || !PT_AA_EYE_LDS) return AaEye{nullptr, 0};
    float* t = (float*)&spill[kSpD0][0];
    const int n = S.n_unit < kAaEyeCap ? S.n_unit : kAaEyeCap;
    const F3 o32 = to_f3(ld3(S.kd + kKdEye) - ld3(S.kd + kKdCenter));
    for (int u = (int)threadIdx.x; u < n; u += (int)kRenderBlock) {
        const UnitF U = S.unit_eye[u];
        const OriginU O = origin_q(U, o32);
        float* r = t + 8 * u;
        r[0] = O.h; r[1] = O.bo0; r[2] = O.co0; r[3] = O.bo1; r[4] = O.co1;
    }
    __syncthreads();
    return AaEye{t, n};
}

// k_render's block shape and work-item -> (pixel, sample slice) mapping (tail
// rows included); no cached primary hit and no primary_shared: every sample
// of every lane traces its own primary ray inside the sample scheduler.
template <bool FORCE64, bool BVH>
__global__ __launch_bounds__(kRenderBlock, PT_RENDER_WAVES) void k_render_aa(SceneK S, RenderK R,
                                                                             void* __restrict__ out) {
    __shared__ double spill[kSpillSlots][kRenderBlock];
    const Spill sp{&spill[0][threadIdx.x], (int)kRenderBlock};
    const uint32_t tid = blockIdx.x * kRenderBlock + threadIdx.x;
    const PixelMap m = pixel_map(R, tid);
    D3 acc = d3(0, 0, 0);
    int32_t row_local = 0, ix = 0;
    const AaEye E = aa_eye_fill<FORCE64>(S, spill);
    if (m.valid) {
        row_local = (int32_t)(m.pl / (uint32_t)R.W);
        ix = (int32_t)m.pl - row_local * R.W;
        const int32_t iy = R.first_row + row_local * R.row_step;
        LaneJob J;
        J.seed = R.seed;
        J.pixel = (uint32_t)ix * (uint32_t)R.H + (uint32_t)iy;
        J.sample0 = R.sample_begin + (int32_t)m.c;
        J.sample_stride = (int32_t)m.split;
        J.n_samples = ((int32_t)m.c < R.spp) ? (R.spp - (int32_t)m.c + (int32_t)m.split - 1) / (int32_t)m.split : 0;
        J.bounces = R.bounces;
        J.rr_depth = R.rr_depth;
        Counters cnt = {};
        acc = render_lane_sampled<FORCE64, BVH>(S, J, AaRay<FORCE64, BVH>{{R.W, R.H, ix, iy}, E}, sp, &cnt, SumSink{});
    }
    SlotJob j;
    j.valid = m.valid;
    j.c = m.c;
    j.row_local = row_local;
    j.ix = ix;
    store_pixel(R, j, acc, out, m.split);
}

// k_render_list's mapping and reduction (the moments in the lane's registers)
template <bool FORCE64, bool BVH>
__global__ __launch_bounds__(kRenderBlock, PT_RENDER_WAVES) void k_render_list_aa(
    SceneK S, ListK R, const uint32_t* __restrict__ list, double* __restrict__ accS,
    double* __restrict__ accQ, uint32_t* __restrict__ accN) {
    __shared__ double spill[kSpillSlots][kRenderBlock];
    const Spill sp{&spill[0][threadIdx.x], (int)kRenderBlock};
    const uint32_t tid = blockIdx.x * kRenderBlock + threadIdx.x;
    const uint32_t entry = tid >> R.split_log2, c = tid & (R.split - 1u);
    // (entries that are no pixel of the frame are skipped, never dereferenced)
    const uint32_t e = entry < R.n_list ? list[entry] : 0xffffffffu;
    const bool valid = e < R.npix;   // the same for all lanes of an entry
    MomentRegs M;
    uint32_t k = 0;
    const AaEye E = aa_eye_fill<FORCE64>(S, spill);
    if (valid) {
        M.clear();
        const uint32_t n0 = accN[e];
        k = adapt_k(n0, R.A);
        const int32_t row = (int32_t)(e / (uint32_t)R.W);
        const int32_t ix = (int32_t)e - row * R.W, iy = R.H - 1 - row;
        LaneJob J;
        J.seed = R.seed;
        J.pixel = (uint32_t)ix * (uint32_t)R.H + (uint32_t)iy;
        J.sample0 = (int32_t)(n0 + c);
        J.sample_stride = (int32_t)R.split;
        J.n_samples = c < k ? (int32_t)((k - c + R.split - 1u) >> R.split_log2) : 0;
        J.bounces = R.bounces;
        J.rr_depth = R.rr_depth;
        Counters cnt = {};
        render_lane_sampled<FORCE64, BVH>(S, J, AaRay<FORCE64, BVH>{{R.W, R.H, ix, iy}, E}, sp, &cnt,
                                          MomentSink<MomentRegs>{M});
    }
    D3 s = valid ? M.sum() : d3(0, 0, 0), q = valid ? M.sumsq() : d3(0, 0, 0);
    for (uint32_t m = 1; m < R.split; m <<= 1) {
        s.x += __shfl_xor(s.x, (int)m); s.y += __shfl_xor(s.y, (int)m); s.z += __shfl_xor(s.z, (int)m);
        q.x += __shfl_xor(q.x, (int)m); q.y += __shfl_xor(q.y, (int)m); q.z += __shfl_xor(q.z, (int)m);
    }
    if (valid && c == 0 && k > 0) {
        double* ps = accS + (size_t)e * 3;
        double* pq = accQ + (size_t)e * 3;
        ps[0] += s.x; ps[1] += s.y; ps[2] += s.z;
        pq[0] += q.x; pq[1] += q.y; pq[2] += q.z;
        accN[e] += k;
    }
}

void pt_aa_render(bool f64, bool bvh, dim3 grid, hipStream_t st, const SceneK& S, const RenderK& R, void* out) {
    const dim3 block(kRenderBlock);
    hipLaunchKernelGGL(PT_KERNEL_F64_BVH(f64, bvh, k_render_aa), grid, block, 0, st, S, R, out);
}

void pt_aa_render_list(bool f64, bool bvh, dim3 grid, hipStream_t st, const SceneK& S, const ListK& R,
                       const uint32_t* list, double* accS, double* accQ, uint32_t* accN) {
    const dim3 block(kRenderBlock);
    hipLaunchKernelGGL(PT_KERNEL_F64_BVH(f64, bvh, k_render_list_aa), grid, block, 0, st, S, R, list, accS, accQ,
                       accN);
}
