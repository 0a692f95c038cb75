// pt_shade_rays.hip — the wavefront path's kernels for caller-supplied rays
// (pt_radiance on a BVH scene): k_wf_shade's body
// (pt_shade_block.h) with the ray step (pt_wavefront.h wf_shade_rays over a
// WfRays source), the primary step of a record (wf_rays_primary_step) and the
// epilogue that writes a record's mean, S and Q as k_render_rays does.  MOM:
// the moments S, Q as well (the WfMoments home [6][slots]).  A translation
// unit of its own, so that the kernels of pt_shade.hip, pt_shade_lens.hip and
// pt_hip.hip stay as they were; build.py gives it the shade units' flags.
// pt_hip.hip launches them through pt_wf_shade_rays / pt_wf_primary_rays /
// pt_wf_final_rays (pt_shade.h); the walk and sort kernels are pt_hip.hip's.
#include "pt_shade_block.h"

template <bool MOM>
__global__ __launch_bounds__(kShadeBlock) void k_wf_shade_rays(
    SceneK S, RaysK R, int32_t step, const RayK* __restrict__ rays, WfPath* __restrict__ W,
    WfShadowQ* __restrict__ SQ, WfClosestQ* __restrict__ CQ, const WfClosestQ* __restrict__ CQP,
    int32_t* __restrict__ lists, int32_t* counters, uint32_t slots, uint16_t* __restrict__ keys,
    double* __restrict__ home) {
    if constexpr (MOM)
        shade_block<false, WfMoments>(S, WfRays{R, rays}, step, W, SQ, CQ, CQP, lists, counters, slots, keys, home);
    else
        shade_block<false, WfSum>(S, WfRays{R, rays}, step, W, SQ, CQ, CQP, lists, counters, slots, keys, nullptr);
}

// The primary rays, one work-item per record (the record's `split` slots share
// it): CQP[entry], spill home in the entry's first slot, list entry = entry
// (k_wf_closest's wshift = split_log2), as k_wf_primary_list.  A record whose
// origin lies outside the filter's frame is decided here in f64 and appends
// nothing.
__global__ __launch_bounds__(256) void k_wf_primary_rays(SceneK S, RaysK R, const RayK* __restrict__ rays,
                                                         WfPath* __restrict__ W, WfClosestQ* __restrict__ CQP,
                                                         int32_t* __restrict__ qlist, int32_t* counters) {
    const uint32_t entry = blockIdx.x * 256u + threadIdx.x;
    const uint32_t want = wf_rays_primary_step(S, WfRays{R, rays}, entry, W, CQP);
    wf_append((want & kWfWantClosest) != 0, counters, qlist, (int32_t)entry);
}

// k_render_rays' epilogue over the slots (one block of 256 per 256 slots): a
// record's slots reduce their sums in the same xor order; slot 0 writes the
// mean s / spp in the output's type and, with MOM, S and Q (the mean from S).
template <bool MOM>
__global__ __launch_bounds__(256) void k_wf_final_rays(RaysK R, const WfPath* __restrict__ W,
                                                       const double* __restrict__ home, uint32_t slots,
                                                       void* __restrict__ out, double* __restrict__ outS,
                                                       double* __restrict__ outQ) {
    const uint32_t tid = blockIdx.x * 256u + threadIdx.x;   // < slots
    const uint32_t entry = tid >> R.split_log2, c = tid & (R.split - 1u);
    const bool valid = entry < R.n_rays;
    D3 s = d3(0, 0, 0), q = d3(0, 0, 0);
    if (valid) {
        if constexpr (MOM) {
            const double* h = home + tid;
            s = d3(h[0], h[slots], h[2 * (size_t)slots]);
            q = d3(h[3 * (size_t)slots], h[4 * (size_t)slots], h[5 * (size_t)slots]);
        } else {
            s = ld3(W[tid].acc);
        }
    }
    for (uint32_t m = 1; m < R.split; m <<= 1) {
        s.x += __shfl_xor(s.x, (int)m); s.y += __shfl_xor(s.y, (int)m); s.z += __shfl_xor(s.z, (int)m);
        if constexpr (MOM) {
            q.x += __shfl_xor(q.x, (int)m); q.y += __shfl_xor(q.y, (int)m); q.z += __shfl_xor(q.z, (int)m);
        }
    }
    if (valid && c == 0) {
        const size_t e = (size_t)entry * 3;
        const double inv = (double)R.spp;   // the mean as store_pixel forms it
        if (R.out_f64) {
            double* o = (double*)out + e;
            o[0] = s.x / inv; o[1] = s.y / inv; o[2] = s.z / inv;
        } else {
            float* o = (float*)out + e;
            o[0] = (float)(s.x / inv); o[1] = (float)(s.y / inv); o[2] = (float)(s.z / inv);
        }
        if constexpr (MOM) {
            outS[e] = s.x; outS[e + 1] = s.y; outS[e + 2] = s.z;
            outQ[e] = q.x; outQ[e + 1] = q.y; outQ[e + 2] = q.z;
        }
    }
}

void pt_wf_shade_rays(dim3 grid, hipStream_t st, const SceneK& S, const RaysK& R, int32_t step, const RayK* rays,
                      WfPath* W, WfShadowQ* SQ, WfClosestQ* CQ, const WfClosestQ* CQP, int32_t* lists,
                      int32_t* counters, uint32_t slots, uint16_t* keys, double* home) {
    const dim3 block(kShadeBlock);
    if (home)
        hipLaunchKernelGGL(k_wf_shade_rays<true>, grid, block, 0, st, S, R, step, rays, W, SQ, CQ, CQP, lists,
                           counters, slots, keys, home);
    else
        hipLaunchKernelGGL(k_wf_shade_rays<false>, grid, block, 0, st, S, R, step, rays, W, SQ, CQ, CQP, lists,
                           counters, slots, keys, home);
}
void pt_wf_primary_rays(dim3 grid, hipStream_t st, const SceneK& S, const RaysK& R, const RayK* rays, WfPath* W,
                        WfClosestQ* CQP, int32_t* qlist, int32_t* counters) {
    hipLaunchKernelGGL(k_wf_primary_rays, grid, dim3(256), 0, st, S, R, rays, W, CQP, qlist, counters);
}
void pt_wf_final_rays(dim3 grid, hipStream_t st, const RaysK& R, const WfPath* W, const double* home,
                      uint32_t slots, void* out, double* outS, double* outQ) {
    if (home)
        hipLaunchKernelGGL(k_wf_final_rays<true>, grid, dim3(256), 0, st, R, W, home, slots, out, outS, outQ);
    else
        hipLaunchKernelGGL(k_wf_final_rays<false>, grid, dim3(256), 0, st, R, W, home, slots, out, outS, outQ);
}
