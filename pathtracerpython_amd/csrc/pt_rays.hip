// pt_rays.hip — the ray kernel (pt_radiance, include/pt_capi.h; DESIGN.md
// §4.4): the path loop for caller-supplied primary rays.  A work-item is
// (record, sample slice) as k_render_list's is (list entry, sample slice); the
// primary ray, the specular term's eye and the Philox pixel word come from the
// record (pt_path.h RayHit; SumSink / MomentSink).  Origins differ across a
// wave, so each lane computes its own origin terms as the lens kernels do,
// but the primary hit is traced once per lane and cached as k_render's is.
// A translation unit of its own (build.py AA_UNITS), so that no other unit's
// code moves.  pt_hip.hip launches it through pt_rays_render.
#include "pt_render.h"
#include "pt_rays.h"

// k_render_list's block shape, spill home and reduction.  MOM: the moments
// S, Q as well, summed sample by sample (MomentSink), the mean from S;
// without them the samples are summed as k_render sums them (SumSink).
template <bool FORCE64, bool BVH, bool MOM>
__global__ __launch_bounds__(kRenderBlock, PT_RENDER_WAVES) void k_render_rays(
    SceneK S, RaysK R, const RayK* __restrict__ rays, void* __restrict__ out, double* __restrict__ outS,
    double* __restrict__ outQ) {
    __shared__ double spill[kSpillSlots][kRenderBlock];
    const Spill sp{&spill[0][threadIdx.x], (int)kRenderBlock};
    const uint32_t tid = blockIdx.x * kRenderBlock + threadIdx.x;
    const uint32_t entry = tid >> R.split_log2, c = tid & (R.split - 1u);
    // (entries past the batch are skipped before any access; the same for all lanes of an entry)
    const bool valid = entry < R.n_rays;
    MomentRegs M;
    M.clear();
    D3 acc = d3(0, 0, 0);
    if (valid) {
        const RayK* ray = rays + entry;
        LaneJob J;
        J.seed = R.seed;
        J.pixel = ray->key;
        J.sample0 = R.sample_begin + (int32_t)c;
        J.sample_stride = (int32_t)R.split;
        J.n_samples = ((int32_t)c < R.spp) ? (R.spp - (int32_t)c + (int32_t)R.split - 1) / (int32_t)R.split : 0;
        J.bounces = R.bounces;
        J.rr_depth = R.rr_depth;
        Counters cnt = {};
        D3 P0 = d3(0, 0, 0);
        int tri0 = -1;
        // the primary hit once per lane: every sample of the record shares it
        if (J.n_samples > 0 && R.bounces > 0)
            tri0 = rays_primary<FORCE64, BVH>(S, R.frame_x, ld3(ray->o), ld3(ray->d), sp, &P0, &cnt);
        if constexpr (MOM) render_lane_cached<FORCE64, false, BVH>(S, J, RayHit{ray, tri0}, P0, sp, &cnt, MomentSink<MomentRegs>{M});
        else acc = render_lane_cached<FORCE64, false, BVH>(S, J, RayHit{ray, tri0}, P0, sp, &cnt, SumSink{});
    }
    D3 s = MOM ? M.sum() : acc, q = M.sumsq();
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

template <bool MOM>
static void rays_render(bool f64, bool bvh, dim3 grid, hipStream_t st, const SceneK& S, const RaysK& R,
                        const RayK* rays, void* out, double* outS, double* outQ) {
    const dim3 block(kRenderBlock);
    hipLaunchKernelGGL(PT_KERNEL_F64_BVH(f64, bvh, k_render_rays, MOM), grid, block, 0, st, S, R, rays, out, outS,
                       outQ);
}
void pt_rays_render(bool f64, bool bvh, dim3 grid, hipStream_t st, const SceneK& S, const RaysK& R,
                    const RayK* rays, void* out, double* outS, double* outQ) {
    if (outS) rays_render<true>(f64, bvh, grid, st, S, R, rays, out, outS, outQ);
    else rays_render<false>(f64, bvh, grid, st, S, R, rays, out, outS, outQ);
}
