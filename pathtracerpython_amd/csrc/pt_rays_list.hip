// pt_rays_list.hip — the kernels of a ray accumulator (pt_accum_create_rays,
// include/pt_capi.h): the list pass over ray records and the
// records' first-hit features.  k_render_rays_list is k_render_list with the
// record rays[e] in the place of pixel e's primary ray, as k_render_rays is
// k_render's: a work-item is (list entry, sample slice) (rays_list_job,
// pt_job.h), the primary hit is traced once per lane and pass with per-lane
// origin terms (rays_primary), the paths run through render_lane_cached (RayHit, MomentSink).
// A translation unit of its own (build.py AA_UNITS), so that no other unit's
// code moves.  pt_hip.hip launches both through the functions at the end.
#include "pt_render.h"
#include "pt_rays_list.h"

#ifndef PT_LIST_WAVES
#define PT_LIST_WAVES PT_RENDER_WAVES
#endif

// k_render_list's block shape, spill home and reduction.  The lanes of an
// entry read the same 56-byte record; they reduce S and Q in store_pixel's
// xor order and lane 0 adds them to the accumulator with plain loads and
// stores (the list is unique).
template <bool FORCE64, bool BVH>
__global__ __launch_bounds__(kRenderBlock, PT_LIST_WAVES) void k_render_rays_list(
    SceneK S, RaysListK R, const RayK* __restrict__ rays, const uint32_t* __restrict__ list,
    double* __restrict__ accS, double* __restrict__ accQ, uint32_t* __restrict__ accN) {
    __shared__ double spill[kSpillSlots][kRenderBlock];
    const Spill sp{&spill[0][threadIdx.x], (int)kRenderBlock};
    const uint32_t tid = blockIdx.x * kRenderBlock + threadIdx.x;
    // (entries that are no record of the accumulator are skipped before any
    // access; the launch's constants stay outside the branch: rays_list_job)
    const RayListJob j = rays_list_job(R, rays, list, accN, tid);
    MomentRegs M;
    M.clear();
    if (j.valid) {
        Counters cnt = {};
        D3 P0 = d3(0, 0, 0);
        int tri0 = -1;
        // the primary hit once per lane and pass: every sample of the record shares it
        if (j.J.n_samples > 0 && R.bounces > 0)
            tri0 = rays_primary<FORCE64, BVH>(S, R.frame_x, ld3(j.ray->o), ld3(j.ray->d), sp, &P0, &cnt);
        render_lane_cached<FORCE64, false, BVH>(S, j.J, RayHit{j.ray, tri0}, P0, sp, &cnt, MomentSink<MomentRegs>{M});
    }
    D3 s = M.sum(), q = M.sumsq();
    for (uint32_t m = 1; m < R.split; m <<= 1) {
        s.x += __shfl_xor(s.x, (int)m); s.y += __shfl_xor(s.y, (int)m); s.z += __shfl_xor(s.z, (int)m);
        q.x += __shfl_xor(q.x, (int)m); q.y += __shfl_xor(q.y, (int)m); q.z += __shfl_xor(q.z, (int)m);
    }
    if (j.valid && (tid & (R.split - 1u)) == 0 && j.k > 0) {
        double* ps = accS + (size_t)j.e * 3;
        double* pq = accQ + (size_t)j.e * 3;
        ps[0] += s.x; ps[1] += s.y; ps[2] += s.z;
        pq[0] += q.x; pq[1] += q.y; pq[2] += q.z;
        accN[j.e] += j.k;
    }
}

// First-hit features of the records: k_features (pt_denoise.h) with record
// e's ray in the place of the eye and the linspace point, traced as the pass
// traces it (rays_primary: an origin outside the frame is decided in f64).
template <bool BVH>
__global__ __launch_bounds__(256) void k_features_rays(SceneK S, double frame_x, const RayK* __restrict__ rays,
                                                       uint32_t n, int32_t* __restrict__ tri,
                                                       int32_t* __restrict__ obj, double* __restrict__ N,
                                                       double* __restrict__ P) {
    __shared__ double spill[kSpillSlots][256];
    const Spill sp{&spill[0][threadIdx.x], 256};
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= (uint64_t)n) return;
    const RayK* ray = rays + e;
    Counters cnt = {};
    D3 P0 = d3(0, 0, 0);
    const int t = rays_primary<false, BVH>(S, frame_x, ld3(ray->o), ld3(ray->d), sp, &P0, &cnt);
    const bool hit = t >= 0 && t < S.n_tri;   // (never indexes the tables with anything else)
    tri[e] = hit ? t : -1;
    obj[e] = hit ? S.tri_obj[t] : -1;
    for (int k = 0; k < 3; ++k) N[e * 3 + k] = hit ? S.tris[t].n[k] : 0.0;
    P[e * 3] = hit ? P0.x : 0.0;
    P[e * 3 + 1] = hit ? P0.y : 0.0;
    P[e * 3 + 2] = hit ? P0.z : 0.0;
}

void pt_rays_render_list(bool f64, bool bvh, dim3 grid, hipStream_t st, const SceneK& S, const RaysListK& R,
                         const RayK* rays, const uint32_t* list, double* accS, double* accQ, uint32_t* accN) {
    const dim3 block(kRenderBlock);
    hipLaunchKernelGGL(PT_KERNEL_F64_BVH(f64, bvh, k_render_rays_list), grid, block, 0, st, S, R, rays, list, accS,
                       accQ, accN);
}

void pt_rays_features(bool bvh, hipStream_t st, const SceneK& S, double frame_x, const RayK* rays, uint32_t n,
                      int32_t* tri, int32_t* obj, double* N, double* P) {
    const dim3 grid((n + 255u) / 256u), block(256);
    if (bvh) hipLaunchKernelGGL((k_features_rays<true>), grid, block, 0, st, S, frame_x, rays, n, tri, obj, N, P);
    else hipLaunchKernelGGL((k_features_rays<false>), grid, block, 0, st, S, frame_x, rays, n, tri, obj, N, P);
}
