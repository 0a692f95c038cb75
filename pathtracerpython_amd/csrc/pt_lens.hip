// pt_lens.hip — the thin-lens kernels (PT_FLAG_LENS, include/pt_capi.h;
// DESIGN.md §4.3): k_render_aa and k_render_list_aa with a lens point per
// sample (pt_path.h LensRay; SumSink / MomentSink).  Every sample's primary
// ray starts at its own origin eye', so there is no wave-shared table of the eye's
// origin terms (pt_aa.hip aa_eye_fill): each lane computes origin_q for its
// origin, and the first two spill rows the table used carry eye' for the
// sample's bounces.  A translation unit of its own (build.py AA_UNITS), so
// that no other unit's code moves.  pt_hip.hip launches them through
// pt_lens_render / pt_lens_render_list.
#include "pt_render.h"
#include "pt_lens.h"

// k_render_aa's block shape, work mapping and store; AA: jitter as well
// (a template parameter, not an argument: pt_path.h lens_point)
template <bool FORCE64, bool BVH, bool AA>
__global__ __launch_bounds__(kRenderBlock, PT_RENDER_WAVES) void k_render_lens(SceneK S, RenderK R,
                                                                               void* __restrict__ out) {
    __shared__ double spill[kSpillSlots][kRenderBlock];
    const Spill sp{&spill[0][threadIdx.x], (int)kRenderBlock};
    const uint32_t tid = blockIdx.x * kRenderBlock + threadIdx.x;
    const PixelMap m = pixel_map(R, tid);
    D3 acc = d3(0, 0, 0);
    int32_t row_local = 0, ix = 0;
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
        acc = render_lane_sampled<FORCE64, BVH>(S, J, LensRay<FORCE64, BVH, AA>{{R.W, R.H, ix, iy}}, sp, &cnt, SumSink{});
    }
    SlotJob j;
    j.valid = m.valid;
    j.c = m.c;
    j.row_local = row_local;
    j.ix = ix;
    store_pixel(R, j, acc, out, m.split);
}

// k_render_list_aa's mapping and reduction
template <bool FORCE64, bool BVH, bool AA>
__global__ __launch_bounds__(kRenderBlock, PT_RENDER_WAVES) void k_render_list_lens(
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
        render_lane_sampled<FORCE64, BVH>(S, J, LensRay<FORCE64, BVH, AA>{{R.W, R.H, ix, iy}}, sp, &cnt,
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

template <bool AA>
static void lens_render(bool f64, bool bvh, dim3 grid, hipStream_t st, const SceneK& S, const RenderK& R, void* out) {
    const dim3 block(kRenderBlock);
    hipLaunchKernelGGL(PT_KERNEL_F64_BVH(f64, bvh, k_render_lens, AA), grid, block, 0, st, S, R, out);
}
void pt_lens_render(bool f64, bool bvh, bool aa, dim3 grid, hipStream_t st, const SceneK& S, const RenderK& R,
                    void* out) {
    if (aa) lens_render<true>(f64, bvh, grid, st, S, R, out);
    else lens_render<false>(f64, bvh, grid, st, S, R, out);
}

template <bool AA>
static void lens_render_list(bool f64, bool bvh, dim3 grid, hipStream_t st, const SceneK& S, const ListK& R,
                             const uint32_t* list, double* accS, double* accQ, uint32_t* accN) {
    const dim3 block(kRenderBlock);
    hipLaunchKernelGGL(PT_KERNEL_F64_BVH(f64, bvh, k_render_list_lens, AA), grid, block, 0, st, S, R, list, accS,
                       accQ, accN);
}
void pt_lens_render_list(bool f64, bool bvh, bool aa, dim3 grid, hipStream_t st, const SceneK& S,
                         const ListK& R, const uint32_t* list, double* accS, double* accQ, uint32_t* accN) {
    if (aa) lens_render_list<true>(f64, bvh, grid, st, S, R, list, accS, accQ, accN);
    else lens_render_list<false>(f64, bvh, grid, st, S, R, list, accS, accQ, accN);
}
