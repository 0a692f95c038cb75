// pt_job.h — the launch records (RenderK, ListK, RaysK) and the mapping work-item ->
// job of a launch (slot_job, list_job, rays_job), without the HIP runtime: the kernels
// (pt_render.h) and the host checks (tests/hostcheck) compile the same text.
#pragma once
#include "pt_path.h"

using namespace pt;

struct RenderK {
    int32_t W, H, spp, bounces;
    uint64_t seed;
    int32_t rr_depth;   // -1: off
    int32_t first_row, row_step, n_rows;
    int32_t sample_begin;
    uint32_t split, split_log2;
    uint32_t npix;
    int32_t out_f64;
    uint32_t out_stride;   // elements between output rows (pt_render_params.out_row_stride)
    // single kernel, launch drain: the pixels from tail_pix on (the image's
    // top rows, dispatched last) get 2^tail_log2 lanes each, from lane
    // tail_lane (a multiple of 64) on; tail_pix = npix: none
    uint32_t tail_pix, tail_lane, tail_log2;
};

// Work-items per k_render block: one wave.  Nothing in the kernel is shared
// beyond a wave (a pixel's lanes reduce with shuffles), and the spill home
// is LDS allocated per block: with 4-wave blocks a wave's slot stayed idle
// until the block's slowest wave ended (its 40 KB held), with 1-wave blocks
// it is refilled as soon as the wave ends.
#ifndef PT_RENDER_BLOCK
#define PT_RENDER_BLOCK 64
#endif
constexpr uint32_t kRenderBlock = PT_RENDER_BLOCK;
// k_render's waves per SIMD: 4 (<= 128 VGPRs, a little scratch spill outside
// the triangle loops): 9.5 ms vs 10.8 ms at 3 waves and 15.3 ms at 2 on the
// 512^2 x 64spp bench (MI355X), see DESIGN.md §5.
#ifndef PT_RENDER_WAVES
#define PT_RENDER_WAVES 4
#endif

// ceil(log2(x)): the shift of a power-of-two lane count (RenderK / ListK split_log2)
inline uint32_t log2_ceil(uint32_t x) {
    uint32_t l = 0;
    while ((1u << l) < x) ++l;
    return l;
}

// Work-item -> (pixel, sample slice) of a launch: `split` adjacent work-items
// share a pixel and stride its samples; the primary ray of main.py:191
// (make_screen_pts / make_rays, utils.py:55-69).
struct SlotJob {
    LaneJob J;
    D3 d0;
    int32_t row_local, ix;
    uint32_t c;
    bool valid;
    int32_t iy;   // the pixel's image row (with ix: aa_dir's pixel, the antialiased shade step)
};
PT_HD SlotJob slot_job(const SceneK& S, const RenderK& R, uint32_t tid) {
    SlotJob j;
    const uint32_t pl = tid >> R.split_log2;
    j.c = tid & (R.split - 1u);
    j.valid = pl < R.npix;
    j.row_local = 0;
    j.ix = 0;
    j.iy = 0;
    j.d0 = d3(0, 0, 0);
    j.J = LaneJob{};
    if (j.valid) {
        j.row_local = (int32_t)(pl / (uint32_t)R.W);
        j.ix = (int32_t)pl - j.row_local * R.W;
        const int32_t iy = R.first_row + j.row_local * R.row_step;
        j.iy = iy;
        const D3 eye = ld3(S.eye);
        const double x = linspace_at(S.ortho[0], S.ortho[2], R.W, j.ix);
        const double y = linspace_at(S.ortho[1], S.ortho[3], R.H, iy);
        j.d0 = d3(x - eye.x, y - eye.y, 0.0 - eye.z);
        const int32_t c = (int32_t)j.c, sp = (int32_t)R.split;
        j.J.seed = R.seed;
        j.J.pixel = (uint32_t)j.ix * (uint32_t)R.H + (uint32_t)iy;
        j.J.sample0 = R.sample_begin + c;
        j.J.sample_stride = sp;
        j.J.n_samples = (c < R.spp) ? (R.spp - c + sp - 1) / sp : 0;
        j.J.bounces = R.bounces;
        j.J.rr_depth = R.rr_depth;
    }
    return j;
}

// An accumulator pass (pt_accum, pt_hip.hip "adaptive sampling"): the launch
// renders a LIST of pixels.
struct ListK {
    int32_t W, H, bounces, rr_depth;   // rr_depth -1: off
    uint64_t seed;
    uint32_t split, split_log2;
    uint32_t n_list, npix;
    uint64_t lanes;   // work-items of the launch (a multiple of 64): the moment home's stride
    AdaptK A;
};
// Work-item -> (list entry, sample slice) of a pass through the wavefront
// kernels, k_render_list's mapping: `split` adjacent slots share the entry's
// pixel e and stride the k = adapt_k(n[e]) samples the pass adds, from sample
// n[e] on.  An entry that is no pixel of the frame is never dereferenced.
struct ListJob {
    LaneJob J;
    D3 d0;
    uint32_t e, k;
    bool valid;
    int32_t ix, iy;   // the entry's pixel (aa_dir's, the antialiased shade step)
};
PT_HD ListJob list_job(const SceneK& S, const ListK& R, const uint32_t* __restrict__ list,
                       const uint32_t* __restrict__ accN, uint32_t tid) {
    ListJob j;
    const uint32_t entry = tid >> R.split_log2, c = tid & (R.split - 1u);
    j.e = entry < R.n_list ? list[entry] : 0xffffffffu;
    j.valid = j.e < R.npix;   // the same for all slots of an entry
    j.k = 0;
    j.ix = j.iy = 0;
    j.d0 = d3(0, 0, 0);
    j.J = LaneJob{};
    // (the launch's constants outside the branch: they stay wave-uniform, and
    // rng_block takes its key in scalar registers)
    j.J.seed = R.seed;
    j.J.sample_stride = (int32_t)R.split;
    j.J.bounces = R.bounces;
    j.J.rr_depth = R.rr_depth;
    if (j.valid) {
        const uint32_t n0 = accN[j.e];
        j.k = adapt_k(n0, R.A);
        const int32_t row = (int32_t)(j.e / (uint32_t)R.W);
        const int32_t ix = (int32_t)j.e - row * R.W, iy = R.H - 1 - row;
        j.ix = ix;
        j.iy = iy;
        const D3 eye = ld3(S.eye);
        const double x = linspace_at(S.ortho[0], S.ortho[2], R.W, ix);
        const double y = linspace_at(S.ortho[1], S.ortho[3], R.H, iy);
        j.d0 = d3(x - eye.x, y - eye.y, 0.0 - eye.z);
        j.J.pixel = (uint32_t)ix * (uint32_t)R.H + (uint32_t)iy;
        j.J.sample0 = (int32_t)(n0 + c);
        j.J.n_samples = c < j.k ? (int32_t)((j.k - c + R.split - 1u) >> R.split_log2) : 0;
    }
    return j;
}

// pt_radiance's launch (include/pt_capi.h): n_rays records, `split` adjacent
// work-items each
struct RaysK {
    int32_t spp, bounces;
    uint64_t seed;
    int32_t rr_depth;   // -1: off
    int32_t sample_begin;
    uint32_t split, split_log2;
    uint32_t n_rays;
    int32_t out_f64;
    double frame_x;   // rays_in_frame's extent (HostScene::frame_x)
};
// Work-item -> (record, sample slice) of a ray launch through the wavefront
// kernels, k_render_rays' mapping (pt_rays.hip): `split` adjacent slots share
// record `entry` and stride its spp samples from sample_begin on; the Philox
// pixel word is the record's key.  There is no pixel: the primary ray, and the
// eye wherever a sample reads it, are the record's.  A record past the batch
// is never dereferenced (ray stays null).
struct RayJob {
    LaneJob J;
    const RayK* ray;
    bool valid;
};
PT_HD RayJob rays_job(const RaysK& R, const RayK* __restrict__ rays, uint32_t tid) {
    RayJob j;
    const uint32_t entry = tid >> R.split_log2;
    const int32_t c = (int32_t)(tid & (R.split - 1u)), sp = (int32_t)R.split;
    j.valid = entry < R.n_rays;
    j.ray = nullptr;
    j.J = LaneJob{};
    // (the launch's constants outside the branch, as list_job keeps them)
    j.J.seed = R.seed;
    j.J.sample_stride = sp;
    j.J.bounces = R.bounces;
    j.J.rr_depth = R.rr_depth;
    if (j.valid) {
        j.ray = rays + entry;
        j.J.pixel = j.ray->key;
        j.J.sample0 = R.sample_begin + c;
        j.J.n_samples = (c < R.spp) ? (R.spp - c + sp - 1) / sp : 0;
    }
    return j;
}

// A pass of a ray accumulator (pt_accum_create_rays, include/pt_capi.h): the
// launch renders a LIST of ray records; element e of the accumulator belongs
// to record e.
struct RaysListK {
    int32_t bounces, rr_depth;   // rr_depth -1: off
    uint64_t seed;
    uint32_t split, split_log2;
    uint32_t n_list, n_rays;
    double frame_x;   // rays_in_frame's extent (HostScene::frame_x)
    AdaptK A;
};
// Work-item -> (list entry, sample slice) of such a pass, k_render_rays_list's
// mapping (pt_rays_list.hip): list_job's with the record rays[e] in the place
// of pixel e's primary ray — `split` adjacent work-items share the entry's
// record and stride the k = adapt_k(n[e]) samples the pass adds, from sample
// n[e] on; the Philox pixel word is the record's key.  An entry that is no
// record of the accumulator is never dereferenced (ray stays null).
struct RayListJob {
    LaneJob J;
    const RayK* ray;
    uint32_t e, k;
    bool valid;
};
PT_HD RayListJob rays_list_job(const RaysListK& R, const RayK* __restrict__ rays,
                               const uint32_t* __restrict__ list, const uint32_t* __restrict__ accN,
                               uint32_t tid) {
    RayListJob j;
    const uint32_t entry = tid >> R.split_log2, c = tid & (R.split - 1u);
    j.e = entry < R.n_list ? list[entry] : 0xffffffffu;
    j.valid = j.e < R.n_rays;   // the same for all lanes of an entry
    j.k = 0;
    j.ray = nullptr;
    j.J = LaneJob{};
    // (the launch's constants outside the branch, as list_job keeps them)
    j.J.seed = R.seed;
    j.J.sample_stride = (int32_t)R.split;
    j.J.bounces = R.bounces;
    j.J.rr_depth = R.rr_depth;
    if (j.valid) {
        const uint32_t n0 = accN[j.e];
        j.k = adapt_k(n0, R.A);
        j.ray = rays + j.e;
        j.J.pixel = j.ray->key;
        j.J.sample0 = (int32_t)(n0 + c);
        j.J.n_samples = c < j.k ? (int32_t)((j.k - c + R.split - 1u) >> R.split_log2) : 0;
    }
    return j;
}
