// pt_rays.h — the launch record and the launcher of the ray kernel
// (pt_rays.hip): the k_render_rays instantiation for a forced-f64 launch, a
// scene with a BVH, or neither, with or without the moments S, Q, on
// grid x kRenderBlock work-items.
#pragma once
#include "pt_render.h"

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

void pt_rays_render(bool f64, bool bvh, dim3 grid, hipStream_t st, const SceneK& S, const RaysK& R,
                    const RayK* rays, void* out, double* outS, double* outQ);
