// pt_rays.h — the launch record and the launcher of the ray kernel
// (pt_rays.hip): the k_render_rays instantiation for a forced-f64 launch, a
// scene with a BVH, or neither, with or without the moments S, Q, on
// grid x kRenderBlock work-items.
#pragma once
#include "pt_render.h"

// (the launch record RaysK: pt_job.h, beside RenderK and ListK)
void pt_rays_render(bool f64, bool bvh, dim3 grid, hipStream_t st, const SceneK& S, const RaysK& R,
                    const RayK* rays, void* out, double* outS, double* outQ);
