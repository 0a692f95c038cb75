// pt_rays_list.h — the launchers of a ray accumulator's kernels
// (pt_rays_list.hip): the list pass k_render_rays_list for a forced-f64
// launch, a scene with a BVH, or neither, on grid x kRenderBlock work-items,
// and the records' first-hit features k_features_rays on ceil(n / 256) blocks
// of 256.
#pragma once
#include "pt_render.h"

// (the launch record RaysListK and the mapping rays_list_job: pt_job.h)
void pt_rays_render_list(bool f64, bool bvh, dim3 grid, hipStream_t st, const SceneK& S, const RaysListK& R,
                         const RayK* rays, const uint32_t* list, double* accS, double* accQ, uint32_t* accN);
void pt_rays_features(bool bvh, hipStream_t st, const SceneK& S, double frame_x, const RayK* rays, uint32_t n,
                      int32_t* tri, int32_t* obj, double* N, double* P);
