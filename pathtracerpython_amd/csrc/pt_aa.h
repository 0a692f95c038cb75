// pt_aa.h — the launchers of the antialiasing kernels (pt_aa.hip): the
// k_render_aa / k_render_list_aa instantiation for a forced-f64 launch, a
// scene with a BVH, or neither, on grid x kRenderBlock work-items.
#pragma once
#include "pt_render.h"

void pt_aa_render(bool f64, bool bvh, dim3 grid, hipStream_t st, const SceneK& S, const RenderK& R, void* out);
void pt_aa_render_list(bool f64, bool bvh, dim3 grid, hipStream_t st, const SceneK& S, const ListK& R,
                       const uint32_t* list, double* accS, double* accQ, uint32_t* accN);
