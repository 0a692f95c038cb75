// pt_lens.h — the launchers of the thin-lens kernels (pt_lens.hip): the
// k_render_lens / k_render_list_lens instantiation for a forced-f64 launch, a
// scene with a BVH, or neither, with or without PT_FLAG_AA beside PT_FLAG_LENS
// (aa: the jitter of the same Philox block), on grid x kRenderBlock work-items.
#pragma once
#include "pt_render.h"

void pt_lens_render(bool f64, bool bvh, bool aa, dim3 grid, hipStream_t st, const SceneK& S, const RenderK& R,
                    void* out);
void pt_lens_render_list(bool f64, bool bvh, bool aa, dim3 grid, hipStream_t st, const SceneK& S,
                         const ListK& R, const uint32_t* list, double* accS, double* accQ, uint32_t* accN);
