// pt_material_host.cpp — TEST INFRASTRUCTURE.  The material part of the lane
// code on the host: which exponents prepare_scene sends to pow_ref's multiply
// loop (Mat::nint, pt_prepare.h) and what pow_ref (pt_core.h) returns, on top
// of pt_accum_host.cpp (and so pt_hostcheck.cpp), so that one library serves
// tests/test_materials_host.py.  Built by that test into a temporary
// directory by the hostcheck Makefile's pattern rule (tests/hostlib.py).
#include "pt_accum_host.cpp"

extern "C" {

// nint[n_obj]: Mat::nint of every object (-1: the general pow).
int hc_mat_nint(const pt_scene_desc* d, int32_t* nint) {
    HostScene H;
    if (!prepare_scene(d, &H).empty()) return -1;
    for (int o = 0; o < d->n_obj; ++o) nint[o] = H.mat[o].nint;
    return 0;
}

// out[i] = pow_ref(x[i], material of object obj).
int hc_pow_ref(const pt_scene_desc* d, int32_t obj, const double* x, int64_t n, double* out) {
    HostScene H;
    if (!prepare_scene(d, &H).empty()) return -1;
    if (obj < 0 || obj >= d->n_obj) return -2;
    for (int64_t i = 0; i < n; ++i) out[i] = pow_ref(x[i], H.mat[obj]);
    return 0;
}

}  // extern "C"
