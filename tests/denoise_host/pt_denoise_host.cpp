// pt_denoise_host.cpp — TEST INFRASTRUCTURE.  The denoiser's per-pixel code
// (pt_denoise.h dn_moments / dn_pixel) compiled for the host, so the CPU suite
// can compare it with the numpy restatement (tests/denoise_ref.py) bit for bit
// without a GPU, and the sanitizer program (denoise_san_main.cpp) can drive
// its border addressing.  Built by tests/test_denoise_host.py with this
// directory's Makefile (g++ -O2 -ffp-contract=off, as the device build).
#define __host__
#define __device__
#define __forceinline__ inline
#include <cstddef>
#include <stdint.h>

#include <vector>

#include "../../include/pt_capi.h"
#include "../../pathtracerpython_amd/csrc/pt_denoise.h"

using namespace pt;

extern "C" {

// The filter on host arrays: c, v, N, P [H*W][3], obj [H*W]; out_c, out_v
// [H*W][3].  Returns 0, or -1 for parameters outside the header's ranges.
int hd_denoise(int32_t W, int32_t H, const pt_denoise_params* d, const double* c, const double* v,
               const int32_t* obj, const double* N, const double* P, double* out_c, double* out_v) {
    if (W <= 0 || H <= 0 || !d || d->iters < 1 || d->iters > 8 || d->normal_sq < 0 || d->normal_sq > 8 ||
        !(d->sigma_l > 0.0) || !(d->sigma_z > 0.0) || !(d->eps > 0.0) || d->reserved != 0)
        return -1;
    const DenoiseK K{d->sigma_l, d->sigma_z, d->eps, d->normal_sq, 0};
    const size_t n3 = (size_t)W * (size_t)H * 3;
    // exactly-sized frames: an index outside the frame is outside the allocation
    std::vector<double> ca(c, c + n3), va(v, v + n3), cb(n3), vb(n3);
    for (int32_t i = 0; i < d->iters; ++i) {
        for (int32_t row = 0; row < H; ++row)
            for (int32_t col = 0; col < W; ++col) {
                const size_t e = (size_t)row * (size_t)W + (size_t)col;
                dn_pixel(W, H, row, col, (int32_t)1 << i, K, ca.data(), va.data(), obj, N, P, &cb[3 * e],
                         &vb[3 * e]);
            }
        ca.swap(cb);
        va.swap(vb);
    }
    for (size_t i = 0; i < n3; ++i) {
        out_c[i] = ca[i];
        out_v[i] = va[i];
    }
    return 0;
}

void hd_moments(const double* S, const double* Q, const uint32_t* n, int64_t npix, double* c, double* v) {
    for (int64_t e = 0; e < npix; ++e) dn_moments(S + 3 * e, Q + 3 * e, n[e], c + 3 * e, v + 3 * e);
}

// the compiler's layout of pt_denoise_params
void hd_abi_layout(int64_t* out) {
    out[0] = (int64_t)sizeof(pt_denoise_params);
    out[1] = (int64_t)offsetof(pt_denoise_params, sigma_l);
    out[2] = (int64_t)offsetof(pt_denoise_params, sigma_z);
    out[3] = (int64_t)offsetof(pt_denoise_params, eps);
    out[4] = (int64_t)offsetof(pt_denoise_params, iters);
    out[5] = (int64_t)offsetof(pt_denoise_params, normal_sq);
    out[6] = (int64_t)offsetof(pt_denoise_params, reserved);
}

}  // extern "C"
