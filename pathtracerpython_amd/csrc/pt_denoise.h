// pt_denoise.h — the edge-avoiding filter of an adaptive render (build
// extension): an a-trous wavelet filter (after Dammertz et al.
// 2010, "Edge-avoiding a-trous wavelet transform for fast global illumination
// filtering") whose luminance stop is driven by the per-pixel variance of the
// mean (as in Schied et al. 2017, SVGF) and whose geometry stops use the
// first hit of the pixel's primary ray.  The rule is stated in
// include/pt_capi.h (pt_denoise_params); every operation is f64, rounded on
// its own (-ffp-contract=off), in the order written there, with IEEE division
// and sqrt: the tests restate it in numpy and compare bits.
//
// dn_moments and dn_pixel are PT_HD functions over plain pointers: the host
// test build (tests/denoise_host) runs the same code.  The kernels and
// k_features (which needs closest(), pt_path.h) are device-only.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include "pt_path.h"   // closest(), for k_features
#endif
#ifndef PT_HD
#define PT_HD __host__ __device__ __forceinline__
#endif

namespace pt {

struct DenoiseK {
    double sigma_l, sigma_z, eps;
    int32_t normal_sq, pad;
};

// Rec. 709 luminance weights A and their squares B (f64 products)
constexpr double kDnA0 = 0.2126, kDnA1 = 0.7152, kDnA2 = 0.0722;
constexpr double kDnB0 = kDnA0 * kDnA0, kDnB1 = kDnA1 * kDnA1, kDnB2 = kDnA2 * kDnA2;

// max(0, x) as a select: a NaN gives 0
PT_HD double dn_pos(double x) { return x > 0.0 ? x : 0.0; }
PT_HD double dn_h5(int d) { return d == 0 ? 0.375 : ((d == 1 || d == -1) ? 0.25 : 0.0625); }
PT_HD double dn_g3(int d) { return d == 0 ? 0.5 : 0.25; }
PT_HD double dn_lum(const double* c) { return (kDnA0 * c[0] + kDnA1 * c[1]) + kDnA2 * c[2]; }
PT_HD double dn_vlum(const double* v) { return (kDnB0 * v[0] + kDnB1 * v[1]) + kDnB2 * v[2]; }

// Colour c[3] and variance of the mean v[3] of a pixel from its moments.
PT_HD void dn_moments(const double* S, const double* Q, uint32_t n, double* c, double* v) {
    if (n >= 2u) {
        const double dn = (double)n, d1 = (double)(n - 1u);
        for (int k = 0; k < 3; ++k) {
            c[k] = S[k] / dn;
            v[k] = (dn_pos(Q[k] - S[k] * S[k] / dn) / d1) / dn;
        }
    } else if (n == 1u) {   // variance unknown: lean on the neighbours
        for (int k = 0; k < 3; ++k) {
            c[k] = S[k];
            v[k] = S[k] * S[k];
        }
    } else {
        for (int k = 0; k < 3; ++k) c[k] = v[k] = 0.0;
    }
}

// One iteration at pixel (row, col) of a W x H frame, stride s: reads
// c, v [H*W][3], obj [H*W], N, P [H*W][3]; writes co[3], vo[3].  Every index
// it forms is a pixel of the frame: the 3 x 3 of the variance prefilter is
// clamped, the 5 x 5 taps outside the frame are skipped.
PT_HD void dn_pixel(int32_t W, int32_t H, int32_t row, int32_t col, int32_t s, const DenoiseK& K,
                    const double* __restrict__ c, const double* __restrict__ v,
                    const int32_t* __restrict__ obj, const double* __restrict__ N,
                    const double* __restrict__ P, double* co, double* vo) {
    const size_t p = (size_t)row * (size_t)W + (size_t)col;
    double vf = 0.0;
    for (int dy = -1; dy <= 1; ++dy) {
        const int32_t r = row + dy < 0 ? 0 : (row + dy > H - 1 ? H - 1 : row + dy);
        for (int dx = -1; dx <= 1; ++dx) {
            const int32_t cc = col + dx < 0 ? 0 : (col + dx > W - 1 ? W - 1 : col + dx);
            vf += (dn_g3(dy) * dn_g3(dx)) * dn_vlum(v + 3 * ((size_t)r * (size_t)W + (size_t)cc));
        }
    }
    const double dl = K.sigma_l * sqrt(vf) + K.eps;
    const double lp = dn_lum(c + 3 * p);
    const int32_t op = obj[p];
    const double Np0 = N[3 * p], Np1 = N[3 * p + 1], Np2 = N[3 * p + 2];
    const double Pp0 = P[3 * p], Pp1 = P[3 * p + 1], Pp2 = P[3 * p + 2];
    double num0 = 0.0, num1 = 0.0, num2 = 0.0, vn0 = 0.0, vn1 = 0.0, vn2 = 0.0, den = 0.0;
    for (int dy = -2; dy <= 2; ++dy) {
        // (64-bit: dy * s reaches 2 * 128 rows past a frame of any height)
        const int64_t r = (int64_t)row + (int64_t)dy * s;
        if (r < 0 || r >= (int64_t)H) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const int64_t cc = (int64_t)col + (int64_t)dx * s;
            if (cc < 0 || cc >= (int64_t)W) continue;
            const size_t q = (size_t)r * (size_t)W + (size_t)cc;
            if (obj[q] != op) continue;
            double w = dn_h5(dy) * dn_h5(dx);
            if (op >= 0) {
                const double* Nq = N + 3 * q;
                const double* Pq = P + 3 * q;
                double nd = dn_pos((Np0 * Nq[0] + Np1 * Nq[1]) + Np2 * Nq[2]);
                for (int j = 0; j < K.normal_sq; ++j) nd = nd * nd;
                const double D0 = Pq[0] - Pp0, D1 = Pq[1] - Pp1, D2 = Pq[2] - Pp2;
                const double dist = sqrt((D0 * D0 + D1 * D1) + D2 * D2);
                const double pd = fabs((Np0 * D0 + Np1 * D1) + Np2 * D2);
                const double xz = dist > 0.0 ? pd / (dist * K.sigma_z) : 0.0;
                double wz = dn_pos(1.0 - xz);
                wz = wz * wz;
                w = (w * nd) * wz;
            }
            const double* cq = c + 3 * q;
            const double* vq = v + 3 * q;
            const double xl = fabs(dn_lum(cq) - lp) / dl;
            w = w * (1.0 / ((1.0 + xl) + 0.5 * (xl * xl)));
            const double ww = w * w;
            num0 += w * cq[0]; num1 += w * cq[1]; num2 += w * cq[2];
            vn0 += ww * vq[0]; vn1 += ww * vq[1]; vn2 += ww * vq[2];
            den += w;
        }
    }
    const double dd = den * den;   // the centre tap makes den > 0
    co[0] = num0 / den; co[1] = num1 / den; co[2] = num2 / den;
    vo[0] = vn0 / dd; vo[1] = vn1 / dd; vo[2] = vn2 / dd;
}

#if defined(__HIPCC__)
constexpr uint32_t kDnBlock = 256;

// S, Q, n -> c, v
__global__ __launch_bounds__(kDnBlock) void k_accum_moments(const double* __restrict__ accS,
                                                            const double* __restrict__ accQ,
                                                            const uint32_t* __restrict__ accN, uint32_t npix,
                                                            double* __restrict__ c, double* __restrict__ v) {
    const uint64_t e = (uint64_t)blockIdx.x * kDnBlock + threadIdx.x;
    if (e >= (uint64_t)npix) return;
    dn_moments(accS + e * 3, accQ + e * 3, accN[e], c + e * 3, v + e * 3);
}

// One iteration: a work-item per pixel e = row * W + col, a block per 256
// pixels of a row-major run, direct global loads (src and dst never alias: the
// caller's ping-pong).  (16 x 16 tiles per block measured 1.7-1.9x slower at
// 4096^2: 384-B row pieces instead of whole lines)
__global__ __launch_bounds__(kDnBlock) void k_denoise_iter(int32_t W, int32_t H, uint32_t npix, int32_t s,
                                                           DenoiseK K, const double* __restrict__ c,
                                                           const double* __restrict__ v,
                                                           const int32_t* __restrict__ obj,
                                                           const double* __restrict__ N,
                                                           const double* __restrict__ P,
                                                           double* __restrict__ co, double* __restrict__ vo) {
    const uint64_t e = (uint64_t)blockIdx.x * kDnBlock + threadIdx.x;
    if (e >= (uint64_t)npix) return;
    const int32_t row = (int32_t)(e / (uint32_t)W), col = (int32_t)(e - (uint64_t)row * (uint32_t)W);
    double a[3], b[3];
    dn_pixel(W, H, row, col, s, K, c, v, obj, N, P, a, b);
    for (int k = 0; k < 3; ++k) {
        co[e * 3 + k] = a[k];
        vo[e * 3 + k] = b[k];
    }
}

// The filtered frame and (optionally) its variance as f32 or f64
template <typename T>
__global__ __launch_bounds__(kDnBlock) void k_denoise_store(const double* __restrict__ c,
                                                            const double* __restrict__ v, uint64_t n3,
                                                            T* __restrict__ out, T* __restrict__ out_var) {
    const uint64_t i = (uint64_t)blockIdx.x * kDnBlock + threadIdx.x;
    if (i >= n3) return;
    out[i] = (T)c[i];
    if (out_var) out_var[i] = (T)v[i];
}

// First-hit features: the primary ray of pixel e as k_render_list builds it,
// closest() from the eye frame (uniform units, then the BVH — the ordered
// walk, or the stackless pass for a tree deeper than its stack).
template <bool BVH>
__global__ __launch_bounds__(256) void k_features(SceneK S, int32_t W, int32_t H, uint32_t npix,
                                                  int32_t* __restrict__ tri, int32_t* __restrict__ obj,
                                                  double* __restrict__ N, double* __restrict__ P) {
    __shared__ double spill[kSpillSlots][256];
    const Spill sp{&spill[0][threadIdx.x], 256};
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= (uint64_t)npix) return;
    const int32_t row = (int32_t)(e / (uint32_t)W);
    const int32_t ix = (int32_t)(e - (uint64_t)row * (uint32_t)W), iy = H - 1 - row;
    const D3 eye = ld3(S.eye);
    const double x = linspace_at(S.ortho[0], S.ortho[2], W, ix);
    const double y = linspace_at(S.ortho[1], S.ortho[3], H, iy);
    const D3 d0 = d3(x - eye.x, y - eye.y, 0.0 - eye.z);
    Counters cnt = {};
    D3 P0 = d3(0, 0, 0);
    const int t = closest<false, false, BVH>(S, eye, d0, -1, sp, &P0, &cnt, true);
    const bool hit = t >= 0 && t < S.n_tri;   // (never indexes the tables with anything else)
    tri[e] = hit ? t : -1;
    obj[e] = hit ? S.tri_obj[t] : -1;
    for (int k = 0; k < 3; ++k) N[e * 3 + k] = hit ? S.tris[t].n[k] : 0.0;
    P[e * 3] = hit ? P0.x : 0.0;
    P[e * 3 + 1] = hit ? P0.y : 0.0;
    P[e * 3 + 2] = hit ? P0.z : 0.0;
}
#endif  // __HIPCC__

}  // namespace pt
