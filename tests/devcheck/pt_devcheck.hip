// pt_devcheck.hip — TEST INFRASTRUCTURE.  The product headers' device-only
// code (everything behind `#if defined(__HIP_DEVICE_COMPILE__)`: v_rcp_f32,
// the v_rcp_f64 / v_rsq_f64 Newton forms, sincos_small, v_minimum3_f32,
// v_max_f32, v_med3_f32, the canonicalise, shadow_unit_m's reordered del and
// wave vote) compiled for gfx950 with the library's own flags and run as
// small kernels over arrays of cases, so the GPU test suite can check the
// arithmetic the GPU executes — the host check (tests/hostcheck) compiles the
// host twins of all of it instead.  Never used by the product.
//
// Every entry point allocates, launches one kernel (one thread per case,
// 64-thread blocks), copies back and frees; it returns 0 or the HIP error as
// a negative number (-1000: a bad argument or scene).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../pathtracerpython_amd/csrc/pt_path.h"
#include "../../pathtracerpython_amd/csrc/pt_prepare.h"
#include "filter_eval.h"

using namespace pt;

namespace {

constexpr int kBlock = 64;
constexpr int kBadArg = -1000;

// device buffers of one call, freed on every way out
struct Bufs {
    std::vector<void*> p;
    hipError_t err = hipSuccess;
    ~Bufs() {
        for (void* q : p) (void)hipFree(q);
    }
    template <class T>
    T* alloc(size_t n) {   // (at least one element: an empty table is never read)
        void* q = nullptr;
        if (err == hipSuccess) err = hipMalloc(&q, (n ? n : 1) * sizeof(T));
        if (err != hipSuccess) return nullptr;
        p.push_back(q);
        return (T*)q;
    }
    template <class T>
    T* upload(const T* h, size_t n) {
        T* q = alloc<T>(n);
        if (q && n && err == hipSuccess) err = hipMemcpy(q, h, n * sizeof(T), hipMemcpyHostToDevice);
        return q;
    }
    template <class T>
    void download(T* h, const T* d, size_t n) {
        if (err == hipSuccess && n) err = hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost);
    }
    void launched() {
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
    }
    int rc() const { return err == hipSuccess ? 0 : -(int)err; }
};
unsigned blocks(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// rcp_d with ONE Newton step: the deliberately weak twin the ulp test must
// reject (a test of the test; the product's rcp_d takes two)
__device__ double rcp_d_weak(double x) {
    double y = __builtin_amdgcn_rcp(x);
    const double e = fma(-x, y, 1.0);
    return fma(y, e, y);
}

__global__ void __launch_bounds__(kBlock) k_math_f64(const double* x, int64_t n, double* out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double s, c;
    sincos_small(x[i], &s, &c);
    double* o = out + 5 * i;
    o[0] = rcp_d(x[i]);
    o[1] = rsqrt_d(x[i]);
    o[2] = sqrt_d(x[i]);
    o[3] = s;
    o[4] = c;
}
// unit_any (pt_path.h: the ray form's reflection of a caller's direction) and
// unit of v[i]
__global__ void __launch_bounds__(kBlock) k_unit_any(const double* v, int64_t n, double* out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const D3 a = d3(v[3 * i], v[3 * i + 1], v[3 * i + 2]);
    const D3 r = unit_any(a), u = unit(a);
    double* o = out + 6 * i;
    o[0] = r.x; o[1] = r.y; o[2] = r.z;
    o[3] = u.x; o[4] = u.y; o[5] = u.z;
}
__global__ void __launch_bounds__(kBlock) k_rcp_weak(const double* x, int64_t n, double* out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = rcp_d_weak(x[i]);
}
__global__ void __launch_bounds__(kBlock) k_rcpf(const float* x, int64_t n, float* out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = rcpf(x[i]);
}
__global__ void __launch_bounds__(kBlock) k_minmax(const float* a, const float* b, const float* c,
                                                   int64_t n, uint32_t* out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float r[6] = {nan_min(a[i], b[i]), nan_min3(a[i], b[i], c[i]), fmax_q(a[i], b[i]),
                        min3f(a[i], b[i], c[i]), med3_q(a[i], b[i], c[i]), pt_canon(a[i])};
    for (int k = 0; k < 6; ++k) out[6 * i + k] = __float_as_uint(r[k]);
}
// every lane of every wave runs a line (shadow_unit_m votes across the wave):
// the lanes past n repeat line n - 1 and write nothing
__global__ void __launch_bounds__(kBlock) k_filter(SceneK S, ptcheck::FilterLines L,
                                                   ptcheck::FilterOut F, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool write = i < n;
    if (!write) i = n - 1;
    ptcheck::filter_line(S, L, i, F, write);
}

}  // namespace

extern "C" {

// out[i][5] = rcp_d, rsqrt_d, sqrt_d, sincos_small's sin and cos of x[i]
int dc_math_f64(const double* x, int64_t n, double* out) {
    if (!x || !out || n < 1) return kBadArg;
    Bufs B;
    double* dx = B.upload(x, (size_t)n);
    double* dout = B.alloc<double>((size_t)n * 5);
    if (B.err == hipSuccess) {
        k_math_f64<<<blocks(n), kBlock>>>(dx, n, dout);
        B.launched();
    }
    B.download(out, dout, (size_t)n * 5);
    return B.rc();
}

// out[i][6] = unit_any(v[i]), unit(v[i])
int dc_unit_any(const double* v, int64_t n, double* out) {
    if (!v || !out || n < 1) return kBadArg;
    Bufs B;
    double* dv = B.upload(v, (size_t)n * 3);
    double* dout = B.alloc<double>((size_t)n * 6);
    if (B.err == hipSuccess) {
        k_unit_any<<<blocks(n), kBlock>>>(dv, n, dout);
        B.launched();
    }
    B.download(out, dout, (size_t)n * 6);
    return B.rc();
}

// out[i] = the one-step reciprocal (the weak twin)
int dc_rcp_weak(const double* x, int64_t n, double* out) {
    if (!x || !out || n < 1) return kBadArg;
    Bufs B;
    double* dx = B.upload(x, (size_t)n);
    double* dout = B.alloc<double>((size_t)n);
    if (B.err == hipSuccess) {
        k_rcp_weak<<<blocks(n), kBlock>>>(dx, n, dout);
        B.launched();
    }
    B.download(out, dout, (size_t)n);
    return B.rc();
}

// out[i] = rcpf(x[i])
int dc_rcpf(const float* x, int64_t n, float* out) {
    if (!x || !out || n < 1) return kBadArg;
    Bufs B;
    float* dx = B.upload(x, (size_t)n);
    float* dout = B.alloc<float>((size_t)n);
    if (B.err == hipSuccess) {
        k_rcpf<<<blocks(n), kBlock>>>(dx, n, dout);
        B.launched();
    }
    B.download(out, dout, (size_t)n);
    return B.rc();
}

// out[i][6] = the bits of nan_min(a,b), nan_min3(a,b,c), fmax_q(a,b),
// min3f(a,b,c), med3_q(a,b,c), pt_canon(a) (hostcheck's hc_minmax: the twins)
int dc_minmax(const float* a, const float* b, const float* c, int64_t n, uint32_t* out) {
    if (!a || !b || !c || !out || n < 1) return kBadArg;
    Bufs B;
    float* da = B.upload(a, (size_t)n);
    float* db = B.upload(b, (size_t)n);
    float* dc = B.upload(c, (size_t)n);
    uint32_t* dout = B.alloc<uint32_t>((size_t)n * 6);
    if (B.err == hipSuccess) {
        k_minmax<<<blocks(n), kBlock>>>(da, db, dc, n, dout);
        B.launched();
    }
    B.download(out, dout, (size_t)n * 6);
    return B.rc();
}

// The device twin of hostcheck's filter self-test: the n lines of
// hc_filter_cases against every uniform and BVH unit of the scene, results in
// hc_filter_cases' layout (filter_eval.h).
int dc_filter(const pt_scene_desc* d, int64_t n, const double* o, const double* dn, const double* lim,
              const float* hlo, const float* hhi, const int32_t* at_eye, int8_t* code, int8_t* hit,
              double* sqd, float* atdt, int8_t* mflag, float* sum) {
    if (!d || n < 1) return kBadArg;
    HostScene H;
    if (!prepare_scene(d, &H).empty()) return kBadArg;
    Bufs B;
    SceneK S = H.k;   // the tables filter_line reads; the others stay null
    S.unit = B.upload(H.unit.data(), H.unit.size());
    S.unit_eye = B.upload(H.unit_eye.data(), H.unit_eye.size());
    S.bunit = B.upload(H.bunit.data(), H.bunit.size());
    const UnitC* uc = B.upload(H.bunitc.data(), H.bunitc.size());
    S.bunitc = H.bunitc.empty() ? nullptr : uc;
    S.trid = B.upload(H.trid.data(), H.trid.size());
    S.tri_obj = B.upload(H.tri_obj.data(), H.tri_obj.size());
    S.kd = B.upload(H.kd.data(), H.kd.size());
    S.tris = nullptr; S.mat = nullptr; S.light_tri = nullptr; S.light_cum = nullptr;
    S.tri_grp = nullptr; S.bnode = nullptr; S.cnode = nullptr; S.qnode = nullptr;
    const size_t nu = (size_t)S.n_unit + S.n_bunit, lu = (size_t)n * nu;
    const size_t n_sum = (size_t)n * S.n_obj_unit * ptcheck::kSumN;
    ptcheck::FilterLines L;
    L.o = B.upload(o, (size_t)n * 3);
    L.dn = B.upload(dn, (size_t)n * 3);
    L.lim = B.upload(lim, (size_t)n);
    L.hlo = B.upload(hlo, (size_t)n);
    L.hhi = B.upload(hhi, (size_t)n);
    L.at_eye = B.upload(at_eye, (size_t)n);
    ptcheck::FilterOut F;
    F.code = B.alloc<int8_t>(lu * 2 * ptcheck::kKinds);
    F.hit = B.alloc<int8_t>(lu * 2);
    F.sqd = B.alloc<double>(lu * 2);
    F.atdt = B.alloc<float>(lu * 4);
    F.mflag = B.alloc<int8_t>(lu);
    F.sum = B.alloc<float>(n_sum);
    if (B.err == hipSuccess) {
        k_filter<<<blocks(n), kBlock>>>(S, L, F, n);
        B.launched();
    }
    B.download(code, F.code, lu * 2 * ptcheck::kKinds);
    B.download(hit, F.hit, lu * 2);
    B.download(sqd, F.sqd, lu * 2);
    B.download(atdt, F.atdt, lu * 4);
    B.download(mflag, F.mflag, lu);
    B.download(sum, F.sum, n_sum);
    return B.rc();
}

}  // extern "C"
