// pt_lens_host.cpp — TEST INFRASTRUCTURE.  The thin-lens lane code (pt_path.h
// lens_point / lens_window / lens_dir, LensRay with either sink through
// render_loop) compiled for the host on top of pt_aa_host.cpp, so the CPU
// suite can check the rule of PT_FLAG_LENS (include/pt_capi.h) against its
// numpy restatement (tests/lens_ref.py) and the oracle without a GPU.  Built
// by tests/test_lens_host.py into a temporary directory by the hostcheck
// Makefile's pattern rule (tests/hostlib.py).
#include "pt_aa_host.cpp"

namespace {

// Whether two scenes have the same bytes in each of the frame records
// {unit, unit_eye, bunit, kd}
void same_records(const HostScene& A, const HostScene& B, int32_t* same) {
    auto eq = [](const auto& a, const auto& b) {
        return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0);
    };
    same[0] = eq(A.unit, B.unit);
    same[1] = eq(A.unit_eye, B.unit_eye);
    same[2] = eq(A.bunit, B.bunit);
    same[3] = eq(A.kd, B.kd);
}

// The filter self-test from origins of the caller's choice: n lines, line i
// from origin(i, rng, U) (its draws come before the line's other ones), tested
// against every unit with filter_eval.h's forms over unit_eye (and the BVH
// units), the directions aimed as hc_filter_selftest aims them.  out[0] =
// wrong certain verdicts against this build's eval64 (must be 0), out[1] =
// ambiguous verdicts, out[2] = tests.
template <class Origin>
void filter_from(const HostScene& H, int64_t n_rays, uint64_t seed, int64_t* out, Origin&& origin) {
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::normal_distribution<double> N(0.0, 1.0);
    const int nu = H.k.n_unit + H.k.n_bunit;
    const int kKinds = ptcheck::kKinds;
    std::vector<double> s_d(7), s_sqd((size_t)nu * 2);
    std::vector<float> s_f(2), s_atdt((size_t)nu * 4), s_sum((size_t)H.k.n_obj_unit * ptcheck::kSumN + 1);
    std::vector<int8_t> s_code((size_t)nu * 2 * kKinds), s_hit((size_t)nu * 2), s_mflag(nu);
    int32_t s_eye = 1;
    const ptcheck::FilterLines LC = {s_d.data(), s_d.data() + 3, s_d.data() + 6, s_f.data(), s_f.data() + 1, &s_eye};
    const ptcheck::FilterOut F = {s_code.data(), s_hit.data(), s_sqd.data(), s_atdt.data(), s_mflag.data(),
                                  s_sum.data()};
    int64_t wrong = 0, amb = 0, tests = 0;
    for (int64_t i = 0; i < n_rays; ++i) {
        const D3 o = origin(i, rng, U);
        D3 dir = d3(N(rng), N(rng), N(rng));
        if (i % 3 == 0) {   // aim near a random vertex
            const TriD& T = H.trid[rng() % H.trid.size()];
            dir = ld3(T.v1) + d3(N(rng), N(rng), N(rng)) * 1e-3 - o;
        } else if (i % 3 == 1) {   // aim at a point of a random edge, off by 1e-2 .. 1e-9
            const TriD& T = H.trid[rng() % H.trid.size()];
            const D3 vv[3] = {ld3(T.v1), ld3(T.v2), ld3(T.v3)};
            const int e = (int)(rng() % 3);
            const double a = U(rng), sc = pow(10.0, -2.0 - 7.0 * U(rng));
            dir = vv[e] + (vv[(e + 1) % 3] - vv[e]) * a + d3(N(rng), N(rng), N(rng)) * sc - o;
        }
        const D3 dn = unit(dir);
        const double lim = 0.5 + 40.0 * U(rng);
        s_d[0] = o.x; s_d[1] = o.y; s_d[2] = o.z;
        s_d[3] = dn.x; s_d[4] = dn.y; s_d[5] = dn.z;
        s_d[6] = lim;
        s_f[0] = (float)(sqrt(lim) * (1 - 1e-6));
        s_f[1] = (float)(sqrt(lim) * (1 + 1e-6));
        ptcheck::filter_line(H.k, LC, 0, F, true);
        for (int u = 0; u < nu; ++u) {
            const bool uni = u < H.k.n_unit;
            for (int m = 0; m < 2; ++m) {
                const int8_t* c = F.code + ((size_t)u * 2 + m) * kKinds;
                const bool h = F.hit[u * 2 + m] != 0;
                const double sqd = F.sqd[u * 2 + m];
                const bool ref_c = h && sqd > kZero;
                const bool ref_s = h && !(sqd < kZero) && sqd < lim;
                // (verdict kinds and their references as hc_filter_selftest's tally)
                const int kinds[6] = {ptcheck::kClosest, ptcheck::kShadow, ptcheck::kMarginF,
                                      ptcheck::kQuadShadow, ptcheck::kQuadClosest, ptcheck::kLean};
                const bool refs[6] = {ref_c, ref_s, ref_s, ref_s, ref_c, ref_c};
                for (int k = 0; k < 6; ++k) {
                    if (k >= 3 && !uni) continue;
                    const int st = c[kinds[k]];
                    if (st < 0) continue;   // no member triangle m
                    ++tests;
                    if (st == kAmb) ++amb;
                    else if ((st == kCand) != refs[k]) ++wrong;
                }
            }
        }
    }
    out[0] = wrong; out[1] = amb; out[2] = tests;
}

}  // namespace

extern "C" {

// out: jx, jy, lx, ly, r of sample `sample` of `pixel` (steps 1-3)
void hc_lens_point(uint64_t seed, uint32_t pixel, uint32_t sample, int32_t aa, double R, double* out) {
    if (aa) lens_point<true>(seed, pixel, sample, R, &out[0], &out[1], &out[2], &out[3]);
    else lens_point<false>(seed, pixel, sample, R, &out[0], &out[1], &out[2], &out[3]);
    uint32_t c[4];
    rng_block(seed, pixel, sample, 0xFFFFFFFFu, 0u, c);
    out[4] = R * sqrt_d(u_of(c[2]));
}

// The window (4 doubles), d0 (3) and eye' (3) of offsets (jx, jy, lx, ly) on
// the scene with lens L (steps 4-5).  -1: the scene or the lens is refused.
int hc_lens_dir(const pt_scene_desc* d, const pt_lens* L, int32_t W, int32_t H, int32_t ix, int32_t iy,
                double jx, double jy, double lx, double ly, double* ortho, double* d0, double* eye) {
    HostScene Hs;
    if (!open_scene(d, &Hs, L)) return -1;
    lens_window(Hs.k, W, H, jx, jy, lx, ly, ortho);
    eye[0] = Hs.kd[kKdEye] + lx; eye[1] = Hs.kd[kKdEye + 1] + ly; eye[2] = Hs.kd[kKdEye + 2];
    const D3 v = lens_dir(Hs.k, W, H, ix, iy, jx, jy, lx, ly, eye[0], eye[1]);
    d0[0] = v.x; d0[1] = v.y; d0[2] = v.z;
    return 0;
}

// prepare_scene's verdict on (scene, lens): 0 accepted, -1 refused
int hc_lens_check(const pt_scene_desc* d, const pt_lens* L) {
    HostScene Hs;
    return prepare_scene(d, &Hs, L).empty() ? 0 : -1;
}

// The frame records that must not depend on how a lens-free scene is made:
// out = {bytes of unit, unit_eye, bunit, kd}, and whether the scene made with
// lens L (may be null) has the same bytes in each as the scene made without
// (same[4]).  X[2]: the "all" frame's centre x and the eye-frame error bound
// eh of unit 0, of the scene made with L.
int hc_lens_records(const pt_scene_desc* d, const pt_lens* L, int64_t* out, int32_t* same, double* X) {
    HostScene A, B;
    if (!prepare_scene(d, &A).empty() || !prepare_scene(d, &B, L).empty()) return -1;
    out[0] = (int64_t)(A.unit.size() * sizeof(UnitF));
    out[1] = (int64_t)(A.unit_eye.size() * sizeof(UnitF));
    out[2] = (int64_t)(A.bunit.size() * sizeof(UnitF));
    out[3] = (int64_t)(A.kd.size() * sizeof(double));
    same_records(A, B, same);
    X[0] = B.k.center[0];
    X[1] = B.unit_eye.empty() ? 0.0 : (double)B.unit_eye[0].eh;
    return 0;
}

// hc_render_aa's frame through the lens: the lane code PT_FLAG_LENS selects
// (with PT_FLAG_AA in p->flags: the jitter as well), `lanes` emulated lanes per
// pixel reduced in store_pixel's xor order.  L null: the scene has no lens.
// Without PT_FLAG_LENS in p->flags the frame is hc_render_aa's (PT_FLAG_AA) or
// the centre-ray one, on the scene prepared with L — what a lens scene gives
// without the flag.
int hc_render_lens(const pt_scene_desc* d, const pt_lens* L, const pt_render_params* p, int force64,
                   int32_t lanes, double* sum, double* S, double* Q) {
    Host h;
    if (!h.open(d, L)) return -1;
    if (lanes < 1 || (lanes & (lanes - 1))) return -2;
    const bool lens = (p->flags & PT_FLAG_LENS) != 0, aa = (p->flags & PT_FLAG_AA) != 0;
    if (lens && !L) return -3;
    render_frame(h, p, lanes, sum, S, Q,
                 [&](int ix, int iy, auto&& f) { with_primary(h, p, force64 != 0, lens, aa, ix, iy, f); });
    return 0;
}

// hc_accum_aa through the lens: the accumulator's pass loop with the lens's
// samples (PT_FLAG_AA in p->flags: jittered as well), one lane per pixel.
int hc_accum_lens(const pt_scene_desc* d, const pt_lens* L, const pt_render_params* p, double tol,
                  double floor, uint32_t min_spp, uint32_t max_spp, uint32_t step_spp, double* S, double* Q,
                  uint32_t* n) {
    Host h;
    if (!L || !h.open(d, L)) return -1;
    const bool aa = (p->flags & PT_FLAG_AA) != 0;
    return accum_passes(h, p, AdaptK{tol, floor, min_spp, max_spp, step_spp}, S, Q, n,
                        [&](int ix, int iy, auto&& f) { with_primary(h, p, false, true, aa, ix, iy, f); });
}

// The filter self-test from the lens: n lines whose origins lie on the lens
// disc of the scene made with L — the centre, the four axis points of the rim,
// points of the rim, then uniform points of the disc — tested against every
// unit with filter_eval.h's forms over unit_eye (and the BVH units), the
// directions aimed as hc_filter_selftest aims them.  out[0] = wrong certain
// verdicts against this build's eval64 (must be 0), out[1] = ambiguous
// verdicts, out[2] = tests.
int hc_lens_filter(const pt_scene_desc* d, const pt_lens* L, int64_t n_rays, uint64_t seed, int64_t* out) {
    HostScene H;
    if (!L || !open_scene(d, &H, L)) return -1;
    const D3 eye = ld3(H.k.eye);
    const double R = L->radius;
    filter_from(H, n_rays, seed, out, [&](int64_t i, std::mt19937_64& rng, std::uniform_real_distribution<double>& U) {
        double lx = 0.0, ly = 0.0;
        if (i >= 1 && i <= 4) {   // the rim's axis points
            lx = i == 1 ? R : i == 2 ? -R : 0.0;
            ly = i == 3 ? R : i == 4 ? -R : 0.0;
        } else if (i > 4) {
            const double phi = 6.283185307179586 * U(rng), r = i % 2 ? R : R * sqrt(U(rng));
            lx = r * cos(phi);
            ly = r * sin(phi);
        }
        return d3(eye.x + lx, eye.y + ly, eye.z);
    });
    return 0;
}

}  // extern "C"
