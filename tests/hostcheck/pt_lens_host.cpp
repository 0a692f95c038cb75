// pt_lens_host.cpp — TEST INFRASTRUCTURE.  The thin-lens lane code (pt_path.h
// lens_point / lens_window / lens_dir, LensRay with either sink through
// render_loop) compiled for the host on top of pt_aa_host.cpp, so the CPU
// suite can check the rule of PT_FLAG_LENS (include/pt_capi.h) against its
// numpy restatement (tests/lens_ref.py) and the oracle without a GPU.  Built
// by tests/test_lens_host.py into a temporary directory with the hostcheck
// Makefile's g++ flags.
#include "pt_aa_host.cpp"

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
    if (!prepare_scene(d, &Hs, L).empty()) return -1;
    bind_host(&Hs);
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
    auto eq = [](const void* a, const void* b, size_t n) { return n == 0 || memcmp(a, b, n) == 0; };
    same[0] = A.unit.size() == B.unit.size() && eq(A.unit.data(), B.unit.data(), (size_t)out[0]);
    same[1] = A.unit_eye.size() == B.unit_eye.size() && eq(A.unit_eye.data(), B.unit_eye.data(), (size_t)out[1]);
    same[2] = A.bunit.size() == B.bunit.size() && eq(A.bunit.data(), B.bunit.data(), (size_t)out[2]);
    same[3] = A.kd.size() == B.kd.size() && eq(A.kd.data(), B.kd.data(), (size_t)out[3]);
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
    HostScene H;
    if (!prepare_scene(d, &H, L).empty()) return -1;
    bind_host(&H);
    if (lanes < 1 || (lanes & (lanes - 1))) return -2;
    const bool lens = (p->flags & PT_FLAG_LENS) != 0, aa = (p->flags & PT_FLAG_AA) != 0;
    if (lens && !L) return -3;
    Counters c = {};
    double spill_mem[kSpillSlots];
    const Spill sp{spill_mem, 1};
    for (int iy = 0; iy < p->height; ++iy) {
        for (int ix = 0; ix < p->width; ++ix) {
            std::vector<D3> a(lanes), s(lanes), q(lanes);
            const AaPixel X{p->width, p->height, ix, iy};
            // the centre ray and its hit, for a launch with neither flag
            const D3 eye = ld3(H.k.eye);
            const D3 dc = d3(linspace_at(H.k.ortho[0], H.k.ortho[2], p->width, ix) - eye.x,
                             linspace_at(H.k.ortho[1], H.k.ortho[3], p->height, iy) - eye.y, 0.0 - eye.z);
            D3 P0 = d3(0, 0, 0);
            int tri0 = -1;
            if (!lens && !aa && p->bounces > 0)
                tri0 = force64 ? closest<true, false>(H.k, eye, dc, -1, sp, &P0, &c, true)
                               : closest<false, false>(H.k, eye, dc, -1, sp, &P0, &c, true);
            for (int l = 0; l < lanes; ++l) {
                const int32_t ns = l < p->spp ? (p->spp - l + lanes - 1) / lanes : 0;
                const LaneJob J = lane_job(p, ix, iy, p->sample_begin + l, lanes, ns);
                MomentRegs M;
                M.clear();
                if (lens && aa) {
                    if (force64) {
                        a[l] = render_lane_lens<true, true, true>(H.k, J, X, sp, &c);
                        render_lane_moments_lens<true, true, true>(H.k, J, X, sp, &c, M);
                    } else {
                        a[l] = render_lane_lens<false, true, true>(H.k, J, X, sp, &c);
                        render_lane_moments_lens<false, true, true>(H.k, J, X, sp, &c, M);
                    }
                } else if (lens) {
                    if (force64) {
                        a[l] = render_lane_lens<true, true, false>(H.k, J, X, sp, &c);
                        render_lane_moments_lens<true, true, false>(H.k, J, X, sp, &c, M);
                    } else {
                        a[l] = render_lane_lens<false, true, false>(H.k, J, X, sp, &c);
                        render_lane_moments_lens<false, true, false>(H.k, J, X, sp, &c, M);
                    }
                } else if (aa) {
                    if (force64) {
                        a[l] = render_lane_aa<true, true>(H.k, J, X, kNoEye, sp, &c);
                        render_lane_moments_aa<true, true>(H.k, J, X, kNoEye, sp, &c, M);
                    } else {
                        a[l] = render_lane_aa<false, true>(H.k, J, X, kNoEye, sp, &c);
                        render_lane_moments_aa<false, true>(H.k, J, X, kNoEye, sp, &c, M);
                    }
                } else {
                    if (force64) {
                        a[l] = render_lane<true, false>(H.k, J, dc, tri0, P0, sp, &c);
                        render_lane_moments<true, false, true>(H.k, J, dc, tri0, P0, sp, &c, M);
                    } else {
                        a[l] = render_lane<false, false>(H.k, J, dc, tri0, P0, sp, &c);
                        render_lane_moments<false, false, true>(H.k, J, dc, tri0, P0, sp, &c, M);
                    }
                }
                s[l] = M.sum();
                q[l] = M.sumsq();
            }
            const D3 ra = xor_reduce(a), rs = xor_reduce(s), rq = xor_reduce(q);
            const size_t e = (size_t)(p->height - 1 - iy) * p->width + ix;
            sum[3 * e] = ra.x; sum[3 * e + 1] = ra.y; sum[3 * e + 2] = ra.z;
            S[3 * e] = rs.x; S[3 * e + 1] = rs.y; S[3 * e + 2] = rs.z;
            Q[3 * e] = rq.x; Q[3 * e + 1] = rq.y; Q[3 * e + 2] = rq.z;
        }
    }
    return 0;
}

// hc_accum_aa through the lens: the accumulator's pass loop with the lens's
// samples (PT_FLAG_AA in p->flags: jittered as well), one lane per pixel.
int hc_accum_lens(const pt_scene_desc* d, const pt_lens* L, const pt_render_params* p, double tol,
                  double floor, uint32_t min_spp, uint32_t max_spp, uint32_t step_spp, double* S, double* Q,
                  uint32_t* n) {
    HostScene H;
    if (!L || !prepare_scene(d, &H, L).empty()) return -1;
    bind_host(&H);
    const bool aa = (p->flags & PT_FLAG_AA) != 0;
    const AdaptK A{tol, floor, min_spp, max_spp, step_spp};
    Counters c = {};
    double spill_mem[kSpillSlots];
    const Spill sp{spill_mem, 1};
    const size_t np = (size_t)p->width * p->height;
    for (size_t i = 0; i < 3 * np; ++i) S[i] = Q[i] = 0.0;
    for (size_t i = 0; i < np; ++i) n[i] = 0;
    for (int pass = 0; pass <= (int)max_spp + 1; ++pass) {
        bool any = false;
        for (size_t e = 0; e < np; ++e) {
            const double err = moment_err(S + 3 * e, Q + 3 * e, n[e], floor);
            if (!adapt_active(n[e], err, A)) continue;
            const uint32_t k = adapt_k(n[e], A);
            if (k == 0) continue;
            any = true;
            const int row = (int)(e / p->width), ix = (int)(e % p->width), iy = p->height - 1 - row;
            const LaneJob J = lane_job(p, ix, iy, (int32_t)n[e], 1, (int32_t)k);
            MomentRegs M;
            M.clear();
            const AaPixel X{p->width, p->height, ix, iy};
            if (aa) render_lane_moments_lens<false, true, true>(H.k, J, X, sp, &c, M);
            else render_lane_moments_lens<false, true, false>(H.k, J, X, sp, &c, M);
            const D3 s = M.sum(), q = M.sumsq();
            S[3 * e] += s.x; S[3 * e + 1] += s.y; S[3 * e + 2] += s.z;
            Q[3 * e] += q.x; Q[3 * e + 1] += q.y; Q[3 * e + 2] += q.z;
            n[e] += k;
        }
        if (!any) return pass;
    }
    return -3;
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
    if (!L || !prepare_scene(d, &H, L).empty()) return -1;
    bind_host(&H);
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
    const D3 eye = ld3(H.k.eye);
    const double R = L->radius;
    int64_t wrong = 0, amb = 0, tests = 0;
    for (int64_t i = 0; i < n_rays; ++i) {
        double lx = 0.0, ly = 0.0;
        if (i >= 1 && i <= 4) {   // the rim's axis points
            lx = i == 1 ? R : i == 2 ? -R : 0.0;
            ly = i == 3 ? R : i == 4 ? -R : 0.0;
        } else if (i > 4) {
            const double phi = 6.283185307179586 * U(rng), r = i % 2 ? R : R * sqrt(U(rng));
            lx = r * cos(phi);
            ly = r * sin(phi);
        }
        const D3 o = d3(eye.x + lx, eye.y + ly, eye.z);
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
    return 0;
}

}  // extern "C"
