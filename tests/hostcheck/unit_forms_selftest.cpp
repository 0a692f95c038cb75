// unit_forms_selftest.cpp — TEST INFRASTRUCTURE.  The render loop's unit
// forms (pt_path.h quad_m, closest_unit_m, closest_add_bf, closest_bits_m)
// checked test by test on the host build: the rays of hc_filter_selftest
// against every uniform unit, the shipped unit-level closest form against the
// per-member reference (verdict_m on the members' weight minimums with the
// lean range) and against eval64.  Built by tests/test_unit_forms_host.py
// by the hostcheck Makefile's pattern rule (tests/hostlib.py).
#include "pt_hostcheck.cpp"

namespace {

// quad_m's plain branchy formula: the reference the shipped one must equal
// bit for bit, however its branches are arranged
QuadM quad_m_branchy(const UnitF& U, const RayPlane& p, const OriginU& O, F3 d) {
    const float beta = fmaf(p.t, lin3(U.tri[0].gb, d), O.bo0);
    const float gam = fmaf(p.t, lin3(U.tri[0].gc, d), O.co0);
    const float s = beta + gam;
    QuadM r;
    r.m0 = min3f(beta, gam, 1.0f - s);
    r.m1 = -INFINITY;
    if (U.quad > 0) {
        r.m1 = min3f(s, 1.0f - gam, -beta);
    } else if (U.quad < 0) {
        const float b1 = fmaf(p.t, lin3(U.tri[1].gb, d), O.bo1);
        const float g1 = fmaf(p.t, lin3(U.tri[1].gc, d), O.co1);
        r.m1 = min3f(b1, g1, (1.0f - b1) - g1);
    }
    return r;
}

bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }

// closest_add_bf (the branch-free bookkeeping of closest_unit_m, its second
// bound a median of three) against closest_add over every sequence of four
// candidates from a set with ties and +inf ("no candidate").  Returns the
// number of sequences that end in another state.
int64_t add_grid() {
    const float as[] = {INFINITY, 0.5f, 1.0f, 1.0f, 2.0f, 3.0e30f};
    const int n = (int)(sizeof as / sizeof *as);
    int64_t bad = 0;
    for (int i = 0; i < n * n * n * n; ++i) {
        ClosestAcc x = closest_init(), y = closest_init();
        for (int k = 0, j = i; k < 4; ++k, j /= n) {
            const float a = as[j % n], b = a + 0.25f;
            closest_add(&x, 10 * k + j % n, a, b);
            closest_add_bf(&y, 10 * k + j % n, a, b);
        }
        if (!(same_bits(x.a1, y.a1) && same_bits(x.a2, y.a2) && same_bits(x.b1, y.b1) && x.i1 == y.i1)) ++bad;
    }
    return bad;
}

}  // namespace

extern "C" {

// out[0]  unit tests whose certain-candidate flag, candidate triangle or
//         interval (as closest_unit_m leaves them in a fresh ClosestAcc)
//         differs from the per-member reference
// out[1]  unit tests with an ambiguous member the unit flag lacks
// out[2]  certain verdicts of the unit form that eval64 contradicts
// out[3]  quad_m weight minimums that differ bitwise from the branchy formula
// out[4]  closest_bits_m results that are not the members' ambiguity bits
// out[5]  candidate sequences closest_add_bf and closest_add leave in
//         different states
// out[6]  unit tests          out[7]  with an ambiguous member
// out[8]  certain candidates, out[9..11] of them through a single triangle,
//         a parallelogram, a skew pair
int hc_unit_forms_selftest(const pt_scene_desc* d, int64_t n_rays, uint64_t seed, int64_t* out) {
    HostScene H;
    if (!prepare_scene(d, &H).empty()) return -1;
    bind_host(&H);
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::normal_distribution<double> N(0.0, 1.0);
    int64_t cdiff = 0, lost = 0, wrong = 0, qdiff = 0, bdiff = 0, tests = 0, amb = 0, cand = 0;
    int64_t kind[3] = {0, 0, 0};
    const D3 C = ld3(H.k.center), Cs = ld3(H.k.center_s);
    for (int64_t i = 0; i < n_rays; ++i) {
        // (the rays of hc_filter_selftest, draw for draw)
        D3 o;
        if (i % 4 == 0) {
            o = ld3(H.k.eye);
        } else {
            const TriD& T = H.trid[rng() % H.trid.size()];
            double a = U(rng), b = U(rng);
            if (a + b > 1) { a = 1 - a; b = 1 - b; }
            o = ld3(T.v1) + (ld3(T.v2) - ld3(T.v1)) * a + (ld3(T.v3) - ld3(T.v1)) * b;
        }
        D3 dir = d3(N(rng), N(rng), N(rng));
        if (i % 3 == 0) {
            const TriD& T = H.trid[rng() % H.trid.size()];
            dir = ld3(T.v1) + d3(N(rng), N(rng), N(rng)) * 1e-3 - o;
        } else if (i % 3 == 1 && (i / 3) % 2 == 0) {
            const TriD& T = H.trid[rng() % H.trid.size()];
            const D3 vv[3] = {ld3(T.v1), ld3(T.v2), ld3(T.v3)};
            const int e = (int)(rng() % 3);
            const double a = U(rng), sc = pow(10.0, -2.0 - 7.0 * U(rng));
            dir = vv[e] + (vv[(e + 1) % 3] - vv[e]) * a + d3(N(rng), N(rng), N(rng)) * sc - o;
        }
        const D3 dn = unit(dir);
        const bool at_eye = i % 4 == 0;
        const F3 o32 = to_f3(o - C), o32s = to_f3(o - Cs), d32 = to_f3(dn);
        const double lim = 0.5 + 40.0 * U(rng);
        const float hlo = (float)(sqrt(lim) * (1 - 1e-6)), hhi = (float)(sqrt(lim) * (1 + 1e-6));
        for (int u = 0; u < H.k.n_unit; ++u) {
            const UnitF& Un = at_eye ? H.unit_eye[u] : H.unit[u];
            const OriginU O = origin_q(Un, at_eye ? o32 : o32s);
            // quad_m on the closest ray's and a shadow ray's plane part
            const RayPlane p = closest_plane_m(Un, O, d32);
            const RayPlane ps = ray_plane(Un, O.h, d32, hlo, hhi);
            const QuadM m = quad_m(Un, p, O, d32), mr = quad_m_branchy(Un, p, O, d32);
            const QuadM s = quad_m(Un, ps, O, d32), sr = quad_m_branchy(Un, ps, O, d32);
            if (!same_bits(m.m0, mr.m0) || !same_bits(m.m1, mr.m1)) ++qdiff;
            if (!same_bits(s.m0, sr.m0) || !same_bits(s.m1, sr.m1)) ++qdiff;
            // the per-member reference
            const Verdict v0 = verdict_m(mr.m0, p), v1 = verdict_m(mr.m1, p);
            const bool rc = v0.cand | v1.cand, ra = v0.amb | v1.amb;
            const int rtc = v0.cand ? Un.t[0] : Un.t[1];
            // the shipped unit form
            ClosestAcc ca = closest_init();
            const bool ua = closest_unit_m(Un, O, false, d32, &ca);
            const bool uc = ca.i1 != -1 || (rc && !(p.at - p.dt < INFINITY));
            ++tests;
            if (uc != rc) ++cdiff;
            else if (rc) {
                // (an interval from +inf is no entry: closest_add's a < a1)
                const float lo = p.at - p.dt, hi = p.at + p.dt;
                if (lo < INFINITY ? !(ca.i1 == rtc && same_bits(ca.a1, lo) && same_bits(ca.b1, hi) &&
                                      ca.a2 == INFINITY)
                                  : ca.i1 != -1)
                    ++cdiff;
            } else if (ca.i1 != -1 || ca.a1 != INFINITY || ca.a2 != INFINITY) {
                ++cdiff;
            }
            if (ra && !ua) ++lost;
            if (closest_bits_m(Un, O, false, d32) != ((v0.amb ? 64u : 0u) | (v1.amb ? 128u : 0u))) ++bdiff;
            {   // a coplanar unit: a certain miss, nothing recorded
                ClosestAcc cc = closest_init();
                if (closest_unit_m(Un, O, true, d32, &cc) || cc.i1 != -1 || cc.a1 != INFINITY ||
                    closest_bits_m(Un, O, true, d32))
                    ++cdiff;
            }
            if (ra) ++amb;
            if (rc) {
                ++cand;
                ++kind[Un.quad == 0 ? 0 : (Un.quad > 0 ? 1 : 2)];
            }
            // eval64 on what the unit form calls certain: without an ambiguity
            // every member's verdict is certain; with one, the candidate's is
            for (int j = 0; j < Un.count; ++j) {
                D3 Q; double sqd;
                const bool h = eval64(H.trid[Un.t[j]], o, dn, &Q, &sqd) && sqd > kZero;
                const bool is_c = ca.i1 == Un.t[j];
                if (is_c) {
                    const double sq = sqrt(sqd);
                    if (!h || sq < (double)p.at - p.dt || sq > (double)p.at + p.dt) ++wrong;
                } else if (!ua && h) {
                    ++wrong;
                }
            }
        }
    }
    out[0] = cdiff; out[1] = lost; out[2] = wrong; out[3] = qdiff; out[4] = bdiff; out[5] = add_grid();
    out[6] = tests; out[7] = amb; out[8] = cand; out[9] = kind[0]; out[10] = kind[1]; out[11] = kind[2];
    return 0;
}

}  // extern "C"
