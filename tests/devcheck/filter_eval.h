// filter_eval.h — TEST INFRASTRUCTURE.  One line of the filter self-test
// against every uniform and BVH unit, written once and compiled twice: by
// g++ into the host check (tests/hostcheck: hc_filter_selftest and
// hc_filter_cases) and by hipcc for gfx950 into the device check
// (tests/devcheck: dc_filter).  Each build runs the product headers' own
// implementation for its side (v_rcp_f32, v_minimum3_f32, the reordered del
// ... on the device; their host twins on the host), so the two outputs are
// the same tests in the same layout on two arithmetics.  The truth both are
// judged by is the host build's eval64 (hc_filter_cases).
//
// Included after pt_path.h and pt_prepare.h, inside no namespace.
#pragma once

namespace ptcheck {
using namespace pt;

// verdict kinds of a (line, unit, member) slot; code -1: no such test
enum : int {
    kClosest = 0,    // classify_tri, closest range
    kShadow = 1,     // classify_tri, shadow range
    kMarginF = 2,    // margin_plane + margin_tri, shadow range
    kQuadShadow = 3, // uniform units: quad_m + margin_m
    kQuadClosest = 4,  // uniform units: quad_m + verdict_m
    kLean = 5,       // uniform units: quad_m + the lean closest range
    kCClosest = 6,   // BVH units in the walks' 64-B form (unitc_f): as 0, 1, 2
    kCShadow = 7,
    kCMarginF = 8,
    kKinds = 9
};
// mflag bits of a (line, unit): claims that must hold (all zero)
enum : int {
    kMfOcc = 1,      // margin_unit's occlusion verdict differs from the members'
    kMfLost = 2      // margin_unit drops an ambiguous member test
};
constexpr int kSumN = 7;   // shadow_unit_m outputs: oc[0..2], amax, key2, leak; the unit's object

struct FilterLines {       // the generated lines, [n] each
    const double* o;       // [n][3]
    const double* dn;      // [n][3] unit direction
    const double* lim;     // shadow range (squared distance)
    const float* hlo;
    const float* hhi;      // its f32 bracket
    const int32_t* at_eye; // origin at the eye (frame `center`) or on a surface
};
struct FilterOut {
    int8_t* code;          // [n][nu][2][kKinds]
    int8_t* hit;           // [n][nu][2]  this build's eval64: hit flag
    double* sqd;           // [n][nu][2]  ... and squared distance
    float* atdt;           // [n][nu][4]  closest plane part: at, dt; the 64-B form's at, dt
    int8_t* mflag;         // [n][nu]
    float* sum;            // [n][n_obj_unit][kSumN]
};

PT_HD int margin_code(float mc, float ma) { return mc > 0.0f ? kCand : (ma >= 0.0f ? kAmb : kMiss); }

// the three single-triangle forms of member i of U
PT_HD void tri_codes(const UnitF& U, int i, const OriginU& O, const RayPlane& pc, const RayPlane& ps,
                     F3 d32, float hlo, float hhi, int8_t* c3) {
    const TriB& B = U.tri[i];
    const float bo = i ? O.bo1 : O.bo0, co = i ? O.co1 : O.co0;
    c3[0] = (int8_t)verdict_code(classify_tri(B, pc, bo, co, d32));
    c3[1] = (int8_t)verdict_code(classify_tri(B, ps, bo, co, d32));
    float cm, nm, mc, ma;
    margin_plane(U, ps, hlo, hhi, INFINITY, &cm, &nm);
    margin_tri(B, ps, bo, co, d32, cm, nm, &mc, &ma);
    c3[2] = (int8_t)margin_code(mc, ma);
}

// Line i against every unit.  `write`: false for a lane that only fills its
// wave (shadow_unit_m votes across the wave: the device runs it with all 64
// lanes active, the spare lanes repeating the last line).
PT_HD void filter_line(const SceneK& S, const FilterLines& L, int64_t i, const FilterOut& F, bool write) {
    const D3 o = ld3(L.o + 3 * i), dn = ld3(L.dn + 3 * i);
    const bool at_eye = L.at_eye[i] != 0;
    const float hlo = L.hlo[i], hhi = L.hhi[i];
    const D3 C = ld3(S.center), Cs = ld3(S.center_s);
    const F3 o32 = to_f3(o - C), o32s = to_f3(o - Cs), d32 = to_f3(dn);
    const int64_t nu = (int64_t)S.n_unit + S.n_bunit;
    for (int u = 0; u < S.n_unit + S.n_bunit; ++u) {
        const bool uni = u < S.n_unit;
        const UnitF& U = uni ? (at_eye ? S.unit_eye[u] : S.unit[u]) : S.bunit[u - S.n_unit];
        const OriginU O = origin_u(U, (uni && !at_eye) ? o32s : o32);
        const RayPlane pc = ray_plane(U, O.h, d32, INFINITY, INFINITY);
        const RayPlane ps = ray_plane(U, O.h, d32, hlo, hhi);
        const int64_t lu = i * nu + u;
        int8_t code[2][kKinds];
        for (int m = 0; m < 2; ++m)
            for (int k = 0; k < kKinds; ++k) code[m][k] = -1;
        float atdt[4] = {pc.at, pc.dt, 0.f, 0.f};
        int8_t mflag = 0;
        for (int m = 0; m < 2; ++m) {
            D3 Q = d3(0, 0, 0);
            double sqd = 0.0;
            // (a single's second slot: no triangle, no hit)
            const bool h = m < U.count && eval64(S.trid[U.t[m]], o, dn, &Q, &sqd);
            if (write) {
                F.hit[lu * 2 + m] = h ? 1 : 0;
                F.sqd[lu * 2 + m] = m < U.count ? sqd : 0.0;
            }
            if (m < U.count) tri_codes(U, m, O, pc, ps, d32, hlo, hhi, &code[m][kClosest]);
        }
        if (!uni && S.bunitc) {   // the walks' 64-B form of the same BVH unit
            const UnitF UC = unitc_f(S, S.bunitc[u - S.n_unit]);
            const OriginU OC = origin_u(UC, o32);
            const RayPlane qc = ray_plane(UC, OC.h, d32, INFINITY, INFINITY);
            const RayPlane qs = ray_plane(UC, OC.h, d32, hlo, hhi);
            atdt[2] = qc.at;
            atdt[3] = qc.dt;
            tri_codes(UC, 0, OC, qc, qs, d32, hlo, hhi, &code[0][kCClosest]);
        }
        if (uni) {   // the render loop's unit form (quad_m): both members' tests
            float cm, nm;
            margin_plane(U, ps, hlo, hhi, INFINITY, &cm, &nm);
            const OriginU Oq = origin_q(U, at_eye ? o32 : o32s);
            const QuadM qs = quad_m(U, ps, Oq, d32), qc = quad_m(U, pc, Oq, d32);
            {   // the merged unit margins (PT_MMERGE, margin_unit) against the members'
                float c0, a0, c1, a1, cu, au;
                margin_m(qs.m0, ps, cm, nm, &c0, &a0);
                margin_m(qs.m1, ps, cm, nm, &c1, &a1);
                margin_unit(cm, nm, fmaxf(qs.m0, qs.m1), ps.del, &cu, &au);
                const bool occ = c0 > 0.0f || c1 > 0.0f;
                if ((cu > 0.0f) != occ) mflag |= kMfOcc;                                  // occlusion: same verdict
                if (!occ && (a0 >= 0.0f || a1 >= 0.0f) && !(au >= 0.0f)) mflag |= kMfLost;   // no lost f64 test
            }
            RayPlane pl = pc;   // the render loop's lean closest range (PT_CLOSEST_LEAN)
            pl.rcand = (fabsf(pl.q) > U.qhi) & (pl.at - pl.dt > kTzHi);
            pl.rmiss = pl.at + pl.dt < kTzLo;
            for (int m = 0; m < 2; ++m) {
                float mc, ma;
                margin_m(m ? qs.m1 : qs.m0, ps, cm, nm, &mc, &ma);
                code[m][kQuadShadow] = (int8_t)margin_code(mc, ma);
                code[m][kQuadClosest] = (int8_t)verdict_code(verdict_m(m ? qc.m1 : qc.m0, pc));
                code[m][kLean] = (int8_t)verdict_code(verdict_m(m ? qc.m1 : qc.m0, pl));
            }
            if (u < S.n_obj_unit) {
                // shadow_unit_m as the render loop enters it for a unit (no
                // occluder yet, nothing ambiguous yet, no leak yet), the line
                // as each of its three shadow rays: rays 0 and 1 take the
                // "until occluded" form, ray 2 the leaked-colour form
                ShadowSet sh;
                for (int k = 0; k < kLightSamples; ++k) {
                    sh.d32[k] = d32;
                    sh.hlo[k] = hlo;
                    sh.hhi[k] = hhi;
                    sh.occ[k] = false;
                    sh.first[k] = S.n_tri;
                    sh.ln[k] = 0.0;
                }
                sh.key2 = S.n_obj;
                sh.leak = S.n_obj - 1;
                float oc[kLightSamples] = {-1.0f, -1.0f, -1.0f};
                float amax = -1.0f;
                uint32_t amb = 0;
                shadow_unit_m(S, U, Oq, false, &sh, oc, &amb, &amax);
                if (write) {
                    float* s = F.sum + (i * S.n_obj_unit + u) * kSumN;
                    s[0] = oc[0]; s[1] = oc[1]; s[2] = oc[2];
                    s[3] = amax;
                    s[4] = (float)sh.key2;
                    s[5] = (float)sh.leak;
                    s[6] = (float)U.obj;
                }
            }
        }
        if (write) {
            for (int m = 0; m < 2; ++m)
                for (int k = 0; k < kKinds; ++k) F.code[(lu * 2 + m) * kKinds + k] = code[m][k];
            for (int k = 0; k < 4; ++k) F.atdt[lu * 4 + k] = atdt[k];
            F.mflag[lu] = mflag;
        }
    }
}

}  // namespace ptcheck
