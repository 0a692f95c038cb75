// pt_light_host.cpp — TEST INFRASTRUCTURE.  The light pick of the lane code
// (pt_core.h pick_light and its forms, light_tri_of) on the host, on top of
// pt_hostcheck.cpp.  Two uses, both from tests/test_light_pick_host.py, built
// by the hostcheck Makefile's pattern rule (tests/hostlib.py) into a temporary directory:
//   * a stand-alone program (main below): the counting forms against the
//     loop form for every u = k / 2^24 and for u outside [0, 1) on synthetic
//     tables, and the light point against the path through light_tri;
//   * a shared library: hc_light_check runs the same comparison on the table
//     prepare_scene builds for a real scene (the Cornell light).
// Exit status / return value 0: every comparison held.
#include "pt_hostcheck.cpp"

#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

namespace {

// A scene that holds only what the pick and the light point read.
struct LightScene {
    std::vector<double> cum, kd;
    std::vector<int32_t> light_tri;
    std::vector<TriD> trid;
    SceneK k{};
    LightScene(const std::vector<double>& areas, int n_obj_tri, uint64_t seed) {
        cum.assign(1, 0.0);
        double acc = 0.0;   // prepare_scene's running sums
        for (size_t i = 0; i < areas.size(); ++i) {
            light_tri.push_back(n_obj_tri + (int)i);
            acc += areas[i];
            cum.push_back(acc);
        }
        kd.assign(kKdCount, 0.0);
        kd[kKdLightSum] = acc;
        std::mt19937_64 rng(seed);
        std::uniform_real_distribution<double> U(-30.0, 30.0);
        trid.assign(n_obj_tri + areas.size(), TriD{});
        for (TriD& T : trid)
            for (int c = 0; c < 3; ++c) { T.v1[c] = U(rng); T.v2[c] = U(rng); T.v3[c] = U(rng); }
        k.n_obj_tri = n_obj_tri;
        k.n_tri = (int32_t)trid.size();
        k.n_light = (int32_t)areas.size();
        k.light_sum = acc;
        k.light_mono = light_table_mono(cum) ? 1 : 0;
        k.light_cum = cum.data();
        k.light_tri = light_tri.data();
        k.trid = trid.data();
        k.kd = kd.data();
    }
};

bool same_bits(double a, double b) { return memcmp(&a, &b, 8) == 0; }

// every form against the loop form at u; returns the number of mismatches
int check_u(const SceneK& S, const LightTab& lt, double u) {
    const int want = pick_light_loop(S, u);
    int bad = 0;
    bad += pick_light(S, u) != want;
    bad += pick_light(S, lt, u) != want;
    if (S.light_mono) {
        bad += pick_light_count(S.light_cum, S.n_light, u) != want;
        if (S.n_light == 2) bad += pick_light_pair(S.light_cum[1], S.light_cum[2], u) != want;
    }
    if (bad) fprintf(stderr, "pick mismatch at u = %a: loop %d, dispatch %d\n", u, want, pick_light(S, u));
    return bad;
}

// the table's invariants, every u = k / 2^24, the u outside [0, 1), and the
// light point of 10^4 random quadruples
int check_scene(const SceneK& S, const char* name, int want_mono) {
    int bad = 0;
    if (want_mono >= 0 && S.light_mono != want_mono) {
        fprintf(stderr, "%s: light_mono %d, expected %d\n", name, S.light_mono, want_mono);
        ++bad;
    }
    if (!same_bits(S.light_cum[S.n_light], S.kd[kKdLightSum])) {
        fprintf(stderr, "%s: cum[n_light] is not light_sum\n", name);
        ++bad;
    }
    for (int i = 0; i < S.n_light; ++i) bad += S.light_tri[i] != light_tri_of(S, i);
    const LightTab lt = light_tab(S);
    if (lt.form != (S.light_mono ? (S.n_light == 2 ? 2 : 1) : 0)) ++bad;
    int seen[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t k = 0; k < (1u << 24) && bad < 10; ++k) {
        const double u = u_of(k << 8);   // the render loop's uniforms, all of them
        bad += check_u(S, lt, u);
        const int li = pick_light_loop(S, u);
        if (li < 8) seen[li] = 1;
    }
    const double outside[] = {-0.5, 1.0, 1.5, std::numeric_limits<double>::quiet_NaN(), -0.0,
                              std::numeric_limits<double>::infinity()};
    for (double u : outside) bad += check_u(S, lt, u);
    std::mt19937_64 rng(12345);
    for (int i = 0; i < 10000; ++i) {
        const double u0 = u_of((uint32_t)rng()), u1 = u_of((uint32_t)rng()), u2 = u_of((uint32_t)rng()),
                     u3 = u_of((uint32_t)rng());
        const D3 a = light_point(S.trid[S.light_tri[pick_light_loop(S, u0)]], u1, u2, u3);
        const D3 b = light_point(S.trid[light_tri_of(S, pick_light(S, u0))], u1, u2, u3);
        const D3 c = light_point(S.trid[light_tri_of(S, pick_light(S, lt, u0))], u1, u2, u3);
        if (!(same_bits(a.x, b.x) && same_bits(a.y, b.y) && same_bits(a.z, b.z) &&
              same_bits(a.x, c.x) && same_bits(a.y, c.y) && same_bits(a.z, c.z))) {
            if (bad < 10) fprintf(stderr, "%s: light point differs at quadruple %d\n", name, i);
            ++bad;
        }
    }
    int n_seen = 0;
    for (int i = 0; i < 8; ++i) n_seen += seen[i];
    printf("%s: n_light %d, mono %d, form %d, %d triangles picked, %d mismatches\n", name, S.n_light,
           S.light_mono, lt.form, n_seen, bad);
    return bad;
}

}  // namespace

extern "C" {

// The checks on the table prepare_scene builds for d.  info: light_mono,
// n_light, the number of mismatches.
int hc_light_check(const pt_scene_desc* d, int32_t* info) {
    HostScene H;
    if (!prepare_scene(d, &H).empty()) return -1;
    bind_host(&H);
    info[0] = H.k.light_mono;
    info[1] = H.k.n_light;
    info[2] = check_scene(H.k, "scene", -1);
    return 0;
}

}  // extern "C"

int main() {
    int bad = 0;
    {   // a quad light (the Cornell light's shape: two triangles of one area)
        LightScene L({3.38, 3.38}, 30, 1);
        bad += check_scene(L.k, "quad", 1);
    }
    {
        LightScene L({0.75}, 4, 2);
        bad += check_scene(L.k, "one", 1);
    }
    {   // a zero-area middle triangle: never picked, by either rule
        LightScene L({1.25, 0.0, 2.5}, 7, 3);
        bad += check_scene(L.k, "zero-middle", 1);
        for (uint32_t k = 0; k < (1u << 24); k += 4099) bad += pick_light(L.k, u_of(k << 8)) == 1;
    }
    {   // two triangles, the second of zero area (the pair form's edge)
        LightScene L({1.5, 0.0}, 2, 4);
        bad += check_scene(L.k, "zero-last", 1);
    }
    {
        std::mt19937_64 rng(99);
        std::uniform_real_distribution<double> A(0.01, 5.0);
        std::vector<double> a;
        for (int i = 0; i < 7; ++i) a.push_back(A(rng));
        LightScene L(a, 11, 5);
        bad += check_scene(L.k, "seven", 1);
    }
    {   // a negative area: the sums go down, the loop form stays
        LightScene L({2.0, -0.5, 1.0}, 5, 6);
        bad += check_scene(L.k, "non-monotone", 0);
        // (the counting form would differ here: the check is needed)
        int differs = 0;
        for (uint32_t k = 0; k < (1u << 24); k += 257)
            differs += pick_light_count(L.k.light_cum, L.k.n_light, u_of(k << 8)) !=
                       pick_light_loop(L.k, u_of(k << 8));
        if (!differs) { fprintf(stderr, "non-monotone: the forms never differ\n"); ++bad; }
    }
    {   // a NaN and an infinite area: not finite, the loop form stays
        LightScene L({1.0, std::numeric_limits<double>::quiet_NaN()}, 3, 7);
        bad += check_scene(L.k, "nan", 0);
        LightScene M({1.0, std::numeric_limits<double>::infinity()}, 3, 8);
        bad += check_scene(M.k, "inf", 0);
    }
    printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
