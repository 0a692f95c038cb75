// pt_rays_host.cpp — TEST INFRASTRUCTURE.  The ray lane code (pt_path.h
// rays_in_frame / rays_primary, RayHit with either sink through render_loop)
// compiled for the host on top of pt_lens_host.cpp, so the CPU suite can check
// the rule of pt_radiance (include/pt_capi.h) against the oracle without a
// GPU.  Built by tests/test_rays_host.py into a temporary directory with the
// hostcheck Makefile's g++ flags.
#include "pt_lens_host.cpp"

extern "C" {

// k_render_rays on the host: for each of the n records, `lanes` (a power of
// two) emulated lanes, lane c taking samples sample_begin + c, + lanes, ...,
// reduced in the kernel's xor order.  sum: the colour sums of the form without
// moments (SumSink); S, Q: the moments' (MomentSink), all [n][3] f64 in
// the records' order.  route[i]: what rays_primary itself reports — 1 when no
// lane's primary query ran the f32 filter's branch (forced f64, or an origin
// outside the frame), 0 when every lane's did, -1 when the lanes disagree.
// box (may be null): pt_scene_create_rays' box.
int hc_radiance(const pt_scene_desc* d, const double* box, const RayK* rays, int64_t n,
                const pt_render_params* p, int force64, int32_t lanes, double* sum, double* S, double* Q,
                int32_t* route) {
    HostScene H;
    if (!prepare_scene(d, &H, nullptr, box).empty()) return -1;
    bind_host(&H);
    if (lanes < 1 || (lanes & (lanes - 1))) return -2;
    Counters c = {};
    double spill_mem[kSpillSlots];
    const Spill sp{spill_mem, 1};
    for (int64_t i = 0; i < n; ++i) {
        const RayK* ray = rays + i;
        std::vector<D3> a(lanes), s(lanes), q(lanes);
        int n_f32 = 0, n_traced = 0;
        for (int l = 0; l < lanes; ++l) {
            LaneJob J;
            J.seed = p->seed;
            J.pixel = ray->key;
            J.sample0 = p->sample_begin + l;
            J.sample_stride = lanes;
            J.n_samples = l < p->spp ? (p->spp - l + lanes - 1) / lanes : 0;
            J.bounces = p->bounces;
            J.rr_depth = (p->flags & PT_FLAG_RR) ? std::max(0, p->rr_depth) : -1;
            D3 P0 = d3(0, 0, 0);
            int tri0 = -1;
            MomentRegs M;
            M.clear();
            if (J.n_samples > 0 && p->bounces > 0) {
                bool f32 = false;
                tri0 = force64 ? rays_primary<true, true>(H.k, H.frame_x, ld3(ray->o), ld3(ray->d), sp, &P0, &c, &f32)
                               : rays_primary<false, true>(H.k, H.frame_x, ld3(ray->o), ld3(ray->d), sp, &P0, &c, &f32);
                ++n_traced;
                n_f32 += f32 ? 1 : 0;
            }
            if (force64) {
                a[l] = render_lane_rays<true, true>(H.k, J, ray, tri0, P0, sp, &c);
                render_lane_moments_rays<true, true>(H.k, J, ray, tri0, P0, sp, &c, M);
            } else {
                a[l] = render_lane_rays<false, true>(H.k, J, ray, tri0, P0, sp, &c);
                render_lane_moments_rays<false, true>(H.k, J, ray, tri0, P0, sp, &c, M);
            }
            s[l] = M.sum();
            q[l] = M.sumsq();
        }
        route[i] = n_f32 == 0 ? 1 : (n_f32 == n_traced ? 0 : -1);
        const D3 ra = xor_reduce(a), rs = xor_reduce(s), rq = xor_reduce(q);
        sum[3 * i] = ra.x; sum[3 * i + 1] = ra.y; sum[3 * i + 2] = ra.z;
        S[3 * i] = rs.x; S[3 * i + 1] = rs.y; S[3 * i + 2] = rs.z;
        Q[3 * i] = rq.x; Q[3 * i + 1] = rq.y; Q[3 * i + 2] = rq.z;
    }
    return 0;
}

// FNV-1a of the frame records of the scene made with lens L (may be null), as
// the entries from before pt_scene_create_rays make it: out = {unit, unit_eye,
// bunit, kd}.  The test holds the parent commit's values.
int hc_rays_record_hash(const pt_scene_desc* d, const pt_lens* L, uint64_t* out) {
    HostScene A;
    if (!prepare_scene(d, &A, L).empty()) return -1;
    auto fnv = [](const void* p, size_t n) {
        uint64_t h = 0xcbf29ce484222325ull;
        const unsigned char* b = (const unsigned char*)p;
        for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
        return h;
    };
    out[0] = fnv(A.unit.data(), A.unit.size() * sizeof(UnitF));
    out[1] = fnv(A.unit_eye.data(), A.unit_eye.size() * sizeof(UnitF));
    out[2] = fnv(A.bunit.data(), A.bunit.size() * sizeof(UnitF));
    out[3] = fnv(A.kd.data(), A.kd.size() * sizeof(double));
    return 0;
}

// hc_lens_records for the box: whether the scene made with `box` (may be null)
// has the same bytes in {unit, unit_eye, bunit, kd} as the scene made without
// (same[4]); X = {the "all" frame's centre x, y, z, rays_in_frame's extent} of
// the scene made with it.
int hc_rays_records(const pt_scene_desc* d, const double* box, int32_t* same, double* X) {
    HostScene A, B;
    if (!prepare_scene(d, &A).empty() || !prepare_scene(d, &B, nullptr, box).empty()) return -1;
    auto eq = [](const void* a, const void* b, size_t n) { return n == 0 || memcmp(a, b, n) == 0; };
    same[0] = A.unit.size() == B.unit.size() && eq(A.unit.data(), B.unit.data(), A.unit.size() * sizeof(UnitF));
    same[1] = A.unit_eye.size() == B.unit_eye.size() &&
              eq(A.unit_eye.data(), B.unit_eye.data(), A.unit_eye.size() * sizeof(UnitF));
    same[2] = A.bunit.size() == B.bunit.size() && eq(A.bunit.data(), B.bunit.data(), A.bunit.size() * sizeof(UnitF));
    same[3] = A.kd.size() == B.kd.size() && eq(A.kd.data(), B.kd.data(), A.kd.size() * sizeof(double));
    X[0] = B.k.center[0]; X[1] = B.k.center[1]; X[2] = B.k.center[2];
    X[3] = B.frame_x;
    return 0;
}

// rays_in_frame's verdict on n origins ([n][3]) of the scene made with box
int hc_rays_in_frame(const pt_scene_desc* d, const double* box, const double* o, int64_t n, int32_t* in) {
    HostScene H;
    if (!prepare_scene(d, &H, nullptr, box).empty()) return -1;
    bind_host(&H);
    for (int64_t i = 0; i < n; ++i) in[i] = rays_in_frame(H.k, H.frame_x, d3(o[3 * i], o[3 * i + 1], o[3 * i + 2])) ? 1 : 0;
    return 0;
}

// hc_lens_filter from the box: n lines whose origins lie in the box of the
// scene made with it — the eye, the eight corners, then uniform points, every
// one admitted by rays_in_frame (out[3] counts those that are not: must be 0)
// — tested against every unit with filter_eval.h's forms over unit_eye (and
// the BVH units), the directions aimed as hc_filter_selftest aims them.
// out[0] = wrong certain verdicts against this build's eval64 (must be 0),
// out[1] = ambiguous verdicts, out[2] = tests.
int hc_rays_filter(const pt_scene_desc* d, const double* box, int64_t n_rays, uint64_t seed, int64_t* out) {
    HostScene H;
    if (!box || !prepare_scene(d, &H, nullptr, box).empty()) return -1;
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
    int64_t wrong = 0, amb = 0, tests = 0, outside = 0;
    for (int64_t i = 0; i < n_rays; ++i) {
        D3 o = ld3(H.k.eye);
        if (i >= 1 && i <= 8) {
            const int c = (int)(i - 1);
            o = d3(box[c & 1 ? 3 : 0], box[c & 2 ? 4 : 1], box[c & 4 ? 5 : 2]);
        } else if (i > 8) {
            o = d3(box[0] + (box[3] - box[0]) * U(rng), box[1] + (box[4] - box[1]) * U(rng),
                   box[2] + (box[5] - box[2]) * U(rng));
        }
        if (!rays_in_frame(H.k, H.frame_x, o)) ++outside;
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
    out[0] = wrong; out[1] = amb; out[2] = tests; out[3] = outside;
    return 0;
}

}  // extern "C"
