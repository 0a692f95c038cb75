// pt_rays_host.cpp — TEST INFRASTRUCTURE.  The ray lane code (pt_path.h
// rays_in_frame / rays_primary, RayHit with either sink through
// render_lane_cached)
// compiled for the host on top of pt_lens_host.cpp, so the CPU suite can check
// the rule of pt_radiance (include/pt_capi.h) against the oracle without a
// GPU.  Built by tests/test_rays_host.py into a temporary directory by the
// hostcheck Makefile's pattern rule (tests/hostlib.py).
#include "pt_lens_host.cpp"

namespace {
// A record's cached primary hit as a lane traces it (trace: the lane has samples
// and bounces); f32 (may be null): whether rays_primary took the filter's branch
template <bool F64>
RayHit ray_hit(Host& h, double frame_x, const RayK* ray, bool trace, D3* P0, bool* f32 = nullptr) {
    *P0 = d3(0, 0, 0);
    if (!trace) return RayHit{ray, -1};
    return RayHit{ray, rays_primary<F64, true>(h.H.k, frame_x, ld3(ray->o), ld3(ray->d), h.sp, P0, &h.c, f32)};
}
}  // namespace

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
    Host h;
    if (!h.open(d, nullptr, box)) return -1;
    if (lanes < 1 || (lanes & (lanes - 1))) return -2;
    pt_render_params q = *p;   // (pt_radiance's launch record: rr_depth clamped at 0)
    q.rr_depth = std::max(0, p->rr_depth);
    for (int64_t i = 0; i < n; ++i) {
        const RayK* ray = rays + i;
        int n_f32 = 0, n_traced = 0;
        store_lanes(&q, ray->key, lanes, (size_t)i, sum, S, Q, [&](const LaneJob& J) {
            return with_bool(force64 != 0, [&](auto F64) {
                const bool trace = J.n_samples > 0 && p->bounces > 0;
                bool f32 = false;
                D3 P0;
                const RayHit hit = ray_hit<decltype(F64)::value>(h, h.H.frame_x, ray, trace, &P0, &f32);
                n_traced += trace ? 1 : 0;
                n_f32 += f32 ? 1 : 0;
                return both_sinks<decltype(F64)::value>(h, J, hit, P0);
            });
        });
        route[i] = n_f32 == 0 ? 1 : (n_f32 == n_traced ? 0 : -1);
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
    same_records(A, B, same);
    X[0] = B.k.center[0]; X[1] = B.k.center[1]; X[2] = B.k.center[2];
    X[3] = B.frame_x;
    return 0;
}

// rays_in_frame's verdict on n origins ([n][3]) of the scene made with box
int hc_rays_in_frame(const pt_scene_desc* d, const double* box, const double* o, int64_t n, int32_t* in) {
    HostScene H;
    if (!open_scene(d, &H, nullptr, box)) return -1;
    for (int64_t i = 0; i < n; ++i) in[i] = rays_in_frame(H.k, H.frame_x, d3(o[3 * i], o[3 * i + 1], o[3 * i + 2])) ? 1 : 0;
    return 0;
}

// The filter self-test (filter_from) from the box: n lines whose origins lie in the box of the
// scene made with it — the eye, the eight corners, then uniform points, every
// one admitted by rays_in_frame (out[3] counts those that are not: must be 0)
// — tested against every unit with filter_eval.h's forms over unit_eye (and
// the BVH units), the directions aimed as hc_filter_selftest aims them.
// out[0] = wrong certain verdicts against this build's eval64 (must be 0),
// out[1] = ambiguous verdicts, out[2] = tests.
int hc_rays_filter(const pt_scene_desc* d, const double* box, int64_t n_rays, uint64_t seed, int64_t* out) {
    HostScene H;
    if (!box || !open_scene(d, &H, nullptr, box)) return -1;
    int64_t outside = 0;
    filter_from(H, n_rays, seed, out, [&](int64_t i, std::mt19937_64& rng, std::uniform_real_distribution<double>& U) {
        D3 o = ld3(H.k.eye);
        if (i >= 1 && i <= 8) {
            const int c = (int)(i - 1);
            o = d3(box[c & 1 ? 3 : 0], box[c & 2 ? 4 : 1], box[c & 4 ? 5 : 2]);
        } else if (i > 8) {
            o = d3(box[0] + (box[3] - box[0]) * U(rng), box[1] + (box[4] - box[1]) * U(rng),
                   box[2] + (box[5] - box[2]) * U(rng));
        }
        if (!rays_in_frame(H.k, H.frame_x, o)) ++outside;
        return o;
    });
    out[3] = outside;
    return 0;
}

}  // extern "C"
