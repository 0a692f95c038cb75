// pt_rays_list_host.cpp — TEST INFRASTRUCTURE.  A ray accumulator's list pass
// (pt_job.h rays_list_job, the mapping k_render_rays_list runs; pt_path.h
// rays_primary, RayHit with MomentSink through render_lane_cached) compiled for
// the host on top of pt_rays_host.cpp, so the CPU suite can check the mapping
// for every work-item and a whole adaptive run over ray records against the
// oracle without a GPU.  Built by tests/test_rays_adaptive_host.py into a
// temporary directory by the hostcheck Makefile's pattern rule (tests/hostlib.py).
#include "pt_rays_host.cpp"

namespace {
// the pass's record as pt_accum_render fills it (rays_list_record), with `split` lanes per record
RaysListK list_record(const pt_render_params* p, const pt_adapt_params* ap, uint32_t split, uint32_t n_list,
                      uint32_t n_rays, double frame_x) {
    const PlanAccum acc{(int32_t)n_rays, 1, n_rays, split, true, -1, -1};
    const PlanScene sc{false, false, 256, false, frame_x};
    const AdaptK A{ap->tol, ap->floor, (uint32_t)ap->min_spp, (uint32_t)ap->max_spp, (uint32_t)ap->step_spp};
    return rays_list_record(p, acc, sc, A, n_list, split);
}
}  // namespace

extern "C" {

// rays_list_job of work-items 0 .. n_tid-1 of a launch: out[tid] = {valid, e,
// k, the record's index (-1: none), J.pixel, J.sample0, J.sample_stride,
// J.n_samples, J.bounces, J.rr_depth} (int64 each); seed_out[tid] = J.seed.
int hc_rays_list_job(const RayK* rays, uint32_t n_rays, const pt_render_params* p, const pt_adapt_params* ap,
                     uint32_t split, const uint32_t* list, uint32_t n_list, const uint32_t* accN, uint32_t n_tid,
                     int64_t* out, uint64_t* seed_out) {
    if (split < 1 || (split & (split - 1))) return -2;
    const RaysListK R = list_record(p, ap, split, n_list, n_rays, 0.0);
    for (uint32_t tid = 0; tid < n_tid; ++tid) {
        const RayListJob j = rays_list_job(R, rays, list, accN, tid);
        int64_t* o = out + (size_t)tid * 10;
        o[0] = j.valid ? 1 : 0;
        o[1] = (int64_t)j.e;
        o[2] = (int64_t)j.k;
        o[3] = j.ray ? (int64_t)(j.ray - rays) : -1;
        o[4] = (int64_t)j.J.pixel;
        o[5] = j.J.sample0;
        o[6] = j.J.sample_stride;
        o[7] = j.J.n_samples;
        o[8] = j.J.bounces;
        o[9] = j.J.rr_depth;
        seed_out[tid] = j.J.seed;
    }
    return 0;
}

// One pass of k_render_rays_list on the host: the work-items of the launch
// (whole blocks of 64, as the kernel's grid) mapped by rays_list_job, each
// lane's primary hit by rays_primary and its paths by render_lane_cached
// (RayHit, MomentSink), an entry's `split` lanes reduced in the kernel's
// xor order and added to S, Q ([n_rays][3]) and n by lane 0.
int hc_rays_list_pass(const pt_scene_desc* d, const double* box, const RayK* rays, uint32_t n_rays,
                      const pt_render_params* p, const pt_adapt_params* ap, int force64, uint32_t split,
                      const uint32_t* list, uint32_t n_list, double* S, double* Q, uint32_t* n) {
    Host h;
    if (!h.open(d, nullptr, box)) return -1;
    if (split < 1 || split > 64 || (split & (split - 1))) return -2;
    const RaysListK R = list_record(p, ap, split, n_list, n_rays, h.H.frame_x);
    const uint64_t threads = ((((uint64_t)n_list << R.split_log2) + 63u) / 64u) * 64u;
    std::vector<uint32_t> n0(n, n + n_rays);   // every lane of the launch reads n before any lane 0 writes it
    for (uint64_t base = 0; base < threads; base += split) {
        std::vector<D3> s(split), q(split);
        RayListJob j0{};
        for (uint32_t l = 0; l < split; ++l) {
            const RayListJob j = rays_list_job(R, rays, list, n0.data(), (uint32_t)(base + l));
            if (l == 0) j0 = j;
            MomentRegs M;
            M.clear();
            if (j.valid)
                with_bool(force64 != 0, [&](auto F64) {
                    D3 P0;
                    const RayHit hit = ray_hit<decltype(F64)::value>(h, R.frame_x, j.ray,
                                                                     j.J.n_samples > 0 && R.bounces > 0, &P0);
                    run_lane<decltype(F64)::value, false>(h, j.J, hit, P0, MomentSink<MomentRegs>{M});
                });
            s[l] = M.sum();
            q[l] = M.sumsq();
        }
        if (j0.valid && j0.k > 0) {
            add3(S + (size_t)j0.e * 3, xor_reduce(s));
            add3(Q + (size_t)j0.e * 3, xor_reduce(q));
            n[j0.e] += j0.k;
        }
    }
    return 0;
}

}  // extern "C"
