// pt_wf_bounce.h — the body of wf_begin_bounce (pt_wavefront.h), included
// once per camera: LENS (a constexpr of the including function, bounce's
// mode) selects the specular term's eye — 0 the scene's, 1 the sample's lens
// point in the record's rows kSpLens (wf_lens_start), 2 the origin of the
// slot's ray record, the three doubles at eye_o (wf_begin_bounce_rays; null
// in the other two, where bounce never reads it).  A text fragment rather than a
// template parameter: the body's constants are named after the function they
// stand in, and wf_begin_bounce<KEY> keeps its name and with it the text the
// kernels without a lens compile to.  No include guard.
// In scope: S, J, W, shq, cq; KEY, LENS, eye_o.
    const Spill sp{W->sp, 1};
    const D3 P = sp.get3(kSpP);
    const int tri = W->tri, b = W->b();
    const uint32_t sample = (uint32_t)(J.sample0 + W->si * J.sample_stride);
    const int obj = S.tri_obj[tri];
    const TriS R = S.tris[tri];
    const Mat& m = S.mat[obj];
    const int ogrp = S.tri_grp[tri];
    ShadowSet sh;
    uint32_t w[16];
#if PT_RNG_PERBLOCK   // as render_loop: one Philox block per light sample, where it is used
#pragma unroll
    for (int k = 0; k < kLightSamples; ++k) {
        uint32_t c[4];
        rng_block(J.seed, J.pixel, sample, (uint32_t)b, (uint32_t)k, c);
        shadow_setup_k<false, !PT_WF_LRNG>(S, P, ld3(R.n), k, u_of(c[0]), u_of(c[1]), u_of(c[2]),
                                           u_of(c[3]), &sh, sp);
    }
    sh.key2 = S.n_obj;
    sh.leak = S.n_obj - 1;
    rng_block(J.seed, J.pixel, sample, (uint32_t)b, 3u, &w[12]);
#else
    // (shadow_setup stores the light points into the home's kSpL slots, where
    // a PT_WF_LRNG record keeps its RNG key: the two switches exclude each
    // other)
    static_assert(!PT_WF_LRNG, "PT_WF_LRNG needs PT_RNG_PERBLOCK (the light points must not overwrite the key)");
    rng_blocks4(J.seed, J.pixel, sample, (uint32_t)b, w);
    {
        double u12[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) u12[i] = u_of(w[i]);
        shadow_setup<false>(S, P, ld3(R.n), u12, &sh, sp);
    }
#endif
    double kf;
    const D3 nd = bounce<LENS>(S, R, m, P, sp.get3(kSpNd), u_of(w[12]), u_of(w[13]), u_of(w[14]), &kf, &sp, eye_o);
    const double kn = W->k * kf;
    bool trace = (b + 1 < J.bounces);
    double kk = kn;
    if (trace && J.rr_depth >= 0 && b >= J.rr_depth) {   // build extension
        double q = fabs(kn);
        q = q < 0.05 ? 0.05 : (q > 1.0 ? 1.0 : q);
        if (u_of(w[15]) >= q) trace = false;
        else kk = kn / q;
    }
    sp.put3(kSpNd, nd);
    const F3 o32 = to_f3(P - ld3(S.kd + kKdCenter));      // the BVH's frame (the walks)
    const F3 o32u = to_f3(P - ld3(S.kd + kKdCenterS));   // the uniform units' frame
    const F3 n32 = to_f3(unit(nd));
    ClosestAcc ca = closest_init();
    const bool any_trace = PT_WAVE_ANY(trace);
    {
        float oc[kLightSamples] = {-1.0f, -1.0f, -1.0f};
        for (int u = 0; u < S.n_obj_unit; ++u) {
            const UnitF U = S.unit[u];
            const OriginU O = PT_QUAD ? origin_q(U, o32u) : origin_u(U, o32u);
            const bool do_shadow = PT_WAVE_ANY(!(oc[0] > 0.0f && oc[1] > 0.0f && oc[2] > 0.0f));
            fused_unit<false, false, true, 3, PT_WF_LRNG != 0>(S, U, O, U.grp == ogrp, do_shadow, any_trace,
                                                               &sh, n32, &ca, sp, nullptr, 15u, oc);
        }
#pragma unroll
        for (int k = 0; k < kLightSamples; ++k) sh.occ[k] = oc[k] > 0.0f;
    }
    if (any_trace) {
        for (int u = S.n_obj_unit; u < S.n_unit; ++u) {   // the light's units
            const UnitF U = S.unit[u];
            closest_unit<false>(S, U, origin_u(U, o32u), n32, U.grp == ogrp, sp, kSpP, kSpNd, &ca,
                                nullptr);
        }
    }
    uint32_t want = KEY ? wf_cell(S, o32) << 16 : 0u;
    wf_put_shadow(shq, o32, ogrp, sh);
    want |= shadow_open<false>(S, &sh);   // the rays still open, one walk each
    if (trace) {
        wf_put_closest(cq, o32, ogrp, n32, ca);
        want |= kWfWantClosest;
    }
#pragma unroll
    for (int k = 0; k < kLightSamples; ++k) W->ln[k] = sh.ln[k];
    W->kk = kk;
    W->set(kWfBounce, trace, b);
    return want;
