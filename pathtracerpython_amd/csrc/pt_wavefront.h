// pt_wavefront.h — the wavefront form of the render loop for scenes with a
// BVH (large meshes, BASELINE config K5).
//
// Why: in the single kernel (k_render) each lane runs its own BVH walks
// (bvh_shadow, bvh_closest) inside the bounce loop.  Walk lengths vary by
// orders of magnitude (an occluded shadow ray ends after a few nodes, an
// unoccluded one crosses the whole mesh), so a wave waits for its longest
// walk: measured VALU lane utilisation 9.7% on K5 (80% on the Cornell box).
// Here the bounce loop of main.py:186-271 is cut at the walks:
//
//   shade    (one work-item per path slot): finish the previous bounce with
//            the walks' results (colour, main.py:208-231; next hit,
//            main.py:197-205), then start the next bounce — RNG, light
//            samples, next ray (main.py:236-268), the fused pass over the
//            uniform units — and append the slot to the shadow / closest
//            query lists;
//   shadow   (persistent, dynamic fetch): the BVH shadow walks;
//   closest  (persistent, dynamic fetch): the BVH closest-hit walks.
//
// A query work-item takes the next query from its list (one atomic per wave)
// as soon as its walk ends, so the waves stay full until the list drains.
// The per-slot arithmetic is that of render_loop (pt_path.h) in the same
// order, so the framebuffer is bitwise identical to k_render's (tested).
// Path state lives in HBM between the kernels: WfPath (256 B per slot, the
// f64 spill home included) and the query records.
// With antialiasing (PT_FLAG_AA) a slot has no cached primary hit: every
// sample starts with its own closest query from the eye (wf_aa_start), issued
// by the shade step that ends the sample before it (wf_shade_aa).
// With the thin lens (PT_FLAG_LENS) likewise, from the sample's own lens point
// (wf_lens_start, wf_shade_lens), with or without PT_FLAG_AA.
#pragma once
#include <stddef.h>

#include "pt_job.h"   // (and pt_path.h)

namespace pt {

// kWfBegin: the slot's pending work is finished and its next bounce is to be
// started (the split shade step: wf_finish, then wf_begin_bounce)
enum : int32_t { kWfDone = 0, kWfPrimary = 1, kWfBounce = 2, kWfBegin = 3 };

// Two 128-B lines per slot: the first holds everything a shade step reads
// and writes (the per-step fields and the spill slots P, Nd), the second the
// slot's RNG key in the light-point slots (written once; PT_WF_LRNG: the f64
// fallbacks redraw a light point from it, Spill::light — with PT_WF_LRNG=0
// the points themselves, written per bounce) and the primary hit (read when
// a sample restarts).
struct alignas(128) WfPath {
    double acc[3];            // sum of this slot's sample colours
    double k, kk;             // throughput before / after the pending bounce
    double ln[kLightSamples]; // l_k . n of the pending bounce's light samples
    int32_t tri, tri0, si;    // the pending bounce's triangle, the primary hit's, the sample
    uint32_t sb;              // state | trace << 2 | b << 3 (the bounce index)
    double sp[kSpillSlots];   // the spill home of pt_path.h (Spill{sp, 1}): P, Nd | key (L), D0, P0
    double pad[2];
    PT_HD int state() const { return (int)(sb & 3u); }
    PT_HD bool trace() const { return ((sb >> 2) & 1u) != 0; }
    PT_HD int b() const { return (int)(sb >> 3); }
    PT_HD void set(int state, bool trace, int b) { sb = (uint32_t)state | (trace ? 4u : 0u) | ((uint32_t)b << 3); }
    // the slot's RNG key in the light-point slots (Spill::light)
    PT_HD void put_rkey(const LaneJob& J) {
        const uint64_t w[3] = {J.seed, (uint64_t)J.pixel | (uint64_t)(uint32_t)J.sample0 << 32,
                               (uint64_t)(uint32_t)J.sample_stride};
        __builtin_memcpy(&sp[kSpL], w, sizeof(w));
    }
};
static_assert(sizeof(WfPath) == 256, "WfPath is 256 B");
static_assert(offsetof(WfPath, si) + 8 == offsetof(WfPath, sp) && offsetof(WfPath, sb) + 4 == offsetof(WfPath, sp),
              "Spill::light reads si and sb just below the home");
static_assert(offsetof(WfPath, sp) + (kSpNd + 3) * sizeof(double) <= 128,
              "P and Nd in the first line");

// shadow walks: in = the state after the uniform units, out = the final
// state.  The one-ray walks of a query write disjoint fields: ray 0 / 1 its
// wocc entry, ray 2 bit 2 of occ and leak.
struct alignas(16) WfShadowQ {
    float o[3];
    int32_t ogrp;
    float d[kLightSamples][3];
    float hlo[kLightSamples], hhi[kLightSamples];
    int32_t occ;              // bit k: shadow ray k occluded (the uniform units; ray 2's walk)
    int32_t key2, leak;
    int32_t wocc[2];          // rays 0, 1: occluded by the BVH (their walks)
};
static_assert(sizeof(WfShadowQ) == 96, "WfShadowQ is 96 B");

// closest walk: in = the candidates of the uniform units, out = all candidates
struct alignas(16) WfClosestQ {
    float o[3];
    int32_t ogrp;
    float d[3];
    int32_t i1;
    float a1, a2, b1;
    int32_t pad;
};
static_assert(sizeof(WfClosestQ) == 48, "WfClosestQ is 48 B");

PT_HD void wf_put_shadow(WfShadowQ* q, F3 o32, int ogrp, const ShadowSet& sh) {
    q->o[0] = o32.x; q->o[1] = o32.y; q->o[2] = o32.z;
    q->ogrp = ogrp;
    int occ = 0;
#pragma unroll
    for (int k = 0; k < kLightSamples; ++k) {
        q->d[k][0] = sh.d32[k].x; q->d[k][1] = sh.d32[k].y; q->d[k][2] = sh.d32[k].z;
        q->hlo[k] = sh.hlo[k];
        q->hhi[k] = sh.hhi[k];
        occ |= sh.occ[k] ? 1 << k : 0;
    }
    q->occ = occ;
    q->key2 = sh.key2;
    q->leak = sh.leak;
    q->wocc[0] = q->wocc[1] = 0;
}
// the walk's view of a query (count-mode fields unused: the wavefront path
// does not count)
PT_HD void wf_get_shadow(const SceneK& S, const WfShadowQ& q, F3* o32, int* ogrp, ShadowSet* sh) {
    *o32 = F3{q.o[0], q.o[1], q.o[2]};
    *ogrp = q.ogrp;
#pragma unroll
    for (int k = 0; k < kLightSamples; ++k) {
        sh->d32[k] = F3{q.d[k][0], q.d[k][1], q.d[k][2]};
        sh->hlo[k] = q.hlo[k];
        sh->hhi[k] = q.hhi[k];
        sh->occ[k] = (q.occ >> k) & 1;
        sh->first[k] = S.n_tri;
        sh->ln[k] = 0.0;
    }
    sh->key2 = q.key2;
    sh->leak = q.leak;
}
// a one-ray walk's view of shadow ray k of a query
PT_HD void wf_get_shadow1(const WfShadowQ& q, int k, F3* o32, int* ogrp, Shadow1* r) {
    *o32 = F3{q.o[0], q.o[1], q.o[2]};
    *ogrp = q.ogrp;
    r->d32 = F3{q.d[k][0], q.d[k][1], q.d[k][2]};
    r->hlo = q.hlo[k];
    r->hhi = q.hhi[k];
    r->k = k;
    r->occ = false;   // (only open rays are walked)
    r->key2 = q.key2;
    r->leak = q.leak;
}
// its result into the query record (fields of ray k only)
// (only an occluded ray writes: wocc is 0 from wf_put_shadow, and a ray's
// leak changes only when it is occluded — an unoccluded ray's walk leaves
// the query record's lines untouched, PT_WF_PUT_OCC)
#ifndef PT_WF_PUT_OCC
#define PT_WF_PUT_OCC 1
#endif
PT_HD void wf_put_shadow1(WfShadowQ* q, const Shadow1& r) {
    if (PT_WF_PUT_OCC && !r.occ) return;
    if (r.k < kLightSamples - 1) {
        q->wocc[r.k] = r.occ ? 1 : 0;
    } else {
        if (r.occ) q->occ |= 1 << r.k;
        q->leak = r.leak;
    }
}
// list entries of the shadow walks: (slot << 2) | ray
PT_HD int32_t wf_shadow_entry(int32_t slot, int k) { return (slot << 2) | k; }

PT_HD void wf_put_closest(WfClosestQ* q, F3 o32, int ogrp, F3 d32, const ClosestAcc& c) {
    q->o[0] = o32.x; q->o[1] = o32.y; q->o[2] = o32.z;
    q->ogrp = ogrp;
    q->d[0] = d32.x; q->d[1] = d32.y; q->d[2] = d32.z;
    q->i1 = c.i1;
    q->a1 = c.a1; q->a2 = c.a2; q->b1 = c.b1;
}
PT_HD ClosestAcc wf_get_acc(const WfClosestQ& q) {
    ClosestAcc c;
    c.a1 = q.a1; c.a2 = q.a2; c.b1 = q.b1; c.i1 = q.i1;
    return c;
}

// What a shade step asks for next (bit k < 3: a walk of shadow ray k, bit 3:
// a closest walk)
enum : uint32_t { kWfWantShadow = 7u, kWfWantClosest = 8u };

// Start the slot (shade step 0): the primary ray's uniform part, as closest()
// does for it in k_render; the BVH part is a closest query.
PT_HD uint32_t wf_start(const SceneK& S, const LaneJob& J, D3 d0, WfPath* W, WfClosestQ* cq) {
    W->acc[0] = W->acc[1] = W->acc[2] = 0.0;
    W->set(kWfDone, false, 0);
    if (J.n_samples <= 0 || J.bounces <= 0) return 0;   // main.py:192 never runs
    const Spill sp{W->sp, 1};
    const D3 eye = ld3(S.eye);
    const D3 dn = unit(d0);
    sp.put3(kSpP, eye);
    sp.put3(kSpNd, d0);
    const F3 o32 = to_f3(eye - ld3(S.center));
    const F3 d32 = to_f3(dn);
    ClosestAcc acc = closest_init();
    for (int u = 0; u < S.n_unit; ++u) {   // from the eye: the unit_eye records
        const UnitF U = S.unit_eye[u];
        closest_unit<false>(S, U, origin_u(U, o32), d32, U.grp == -1, sp, kSpP, kSpNd, &acc,
                            nullptr);
    }
    wf_put_closest(cq, o32, -1, d32, acc);
    W->set(kWfPrimary, false, 0);
    return kWfWantClosest;
}

// Antialiasing (PT_FLAG_AA, pt_path.h AaRay): the slot has no cached primary
// hit.  Sample W->si starts with its own closest query from the eye along the
// jittered ray: wf_start's body for that d0, the candidates of the eye-frame
// units into the slot's own query record (walked like a bounce's query, the
// slot's spill home holding the eye and d0).  The eye units are tested in
// eye_closest's unit form (PT_WF_AA_PRIMARY_M: origin_q / closest_unit_m, the
// ambiguous members decided in f64) or in wf_start's per-triangle form; both
// are conservative filters in front of the same closest_finish.
#ifndef PT_WF_AA_PRIMARY_M
#define PT_WF_AA_PRIMARY_M (PT_AA_PRIMARY_M && PT_LIGHT_QUAD && PT_QUAD && PT_MARGIN)
#endif
PT_HD uint32_t wf_aa_start(const SceneK& S, const LaneJob& J, const AaPixel& X, WfPath* W,
                           WfClosestQ* cq) {
    const Spill sp{W->sp, 1};
    double jx, jy;
    aa_jitter(J.seed, J.pixel, (uint32_t)(J.sample0 + W->si * J.sample_stride), &jx, &jy);
    const D3 d0 = aa_dir(S, X.W, X.H, X.ix, X.iy, jx, jy);
    const D3 eye = ld3(S.eye);
    const D3 dn = unit(d0);
    sp.put3(kSpP, eye);
    sp.put3(kSpNd, d0);
    const F3 o32 = to_f3(eye - ld3(S.center));
    const F3 d32 = to_f3(dn);
    ClosestAcc acc = closest_init();
    for (int u = 0; u < S.n_unit; ++u) {   // from the eye: the unit_eye records
        const UnitF U = S.unit_eye[u];
#if PT_WF_AA_PRIMARY_M
        const OriginU O = origin_q(U, o32);
        if (closest_unit_m(U, O, U.grp == -1, d32, &acc))   // rare
            fused_fallback<false, false, true, 2>(S, U, closest_bits_m(U, O, U.grp == -1, d32), nullptr,
                                                  &acc, sp, nullptr, nullptr);
#else
        closest_unit<false>(S, U, origin_u(U, o32), d32, U.grp == -1, sp, kSpP, kSpNd, &acc,
                            nullptr);
#endif
    }
    wf_put_closest(cq, o32, -1, d32, acc);
    W->set(kWfPrimary, false, 0);
    return kWfWantClosest;
}

// The thin lens (PT_FLAG_LENS, pt_path.h LensRay): wf_aa_start with the
// lens rule.  Sample W->si starts at its own lens point eye' along lens_dir's
// ray; eye' is the query's origin (kSpP, which wf_finish reads back as the
// origin of closest_finish) and stays in the record's rows kSpLens for the
// sample's bounces (bounce<true>; these forms cache no primary hit, so the
// rows are free).  The eye units are tested in eye_closest's per-lane form
// from the slot's own origin.  AA: PT_FLAG_AA beside the lens, a template parameter
// down to the kernels (pt_path.h lens_point).
template <bool AA>
PT_HD uint32_t wf_lens_start(const SceneK& S, const LaneJob& J, const AaPixel& X, WfPath* W,
                             WfClosestQ* cq) {
    const Spill sp{W->sp, 1};
    double jx, jy, lx, ly;
    lens_point<AA>(J.seed, J.pixel, (uint32_t)(J.sample0 + W->si * J.sample_stride), S.kd[kKdLensR], &jx, &jy,
                   &lx, &ly);
    const D3 eye = d3(S.kd[kKdEye] + lx, S.kd[kKdEye + 1] + ly, S.kd[kKdEye + 2]);
    const D3 d0 = lens_dir(S, X.W, X.H, X.ix, X.iy, jx, jy, lx, ly, eye.x, eye.y);
    sp.put(kSpLens, eye.x);
    sp.put(kSpLens + 1, eye.y);
    const D3 dn = unit(d0);
    sp.put3(kSpP, eye);
    sp.put3(kSpNd, d0);
    const F3 o32 = to_f3(eye - ld3(S.kd + kKdCenter));
    const F3 d32 = to_f3(dn);
    ClosestAcc acc = closest_init();
    for (int u = 0; u < S.n_unit; ++u) {   // from the lens point: the unit_eye records
        const UnitF U = S.unit_eye[u];
#if PT_WF_AA_PRIMARY_M
        const OriginU O = origin_q(U, o32);
        if (closest_unit_m(U, O, U.grp == -1, d32, &acc))   // rare
            fused_fallback<false, false, true, 2>(S, U, closest_bits_m(U, O, U.grp == -1, d32), nullptr,
                                                  &acc, sp, nullptr, nullptr);
#else
        closest_unit<false>(S, U, origin_u(U, o32), d32, U.grp == -1, sp, kSpP, kSpNd, &acc,
                            nullptr);
#endif
    }
    wf_put_closest(cq, o32, -1, d32, acc);
    W->set(kWfPrimary, false, 0);
    return kWfWantClosest;
}

// The body of render_loop up to its walks: RNG, light samples, next
// ray, the fused pass over the uniform units (pt_path.h render_loop).
// The sort key of a query origin (the BVH frame; render_wavefront's sort):
// 4 bits per axis over the root node's grid, in Morton order (neighbouring
// cells get neighbouring keys)
PT_HD uint32_t wf_cell(const SceneK& S, F3 o) {
    if (S.qroot < 0) return 0;
    const QNode& Q = S.qnode[S.qroot];
    const float v[3] = {o.x, o.y, o.z};
    uint32_t c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float f = (v[a] - Q.org[a]) * (16.0f / (255.0f * q_step(Q.ex, a)));
        const int i = (int)f;
        c[a] = (uint32_t)(f > 0.0f ? (i > 15 ? 15 : i) : 0);
    }
    uint32_t m = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int a = 0; a < 3; ++a) m |= ((c[a] >> b) & 1u) << (3 * b + a);
    return m;
}
// KEY: the origin's cell in bits 16..27 of the result (the shade kernels take it off, pt_shade.hip)
// The body is pt_wf_bounce.h, once per camera (wf_begin_bounce_lens: the
// specular term's eye is the sample's lens point, wf_lens_start).
template <bool KEY = false>
PT_HD uint32_t wf_begin_bounce(const SceneK& S, const LaneJob& J, WfPath* W, WfShadowQ* shq,
                               WfClosestQ* cq) {
    constexpr bool LENS = false;
    constexpr const double* eye_o = nullptr;
#include "pt_wf_bounce.h"
}
template <bool KEY = false>
PT_HD uint32_t wf_begin_bounce_lens(const SceneK& S, const LaneJob& J, WfPath* W, WfShadowQ* shq,
                                    WfClosestQ* cq) {
    constexpr bool LENS = true;
    constexpr const double* eye_o = nullptr;
#include "pt_wf_bounce.h"
}
// caller-supplied rays: the eye is the record's origin (bounce<2>, RayHit::eye_o)
template <bool KEY = false>
PT_HD uint32_t wf_begin_bounce_rays(const SceneK& S, const LaneJob& J, const double* eye_o, WfPath* W,
                                    WfShadowQ* shq, WfClosestQ* cq) {
    constexpr int LENS = 2;
#include "pt_wf_bounce.h"
}

// Shade step >= 1, first half: finish the pending work of the slot with the
// walks' results (the colour, the next hit, path end / next sample).  Returns
// kWfNextBounce when the slot's next bounce is to be started (state kWfBegin;
// the second half is wf_begin_bounce), else kWfNextNone.  pq: the slot's
// primary query (one per pixel / entry, wf_primary_step)
//
// Home: where a path's colour goes when the path ends.  WfSum (the uniform
// render): nowhere, W->acc runs on over the slot's samples.  WfMoments (the
// list form, an accumulator pass): MomentSink's rule (pt_path.h) — the
// colour is added to the slot's six sums and W->acc restarts at 0, wherever
// `done` is set below; a primary ray that escapes or hits the light adds its
// constant n_samples times, as render_lane_cached does for a MomentSink.
struct WfSum { static constexpr bool kMoments = false; };
struct WfMoments : MomentMem { static constexpr bool kMoments = true; };
//
// AA (antialiasing): a primary query per sample, in the slot's own record cq
// (wf_aa_start), and nothing cached in kSpD0 / kSpP0 / tri0.  A sample whose
// primary ray escapes or hits the light is complete at once (Sched::start's
// order), and a path's end restarts from the eye.  Returns
// kWfNextPrimary when the slot's next sample is to be started in this shade
// step (wf_aa_start; d0 and pq are unused).
// LENS (the thin lens, wf_lens_start): AA's per-sample form whether or not the
// launch is antialiased (AA is then the jitter alone), the primary query's
// origin being the sample's lens point, which kSpP still holds.
// RAYS (caller-supplied rays, wf_rays_primary_step): the centre-ray form — a
// primary query per record, its hit cached in tri0 / kSpP0 — with the record
// `ray` in the place of (the job's d0, kSpD0, the scene's eye), as RayHit
// has it: the home keeps no direction, a sample's restart reads ray->d.  A
// record whose primary query was decided in f64 (pq->pad = kWfPrimF64) has
// issued no walk: its hit is in its first slot W0 (tri0, kSpP0).
enum : int { kWfNextNone = 0, kWfNextBounce = 1, kWfNextPrimary = 2 };
enum : int32_t { kWfPrimF32 = 0, kWfPrimF64 = 1 };   // WfClosestQ::pad of a record's primary query
template <class Home, bool AA = false, bool LENS = false, bool RAYS = false>
PT_HD int wf_finish(const SceneK& S, const LaneJob& J, D3 d0, WfPath* W, const WfShadowQ* shq,
                    const WfClosestQ* cq, const WfClosestQ* pq, Home home, const RayK* ray = nullptr,
                    const WfPath* W0 = nullptr) {
    const Spill sp{W->sp, 1};
    if constexpr (AA || LENS) {
        if (W->state() == kWfPrimary) {   // AaRay::primary: closest(eye, d0 of this sample)
            const D3 dj = sp.get3(kSpNd);
            D3 P0 = d3(0, 0, 0);
            D3 eye;
            if constexpr (LENS) eye = sp.get3(kSpP);   // LensRay::primary: from the sample's lens point
            else eye = ld3(S.eye);
            const int tri0 = closest_finish<false, false, true>(S, wf_get_acc(*cq), eye, unit(dj),
                                                                &P0, nullptr);
            if (tri0 >= 0 && tri0 < S.n_obj_tri) {
                W->set(kWfBegin, false, 0);   // (b = 0; begin_bounce sets the state)
                W->tri = tri0;
                W->k = 1.0;
                sp.put3(kSpP, P0);   // (kSpNd holds d0, the incoming direction of bounce 0)
                return kWfNextBounce;
            }
            // the sample is complete: 0, or the light's colour (main.py:214-215)
            if constexpr (Home::kMoments) {
                home.add(tri0 < 0 ? d3(0, 0, 0) : ld3(S.kd + kKdLightRgb));
            } else {
                if (tri0 >= 0) {
                    const D3 acc = ld3(W->acc) + ld3(S.kd + kKdLightRgb);
                    W->acc[0] = acc.x; W->acc[1] = acc.y; W->acc[2] = acc.z;
                }
            }
            const int si = W->si + 1;
            W->si = si;
            if (si < J.n_samples) return kWfNextPrimary;
            W->set(kWfDone, false, 0);
            return kWfNextNone;
        }
    } else
    if (W->state() == kWfPrimary) {   // k_render: closest(eye, d0) then render_lane_cached's prologue
        D3 P0 = d3(0, 0, 0);
        int tri0;
        if constexpr (RAYS) {
            d0 = ld3(ray->d);
            if (pq->pad == kWfPrimF64) {   // decided in f64 by the primary step
                tri0 = W0->tri0;
                P0 = ld3(W0->sp + kSpP0);
            } else {
                tri0 = closest_finish<false, false, true>(S, wf_get_acc(*pq), ld3(ray->o), unit(d0), &P0,
                                                          nullptr);
            }
        } else {
            tri0 = closest_finish<false, false, true>(S, wf_get_acc(*pq), ld3(S.eye), unit(d0), &P0, nullptr);
        }
        if (tri0 < 0 || tri0 >= S.n_obj_tri) {   // primary ray escapes or hits the light
            const D3 v = tri0 < 0 ? d3(0, 0, 0) : ld3(S.kd + kKdLightRgb);
            D3 acc = d3(0, 0, 0);
            if constexpr (Home::kMoments) {
                for (int i = 0; i < J.n_samples; ++i) home.add(v);
            } else {
                for (int i = 0; i < J.n_samples; ++i) acc = acc + v;
            }
            W->acc[0] = acc.x; W->acc[1] = acc.y; W->acc[2] = acc.z;
            W->set(kWfDone, false, 0);
            return kWfNextNone;
        }
        W->si = 0;
        W->set(kWfBegin, false, 0);   // (b = 0; begin_bounce sets the state)
        // (a record decided in f64: its first slot holds the hit already, and
        // the record's other slots read it there in this very step)
        bool own = true;
        if constexpr (RAYS) own = W != W0 || pq->pad != kWfPrimF64;
        W->tri = tri0;
        if (own) W->tri0 = tri0;
        W->k = 1.0;
        if constexpr (!RAYS) {   // (rays: the direction comes back from the record)
            sp.put(kSpD0, d0.x);
            sp.put(kSpD0 + 1, d0.y);
        }
        if (own) sp.put3(kSpP0, P0);
        sp.put3(kSpP, P0);
        sp.put3(kSpNd, d0);   // incoming direction of bounce 0 (main.py:191)
        return kWfNextBounce;
    }
    if (W->state() != kWfBounce) return kWfNextNone;
    // the colour of the pending bounce (main.py:208-231)
    ShadowSet sh;
#pragma unroll
    for (int k = 0; k < kLightSamples; ++k) {
        sh.occ[k] = (shq->occ >> k) & 1;
        sh.ln[k] = W->ln[k];
        sh.first[k] = S.n_tri;
    }
    sh.leak = shq->leak;
    for (int k = 0; k < kLightSamples - 1; ++k) sh.occ[k] = sh.occ[k] | (shq->wocc[k] != 0);
    const D3 col = shadow_color<false>(S, S.tri_obj[W->tri], sh, nullptr);   // the pending bounce's object
    D3 acc = ld3(W->acc);
    double k = W->k;
    acc = acc + col * k;   // main.py:230-231 (k before this bounce's update)
    k = W->kk;
    bool done = !W->trace();
    int tri = W->tri, b = W->b(), si = W->si;
    if (!done) {
        D3 Pn;
        const int tn = closest_finish<false, false, true>(S, wf_get_acc(*cq), sp.get3(kSpP),
                                                         unit(sp.get3(kSpNd)), &Pn, nullptr, &sp);
        if (tn < 0) {
            done = true;
        } else if (tn >= S.n_obj_tri) {   // light: main.py:214-215
            acc = acc + ld3(S.kd + kKdLightRgb) * k;
            done = true;
        } else {
            tri = tn;
            ++b;
        }
    }
    if (done) {
        if constexpr (Home::kMoments) {   // MomentSink::end
            home.add(acc);
            acc = d3(0, 0, 0);
        }
        ++si;
        if constexpr (AA || LENS) {   // next sample: its own primary query
            W->acc[0] = acc.x; W->acc[1] = acc.y; W->acc[2] = acc.z;
            W->si = si;
            if (si < J.n_samples) return kWfNextPrimary;
            W->set(kWfDone, false, 0);
            return kWfNextNone;
        } else
        if (si < J.n_samples) {   // next sample from the cached primary hit
            b = 0;
            tri = W->tri0;
            k = 1.0;
            sp.put3(kSpP, sp.get3(kSpP0));
            if constexpr (RAYS) sp.put3(kSpNd, ld3(ray->d));   // RayHit::restart
            else sp.put3(kSpNd, d3(sp.get(kSpD0), sp.get(kSpD0 + 1), 0.0 - S.eye[2]));
        }
    }
    W->acc[0] = acc.x; W->acc[1] = acc.y; W->acc[2] = acc.z;
    W->k = k;
    W->tri = tri;
    W->si = si;
    if (si >= J.n_samples) {
        W->set(kWfDone, false, 0);
        return kWfNextNone;
    }
    W->set(kWfBegin, false, b);   // (begin_bounce sets the state and trace)
    return kWfNextBounce;
}

// Shade step >= 1: wf_finish, then the next bounce's start.  Returns the
// queries wanted.  (One call site of wf_begin_bounce: round 4 started the
// next bounce from two, inlined twice — 141 instead of 113 VGPRs for
// k_wf_shade, the same time)
template <bool KEY = false, class Home = WfSum>
PT_HD uint32_t wf_shade(const SceneK& S, const LaneJob& J, D3 d0, WfPath* W, WfShadowQ* shq,
                        WfClosestQ* cq, const WfClosestQ* pq, Home home = Home{}) {
    return wf_finish(S, J, d0, W, shq, cq, pq, home) == kWfNextBounce ? wf_begin_bounce<KEY>(S, J, W, shq, cq) : 0u;
}
// The antialiased shade step: after wf_finish either the next bounce's start
// or the next sample's primary query (X: the slot's pixel, for aa_dir).
template <bool KEY = false, class Home = WfSum>
PT_HD uint32_t wf_shade_aa(const SceneK& S, const LaneJob& J, const AaPixel& X, WfPath* W, WfShadowQ* shq,
                           WfClosestQ* cq, Home home = Home{}) {
    const int next = wf_finish<Home, true>(S, J, d3(0, 0, 0), W, shq, cq, nullptr, home);
    if (next == kWfNextBounce) return wf_begin_bounce<KEY>(S, J, W, shq, cq);
    return next == kWfNextPrimary ? wf_aa_start(S, J, X, W, cq) : 0u;
}
// The thin-lens shade step: wf_shade_aa with the lens's sample start and the
// specular term's eye (AA: PT_FLAG_AA beside the lens).
template <bool KEY, bool AA, class Home = WfSum>
PT_HD uint32_t wf_shade_lens(const SceneK& S, const LaneJob& J, const AaPixel& X, WfPath* W, WfShadowQ* shq,
                             WfClosestQ* cq, Home home = Home{}) {
    const int next = wf_finish<Home, AA, true>(S, J, d3(0, 0, 0), W, shq, cq, nullptr, home);
    if (next == kWfNextBounce) return wf_begin_bounce_lens<KEY>(S, J, W, shq, cq);
    return next == kWfNextPrimary ? wf_lens_start<AA>(S, J, X, W, cq) : 0u;
}

// The ray shade step: wf_shade with the record (W0: the record's first slot).
template <bool KEY = false, class Home = WfSum>
PT_HD uint32_t wf_shade_rays(const SceneK& S, const LaneJob& J, const RayK* ray, WfPath* W, const WfPath* W0,
                             WfShadowQ* shq, WfClosestQ* cq, const WfClosestQ* pq, Home home = Home{}) {
    return wf_finish<Home, false, false, true>(S, J, d3(0, 0, 0), W, shq, cq, pq, home, ray, W0) == kWfNextBounce
               ? wf_begin_bounce_rays<KEY>(S, J, ray->o, W, shq, cq)
               : 0u;
}

// Where the slots of a launch get their jobs (pt_job.h): the pixels of a
// frame, `split` slots each, the entries of an accumulator pass's active
// list, or the records of a ray batch (kRays: no pixel, ix or iy; the job
// carries the record).  n_prim(): the launch's primary queries, one per pixel
// / entry / record.
struct WfFrame {
    static constexpr bool kRays = false;
    const RenderK& R;
    PT_HD SlotJob job(const SceneK& S, uint32_t tid) const { return slot_job(S, R, tid); }
    PT_HD uint32_t n_prim() const { return R.npix; }
};
struct WfActive {
    static constexpr bool kRays = false;
    const ListK& R;
    const uint32_t* list;
    const uint32_t* accN;
    PT_HD ListJob job(const SceneK& S, uint32_t tid) const { return list_job(S, R, list, accN, tid); }
    PT_HD uint32_t n_prim() const { return R.n_list; }
};

struct WfRays {
    static constexpr bool kRays = true;
    const RaysK& R;
    const RayK* rays;
    PT_HD RayJob job(const SceneK&, uint32_t tid) const { return rays_job(R, rays, tid); }
    PT_HD uint32_t n_prim() const { return R.n_rays; }
};

// The primary query of pixel / entry `entry` (centre rays: its `split` slots
// share it, main.py:191): the uniform part of the eye ray into CQP[entry],
// the spill home in the entry's first slot.  Returns the queries wanted.
template <class Src>
PT_HD uint32_t wf_primary_step(const SceneK& S, const Src& src, uint32_t entry, WfPath* W, WfClosestQ* CQP) {
    if (entry >= src.n_prim()) return 0u;
    const uint32_t slot = entry << src.R.split_log2;
    const auto j = src.job(S, slot);
    return j.valid ? wf_start(S, j.J, j.d0, &W[slot], &CQP[entry]) : 0u;
}

// The primary query of record `entry` of a ray batch (its `split` slots share
// it): wf_start's body from the record's origin, in eye_closest's unit form
// (per-lane origin_q over unit_eye) — what rays_primary runs for an origin
// inside the f32 filter's frame; the home rows kSpP / kSpNd of the entry's
// first slot get o and d.  An origin outside the frame (a NaN included,
// rays_in_frame): the query is decided here in f64, once per record, as
// closest<true, false, true> decides it in k_render_rays; no walk is issued,
// tri0 and P0 stay in the first slot's record and CQP[entry].pad says so.
// Returns the queries wanted.
PT_HD uint32_t wf_rays_primary_step(const SceneK& S, const WfRays& src, uint32_t entry, WfPath* W,
                                    WfClosestQ* CQP) {
    if (entry >= src.n_prim()) return 0u;
    const uint32_t slot = entry << src.R.split_log2;
    const RayJob j = src.job(S, slot);
    if (j.J.n_samples <= 0 || j.J.bounces <= 0) return 0u;   // (wf_start: main.py:192 never runs)
    WfPath* const W0 = &W[slot];
    WfClosestQ* const cq = &CQP[entry];
    const Spill sp{W0->sp, 1};
    const D3 o = ld3(j.ray->o), d0 = ld3(j.ray->d);
    if (!rays_in_frame(S, src.R.frame_x, o)) {
        D3 P0 = d3(0, 0, 0);
        W0->tri0 = closest<true, false, true>(S, o, d0, -1, sp, &P0, nullptr, true);
        sp.put3(kSpP0, P0);
        cq->pad = kWfPrimF64;
        return 0u;
    }
    const D3 dn = unit(d0);
    sp.put3(kSpP, o);
    sp.put3(kSpNd, d0);
    const F3 o32 = to_f3(o - ld3(S.kd + kKdCenter));
    const F3 d32 = to_f3(dn);
    ClosestAcc acc = closest_init();
    for (int u = 0; u < S.n_unit; ++u) {   // the unit_eye records, from the record's origin
        const UnitF U = S.unit_eye[u];
#if PT_WF_AA_PRIMARY_M
        const OriginU O = origin_q(U, o32);
        if (closest_unit_m(U, O, U.grp == -1, d32, &acc))   // rare
            fused_fallback<false, false, true, 2>(S, U, closest_bits_m(U, O, U.grp == -1, d32), nullptr,
                                                  &acc, sp, nullptr, nullptr);
#else
        closest_unit<false>(S, U, origin_u(U, o32), d32, U.grp == -1, sp, kSpP, kSpNd, &acc,
                            nullptr);
#endif
    }
    wf_put_closest(cq, o32, -1, d32, acc);
    cq->pad = kWfPrimF32;
    return kWfWantClosest;
}

// One shade step of slot tid < slots (the four shade kernels' body, and the
// host checks').  Returns the queries wanted, the shadow list's sort key
// (wf_cell) in bits 16..27.
// Step 0 initialises the slot, and its sums where the home has some: the
// buffers hold the state of an earlier pass or render.  Centre rays: the
// primary queries are wf_primary_step's, one per pixel / entry.  AA: no shared
// primary query — step 0 starts the slot's first sample's own, and every
// later sample starts in the step that ends the one before it.
// Later steps: a finished slot costs one load, its job is only built when it
// runs.
// LENS (the thin lens): AA's form — a primary query per sample — whether or
// not the launch is antialiased, started by wf_lens_start.
template <bool AA, bool LENS = false, class Src, class Home>
PT_HD uint32_t wf_slot_step(const SceneK& S, const Src& src, int32_t step, uint32_t tid, WfPath* W,
                            WfShadowQ* SQ, WfClosestQ* CQ, const WfClosestQ* CQP, Home home) {
    const uint32_t entry = tid >> src.R.split_log2;
    uint32_t want = 0;
    if (step == 0) {
        auto j = src.job(S, tid);
        if constexpr (Home::kMoments) home.clear();
        W[tid].acc[0] = W[tid].acc[1] = W[tid].acc[2] = 0.0;
        W[tid].put_rkey(j.J);
        const bool go = j.valid && j.J.n_samples > 0 && j.J.bounces > 0;
        if constexpr (AA || LENS) {
            W[tid].si = 0;
            W[tid].set(kWfDone, false, 0);
            j.J.seed = src.R.seed;   // (wave-uniform: aa_jitter's rng_block takes its key in scalar registers)
            if constexpr (LENS) {
                if (go) want = wf_lens_start<AA>(S, j.J, AaPixel{src.R.W, src.R.H, j.ix, j.iy}, &W[tid], &CQ[tid]);
            } else {
                if (go) want = wf_aa_start(S, j.J, AaPixel{src.R.W, src.R.H, j.ix, j.iy}, &W[tid], &CQ[tid]);
            }
        } else {
            W[tid].set(go ? kWfPrimary : kWfDone, false, 0);
        }
    } else if (entry < src.n_prim() && W[tid].state() != kWfDone) {
        auto j = src.job(S, tid);
        if constexpr (LENS) {
            j.J.seed = src.R.seed;   // (as in step 0; the slot is valid)
            want = wf_shade_lens<true, AA>(S, j.J, AaPixel{src.R.W, src.R.H, j.ix, j.iy}, &W[tid], &SQ[tid],
                                           &CQ[tid], home);
        } else if constexpr (AA) {
            j.J.seed = src.R.seed;   // (as in step 0; the slot is valid)
            want = wf_shade_aa<true>(S, j.J, AaPixel{src.R.W, src.R.H, j.ix, j.iy}, &W[tid], &SQ[tid], &CQ[tid],
                                     home);
        } else if constexpr (Src::kRays) {
            want = wf_shade_rays<true>(S, j.J, j.ray, &W[tid], &W[entry << src.R.split_log2], &SQ[tid], &CQ[tid],
                                       &CQP[entry], home);
        } else {
            want = wf_shade<true>(S, j.J, j.d0, &W[tid], &SQ[tid], &CQ[tid], &CQP[entry], home);
        }
    }
    return want;
}

}  // namespace pt
