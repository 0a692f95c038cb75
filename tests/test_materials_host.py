"""The material scenes (tests/material_scenes.py) on the host: exponents that
are no small integer, kd = 0, ks = 0 — the general pow behind pow_ref
(pt_core.h), the `nint` rule (pt_prepare.h) and the NaN samples that
np.float64 ** float gives for a negative base and a fractional exponent.
The oracle against the reference's own renders of these scenes
(tests/golden/mat_*.npz, gen_golden.py materials), the host build of the lane
code against the oracle per sample with equal NaN positions, the share of NaN
sample-pixels the frames hold, and the accumulator's moments and stop rule on
NaN sums.  The GPU cases are tests/test_gpu_materials.py."""
import ctypes as C
import glob
import math
import os

import numpy as np
import pytest

import hostlib
import material_scenes as ms
from adaptive_sim import active_numpy, err_numpy, histogram, k_numpy, simulate
from conftest import GOLDEN, hc_render
from material_scenes import compare
from oracle import oracle
from pathtracerpython_amd._abi import PT_FLAG_RR, make_params
from pathtracerpython_amd.pack import pack_scene
from pathtracerpython_amd.render import from_list_order

TOL = 1e-12
RR_MODES = [(False, 3), (True, 1)]
RULE = (4, 16, 4)            # min_spp, max_spp, step_spp of the adaptive cases
ADAPT_TOL, FLOOR = 0.05, 0.01
_dp = C.POINTER(C.c_double)
_up = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """{case: (scene, packed)}"""
    out = {}
    for case in ms.SCENES:
        sc = ms.material_scene(tmp_path_factory.mktemp("mat_" + case), case)
        out[case] = (sc, pack_scene(sc))
    return out


@pytest.fixture(scope="module")
def frames(scenes):
    """{(case, rr, rr_depth): (per-sample frames, their counters)} of the oracle."""
    return {(case, rr, rd): ms.oracle_frames(scenes[case][1], case, rr, rd)
            for case in ms.SCENES for rr, rd in RR_MODES}


@pytest.fixture(scope="module")
def mat_host(tmp_path_factory):
    """tests/hostcheck/pt_material_host.cpp (the lane code, the accumulator's
    and the material helpers) built by the hostcheck Makefile into a temporary
    directory."""
    lib = hostlib.build(tmp_path_factory.mktemp("mat_host"), "pt_material_host")
    lib.hc_render.restype = C.c_int
    lib.hc_render_wavefront.restype = C.c_int
    lib.hc_render_moments.restype = C.c_int
    lib.hc_adapt_rule.restype = C.c_int
    lib.hc_adapt_rule.argtypes = [_dp, _dp, _up, C.c_int64, C.c_double, C.c_double, C.c_uint32,
                                  C.c_uint32, C.c_uint32, _dp, C.POINTER(C.c_uint8), _up]
    lib.hc_mat_nint.restype = C.c_int
    lib.hc_pow_ref.restype = C.c_int
    lib.hc_pow_ref.argtypes = [C.c_void_p, C.c_int32, _dp, C.c_int64, _dp]
    return lib


# ------------------------------------------------ the reference's renders --
def golden_files():
    return sorted(os.path.basename(f) for f in glob.glob(os.path.join(GOLDEN, "mat_*.npz")))


def test_the_four_fixtures_are_there():
    assert golden_files() == ["mat_frac_12x12_s2_b4_seed5.npz", "mat_mesh_10x10_s2_b4_seed5.npz",
                              "mat_neg_12x12_s2_b4_seed5.npz", "mat_zero_12x12_s2_b4_seed5.npz"]


@pytest.mark.parametrize("name", golden_files())
def test_oracle_equals_the_reference(scenes, name):
    """The scene the writer gives here is the one the reference rendered
    (its material table), and the oracle's frame is the reference's: NaN
    pixels where np.float64 ** float gave them."""
    g = np.load(os.path.join(GOLDEN, name))
    case = name.split("_")[1]
    sc, pk = scenes[case]
    assert np.array_equal(ms.material_table(sc), g["materials"])
    assert np.array_equal(np.asarray(pk.mat).reshape(-1, 8), g["materials"])
    W, H, spp, B, seed = (int(g[k]) for k in ("width", "height", "spp", "bounces", "seed"))
    ref, _ = oracle.render(pk, W, H, spp, B, seed)
    nan, worst = compare(ref, g["colors"], TOL, name)
    print(f"{name}: {nan // 3} NaN pixels of {W * H}, finite pixels to {worst:.3e}")
    assert (nan > 0) == (case in ms.NAN_SCENES)
    assert nan < 3 * W * H


# ------------------------------------------------------ exposure condition --
@pytest.mark.parametrize("case", ms.SCENES)
def test_share_of_nan_sample_pixels(frames, case):
    """5 .. 35 % of the sample-pixels of frac, neg and the mesh scene are NaN:
    enough that the path is exercised, few enough that the comparison of the
    finite ones carries weight; none in big, edge16 and zero.  With Russian
    roulette fewer of them reach a pixel, never none."""
    f, _ = frames[(case, False, 3)]
    frr, _ = frames[(case, True, 1)]
    share, share_rr = ms.nan_share(f), ms.nan_share(frr)
    print(f"{case}: NaN sample-pixels {share:.3f}, with RR at depth 1 {share_rr:.3f}")
    assert not np.isinf(f).any() and not np.isinf(frr).any()
    # a NaN sample is NaN in every channel (the throughput is a scalar)
    assert np.array_equal(np.isnan(f).any(axis=-1), np.isnan(f).all(axis=-1))
    if case in ms.NAN_SCENES:
        assert 0.05 <= share <= 0.35
        assert 0.0 < share_rr < share
    else:
        assert share == 0.0 and share_rr == 0.0


# --------------------------------------------------------- the lane code --
@pytest.mark.parametrize("rr,rr_depth", RR_MODES, ids=["norr", "rr1"])
@pytest.mark.parametrize("case", ms.SCENES)
def test_host_build_equals_the_oracle_per_sample(mat_host, scenes, frames, case, rr, rr_depth):
    """hc_render, hybrid and forced f64, the count-mode lane code and the
    render kernel's own: every per-sample frame under compare(1e-12), hybrid
    == forced f64 bit for bit, and the oracle's work counters."""
    pk = scenes[case][1]
    ref, ostats = frames[(case, rr, rr_depth)]
    W, H, B, seed = ms.FRAME
    worst = 0.0
    for s in range(len(ref)):
        p = make_params(W, H, 1, B, seed, PT_FLAG_RR if rr else 0, rr_depth, sample_begin=s)
        a, st = hc_render(mat_host, pk, p, False, count=True)
        b, st64 = hc_render(mat_host, pk, p, True, count=True)
        c, _ = hc_render(mat_host, pk, p, False, count=False)
        d, _ = hc_render(mat_host, pk, p, True, count=False)
        what = f"{case} sample {s} rr {rr}"
        worst = max(worst, compare(a, ref[s], TOL, what)[1], compare(c, ref[s], TOL, what)[1])
        assert ms.same_bits(a, b) and ms.same_bits(c, d), what
        for k in ms.COUNTERS:
            assert st[k] == ostats[s][k] == st64[k], (what, k)
    print(f"{case} rr {rr}: host build vs oracle {worst:.3e}")


@pytest.mark.parametrize("rr,rr_depth", RR_MODES, ids=["norr", "rr1"])
def test_mesh_wavefront_form_equals_the_lane_code(mat_host, scenes, frames, rr, rr_depth):
    """The wavefront shade step has its own copy of the throughput update and
    the roulette (pt_wavefront.h): bit for bit the lane code's, NaN included."""
    pk = scenes["mesh"][1]
    info = (C.c_int32 * 6)()
    assert mat_host.hc_bvh_info(C.byref(pk.desc), info) == 0 and info[0] > 1
    W, H, B, seed = ms.FRAME
    ref, _ = frames[("mesh", rr, rr_depth)]
    for s in range(len(ref)):
        p = make_params(W, H, 1, B, seed, PT_FLAG_RR if rr else 0, rr_depth, sample_begin=s)
        lane, _ = hc_render(mat_host, pk, p, False, count=False)
        out = np.zeros((H, W, 3))
        assert mat_host.hc_render_wavefront(C.byref(pk.desc), C.byref(p), out.ctypes.data_as(_dp),
                                            None, None) == 0
        assert ms.same_bits(out, lane)
        compare(out, ref[s], TOL, f"mesh wavefront sample {s}")


def test_zero_throughput_ends_the_colour(mat_host, scenes):
    """zero: a path that meets cube2 (kd = ks = 0) first adds nothing
    afterwards — 5 bounces give those pixels what 1 bounce gives them."""
    pk = scenes["zero"][1]
    W, H, B, seed = ms.FRAME
    first = ms.first_hit_objects(pk, W, H) == ms.CUBE2
    assert 10 <= first.sum() < W * H // 2
    for s in range(2):
        deep, _ = hc_render(mat_host, pk, make_params(W, H, 1, B, seed, sample_begin=s), False,
                            count=False)
        one, _ = hc_render(mat_host, pk, make_params(W, H, 1, 1, seed, sample_begin=s), False,
                           count=False)
        o1, _ = oracle.render(pk, W, H, 1, 1, seed, sample_begin=s)
        assert np.isfinite(deep).all()
        assert np.array_equal(deep[first], one[first])
        assert np.abs(one - from_list_order(o1, W, H)).max() <= TOL
        assert not np.array_equal(deep[~first], one[~first])


# ------------------------------------------------------- nint and pow_ref --
def test_nint_rule_and_pow_ref(mat_host, scenes):
    """Exponents 0 .. 16 that are integers take the multiply loop, everything
    else the general pow: Mat::nint of every material here, and pow_ref bit
    for bit the loop's product or libm's pow (NaN for a negative base and a
    fractional exponent, as numpy)."""
    x = np.array([-1.0, -0.83, -0.5, -1e-3, 0.25, 0.5, 0.77, 0.999, 1.0])
    seen = set()
    for case in ms.SCENES:
        pk = scenes[case][1]
        n_obj = len(pk.mat)
        nint = np.zeros(n_obj, dtype=np.int32)
        assert mat_host.hc_mat_nint(C.byref(pk.desc), nint.ctypes.data_as(C.POINTER(C.c_int32))) == 0
        for o in range(n_obj):
            n = float(np.asarray(pk.mat).reshape(-1, 8)[o, 7])
            loop = n >= 0 and n <= 16 and n == math.floor(n)
            assert nint[o] == (int(n) if loop else -1), (case, o, n)
            out = np.zeros(len(x))
            assert mat_host.hc_pow_ref(C.addressof(pk.desc), o, x.ctypes.data_as(_dp), len(x),
                                       out.ctypes.data_as(_dp)) == 0
            for xi, got in zip(x, out):
                if loop:
                    want = 1.0
                    for _ in range(int(n)):
                        want *= float(xi)
                else:
                    with np.errstate(invalid="ignore"):
                        want = float(np.float64(xi) ** n)    # main.py:264
                assert (math.isnan(want) and math.isnan(got)) or want == got, (case, n, xi, got, want)
                # and the loop's product is numpy's power to rounding
                with np.errstate(invalid="ignore"):
                    ref = float(np.float64(xi) ** n)
                assert math.isnan(ref) == math.isnan(got)
                assert math.isnan(ref) or abs(got - ref) <= 1e-14 * max(1.0, abs(ref))
            seen.add(n)
    assert {0.0, 1.0, 5.0, 16.0, 17.0, 40.0, 0.5, 2.5, -1.0, -2.5} <= seen


# ------------------------------------------------------ the accumulator --
def host_moments(lib, packed, p):
    H, W = p.height, p.width
    S, Q = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    n = np.zeros((H, W), dtype=np.uint32)
    assert lib.hc_render_moments(C.byref(packed.desc), C.byref(p), 0, 0, S.ctypes.data_as(_dp),
                                 Q.ctypes.data_as(_dp), n.ctypes.data_as(_up)) == 0
    return S, Q, n


def host_rule(lib, S, Q, n, tol, floor, rule):
    shape = n.shape
    S, Q = np.ascontiguousarray(S), np.ascontiguousarray(Q)
    n = np.ascontiguousarray(n, dtype=np.uint32)
    err = np.zeros(shape)
    act = np.zeros(shape, dtype=np.uint8)
    k = np.zeros(shape, dtype=np.uint32)
    assert lib.hc_adapt_rule(S.ctypes.data_as(_dp), Q.ctypes.data_as(_dp), n.ctypes.data_as(_up),
                             n.size, tol, floor, *rule, err.ctypes.data_as(_dp),
                             act.ctypes.data_as(C.POINTER(C.c_uint8)), k.ctypes.data_as(_up)) == 0
    return err, act.astype(bool), k


def test_moments_and_stop_rule_on_nan_sums(mat_host, scenes, frames):
    """frac: S, Q, n of the host accumulator against the oracle's per-sample
    sums (NaN where a sample was NaN); moment_err (fmax) and adaptive_sim
    (np.maximum) end at the same err, NaN at the same pixels; a pixel whose S
    is NaN is listed exactly while n < min_spp."""
    pk = scenes["frac"][1]
    c, _ = frames[("frac", False, 3)]
    W, H, B, seed = ms.FRAME
    S, Q, n = host_moments(mat_host, pk, make_params(W, H, len(c), B, seed))
    wS, wQ = c[0].copy(), c[0] ** 2
    for s in range(1, len(c)):
        wS, wQ = wS + c[s], wQ + c[s] ** 2
    nan_px = np.isnan(wS).any(axis=-1)
    assert 20 <= nan_px.sum() < W * H // 2
    compare(S, wS, TOL, "S")
    compare(Q, wQ, TOL, "Q")
    assert (n == len(c)).all()
    for n_now in (2, 3, 4, 5, 16):
        nn = np.full((H, W), n_now, dtype=np.uint32)
        err, act, k = host_rule(mat_host, S, Q, nn, ADAPT_TOL, FLOOR, RULE)
        want = err_numpy(S, Q, nn, FLOOR)
        assert np.array_equal(np.isnan(err), nan_px)
        assert ms.same_bits(err, want)
        assert np.array_equal(act, active_numpy(nn, want, ADAPT_TOL, RULE[0], RULE[1]))
        assert np.array_equal(act[nan_px], np.full(int(nan_px.sum()), n_now < RULE[0]))
        assert np.array_equal(k, k_numpy(nn, *RULE))
    # below two samples err is +inf whatever S holds
    err, act, _ = host_rule(mat_host, S, Q, np.ones((H, W), dtype=np.uint32), ADAPT_TOL, FLOOR, RULE)
    assert np.isinf(err).all() and act.all()


def test_host_adaptive_run_equals_the_simulation(mat_host, scenes):
    """A whole adaptive run on frac with the host build's samples and the
    select's own rule (hc_adapt_rule): the count map, S, Q and err of
    adaptive_sim on the oracle's frames.  A pixel stops at min_spp when a NaN
    came within its first min_spp samples, else at the end of the pass that
    brought one."""
    pk = scenes["frac"][1]
    W, H, B, seed = ms.FRAME
    mn, mx, st = RULE
    c, _ = ms.oracle_frames(pk, "frac", n_samples=mx)
    sim = simulate(c, ADAPT_TOL, FLOOR, mn, mx, st)
    print(f"frac adaptive: counts {histogram(sim['n'])}, passes {sim['passes']}, "
          f"margin {sim['margin']:.3e}")
    assert sim["margin"] >= 1e-6          # sums 1e-12 apart flip no stop decision
    host = np.stack([host_moments(mat_host, pk, make_params(W, H, 1, B, seed, sample_begin=s))[0]
                     for s in range(mx)])
    compare(host, c, TOL, "per-sample frames")
    n = np.zeros((H, W), dtype=np.uint32)
    S, Q = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    passes = []
    while True:
        err, act, k = host_rule(mat_host, S, Q, n, ADAPT_TOL, FLOOR, RULE)
        if not act.any():
            break
        assert len(passes) < mx
        k = np.where(act, k, 0)
        passes.append((int(act.sum()), int(k.sum())))
        for e in zip(*np.nonzero(act)):
            for s in range(int(n[e]), int(n[e] + k[e])):
                S[e] += host[s][e]
                Q[e] += host[s][e] ** 2
        n = n + k.astype(np.uint32)
    assert np.array_equal(n, sim["n"]) and passes == sim["passes"]
    compare(S, sim["S"], TOL, "S")
    compare(Q, sim["Q"], TOL, "Q")
    assert np.array_equal(np.isnan(err), np.isnan(sim["err"]))
    first_nan = np.where(np.isnan(c).any(axis=-1).any(axis=0),
                         np.isnan(c).any(axis=-1).argmax(axis=0), mx)
    early = first_nan < mn
    assert early.any() and (n[early] == mn).all()
    late = (first_nan >= mn) & (first_nan < n)
    assert late.any()        # a NaN that arrived in a later pass
    assert (n[late] == mn + st * ((first_nan[late] - mn) // st + 1)).all()
    assert np.array_equal(np.isnan(S).any(axis=-1), first_nan < n)
