"""Adaptive sampling on the GPU at the launch shapes tests/test_gpu_adaptive.py
does not reach: the list kernel at 16, 32 and 64 lanes per pixel (the
shared primary hit, the six-sum reduction over a whole wave, lanes with
unequal sample shares, pixels with unequal n and k in one pass), BVH scenes at
those splits, and the select kernels on frames whose block counts fill more
than one wave and more than one 1024-block chunk of k_accum_select_scan.
Every bound is against the f64 oracle's per-sample frames or numpy on the
values read back."""
import time

import numpy as np
import pytest

from adaptive_sim import (active_numpy, block_counts, err_numpy, histogram, k_numpy, moments_upto,
                          oracle_samples, simulate)
from oracle import oracle
from pathtracerpython_amd._abi import PT_FLAG_RR, make_adapt
from pathtracerpython_amd.adaptive import Accumulator, render_adaptive
from pathtracerpython_amd.render import Renderer, to_list_order

pytestmark = pytest.mark.gpu

TOL = 1e-12
FLOOR = 0.01
# Cornell 7x5, 3 bounces, seed 9.  A list-kernel block is one wave of 64
# work-items, so the 35 list entries end inside a block at 16 lanes per pixel
# (560 work-items, 8.75 blocks) and at 32 (1120, 17.5): the launch's tail lanes
# (entry >= n_list) run too.  At 64 lanes a block is exactly one pixel.
W75, H75, B75, SEED75 = 7, 5, 3, 9


@pytest.fixture(scope="module")
def R(cornell):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    r = Renderer(cornell)
    yield r
    r.close()


@pytest.fixture(scope="module")
def frames75(packed):
    """The oracle's 100 per-sample frames of the 7x5 frame (read-only)."""
    f = oracle_samples(packed, W75, H75, B75, SEED75, 100)
    f.setflags(write=False)
    return f


def uniform_moments(r, W, H, spp, bounces, seed, **kw):
    """min = max = step = spp through the accumulator: (S, Q, n, passes)."""
    adapt = make_adapt(0.0, spp, spp, spp)
    p = r.params(W, H, spp, bounces, seed, **kw)
    with Accumulator(r, W, H) as acc:
        passes = []
        while True:
            n_active, k = acc.select(adapt)
            if not n_active:
                break
            assert len(passes) < 2, "a min = max = step run is one pass"
            acc.render(p, adapt)
            passes.append((n_active, k))
        d = acc.read(S=True, Q=True, n=True)
    return d["S"], d["Q"], d["n"], passes


def moment_gaps(S, Q, frames):
    return (float(np.abs(S - frames.sum(axis=0)).max()),
            float(np.abs(Q - (frames ** 2).sum(axis=0)).max()))


# A ------------------------------------- 16, 32, 64 lanes per pixel (Cornell) --
# Lanes per pixel of these passes, by choose_split (pt_plan.h) as
# plan_pass calls it for pt_accum_render (tests/test_plan_host.py holds the numbers): spp' = min(kmin, 64) with kmin the pass's smallest
# k (= spp here: one pass from n = 0), cap = the largest power of two <= spp';
# the scene has no BVH and the launch (35 pixels) is far below min_lanes, so
# the second loop doubles the split up to the cap whatever the first left:
#   spp 16 -> 16, 17 -> 16, 31 -> 16, 32 -> 32, 48 -> 32, 64 -> 64, 100 -> 64.
# From 16 lanes on the hybrid kernel takes primary_shared (PT_PRIMARY_SHARED):
# Cornell has 19 eye-frame units, so at 16 lanes the lanes 0-2 test two units
# and the others one, at 32 lanes 13 lanes test none, at 64 lanes 45.  A lane
# takes ceil((spp - c) / split) samples: 17 -> lane 0 two and the rest one,
# 31 -> lane 15 one and the rest two, 48 -> lanes 0-15 two and 16-31 one,
# 100 -> lanes 0-35 two and 36-63 one.
@pytest.mark.parametrize("spp", [16, 17, 31, 32, 48, 64])
def test_wide_split_moments_match_the_oracle(R, frames75, spp):
    t0 = time.perf_counter()
    S, Q, n, passes = uniform_moments(R, W75, H75, spp, B75, SEED75)
    dS, dQ = moment_gaps(S, Q, frames75[:spp])
    S64, Q64, n64, p64 = uniform_moments(R, W75, H75, spp, B75, SEED75, force_f64=True)
    eS, eQ = moment_gaps(S64, Q64, frames75[:spp])
    print(f"spp {spp}: hybrid |S - sum c| = {dS:.3e}, |Q - sum c^2| = {dQ:.3e}; forced f64 "
          f"{eS:.3e}, {eQ:.3e}; bitwise equal S {np.array_equal(S, S64)}, Q {np.array_equal(Q, Q64)}; "
          f"{time.perf_counter() - t0:.3f} s")
    assert dS <= TOL and dQ <= TOL
    assert (n == spp).all() and passes == [(35, 35 * spp)]
    # the forced-f64 kernel runs the per-lane closest() instead of
    # primary_shared: an independent path to the same primary hit
    assert eS <= TOL and eQ <= TOL
    assert (n64 == spp).all() and p64 == passes
    # primary_shared's hit is closest()'s bit for bit (pt_render.h) and both
    # kernels reduce in the same order, so the moments are the same bits, as
    # test_moments_match_the_oracle_per_sample asserts at 8 lanes
    assert np.array_equal(S, S64) and np.array_equal(Q, Q64)


def test_wide_split_russian_roulette(R, packed):
    S, Q, n, passes = uniform_moments(R, W75, H75, 32, B75, SEED75, rr=True, rr_depth=1)
    c = oracle_samples(packed, W75, H75, B75, SEED75, 32, flags=PT_FLAG_RR, rr_depth=1)
    dS, dQ = moment_gaps(S, Q, c)
    print(f"RR, 32 lanes: |S - sum c| = {dS:.3e}, |Q - sum c^2| = {dQ:.3e}")
    assert (n == 32).all() and passes == [(35, 35 * 32)]
    assert dS <= TOL and dQ <= TOL


def test_a_step_above_the_widest_split(R, frames75):
    """k = 100 in one pass: the split stays at 64 (kmin is capped there), so
    the lanes take 2 or 1 samples."""
    S, Q, n, passes = uniform_moments(R, W75, H75, 100, B75, SEED75)
    dS, dQ = moment_gaps(S, Q, frames75)
    print(f"k = 100 at 64 lanes: |S - sum c| = {dS:.3e}, |Q - sum c^2| = {dQ:.3e}")
    assert (n == 100).all() and passes == [(35, 3500)]
    assert dS <= TOL and dQ <= TOL


# B -------------------------------------- mixed k and n in one 32-lane pass --
# Rule 2's tol, chosen on the oracle's frames with simulate(): tol 0.02 / 0.03 /
# 0.05 send 13 / 9 / 7 of the 35 pixels on to 32 samples with margins 6.0e-2 /
# 1.3e-2 / 5.7e-3; 0.02 has the widest margin and the most even split.
B_TOL = 0.02
B_COUNTS = {16: 22, 32: 13}                       # after rule 2, from the oracle simulation
B_PASSES = [(35, 560), (13, 208), (35, 1472)]     # 1472 = 22 * 48 + 13 * 32


def test_mixed_k_and_n_in_one_wide_pass(R, frames75):
    """Three rules in a row on one accumulator.  Rule 1 (min = max = 16) and
    rule 2 (tol, min 16, max 32, step 16) leave pixels at n = 16 and n = 32;
    rule 3 (min = max = 64, step 48) then lists them all: k = 48 from n = 16,
    k = 32 from n = 32, kmin = 32 -> 32 lanes per pixel, so the k = 48 pixels
    give lanes 0-15 two samples and lanes 16-31 one, and sample0 = n[e] + c
    differs between the pixels of the pass.  16 + 48 = 64: that pass also
    finishes the n = 16 pixels, and rule 3's next select is empty."""
    fr = frames75[:64]
    sim = simulate(fr[:32], B_TOL, FLOOR, 16, 32, 16)   # rules 1 and 2 are this run
    print(f"rule 2 on the oracle's frames: counts {histogram(sim['n'])}, margin {sim['margin']:.3e}")
    assert histogram(sim["n"]) == B_COUNTS and 5 <= B_COUNTS[32] <= 30
    assert sim["margin"] >= 1e-6
    rules = [(0.0, 16, 16, 16), (B_TOL, 16, 32, 16), (0.0, 64, 64, 48)]
    n_pred = np.zeros((H75, W75), dtype=np.int64)
    passes, worst = [], (0.0, 0.0)
    with Accumulator(R, W75, H75) as acc:
        for tol, mn, mx, st in rules:
            adapt = make_adapt(tol, mx, mn, st, FLOOR)
            p = R.params(W75, H75, mx, B75, SEED75)
            for _ in range(3):
                S_pred, Q_pred = moments_upto(fr, n_pred)
                act = active_numpy(n_pred, err_numpy(S_pred, Q_pred, n_pred, FLOOR), tol, mn, mx)
                k = np.where(act, k_numpy(n_pred, mn, mx, st), 0)
                assert acc.select(adapt) == (int(act.sum()), int(k.sum()))
                if not act.any():
                    break
                if mx == 64:   # the pass this test is about
                    assert histogram(k[act]) == {32: B_COUNTS[32], 48: B_COUNTS[16]}
                acc.render(p, adapt)
                passes.append((int(act.sum()), int(k.sum())))
                n_pred = n_pred + k
                d = acc.read(S=True, Q=True, n=True)
                assert np.array_equal(d["n"], n_pred)
                S_pred, Q_pred = moments_upto(fr, n_pred)
                dS, dQ = float(np.abs(d["S"] - S_pred).max()), float(np.abs(d["Q"] - Q_pred).max())
                print(f"rule {(tol, mn, mx, st)} pass {passes[-1]}: counts {histogram(n_pred)}, "
                      f"|S - oracle| = {dS:.3e}, |Q - oracle| = {dQ:.3e}")
                worst = (max(worst[0], dS), max(worst[1], dQ))
                assert dS <= TOL and dQ <= TOL
            else:
                raise AssertionError("a rule of this test takes at most two passes")
            if mx == 32:
                assert histogram(n_pred) == B_COUNTS
    print(f"largest |S - oracle| = {worst[0]:.3e}, |Q - oracle| = {worst[1]:.3e}")
    assert passes == B_PASSES and (n_pred == 64).all()


# C ---------------------------------------------------- BVH at wide splits --
# With a BVH choose_split grows the split to the cap (the largest power of two
# <= min(kmin, 64)) while frame pixels * split <= 2^26: 16 and 64 lanes here.
@pytest.fixture(scope="module")
def mesh_renderer(mesh_golden):
    sc, _ = mesh_golden
    r = Renderer(sc)
    yield r
    r.close()


@pytest.mark.parametrize("spp", [16, 64])
def test_bvh_scene_at_wide_splits(mesh_renderer, spp):
    r = mesh_renderer
    res = render_adaptive(r, 12, 12, spp, 3, 5, tol=0.0, min_spp=spp, step_spp=spp)
    fb = r.render(12, 12, spp=spp, bounces=3, seed=5, out_f64=True, megakernel=True)
    t0 = time.perf_counter()
    ref, _ = oracle.render(r.packed, 12, 12, spp, 3, 5)
    t_or = time.perf_counter() - t0
    d_mk = float(np.abs(res.fb - fb).max())
    d_or = float(np.abs(to_list_order(res.fb) - ref).max())
    print(f"BVH scene, {spp} lanes: |adaptive - megakernel| = {d_mk:.3e}, "
          f"|adaptive - oracle| = {d_or:.3e} (oracle {t_or:.2f} s)")
    assert (res.counts == spp).all() and res.passes == [(144, 144 * spp)]
    assert d_or <= TOL and d_mk <= TOL


# D --------------------------- the select kernels beyond a wave and a chunk --
# nb = ceil(W * H / 256) block counts go through the one 1024-thread block of
# k_accum_select_scan in chunks of 1024, 16 waves of 64 each:
#   130 x 130: nb   67, the second wave partially filled (the cross-wave
#              term); the last select block holds 4 pixels
#   512 x 512: nb 1024, one full chunk, all 16 waves
#   641 x 409: nb 1025, a second chunk of one element; the last block holds 25
#   725 x 725: nb 2054, the carry across two chunk boundaries
# Cornell at 1 bounce, rule min 2, max 6, step 2.  D_TOL chosen on the oracle's
# two first frames of each size (seed 9): the select after the min-spp pass
# then lists 446 / 7,046 / 6,945 / 14,283 pixels, the per-block counts take 22 /
# 60 / 63 / 76 distinct values, 31 / 625 / 672 / 1,421 blocks are empty (the
# background around the room and the unlit parts have zero variance) and 552
# blocks from index 1024 on are non-empty at 725 x 725.
SCAN_FRAMES = [(130, 130), (512, 512), (641, 409), (725, 725)]
D_TOL = 0.1


@pytest.mark.parametrize("W,H", SCAN_FRAMES, ids=lambda v: str(v))
def test_select_scan_regimes_are_numpy_bit_for_bit(R, packed, W, H):
    import torch
    t0 = time.perf_counter()
    mn, mx, st = 2, 6, 2
    npix = W * H
    nb = (npix + 255) // 256
    adapt = make_adapt(D_TOL, mx, mn, st, FLOOR)
    p = R.params(W, H, mx, 1, 9)
    lengths = []
    with Accumulator(R, W, H) as acc:
        for i in range(mx + 1):
            n_active, k = acc.select(adapt)
            d = acc.read(S=True, Q=True, n=True, err=True, active=True)
            want = err_numpy(d["S"], d["Q"], d["n"], FLOOR)
            assert np.array_equal(d["err"].view(np.uint64), want.view(np.uint64))
            act = active_numpy(d["n"], want, D_TOL, mn, mx)
            assert d["list"].dtype == np.uint32
            assert np.array_equal(d["list"], np.flatnonzero(act))   # ascending, unique
            assert n_active == len(d["list"]) == int(act.sum())
            assert k == int(k_numpy(d["n"], mn, mx, st)[act].sum())
            lengths.append(n_active)
            bc = block_counts(act)
            assert len(bc) == nb
            if i == 0:
                # the whole frame: every block full but the last, which holds
                # the frame's remainder at the offset 256 * (nb - 1)
                assert n_active == npix and bc[-1] == npix - 256 * (nb - 1)
            if i == 1:
                # the select after the min-spp pass is no degenerate list
                assert (d["n"] == mn).all()
                assert 0 < n_active < npix
                assert len(np.unique(bc)) >= 8
                assert (bc == 0).any()
                if nb > 2048:
                    assert (bc[1024:] > 0).any()
                elif nb > 1024:
                    # 641 x 409: block 1024 is the last 25 pixels of the bottom
                    # row, background on every seed (S = Q = 0, err = 0), so it
                    # is listed only while n < min_spp: the first select (above)
                    # is the one that carries an offset into the second chunk
                    assert bc[1024] == 0 and not d["S"].reshape(-1, 3)[256 * 1024:].any()
            if not n_active:
                break
            acc.render(p, adapt)
        assert n_active == 0 and d["n"].max() <= mx and d["n"].min() >= mn
        f64 = torch.full((H, W, 3), -1.0, dtype=torch.float64, device="cuda")
        f32 = torch.full((H, W, 3), -1.0, dtype=torch.float32, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        acc.resolve_device(f64.data_ptr(), True, s)
        acc.resolve_device(f32.data_ptr(), False, s)
        torch.cuda.synchronize()
    fb = d["S"] / d["n"][..., None]
    assert np.array_equal(f64.cpu().numpy(), fb)
    assert np.array_equal(f32.cpu().numpy(), fb.astype(np.float32))
    print(f"{W}x{H}: nb {nb}, list lengths {lengths}, counts {histogram(d['n'])}, "
          f"{time.perf_counter() - t0:.2f} s")
    if (W, H) == SCAN_FRAMES[0]:
        # a list of hundreds of scattered entries (e != entry) against the oracle
        fr = oracle_samples(packed, W, H, 1, 9, mx)
        S_or, Q_or = moments_upto(fr, d["n"])
        dS, dQ = float(np.abs(d["S"] - S_or).max()), float(np.abs(d["Q"] - Q_or).max())
        print(f"{W}x{H}: |S - oracle| = {dS:.3e}, |Q - oracle| = {dQ:.3e}")
        assert dS <= TOL and dQ <= TOL
