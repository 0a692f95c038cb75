"""Ray accumulators on the host (pt_accum_create_rays, include/pt_capi.h): the
work-item mapping of the list pass over ray records (pt_job.h rays_list_job)
against a numpy restatement for every work-item, a whole adaptive run through
that mapping and the ray lane code (tests/hostcheck/pt_rays_list_host.cpp)
against the oracle's per-sample colours and the simulation of the stop rule
(tests/rays_adaptive_ref.py, tests/adaptive_sim.py), and the Python layer:
checkpoint keys, the command line's argument checks and the image-order helper.
The GPU cases are tests/test_gpu_rays_adaptive.py."""
import ctypes as C
import os

import numpy as np
import pytest

import hostlib
import adaptive_sim
import rays_adaptive_ref as ref
from conftest import ROOT

from pathtracerpython_amd import adaptive, cameras
from pathtracerpython_amd._abi import PT_FLAG_RR, make_adapt, make_params, make_rays
from pathtracerpython_amd.render import from_list_order

_dp = C.POINTER(C.c_double)
_up = C.POINTER(C.c_uint32)
TOL = 1e-12   # the project's f64 bar, relative to max(1, |value|)
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def list_host(tmp_path_factory):
    """tests/hostcheck/pt_rays_list_host.cpp built by the hostcheck Makefile
    into a temporary directory."""
    lib = hostlib.build(tmp_path_factory.mktemp("rays_list_host"), "pt_rays_list_host")
    lib.hc_rays_list_job.restype = C.c_int
    lib.hc_rays_list_job.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, _up, C.c_uint32,
                                     _up, C.c_uint32, C.POINTER(C.c_int64), C.POINTER(C.c_uint64)]
    lib.hc_rays_list_pass.restype = C.c_int
    lib.hc_rays_list_pass.argtypes = [C.c_void_p, _dp, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_uint32, _up, C.c_uint32, _dp, _dp, _up]
    return lib


def test_abi_has_the_ray_accumulator():
    from pathtracerpython_amd import _native, build
    header = open(os.path.join(ROOT, "include", "pt_capi.h")).read()
    assert "int pt_accum_create_rays(" in header and "pt_accum_create_rays" in _native.EXPORTS
    assert "#define PT_API_VERSION 7" in header   # additive: the version stays
    if os.path.exists(_native.LIB_PATH):   # (a built tree: the library exports it)
        assert b"pt_accum_create_rays\0" in open(_native.LIB_PATH, "rb").read()
    # the list kernel's unit is compiled and covered by the build id as pt_rays.hip is
    assert build.AA_UNITS["pt_rays_list.hip"] == build.AA_UNITS["pt_rays.hip"]
    assert any(f.endswith("pt_rays_list.hip") for f in build.source_files())
    # the mapping's header compiles without the HIP runtime
    assert "hip_runtime" not in open(os.path.join(build.CSRC, "pt_job.h")).read()


# ------------------------------------------------------------ the mapping --
def job_numpy(keys, n_rays, rule, split, lst, accN, n_tid, bounces, rr_depth, seed):
    """rays_list_job restated: the ten fields hc_rays_list_job reports, per work-item."""
    _, _, lo, hi, step = rule
    log2 = int(split).bit_length() - 1
    out = np.zeros((n_tid, 10), dtype=np.int64)
    for tid in range(n_tid):
        entry, c = tid >> log2, tid & (split - 1)
        e = int(lst[entry]) if entry < len(lst) else NONE
        valid = e < n_rays
        row = [int(valid), e, 0, -1, 0, 0, split, 0, bounces, rr_depth]
        if valid:
            n0 = int(accN[e])
            k = int(adaptive_sim.k_numpy(n0, lo, hi, step))
            row[2], row[3], row[4], row[5] = k, e, int(keys[e]), n0 + c
            row[7] = (k - c + split - 1) >> log2 if c < k else 0
        out[tid] = row
    return out


@pytest.mark.parametrize("split", [1, 4, 64])
@pytest.mark.parametrize("n_list", [1, 63, 64, 65])
def test_mapping_every_work_item(list_host, n_list, split):
    """rays_list_job = the numpy restatement for every tid of the launch (whole
    blocks of 64): lists of 1, 63, 64 and 65 entries, 1, 4 and 64 lanes per
    record, unequal n (0, 3, 4, 30 and others, so unequal k in one launch),
    entries that are no record (e = n, e = 2^32 - 1), both rules."""
    rng = np.random.default_rng(100 * n_list + split)
    n_rays = 70
    keys = rng.integers(0, 1 << 32, size=n_rays, dtype=np.uint64).astype(np.uint32)
    rec = make_rays(rng.normal(size=(n_rays, 3)), rng.normal(size=(n_rays, 3)), keys)
    lst = rng.permutation(n_rays)[:n_list].astype(np.uint32)
    if n_list >= 63:
        lst[5], lst[40] = n_rays, NONE   # no records: skipped, never dereferenced
    n_tid = ((n_list * split + 63) // 64) * 64
    for rule, rr_depth, flags in ((ref.RULES["r4-32-4"], -1, 0), (ref.RULES["r3-17-5"], 1, PT_FLAG_RR)):
        accN = rng.choice([0, 3, 4, 30, 1, 13, 16, 31], size=n_rays).astype(np.uint32)
        accN = np.minimum(accN, rule[3]).astype(np.uint32)
        p = make_params(n_rays, 1, rule[3], 3, 0x123456789abc, flags, 1)
        ap = make_adapt(rule[0], rule[3], rule[2], rule[4], rule[1])
        out = np.zeros((n_tid, 10), dtype=np.int64)
        seeds = np.zeros(n_tid, dtype=np.uint64)
        rc = list_host.hc_rays_list_job(C.c_void_p(rec.ctypes.data), n_rays, C.addressof(p), C.addressof(ap), split,
                                        lst.ctypes.data_as(_up), n_list, accN.ctypes.data_as(_up), n_tid,
                                        out.ctypes.data_as(C.POINTER(C.c_int64)),
                                        seeds.ctypes.data_as(C.POINTER(C.c_uint64)))
        assert rc == 0
        want = job_numpy(keys, n_rays, rule, split, lst, accN, n_tid, 3, rr_depth, p.seed)
        assert np.array_equal(out, want), f"first difference at tid {np.nonzero((out != want).any(axis=1))[0][:4]}"
        assert (seeds == 0x123456789abc).all()   # the launch's constants also where there is no job
        # an entry's lanes take its k samples once each
        take = out[:, 7].reshape(-1, split).sum(axis=1)
        assert np.array_equal(take, out[::split, 2])


def test_mapping_k_not_a_multiple_of_split(list_host):
    """k = 5 on 4 lanes: 2, 1, 1, 1 samples, from sample n on with stride 4."""
    rec = make_rays(np.zeros((2, 3)), np.ones((2, 3)), [11, 12])
    rule = ref.RULES["r3-17-5"]
    p = make_params(2, 1, 17, 3, 9)
    ap = make_adapt(rule[0], rule[3], rule[2], rule[4], rule[1])
    lst, accN = np.array([1], dtype=np.uint32), np.array([0, 3], dtype=np.uint32)
    out, seeds = np.zeros((64, 10), dtype=np.int64), np.zeros(64, dtype=np.uint64)
    assert list_host.hc_rays_list_job(C.c_void_p(rec.ctypes.data), 2, C.addressof(p), C.addressof(ap), 4,
                                      lst.ctypes.data_as(_up), 1, accN.ctypes.data_as(_up), 64,
                                      out.ctypes.data_as(C.POINTER(C.c_int64)),
                                      seeds.ctypes.data_as(C.POINTER(C.c_uint64))) == 0
    assert out[:4, 2].tolist() == [5] * 4 and out[:4, 7].tolist() == [2, 1, 1, 1]
    assert out[:4, 5].tolist() == [3, 4, 5, 6] and out[:4, 4].tolist() == [12] * 4
    assert not out[4:, 0].any() and (out[4:, 3] == -1).all()


# ------------------------------------------------- the run against the oracle --
def pass_split(L, kmin):
    """pt_accum_band's rule: min(L, largest power of two <= min(kmin, 64))."""
    cap = 1
    while cap * 2 <= min(kmin, 64):
        cap *= 2
    return min(L, cap)


def host_run(lib, b, rule, L, rr_depth=None, force64=False):
    """The pass loop on the host: numpy's select (adaptive_sim), the host list
    pass.  Yields (S, Q, n, (n_active, added)) after every pass."""
    tol, floor, lo, hi, step = ref.RULES[rule]
    rec = make_rays(b.o, b.d, b.keys)
    p = make_params(b.n, 1, hi, ref.BOUNCES, ref.SEED, 0 if rr_depth is None else PT_FLAG_RR,
                    3 if rr_depth is None else rr_depth)
    ap = make_adapt(tol, hi, lo, step, floor)
    S, Q, n = np.zeros((b.n, 3)), np.zeros((b.n, 3)), np.zeros(b.n, dtype=np.uint32)
    box = np.ascontiguousarray(b.box, dtype=np.float64)
    for _ in range(hi + 1):
        err = adaptive_sim.err_numpy(S, Q, n, floor)
        act = adaptive_sim.active_numpy(n, err, tol, lo, hi)
        lst = np.nonzero(act)[0].astype(np.uint32)
        if len(lst) == 0:
            return
        k = adaptive_sim.k_numpy(n[lst], lo, hi, step)
        rc = lib.hc_rays_list_pass(C.addressof(b.pk.desc), box.ctypes.data_as(_dp), C.c_void_p(rec.ctypes.data), b.n,
                                   C.addressof(p), C.addressof(ap), int(force64), pass_split(L, int(k.min())),
                                   lst.ctypes.data_as(_up), len(lst), S.ctypes.data_as(_dp), Q.ctypes.data_as(_dp),
                                   n.ctypes.data_as(_up))
        assert rc == 0
        yield S, Q, n, (len(lst), int(k.sum()))
    raise AssertionError("the run did not end")


def rel(got, want):
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


@pytest.mark.parametrize("rule,L,rr_depth", [("r4-32-4", 4, None), ("r3-17-5", 4, None), ("r4-32-4", 1, None),
                                             ("r3-17-5", 8, 1)])
def test_host_run_is_the_simulation(list_host, cornell, rule, L, rr_depth):
    """The Cornell batch through the host list pass: after every pass S and Q
    within 1e-12 (relative to max(1, |value|)) of the oracle's samples summed
    up to the counts, the passes and the final count map equal to the
    simulation's exactly."""
    b = ref.batch_of("cornell", cornell)
    sim = b.check_preconditions(rule, rr_depth)
    samples = b.samples(rr_depth)
    passes = []
    worst = 0.0
    for S, Q, n, ps in host_run(list_host, b, rule, L, rr_depth):
        passes.append(ps)
        wS, wQ = adaptive_sim.moments_upto(samples, n)
        worst = max(worst, rel(S, wS), rel(Q, wQ))
        assert rel(S, wS) <= TOL and rel(Q, wQ) <= TOL, f"pass {len(passes)}"
    print(f"{rule} L={L} rr={rr_depth}: {len(passes)} passes, worst |S|, |Q| difference {worst:.3e}")
    assert passes == sim["passes"]
    assert np.array_equal(n, sim["n"])
    assert rel(S, sim["S"]) <= TOL and rel(Q, sim["Q"]) <= TOL


def test_host_run_forced_f64_is_the_hybrid(list_host, cornell):
    b = ref.batch_of("cornell", cornell)
    a = [(S.copy(), Q.copy(), n.copy()) for S, Q, n, _ in host_run(list_host, b, "r3-17-5", 4)][-1]
    f = [(S.copy(), Q.copy(), n.copy()) for S, Q, n, _ in host_run(list_host, b, "r3-17-5", 4, force64=True)][-1]
    for x, y in zip(a, f):
        assert x.tobytes() == y.tobytes()


# --------------------------------------------------------- the Python layer --
def test_checkpoint_keys(packed):
    """A ray run's key holds the records' hash and the shape; a frame run's key
    is what it was."""
    frame = adaptive.accum_key(packed, 12, 8, 3, 9, False, 3, 4)
    assert frame == {"scene": frame["scene"], "width": 12, "height": 8, "bounces": 3, "seed": 9, "rr": False,
                     "rr_depth": 3, "lanes_per_pixel": 4}
    assert adaptive.accum_key(packed, 12, 8, 3, 9, False, 3, 4, True) == dict(frame, aa=True)
    assert adaptive.accum_key(packed, 12, 8, 3, 9, False, 3, 4, lens=(0.5, -20)) == dict(frame, lens=[0.5, -20.0])
    o, d, k = cameras.to_image_order(*cameras.look_at_rays((2, 1.5, 3), (0, 0, -24), W=12, H=8), 12, 8)
    rec = make_rays(o, d, k)
    ray = adaptive.accum_key(packed, 12, 8, 3, 9, False, 3, 4, rays=rec, shape=(8, 12))
    assert ray != frame and {x: ray[x] for x in frame} == frame
    assert len(ray["rays"]) == 64 and ray["shape"] == [8, 12]
    flat = adaptive.accum_key(packed, 96, 1, 3, 9, False, 3, 4, rays=rec)
    assert flat["shape"] == [96] and flat["rays"] == ray["rays"]
    rec2 = rec.copy()
    rec2["key"][5] += 1
    assert adaptive.accum_key(packed, 12, 8, 3, 9, False, 3, 4, rays=rec2, shape=(8, 12))["rays"] != ray["rays"]


def test_ray_records_shapes():
    o, d = np.zeros((6, 3)), np.ones((6, 3))
    rec, hw = adaptive.ray_records(o, d)
    assert hw == (1, 6) and list(rec["key"]) == list(range(6))
    assert adaptive.ray_records(o, d, shape=(2, 3))[1] == (2, 3)
    for bad in ((4, 2), (0, 6), (6,)):
        with pytest.raises((ValueError, TypeError)):
            adaptive.ray_records(o, d, shape=bad)
    with pytest.raises(ValueError):
        adaptive.ray_records(np.zeros((0, 3)), np.zeros((0, 3)))


# --look-at reaches the accumulator through its own switch, --ray-accum: without
# it the command line is what it was (tests/test_rays_host.py holds --look-at
# to refusing --noise and --denoise), with it check_args accepts and refuses
# exactly the issue's combinations.
LOOK = ["scene.sdl", "--look-at", "1", "2", "9", "0", "0", "-20"]
ACCUM = LOOK + ["--ray-accum"]


@pytest.mark.parametrize("extra", [["--noise", "0.05", "-r", "16"], ["--denoise", "-r", "4"],
                                   ["--noise", "0.05", "-r", "16", "--denoise", "--denoise-iters", "3",
                                    "--denoise-sigma", "1.5", "--save-aov", "aov", "--checkpoint", "f.npz"],
                                   ["--denoise", "-r", "4", "--save-aov", "aov"],
                                   ["--noise", "0.05", "-r", "16", "--save-aov", "aov"],
                                   ["--noise", "0.05", "-r", "16", "--checkpoint", "f.npz"],
                                   ["--noise", "0.02", "-r", "32", "--min-spp", "4", "--step-spp", "4", "--rr",
                                    "--seed", "3", "--size", "8", "6", "--out", "x.png", "--save-raw", "x.npy",
                                    "--up", "0", "0", "1", "--fov", "50"]])
def test_cli_look_at_accepts_the_accumulator_flags(extra):
    from pathtracerpython_amd import main as cli
    cli.check_args(cli.setup(ACCUM + extra))


@pytest.mark.parametrize("extra,name", [(["--aa"], "--aa"), (["--aperture", "0.2", "--focus-z", "-20"], "--aperture"),
                                        (["--devices", "2"], "--devices > 1"),
                                        (["--local-devices", "1"], "--local-devices"),
                                        (["--chunk-spp", "2", "-r", "4"], "--chunk-spp")])
@pytest.mark.parametrize("base", [LOOK, ACCUM + ["--noise", "0.05", "-r", "16", "--denoise"]], ids=["plain", "accum"])
def test_cli_look_at_refuses_by_name(base, extra, name):
    from pathtracerpython_amd import main as cli
    with pytest.raises(SystemExit) as e:
        cli.check_args(cli.setup(base + extra))
    assert "--look-at does not combine with " + name in str(e.value)


def test_cli_ray_accum_switch():
    """--checkpoint needs --noise; the switch needs --look-at and something for
    the accumulator to do; the rule's and the filter's own checks still apply;
    without the switch every accumulator flag is refused by name, pointing to it."""
    from pathtracerpython_amd import main as cli
    for extra, match in ((["--checkpoint", "f.npz", "--denoise", "-r", "4"], "--checkpoint with --noise"),
                         ([], "--noise or --denoise"), (["--save-aov", "aov"], "--noise or --denoise"),
                         (["--noise", "0.05", "-r", "1"], "max_spp"), (["--denoise", "-r", "1"], "-r >= 2"),
                         (["--denoise", "-r", "4", "--denoise-iters", "9"], "--denoise-iters")):
        with pytest.raises(SystemExit, match=match):
            cli.check_args(cli.setup(ACCUM + extra))
    with pytest.raises(SystemExit, match="--ray-accum goes with --look-at"):
        cli.check_args(cli.setup(["scene.sdl", "--ray-accum", "--noise", "0.05", "-r", "16"]))
    for extra, name in ((["--noise", "0.05", "-r", "16"], "--noise"), (["--denoise", "-r", "4"], "--denoise"),
                        (["--checkpoint", "f.npz"], "--checkpoint"), (["--save-aov", "aov"], "--save-aov")):
        with pytest.raises(SystemExit) as e:
            cli.check_args(cli.setup(LOOK + extra))
        assert f"--look-at does not combine with {name} unless --ray-accum" in str(e.value)


@pytest.mark.parametrize("W,H", [(12, 8), (5, 7), (1, 4), (4, 1)])
def test_image_order_helper(W, H):
    """to_image_order puts the ray of list index k = ix*H + iy at record
    e = (H-1-iy)*W + ix, which is from_list_order's placement, and
    from_image_order undoes it."""
    o, d, k = cameras.look_at_rays((2, 1.5, 3), (0, 0, -24), fov_y=30.0, W=W, H=H)
    o[:, 0] += np.arange(W * H)   # (distinct origins)
    oi, di, ki = cameras.to_image_order(o, d, k, W, H)
    for iy in range(H):
        for ix in range(W):
            assert ki[(H - 1 - iy) * W + ix] == ix * H + iy
    assert np.array_equal(di.reshape(H, W, 3), from_list_order(d, W, H))
    assert np.array_equal(oi.reshape(H, W, 3), from_list_order(o, W, H))
    assert np.array_equal(oi[np.argsort(ki)], o) and np.array_equal(di[np.argsort(ki)], d)
    for img, lst in ((oi, o), (di, d), (ki, k), (di.reshape(H, W, 3), d), (ki.reshape(H, W), k)):
        assert np.array_equal(cameras.from_image_order(img, W, H), lst)
    assert ki.dtype == np.uint32 and oi.flags.c_contiguous
