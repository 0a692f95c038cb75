"""Adaptive sampling on row bands on the GPU (pt_accum_set_band, band tiles,
pt_accum_write; k_accum_select_* band form, k_accum_export_band /
k_accum_import_band in pt_hip.hip): the band select against numpy bit for bit,
banded runs against the whole-frame run (bitwise with a fixed lane count),
tiles and the host restore, resumed runs, the denoise of a merged accumulator,
the refusals and the CLI.  Bands are emulated on one GPU
(MultiRenderer(scene, [0]*n)).  Host-side cases: tests/test_adaptive_bands.py."""
import ctypes as C

import numpy as np
import pytest

from adaptive_sim import active_numpy, err_numpy, k_numpy, oracle_samples, simulate
from pathtracerpython_amd import _native, adaptive
from pathtracerpython_amd._abi import band_pixels, make_adapt, make_band
from pathtracerpython_amd.adaptive import Accumulator, render_adaptive, run_passes
from pathtracerpython_amd.render import MultiRenderer, Renderer

pytestmark = pytest.mark.gpu

RULES = [(4, 32, 4), (3, 17, 5)]
SIZES = [(24, 24), (24, 23)]
BOUNCES, SEED, TOL, FLOOR = 3, 9, 0.05, 0.01     # runs24 of tests/test_gpu_adaptive.py


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else a.dtype)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def R(cornell):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    r = Renderer(cornell)
    yield r
    r.close()


@pytest.fixture(scope="module")
def multis(cornell):
    """MultiRenderer(cornell, [0]*n) for the worlds of the tests, made once."""
    made = {}

    def get(n):
        if n not in made:
            made[n] = MultiRenderer(cornell, [0] * n)
        return made[n]
    yield get
    for m in made.values():
        m.close()


def run_kw(rule, **kw):
    mn, mx, st = rule
    return dict(max_spp=mx, bounces=BOUNCES, seed=SEED, tol=TOL, min_spp=mn, step_spp=st, floor=FLOOR, **kw)


@pytest.fixture(scope="module")
def single(R):
    """The one-accumulator runs, made once per (W, H, rule, lanes)."""
    made = {}

    def get(W, H, rule, lanes):
        key = (W, H, rule, lanes)
        if key not in made:
            made[key] = render_adaptive(R, W, H, **run_kw(rule, lanes_per_pixel=lanes, moments=True))
        return made[key]
    return get


@pytest.fixture(scope="module")
def margins(packed):
    """simulate()'s margin of each fixture on the oracle's frames: no stop
    decision is near tol, so sums that differ by 1e-12 cannot flip one."""
    out = {}
    for W, H in SIZES:
        frames = oracle_samples(packed, W, H, BOUNCES, SEED, 32)
        for mn, mx, st in RULES:
            out[(W, H, (mn, mx, st))] = simulate(frames[:mx], TOL, FLOOR, mn, mx, st)["margin"]
    return out


def state_after_uniform(R, W, H, spp=4):
    with Accumulator(R, W, H) as acc:
        run_passes(acc, R.params(W, H, spp, BOUNCES, SEED), make_adapt(0.0, spp, spp, spp))
        return acc.read(S=True, Q=True, n=True)


# 1 ------------------------------------------------------------- select --
BANDS37 = [(0, 23, 1, 0), (0, 23, 2, 1), (0, 23, 3, 0), (0, 23, 8, 7), (3, 21, 1, 0), (3, 21, 2, 1),
           (3, 21, 3, 0), (3, 21, 8, 7)]


@pytest.fixture(scope="module")
def state37(R):
    return state_after_uniform(R, 37, 23)


def check_select(acc, d, band, rule, W, H):
    mn, mx, st = rule
    acc.write(d["S"], d["Q"], d["n"])          # err = +inf everywhere again
    acc.set_band(band)
    n_active, k = acc.select(make_adapt(TOL, mx, mn, st, FLOOR))
    got = acc.read(err=True, active=True)
    e = band_pixels(W, H, band)
    want = err_numpy(d["S"], d["Q"], d["n"], FLOOR).reshape(-1)
    err = got["err"].reshape(-1)
    assert np.array_equal(bits(err[e]), bits(want[e]))
    outside = np.ones(W * H, dtype=bool)
    outside[e] = False
    assert np.isposinf(err[outside]).all()     # written only inside the band
    n = d["n"].reshape(-1)
    act = active_numpy(n[e], want[e], TOL, mn, mx)
    assert got["list"].dtype == np.uint32 and np.array_equal(got["list"], e[act])
    assert n_active == int(act.sum()) and k == int(k_numpy(n[e], mn, mx, st)[act].sum())
    return n_active


@pytest.mark.parametrize("band", BANDS37, ids=lambda b: "rows%d_%d_step%d_phase%d" % b)
def test_band_select_is_numpy_bit_for_bit(R, state37, band):
    assert (state37["n"] == 4).all()
    with Accumulator(R, 37, 23) as acc:
        n_active = check_select(acc, state37, make_band(23, *band), (4, 32, 4), 37, 23)
        assert 0 < n_active < len(band_pixels(37, 23, make_band(23, *band)))


def test_band_select_of_more_than_1024_blocks(R):
    """1024 x 520, every second row: 260 rows = 1040 select blocks, the scan's
    second chunk — on synthetic moments (select only, nothing is rendered)."""
    W, H = 1024, 520
    rng = np.random.default_rng(5)
    n = rng.integers(0, 40, size=(H, W)).astype(np.uint32)
    c = rng.random((H, W, 3))
    S = c * n[..., None]
    Q = S * c * (1.0 + 0.3 * rng.random((H, W, 1)))
    band = make_band(H, 0, H, 2, 1)
    assert (len(band_pixels(W, H, band)) + 255) // 256 == 1040
    with Accumulator(R, W, H) as acc:
        n_active = check_select(acc, dict(S=S, Q=Q, n=n), band, (4, 32, 4), W, H)
    assert 0 < n_active < 260 * W


def test_an_empty_band_selects_nothing(R):
    with Accumulator(R, 9, 5, band=make_band(5, 0, 5, 8, 7)) as acc:
        assert acc.select(make_adapt(TOL, 32, 4, 4, FLOOR)) == (0, 0)
        acc.render(R.params(9, 5, 32, BOUNCES, SEED), make_adapt(TOL, 32, 4, 4, FLOOR))
        d = acc.read(n=True, err=True)
        assert not d["n"].any() and np.isposinf(d["err"]).all()
        assert all(v.size == 0 for v in acc.export_band().values())
        acc.set_band(make_band(5, 2, 2))
        assert acc.select(make_adapt(TOL, 32, 4, 4, FLOOR)) == (0, 0)
        acc.set_band(make_band(5))
        assert acc.select(make_adapt(TOL, 32, 4, 4, FLOOR)) == (45, 180)


# 2 ------------------------------------------- banded run = whole frame --
@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("rule", RULES, ids=lambda r: "min%d_max%d_step%d" % r)
@pytest.mark.parametrize("W,H", SIZES)
def test_banded_run_equals_the_whole_frame_run(single, multis, margins, W, H, rule, world):
    assert margins[(W, H, rule)] > 1e-9
    one = single(W, H, rule, 4)
    res = multis(world).render_adaptive(W, H, **run_kw(rule, lanes_per_pixel=4, moments=True))
    assert same(res.S, one.S) and same(res.Q, one.Q) and same(res.counts, one.counts)
    assert same(res.err, one.err) and same(res.fb, one.fb)
    assert res.passes == one.passes and res.samples == one.samples
    assert len(np.unique(res.counts)) > 2
    # lanes chosen per pass: the counts are the same, the sums differ by their order at most
    one0 = single(W, H, rule, 0)
    res0 = multis(world).render_adaptive(W, H, **run_kw(rule, moments=True))
    dS = float((np.abs(res0.S - one0.S) / np.maximum(np.abs(one0.S), 1e-300)).max())
    dQ = float((np.abs(res0.Q - one0.Q) / np.maximum(np.abs(one0.Q), 1e-300)).max())
    print(f"{W}x{H} {rule} world {world}, lanes 0: rel |dS| = {dS:.3e}, rel |dQ| = {dQ:.3e}")
    assert same(res0.counts, one0.counts) and res0.passes == one0.passes
    assert dS <= 1e-12 and dQ <= 1e-12
    assert same(one0.counts, one.counts)


def test_the_fixed_lane_count_is_honoured(single, multis):
    """Two lanes per pixel sum a pixel's samples in another order than four:
    the same counts, sums equal to the sum order but not to the bit — and a
    banded run with two lanes is the whole-frame run with two, bit for bit."""
    rule = (4, 32, 4)
    four, two = single(24, 23, rule, 4), single(24, 23, rule, 2)
    assert same(two.counts, four.counts) and two.passes == four.passes
    assert np.abs(two.S - four.S).max() <= 1e-12 * np.abs(four.S).max()
    assert not np.array_equal(two.S, four.S)
    res = multis(3).render_adaptive(24, 23, **run_kw(rule, lanes_per_pixel=2, moments=True))
    assert same(res.S, two.S) and same(res.Q, two.Q) and same(res.counts, two.counts)


# 3 ---------------------------------------------------------------- BVH --
@pytest.mark.parametrize("megakernel", [False, True], ids=["wavefront", "megakernel"])
def test_bvh_scene_in_three_bands(mesh_golden, megakernel):
    sc, _ = mesh_golden
    kw = dict(max_spp=16, bounces=3, seed=5, tol=0.05, min_spp=4, step_spp=4, lanes_per_pixel=4,
              moments=True)
    with Renderer(sc) as r:
        one = render_adaptive(r, 12, 11, **kw)          # through the wavefront list form
    with MultiRenderer(sc, [0, 0, 0]) as m:
        res = m.render_adaptive(12, 11, megakernel=megakernel, **kw)
    assert same(res.S, one.S) and same(res.Q, one.Q) and same(res.counts, one.counts)
    assert same(res.err, one.err) and res.passes == one.passes
    assert len(one.passes) > 1 and one.counts.max() > one.counts.min()


# 4 -------------------------------------------------------------- tiles --
@pytest.mark.parametrize("band", [(0, 23, 3, 1), (3, 21, 2, 0), (0, 23, 1, 0)],
                         ids=lambda b: "rows%d_%d_step%d_phase%d" % b)
def test_tiles_round_trip(R, state37, band):
    W, H = 37, 23
    b = make_band(H, *band)
    e = band_pixels(W, H, b)
    with Accumulator(R, W, H) as acc:
        acc.write(state37["S"], state37["Q"], state37["n"])
        acc.select(make_adapt(TOL, 32, 4, 4, FLOOR))       # err of the whole frame
        d = acc.read(S=True, Q=True, n=True, err=True)
        acc.set_band(b)
        t = acc.export_band()
    assert t["S"].shape == (len(e), 3) and t["n"].dtype == np.uint32
    assert same(t["S"], d["S"].reshape(-1, 3)[e]) and same(t["Q"], d["Q"].reshape(-1, 3)[e])
    assert same(t["err"], d["err"].reshape(-1)[e]) and same(t["n"], d["n"].reshape(-1)[e])
    # a numpy-built tile into an empty accumulator (whose own band is another)
    rng = np.random.default_rng(1)
    tile = dict(S=rng.random((len(e), 3)), Q=rng.random((len(e), 3)), err=rng.random(len(e)),
                n=rng.integers(1, 99, len(e)).astype(np.uint32))
    with Accumulator(R, W, H, band=make_band(H, 0, H, 2, 1)) as acc:
        acc.import_band(b, tile)
        assert acc.band.rows() == (0, H, 2, 1)
        d = acc.read(S=True, Q=True, n=True, err=True)
        acc.set_band(b)
        back = acc.export_band()
    for k in tile:
        assert same(back[k], tile[k])
    want = dict(S=np.zeros((W * H, 3)), Q=np.zeros((W * H, 3)), err=np.full(W * H, np.inf),
                n=np.zeros(W * H, dtype=np.uint32))
    for k in tile:
        want[k][e] = tile[k]
        assert same(d[k].reshape(want[k].shape), want[k])   # nothing outside the band's rows


def test_write_then_read_is_a_round_trip(R, state37):
    W, H = 37, 23
    with Accumulator(R, W, H) as acc:
        acc.select(make_adapt(TOL, 32, 4, 4, FLOOR))
        acc.write(state37["S"], state37["Q"], state37["n"])
        d = acc.read(S=True, Q=True, n=True, err=True)
        assert same(d["S"], state37["S"]) and same(d["Q"], state37["Q"]) and same(d["n"], state37["n"])
        assert np.isposinf(d["err"]).all()
        check_select(acc, state37, make_band(H), (4, 32, 4), W, H)
        S = state37["S"]
        for bad in ((None, S, state37["n"]), (S, None, state37["n"]), (S, S, None)):
            p = [None if a is None else a.ctypes.data_as(C.c_void_p) for a in bad]
            dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
            assert acc._lib.pt_accum_write(acc._h, C.cast(p[0], dp), C.cast(p[1], dp), C.cast(p[2], up)) == -1
        with pytest.raises(ValueError):
            acc.write(S[:5], S, state37["n"])


# 5 ------------------------------------------------------------- resume --
@pytest.mark.parametrize("rule", RULES, ids=lambda r: "min%d_max%d_step%d" % r)
def test_a_resumed_run_is_the_uninterrupted_run(R, single, rule):
    mn, mx, st = rule
    one = single(24, 23, rule, 0)
    p, adapt = R.params(24, 23, mx, BOUNCES, SEED), make_adapt(TOL, mx, mn, st, FLOOR)
    with Accumulator(R, 24, 23) as acc:
        first = []
        for _ in range(2):
            first.append(acc.select(adapt))
            acc.render(p, adapt)
        d = acc.read(S=True, Q=True, n=True)
    with Accumulator(R, 24, 23) as acc:
        acc.write(d["S"], d["Q"], d["n"])
        rest = run_passes(acc, p, adapt)
        d = acc.read(S=True, Q=True, n=True, err=True)
    assert first + rest == one.passes
    assert same(d["S"], one.S) and same(d["Q"], one.Q) and same(d["n"], one.counts)
    assert same(d["err"], one.err)


def test_checkpointed_runs_and_the_cli(R, single, tmp_path, capsys):
    from conftest import CORNELL
    from pathtracerpython_amd import main as cli
    rule = (4, 32, 4)
    one = single(24, 23, rule, 0)
    ck = str(tmp_path / "run.npz")
    assert render_adaptive(R, 24, 23, **run_kw(rule, checkpoint=ck, max_passes=2)) is None
    st = adaptive.AccumCheckpoint(ck)
    with np.load(ck, allow_pickle=False) as z:
        assert z["passes"].tolist() == [list(p) for p in one.passes[:2]]
    res = render_adaptive(R, 24, 23, **run_kw(rule, checkpoint=ck, moments=True))
    assert same(res.S, one.S) and same(res.Q, one.Q) and same(res.counts, one.counts)
    assert same(res.err, one.err) and res.passes == one.passes
    with pytest.raises(ValueError, match="another render"):
        render_adaptive(R, 24, 23, **{**run_kw(rule, checkpoint=ck), "seed": 10})
    # the CLI: stopped after two passes by the Python call, finished by --checkpoint
    st.remove()
    assert render_adaptive(R, 24, 23, **run_kw(rule, checkpoint=ck, max_passes=2)) is None
    raw = str(tmp_path / "fb.npy")
    fb = cli.main([CORNELL, "-r", "32", "-b", str(BOUNCES), "--seed", str(SEED), "--size", "24", "23",
                   "--noise", str(TOL), "--min-spp", "4", "--step-spp", "4", "--checkpoint", ck,
                   "--save-raw", raw])
    assert same(fb, one.fb) and same(np.load(raw), one.fb)
    assert f"adaptive: {len(one.passes)} passes, {one.samples} samples" in capsys.readouterr().out
    with np.load(ck, allow_pickle=False) as z:
        assert same(np.array(z["n"]), one.counts) and len(z["passes"]) == len(one.passes)
    # a finished file renders nothing more
    again = render_adaptive(R, 24, 23, **run_kw(rule, checkpoint=ck))
    assert again.passes == one.passes and same(again.fb, one.fb)


# 6 ------------------------------------------------------------ denoise --
def test_denoise_of_a_merged_accumulator(R, multis):
    kw = run_kw((4, 32, 4), denoise=True, lanes_per_pixel=4)
    one = R.render_adaptive(24, 23, **kw)
    res = multis(3).render_adaptive(24, 23, **kw)
    assert same(res.denoised, one.denoised) and same(res.denoised_var, one.denoised_var)
    for k in ("tri", "obj", "N", "P"):
        assert same(res.features[k], one.features[k])
    assert same(res.fb, one.fb) and not np.array_equal(res.denoised, res.fb)


# 7 ----------------------------------------------------------- refusals --
def test_refusals_leave_the_handle_usable(R):
    import torch
    W = H = 8
    adapt = make_adapt(0.0, 2, 2, 2)
    p = R.params(W, H, 2, 2, SEED)
    bad = [dict(row_step=0), dict(row_step=-1), dict(row_step=2, row_phase=2), dict(row_phase=-1),
           dict(row_begin=5, row_end=4), dict(row_begin=-1), dict(row_end=9), dict(row_begin=9, row_end=9),
           dict(lanes_per_pixel=3), dict(lanes_per_pixel=128), dict(lanes_per_pixel=-2)]
    with Accumulator(R, W, H) as acc:
        tile = torch.zeros(60 * W * H, dtype=torch.uint8, device="cuda")
        for kw in bad:
            b = make_band(H, **kw)
            with pytest.raises(_native.NativeError, match=r"pt_accum_set_band failed \(-1\): \S"):
                acc.set_band(b)
            with pytest.raises(_native.NativeError, match=r"\(-1\): \S"):
                acc.import_band(b, tile.data_ptr())
        b = make_band(H)
        b.reserved = 1
        with pytest.raises(_native.NativeError, match=r"\(-1\): .*reserved"):
            acc.set_band(b)
        assert acc._lib.pt_accum_set_band(acc._h, None) == -1
        assert acc.band.rows() == (0, H, 1, 0)
        assert acc.select(adapt) == (64, 128)       # still the whole frame
        # a banded accumulator: no features, no denoise; the render params keep their refusals
        acc.set_band(make_band(H, 0, H, 2, 1, lanes_per_pixel=2))
        out = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda")
        with pytest.raises(_native.NativeError, match=r"pt_accum_features failed \(-1\): .*whole frame"):
            acc.features()
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        assert acc._lib.pt_accum_read_features(acc._h, ip(), ip(), dp(), dp()) == -1
        with pytest.raises(_native.NativeError, match=r"\(-1\): .*whole frame"):
            acc.denoise_device(out.data_ptr())
        with pytest.raises(_native.NativeError, match=r"\(-1\): \S"):
            acc.denoise()
        from pathtracerpython_amd._abi import with_flags
        with pytest.raises(_native.NativeError, match=r"\(-1\): \S"):
            acc.render(with_flags(p, row_step=2, row_phase=1), adapt)
        with pytest.raises(_native.NativeError, match=r"\(-1\): \S"):
            acc.render(with_flags(p, lanes_per_pixel=2), adapt)
        assert not acc.read(n=True)["n"].any()      # nothing was rendered
        assert acc.select(adapt) == (32, 64)
        acc.render(p, adapt)
        assert acc.select(adapt) == (0, 0)
        n = acc.read(n=True)["n"]
        assert (n[0::2] == 2).all() and not n[1::2].any()   # iy odd = image rows 0, 2, ... of 8
        acc.set_band(make_band(H, lanes_per_pixel=2))
        assert acc.select(adapt) == (32, 64)
        acc.render(p, adapt)
        d = acc.read(S=True, n=True)
        den, var = acc.denoise()                    # whole again: allowed
        assert (d["n"] == 2).all() and np.isfinite(den).all()
    with Accumulator(R, W, H) as ref:
        run_passes(ref, p, adapt)
        assert np.abs(ref.read(S=True)["S"] - d["S"]).max() <= 1e-12


# CLI ------------------------------------------------------------------------
def test_cli_local_devices(multis, tmp_path, capsys, monkeypatch):
    from conftest import CORNELL
    from pathtracerpython_amd import main as cli
    monkeypatch.setattr(cli, "local_device_ids", lambda n: [0] * n)   # two bands on one GPU
    aov = str(tmp_path / "aov")
    fb = cli.main([CORNELL, "-r", "12", "-b", "2", "--seed", "9", "--size", "16", "16", "--noise", "0.05",
                   "--min-spp", "4", "--step-spp", "4", "--local-devices", "2", "--save-aov", aov,
                   "--out", str(tmp_path / "a.png")])
    res = multis(2).render_adaptive(16, 16, 12, 2, 9, tol=0.05, min_spp=4, step_spp=4)
    assert same(fb, res.fb) and same(np.load(aov + "_counts.npy"), res.counts)
    assert same(np.load(aov + "_err.npy"), res.err) and (tmp_path / "a.png").exists()
    out = capsys.readouterr().out
    assert f"adaptive: {len(res.passes)} passes, {res.samples} samples" in out and "2 local GPUs" in out
    # a plain render and --denoise take the same road
    fb = cli.main([CORNELL, "-r", "4", "-b", "2", "--seed", "9", "--size", "16", "16", "--local-devices", "2"])
    assert same(fb, multis(2).render(16, 16, 4, 2, 9, out_f64=True))
    fb = cli.main([CORNELL, "-r", "4", "-b", "2", "--seed", "9", "--size", "16", "16", "--local-devices", "2",
                   "--denoise"])
    res = multis(2).render_adaptive(16, 16, 4, 2, 9, tol=0.0, min_spp=4, step_spp=4,
                                    denoise=dict(iters=5, sigma_l=2.0))
    assert same(fb, res.denoised)
