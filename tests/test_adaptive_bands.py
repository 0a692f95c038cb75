"""Adaptive sampling on row bands, on the host: the band mapping of the select
(pt_path.h band_pixel, compiled for the host) against _abi.band_pixels and a
direct numpy construction, the resumable run (adaptive.AccumCheckpoint) and
the multi-device driver (MultiRenderer.render_adaptive) on stand-in
accumulators, the CLI refusals and the ABI.  The GPU cases are
tests/test_gpu_adaptive_bands.py."""
import ctypes as C
import os

import numpy as np
import pytest

import hostlib
from adaptive_sim import simulate
from conftest import CORNELL, ROOT
from test_adaptive import FakeAccum, fake_frames

from pathtracerpython_amd import _abi, adaptive
from pathtracerpython_amd._abi import band_pixels, band_rows, make_band
from pathtracerpython_amd.distributed import rank_band
from pathtracerpython_amd.render import MultiRenderer


# --------------------------------------------------------- band mapping --
@pytest.fixture(scope="module")
def band_host(tmp_path_factory):
    """tests/hostcheck/pt_accum_band_host.cpp built by the hostcheck
    Makefile into a temporary directory."""
    lib = hostlib.build(tmp_path_factory.mktemp("band_host"), "pt_accum_band_host")
    lib.hc_band_pixels.restype = C.c_int64
    lib.hc_band_pixels.argtypes = [C.c_int32] * 6 + [C.POINTER(C.c_uint32), C.c_int64]
    return lib


def host_band_pixels(lib, W, H, band):
    n = lib.hc_band_pixels(W, H, *band.rows(), None, 0)
    assert n >= 0
    out = np.zeros(max(n, 1), dtype=np.uint32)
    assert lib.hc_band_pixels(W, H, *band.rows(), out.ctypes.data_as(C.POINTER(C.c_uint32)), n) == n
    return out[:n]


def direct_pixels(W, H, band):
    """e = (H-1-iy)*W + ix over the band's rows, top row first."""
    e = [(H - 1 - iy) * W + ix for iy in reversed(band_rows(H, *band.rows())) for ix in range(W)]
    return np.array(e, dtype=np.int64)


@pytest.mark.parametrize("W,H", [(37, 23), (5, 7), (300, 9)])
@pytest.mark.parametrize("step,phase", [(1, 0), (2, 1), (3, 0), (8, 7)])
def test_band_pixel_equals_numpy(band_host, W, H, step, phase):
    for rb, re in ((0, H), (3, H - 2)):
        band = make_band(H, rb, re, step, phase)
        want = direct_pixels(W, H, band)
        got = band_pixels(W, H, band)
        assert got.dtype == np.int64 and np.array_equal(got, want)
        assert np.array_equal(host_band_pixels(band_host, W, H, band), want)
        assert (np.diff(want) > 0).all()            # ascending, unique
        assert len(want) == W * len(band_rows(H, rb, re, step, phase))
        if want.size:
            assert 0 <= want[0] and want[-1] < W * H


def test_the_default_band_is_the_identity(band_host):
    for W, H in ((37, 23), (5, 7), (300, 9)):
        assert np.array_equal(host_band_pixels(band_host, W, H, make_band(H)), np.arange(W * H))
        assert np.array_equal(band_pixels(W, H, make_band(H)), np.arange(W * H))


def test_empty_band(band_host):
    band = make_band(5, 0, 5, 8, 7)
    assert band_rows(5, *band.rows()) == []
    assert band_pixels(9, 5, band).size == 0 and host_band_pixels(band_host, 9, 5, band).size == 0
    assert host_band_pixels(band_host, 9, 5, make_band(5, 3, 3)).size == 0


@pytest.mark.parametrize("W,H,world", [(37, 23, 2), (37, 23, 3), (5, 7, 8), (300, 9, 4), (6, 5, 8)])
def test_the_bands_of_a_world_partition_the_frame(band_host, W, H, world):
    parts = [host_band_pixels(band_host, W, H, make_band(H, *rank_band(H, d, world)))
             for d in range(world)]
    for d, p in enumerate(parts):
        assert np.array_equal(p, band_pixels(W, H, make_band(H, *rank_band(H, d, world))))
    assert np.array_equal(np.sort(np.concatenate(parts)), np.arange(W * H))


# ------------------------------------------------------ stand-in accums --
class BandFakeAccum(FakeAccum):
    """FakeAccum with a band, band tiles (the dict form) and write."""

    def __init__(self, renderer=None, width=6, height=4, band=None):
        super().__init__(renderer, width, height)
        self.width, self.height = width, height
        self.err = np.full((height, width), np.inf)
        self.set_band(make_band(height) if band is None else band)

    def set_band(self, band):
        self.band = band
        self.mask = np.zeros(self.H * self.W, dtype=bool)
        self.mask[band_pixels(self.W, self.H, band)] = True
        self.mask = self.mask.reshape(self.H, self.W)

    def select(self, adapt):
        err = self.err
        n_active, k = super().select(adapt)
        self.err = np.where(self.mask, self.err, err)   # err is written only inside the band
        self.act &= self.mask
        self.k = np.where(self.act, self.k, 0)
        return int(self.act.sum()), int(self.k.sum())

    def export_band(self):
        e = band_pixels(self.W, self.H, self.band)
        return dict(S=self.S.reshape(-1, 3)[e], Q=self.Q.reshape(-1, 3)[e],
                    err=self.err.reshape(-1)[e], n=self.n.reshape(-1)[e].astype(np.uint32))

    def import_band(self, band, tile):
        e = band_pixels(self.W, self.H, band)
        self.S.reshape(-1, 3)[e] = tile["S"]
        self.Q.reshape(-1, 3)[e] = tile["Q"]
        self.err.reshape(-1)[e] = tile["err"]
        self.n.reshape(-1)[e] = tile["n"]

    def write(self, S, Q, n):
        self.calls.append("write")
        self.S, self.Q, self.n = np.array(S), np.array(Q), np.array(n).astype(np.int64)
        self.err = np.full((self.H, self.W), np.inf)

    def read(self, **kw):
        return dict(S=self.S.copy(), Q=self.Q.copy(), n=self.n.astype(np.uint32), err=self.err)

    def close(self):
        pass


class FakeRenderer:
    packed = "scene A"

    class scene:
        width, height, seed = 6, 4, 3


@pytest.fixture
def stand_ins(monkeypatch):
    made = []

    def make(*a, **k):
        made.append(BandFakeAccum(*a, **k))
        return made[-1]
    monkeypatch.setattr(adaptive, "Accumulator", make)
    monkeypatch.setattr(adaptive, "scene_fingerprint", lambda packed: packed)
    monkeypatch.setattr(adaptive, "transfer_band",
                        lambda src, dst, band: dst.import_band(band, src.export_band()))
    return made


# ----------------------------------------------------------- checkpoint --
RULE = dict(max_spp=17, bounces=2, tol=0.05, min_spp=3, step_spp=5)


def test_a_stopped_and_resumed_run_equals_the_uninterrupted_one(stand_ins, tmp_path):
    whole = adaptive.render_adaptive(FakeRenderer(), **RULE)
    ref = stand_ins[-1]
    assert len(whole.passes) > 3
    ck = str(tmp_path / "run.npz")
    seen = []
    part = adaptive.render_adaptive(FakeRenderer(), checkpoint=ck, max_passes=2,
                                    on_pass=lambda i, n, k: seen.append(i), **RULE)
    assert part is None and seen == [1, 2] and os.path.exists(ck)
    assert stand_ins[-1].calls == ["select", "render", "select", "render", "select"]
    with np.load(ck, allow_pickle=False) as z:     # loads without pickle
        assert set(z.files) == {"key", "rule", "S", "Q", "n", "passes"}
        assert z["n"].dtype == np.uint32 and z["passes"].tolist() == [list(p) for p in whole.passes[:2]]
    res = adaptive.render_adaptive(FakeRenderer(), checkpoint=ck,
                                   on_pass=lambda i, n, k: seen.append(i), **RULE)
    acc = stand_ins[-1]
    assert acc.calls[0] == "write" and seen == list(range(1, len(whole.passes) + 1))
    assert res.passes == whole.passes and res.samples == whole.samples
    assert np.array_equal(res.counts, whole.counts)
    assert np.array_equal(acc.S, ref.S) and np.array_equal(acc.Q, ref.Q) and np.array_equal(acc.n, ref.n)
    assert np.array_equal(res.fb, whole.fb) and np.array_equal(res.err, whole.err)
    # a finished checkpoint renders nothing
    again = adaptive.render_adaptive(FakeRenderer(), checkpoint=ck, **RULE)
    assert stand_ins[-1].calls == ["write", "select"]
    assert again.passes == whole.passes and np.array_equal(again.fb, whole.fb)


def test_checkpoint_every_and_the_closing_write(stand_ins, tmp_path):
    ck = str(tmp_path / "run.npz")
    assert adaptive.render_adaptive(FakeRenderer(), checkpoint=ck, checkpoint_every=2, max_passes=3,
                                    **RULE) is None
    st = adaptive.AccumCheckpoint(ck).load(json_key())
    assert len(st["passes"]) == 3 and np.array_equal(st["n"], stand_ins[-1].n)   # written on the way out
    with pytest.raises(ValueError, match="checkpoint_every"):
        adaptive.render_adaptive(FakeRenderer(), checkpoint=ck, checkpoint_every=0, **RULE)


def json_key(**kw):
    return {**dict(scene="scene A", width=6, height=4, bounces=2, seed=3, rr=False, rr_depth=3,
                   lanes_per_pixel=0), **kw}


def test_a_file_of_another_render_is_refused(stand_ins, tmp_path):
    ck = str(tmp_path / "run.npz")
    assert adaptive.render_adaptive(FakeRenderer(), checkpoint=ck, max_passes=2, **RULE) is None

    class Other(FakeRenderer):
        packed = "scene B"
    for r, kw in ((Other(), {}), (FakeRenderer(), dict(width=5)), (FakeRenderer(), dict(height=3)),
                  (FakeRenderer(), dict(seed=4)), (FakeRenderer(), dict(bounces=3)),
                  (FakeRenderer(), dict(lanes_per_pixel=4))):
        n_made = len(stand_ins)
        with pytest.raises(ValueError, match="belongs to another render"):
            adaptive.render_adaptive(r, checkpoint=ck, **{**RULE, **kw})
        assert len(stand_ins) == n_made            # refused before any device work
    st = adaptive.AccumCheckpoint(ck).load(json_key())
    assert len(st["passes"]) == 2 and st["rule"]["tol"] == 0.05


def test_a_changed_rule_resumes(stand_ins, tmp_path):
    """The rule is no part of the key: a lower tol and a larger budget continue
    from the moments the file holds."""
    ck = str(tmp_path / "run.npz")
    first = adaptive.render_adaptive(FakeRenderer(), checkpoint=ck, **RULE)
    res = adaptive.render_adaptive(FakeRenderer(), checkpoint=ck, **{**RULE, "tol": 0.01, "max_spp": 22})
    acc = stand_ins[-1]
    assert acc.calls[0] == "write" and "render" in acc.calls
    assert res.passes[:len(first.passes)] == first.passes and len(res.passes) > len(first.passes)
    assert (res.counts >= first.counts).all() and res.counts.max() == 22
    assert adaptive.AccumCheckpoint(ck).load(json_key())["rule"]["tol"] == 0.01


# --------------------------------------------------------- multi-device --
def multi_of(n):
    m = MultiRenderer.__new__(MultiRenderer)
    m.devices = [0] * n
    m.renderers = [FakeRenderer() for _ in range(n)]
    return m


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("rule", [(4, 32, 4), (3, 17, 5)])
def test_multi_renderer_on_stand_ins(stand_ins, rule, world):
    mn, mx, st = rule
    seen = []
    res = multi_of(world).render_adaptive(6, 5, mx, 2, tol=0.05, min_spp=mn, step_spp=st, floor=0.01,
                                          lanes_per_pixel=4, on_pass=lambda i, n, k: seen.append((i, n, k)))
    sim = simulate(fake_frames(5, 6, mx), 0.05, 0.01, mn, mx, st)
    assert res.passes == sim["passes"]             # the sum over the devices, pass by pass
    assert seen == [(i + 1, n, k) for i, (n, k) in enumerate(res.passes)]
    assert np.array_equal(res.counts, sim["n"]) and np.array_equal(res.fb, sim["mean"])
    assert np.array_equal(res.err, sim["err"])
    assert len(stand_ins) == world
    for d, acc in enumerate(stand_ins):
        assert acc.band.rows() == rank_band(5, d, world) or d == 0
        assert acc.band.lanes_per_pixel == 4
        # select, render, ..., one closing select: a device that has finished
        # is not asked again
        renders = acc.calls.count("render")
        assert acc.calls == ["select", "render"] * renders + ["select"]
        if d >= 5:
            assert renders == 0                    # world 8 on 5 rows: empty bands
    assert stand_ins[0].band.rows() == (0, 5, 1, 0)   # widened for the read
    assert max(acc.calls.count("render") for acc in stand_ins) == len(sim["passes"])


def test_devices_that_finish_early_leave_the_round_robin(monkeypatch, stand_ins):
    """World 2 on a frame whose odd image rows are constant: device 1 is done
    after its first pass (min_spp) and is not selected again while device 0
    goes on."""
    def sample(s, H, W):
        c = FakeAccum.sample(s, H, W)
        c[(H - 1 - np.arange(H)) % 2 == 1] = 1.0
        return c
    monkeypatch.setattr(BandFakeAccum, "sample", staticmethod(sample))
    res = multi_of(2).render_adaptive(6, 5, 32, 2, tol=0.05, min_spp=4, step_spp=4, floor=0.01)
    sim = simulate(np.stack([sample(s, 5, 6) for s in range(32)]), 0.05, 0.01, 4, 32, 4)
    assert res.passes == sim["passes"] and np.array_equal(res.counts, sim["n"])
    assert np.array_equal(res.fb, sim["mean"])
    a0, a1 = stand_ins
    assert a1.calls == ["select", "render", "select"]
    assert a0.calls == ["select", "render"] * len(sim["passes"]) + ["select"] and len(sim["passes"]) > 2
    assert (res.counts[[1, 3]] == 4).all()         # image rows 1, 3 = iy 3, 1: device 1's


def test_multi_renderer_takes_no_checkpoint(stand_ins, tmp_path):
    for kw in (dict(checkpoint=str(tmp_path / "x.npz")), dict(max_passes=2), dict(checkpoint_every=2)):
        with pytest.raises(ValueError, match="not checkpointed"):
            multi_of(2).render_adaptive(6, 5, 8, 2, **kw)
    assert not stand_ins


# ------------------------------------------------------------------ CLI --
def test_cli_local_devices_refusals(tmp_path, monkeypatch):
    from pathtracerpython_amd import _native, launch
    from pathtracerpython_amd import main as cli

    def no_work(*a, **k):
        raise AssertionError("device or rank work started")
    monkeypatch.setattr(launch, "spawn_ranks", no_work)
    monkeypatch.setattr(_native, "lib", no_work)
    ck = str(tmp_path / "x.npz")
    for noise in ([], ["--noise", "0.05"], ["--denoise"]):
        for extra, msg in ((["--devices", "2"], "--local-devices does not combine with --devices"),
                           (["--chunk-spp", "2"], "--local-devices does not combine with --chunk-spp"),
                           (["--checkpoint", ck], "--local-devices does not combine with --chunk-spp"),
                           (["--chunk-spp", "2", "--checkpoint", ck], "--local-devices does not combine")):
            with pytest.raises(SystemExit, match=msg):
                cli.main([CORNELL, "-r", "16", "--local-devices", "2"] + noise + extra)
    with pytest.raises(SystemExit, match="--local-devices must be >= 1"):
        cli.main([CORNELL, "-r", "16", "--local-devices", "0"])
    assert not os.path.exists(ck)
    assert cli.setup([CORNELL]).local_devices is None


def test_cli_noise_takes_a_checkpoint(tmp_path):
    from pathtracerpython_amd import main as cli
    ck = str(tmp_path / "x.npz")
    for extra in ([], ["--denoise"]):
        args = cli.setup([CORNELL, "-r", "16", "--noise", "0.05", "--checkpoint", ck] + extra)
        assert cli.check_args(args) is None and args.checkpoint == ck
    # the refusals around it stay
    for argv, msg in (([CORNELL, "-r", "16", "--checkpoint", ck], "--checkpoint needs --chunk-spp"),
                      ([CORNELL, "-r", "16", "--denoise", "--checkpoint", ck], "--checkpoint needs --chunk-spp"),
                      ([CORNELL, "-r", "16", "--noise", "0.05", "--chunk-spp", "2", "--checkpoint", ck],
                       "--noise does not combine with --chunk-spp / --checkpoint"),
                      ([CORNELL, "-r", "16", "--noise", "0.05", "--devices", "2", "--checkpoint", ck],
                       "--noise runs on one device")):
        with pytest.raises(SystemExit, match=msg):
            cli.check_args(cli.setup(argv))


# ------------------------------------------------------------------ ABI --
def test_abi_has_the_band():
    from pathtracerpython_amd import _native
    assert _abi.PT_API_VERSION == 7   # additive: the version stays
    assert C.sizeof(_abi.PtAccumBand) == 24
    assert [n for n, _ in _abi.PtAccumBand._fields_] == ["row_begin", "row_end", "row_step", "row_phase",
                                                         "lanes_per_pixel", "reserved"]
    b = make_band(9)
    assert (b.rows(), b.lanes_per_pixel, b.reserved) == ((0, 9, 1, 0), 0, 0)
    b = make_band(9, 1, 8, 3, 2, 16)
    assert (b.rows(), b.lanes_per_pixel) == ((1, 8, 3, 2), 16)
    names = ("pt_accum_set_band", "pt_accum_tile_bytes", "pt_accum_export_band_device",
             "pt_accum_import_band_device", "pt_accum_write")
    assert set(names) <= set(_native.EXPORTS)
    lib = _native.lib()   # loading needs no GPU
    for n in names:
        assert getattr(lib, n).argtypes is not None
    hdr = open(os.path.join(ROOT, "include", "pt_capi.h")).read()
    for n in names + ("pt_accum_band",):
        assert n in hdr
    nbytes = C.c_uint64(0)
    assert lib.pt_accum_tile_bytes(37, 23, C.byref(nbytes)) == 0 and nbytes.value == 60 * 37 * 23
    assert nbytes.value == adaptive.tile_bytes(37, 23)
    assert lib.pt_accum_tile_bytes(0, 23, C.byref(nbytes)) == -1
    assert hasattr(adaptive.Accumulator, "set_band") and hasattr(MultiRenderer, "render_adaptive")
