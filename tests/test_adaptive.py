"""Adaptive sampling on the host (pathtracerpython_amd/adaptive.py, pt_path.h
MomentSink): the kernel's moment accumulation compiled for the host against
the oracle's per-sample colours, the stop rule against numpy bit for bit, the
pass loop against a stand-in accumulator, the CLI refusals and the ABI.  The
GPU cases are tests/test_gpu_adaptive.py."""
import ctypes as C
import os

import numpy as np
import pytest

import hostlib
from adaptive_sim import (active_numpy, err_numpy, histogram, k_numpy, oracle_samples, simulate)
from conftest import CORNELL, ROOT

from pathtracerpython_amd import adaptive
from pathtracerpython_amd._abi import make_adapt, make_params

_dp = C.POINTER(C.c_double)
_up = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def accum_host(tmp_path_factory):
    """tests/hostcheck/pt_accum_host.cpp built by the hostcheck Makefile
    into a temporary directory."""
    lib = hostlib.build(tmp_path_factory.mktemp("accum_host"), "pt_accum_host")
    lib.hc_render_moments.restype = C.c_int
    lib.hc_adapt_rule.restype = C.c_int
    lib.hc_adapt_rule.argtypes = [_dp, _dp, _up, C.c_int64, C.c_double, C.c_double, C.c_uint32,
                                  C.c_uint32, C.c_uint32, _dp, C.POINTER(C.c_uint8), _up]
    return lib


def host_moments(lib, packed, p, force64=False, home=0):
    H, W = p.height, p.width
    S = np.zeros((H, W, 3))
    Q = np.zeros((H, W, 3))
    n = np.zeros((H, W), dtype=np.uint32)
    rc = lib.hc_render_moments(C.byref(packed.desc), C.byref(p), int(force64), int(home),
                               S.ctypes.data_as(_dp), Q.ctypes.data_as(_dp), n.ctypes.data_as(_up))
    assert rc == 0
    return S, Q, n


@pytest.fixture(scope="module")
def samples16(packed):
    """Cornell 16x16, 3 bounces, seed 9: the oracle's 8 per-sample frames."""
    return oracle_samples(packed, 16, 16, 3, 9, 8)


def test_host_moments_match_the_oracle_per_sample(accum_host, packed, samples16):
    p = make_params(16, 16, 8, 3, 9)
    S, Q, n = host_moments(accum_host, packed, p)
    dS = float(np.abs(S - samples16.sum(axis=0)).max())
    dQ = float(np.abs(Q - (samples16 ** 2).sum(axis=0)).max())
    print(f"host moments vs oracle: |S - sum c| = {dS:.3e}, |Q - sum c^2| = {dQ:.3e}")
    assert dS <= 1e-12 and dQ <= 1e-12
    assert (n == 8).all()
    # hybrid == forced f64 bit for bit; the two moment homes hold the same bits
    S64, Q64, _ = host_moments(accum_host, packed, p, force64=True)
    assert np.array_equal(S, S64) and np.array_equal(Q, Q64)
    Sm, Qm, _ = host_moments(accum_host, packed, p, home=1)
    assert np.array_equal(S, Sm) and np.array_equal(Q, Qm)


def test_host_moments_continue_across_launches(accum_host, packed):
    """Samples 0..3 and 4..7 in two launches add up to samples 0..7 of one."""
    S8, Q8, _ = host_moments(accum_host, packed, make_params(16, 16, 8, 3, 9))
    Sa, Qa, _ = host_moments(accum_host, packed, make_params(16, 16, 4, 3, 9))
    Sb, Qb, _ = host_moments(accum_host, packed, make_params(16, 16, 4, 3, 9, sample_begin=4))
    assert np.abs(Sa + Sb - S8).max() <= 1e-12 and np.abs(Qa + Qb - Q8).max() <= 1e-12


def test_host_moments_rr_and_no_bounces(accum_host, packed):
    from pathtracerpython_amd._abi import PT_FLAG_RR
    c = oracle_samples(packed, 8, 8, 4, 9, 4, flags=PT_FLAG_RR, rr_depth=1)
    S, Q, _ = host_moments(accum_host, packed, make_params(8, 8, 4, 4, 9, PT_FLAG_RR, 1))
    assert np.abs(S - c.sum(axis=0)).max() <= 1e-12
    assert np.abs(Q - (c ** 2).sum(axis=0)).max() <= 1e-12
    S, Q, n = host_moments(accum_host, packed, make_params(8, 8, 4, 0, 9))
    assert not S.any() and not Q.any() and (n == 4).all()


def test_stop_rule_is_numpy_bit_for_bit(accum_host, samples16):
    """moment_err / adapt_active / adapt_k (the select kernel's code) on the
    moments after 1..8 samples, against the formula in numpy."""
    S = np.zeros((16, 16, 3))
    Q = np.zeros((16, 16, 3))
    for s in range(8):
        S = S + samples16[s]
        Q = Q + samples16[s] ** 2
        n = np.full((16, 16), s + 1, dtype=np.uint32)
        n[0, :5] = [0, 1, 2, 3, 20][:5]    # below two samples, at and past the caps
        for tol, floor, rule in ((0.05, 0.01, (4, 32, 4)), (0.0, 1e-3, (3, 17, 5))):
            err = np.zeros((16, 16))
            act = np.zeros((16, 16), dtype=np.uint8)
            k = np.zeros((16, 16), dtype=np.uint32)
            rc = accum_host.hc_adapt_rule(S.ctypes.data_as(_dp), Q.ctypes.data_as(_dp),
                                          n.ctypes.data_as(_up), 256, tol, floor, *rule,
                                          err.ctypes.data_as(_dp),
                                          act.ctypes.data_as(C.POINTER(C.c_uint8)),
                                          k.ctypes.data_as(_up))
            assert rc == 0
            want = err_numpy(S, Q, n, floor)
            assert np.array_equal(err.view(np.uint64), want.view(np.uint64))
            assert np.isinf(err[0, 0]) and np.isinf(err[0, 1]) and np.isfinite(err[0, 2])
            assert np.array_equal(act.astype(bool), active_numpy(n, want, tol, rule[0], rule[1]))
            assert np.array_equal(k, k_numpy(n, *rule))


def test_simulated_run_on_the_oracle_frames(packed):
    """The numpy simulation of the rule on the oracle's 32 per-sample frames
    of Cornell 24x24, 3 bounces, seed 9: the count maps the GPU test expects."""
    c = oracle_samples(packed, 24, 24, 3, 9, 32)
    r = simulate(c, 0.05, 0.01, 4, 32, 4)
    assert histogram(r["n"]) == {4: 236, 8: 72, 12: 45, 16: 25, 20: 19, 24: 21, 28: 7, 32: 151}
    assert [a for a, _ in r["passes"]] == [576, 340, 268, 223, 198, 179, 158, 151]
    assert sum(k for _, k in r["passes"]) == int(r["n"].sum()) == 8372
    # no stop decision is close to tol (3.38e-4 relative at the closest): sums
    # that differ by 1e-12 cannot flip one
    assert r["margin"] >= 3e-4
    r = simulate(c, 0.05, 0.01, 3, 17, 5)
    assert histogram(r["n"]) == {3: 240, 8: 84, 13: 48, 17: 204}
    var0 = (c.max(axis=0) == c.min(axis=0)).all(axis=-1)
    assert int(var0.sum()) == 96
    # tol = 0: zero-variance pixels stop at min_spp, every other one at max_spp
    r = simulate(c, 0.0, 0.01, 4, 32, 4)
    assert (r["n"][var0] == 4).all() and (r["n"][~var0] == 32).all()


# ------------------------------------------------ the pass loop (host) --
class FakeAccum:
    """A stand-in pt_accum: sample s of pixel e is a known function of (s, e)
    (the keyed-RNG property), the rule evaluated in numpy."""

    def __init__(self, renderer=None, width=6, height=4):
        self.W, self.H = width, height
        self.n = np.zeros((height, width), dtype=np.int64)
        self.S = np.zeros((height, width, 3))
        self.Q = np.zeros((height, width, 3))
        self.calls = []
        self.err = None

    @staticmethod
    def sample(s, H, W):
        e = np.arange(H * W, dtype=np.float64).reshape(H, W, 1)
        # pixels of column 0 are constant (zero variance); the noise grows with e
        amp = np.where(np.arange(H * W).reshape(H, W, 1) % W == 0, 0.0, 0.1 * e)
        return 1.0 + amp * np.sin(1.7 * s + e + np.arange(3))

    def select(self, adapt):
        self.err = err_numpy(self.S, self.Q, self.n, adapt.floor)
        self.act = active_numpy(self.n, self.err, adapt.tol, adapt.min_spp, adapt.max_spp)
        self.k = np.where(self.act, k_numpy(self.n, adapt.min_spp, adapt.max_spp, adapt.step_spp), 0)
        self.calls.append("select")
        return int(self.act.sum()), int(self.k.sum())

    def render(self, params, adapt):
        self.calls.append("render")
        for e in zip(*np.nonzero(self.act)):
            for s in range(self.n[e], self.n[e] + self.k[e]):
                c = self.sample(s, self.H, self.W)[e]
                self.S[e] += c
                self.Q[e] += c * c
        self.n = self.n + self.k

    def read(self, **kw):
        return dict(S=self.S, n=self.n.astype(np.uint32), err=self.err)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass


def fake_frames(H, W, n):
    return np.stack([FakeAccum.sample(s, H, W) for s in range(n)])


@pytest.mark.parametrize("rule", [(4, 32, 4), (3, 17, 5), (2, 2, 7), (8, 8, 3)])
def test_pass_schedule_and_stop(rule):
    mn, mx, st = rule
    acc = FakeAccum()
    adapt = make_adapt(0.05, mx, mn, st, 0.01)
    seen = []
    passes = adaptive.run_passes(acc, make_params(6, 4, mx, 1, 0), adapt,
                                 on_pass=lambda i, n, k: seen.append((i, n, k)))
    sim = simulate(fake_frames(4, 6, mx), 0.05, 0.01, mn, mx, st)
    assert passes == sim["passes"] and np.array_equal(acc.n, sim["n"])
    assert seen == [(i + 1, n, k) for i, (n, k) in enumerate(passes)]
    # select, render, ..., and one closing select that finds nothing
    assert acc.calls == ["select", "render"] * len(passes) + ["select"]
    # the k rule: to min_spp first, then steps that end exactly at max_spp
    assert set(np.unique(acc.n)) <= {mn + i * st for i in range(mx)} | {mx}
    assert (acc.n[:, 0] == mn).all() and acc.n.max() == mx
    done = ~active_numpy(acc.n, err_numpy(acc.S, acc.Q, acc.n, 0.01), 0.05, mn, mx)
    assert done.all()


def test_tol_zero_and_uniform():
    acc = FakeAccum()
    adaptive.run_passes(acc, make_params(6, 4, 12, 1, 0), make_adapt(0.0, 12, 4, 4))
    assert (acc.n[:, 0] == 4).all() and (acc.n[:, 1:] == 12).all()
    acc = FakeAccum()
    passes = adaptive.run_passes(acc, make_params(6, 4, 8, 1, 0), make_adapt(0.5, 8, 8, 3))
    assert passes == [(24, 72), (24, 72), (24, 48)] and (acc.n == 8).all()


def test_runaway_loop_is_an_error():
    class Stuck(FakeAccum):
        def render(self, params, adapt):
            pass
    with pytest.raises(RuntimeError, match="did not end"):
        adaptive.run_passes(Stuck(), make_params(6, 4, 4, 1, 0), make_adapt(0.05, 4, 2, 1))


def test_render_adaptive_on_a_stand_in(monkeypatch):
    class R:
        class scene:
            width, height, seed = 6, 4, 3
    monkeypatch.setattr(adaptive, "Accumulator", FakeAccum)
    seen = []
    res = adaptive.render_adaptive(R(), max_spp=17, bounces=2, tol=0.05, min_spp=3, step_spp=5,
                                   on_pass=lambda i, n, k: seen.append(i))
    sim = simulate(fake_frames(4, 6, 17), 0.05, 0.01, 3, 17, 5)
    assert res.passes == sim["passes"] and seen == list(range(1, len(res.passes) + 1))
    assert res.samples == int(sim["n"].sum()) and res.counts.dtype == np.uint32
    assert np.array_equal(res.counts, sim["n"]) and np.abs(res.fb - sim["mean"]).max() <= 1e-15
    assert res.fb.shape == (4, 6, 3) and res.err.shape == (4, 6)


@pytest.mark.parametrize("bad", [dict(min_spp=1), dict(min_spp=9, max_spp=8), dict(step_spp=0),
                                 dict(tol=-0.1), dict(tol=float("nan")), dict(floor=0.0),
                                 dict(min_spp=2.5)])
def test_argument_validation(bad):
    """Refused before the renderer is touched (None would raise otherwise)."""
    kw = {**dict(max_spp=8, tol=0.05), **bad}
    with pytest.raises(ValueError):
        adaptive.render_adaptive(None, 4, 4, **kw)


# ------------------------------------------------------------------ CLI --
def test_cli_noise_refusals(tmp_path, monkeypatch):
    """--noise with --devices 2, --chunk-spp or --checkpoint is refused before
    any rank process or device work."""
    from pathtracerpython_amd import _native, launch
    from pathtracerpython_amd import main as cli

    def no_work(*a, **k):
        raise AssertionError("device or rank work started")
    monkeypatch.setattr(launch, "spawn_ranks", no_work)
    monkeypatch.setattr(_native, "lib", no_work)
    ck = str(tmp_path / "x.npz")
    for extra, msg in ((["--devices", "2"], "one device"),
                       (["--chunk-spp", "2"], "--chunk-spp"),
                       (["--chunk-spp", "2", "--checkpoint", ck], "--chunk-spp"),
                       (["--min-spp", "1"], "min_spp"),
                       (["--step-spp", "0"], "step_spp")):
        with pytest.raises(SystemExit, match=msg):
            cli.main([CORNELL, "-r", "16", "--noise", "0.05"] + extra)
    with pytest.raises(SystemExit, match="--noise"):
        cli.main([CORNELL, "-r", "16", "--save-aov", str(tmp_path / "a")])
    with pytest.raises(SystemExit, match="tol"):
        cli.main([CORNELL, "-r", "16", "--noise", "-1"])
    assert not os.path.exists(ck)
    a = cli.setup([CORNELL, "--noise", "0.02"])
    assert (a.noise, a.min_spp, a.step_spp, a.save_aov) == (0.02, 8, 8, None)


# ------------------------------------------------------------------ ABI --
def test_abi_has_the_accumulator():
    from pathtracerpython_amd import _abi, _native
    assert _abi.PT_API_VERSION == 7   # additive: the version stays
    assert C.sizeof(_abi.PtAdaptParams) == 32
    assert [n for n, _ in _abi.PtAdaptParams._fields_] == ["tol", "floor", "min_spp", "max_spp",
                                                           "step_spp", "reserved"]
    names = ("pt_accum_create", "pt_accum_destroy", "pt_accum_reset", "pt_accum_select",
             "pt_accum_render", "pt_accum_resolve_device", "pt_accum_read")
    assert set(names) <= set(_native.EXPORTS)
    lib = _native.lib()   # loading needs no GPU
    for n in names:
        assert getattr(lib, n).argtypes is not None
    hdr = open(os.path.join(ROOT, "include", "pt_capi.h")).read()
    for n in names + ("pt_adapt_params",):
        assert n in hdr
    import pathtracerpython_amd as pkg
    assert pkg.render_adaptive is adaptive.render_adaptive
    assert hasattr(pkg.Renderer, "render_adaptive")
