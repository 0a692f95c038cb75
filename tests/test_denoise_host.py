"""The denoiser on the host (pathtracerpython_amd/csrc/pt_denoise.h compiled by
tests/denoise_host): the per-pixel code against the numpy restatement of
include/pt_capi.h's rule bit for bit, its effect on the oracle's frames, a
sanitizer run of its border addressing as a stand-alone program, and the
ctypes mirror of pt_denoise_params.  GPU side: tests/test_gpu_denoise.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from adaptive_sim import oracle_samples, simulate
from conftest import ROOT
from denoise_ref import (DEFAULTS, SHAPES, denoise_numpy, features_oracle, moments_numpy, rmse,
                         same_bits, synthetic)
from oracle import oracle
from pathtracerpython_amd._abi import DENOISE_DEFAULTS, PtDenoiseParams, make_denoise
from pathtracerpython_amd.render import from_list_order

HOST = os.path.join(ROOT, "tests", "denoise_host")
_dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def hd():
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    lib = C.CDLL(os.path.join(HOST, "build", "libdenoisehost.so"))
    lib.hd_denoise.restype = C.c_int
    lib.hd_denoise.argtypes = [C.c_int32, C.c_int32, C.POINTER(PtDenoiseParams), _dp, _dp,
                               C.POINTER(C.c_int32), _dp, _dp, _dp, _dp]
    lib.hd_moments.restype = None
    lib.hd_moments.argtypes = [_dp, _dp, C.POINTER(C.c_uint32), C.c_int64, _dp, _dp]
    lib.hd_abi_layout.restype = None
    return lib


def host_denoise(lib, a, **kw):
    H, W = a["obj"].shape
    oc, ov = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    d = make_denoise(**kw)
    rc = lib.hd_denoise(W, H, C.byref(d), a["c"].ctypes.data_as(_dp), a["v"].ctypes.data_as(_dp),
                        a["obj"].ctypes.data_as(C.POINTER(C.c_int32)), a["N"].ctypes.data_as(_dp),
                        a["P"].ctypes.data_as(_dp), oc.ctypes.data_as(_dp), ov.ctypes.data_as(_dp))
    assert rc == 0
    return oc, ov


def test_defaults_are_the_headers():
    assert DENOISE_DEFAULTS == DEFAULTS == dict(iters=5, sigma_l=2.0, sigma_z=0.1, eps=1e-10, normal_sq=5)
    d = make_denoise()
    assert (d.iters, d.sigma_l, d.sigma_z, d.eps, d.normal_sq, d.reserved) == (5, 2.0, 0.1, 1e-10, 5, 0)


def test_abi_struct_layout(hd):
    out = (C.c_int64 * 7)()
    hd.hd_abi_layout(out)
    P = PtDenoiseParams
    assert list(out) == [C.sizeof(P), P.sigma_l.offset, P.sigma_z.offset, P.eps.offset, P.iters.offset,
                         P.normal_sq.offset, P.reserved.offset]
    assert C.sizeof(P) == 40 and P.reserved.offset == 32


@pytest.mark.parametrize("iters", [1, 5, 8])
@pytest.mark.parametrize("W,H", SHAPES, ids=lambda x: str(x))
def test_host_build_equals_numpy_bit_for_bit(hd, W, H, iters):
    a = synthetic(W, H)
    oc, ov = host_denoise(hd, a, iters=iters)
    rc, rv = denoise_numpy(a["c"], a["v"], a["obj"], a["N"], a["P"], iters=iters)
    assert np.isfinite(oc).all() and np.isfinite(ov).all()      # zero variances and escapes included
    assert same_bits(oc, rc) and same_bits(ov, rv)


def test_the_synthetic_mixture_has_its_cases():
    for W, H in SHAPES[4:]:
        a = synthetic(W, H)
        esc = a["obj"] < 0
        assert esc.any() and (~esc).any() and len(np.unique(a["obj"])) >= 4
        assert not a["N"][esc].any() and not a["P"][esc].any()
        v = a["v"]
        assert (v == 0).any() and ((v > 0) & (v < 1e-299)).any() and (v > 1e3).any()


def test_other_parameters(hd):
    a = synthetic(37, 19)
    kw = dict(iters=3, sigma_l=0.7, sigma_z=0.03, eps=1e-6, normal_sq=0)
    oc, ov = host_denoise(hd, a, **kw)
    rc, rv = denoise_numpy(a["c"], a["v"], a["obj"], a["N"], a["P"], **kw)
    assert same_bits(oc, rc) and same_bits(ov, rv)
    kw["normal_sq"] = 8
    oc, ov = host_denoise(hd, a, **kw)
    rc, rv = denoise_numpy(a["c"], a["v"], a["obj"], a["N"], a["P"], **kw)
    assert same_bits(oc, rc) and same_bits(ov, rv)


def test_a_skipped_tap_leaves_the_sums_alone(hd):
    """One object per pixel skips every tap but the centre: the pixel keeps its
    colour and variance (to the rounding of w*c/w), in the host build and in
    numpy alike."""
    a = synthetic(5, 7)
    a["obj"] = np.arange(35, dtype=np.int32).reshape(7, 5)
    a["N"][:] = [0.0, 0.0, 1.0]
    oc, ov = host_denoise(hd, a, iters=5)
    # w/w is 1 and (w*w)/(w*w) is 1 for the one tap kept, so c and v are
    # (w*c)/w and (w*w*v)/(w*w): within an ulp or two of the input
    assert np.allclose(oc, a["c"], rtol=1e-15, atol=0) and np.allclose(ov, a["v"], rtol=1e-15, atol=0)
    rc, rv = denoise_numpy(a["c"], a["v"], a["obj"], a["N"], a["P"], iters=5)
    assert same_bits(oc, rc) and same_bits(ov, rv)


def test_moments_equal_numpy_bit_for_bit(hd):
    rs = np.random.RandomState(3)
    n = rs.randint(0, 6, 500).astype(np.uint32)
    S = rs.uniform(0, 3, (500, 3)) * n[:, None]
    Q = S * S / np.maximum(n, 1)[:, None] * rs.uniform(0.9999, 1.5, (500, 3))   # some below S*S/n
    c, v = np.zeros((500, 3)), np.zeros((500, 3))
    hd.hd_moments(S.ctypes.data_as(_dp), Q.ctypes.data_as(_dp), n.ctypes.data_as(C.POINTER(C.c_uint32)), 500,
                  c.ctypes.data_as(_dp), v.ctypes.data_as(_dp))
    rc, rv = moments_numpy(S, Q, n)
    assert (n == 0).any() and (n == 1).any() and (rv == 0).any()
    assert same_bits(c, rc) and same_bits(v, rv)
    assert not c[n == 0].any() and not v[n == 0].any()
    assert np.array_equal(v[n == 1], S[n == 1] * S[n == 1])


# ------------------------------------------------------------ ABI and CLI --
def test_abi_has_the_denoiser():
    from pathtracerpython_amd import _native
    names = ("pt_denoise_device", "pt_denoise", "pt_accum_features", "pt_accum_read_features",
             "pt_accum_denoise_device")
    assert set(names) <= set(_native.EXPORTS)
    lib = _native.lib()   # loading needs no GPU
    for n in names:
        assert getattr(lib, n).argtypes is not None
    hdr = open(os.path.join(ROOT, "include", "pt_capi.h")).read()
    for n in names + ("pt_denoise_params",):
        assert n in hdr
    # bad parameters are refused before any device is looked for
    z = np.zeros(3)
    zi = np.zeros(1, dtype=np.int32)
    for kw in (dict(iters=0), dict(iters=9), dict(normal_sq=9), dict(sigma_l=0.0), dict(sigma_z=-1.0),
               dict(eps=0.0)):
        d = make_denoise(**kw)
        vp = C.c_void_p(z.ctypes.data)
        assert lib.pt_denoise(1, 1, C.byref(d), vp, vp, C.c_void_p(zi.ctypes.data), vp, vp, 0, vp, None) == -1
        assert _native.last_error()


def test_cli_refuses_denoise_combinations(monkeypatch, tmp_path):
    from conftest import CORNELL
    from pathtracerpython_amd import _native, launch
    from pathtracerpython_amd import main as cli

    def no_work(*a, **k):
        raise AssertionError("device or rank work started")
    monkeypatch.setattr(launch, "spawn_ranks", no_work)
    monkeypatch.setattr(_native, "lib", no_work)
    for extra, msg in ((["--devices", "2"], "one device"),
                       (["--chunk-spp", "2"], "--chunk-spp"),
                       (["--denoise-iters", "0"], "iters"),
                       (["--denoise-iters", "9"], "iters"),
                       (["--denoise-sigma", "0"], "sigma")):
        with pytest.raises(SystemExit, match=msg):
            cli.main([CORNELL, "-r", "16", "--denoise"] + extra)
        with pytest.raises(SystemExit, match=msg):
            cli.main([CORNELL, "-r", "16", "--noise", "0.05", "--denoise"] + extra)
    with pytest.raises(SystemExit, match="-r >= 2"):
        cli.main([CORNELL, "-r", "1", "--denoise"])
    a = cli.setup([CORNELL, "--denoise"])
    assert (a.denoise, a.denoise_iters, a.denoise_sigma) == (True, 5, 2.0)
    assert cli.setup([CORNELL]).denoise is False


# ---------------------------------------------------------------- quality --
@pytest.fixture(scope="module")
def cornell48(packed):
    """Cornell 48 x 48, 4 bounces: the oracle's 32 per-sample frames of seed 9,
    its 1024-spp frame of seed 10 (the yardstick) and the first-hit features."""
    frames = oracle_samples(packed, 48, 48, 4, 9, 32)
    ref, _ = oracle.render(packed, 48, 48, 1024, 4, 10)
    return frames, from_list_order(ref, 48, 48), features_oracle(packed, 48, 48)


def quality(hd, S, Q, n, feat, ref):
    c, v = moments_numpy(S, Q, n)
    _, obj, N, P = feat
    a = dict(c=np.ascontiguousarray(c), v=np.ascontiguousarray(v), obj=obj, N=N, P=P)
    oc, _ = host_denoise(hd, a)
    return rmse(c, ref), rmse(oc, ref)


def test_uniform_16spp_rmse_ratio(hd, cornell48):
    frames, ref, feat = cornell48
    S, Q = frames[:16].sum(axis=0), (frames[:16] ** 2).sum(axis=0)
    noisy, filt = quality(hd, S, Q, np.full((48, 48), 16, dtype=np.uint32), feat, ref)
    print(f"uniform 16 spp: RMSE noisy {noisy:.5f}, filtered {filt:.5f}, ratio {filt / noisy:.3f}")
    assert filt / noisy <= 0.70


def test_simulated_adaptive_rmse_ratio(hd, cornell48):
    frames, ref, feat = cornell48
    sim = simulate(frames, 0.05, 0.01, 4, 32, 4)
    noisy, filt = quality(hd, sim["S"], sim["Q"], sim["n"].astype(np.uint32), feat, ref)
    print(f"adaptive (4, 32, 4) tol 0.05, {sim['n'].mean():.1f} spp mean: RMSE noisy {noisy:.5f}, "
          f"filtered {filt:.5f}, ratio {filt / noisy:.3f}")
    assert filt / noisy <= 0.70


# -------------------------------------------------------------- sanitizer --
def test_sanitizer_program_over_the_shapes():
    """ASan + UBSan over the host tap function, as a program of its own."""
    subprocess.run(["make", "-s", "-C", HOST, "sanitize"], check=True)
    r = subprocess.run([os.path.join(HOST, "build", "denoise_san")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "21 runs ok" in r.stdout
