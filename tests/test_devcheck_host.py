"""The CPU side of the device check (tests/devcheck, tests/test_gpu_devcheck.py):
its build recipe mirrors the library's, the cases it runs are the filter
self-test's own, the numpy judgement reproduces the self-test's totals on the
host's verdicts, the host twins of the min / max family keep their contracts,
and the ulp measure measures."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import devcheck_lib as dl
import hp_ref
from conftest import ROOT, quad_scene, random_scene
from pathtracerpython_amd import build as hipbuild
from pathtracerpython_amd.pack import pack_scene


def test_devcheck_flags_mirror_the_library_build():
    """tests/devcheck/Makefile compiles with exactly build.py's FLAGS
    (-ffp-contract=off above all) and with build.py's compiler default."""
    mk = open(os.path.join(ROOT, "tests", "devcheck", "Makefile")).read()
    flags = re.search(r"^FLAGS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert flags == hipbuild.FLAGS
    assert "-ffp-contract=off" in flags and "--offload-arch=gfx950" in flags
    assert re.search(r"^\t\$\(HIPCC\) \$\(FLAGS\) -shared -o \S+ pt_devcheck\.hip$", mk, re.M)
    assert re.search(r"^HIPCC\s*\?=\s*(\S+)$", mk, re.M).group(1) == "/opt/rocm/bin/hipcc"


def test_ulp_measure_has_teeth():
    """A correctly rounded value measures <= 0.5 ulp, one nudged 3 ulp is
    flagged; mpmath and np.longdouble give the same reference."""
    rs = np.random.RandomState(1)
    x = np.ldexp(1.0 + rs.uniform(0, 1, 3000), rs.randint(-1021, 1021, 3000))
    for fn in ("rcp", "rsqrt", "sqrt"):
        hi, lo = hp_ref.ref(fn, x)
        assert hp_ref.ulp_err(hi, hi, lo).max() <= 0.5
        off = hi
        for _ in range(3):
            off = np.nextafter(off, np.inf)
        e = hp_ref.ulp_err(off, hi, lo)
        assert e.min() >= 2.5 and e.max() <= 3.5
        if hp_ref.mpmath is not None and hp_ref.LD_BITS >= 63:
            h2, l2 = hp_ref.ref_bulk(fn, x)     # (double rounding may move hi by one ulp: hi + lo agrees)
            assert np.abs((hi - h2) / np.spacing(np.abs(hi)) + (lo - l2)).max() <= 2.0 ** -9
    # just under a power of two the ulp is the smaller one
    hi, lo = np.array([1.0]), np.array([-0.25])
    assert hp_ref.ulp_err(np.array([1.0 - 2.0 ** -53]), hi, lo)[0] == pytest.approx(0.5)
    assert hp_ref.LD_BITS >= 63 or hp_ref.mpmath is not None


CASES = [("cornell", 2000, 1), ("cornell", 2000, 2), ("quad", 1000, 3), ("mesh200", 500, 12)]


@pytest.mark.parametrize("name,n,seed", CASES, ids=["%s-%d" % (c[0], c[2]) for c in CASES])
def test_filter_cases_are_the_selftest(hostcheck, packed, tmp_path, name, n, seed):
    """hc_filter_cases' totals equal hc_filter_selftest's for the same (n,
    seed), and the totals recomputed in numpy from the exported verdicts and
    the exported truth equal them too: the exported cases are the tested
    cases, and devcheck_lib.judge judges as the self-test does.  The share of
    tests whose f64 decision lies within 1e-12 of a threshold (left out of the
    device's eval64 comparison) stays under 1e-3; shadow_unit_m's host form
    meets the claims the GPU test makes of the device's."""
    pk = {"cornell": lambda: packed, "quad": lambda: pack_scene(quad_scene(tmp_path, 3)),
          "mesh200": lambda: pack_scene(random_scene(tmp_path, 200, 12))}[name]()
    out = (C.c_int64 * 5)()
    assert hostcheck.hc_filter_selftest(C.byref(pk.desc), C.c_int64(n), C.c_uint64(seed), out) == 0
    cases = dl.Cases(hostcheck, pk, n, seed)
    assert cases.totals == list(out)
    j = dl.judge(cases, cases.host)
    assert [j["wrong_total"], j["amb"], j["tests"], j["cand"], j["mdiff"]] == list(out)
    assert j["wrong"] == {k: 0 for k in range(dl.KINDS)} and j["c_mdiff"] == 0
    assert (j["c_tests"] > 0) == (name == "mesh200")
    member = cases.host.code[..., dl.CLOSEST] >= 0
    share = (cases.near != 0).sum() / member.sum()
    print(f"{name} seed {seed}: near-threshold share {share:.2e}")
    assert share <= 1e-3
    sj = dl.judge_shadow_unit(cases, cases.host)
    assert sj["occ"] == 0 and sj["amax"] == 0 and sj["leak"] == 0
    assert sj["certain"] > 0.5 * sj["units"] and sj["moved"] > 0


def test_judge_flags_a_wrong_verdict(hostcheck, packed):
    """A certain verdict turned round, a candidate interval moved off the
    truth and a lost unit test are each counted."""
    cases = dl.Cases(hostcheck, packed, 200, 5)
    r = cases.host
    code, atdt, summ = r.code.copy(), r.atdt.copy(), r.sum.copy()
    i = tuple(np.argwhere(code[..., dl.SHADOW] == dl.K_MISS)[0])
    r.code[i + (dl.SHADOW,)] = dl.K_CAND
    assert dl.judge(cases, r)["wrong"][dl.SHADOW] == 1
    r.code[...] = code
    i = tuple(np.argwhere(code[..., dl.CLOSEST] == dl.K_CAND)[0])
    r.atdt[i[:2] + (0,)] *= 1.01
    assert dl.judge(cases, r)["wrong"][dl.CLOSEST] >= 1
    r.atdt[...] = atdt
    k = tuple(np.argwhere(r.sum[..., 0] <= 0)[0])
    r.sum[k + (0,)] = 1.0
    assert dl.judge_shadow_unit(cases, r)["occ"] + dl.judge_shadow_unit(cases, r)["amax"] >= 1
    r.sum[...] = summ
    assert dl.judge(cases, r)["wrong_total"] == 0


def test_min_max_host_twins_keep_their_contracts(hostcheck):
    """The host twins (what the CPU suite runs in the device instructions'
    place): nan_min / nan_min3 propagate NaN, fmax_q returns the other operand
    of a NaN, med3_q is the median on its domain, pt_canon the identity."""
    V = np.array([0.0, -0.0, 1e-42, -1e-42, 1.0, -1.0, 3.4028235e38, -3.4028235e38, np.inf, -np.inf,
                  np.nan], dtype=np.float32)
    t = np.array(list(itertools.product(V, repeat=3)), dtype=np.float32)
    a, b, c = (np.ascontiguousarray(t[:, i]) for i in range(3))
    out = dl.minmax(hostcheck, a, b, c, entry="hc_minmax").view(np.float32)
    nan2 = np.isnan(a) | np.isnan(b)
    assert np.array_equal(np.isnan(out[:, 0]), nan2)
    assert np.array_equal(np.isnan(out[:, 1]), nan2 | np.isnan(c))
    assert np.array_equal(out[~nan2, 0], np.minimum(a, b)[~nan2])
    one = np.isnan(a) ^ np.isnan(b)
    assert np.array_equal(out[one, 2], np.where(np.isnan(a), b, a)[one])
    ok = ~np.isnan(t).any(axis=1) & (b <= c)
    assert np.array_equal(out[ok, 4], np.median(t[ok], axis=1))
    assert np.array_equal(out[:, 5].view(np.uint32), a.view(np.uint32))
