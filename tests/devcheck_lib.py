"""The device check library (tests/devcheck): loading it, its entry points as
numpy functions, the host's filter cases (hostcheck's hc_filter_cases) and the
judgement of a set of verdicts against the host's f64 truth — the same numpy
code judges the host's own verdicts on the CPU and the device's on the GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "devcheck")
LIB = os.path.join(DIR, "build", "libdevcheck.so")

K_MISS, K_CAND, K_AMB = 0, 1, 2
# verdict kinds of a slot (filter_eval.h)
CLOSEST, SHADOW, MARGIN, QUAD_SHADOW, QUAD_CLOSEST, LEAN, C_CLOSEST, C_SHADOW, C_MARGIN = range(9)
KINDS = 9
KIND_NAMES = ("closest", "shadow", "margin", "quad shadow", "quad closest", "lean closest",
              "64-B closest", "64-B shadow", "64-B margin")
CLOSEST_KINDS = (CLOSEST, QUAD_CLOSEST, LEAN, C_CLOSEST)
SUM_N = 7
K_ZERO = 1e-5


def load():
    """libdevcheck.so, built here if it is missing; a failure of either is an
    error (never a skip)."""
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", DIR], check=True)
    lib = C.CDLL(LIB)
    for f in ("dc_math_f64", "dc_unit_any", "dc_rcp_weak", "dc_rcpf", "dc_minmax", "dc_filter"):
        getattr(lib, f).restype = C.c_int
    return lib


@pytest.fixture(scope="session")
def devcheck():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return load()


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def math_f64(lib, x):
    """(n, 5): rcp_d, rsqrt_d, sqrt_d, sincos_small's sin and cos."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty((x.size, 5), dtype=np.float64)
    rc = lib.dc_math_f64(_p(x, C.c_double), C.c_int64(x.size), _p(out, C.c_double))
    assert rc == 0, rc
    return out


def unit_any(lib, v):
    """(unit_any(v), unit(v)), (n, 3) each, of the device."""
    v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1, 3)
    out = np.empty((v.shape[0], 6), dtype=np.float64)
    rc = lib.dc_unit_any(_p(v, C.c_double), C.c_int64(v.shape[0]), _p(out, C.c_double))
    assert rc == 0, rc
    return out[:, :3], out[:, 3:]


def rcp_weak(lib, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty(x.size, dtype=np.float64)
    rc = lib.dc_rcp_weak(_p(x, C.c_double), C.c_int64(x.size), _p(out, C.c_double))
    assert rc == 0, rc
    return out


def rcpf(lib, x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty(x.size, dtype=np.float32)
    rc = lib.dc_rcpf(_p(x, C.c_float), C.c_int64(x.size), _p(out, C.c_float))
    assert rc == 0, rc
    return out


def minmax(lib, a, b, c, entry="dc_minmax"):
    """(n, 6) uint32 bit patterns: nan_min, nan_min3, fmax_q, min3f, med3_q,
    pt_canon — of the device library, or of hostcheck with entry="hc_minmax"."""
    a, b, c = (np.ascontiguousarray(v, dtype=np.float32) for v in (a, b, c))
    out = np.empty((a.size, 6), dtype=np.uint32)
    rc = getattr(lib, entry)(_p(a, C.c_float), _p(b, C.c_float), _p(c, C.c_float),
                             C.c_int64(a.size), _p(out, C.c_uint32))
    assert rc == 0, rc
    return out


# ------------------------------------------------------------ filter cases --
class Results:
    """One build's results of the cases (filter_eval.h FilterOut)."""

    def __init__(self, n, nu, n_obj_unit):
        self.code = np.full((n, nu, 2, KINDS), -9, dtype=np.int8)
        self.hit = np.zeros((n, nu, 2), dtype=np.int8)
        self.sqd = np.zeros((n, nu, 2), dtype=np.float64)
        self.atdt = np.zeros((n, nu, 4), dtype=np.float32)
        self.mflag = np.full((n, nu), -9, dtype=np.int8)
        self.sum = np.zeros((n, n_obj_unit, SUM_N), dtype=np.float32)

    def args(self):
        return (_p(self.code, C.c_int8), _p(self.hit, C.c_int8), _p(self.sqd, C.c_double),
                _p(self.atdt, C.c_float), _p(self.mflag, C.c_int8), _p(self.sum, C.c_float))


class Cases:
    """The lines of hc_filter_selftest(n, seed) on a scene with the host
    build's results of them: `host.hit`, `host.sqd` are the f64 truth."""

    def __init__(self, hostcheck, packed, n, seed):
        dims = (C.c_int32 * 4)()
        assert hostcheck.hc_filter_dims(C.byref(packed.desc), dims) == 0
        self.n_unit, self.n_bunit, self.n_obj_unit, self.has_unitc = (int(v) for v in dims)
        self.packed, self.n, self.seed = packed, n, seed
        self.nu = self.n_unit + self.n_bunit
        self.o = np.zeros((n, 3))
        self.dn = np.zeros((n, 3))
        self.lim = np.zeros(n)
        self.hlo = np.zeros(n, dtype=np.float32)
        self.hhi = np.zeros(n, dtype=np.float32)
        self.at_eye = np.zeros(n, dtype=np.int32)
        self.host = Results(n, self.nu, self.n_obj_unit)
        # the host's f64 decisions within 1e-12 (relative) of a threshold
        self.near = np.zeros((n, self.nu, 2), dtype=np.int8)
        out = (C.c_int64 * 5)()
        rc = hostcheck.hc_filter_cases(C.byref(packed.desc), C.c_int64(n), C.c_uint64(seed),
                                       *self.line_args(), *self.host.args(),
                                       _p(self.near, C.c_int8), out)
        assert rc == 0, rc
        self.totals = list(out)

    def line_args(self):
        return (_p(self.o, C.c_double), _p(self.dn, C.c_double), _p(self.lim, C.c_double),
                _p(self.hlo, C.c_float), _p(self.hhi, C.c_float), _p(self.at_eye, C.c_int32))

    def device(self, lib):
        r = Results(self.n, self.nu, self.n_obj_unit)
        rc = lib.dc_filter(C.byref(self.packed.desc), C.c_int64(self.n), *self.line_args(), *r.args())
        assert rc == 0, rc
        return r


def judge(cases, r):
    """Verdicts `r` (the host's own or the device's) against the host's f64
    truth.  Returns a dict: `wrong[kind]` certain verdicts that contradict the
    truth (closest kinds: or whose |t| interval misses sqrt(sqd)), `amb`,
    `tests`, `cand`, `mdiff` as hc_filter_selftest counts them (kinds 0..5),
    and the 64-B form's own counts."""
    T = cases.host
    h = T.hit != 0
    ref_c = h & (T.sqd > K_ZERO)
    ref_s = h & ~(T.sqd < K_ZERO) & (T.sqd < cases.lim[:, None, None])
    sq = np.sqrt(T.sqd)
    code = r.code.astype(np.int64)
    assert (code >= -1).all() and (code <= K_AMB).all(), "slots the kernel did not write"
    assert (r.mflag >= 0).all()
    wrong = {}
    for k in range(KINDS):
        c = code[..., k]
        ref = ref_c if k in CLOSEST_KINDS else ref_s
        w = (c >= 0) & (c != K_AMB) & ((c == K_CAND) != ref)
        if k in (CLOSEST, C_CLOSEST):   # the candidate's |t| interval must cover the truth
            at = r.atdt[..., 0 if k == CLOSEST else 2].astype(np.float64)[..., None]
            dt = r.atdt[..., 1 if k == CLOSEST else 3].astype(np.float64)[..., None]
            w |= (c == K_CAND) & ref & ((sq < at - dt) | (sq > at + dt))
        wrong[k] = int(w.sum())
    counted = (CLOSEST, SHADOW, QUAD_SHADOW, QUAD_CLOSEST)
    tests = sum(int((code[..., k] >= 0).sum()) for k in counted)
    amb = sum(int((code[..., k] == K_AMB).sum()) for k in counted)
    cand = int(((code[..., CLOSEST] == K_CAND) & ref_c).sum())

    def relation(a, b):   # form b against form a: the same, or a miss that became ambiguous
        ca, cb = code[..., a], code[..., b]
        return int(((ca >= 0) & (cb != ca) & ~((ca == K_MISS) & (cb == K_AMB))).sum())

    mdiff = relation(SHADOW, MARGIN) + relation(QUAD_CLOSEST, LEAN) + \
        int((r.mflag & 1 != 0).sum()) + int((r.mflag & 2 != 0).sum())
    return dict(wrong=wrong, wrong_total=sum(wrong[k] for k in range(6)), amb=amb, tests=tests,
                cand=cand, mdiff=mdiff,
                c_tests=int((code[..., C_CLOSEST] >= 0).sum() + (code[..., C_SHADOW] >= 0).sum()),
                c_amb=int((code[..., C_CLOSEST] == K_AMB).sum() + (code[..., C_SHADOW] == K_AMB).sum()),
                c_mdiff=relation(C_SHADOW, C_MARGIN),
                merged=int((r.mflag != 0).sum()))


def judge_shadow_unit(cases, r):
    """shadow_unit_m's outputs (the line as each of its three shadow rays, the
    state a unit is entered with: nothing occluded, nothing ambiguous, no
    leak) against the truth.  Returns the counts of violations:
      occ   oc[k] > 0 where no member truly occludes the line
      amax  amax < 0 (nothing left for f64) where some oc[k] > 0 differs from
            the truth, i.e. a test was not certain and correct
      leak  key2 / leak moved where no member truly occludes the last ray, or
            moved to anything but the unit's object
    and `certain`, the units decided without f64 (amax < 0)."""
    T = cases.host
    nou = cases.n_obj_unit
    h = T.hit[:, :nou] != 0
    sqd = T.sqd[:, :nou]
    occ_true = (h & ~(sqd < K_ZERO) & (sqd < cases.lim[:, None, None])).any(axis=-1)
    oc = r.sum[..., 0:3]
    amax, key2, leak = r.sum[..., 3], r.sum[..., 4], r.sum[..., 5]
    assert not np.isnan(amax).any()
    n_obj = cases.packed.n_obj
    occ = int(((oc > 0) & ~occ_true[..., None]).sum())
    am = int(((amax < 0)[..., None] & ((oc > 0) != occ_true[..., None])).sum())
    moved = (key2 != n_obj) | (leak != n_obj - 1)
    obj = r.sum[..., 6]
    lk = int((moved & ~occ_true).sum() + (moved & ((key2 != obj) | (leak != obj))).sum())
    return dict(occ=occ, amax=am, leak=lk, certain=int((amax < 0).sum()), units=int(amax.size),
                occluded=int(occ_true.sum()), moved=int(moved.sum()))
