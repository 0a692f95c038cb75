"""The device-only code of the product headers on the GPU (tests/devcheck):
everything behind `#if defined(__HIP_DEVICE_COMPILE__)`, which the host check
replaces by a host twin and which whole frames only reach by chance.

1. rcp_d, rsqrt_d, sqrt_d, sincos_small against a high-precision reference
   (hp_ref.py: mpmath at 100 bits) on the inputs the tracer feeds them;
2. rcpf (v_rcp_f32) against the share of the filter's eq budget it is given;
3. the min / max family against the host twins the CPU suite tests instead;
4. the filter self-test (hostcheck's lines, the host's f64 truth) run by the
   device's own arithmetic, in the Cornell frame and off it (frames.py);
5. frames of the off-frame scenes through Renderer.
"""
import itertools

import numpy as np
import pytest

import devcheck_lib as dl
import frames
import hp_ref
from conftest import quad_scene, random_scene
from devcheck_lib import devcheck   # noqa: F401  (fixture)
from oracle import oracle
from pathtracerpython_amd.pack import pack_scene
from pathtracerpython_amd.render import Renderer, to_list_order

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------ 1. f64 math --
EXPS = [-1021, -600, -40, -17, -1, 0, 1, 17, 40, 600, 1020]   # odd and even: sqrt's [1, 4)
# limits (ulps), derived in pt_math.h's terms:
#   rcp_d   the last step is one rounded fma on a 2^-48-accurate iterate, so
#           the result is faithfully rounded: error < 1 ulp
#   rsqrt_d the rounded product h * y adds up to about half an ulp: <= 2 ulp
#   sqrt_d  one more rounded multiply (x * rsqrt_d(x)): <= 3 ulp
RCP_ULP, RSQRT_ULP, SQRT_ULP = 1.0, 2.0, 3.0
# sincos_small: the reduction drops the third part of pi/2, so its error is
# absolute, not relative, next to a zero of sin or cos
SINCOS_ABS = 2.0 ** -52
SUMSQ_ABS = 2.0 ** -51


def grid():
    """Per exponent: 2^14 random 52-bit mantissas and the 256 nearest each
    end of [1, 2); positive."""
    rs = np.random.RandomState(20)
    out = []
    for e in EXPS:
        m = np.concatenate([rs.randint(0, 2 ** 52, 2 ** 14, dtype=np.int64),
                            np.arange(256, dtype=np.int64),
                            2 ** 52 - 1 - np.arange(256, dtype=np.int64)])
        out.append(np.ldexp(1.0 + m.astype(np.float64) * 2.0 ** -52, e))
    x = np.concatenate(out)
    assert np.isfinite(x).all() and (x >= 2.0 ** -1022).all()
    return x


def bounce_k():
    """k of u = k 2^-24: every k < 4096, every k > 2^24 - 4096, every 16th
    between; (ends, bulk)."""
    ends = np.concatenate([np.arange(4096), np.arange(2 ** 24 - 4095, 2 ** 24)])
    return ends.astype(np.float64), np.arange(4096, 2 ** 24 - 4095, 16).astype(np.float64)


@pytest.fixture(scope="module")
def grid_out(devcheck):
    x = grid()
    return x, dl.math_f64(devcheck, x)


def test_rcp_d(devcheck, grid_out):
    x, out = grid_out
    hi, lo = hp_ref.ref("rcp", x)
    e = max(hp_ref.ulp_err(out[:, 0], hi, lo).max(),
            hp_ref.ulp_err(dl.math_f64(devcheck, -x)[:, 0], -hi, -lo).max())   # both signs
    print(f"rcp_d: max {e:.4f} ulp over {2 * x.size} inputs")
    assert e < RCP_ULP


def test_weak_rcp_twin_fails_the_limit(devcheck):
    """The same check rejects rcp_d with one Newton step (devcheck's own
    deliberately weak twin): the limit has teeth."""
    x = grid()[::7]
    hi, lo = hp_ref.ref("rcp", x)
    e = hp_ref.ulp_err(dl.rcp_weak(devcheck, x), hi, lo).max()
    print(f"one-step rcp: max {e:.2f} ulp")
    assert not e < RCP_ULP


def test_rsqrt_d_sqrt_d(devcheck, grid_out):
    x, out = grid_out
    hi, lo = hp_ref.ref("rsqrt", x)
    er = hp_ref.ulp_err(out[:, 1], hi, lo).max()
    hi, lo = hp_ref.ref("sqrt", x)
    es = hp_ref.ulp_err(out[:, 2], hi, lo).max()
    print(f"rsqrt_d: max {er:.4f} ulp, sqrt_d: max {es:.4f} ulp over {x.size} inputs")
    assert er <= RSQRT_ULP
    assert es <= SQRT_ULP


def test_sqrt_d_bounce_inputs(devcheck):
    """bounce's own arguments: u = k 2^-24 and 1 - u; sqrt_d(0) is 0."""
    ends, bulk = bounce_k()
    worst = 0.0
    for k, ref in ((ends, hp_ref.ref), (bulk, hp_ref.ref_bulk)):
        u = k * 2.0 ** -24
        for x in (u, 1.0 - u):
            got = dl.math_f64(devcheck, x)[:, 2]
            z = x == 0.0
            assert (got[z] == 0.0).all() and not np.signbit(got[z]).any()
            hi, lo = ref("sqrt", x[~z])
            worst = max(worst, hp_ref.ulp_err(got[~z], hi, lo).max())
    assert dl.math_f64(devcheck, np.zeros(1))[0, 2] == 0.0
    print(f"sqrt_d on bounce's inputs: max {worst:.4f} ulp")
    assert worst <= SQRT_ULP


def test_sincos_small(devcheck):
    ends, bulk = bounce_k()
    rs = np.random.RandomState(21)
    j = np.arange(6) * (np.pi / 2)
    near = np.concatenate([j, np.nextafter(j, 8.0), np.nextafter(j[1:], 0.0),
                           [5e-324, 2.0 ** -1022]])
    sets = [(6.28 * (ends * 2.0 ** -24), hp_ref.ref),        # th = fl(kTau u): 6.28, not 2 pi
            (6.28 * (bulk * 2.0 ** -24), hp_ref.ref_bulk),
            (rs.uniform(0.0, 8.0, 2 ** 16), hp_ref.ref),
            (near, hp_ref.ref)]
    worst = wsum = 0.0
    for x, ref in sets:
        assert (x >= 0).all() and (x < 8).all()
        out = dl.math_f64(devcheck, x)
        for col, fn in ((3, "sin"), (4, "cos")):
            hi, lo = ref(fn, x)
            worst = max(worst, hp_ref.abs_err(out[:, col], hi, lo).max())
        wsum = max(wsum, np.abs(hp_ref.sumsq_minus_1(out[:, 3], out[:, 4])).max())
    print(f"sincos_small: max abs error {worst / 2.0 ** -52:.4f} x 2^-52, "
          f"|s^2 + c^2 - 1| max {wsum / 2.0 ** -51:.4f} x 2^-51")
    assert worst <= SINCOS_ABS
    assert wsum <= SUMSQ_ABS


# ---------------------------------------------------------------- 2. rcpf --
# The filter's eq (pt_prepare.h, "P.eq = s * aff_err(nd3, 0.0, 1.0) + 8 * u *
# n1": the 8u n1 >= 8u|q| "covering the rounding of 1/q and t") gives the
# error of t = -h * rcpf(q) a share of 3u|t| (pt_core.h ray_plane_e: "eq
# absorbs the 3u|t| of 1/q and t"): 2u for a 1-ulp reciprocal, u for the
# product.  So |rcpf(q) q - 1| must stay within 2u = 2^-23.
RCPF_REL = 2.0 ** -23


@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["pos", "neg"])
@pytest.mark.parametrize("e", [-17, -8, -1, 0])
def test_rcpf_all_mantissas(devcheck, e, sign):
    """Every f32 mantissa at four exponents bracketing |q| from the 1e-5
    threshold to 1."""
    m = np.arange(2 ** 23, dtype=np.float64)
    x = (sign * np.ldexp(1.0 + m * 2.0 ** -23, e)).astype(np.float32)
    r = dl.rcpf(devcheck, x).astype(np.float64)
    xd = x.astype(np.float64)
    q = 1.0 / xd                                # the exact quotient, rounded to 53 bits
    ulps = np.abs(r - q) / np.spacing(np.abs(q).astype(np.float32)).astype(np.float64)
    rel = np.abs(r * xd - 1.0)                  # (24 x 24 bits: the product is exact)
    print(f"rcpf 2^{e} {'+' if sign > 0 else '-'}: max {ulps.max():.4f} ulp, "
          f"|r q - 1| max {rel.max() / RCPF_REL:.4f} x 2^-23")
    assert rel.max() <= RCPF_REL


def test_rcpf_specials(devcheck):
    inf = np.float32(np.inf)
    x = np.array([0.0, -0.0, inf, -inf, np.nan, 2.0 ** -126, -2.0 ** -126, 2.0 ** -140, 2.0 ** -149],
                 dtype=np.float32)
    r = dl.rcpf(devcheck, x)
    print("rcpf of", list(x), "=", list(r))
    assert r[0] == inf and r[1] == -inf
    assert r[2] == 0 and not np.signbit(r[2]) and r[3] == 0 and np.signbit(r[3])
    assert np.isnan(r[4])
    # smallest normal and denormals: whatever the instruction returns (printed
    # above; a reciprocal above FLT_MAX is inf), the test cannot be a certain
    # candidate, since rcand needs |q| > qhi and qhi >= (1e-5 + eq)(1 + 1e-4)
    # (pt_prepare.h make_unit) — and it returns no NaN for them
    qhi_min = np.float32(1e-5 * (1 + 1e-4))
    assert (np.abs(x[5:]) < qhi_min).all()
    assert not np.isnan(r[5:]).any() and (r[5] > 0) and (r[6] < 0)


# --------------------------------------------------------- 3. min and max --
FMAX = np.finfo(np.float32).max
VALUES = np.array([0.0, -0.0, 1e-42, -1e-42, 1.0, -1.0, FMAX, -FMAX, np.inf, -np.inf, np.nan],
                  dtype=np.float32)
NAN_MIN, NAN_MIN3, FMAX_Q, MIN3F, MED3_Q, CANON = range(6)
NAMES = ("nan_min", "nan_min3", "fmax_q", "min3f", "med3_q", "pt_canon")
READS = {NAN_MIN: (0, 1), NAN_MIN3: (0, 1, 2), FMAX_Q: (0, 1), MIN3F: (0, 1, 2), MED3_Q: (0, 1, 2),
         CANON: (0,)}


def test_min_max_family_equals_host_twins(devcheck, hostcheck):
    """All pairs and triples of {+-0, +-denormal, +-1, +-FLT_MAX, +-inf, NaN}:
    the device result has the host twin's NaN-ness and otherwise its value.
    med3_q only on the triples its contract allows (b <= c, no NaN).  The sign
    of a zero result is compared where the host twin defines it: pt_canon
    always (the identity); nan_min, nan_min3, fmax_q, min3f and med3_q unless
    their operands hold zeros of both signs (fminf / fmaxf leave the sign of
    min(+0, -0) open)."""
    t = np.array(list(itertools.product(VALUES, repeat=3)), dtype=np.float32)
    a, b, c = (np.ascontiguousarray(t[:, i]) for i in range(3))
    dev = dl.minmax(devcheck, a, b, c)
    host = dl.minmax(hostcheck, a, b, c, entry="hc_minmax")
    ops = np.stack([a, b, c], axis=1)
    for f in range(6):
        d, h = dev[:, f].view(np.float32), host[:, f].view(np.float32)
        rd = ops[:, list(READS[f])]
        use = np.ones(len(t), dtype=bool)
        if f == MED3_Q:
            use = ~np.isnan(rd).any(axis=1) & (b <= c)
        assert np.array_equal(np.isnan(d[use]), np.isnan(h[use])), NAMES[f]
        ok = use & ~np.isnan(h)
        assert np.array_equal(d[ok], h[ok]), NAMES[f]
        zeros = rd == 0
        mixed = (zeros & np.signbit(rd)).any(axis=1) & (zeros & ~np.signbit(rd)).any(axis=1)
        sgn = ok & (h == 0) & (~mixed if f != CANON else True)
        assert np.array_equal(np.signbit(d[sgn]), np.signbit(h[sgn])), NAMES[f] + " zero sign"
    # the claims the margins rest on, of the device results themselves
    nan2 = np.isnan(a) | np.isnan(b)
    assert np.isnan(dev[:, NAN_MIN].view(np.float32)[nan2]).all()           # propagates NaN
    assert np.isnan(dev[:, NAN_MIN3].view(np.float32)[nan2 | np.isnan(c)]).all()
    fm = dev[:, FMAX_Q].view(np.float32)
    one = np.isnan(a) ^ np.isnan(b)                                         # quiet NaN: the other operand
    other = np.where(np.isnan(a), b, a)
    assert np.array_equal(fm[one].view(np.uint32), other[one].view(np.uint32))
    for v in (np.inf, -np.inf, -1.0):                                       # cop's values: the identity
        k = a.view(np.uint32) == np.float32(v).view(np.uint32)
        assert k.any() and (dev[k, CANON] == np.float32(v).view(np.uint32)).all()


# ------------------------------------------------- 4. the filter self-test --
def check_filter(devcheck, hostcheck, pk, n, seed, what, bar):
    cases = dl.Cases(hostcheck, pk, n, seed)
    r = cases.device(devcheck)
    hj, dj = dl.judge(cases, cases.host), dl.judge(cases, r)
    assert hj["wrong_total"] == 0 and hj["mdiff"] == 0      # the host's own (the CPU suite's claim)
    print(f"{what}: {dj['tests']} tests, ambiguous device {dj['amb']} / host {hj['amb']}, "
          f"64-B form device {dj['c_amb']} / host {hj['c_amb']} of {dj['c_tests']}")
    # no certain device verdict contradicts the host's f64 truth, in any kind,
    # and every certain closest candidate's |t| interval holds sqrt(sqd)
    assert dj["wrong"] == {k: 0 for k in range(dl.KINDS)}, dj["wrong"]
    assert dj["tests"] == hj["tests"] and dj["cand"] > 0
    # margin form against classify_tri, lean against full closest range, the
    # merged unit margins: the relations the host asserts, of the device's values
    assert dj["mdiff"] == 0 and dj["c_mdiff"] == 0 and dj["merged"] == 0
    # device and host verdicts differ only between certain and ambiguous
    dc, hc = r.code, cases.host.code
    diff = dc != hc
    # (that this is another arithmetic than the host's shows in the plane
    # parts: v_rcp_f32 against the host twin's IEEE division)
    tdiff = int((r.atdt.view(np.uint32) != cases.host.atdt.view(np.uint32)).sum())
    print(f"{what}: {int(diff.sum())} verdicts differ between device and host, "
          f"{tdiff} of {r.atdt.size} |t| and dt values")
    assert tdiff > 0
    assert ((dc[diff] == dl.K_AMB) | (hc[diff] == dl.K_AMB)).all()
    if bar:      # the host test's bar (test_filter_never_wrong_cornell)
        assert dj["amb"] < 0.02 * dj["tests"]
    else:
        # off the Cornell frame the host's own share passes 2 % (x 1e4: 5.8 %
        # of the tests, the bounds grow with the extent), so the bar there is
        # the host's count: the device may turn borderline tests ambiguous,
        # not double them
        assert dj["amb"] < max(2 * hj["amb"], 0.02 * dj["tests"])
    # shadow_unit_m, the render loop's function, with full waves
    sj = dl.judge_shadow_unit(cases, r)
    print(f"{what}: shadow_unit_m {sj}")
    assert sj["occ"] == 0 and sj["amax"] == 0 and sj["leak"] == 0
    assert sj["certain"] > 0.5 * sj["units"]
    # (a scene scaled up has no occluder within the generator's unscaled shadow range)
    assert sj["moved"] > 0 or sj["occluded"] == 0
    return cases, r


def check_eval64(cases, r, what):
    """The device's eval64 (rcp_d inside) against the host's: the hit flag and
    sqd to 4 ulp on every test whose host decision is not within 1e-12
    (relative) of a threshold; those excluded are at most 1e-3 of the tests."""
    T = cases.host
    member = T.code[..., dl.CLOSEST] >= 0
    use = member & (cases.near == 0)
    share = 1.0 - use.sum() / member.sum()
    ulps = np.abs(r.sqd - T.sqd)[use] / np.spacing(np.abs(T.sqd[use]))
    print(f"{what}: eval64 excluded share {share:.2e}, sqd max {ulps.max():.2f} ulp, "
          f"hit flags differing {int((r.hit != T.hit)[use].sum())}")
    assert share <= 1e-3
    assert np.array_equal(r.hit[use], T.hit[use])
    assert ulps.max() <= 4


FILTER_SCENES = [("cornell-1", 2000, 1), ("cornell-2", 2000, 2), ("quad", 1000, 3), ("mesh200", 500, 12)]


def filter_scene(name, packed, tmp_path):
    if name.startswith("cornell"):
        return packed
    if name == "quad":
        return pack_scene(quad_scene(tmp_path, 3))     # skew pairs and every labelling
    return pack_scene(random_scene(tmp_path, 200, 12))  # BVH units


@pytest.fixture(scope="module")
def filter_runs():
    return {}


@pytest.mark.parametrize("name,n,seed", FILTER_SCENES, ids=[s[0] for s in FILTER_SCENES])
def test_filter_selftest_on_device(devcheck, hostcheck, packed, tmp_path, filter_runs, name, n, seed):
    pk = filter_scene(name, packed, tmp_path)
    filter_runs[name] = check_filter(devcheck, hostcheck, pk, n, seed, name, bar=True)
    if name == "mesh200":
        assert filter_runs[name][0].has_unitc     # the walks' 64-B leaf form went through it too


@pytest.mark.parametrize("name,n,seed", FILTER_SCENES, ids=[s[0] for s in FILTER_SCENES])
def test_device_eval64_equals_host(devcheck, hostcheck, packed, tmp_path, filter_runs, name, n, seed):
    if name not in filter_runs:
        cases = dl.Cases(hostcheck, filter_scene(name, packed, tmp_path), n, seed)
        filter_runs[name] = (cases, cases.device(devcheck))
    check_eval64(*filter_runs[name], name)


# ------------------------------------------------ 5. off the Cornell frame --
@pytest.fixture(scope="module")
def base_scenes(packed, tmp_path_factory):
    return {"cornell": packed,
            "mesh": pack_scene(random_scene(tmp_path_factory.mktemp("offframe"), 300, 21))}


@pytest.mark.parametrize("fname", frames.GPU_FRAMES)
def test_filter_selftest_off_frame(devcheck, hostcheck, base_scenes, fname):
    _, s, tx, ty = frames.frame(fname)
    for scene, n in (("cornell", 1000), ("mesh", 200)):
        pk = frames.transformed(base_scenes[scene], s, tx, ty)
        check_filter(devcheck, hostcheck, pk, n, 3, f"{scene} {fname}", bar=False)


@pytest.mark.parametrize("fname", frames.GPU_FRAMES)
@pytest.mark.parametrize("scene", ["cornell", "mesh"])
def test_frames_off_frame(base_scenes, scene, fname):
    """12 x 12 x 2 spp x 4 bounces through Renderer: hybrid == forced f64 bit
    for bit, the wavefront kernels == the single kernel bit for bit (the BVH
    scene), the oracle within the frame's tolerance (frames.py)."""
    _, s, tx, ty = frames.frame(fname)
    pk = frames.transformed(base_scenes[scene], s, tx, ty)
    W, H, spp, B, seed = frames.FRAME
    with Renderer(None, packed=pk) as r:
        a = r.render(W, H, spp, B, seed, out_f64=True)
        b = r.render(W, H, spp, B, seed, out_f64=True, force_f64=True)
        assert np.array_equal(a, b)
        if scene == "mesh":
            m = r.render(W, H, spp, B, seed, out_f64=True, megakernel=True)
            assert np.array_equal(a, m)
            mf = r.render(W, H, spp, B, seed, out_f64=True, megakernel=True, force_f64=True)
            assert np.array_equal(a, mf)
    ref, _ = oracle.render(pk, W, H, spp, B, seed)
    err = frames.rel_err(to_list_order(a), ref)
    print(f"{scene} {fname}: relative L-inf vs oracle {err:.3e} (tolerance "
          f"{frames.oracle_tol(scene, fname):.3e})")
    assert err <= frames.oracle_tol(scene, fname)
