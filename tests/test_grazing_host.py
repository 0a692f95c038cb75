"""The grazing scenes (tests/grazing.py) through the host build of the kernel's
lane code: thousands of deterministic rays within 1e-9 .. 1e-3 of every
threshold of the f32 filter (triangle edges, |n.d| > 1e-5, sqd > 1e-5,
sqd < |L - P|^2), on both sides.  A wrong certain verdict there changes a
pixel (the builder asserts it for the shadow-ray units of the uniform
variants), so hybrid == forced f64 and the oracle parity catch a filter term
that is missing: without `del` or qhi in shadow_unit_m's fold, or qhi in
ray_plane_e, the renders below fail.  They do not measure the bounds' slack
(a halved `del` passes).  The scenes are proven sound here before
tests/test_gpu_grazing.py takes them to the device path."""
import ctypes as C

import numpy as np
import pytest

import grazing
from conftest import hc_render
from oracle import oracle
from pathtracerpython_amd._abi import make_params
from pathtracerpython_amd.pack import pack_scene
from pathtracerpython_amd.render import to_list_order

SHAPES = [(32, 32, 8, 1), (32, 32, 64, 1), (24, 24, 6, 3)]
SEED = 5


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """{W: {variant: (scene, report, packed)}}; building them asserts the
    builder's conditions on the report."""
    out = {}
    for W in (24, 32):
        s = grazing.grazing_scenes(tmp_path_factory.mktemp("graze%d" % W), W)
        out[W] = {v: (sc, rep, pack_scene(sc)) for v, (sc, rep) in s.items()}
    return out


def test_builder_report(scenes):
    for W, s in scenes.items():
        for v, (sc, rep, pk) in s.items():
            print("grazing %s %dx%d: %d triangles; pixels one shadow verdict decides: %s; "
                  "per decade below/above the boundary: %s"
                  % (v, W, W, rep["n_tris"], rep["decisive"], grazing.format_counts(rep["counts"])))
            if v != "bvh":
                assert rep["decisive"]["E"] >= 20 and rep["decisive"]["P"] >= 6 and \
                    rep["decisive"]["Z"] >= 12
            assert (rep["n_tris"] >= 64) == (v == "bvh")       # kBvhMinTris
            assert (rep["graze"][0] == 0) == (v == "first")
            grazing.check_counts(rep["counts"], "E", 20)
        total = grazing.add_counts([s[v][1] for v in grazing.VARIANTS])
        for c in "PZR":
            grazing.check_counts(total, c, 10)


@pytest.mark.parametrize("variant", grazing.VARIANTS)
def test_filter_selftest(hostcheck, scenes, variant):
    pk = scenes[32][variant][2]
    out = (C.c_int64 * 5)()
    assert hostcheck.hc_filter_selftest(C.byref(pk.desc), C.c_int64(1500), C.c_uint64(SEED), out) == 0
    wrong, amb, tests, cand, mdiff = list(out)
    assert wrong == 0 and mdiff == 0 and cand > 0


@pytest.mark.parametrize("variant", grazing.VARIANTS)
@pytest.mark.parametrize("W,H,spp,B", SHAPES)
def test_hybrid_equals_f64_and_oracle(hostcheck, scenes, variant, W, H, spp, B):
    """The render loop's own lane code (count=False): hybrid == forced f64
    bit for bit, and the oracle to rounding."""
    pk = scenes[W][variant][2]
    p = make_params(W, H, spp, B, SEED)
    a, _ = hc_render(hostcheck, pk, p, False, count=False)
    b, _ = hc_render(hostcheck, pk, p, True, count=False)
    assert np.array_equal(a, b)
    ref, _ = oracle.render(pk, W, H, spp, B, SEED)
    assert np.abs(to_list_order(a) - ref).max() <= 1e-12


@pytest.mark.parametrize("W,H,spp,B", SHAPES)
def test_wavefront_equals_single_kernel(hostcheck, scenes, W, H, spp, B):
    pk = scenes[W]["bvh"][2]
    info = (C.c_int32 * 6)()
    assert hostcheck.hc_bvh_info(C.byref(pk.desc), info) == 0 and info[0] > 1 and info[2] > 0
    p = make_params(W, H, spp, B, SEED)
    ref, _ = hc_render(hostcheck, pk, p, False, count=False)
    out = np.zeros((H, W, 3))
    assert hostcheck.hc_render_wavefront(C.byref(pk.desc), C.byref(p),
                                         out.ctypes.data_as(C.POINTER(C.c_double)), None,
                                         None) == 0
    assert np.array_equal(out, ref)


@pytest.mark.parametrize("variant", grazing.VARIANTS)
def test_reaches_the_ambiguous_band(hostcheck, scenes, packed, variant):
    """A diagnostic that the deterministic rays reach the filter's ambiguous
    band: more f64 fallbacks than plain Cornell at the same frame."""
    W, H, spp, B = 32, 32, 8, 1
    pk = scenes[W][variant][2]
    p = make_params(W, H, spp, B, SEED)
    a, st = hc_render(hostcheck, pk, p, False, count=True)
    b, st64 = hc_render(hostcheck, pk, p, True, count=True)
    assert np.array_equal(a, b)
    ref, ost = oracle.render(pk, W, H, spp, B, SEED)
    assert np.abs(to_list_order(a) - ref).max() <= 1e-12
    for k in ("closest_tests", "shadow_tests", "ray_bounces", "shading_points", "light_hits",
              "escapes"):
        assert st[k] == ost[k] == st64[k], k
    _, plain = hc_render(hostcheck, packed, p, False, count=True)
    print("f64_fallbacks %s %dx%d spp %d B %d: grazing %d, plain Cornell %d"
          % (variant, W, H, spp, B, st["f64_fallbacks"], plain["f64_fallbacks"]))
    assert st["f64_fallbacks"] > plain["f64_fallbacks"]
