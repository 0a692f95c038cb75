"""The grazing scenes (tests/grazing.py) on the GPU: thousands of deterministic
rays within 1e-9 .. 1e-3 of every threshold of the f32 filter, on both sides,
through the render kernels (K2's uniform units, the BVH walks' leaf units)
and the batched entry points.  On the host build (tests/test_grazing_host.py,
which proves the scenes sound first) these frames fail when the candidate
fold of shadow_unit_m loses its `del` or its |n.d| > qhi term, or ray_plane_e
its qhi term; the scenes cannot see a halved `del` or kTzLo for kTzHi (the
bounds' slack is orders larger), nor closest_unit_m, whose rays are random
bounces.  Building the scenes here re-asserts the builder's conditions."""
import numpy as np
import pytest

import grazing
from oracle import oracle
from pathtracerpython_amd.pack import pack_scene
from pathtracerpython_amd.render import Renderer, to_list_order

pytestmark = pytest.mark.gpu

TOL = 1e-12
SHAPES = [(32, 32, 8, 1), (32, 32, 64, 1), (24, 24, 6, 3)]
SEED = 5


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """{W: {variant: (scene, report, packed)}}"""
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    out = {}
    for W in (24, 32):
        s = grazing.grazing_scenes(tmp_path_factory.mktemp("graze%d" % W), W)
        out[W] = {v: (sc, rep, pack_scene(sc)) for v, (sc, rep) in s.items()}
    return out


@pytest.mark.parametrize("variant", grazing.VARIANTS)
@pytest.mark.parametrize("W,H,spp,B", SHAPES)
def test_grazing_frame(scenes, variant, W, H, spp, B):
    """hybrid == forced f64 bit for bit; the oracle over the whole frame, f64
    <= 1e-12 and f32 <= 1e-6; the reference's work counters."""
    sc, rep, pk = scenes[W][variant]
    with Renderer(sc, packed=pk) as r:
        fb = r.render(W, H, spp, B, SEED, out_f64=True)
        f64 = r.render(W, H, spp, B, SEED, out_f64=True, force_f64=True)
        f32 = r.render(W, H, spp, B, SEED)
        _, st = r.render(W, H, spp, B, SEED, out_f64=True, stats=True)
    ref, ost = oracle.render(pk, W, H, spp, B, SEED)
    assert np.array_equal(fb, f64)
    assert np.abs(to_list_order(fb) - ref).max() <= TOL
    assert f32.dtype == np.float32
    assert np.abs(to_list_order(f32) - ref).max() <= 1e-6
    for k in ost:
        if k not in ("f64_fallbacks", "f64_rescans"):
            assert st[k] == ost[k], k


@pytest.mark.parametrize("W,H,spp,B", SHAPES)
def test_grazing_bvh_wavefront_megakernel_band(scenes, W, H, spp, B):
    """bvh variant: wavefront kernels == single kernel bit for bit; a
    contiguous band equals those rows of the frame."""
    sc, rep, pk = scenes[W]["bvh"]
    with Renderer(sc, packed=pk) as r:
        wf = r.render(W, H, spp, B, SEED, out_f64=True)
        mk = r.render(W, H, spp, B, SEED, out_f64=True, megakernel=True)
        band = r.render(W, H, spp, B, SEED, out_f64=True, row_begin=5, row_end=H - 3)
    assert np.array_equal(wf, mk)
    assert np.array_equal(band, wf[3:H - 5])


@pytest.mark.parametrize("W,H,spp,B", SHAPES)
def test_grazing_uniform_interleaved_bands(scenes, W, H, spp, B):
    """uniform variant: a 4-way interleaved band split at a fixed
    lanes_per_pixel assembles to the whole frame bit for bit (a band launch
    would choose more lanes per pixel: the grazing rows must not depend on it)."""
    from pathtracerpython_amd.distributed import assemble, max_band_rows
    sc, rep, pk = scenes[W]["uniform"]
    lanes = min(8, spp)
    lanes = 1 << (lanes.bit_length() - 1)
    world = 4
    with Renderer(sc, packed=pk) as r:
        full = r.render(W, H, spp, B, SEED, out_f64=True, lanes_per_pixel=lanes)
        tiles = []
        for ph in range(world):
            t = r.render(W, H, spp, B, SEED, out_f64=True, row_step=world, row_phase=ph,
                         lanes_per_pixel=lanes)
            pad = np.zeros((max_band_rows(H, world), W, 3))
            pad[:t.shape[0]] = t
            tiles.append(pad)
    assert np.array_equal(assemble(tiles, H), full)
    ref, _ = oracle.render(pk, W, H, spp, B, SEED)
    assert np.abs(to_list_order(full) - ref).max() <= TOL


@pytest.mark.parametrize("variant", grazing.VARIANTS)
@pytest.mark.parametrize("W", [24, 32])
def test_grazing_batched_apis(scenes, variant, W):
    """closest_unit and fused_unit<MARGIN=false> on the grazing rays:
    pt_intersect_objects with the frame's primary rays, pt_compute_color at
    their hit points with all three light points at corners of the light."""
    sc, rep, pk = scenes[W][variant]
    rays = grazing.primary_rays(W, W)
    otri, oP = oracle.intersect_objects(pk, rays)
    assert np.array_equal(otri, rep["hit_tri"])
    on = np.nonzero((otri >= 0) & (otri < pk.n_obj_tri))[0]
    u = np.tile(np.array([0.25, 1.0, 0.0, 0.0, 0.75, 0.0, 1.0, 0.0, 0.25, 0.0, 0.0, 1.0]),
                (len(on), 1))
    obj, nrm = pk.tri_obj[otri[on]], pk.tri_n[otri[on]]
    want = oracle.compute_color(pk, obj, oP[on], nrm, u)
    with Renderer(sc, packed=pk) as r:
        tri, P = r.intersect_objects(rays)
        got = r.compute_color(obj, oP[on], nrm, u)
    assert np.array_equal(tri, otri)
    hit = otri >= 0
    assert np.abs(P[hit] - oP[hit]).max() <= 1e-9
    assert np.abs(got - want).max() <= TOL
    # the shadow verdicts matter: lit and shadowed points both occur
    amb = pk.mat[obj, :3] * pk.mat[obj, 3:4] * pk.ambient
    lit = np.abs(want - amb).max(axis=1) > 1e-6
    assert lit.any() and not lit.all()
