"""The render loop's unit forms (pt_path.h quad_m, closest_unit_m, fused_unit)
on the GPU: the three unit kinds of quad_m, the closest ray's unit-level
ambiguity flag and the rare block's rebuild of the per-member bits.  Every
case asserts hybrid == forced f64 bit for bit and the oracle to 1e-12; the
frames are small, the shapes are the ones where the code takes another path:
  * all three unit kinds (single, parallelogram, skew pair) in one wave's
    unit list (conftest.quad_scene);
  * 1 bounce: no lane traces a next ray, so the closest part and its rebuild
    are skipped for the whole wave; 2 and 4 bounces: they run;
  * 64 spp: 64 lanes of a pixel in one wave (the lane cap), 4 spp: 16 pixels;
  * Russian roulette: tracing and non-tracing lanes share a wave;
  * a BVH scene: the wavefront shade step shares the code with the single
    kernel and must give its frame."""
import numpy as np
import pytest

from conftest import quad_scene
from oracle import oracle
from pathtracerpython_amd._abi import PT_FLAG_RR
from pathtracerpython_amd.pack import pack_scene
from pathtracerpython_amd.render import Renderer, to_list_order

pytestmark = pytest.mark.gpu

TOL = 1e-12


@pytest.fixture(scope="module")
def R(cornell):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    r = Renderer(cornell)
    yield r
    r.close()


def check(r, pk, W, H, spp, B, seed, rr=False):
    fb = r.render(W, H, spp, B, seed, rr=rr, out_f64=True)
    f64 = r.render(W, H, spp, B, seed, rr=rr, out_f64=True, force_f64=True)
    ref, _ = oracle.render(pk, W, H, spp, B, seed, flags=PT_FLAG_RR if rr else 0)
    err = float(np.abs(to_list_order(fb) - ref).max())
    print("unit forms %dx%d spp %d B %d rr %d: L-inf vs oracle %.3e" % (W, H, spp, B, rr, err))
    assert np.array_equal(fb, f64)
    assert err <= TOL
    return fb


@pytest.mark.parametrize("seed", [3, 8])
def test_quad_scene_all_unit_kinds(tmp_path, seed):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    sc = quad_scene(tmp_path, seed)
    pk = pack_scene(sc)
    with Renderer(sc, packed=pk) as r:
        check(r, pk, 28, 28, 3, 5, seed)


@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("spp", [4, 64])
def test_cornell_bounces_and_lanes(R, packed, spp, B):
    check(R, packed, 16, 16, spp, B, 9)


def test_cornell_russian_roulette(R, packed):
    check(R, packed, 16, 16, 4, 8, 5, rr=True)


def test_k5_wavefront_equals_megakernel(tmp_path):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from pathtracerpython_amd import scene_reader
    from pathtracerpython_amd.synth import write_k5_scene
    scene_reader.VERBOSE = False
    sc = scene_reader.Scene(write_k5_scene(str(tmp_path), n_tris=3000, seed=0, size=16))
    pk = pack_scene(sc)
    with Renderer(sc, packed=pk) as r:
        wf = check(r, pk, 16, 16, 2, 4, 9)
        mk = r.render(16, 16, 2, 4, 9, out_f64=True, megakernel=True)
    assert np.array_equal(wf, mk)
