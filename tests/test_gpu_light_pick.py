"""The light pick's counting forms on the GPU (pt_core.h pick_light,
light_tab; tests/test_light_pick_host.py proves them against the loop for
every uniform on the host): the Cornell light (two triangles: the pair form,
read ahead of the Philox rounds in the render loop) and a five-triangle fan
light of unequal areas (the general count) through k_render at 1 and 16 lanes
per pixel, its forced-f64 instantiation and the batched compute_color entry
with pick uniforms at 0, 1 - 2^-24, a table boundary and outside [0, 1), all
against the oracle at 1e-12; and the wavefront kernels, whose rare f64 blocks
draw the light point again (light_redraw), bit for bit the single kernel on
the 80-triangle mesh scene of tests/material_scenes.py."""
import os
import shutil

import numpy as np
import pytest

import material_scenes as ms
from conftest import CORNELL
from oracle import oracle
from pathtracerpython_amd.pack import pack_scene
from pathtracerpython_amd.render import Renderer, to_list_order

pytestmark = pytest.mark.gpu

TOL = 1e-12
W, H = 24, 16
# the first uniform of a light sample picks the triangle: the ends of the
# render loop's range, a boundary of the Cornell table (two equal areas), and
# values only a caller of the batched entry can pass
PICKS = [0.0, 1.0 - 2.0 ** -24, 0.5, 0.5 - 2.0 ** -24, 1.0, 1.5, -0.5, float("nan")]


def fan_light_scene(tmp_path):
    """The Cornell room under a five-triangle fan light in the ceiling light's
    plane, every triangle of another area."""
    src = os.path.dirname(CORNELL)
    for f in os.listdir(src):
        shutil.copy(os.path.join(src, f), tmp_path / f)
    rim = [(-0.91, -23.324), (-0.91, -26.488), (0.2, -26.9), (0.91, -25.0), (0.6, -23.1)]
    lines = ["v 0.1 3.836 -24.6"] + ["v %.4f 3.836 %.4f" % p for p in rim]
    lines += ["f 1 %d %d" % (2 + i, 2 + (i + 1) % 5) for i in range(5)]
    (tmp_path / "luzcornell.obj").write_text("\n".join(lines) + "\n")
    from pathtracerpython_amd import scene_reader
    scene_reader.VERBOSE = False
    return scene_reader.Scene(str(tmp_path / "cornellroom.sdl"))


@pytest.fixture(scope="module")
def lights(cornell, packed, tmp_path_factory):
    """{name: (Renderer, packed scene)}: the Cornell light and the fan light."""
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    fan = fan_light_scene(tmp_path_factory.mktemp("fan_light"))
    pk = pack_scene(fan)
    areas = np.asarray(pk.tri_area)[pk.desc.n_obj_tri:]
    assert len(areas) == 5 and len(set(np.round(areas, 6))) == 5 and (areas > 0).all()
    out = {"cornell": (Renderer(cornell), packed), "fan": (Renderer(fan, packed=pk), pk)}
    yield out
    for r, _ in out.values():
        r.close()


@pytest.mark.parametrize("lanes,spp,B", [(1, 3, 4), (16, 16, 4), (1, 2, 1)])
@pytest.mark.parametrize("name", ["cornell", "fan"])
def test_render_equals_f64_and_the_oracle(lights, name, lanes, spp, B):
    r, pk = lights[name]
    fb = r.render(W, H, spp, B, 7, out_f64=True, lanes_per_pixel=lanes)
    assert np.array_equal(fb, r.render(W, H, spp, B, 7, out_f64=True, lanes_per_pixel=lanes,
                                       force_f64=True))
    ref, _ = oracle.render(pk, W, H, spp, B, 7)
    err = np.abs(to_list_order(fb) - ref).max()
    print(f"{name} lanes {lanes} spp {spp} bounces {B}: {err:.3e}")
    assert err <= TOL


@pytest.mark.parametrize("name", ["cornell", "fan"])
def test_compute_color_with_edge_pick_uniforms(lights, kat, name):
    """pt_compute_color at the golden file's shading points with the pick
    uniform of every light sample replaced by the values of PICKS (the oracle
    sends a pick outside every interval to the light's first triangle, as the
    lane code does)."""
    r, pk = lights[name]
    obj, P, n = kat["cc_obj"], kat["cc_p"], kat["cc_n"]
    u = np.array(kat["cc_u"], dtype=np.float64, copy=True)
    assert u.shape[1] == 12 and len(u) >= 3
    reps = -(-len(PICKS) * 3 // len(u))          # every value in every slot
    obj, P, n, u = (np.concatenate([a] * reps) for a in (obj, P, n, u))
    for i in range(len(u)):
        for k in range(3):
            u[i, 4 * k] = PICKS[(i + 3 * k) % len(PICKS)]
    want = oracle.compute_color(pk, obj, P, n, u)
    got = r.compute_color(obj, P, n, u)
    assert np.isfinite(want).all()
    err = np.abs(got - want).max()
    print(f"{name}: {len(u)} points, {err:.3e}")
    assert err <= TOL


def test_wavefront_equals_the_single_kernel_on_the_mesh_scene(tmp_path):
    """80 triangles behind the BVH (material_scenes 'mesh'): the wavefront
    shade step and shadow walks go through pick_light / light_redraw as the
    single kernel goes through shadow_setup_k — same bits, NaN samples
    included, and the oracle's frame."""
    sc = ms.material_scene(tmp_path, "mesh")
    pk = pack_scene(sc)
    Wm, Hm, B, seed = ms.FRAME
    with Renderer(sc, packed=pk) as r:
        wf = r.render(Wm, Hm, 4, B, seed, out_f64=True)
        mk = r.render(Wm, Hm, 4, B, seed, out_f64=True, megakernel=True)
    assert ms.same_bits(wf, mk)
    ref, _ = oracle.render(pk, Wm, Hm, 4, B, seed)
    from pathtracerpython_amd.render import from_list_order
    ms.compare(wf, from_list_order(ref, Wm, Hm), TOL, "mesh wavefront")
