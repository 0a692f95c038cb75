"""Radiance for caller-supplied rays on the GPU (pt_radiance, include/pt_capi.h;
pt_rays.hip k_render_rays): tests/test_rays_host.py's cases through
Renderer.render_rays — the oracle on descriptors with the ray's origin as the
eye (tests/rays_ref.py), the frame through the ray entry, the independence of
the batch, the forced-f64 self-check inside and outside the box and on a plain
scene, the refusals, the launch record and the command line."""
import ctypes as C

import numpy as np
import pytest

import rays_ref
from pathtracerpython_amd import _native, cameras
from pathtracerpython_amd._abi import (PT_FLAG_AA, PT_FLAG_COUNT, PT_FLAG_FORCE_F64, PT_FLAG_KERNEL_TIMES,
                                       PT_FLAG_LENS, PT_FLAG_MEGAKERNEL, PT_FLAG_OUT_F64, PT_FLAG_RR,
                                       PT_FLAG_WALK_COUNT, make_params, make_rays)
from pathtracerpython_amd.render import Renderer

pytestmark = pytest.mark.gpu

TOL, TOL32 = 1e-12, 1e-6


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else a.dtype)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"


@pytest.fixture(scope="module")
def benches(tmp_path_factory, cornell, mesh_golden):
    """name -> (rays_ref.Bench, Renderer with the bench's box, Renderer without)."""
    gpu()
    made = {}

    def get(name):
        if name not in made:
            b = rays_ref.Bench(rays_ref.make_scene(name, tmp_path_factory.mktemp(name), cornell, mesh_golden))
            made[name] = (b, Renderer(b.scene, ray_box=(b.box[:3], b.box[3:])), Renderer(b.scene))
        return made[name]
    yield get
    for _, r, q in made.values():
        r.close()
        q.close()


# 1 ----------------------------------------------------------- the oracle --
@pytest.mark.parametrize("case", rays_ref.PARITY_CASES, ids=rays_ref.case_id)
def test_oracle_parity(benches, case):
    """Every record's mean, S and Q within 1e-12 of the oracle (f32 output:
    1e-6), none excluded; the library's lane count, 1 and 4; with and without
    the box."""
    name, n, spp, bounces, rr_depth, s0 = case
    b, boxed, plain = benches(name)
    esc, light, spec = rays_ref.first_hits(b.pk, b.o, b.d)
    assert esc >= 1 and light >= 1 and spec >= 1
    want = b.samples(n, bounces, rr_depth, s0, spp)
    mean, S, Q = want.sum(axis=0) / spp, want.sum(axis=0), (want ** 2).sum(axis=0)
    kw = dict(spp=spp, bounces=bounces, seed=9, rr=rr_depth is not None,
              rr_depth=3 if rr_depth is None else rr_depth, sample_begin=s0)
    for r in (boxed, plain):
        for lanes in (0, 1, 4):
            if lanes > spp:
                continue
            rgb = r.render_rays(b.o[:n], b.d[:n], b.keys[:n], lanes_per_pixel=lanes, **kw)
            g, gS, gQ = r.render_rays(b.o[:n], b.d[:n], b.keys[:n], lanes_per_pixel=lanes, moments=True, **kw)
            errs = [float(np.abs(x - y).max()) for x, y in ((rgb, mean), (g, mean), (gS, S), (gQ, Q))]
            print(f"{rays_ref.case_id(case)} {'box' if r is boxed else 'plain'} lanes {lanes}: mean {errs[0]:.3e} "
                  f"/ {errs[1]:.3e}, S {errs[2]:.3e}, Q {errs[3]:.3e}")
            assert max(errs) <= TOL
            assert same(g, gS / spp)
    f32 = boxed.render_rays(b.o[:n], b.d[:n], b.keys[:n], out_f64=False, **kw)
    assert f32.dtype == np.float32 and float(np.abs(f32 - mean).max()) <= TOL32


# 2 ------------------------------------------------------ the frame's rays --
@pytest.mark.parametrize("W,H", [(12, 12), (7, 5)])
def test_frame_through_the_ray_entry_is_the_frame(benches, cornell, W, H):
    """render_rays of scene_camera_rays is Renderer.render, bit for bit in f64
    at 1 and 4 lanes per pixel.  (On a scene without a BVH k_render gives the
    frame's top sixteenth of rows 2^3 times the lanes where spp allows it;
    spp = 1 at one lane and spp = 5 at four leave no room for that, so every
    pixel has the fixed lane count.)"""
    _, _, r = benches("cornell")
    o, d, keys = cameras.scene_camera_rays(cornell, W, H)
    for lanes, spp in ((1, 1), (4, 5)):
        frame = r.render(W, H, spp, 3, 9, out_f64=True, lanes_per_pixel=lanes)
        rgb = r.render_rays(o, d, keys, spp=spp, bounces=3, seed=9, lanes_per_pixel=lanes)
        assert same(np.ascontiguousarray(cameras.rays_to_image(rgb, W, H)), frame)
        assert r.last_launch()["lanes_per_pixel"] == lanes


def test_frame_of_a_mesh_scene_through_the_ray_entry(benches):
    """The BVH instantiation against k_render's (megakernel=True), 1 and 4 lanes."""
    b, _, r = benches("mesh")
    o, d, keys = cameras.scene_camera_rays(b.scene, 12, 12)
    for lanes in (1, 4):
        frame = r.render(12, 12, 8, 3, 9, out_f64=True, megakernel=True, lanes_per_pixel=lanes)
        rgb = r.render_rays(o, d, keys, spp=8, bounces=3, seed=9, lanes_per_pixel=lanes)
        assert same(np.ascontiguousarray(cameras.rays_to_image(rgb, 12, 12)), frame)


# 3 ------------------------------------------------------------- the batch --
def test_a_record_does_not_depend_on_its_batch(benches):
    b, r, _ = benches("cornell")
    n = 65
    kw = dict(spp=8, bounces=3, seed=9, moments=True)
    for lanes in (1, 4):
        base = r.render_rays(b.o[:n], b.d[:n], b.keys[:n], lanes_per_pixel=lanes, **kw)
        perm = np.random.default_rng(3).permutation(n)
        sh = r.render_rays(b.o[perm], b.d[perm], b.keys[perm], lanes_per_pixel=lanes, **kw)
        one = r.render_rays(b.o[:20], b.d[:20], b.keys[:20], lanes_per_pixel=lanes, **kw)
        two = r.render_rays(b.o[20:n], b.d[20:n], b.keys[20:n], lanes_per_pixel=lanes, **kw)
        pad = r.render_rays(b.o[:n + 30][::-1], b.d[:n + 30][::-1], b.keys[:n + 30][::-1], lanes_per_pixel=lanes, **kw)
        for x, y, z, w, v in zip(base, sh, one, two, pad):
            assert same(x[perm], y)
            assert same(x, np.concatenate([z, w]))
            assert same(x, np.ascontiguousarray(v[::-1][:n]))
    twin = r.render_rays(b.o[[4, 4, 9]], b.d[[4, 4, 9]], b.keys[[4, 4, 9]], **kw)
    assert all(same(x[0], x[1]) for x in twin)
    fixed = r.render_rays(b.o[:n], b.d[:n], b.keys[:n], lanes_per_pixel=1, **kw)[0]
    auto = r.render_rays(b.o[:n], b.d[:n], b.keys[:n], lanes_per_pixel=0, **kw)[0]
    assert float(np.abs(fixed - auto).max()) <= TOL


# 4 ---------------------------------------------------- f64 and the frames --
@pytest.mark.parametrize("name", ["cornell", "mesh"])
def test_forced_f64_is_the_hybrid_result_bit_for_bit(benches, name):
    """Origins inside the box, outside it (rays_ref.OFF_AXIS[1]), and every
    origin on a scene made without a box."""
    b, boxed, plain = benches(name)
    n = 64
    assert b.outside[:n].any() and not b.outside[:n].all()
    for r in (boxed, plain):
        for lanes in (1, 4):
            kw = dict(spp=5, bounces=3, seed=9, moments=True, lanes_per_pixel=lanes)
            hyb = r.render_rays(b.o[:n], b.d[:n], b.keys[:n], **kw)
            f64 = r.render_rays(b.o[:n], b.d[:n], b.keys[:n], force_f64=True, **kw)
            assert all(same(x, y) for x, y in zip(hyb, f64))


# 5 ------------------------------------------------- refusals and plumbing --
def test_refusals_and_the_empty_batch(benches):
    b, r, _ = benches("cornell")
    lib = _native.lib()
    rec = make_rays(b.o[:4], b.d[:4], b.keys[:4])
    out = np.full((4, 3), -1.0)
    S, Q = np.full((4, 3), -1.0), np.full((4, 3), -1.0)

    def call(p, rays=rec, n=4, rgb=out, s=None, q=None):
        return lib.pt_radiance(r._h, C.c_void_p(rays.ctypes.data) if rays is not None else None, n, C.byref(p),
                               C.c_void_p(rgb.ctypes.data) if rgb is not None else None,
                               C.c_void_p(s.ctypes.data) if s is not None else None,
                               C.c_void_p(q.ctypes.data) if q is not None else None)
    ok = make_params(1, 1, 2, 2, 9, PT_FLAG_OUT_F64)
    for flag in (PT_FLAG_AA, PT_FLAG_LENS, PT_FLAG_COUNT, PT_FLAG_WALK_COUNT, PT_FLAG_KERNEL_TIMES,
                 PT_FLAG_MEGAKERNEL, 1 << 20):
        assert call(make_params(1, 1, 2, 2, 9, PT_FLAG_OUT_F64 | flag)) == -1, hex(flag)
        assert "flag" in _native.last_error()
    assert (out == -1.0).all()
    bad = rec.copy()
    bad["reserved"][2] = 1
    assert call(ok, rays=bad) == -1 and "reserved" in _native.last_error()
    assert call(ok, rays=None) == -1
    assert call(ok, rgb=None) == -1
    assert call(ok, n=1 << 30) == -1 and call(ok, n=-1) == -1
    assert call(ok, s=S) == -1 and call(ok, q=Q) == -1        # S and Q: both or neither
    assert call(make_params(1, 1, 0, 2, 9)) == -1             # spp
    assert call(make_params(1, 1, 2, 2, 9, lanes_per_pixel=4)) == -1     # > spp
    assert call(make_params(1, 1, 8, 2, 9, lanes_per_pixel=3)) == -1
    assert (out == -1.0).all() and (S == -1.0).all()
    # n_rays = 0 succeeds and writes nothing, with or without arrays
    assert call(ok, n=0) == 0 and call(ok, rays=None, n=0, rgb=None) == 0
    assert (out == -1.0).all()
    empty = r.render_rays(np.zeros((0, 3)), np.zeros((0, 3)), spp=2, bounces=2)
    assert empty.shape == (0, 3)
    # allowed: RR, forced f64, f64 output
    assert call(make_params(1, 1, 2, 2, 9, PT_FLAG_OUT_F64 | PT_FLAG_RR | PT_FLAG_FORCE_F64), s=S, q=Q) == 0
    assert (out >= 0.0).all() and same(out, S / 2)
    # keys=None are 0..n-1; the scene's size plays no part
    a = r.render_rays(b.o[:5], b.d[:5], spp=2, bounces=2, seed=9)
    assert same(a, r.render_rays(b.o[:5], b.d[:5], np.arange(5), spp=2, bounces=2, seed=9))
    with pytest.raises(ValueError):
        Renderer(b.scene, lens=(0.1, -20.0), ray_box=([0, 0, 0], [1, 1, 1]))
    with pytest.raises(_native.NativeError):
        Renderer(b.scene, ray_box=([0, 0, 2], [1, 1, 1]))


def test_launch_record_and_kernel_time(benches):
    b, r, _ = benches("cornell")
    r.render_rays(b.o[:65], b.d[:65], b.keys[:65], spp=8, bounces=2, seed=9, lanes_per_pixel=4, rr=True)
    info = r.last_launch()
    assert info["path"] == 1 and info["steps"] == 1 and info["lanes_per_pixel"] == 4
    assert info["flags"] == PT_FLAG_RR | PT_FLAG_OUT_F64
    assert r.last_kernel_ms() > 0.0
    r.render_rays(b.o[:65], b.d[:65], b.keys[:65], spp=8, bounces=2, seed=9)
    assert r.last_launch()["lanes_per_pixel"] in (1, 2, 4, 8)
    r.render(8, 8, 2, 2, 9)   # a frame's launch replaces the record
    assert r.last_launch()["flags"] == 0


def test_device_entry_on_torch_tensors(benches):
    """pt_radiance_device on caller-owned device memory, ordered on a stream."""
    import torch
    b, r, _ = benches("cornell")
    n = 65
    rec = make_rays(b.o[:n], b.d[:n], b.keys[:n])
    rays = torch.from_numpy(np.frombuffer(rec.tobytes(), dtype=np.uint8).copy()).cuda()
    rgb = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    S, Q = torch.zeros_like(rgb), torch.zeros_like(rgb)
    p = make_params(1, 1, 8, 3, 9, PT_FLAG_OUT_F64, lanes_per_pixel=4)
    st = torch.cuda.current_stream().cuda_stream
    _native.check(_native.lib().pt_radiance_device(r._h, C.c_void_p(rays.data_ptr()), n, C.byref(p),
                                                   C.c_void_p(rgb.data_ptr()), C.c_void_p(S.data_ptr()),
                                                   C.c_void_p(Q.data_ptr()), C.c_void_p(st)), "pt_radiance_device")
    torch.cuda.synchronize()
    want = r.render_rays(b.o[:n], b.d[:n], b.keys[:n], spp=8, bounces=3, seed=9, lanes_per_pixel=4, moments=True)
    assert same(rgb.cpu().numpy(), want[0]) and same(S.cpu().numpy(), want[1]) and same(Q.cpu().numpy(), want[2])


# 6 ------------------------------------------------------- the command line --
def test_cli_look_at_writes_an_image(cornell, tmp_path, capsys):
    gpu()
    from PIL import Image
    from pathtracerpython_amd import main as cli
    from conftest import CORNELL
    out, raw = str(tmp_path / "look.png"), str(tmp_path / "look.npy")
    argv = [CORNELL, "--look-at", "2.5", "1.5", "4", "0", "0", "-24", "--fov", "30", "-r", "4", "-b", "2",
            "--seed", "9", "--size", "10", "8", "--out", out, "--save-raw", raw]
    fb = cli.main(argv)
    assert fb.shape == (8, 10, 3) and fb.dtype == np.float64 and same(np.load(raw), fb)
    assert Image.open(out).size == (10, 8)
    o, d, keys = cameras.look_at_rays((2.5, 1.5, 4.0), (0.0, 0.0, -24.0), (0.0, 1.0, 0.0), 30.0, 10, 8)
    with Renderer(cornell, ray_box=((2.5, 1.5, 4.0), (2.5, 1.5, 4.0))) as r:
        want = r.render_rays(o, d, keys, spp=4, bounces=2, seed=9)
    assert same(fb, np.ascontiguousarray(cameras.rays_to_image(want, 10, 8)))
    assert fb.max() > 0.0 and "look-at" in capsys.readouterr().out
    with pytest.raises(SystemExit, match="--look-at"):
        cli.main(argv + ["--aa"])
