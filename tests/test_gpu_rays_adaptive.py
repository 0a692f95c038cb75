"""Ray accumulators on the GPU (pt_accum_create_rays, include/pt_capi.h;
pt_rays_list.hip k_render_rays_list, k_features_rays): adaptive runs over ray
records against the numpy simulation of the stop rule on the oracle's
per-sample colours (tests/rays_adaptive_ref.py, tests/adaptive_sim.py), the
launch shapes, the equivalence with a frame accumulator on the frame's own
rays, the records' features against the oracle, forced f64, Russian roulette,
the denoiser against its numpy restatement, resumable runs, the refusals and
the command line.  Host-side cases: tests/test_rays_adaptive_host.py."""
import ctypes as C

import numpy as np
import pytest

import adaptive_sim
import rays_adaptive_ref as ref
from denoise_ref import denoise_numpy, moments_numpy, same_bits
from oracle import oracle
from pathtracerpython_amd import _native, cameras
from pathtracerpython_amd._abi import (PATH_NAMES, PT_FLAG_AA, PT_FLAG_COUNT, PT_FLAG_FORCE_F64, PT_FLAG_KERNEL_TIMES,
                                       PT_FLAG_LENS, PT_FLAG_MEGAKERNEL, PT_FLAG_OUT_F64, PT_FLAG_RAYS_SINGLE,
                                       PT_FLAG_RR, PT_FLAG_WALK_COUNT, PT_PATH_SINGLE, make_adapt, make_band,
                                       make_params, make_rays)
from pathtracerpython_amd.adaptive import Accumulator, RayAccumulator, run_passes
from pathtracerpython_amd.render import Renderer

pytestmark = pytest.mark.gpu

TOL = 1e-12   # the project's f64 bar, relative to max(1, |value|)


def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def rel(got, want):
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


@pytest.fixture(scope="module")
def envs(cornell, mesh_golden):
    """name -> (rays_adaptive_ref.Batch, Renderer made with the batch's box)."""
    gpu()
    made = {}

    def get(name):
        if name not in made:
            b = ref.batch_of(name, cornell if name == "cornell" else mesh_golden[0])
            made[name] = (b, Renderer(b.scene, ray_box=(b.box[:3], b.box[3:])))
        return made[name]
    yield get
    for _, r in made.values():
        r.close()


def rule_params(rule, n, height=1, flags=0, rr_depth=3):
    tol, floor, lo, hi, step = ref.RULES[rule] if isinstance(rule, str) else rule
    return (make_params(n // height, height, hi, ref.BOUNCES, ref.SEED, flags, rr_depth),
            make_adapt(tol, hi, lo, step, floor))


def flat(d):
    """An accumulator's (1, n, ...) arrays as (n, ...)."""
    return {k: (v if k == "list" else v.reshape(v.shape[1:])) for k, v in d.items()}


def band_of(L, height=1):
    return dict(band=make_band(height, lanes_per_pixel=L)) if L else {}


def full_run(r, o, d, keys, rule, L=0, flags=0, rr_depth=3, shape=None):
    """(S, Q, n, passes) of a whole run on a flat ray accumulator."""
    H = 1 if shape is None else shape[0]
    p, adapt = rule_params(rule, len(o), H, flags, rr_depth)
    with RayAccumulator(r, o, d, keys, shape, **band_of(L, H)) as acc:
        passes = run_passes(acc, p, adapt)
        m = acc.read(S=True, Q=True, n=True)
    m = m if shape is not None else flat(m)
    return m["S"], m["Q"], m["n"], passes


# 1 ------------------------------------------------------- the simulation --
@pytest.mark.parametrize("rule", list(ref.RULES))
@pytest.mark.parametrize("name", ["cornell", "mesh"])
def test_run_is_the_simulation(envs, name, rule):
    """Cornell (no BVH) and the mesh golden (the BVH instantiation) under both
    rules, the library's own lane count: after every pass n and (n_active,
    pass_samples) are the simulation's; err and the list are numpy's on the
    device's own S, Q, n bit for bit; at the end S and Q are within 1e-12 of
    the oracle's samples summed up to the counts, and resolve is S / n."""
    import torch
    b, r = envs(name)
    sim = b.check_preconditions(rule)
    traj = ref.trajectory(b.samples(), rule)
    assert [(a, k) for a, k, _ in traj] == sim["passes"] and np.array_equal(traj[-1][2], sim["n"])
    tol, floor, lo, hi, step = ref.RULES[rule]
    p, adapt = rule_params(rule, b.n)
    with RayAccumulator(r, b.o, b.d, b.keys) as acc:
        assert (acc.height, acc.width) == (1, b.n)
        for i in range(len(traj) + 1):
            got = acc.select(adapt)
            m = flat(acc.read(S=True, Q=True, n=True, err=True, active=True))
            err = adaptive_sim.err_numpy(m["S"], m["Q"], m["n"], floor)
            assert same(m["err"], err)
            act = adaptive_sim.active_numpy(m["n"], err, tol, lo, hi)
            assert np.array_equal(m["list"], np.nonzero(act)[0].astype(np.uint32))
            if i == len(traj):
                assert got == (0, 0)
                break
            assert got == traj[i][:2], f"pass {i + 1}"
            acc.render(p, adapt)
            info = r.last_launch()
            assert info["path"] == PT_PATH_SINGLE and info["steps"] == 1 and info["flags"] == 0
            assert np.array_equal(flat(acc.read(n=True))["n"], traj[i][2]), f"after pass {i + 1}"
        wS, wQ = adaptive_sim.moments_upto(b.samples(), m["n"])
        print(f"{name} {rule}: {len(traj)} passes, |S| {rel(m['S'], wS):.3e}, |Q| {rel(m['Q'], wQ):.3e} "
              f"(relative to max(1, |value|))")
        assert rel(m["S"], wS) <= TOL and rel(m["Q"], wQ) <= TOL
        out = torch.empty((b.n, 3), dtype=torch.float64, device="cuda")
        acc.resolve_device(out.data_ptr(), True, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert same(out.cpu().numpy(), m["S"] / m["n"][:, None].astype(np.float64))


# 2 ---------------------------------------------------------- launch shapes --
@pytest.mark.parametrize("L", [1, 2, 8, 64])
def test_lanes_per_record(envs, L):
    """A fixed lane count on rule (4, 32, 4): split = min(L, 4) in every pass
    (kmin = 4), the simulation's counts and the oracle's moments."""
    b, r = envs("cornell")
    sim = b.simulate("r4-32-4")
    S, Q, n, passes = full_run(r, b.o, b.d, b.keys, "r4-32-4", L)
    assert r.last_launch()["lanes_per_pixel"] == min(L, 4)
    assert passes == sim["passes"] and np.array_equal(n, sim["n"])
    wS, wQ = adaptive_sim.moments_upto(b.samples(), n)
    assert rel(S, wS) <= TOL and rel(Q, wQ) <= TOL


@pytest.mark.parametrize("name", ["cornell", "mesh"])
@pytest.mark.parametrize("L,spp", [(8, 8), (64, 64), (0, 64)])
def test_wide_splits(envs, name, L, spp):
    """min = max = step = spp on 65 records: one pass at 8 and at 64 lanes per
    record (fixed, and the library's own choice for a launch this small)."""
    b, r = envs(name)
    s = b.samples(None, 64)[:spp, :65]
    S, Q, n, passes = full_run(r, b.o[:65], b.d[:65], b.keys[:65], (0.0, 0.01, spp, spp, spp), L)
    assert passes == [(65, 65 * spp)] and (n == spp).all()
    assert r.last_launch()["lanes_per_pixel"] == spp
    assert rel(S, s.sum(axis=0)) <= TOL and rel(Q, (s ** 2).sum(axis=0)) <= TOL


def test_one_record(envs):
    b, r = envs("cornell")
    sim = b.simulate("r4-32-4")
    i = int(np.argmax((sim["n"] > 4) & (sim["n"] < 32)))   # a record that stops on its error
    S, Q, n, passes = full_run(r, b.o[i:i + 1], b.d[i:i + 1], b.keys[i:i + 1], "r4-32-4")
    assert n.shape == (1,) and n[0] == sim["n"][i] and 4 < n[0] < 32
    assert len(passes) == n[0] // 4 and all(ps == (1, 4) for ps in passes)
    assert rel(S[0], sim["S"][i]) <= TOL and rel(Q[0], sim["Q"][i]) <= TOL


@pytest.mark.parametrize("m", [63, 64, 65])
def test_list_lengths(envs, m):
    """A list of 63, 64 or 65 entries: every other record is written at its
    budget, so one pass takes the first m records from 0 to 4 samples and
    touches nothing else."""
    b, r = envs("mesh")
    p, adapt = rule_params("r4-32-4", b.n)
    n0 = np.full((1, b.n), 32, dtype=np.uint32)
    n0[0, :m] = 0
    with RayAccumulator(r, b.o, b.d, b.keys) as acc:
        acc.write(np.zeros((1, b.n, 3)), np.zeros((1, b.n, 3)), n0)
        assert acc.select(adapt) == (m, 4 * m)
        acc.render(p, adapt)
        d = flat(acc.read(S=True, Q=True, n=True))
    s = b.samples()[:4, :m]
    assert (d["n"][:m] == 4).all() and (d["n"][m:] == 32).all()
    assert not d["S"][m:].any() and not d["Q"][m:].any()
    assert rel(d["S"][:m], s.sum(axis=0)) <= TOL and rel(d["Q"][:m], (s ** 2).sum(axis=0)) <= TOL


def test_unequal_n_and_k_in_one_pass(envs):
    """Records written at n = 0, 3, 4, 30 with the oracle's moments, then one
    pass to min = max = 64: k = 64, 61, 60, 34 side by side, kmin = 34 -> 32
    lanes per record, sample0 = n[e] + c differs between the entries."""
    b, r = envs("cornell")
    s = b.samples(None, 64)
    n0 = np.array([0, 3, 4, 30], dtype=np.uint32)[np.arange(b.n) % 4]
    S0, Q0 = adaptive_sim.moments_upto(s, n0)
    p, adapt = rule_params((0.0, 0.01, 64, 64, 64), b.n)
    with RayAccumulator(r, b.o, b.d, b.keys) as acc:
        acc.write(S0[None], Q0[None], n0[None])
        assert acc.select(adapt) == (b.n, int((64 - n0.astype(np.int64)).sum()))
        acc.render(p, adapt)
        assert r.last_launch()["lanes_per_pixel"] == 32
        d = flat(acc.read(S=True, Q=True, n=True))
        assert acc.select(adapt) == (0, 0)
    assert (d["n"] == 64).all()
    assert rel(d["S"], s.sum(axis=0)) <= TOL and rel(d["Q"], (s ** 2).sum(axis=0)) <= TOL


def test_order_and_batch_do_not_matter(envs):
    """At a fixed lane count a record's S, Q and n are the same bits wherever
    it stands: the records shuffled, and split over two accumulators."""
    b, r = envs("mesh")
    S, Q, n, _ = full_run(r, b.o, b.d, b.keys, "r4-32-4", 4)
    perm = np.random.default_rng(3).permutation(b.n)
    Sp, Qp, npm, _ = full_run(r, b.o[perm], b.d[perm], b.keys[perm], "r4-32-4", 4)
    assert same(Sp, S[perm]) and same(Qp, Q[perm]) and same(npm, n[perm])
    for part in (slice(0, 77), slice(77, b.n)):
        Sa, Qa, na, _ = full_run(r, b.o[part], b.d[part], b.keys[part], "r4-32-4", 4)
        assert same(Sa, S[part]) and same(Qa, Q[part]) and same(na, n[part])


# 3 ------------------------------------------------------ frame equivalence --
def test_the_frames_rays_are_the_frame(cornell):
    """Cornell's own 12 x 12 rays in image order on a 12 x 12 ray accumulator
    against a frame accumulator, both at 4 lanes, same rule, seed and bounces:
    the pass history, S, Q, n, err, the resolved frame, the features and the
    denoised frame and variance, bit for bit."""
    import torch
    gpu()
    W = H = 12
    o, d, k = cameras.to_image_order(*cameras.scene_camera_rays(cornell, W, H), W, H)
    tol, floor, lo, hi, step = ref.RULES["r4-32-4"]
    adapt = make_adapt(tol, hi, lo, step, floor)
    got = []
    with Renderer(cornell) as r:
        p = r.params(W, H, hi, ref.BOUNCES, ref.SEED)
        for make in (lambda: Accumulator(r, W, H, band=make_band(H, lanes_per_pixel=4)),
                     lambda: RayAccumulator(r, o, d, k, (H, W), band=make_band(H, lanes_per_pixel=4))):
            with make() as acc:
                passes = run_passes(acc, p, adapt)
                m = acc.read(S=True, Q=True, n=True, err=True)
                fb = torch.empty((H, W, 3), dtype=torch.float64, device="cuda")
                acc.resolve_device(fb.data_ptr(), True, torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                den, var = acc.denoise()
                got.append(dict(m, passes=passes, fb=fb.cpu().numpy(), den=den, var=var, **acc.features()))
    frame, rays = got
    assert frame["passes"] == rays["passes"] and len(frame["passes"]) >= 4
    assert len(np.unique(frame["n"])) >= 4
    for key in ("S", "Q", "n", "err", "fb", "tri", "obj", "N"):
        assert same(frame[key], rays[key]), key
    dP = float(np.abs(frame["P"] - rays["P"]).max())
    print(f"features P: frame against ray accumulator, largest difference {dP:.3e}, "
          f"bitwise equal {same(frame['P'], rays['P'])}")
    assert dP <= 1e-11
    if same(frame["P"], rays["P"]):
        assert same(frame["den"], rays["den"]) and same(frame["var"], rays["var"])
    else:   # (the filter reads P: its output then follows P's last bits)
        c, v = moments_numpy(rays["S"], rays["Q"], rays["n"])
        rc, rv = denoise_numpy(c, v, rays["obj"], rays["N"], rays["P"])
        assert same_bits(rays["den"], rc) and same_bits(rays["var"], rv)


# 4 ---------------------------------------------------------------- features --
@pytest.mark.parametrize("name", ["cornell", "mesh"])
def test_features_of_the_batch(envs, name):
    """tri is the oracle's intersect_objects, P within 1e-11, the records from
    OFF_AXIS[1] outside the scene's box (decided in f64) included."""
    b, r = envs(name)
    tri, P = oracle.intersect_objects(b.pk, np.concatenate([b.o, b.d], axis=1))
    with RayAccumulator(r, b.o, b.d, b.keys) as acc:
        f = flat(acc.features())
    hit = tri >= 0
    assert b.outside.sum() >= 48 and hit[b.outside].any()
    assert np.array_equal(f["tri"], np.where(hit, tri, -1))
    t = np.where(hit, tri, 0)
    assert np.array_equal(f["obj"], np.where(hit, b.pk.tri_obj[t], -1))
    assert same_bits(f["N"], np.where(hit[:, None], b.pk.tri_n[t], 0.0))
    dP = float(np.abs(f["P"] - np.where(hit[:, None], P, 0.0)).max())
    print(f"{name}: {int(hit.sum())} hits, {int((~hit).sum())} escapes, |P - oracle| = {dP:.3e} "
          f"({float(np.abs(f['P'] - np.where(hit[:, None], P, 0.0))[b.outside].max()):.3e} outside the box)")
    assert dP <= 1e-11


# 5 -------------------------------------------------------- other equalities --
@pytest.mark.parametrize("name", ["cornell", "mesh"])
def test_forced_f64_is_the_hybrid(envs, name):
    b, r = envs(name)
    a = full_run(r, b.o, b.d, b.keys, "r3-17-5", 4)
    f = full_run(r, b.o, b.d, b.keys, "r3-17-5", 4, flags=PT_FLAG_FORCE_F64)
    assert r.last_launch()["flags"] == PT_FLAG_FORCE_F64
    assert same(a[0], f[0]) and same(a[1], f[1]) and same(a[2], f[2]) and a[3] == f[3]


def test_russian_roulette_from_depth_1(envs):
    b, r = envs("cornell")
    sim = b.check_preconditions("r4-32-4", 1)
    S, Q, n, passes = full_run(r, b.o, b.d, b.keys, "r4-32-4", flags=PT_FLAG_RR | PT_FLAG_RAYS_SINGLE, rr_depth=1)
    assert passes == sim["passes"] and np.array_equal(n, sim["n"])
    wS, wQ = adaptive_sim.moments_upto(b.samples(1), n)
    assert rel(S, wS) <= TOL and rel(Q, wQ) <= TOL
    assert not np.array_equal(n, b.simulate("r4-32-4")["n"])   # (the roulette changes the run)


LOOK = dict(eye=(2.5, 1.5, 4.0), target=(0.0, 0.0, -24.0), fov_y=30.0, W=16, H=12)


def test_denoise_is_the_numpy_restatement(cornell):
    """A 16 x 12 look-at accumulator: the filtered frame and its variance are
    denoise_ref's on the accumulator's own moments and features, bit for bit."""
    gpu()
    W, H = LOOK["W"], LOOK["H"]
    o, d, k = cameras.to_image_order(*cameras.look_at_rays(**LOOK), W, H)
    p, adapt = rule_params("r4-32-4", W * H, H)
    with Renderer(cornell, ray_box=(LOOK["eye"], LOOK["eye"])) as r, RayAccumulator(r, o, d, k, (H, W)) as acc:
        run_passes(acc, p, adapt)
        for kw in ({}, dict(iters=2, sigma_l=1.0)):
            out, var = acc.denoise(**kw)
            m = acc.read(S=True, Q=True, n=True)
            f = acc.features()
            c, v = moments_numpy(m["S"], m["Q"], m["n"])
            rc, rv = denoise_numpy(c, v, f["obj"], f["N"], f["P"], **kw)
            assert np.isfinite(out).all() and same_bits(out, rc) and same_bits(var, rv)
        assert len(np.unique(m["n"])) > 2 and len(np.unique(f["obj"])) >= 3
        res = r.render_rays_adaptive(o, d, k, (H, W), 32, ref.BOUNCES, 0.05, 4, 4, 0.01, ref.SEED, denoise=True,
                                     iters=2, sigma_l=1.0, moments=True)
    assert res.fb.shape == (H, W, 3) and res.counts.shape == (H, W) and res.err.shape == (H, W)
    assert same(res.S, m["S"]) and same(res.counts, m["n"]) and same_bits(res.denoised, out)
    assert same_bits(res.denoised_var, var) and same(res.features["tri"], f["tri"])


def test_a_resumed_run_is_the_uninterrupted_run(envs, tmp_path):
    b, r = envs("mesh")
    kw = dict(max_spp=32, bounces=ref.BOUNCES, tol=0.05, min_spp=4, step_spp=4, floor=0.01, seed=ref.SEED,
              lanes_per_pixel=4, moments=True)
    whole = r.render_rays_adaptive(b.o, b.d, b.keys, **kw)
    assert whole.fb.shape == (b.n, 3) and whole.counts.shape == (b.n,) and whole.err.shape == (b.n,)
    ck = str(tmp_path / "rays.npz")
    assert r.render_rays_adaptive(b.o, b.d, b.keys, checkpoint=ck, max_passes=3, **kw) is None
    with pytest.raises(ValueError, match="another render"):   # other records: another key
        r.render_rays_adaptive(b.o, b.d, b.keys[::-1].copy(), checkpoint=ck, **kw)
    res = r.render_rays_adaptive(b.o, b.d, b.keys, checkpoint=ck, **kw)
    assert res.passes == whole.passes == b.simulate("r4-32-4")["passes"]
    for x, y in ((res.S, whole.S), (res.Q, whole.Q), (res.counts, whole.counts), (res.err, whole.err),
                 (res.fb, whole.fb)):
        assert same(x, y)


# 6 ---------------------------------------------------------------- refusals --
@pytest.mark.parametrize("flag,name", [(PT_FLAG_AA, "PT_FLAG_AA"), (PT_FLAG_LENS, "PT_FLAG_LENS"),
                                       (PT_FLAG_MEGAKERNEL, "PT_FLAG_MEGAKERNEL"), (PT_FLAG_COUNT, "PT_FLAG_COUNT"),
                                       (PT_FLAG_WALK_COUNT, "PT_FLAG_WALK_COUNT"),
                                       (PT_FLAG_KERNEL_TIMES, "PT_FLAG_KERNEL_TIMES"),
                                       (PT_FLAG_OUT_F64, "PT_FLAG_OUT_F64"), (1 << 7, "unknown bits")])
def test_flags_a_ray_pass_refuses(envs, flag, name):
    b, r = envs("mesh")
    p, adapt = rule_params("r4-32-4", 8, flags=flag | PT_FLAG_RR)
    with RayAccumulator(r, b.o[:8], b.d[:8], b.keys[:8]) as acc:
        with pytest.raises(_native.NativeError, match=name):
            acc.render(p, adapt)
        assert not acc.read(n=True)["n"].any()
        for bad in (dict(width=9), dict(height=2), dict(spp=31), dict(row_step=2), dict(sample_begin=1),
                    dict(lanes_per_pixel=2), dict(out_row_stride=64)):
            q, _ = rule_params("r4-32-4", 8)
            for key, v in bad.items():
                setattr(q, key, v)
            with pytest.raises(_native.NativeError):
                acc.render(q, adapt)
        q, _ = rule_params("r4-32-4", 8, flags=PT_FLAG_RAYS_SINGLE)   # accepted, no effect
        acc.render(q, adapt)
        info = r.last_launch()
        assert PATH_NAMES[info["path"]] == "single" and info["flags"] == PT_FLAG_RAYS_SINGLE
        assert (acc.read(n=True)["n"] == 4).all()


def test_shapes_create_refuses(envs):
    import torch
    b, r = envs("cornell")
    lib = _native.lib()
    rec = torch.from_numpy(make_rays(b.o[:4], b.d[:4], b.keys[:4]).view(np.uint8)).cuda()
    torch.cuda.synchronize()
    for w, h in ((0, 1), (1, 0), (-1, 4), (1 << 15, 1 << 15), (1 << 30, 1)):
        out = C.c_void_p(1)
        assert lib.pt_accum_create_rays(r._h, C.c_void_p(rec.data_ptr()), w, h, C.byref(out)) == -1
        assert not out.value and "2^30" in _native.last_error()
    out = C.c_void_p()
    assert lib.pt_accum_create_rays(r._h, None, 2, 2, C.byref(out)) == -1 and not out.value
    assert lib.pt_accum_create_rays(None, C.c_void_p(rec.data_ptr()), 2, 2, C.byref(out)) == -1
    with pytest.raises(ValueError):
        RayAccumulator(r, b.o[:4], b.d[:4], b.keys[:4], shape=(3, 2))


def test_denoise_on_a_banded_ray_accumulator_is_refused(envs):
    b, r = envs("cornell")
    with RayAccumulator(r, b.o[:48], b.d[:48], b.keys[:48], (6, 8), band=make_band(6, 0, 6, 2, 1)) as acc:
        p, adapt = rule_params("r4-32-4", 48, 6)
        assert acc.select(adapt) == (24, 96)       # the band's three rows of eight
        acc.render(p, adapt)
        n = acc.read(n=True)["n"]
        assert (n[1::2] == 0).all() and (n[0::2] == 4).all()   # iy odd: image rows 0, 2, 4
        for call in (acc.features, acc.denoise):
            with pytest.raises(_native.NativeError, match="whole frame"):
                call()
        acc.set_band(make_band(6))
        acc.denoise()


# 7 ------------------------------------------------------- the command line --
def test_cli_look_at_through_the_accumulator(cornell, tmp_path, capsys):
    gpu()
    from PIL import Image
    from pathtracerpython_amd import main as cli
    from conftest import CORNELL
    out, raw, aov = str(tmp_path / "img.png"), str(tmp_path / "fb.npy"), str(tmp_path / "aov")
    argv = [CORNELL, "-r", "32", "-b", "3", "--look-at", "2.5", "1.5", "4", "0", "0", "-24", "--fov", "30",
            "--size", "16", "12", "--seed", "9", "--ray-accum", "--noise", "0.05", "--min-spp", "4", "--step-spp", "4",
            "--denoise", "--denoise-iters", "2", "--denoise-sigma", "1.0", "--save-aov", aov, "--out", out,
            "--save-raw", raw]
    fb = cli.main(argv)
    text = capsys.readouterr().out
    assert "adaptive:" in text and "denoise:" in text and "look-at" in text
    assert fb.shape == (12, 16, 3) and same(np.load(raw), fb) and Image.open(out).size == (16, 12)
    o, d, k = cameras.to_image_order(*cameras.look_at_rays(**LOOK), 16, 12)
    with Renderer(cornell, ray_box=(LOOK["eye"], LOOK["eye"])) as r:
        res = r.render_rays_adaptive(o, d, k, (12, 16), 32, 3, 0.05, 4, 4, 0.01, 9, denoise=True, iters=2,
                                     sigma_l=1.0)
    assert same(fb, res.denoised)
    assert same(np.load(aov + "_counts.npy"), res.counts) and same(np.load(aov + "_err.npy"), res.err)
    assert same(np.load(aov + "_noisy.npy"), res.fb) and same(np.load(aov + "_obj.npy"), res.features["obj"])
    assert same(np.load(aov + "_point.npy"), res.features["P"]) and same(np.load(aov + "_var.npy"), res.denoised_var)
    ck = str(tmp_path / "ck.npz")
    plain = [a for a in argv if a not in ("--denoise",)]
    for drop in ("--denoise-iters", "--denoise-sigma", "--save-aov"):
        i = plain.index(drop)
        del plain[i:i + 2]
    a = cli.main(plain + ["--checkpoint", ck])
    assert same(a, res.fb) and same(cli.main(plain + ["--checkpoint", ck]), a)   # (the second: all from the file)
    with pytest.raises(SystemExit, match="unless --ray-accum"):   # without the switch: as it always was
        cli.main([x for x in plain if x != "--ray-accum"])
