"""The host's launch rules (pathtracerpython_amd/csrc/pt_plan.h) without a GPU:
the checks' precedence and texts, the lanes per pixel, the tail rows, the
work-items, the 2^32 / 2^30 / 2^29 guards and the route of pt_render_device,
pt_radiance_device and the accumulator passes, through the exports of
tests/hostcheck.

Every expected value below is a literal.  They were printed once by the
functions as they stood in pt_hip.hip before they moved to the header, and
agree with the hand derivations elsewhere in the tree (choose_split's comment,
test_gpu_adaptive_wide.py's pass sizes, the 64M-slot limit of DESIGN.md)."""
import ctypes as C

import pytest

from pathtracerpython_amd._abi import (PT_FLAG_AA, PT_FLAG_COUNT, PT_FLAG_FORCE_F64, PT_FLAG_KERNEL_TIMES,
                                       PT_FLAG_LENS, PT_FLAG_MEGAKERNEL, PT_FLAG_RAYS_SINGLE, PT_FLAG_WALK_COUNT,
                                       make_adapt, make_params)

# a scene's facts: bvh, walkable, n_cu, has_lens
K2 = (0, 0, 256, 0)        # no BVH (the Cornell room)
K5 = (1, 1, 256, 0)        # a BVH the walk kernels take
DEEP = (1, 0, 256, 0)      # a BVH deeper than the walk stack
LENSED = (1, 1, 256, 1)

LANES = "lanes_per_pixel must be 0 or a power of two <= min(64, spp)"
ITEMS = "launch needs 2^32 or more work-items (32-bit lane index)"
AA_NO_COUNT = ("PT_FLAG_AA does not combine with PT_FLAG_COUNT, PT_FLAG_WALK_COUNT or PT_FLAG_KERNEL_TIMES: "
               "the antialiasing kernels do not count")
LENS_NO_COUNT = ("PT_FLAG_LENS does not combine with PT_FLAG_COUNT, PT_FLAG_WALK_COUNT or PT_FLAG_KERNEL_TIMES: "
                 "the lens kernels do not count")
LENS_NO_SCENE = "PT_FLAG_LENS needs a scene created with a lens (pt_scene_create_lens)"
UNKNOWN = "unknown flag bits (bit 7, v4's PT_FLAG_TREE_WALK, is retired)"
WHOLE = ("an accumulator pass renders the whole frame: row_begin 0, row_end height, row_step 1, sample_begin 0, "
         "out_row_stride 0, lanes_per_pixel 0")

FRAME_FIELDS = ("split", "split_log2", "npix", "tail_pix", "tail_lane", "tail_log2", "items", "wavefront",
                "rr_depth", "out_stride", "first_row", "n_rows")


def _ints(v):
    return (C.c_int32 * len(v))(*v)


def frame(lib, scene, p):
    """pt_render_device's plan: a dict of FRAME_FIELDS, or the refusal's text."""
    out, msg = (C.c_int64 * 12)(), C.create_string_buffer(512)
    rc = lib.hc_plan_frame(C.byref(p), _ints(scene), out, msg, 512)
    assert rc in (0, -1)
    return dict(zip(FRAME_FIELDS, out)) if rc == 0 else msg.value.decode()


def rays(lib, scene, p, n, has_s=0, has_q=0):
    """pt_radiance_device's plan: (split, split_log2, items, wavefront), or the refusal's text."""
    out, msg = (C.c_int64 * 4)(), C.create_string_buffer(512)
    rc = lib.hc_plan_rays(C.byref(p), C.c_int64(n), has_s, has_q, _ints(scene), out, msg, 512)
    assert rc in (0, -1)
    return tuple(out) if rc == 0 else msg.value.decode()


def check_pass(lib, scene, acc, p, ap):
    """An accumulator pass's checks (acc: W, H, lanes, rays, aa, lens): '' or the refusal's text."""
    msg = C.create_string_buffer(1024)
    rc = lib.hc_plan_check_pass(C.byref(p), C.byref(ap), _ints(acc), _ints(scene), msg, 1024)
    assert (rc == 0) == (msg.value == b"")
    return msg.value.decode()


def plan_pass(lib, scene, acc, count, kmin, flags=0):
    """(split, items, blocks, wf_blocks, wavefront) of a pass, or the refusal's text."""
    out, msg = (C.c_int64 * 5)(), C.create_string_buffer(512)
    rc = lib.hc_plan_pass(_ints(acc), _ints(scene), C.c_uint32(flags), C.c_uint32(count), C.c_uint32(kmin), out,
                          msg, 512)
    assert rc in (0, -1)
    return tuple(out) if rc == 0 else msg.value.decode()


@pytest.fixture(scope="module")
def lib(hostcheck):
    hostcheck.hc_plan_lane_cap.restype = C.c_uint32
    for f in (hostcheck.hc_plan_frame, hostcheck.hc_plan_rays, hostcheck.hc_plan_check_pass, hostcheck.hc_plan_pass):
        f.restype = C.c_int
    return hostcheck


def test_lane_cap(lib):
    assert [lib.hc_plan_lane_cap(s) for s in (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 4096)] == \
        [1, 2, 2, 4, 4, 4, 8, 32, 64, 64, 64]
    # spp below the cap, on both kinds of scene
    for scene in (K2, K5):
        assert [frame(lib, scene, make_params(64, 64, s, 3, 1))["split"] for s in (1, 3, 5)] == [1, 2, 4]


def test_whole_frame_without_a_bvh(lib):
    # 512^2 x 64 spp: 16 lanes per pixel (PT_MIN_SPL 4); the top sixteenth of the rows, from row 480 on, 64
    f = frame(lib, K2, make_params(512, 512, 64, 3, 1))
    assert f == dict(split=16, split_log2=4, npix=262144, tail_pix=245760, tail_lane=3932160, tail_log2=6,
                     items=4980736, wavefront=0, rr_depth=-1, out_stride=1536, first_row=0, n_rows=512)
    assert f["tail_pix"] == 480 * 512 and f["items"] == 480 * 512 * 16 + 32 * 512 * 64


def test_first_band_of_n(lib):
    # the same frame's first band of an N-way split: the launch keeps 2^20 lanes (256 CUs x 4 rounds)
    got = {}
    for n in (2, 4, 8):
        f = frame(lib, K2, make_params(512, 512, 64, 3, 1, row_step=n))   # interleaved rows
        g = frame(lib, K2, make_params(512, 512, 64, 3, 1, row_end=512 // n))   # a block of rows: no tail rows
        assert f["split"] == g["split"] and g["tail_pix"] == g["npix"]
        got[n] = (f["split"], f["npix"], f["tail_pix"], f["tail_lane"], f["tail_log2"], f["items"], g["items"])
    assert got == {2: (16, 131072, 122880, 1966080, 6, 2490368, 2097152),
                   4: (16, 65536, 61440, 983040, 6, 1245184, 1048576),
                   8: (32, 32768, 30720, 983040, 6, 1114112, 1048576)}


def test_bvh_slots(lib):
    # 64 slots per pixel at the K5 sizes: 16M slots, and 64M, the limit
    f = frame(lib, K5, make_params(512, 512, 64, 3, 1))
    assert (f["split"], f["items"], f["tail_pix"], f["wavefront"]) == (64, 16777216, 262144, 1)
    f = frame(lib, K5, make_params(1024, 1024, 256, 3, 1))
    assert (f["split"], f["items"], f["wavefront"]) == (64, 67108864, 1)
    # the band's fixed count of an accumulator pass, capped at the pass's samples
    assert plan_pass(lib, K5, (7, 5, 4, 0, -1, -1), 35, 3) == (2, 70, 2, 1, 1)
    assert plan_pass(lib, K5, (7, 5, 4, 0, -1, -1), 35, 100) == (4, 140, 3, 1, 1)
    assert plan_pass(lib, K5, (7, 5, 64, 0, -1, -1), 35, 100) == (64, 2240, 35, 9, 1)


def test_accumulator_pass_of_35_pixels(lib):
    acc = (7, 5, 0, 0, -1, -1)
    got = [plan_pass(lib, K2, acc, 35, k) for k in (16, 17, 31, 32, 48, 64, 100)]
    assert [g[0] for g in got] == [16, 16, 16, 32, 32, 64, 64]
    assert [g[1:] for g in got] == [(560, 9, 3, 0)] * 3 + [(1120, 18, 5, 0)] * 2 + [(2240, 35, 9, 0)] * 2


def test_lanes_per_pixel_check(lib):
    p = make_params(64, 64, 16, 3, 1, lanes_per_pixel=16)
    assert frame(lib, K2, p)["split"] == 16
    for spp, lanes in ((16, 3), (16, 32), (100, 128), (16, -2)):
        assert frame(lib, K2, make_params(64, 64, spp, 3, 1, lanes_per_pixel=lanes)) == LANES
        assert rays(lib, K2, make_params(1, 1, spp, 3, 1, lanes_per_pixel=lanes), 10) == LANES


def test_routes(lib):
    assert frame(lib, K5, make_params(64, 64, 16, 3, 1))["wavefront"] == 1
    for flag in (PT_FLAG_COUNT, PT_FLAG_FORCE_F64, PT_FLAG_MEGAKERNEL):
        f = frame(lib, K5, make_params(64, 64, 16, 3, 1, flag))
        assert (f["split"], f["items"], f["wavefront"]) == (16, 65536, 0)
    assert frame(lib, DEEP, make_params(64, 64, 16, 3, 1))["wavefront"] == 0
    assert frame(lib, K2, make_params(64, 64, 16, 3, 1))["wavefront"] == 0
    # 2^29 path slots take the single kernel, one row less the wavefront
    f = frame(lib, K5, make_params(4096, 2048, 64, 3, 1, lanes_per_pixel=64))
    assert (f["items"], f["wavefront"]) == (1 << 29, 0)
    f = frame(lib, K5, make_params(4096, 2047, 64, 3, 1, lanes_per_pixel=64))
    assert (f["items"], f["wavefront"]) == (536608768, 1)
    # rays: the frames' rule, and PT_FLAG_RAYS_SINGLE
    assert rays(lib, K5, make_params(1, 1, 16, 3, 1), 1000) == (16, 4, 16000, 1)
    assert rays(lib, K5, make_params(1, 1, 16, 3, 1, PT_FLAG_RAYS_SINGLE), 1000) == (16, 4, 16000, 0)
    assert rays(lib, K5, make_params(1, 1, 16, 3, 1, PT_FLAG_FORCE_F64), 1000) == (16, 4, 16000, 0)
    assert rays(lib, DEEP, make_params(1, 1, 16, 3, 1), 1000) == (16, 4, 16000, 0)
    assert rays(lib, K2, make_params(1, 1, 16, 3, 1), 1000) == (16, 4, 16000, 0)
    assert rays(lib, K2, make_params(1, 1, 64, 3, 1), 35) == (64, 6, 2240, 0)
    # a frame accumulator's pass follows the frames' rule; a ray accumulator's is the single kernel
    assert plan_pass(lib, K5, (7, 5, 0, 0, -1, -1), 35, 16)[4] == 1
    assert plan_pass(lib, K5, (7, 5, 0, 0, -1, -1), 35, 16, PT_FLAG_MEGAKERNEL)[4] == 0
    assert plan_pass(lib, K5, (7, 5, 0, 1, -1, -1), 35, 16)[4] == 0


def test_precedence_and_texts(lib):
    def P(flags, **kw):
        return make_params(64, 64, 16, 3, 1, flags, **kw)
    assert frame(lib, LENSED, P(PT_FLAG_LENS | PT_FLAG_COUNT | PT_FLAG_AA)) == LENS_NO_COUNT
    assert frame(lib, LENSED, P(PT_FLAG_LENS | PT_FLAG_KERNEL_TIMES)) == LENS_NO_COUNT
    assert frame(lib, K5, P(PT_FLAG_AA | PT_FLAG_COUNT)) == AA_NO_COUNT
    # the stats flags of an antialiased launch: refused where the single kernel takes it
    assert frame(lib, DEEP, P(PT_FLAG_AA | PT_FLAG_WALK_COUNT)) == AA_NO_COUNT
    assert frame(lib, K5, P(PT_FLAG_AA | PT_FLAG_WALK_COUNT | PT_FLAG_MEGAKERNEL)) == AA_NO_COUNT
    assert frame(lib, K5, P(PT_FLAG_AA | PT_FLAG_WALK_COUNT))["wavefront"] == 1
    assert frame(lib, K5, P(PT_FLAG_LENS)) == LENS_NO_SCENE
    assert frame(lib, DEEP, P(PT_FLAG_LENS | PT_FLAG_AA | PT_FLAG_MEGAKERNEL)) == LENS_NO_SCENE
    assert frame(lib, LENSED, P(PT_FLAG_LENS))["wavefront"] == 1
    assert frame(lib, K5, P(1 << 7)) == UNKNOWN
    assert frame(lib, K5, P((1 << 7) | PT_FLAG_LENS | PT_FLAG_COUNT)) == UNKNOWN
    assert frame(lib, K5, P(0, out_row_stride=191)) == "out_row_stride must be 0 or >= width*3"
    assert frame(lib, K5, P(0, out_row_stride=191, lanes_per_pixel=3)) == "out_row_stride must be 0 or >= width*3"
    assert frame(lib, K5, P(0, out_row_stride=192))["out_stride"] == 192
    assert rays(lib, K5, make_params(1, 1, 16, 3, 1, PT_FLAG_AA), 10) == (
        "unsupported flag bits: pt_radiance takes PT_FLAG_RR, PT_FLAG_FORCE_F64, PT_FLAG_OUT_F64 and "
        "PT_FLAG_RAYS_SINGLE only (the ray kernels do not count, jitter or draw a lens point)")
    assert rays(lib, K5, make_params(1, 1, 16, 3, 1), 10, has_s=1) == "out_S and out_Q: both or neither"


def test_accumulator_pass_checks(lib):
    ap = make_adapt(0.01, 16, 8, 8)
    ray_acc, frame_acc = (8, 6, 0, 1, -1, -1), (8, 6, 0, 0, -1, -1)
    tail = ("): a pass of a ray accumulator takes PT_FLAG_RR, PT_FLAG_FORCE_F64 and PT_FLAG_RAYS_SINGLE only "
            "(the ray list kernel does not count, jitter or draw a lens point, and is the single kernel already)")
    assert check_pass(lib, K5, ray_acc, make_params(8, 6, 16, 3, 1, PT_FLAG_AA | PT_FLAG_COUNT), ap) == \
        "unsupported flag bits (PT_FLAG_COUNT, PT_FLAG_AA" + tail
    assert check_pass(lib, K5, ray_acc, make_params(8, 6, 16, 3, 1, PT_FLAG_AA | (1 << 20)), ap) == \
        "unsupported flag bits (PT_FLAG_AA, unknown bits" + tail
    assert check_pass(lib, K5, ray_acc, make_params(8, 6, 16, 3, 1, PT_FLAG_RAYS_SINGLE), ap) == ""
    assert check_pass(lib, K5, frame_acc, make_params(8, 6, 16, 3, 1, PT_FLAG_RAYS_SINGLE), ap) == UNKNOWN
    for acc in (ray_acc, frame_acc):
        assert check_pass(lib, K5, acc, make_params(8, 6, 16, 3, 1), ap) == ""
        assert check_pass(lib, K5, acc, make_params(8, 5, 16, 3, 1), ap) == "width/height are not the accumulator's"
        assert check_pass(lib, K5, acc, make_params(8, 6, 16, 3, 1, row_step=2), ap) == WHOLE
        assert check_pass(lib, K5, acc, make_params(8, 6, 16, 3, 1, lanes_per_pixel=4), ap) == WHOLE
        assert check_pass(lib, K5, acc, make_params(8, 6, 8, 3, 1), ap) == "spp must be the budget max_spp"
        assert check_pass(lib, K5, acc, make_params(8, 6, 16, 3, 1), make_adapt(0.01, 16, 1, 8)) == \
            "need 2 <= min_spp <= max_spp"
    # the remembered PT_FLAG_AA / PT_FLAG_LENS, then the scene's say
    assert check_pass(lib, K5, (8, 6, 0, 0, 0, -1), make_params(8, 6, 16, 3, 1, PT_FLAG_AA), ap).startswith(
        "this accumulator's passes so far were made with the other value of PT_FLAG_AA: ")
    assert check_pass(lib, LENSED, (8, 6, 0, 0, -1, 1), make_params(8, 6, 16, 3, 1), ap).startswith(
        "this accumulator's passes so far were made with the other value of PT_FLAG_LENS: ")
    assert check_pass(lib, K5, frame_acc, make_params(8, 6, 16, 3, 1, PT_FLAG_LENS), ap) == LENS_NO_SCENE
    assert check_pass(lib, DEEP, frame_acc, make_params(8, 6, 16, 3, 1, PT_FLAG_AA | PT_FLAG_WALK_COUNT), ap) == \
        AA_NO_COUNT
    assert check_pass(lib, K5, frame_acc, make_params(8, 6, 16, 3, 1, PT_FLAG_COUNT), ap).startswith(
        "unsupported flag bits: an accumulator pass takes ")


def test_work_item_guards(lib):
    # 2^28 pixels x 16 lanes = 2^32: refused
    assert frame(lib, K2, make_params(65536, 4096, 64, 3, 1, lanes_per_pixel=16)) == ITEMS
    # x 8 and x 4: with the tail rows' lanes still below 2^32
    f = frame(lib, K2, make_params(65536, 4096, 64, 3, 1, lanes_per_pixel=8))
    assert (f["tail_pix"], f["tail_lane"], f["tail_log2"], f["items"]) == (251658240, 2013265920, 6, 3087007744)
    f = frame(lib, K2, make_params(65536, 4096, 64, 3, 1, lanes_per_pixel=4))
    assert (f["tail_pix"], f["tail_lane"], f["tail_log2"], f["items"]) == (251658240, 1006632960, 5, 1543503872)
    # 3 * 2^30 lanes, where only the tail rows' extra lanes would overflow: accepted, without a tail
    f = frame(lib, K2, make_params(49152, 8192, 64, 3, 1, lanes_per_pixel=8))
    assert (f["npix"], f["tail_pix"], f["tail_lane"], f["tail_log2"], f["items"]) == \
        (402653184, 402653184, 3221225472, 3, 3221225472)
    # rays
    p = make_params(1, 1, 64, 3, 1, lanes_per_pixel=64)
    assert rays(lib, K2, p, 1 << 26) == ITEMS
    assert rays(lib, K2, p, (1 << 26) - 1) == (64, 6, 4294967232, 0)
    assert rays(lib, K2, make_params(1, 1, 1, 3, 1), 1 << 30) == "need 0 <= n_rays < 2^30"
    assert rays(lib, K2, make_params(1, 1, 1, 3, 1), (1 << 30) - 1) == (1, 0, 1073741823, 0)
    # an accumulator pass
    acc = (65536, 1024, 64, 0, -1, -1)
    assert plan_pass(lib, K2, acc, 1 << 26, 64) == ITEMS
    assert plan_pass(lib, K2, acc, (1 << 26) - 1, 64) == (64, 4294967232, 67108863, 16777216, 0)
