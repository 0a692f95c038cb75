"""The light pick of the lane code on the host (pt_core.h): pick_light's
counting forms — the pair form of a two-triangle light, the general count, the
table read ahead of its use (light_tab) — against the reference rule's loop
for EVERY u = k / 2^24 and for u outside [0, 1) and NaN, the host's check that
chooses the form (SceneK::light_mono, pt_prepare.h), and the light point bit
for bit the one found through the light_tri table.
tests/hostcheck/pt_light_host.cpp holds the comparisons: as a stand-alone
program on synthetic tables (one triangle, a zero-area middle or last
triangle, seven random areas, tables that are not monotone or not finite and
must keep the loop), and as a library on the table prepare_scene builds for
the Cornell room.  The GPU cases are tests/test_gpu_light_pick.py."""
import ctypes as C
import subprocess

import pytest

import hostlib


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """(program, library) of pt_light_host.cpp, by the hostcheck Makefile."""
    d = tmp_path_factory.mktemp("light_host")
    exe, so = hostlib.make(d, "pt_light_host"), hostlib.make(d, "libpt_light_host.so")
    return exe, so


def test_counting_forms_equal_the_loop_on_synthetic_tables(built):
    """Exit 0: on every table the forms agree with the loop for all 2^24
    uniforms and the six outside values, the host's check sorted the tables
    (mono: quad, one, zero-middle, zero-last, seven; loop: non-monotone, nan,
    inf), and 10^4 light points per table are bit-identical."""
    r = subprocess.run([built[0]], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok"
    forms = {ln.split(":")[0]: ln for ln in lines[:-1]}
    assert set(forms) == {"quad", "one", "zero-middle", "zero-last", "seven", "non-monotone", "nan",
                          "inf"}
    assert "form 2" in forms["quad"] and "2 triangles picked" in forms["quad"]
    assert "form 1" in forms["seven"] and "7 triangles picked" in forms["seven"]
    assert "form 1" in forms["zero-middle"] and "2 triangles picked" in forms["zero-middle"]
    assert "form 2" in forms["zero-last"] and "1 triangles picked" in forms["zero-last"]
    for name in ("non-monotone", "nan", "inf"):
        assert "form 0" in forms[name]


def test_cornell_light_takes_the_pair_form(built, packed):
    """prepare_scene's table of the Cornell light: monotone, two triangles
    (the pair form), light_tri[i] == n_obj_tri + i, cum[n_light] the bits of
    light_sum, and no mismatch over all uniforms."""
    lib = C.CDLL(built[1])
    lib.hc_light_check.restype = C.c_int
    info = (C.c_int32 * 3)()
    assert lib.hc_light_check(C.byref(packed.desc), info) == 0
    assert list(info) == [1, 2, 0]
