"""The render loop's unit forms on the host build, test by test
(tests/hostcheck/unit_forms_selftest.cpp): quad_m against the plain branchy
formula kept in the test file (bitwise: a restructured quad_m must keep its
values), and the closest ray's unit-level form (closest_unit_m, closest_add_bf) against the
per-member verdicts and eval64 — the same certain candidate, triangle and
interval, no ambiguity lost, no certain verdict the f64 evaluation
contradicts, and closest_bits_m rebuilding exactly the members' bits."""
import ctypes as C
import os

import pytest

import hostlib
import grazing
from conftest import quad_scene
from pathtracerpython_amd.pack import pack_scene

NAMES = ("candidate/triangle/interval differs", "ambiguity lost", "certain verdict wrong (eval64)",
         "quad_m differs from the branchy formula", "closest_bits_m differs", "closest_add_bf differs from closest_add")


@pytest.fixture(scope="module")
def forms():
    """unit_forms_selftest.cpp built by the hostcheck Makefile."""
    lib = hostlib.build(os.path.join(hostlib.HOSTCHECK, "build"), "unit_forms_selftest")
    lib.hc_unit_forms_selftest.restype = C.c_int
    return lib


def run(lib, pk, n, seed):
    out = (C.c_int64 * 12)()
    assert lib.hc_unit_forms_selftest(C.byref(pk.desc), C.c_int64(n), C.c_uint64(seed), out) == 0
    o = list(out)
    print("unit forms: %d unit tests, %d with an ambiguous member, %d certain candidates "
          "(single %d, parallelogram %d, skew %d); failures %s" % (o[6], o[7], o[8], o[9], o[10], o[11], o[:6]))
    for name, v in zip(NAMES, o[:6]):
        assert v == 0, name
    return dict(tests=o[6], amb=o[7], cand=o[8], single=o[9], par=o[10], skew=o[11])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_unit_forms_cornell(forms, packed, seed):
    r = run(forms, packed, 20000, seed)
    assert r["amb"] >= 1000 and r["cand"] >= 1000


@pytest.mark.parametrize("seed", [3, 8])
def test_unit_forms_quad_scene(forms, tmp_path, seed):
    r = run(forms, pack_scene(quad_scene(tmp_path, seed)), 4000, seed)
    assert r["single"] >= 1 and r["par"] >= 1 and r["skew"] >= 1


def test_unit_forms_grazing_uniform(forms, tmp_path):
    sc, rep = grazing.grazing_scene(tmp_path, "uniform", 24)
    r = run(forms, pack_scene(sc), 1500, 5)
    assert r["cand"] > 0
