"""What pf_conv2d runs for a grid of arguments is what it ran before the plan was gathered into csrc/conv_plan.hip (-m "not gpu"): form,
tile, wave groups, K split wanted / granted, statistics tiles and K-split scratch from pf_conv_describe (tools/conv_plan_table.py) against
tests/golden/conv_plans.json, which was recorded from the commit before that entry existed (its two query entries, and its launchers made
to report their template arguments - profiles/r08_conv_plan_probe.patch).  A change that alters a conv plan on purpose regenerates the
file with `python tools/conv_plan_table.py --write` and says so."""
import ctypes as C
import json
import os

import pytest

from polyffusion_amd import _lib
from tools import conv_plan_table as cpt


@pytest.fixture(scope="module")
def recorded():
    with open(cpt.GOLDEN) as f:
        return json.load(f)


def _lib_of(variant):
    if not os.path.exists(_lib.lib_path(variant)):
        from polyffusion_amd.build import build
        build(verbose=False, variant=variant)
    return _lib.load(variant)


def test_recorded_table_reaches_every_form(recorded):
    assert len(recorded) > 2000
    forms = {row[0] for row in recorded.values()}
    assert forms == set(range(len(_lib.CONV_FORMS)))   # at least one accepted case of each of the seven forms
    # with and without the K-split scratch: a granted row splits, its ungranted twin does not
    granted = [k for k in recorded if k.endswith(" +ws")]
    assert granted and all(recorded[k][6] == recorded[k][5] > 1 and recorded[k[:-4]][6] == 1 for k in granted)


@pytest.mark.parametrize("variant", ["", "f16"])
def test_plans_equal_the_recorded_table(recorded, variant):
    _lib_of(variant)
    diff = cpt.differences(recorded, cpt.table(cpt._Describe(variant)))
    assert not diff, "\n".join(diff[:40])


@pytest.mark.parametrize("variant", ["", "f16"])
def test_older_queries_read_the_same_plan(variant):
    lib = _lib_of(variant)
    info, n = _lib.ConvPlanInfo(), 0
    for key, a in cpt.cases():
        if lib.pf_conv_describe(C.byref(a), C.byref(info)) != 0:
            continue
        for ws in ((None, 0), (cpt.P, info.splitk_ws_bytes)):
            a.splitk_ws, a.splitk_ws_bytes = ws
            assert lib.pf_conv_describe(C.byref(a), C.byref(info)) == 0
            assert (lib.pf_conv_stats_tiles(C.byref(a)), lib.pf_conv_splitk_ws_bytes(C.byref(a))) == (info.stats_tiles, info.splitk_ws_bytes), key
            n += 1
    assert n > 4000


def test_describe_refuses_what_conv2d_refuses():
    lib = _lib.load()
    key, a = next(cpt.cases())
    a.ks = 2
    info = _lib.ConvPlanInfo(form=5, tile_h=7)
    assert lib.pf_conv_describe(C.byref(a), C.byref(info)) == -1
    msg = lib.pf_last_error()
    assert msg == b"conv: ks must be 1 or 3 (got 2)" and (info.form, info.tile_h, info.flops) == (0, 0, 0.0)
    assert lib.pf_conv2d(C.byref(a), None) == -1 and lib.pf_last_error() == msg   # refused before anything touches a device
    a.ks, a.a_planes, a.precision, a.prologue, a.batch, a.hin, a.win, a.c0 = 1, 1, 1, 0, 2048, 1, 1024, 512   # the planes GEMM's 2 GiB check
    assert lib.pf_conv_describe(C.byref(a), C.byref(info)) == -1 and lib.pf_last_error().startswith(b"gemm_planes: the A plane pair must stay below 2 GiB")
