"""The conv case matrix on a machine without a GPU (-m "not gpu"; tests/conv_matrix.py): it reaches every plan class of
tests/golden/conv_plans.json in both builds, with the edges each class admits; its float64 oracle equals compositions of torch's own ops;
and its error budget has teeth - the float64 emulation of the documented split with one defect at a time leaves it, the unbroken emulation
and torch float32 stay inside on every case.  The class list is read from the recorded table, so a new plan class fails the gate until
conv_matrix._families() learns it."""
import os

import numpy as np
import pytest
import torch

import conv_matrix as cm
from polyffusion_amd import _lib
from tools import conv_error_model

VARIANTS = ("", "f16")


def _lib_of(variant):
    if not os.path.exists(_lib.lib_path(variant)):
        from polyffusion_amd.build import build
        build(verbose=False, variant=variant)
    return _lib.load(variant)


@pytest.fixture(scope="module")
def matrix():
    return cm.cases(_lib_of(""))


def _ragged(s, cls):
    ho, wo = (s.h, s.w) if s.fold else cm.out_hw(s)
    return ho % cls[1] != 0 or wo % cls[2] != 0


def test_matrix_reaches_every_recorded_plan_class_with_its_edges(matrix):
    classes = cm.recorded_classes()
    assert len(classes) == 25
    assert len({k for k, _ in matrix}) == len(matrix)
    for variant in VARIANTS:   # the plan does not depend on the element type: both builds put every case in the class it was built for
        lib = _lib_of(variant)
        for key, s in matrix:
            info = cm.describe(lib, s)
            assert info is not None and cm.plan_class(info) == s.cls, (variant, key)
            if s.stats:
                assert int(cm.stats_tile_map(s, info).max()) + 1 == info.stats_tiles, key
    missing = []
    for cls in classes:
        members = [s for _, s in matrix if s.cls == cls]
        if not members:
            missing.append((cls, "no case"))
            continue
        # what a class cannot have: the 16x16 tile and the Winograd form need sizes that are multiples of 16, the Winograd form N % 64 == 0
        # on its 64-channel tile, the planes GEMM a single source (conv_validate, conv_wino_eligible, conv_pick_tile)
        want = {"ragged pixels": cls[0] != cm.WINO and cls[:3] != (cm.SPLIT, 16, 16), "N off the tile": cls[0] != cm.WINO,
                "two sources": cls[0] != cm.PLANES, "stats_out": True, "ld_out > n": True}
        have = {"ragged pixels": any(_ragged(s, cls) for s in members), "N off the tile": any(s.n % cls[3] for s in members),
                "two sources": any(s.c1 for s in members), "stats_out": any(s.stats for s in members), "ld_out > n": any(s.ldo for s in members)}
        missing += [(cls, what) for what, w in want.items() if w and not have[what]]
        # every option the class admits on one of its geometries appears in it
        lib = _lib_of("")
        for opt in cm.OPTIONS:
            if any(cm.has_option(s, opt) for s in members):
                continue
            for s in members:
                t = cm.with_option(s, opt, cls[3])
                info = None if t is None or t is s else cm.describe(lib, t)
                if info is not None and cm.plan_class(info) == cls and cm.gmac(t) <= 0.3:
                    missing.append((cls, opt))
                    break
    assert not missing, missing
    for opt in cm.OPTIONS:
        assert any(cm.has_option(s, opt) for _, s in matrix), opt
    rows = [int(r) for k, s in matrix if s.sbias == 2 for r in cm.inputs(k, s)["sbias_rows"]]
    assert min(rows) < 0 and max(rows) >= cm.SB_NROWS
    # half benign, half harsh; only the classes whose cheapest member is large are checked on windows
    assert abs(sum(s.harsh for _, s in matrix) * 2 - len(matrix)) <= len(classes)
    assert all(cm.gmac(s) <= cm.BIG_GMAC or s.cls in cm.BIG_CLASSES for _, s in matrix)


def test_windows_of_a_big_case_cover_corners_edges_and_interior(matrix):
    lib = _lib_of("")
    big = [(k, s) for k, s in matrix if cm.gmac(s) > cm.BIG_GMAC]
    assert big
    for key, s in big:
        info = cm.describe(lib, s)
        ho, wo = cm.out_hw(s)
        regs = cm.regions(s, info)
        assert {b for b, _, _ in regs} == {0, s.b - 1} and len(regs) == 10 * len({0, s.b - 1})
        up = 2 if s.fold else 1
        for b, oy, ox in regs:
            assert oy[0] >= 0 and oy[-1] < ho and ox[0] >= 0 and ox[-1] < wo, key
            # at least two whole workgroup tiles in both directions, and a tile boundary strictly inside
            assert len(oy) >= 2 * up * info.tile_h and len(ox) >= 2 * up * info.tile_w
            assert oy[0] // (up * info.tile_h) != oy[-1] // (up * info.tile_h) and ox[0] // (up * info.tile_w) != ox[-1] // (up * info.tile_w)
        corners = {(oy[0] == 0, oy[-1] == ho - 1, ox[0] == 0, ox[-1] == wo - 1) for _, oy, ox in regs}
        assert {(True, False, True, False), (True, False, False, True), (False, True, True, False), (False, True, False, True),
                (False, False, False, False)} <= corners, key


def test_oracle_equals_the_torch_composition_in_float64(matrix):
    """guards the oracle's own indexing: upsampling, stride parity, bottom-right padding, the concat and x1_bmod, the GeGLU interleave"""
    n = 0
    for key, s in matrix:
        if cm.gmac(s) >= cm.CHEAP_GMAC:
            continue
        d = cm.inputs(key, s)
        ho, wo = cm.out_hw(s)
        for variant in VARIANTS if s.a_planes else ("",):
            want = cm.torch_compose(s, d, torch.float64, variant)
            for b in range(s.b):
                got = cm.oracle(s, d, b, np.arange(ho), np.arange(wo), variant).ref
                assert got.shape == want[b].shape
                assert float((got - want[b]).abs().max()) <= 1e-12 * float(want[b].abs().max()), (key, variant, b)
        n += 1
    assert n > 80


@pytest.fixture(scope="module")
def teeth(matrix):
    """per case and build: the largest err / tol of the unbroken emulation and of torch float32, and on the small cases of every defect"""
    lib = _lib_of("")
    rows = []
    for key, s in matrix:
        d = cm.inputs(key, s)
        regs = cm.regions(s, cm.describe(lib, s))
        f32 = {}
        for variant in VARIANTS:
            mode = cm.mode_of(s, variant)
            if variant and not (s.a_planes or mode != "f32"):
                continue
            if s.a_planes or not f32:
                f32[0] = cm.torch_compose(s, d, torch.float32, variant).double()
            r = dict(key=key, harsh=s.harsh, variant=variant, mode=mode, f32=0.0, emu=0.0, **{x: 0.0 for x in cm.DEFECTS})
            wino = {}
            for b, oy, ox in regs:
                o = cm.oracle(s, d, b, oy, ox, variant)
                iy, ix = torch.as_tensor(oy), torch.as_tensor(ox)
                # torch float32 against the budget of the exact-fp32 mode (the tightest)
                r["f32"] = max(r["f32"], float(((f32[0][b][iy][:, ix] - o.ref).abs() / cm.budget(s.but(prec=0), "", o)).max()))
                if mode == "f32":
                    continue
                tol = cm.budget(s, variant, o)
                if s.wino:
                    if b not in wino:
                        wino[b] = cm.emulate_wino(s, d, b, variant)[0]
                    got = wino[b][iy][:, ix]
                else:
                    got = cm.emulate(s, d, b, oy, ox, variant)[0]
                r["emu"] = max(r["emu"], float(((got - o.ref).abs() / tol).max()))
                if s.wino or cm.gmac(s) > 0.02:
                    continue
                for x in cm.DEFECTS:
                    if (x == "replicate" and s.ks != 3) or (x == "sbias_row" and not s.sbias):
                        continue
                    r[x] = max(r[x], float(((cm.emulate(s, d, b, oy, ox, variant, defect=x)[0] - o.ref).abs() / tol).max()))
            rows.append(r)
    return rows


def test_references_alone_stay_inside_the_budget(teeth):
    worst = {w: max(teeth, key=lambda r: r[w]) for w in ("f32", "emu")}
    print({w: (round(r[w], 3), r["key"], r["variant"]) for w, r in worst.items()})
    assert all(r["f32"] <= 1.0 and r["emu"] <= 1.0 for r in teeth), worst
    assert worst["f32"]["f32"] > 0 and worst["emu"]["emu"] > 0


@pytest.mark.parametrize("defect", cm.DEFECTS)
def test_a_defective_split_leaves_the_budget(teeth, defect):
    """the a_lo * w_hi term dropped | the weights' lo piece zeroed for one tap | one border tap read with replicate padding | the per-sample
    bias row off by one: each beyond tol on an element of a benign and of a harsh case, with bf16 and with fp16 pieces"""
    for mode in ("bf16", "f16"):
        for harsh in (0, 1):
            hit = [r["key"] for r in teeth if r["mode"] == mode and r["harsh"] == harsh and r[defect] > 1.0]
            assert hit, (defect, mode, harsh)


def test_constants_equal_the_recorded_measurement():
    assert conv_error_model.constants_in_file() == conv_error_model.constants_in_module()
    assert cm.M == 4.0 and cm.UNIT == {"f32": 0.0, "bf16": 2.0 ** -18, "f16": 2.0 ** -22}
