"""The small-kernel matrix without a GPU (tests/small_matrix.py): the table reaches every branch it lists, every float64 oracle agrees with
torch's own double statement of the operation, the undefective fp32 emulator of every kernel is inside its tolerance on every case, and
every listed defect, switched on in the emulator, is outside it on at least one - so the tolerances tests/test_gpu_small_matrix.py holds
the kernels to pass a correct kernel and reject a subtly wrong one.  The recorded constants equal profiles/small_error_model.md."""
import os
import re
import sys

import pytest
import torch

import small_matrix as sm
from polyffusion_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = sm.cases()
_inputs = {}


def inputs(key, s):
    if key not in _inputs:
        _inputs[key] = sm.inputs(key, s)
    return _inputs[key]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from polyffusion_amd.build import build
        build(verbose=False)
    return _lib.load()


def test_keys_are_unique_and_every_case_says_why_it_exists():
    keys = [k for k, _ in ALL]
    assert len(keys) == len(set(keys))
    for key, s in ALL:
        assert s.why, key
        reached = sm.BRANCHES[s.kind](s)
        assert set(s.why) <= reached, (key, set(s.why) - reached)


@pytest.mark.parametrize("kind", sm.KINDS)
def test_the_table_reaches_every_listed_branch(kind):
    reached, named = set(), set()
    for key, s in sm.cases(kind):
        reached |= sm.BRANCHES[kind](s)
        named |= set(s.why)
    assert sm.REQUIRED[kind] <= reached, sm.REQUIRED[kind] - reached
    assert named <= reached


def test_the_shapes_are_the_issue_s():
    """the sizes the table must hold, spelled out once more against the specs themselves"""
    gn = [s for _, s in sm.cases("gn") if s.entry == "data"]
    assert {s.hw for s in gn} >= {15, 255, 256, 257, 600, 64 * 256 + 37}
    assert {(s.c0, s.c1, s.groups) for s in gn} >= {(4, 0, 1), (4, 0, 4), (32, 0, 32), (96, 0, 32), (256, 128, 32), (64, 32, 32), (1024, 0, 32)}
    assert any(s.hw == 64 * 256 + 37 and (s.b, s.c0, s.c1) == (1, 32, 0) for s in gn)
    for entry in ("data", "tiles"):
        assert {(s.regime, ) for _, s in sm.cases("gn") if s.entry == entry} == {(r,) for r in sm.GN_REGIMES}
        assert {s.eps for _, s in sm.cases("gn") if s.entry == entry} == {1e-5, 1e-6}
    tiles = [s for _, s in sm.cases("gn") if s.entry == "tiles"]
    assert {(s.t0, s.t1) for s in tiles if s.c1} == {(1, 5), (1, 9)} and any(s.c1 == 0 for s in tiles)
    ln = [s for _, s in sm.cases("ln")]
    assert {s.c for s in ln if s.entry == "stats"} == set(sm.LN_C) and {s.c for s in ln if s.entry == "planes"} == set(sm.LN_C) - {2048}
    assert {s.rows for s in ln} == {1, 3, 4, 5}
    stem = [s for _, s in sm.cases("stem")]
    assert {(s.cin, s.cout) for s in stem} == {(1, 64), (2, 64), (2, 32), (3, 64), (4, 128)}
    assert {(s.h, s.w) for s in stem} == set(sm.STEM_HW) and {s.b for s in stem} == {1, 3}
    head = [s for _, s in sm.cases("head")]
    assert {(s.cin, s.cout) for s in head} >= {(ci, co) for ci in (16, 32, 48) for co in (1, 2, 3, 4)}
    assert {(s.h, s.w) for s in head} == set(sm.HEAD_HW) and {s.b for s in head} == {1, 3}
    assert any(sm.head_oracle(s, inputs(k, s)).vmax >= 100.0 for k, s in sm.cases("head") if s.regime == "extreme")
    tm = [s for _, s in sm.cases("time")]
    assert {(s.channels, s.d_t) for s in tm} == {(32, 128), (64, 256), (320, 1280)} and any(s.table and s.batch == 1000 for s in tm)
    mv = [s for _, s in sm.cases("mv")]
    assert {s.b for s in mv} == {1, 7, 8, 9, 17} and {s.n for s in mv} == {1, 31, 32, 33, 100} and {s.k for s in mv} == {32, 256, 288, 2048, 20, 36}
    assert {s.npg for s in mv} == {0, 32, 48} and any(s.exp for s in mv) and any(not s.bias for s in mv)


@pytest.mark.parametrize("key,s", ALL, ids=[k for k, _ in ALL])
def test_the_oracle_agrees_with_torch_double(key, s):
    d = inputs(key, s)
    if s.kind == "gn":
        o = sm.gn_oracle(s, d)
        x = sm._gn_x(s, d).double()
        got, want = x * o.scale[:, None, :] + o.shift[:, None, :], sm.gn_torch(s, d)
        scale = (x.abs() * o.scale[:, None, :].abs() + o.shift[:, None, :].abs()).max()
    elif s.kind == "ln":
        got, want = sm.ln_oracle(s, d).y, sm.ln_torch(s, d)
        scale = sm.ln_oracle(s, d).t.abs().max() + 1
        if s.regime == "const":     # torch's own double mean of a constant row is off by an ulp of double, times rstd = 316
            scale = scale + 1e3 * d["x"].abs().max().double()
    elif s.kind == "stem":
        o = sm.stem_oracle(s, d)
        got, want, scale = o.ref, sm.stem_torch(s, d), o.T.max()
    elif s.kind == "head":
        o = sm.head_oracle(s, d)
        got, want, scale = o.ref, sm.head_torch(s, d), o.T.max() + 1
    elif s.kind == "time":
        got, want, scale = sm.time_oracle(s, d).ref, sm.time_torch(s, d), 1.0
    else:
        o = sm.mv_oracle(s, d)
        got, want, scale = o.ref, sm.mv_torch(s, d), o.ref.abs().max() + o.T.max()
    assert got.shape == want.shape and got.dtype == torch.float64
    assert float((got - want).abs().max()) <= 1e-12 * float(scale), key


@pytest.mark.parametrize("key,s", ALL, ids=[k for k, _ in ALL])
def test_the_emulated_kernel_is_inside_the_tolerance(key, s):
    r = sm.emulated_ratio(key, s, inputs(key, s))
    assert r <= 1.0, (key, r)


@pytest.mark.parametrize("kind,defect", [(k, df) for k in sm.KINDS for df in sm.DEFECTS[k]])
def test_every_defect_is_caught(kind, defect):
    caught = [key for key, s in sm.cases(kind) if sm.emulated_ratio(key, s, inputs(key, s), defect) > 1.0]
    assert caught, f"{kind}: no case rejects the defect '{defect}'"
    print(f"{kind} {defect}: rejected by {len(caught)} case(s), first {caught[0]}")


def test_every_refusal_is_answered_before_any_launch(lib):
    for name, fn, args in sm.refused():
        assert getattr(lib, fn)(*args) == -1, name
        assert lib.pf_last_error(), name
    assert lib.pf_conv_in_stats_tiles(2, 64, 17, 33) == 6 and lib.pf_conv_in_stats_tiles(1, 64, 1, 1) == 1
    assert lib.pf_conv_in_stats_tiles(3, 64, 16, 16) == 0 and lib.pf_conv_in_stats_tiles(2, 32, 16, 16) == 0


def test_header_declares_and_both_builds_export_the_entry_points(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "pfhip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pf_[a-z0-9_]+)\s*\(", hdr))
    if not os.path.exists(_lib.lib_path("f16")):
        from polyffusion_amd.build import build
        build(verbose=False, variant="f16")
    for name in ("pf_conv_in", "pf_conv_in_stats_tiles", "pf_conv_out", "pf_time_embed", "pf_matvec"):
        assert name in declared and name in _lib.SIGNATURES
        assert hasattr(lib, name) and hasattr(_lib.load("f16"), name)


def test_the_recorded_constants_are_the_profile_s_and_what_the_table_measures():
    """profiles/small_error_model.md holds what tools/small_error_model.py measured; small_matrix.MEASURED equals it and the table's maximum"""
    sys.path.insert(0, REPO)
    from tools import small_error_model as tool
    text = open(tool.OUT).read()
    for kind in sm.KINDS:
        row = re.search(r"\| %s \| ([0-9.]+) \|" % re.escape(tool.NAMES[kind]), text)
        assert row is not None and float(row.group(1)) == sm.MEASURED[kind], kind
        worst = max(sm.measured_ratio(key, s, inputs(key, s)) for key, s in sm.cases(kind))
        assert tool.up2(worst) == sm.MEASURED[kind], (kind, worst)
    assert "GroupNorm envelope" in text and "passes 1e-4" in text
    assert sm.M == {k: sm.MARGIN * v for k, v in sm.MEASURED.items()} and sm.MARGIN == 4.0
