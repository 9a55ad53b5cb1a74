"""The recurrent-kernel matrix without a GPU (tests/rnn_matrix.py): the table reaches every branch it lists, the undefective fp32 emulator of
every kernel is inside its tolerance on every case, every listed defect, switched on in the emulator, is outside it on at least one - so
the tolerances tests/test_gpu_rnn_matrix.py holds the kernels to pass a correct kernel and reject a subtly wrong one - every benign
encoder tolerance stays at or below 1e-5, and the library refuses what it must before any launch.  The recorded constants equal
profiles/rnn_error_model.md."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import rnn_matrix as rm
from polyffusion_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = rm.cases()


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
        reached = rm.branches(s)
        assert set(s.why) <= reached, (key, set(s.why) - reached)


@pytest.mark.parametrize("kind", rm.KINDS)
def test_the_table_reaches_every_listed_branch(kind):
    reached = set()
    for key, s in rm.cases(kind):
        reached |= rm.branches(s)
    assert rm.REQUIRED[kind] <= reached, rm.REQUIRED[kind] - reached


def test_the_shapes_are_the_issue_s():
    """the sizes the table must hold, spelled out once more against the specs themselves"""
    gates = [s for _, s in rm.cases("gates")]
    assert {(s.rows, s.hidden) for s in gates} == {(1, 4), (3, 20), (9, 100), (17, 512)}
    assert {s.regime for s in gates} == {"benign", "saturated", "hbig"} and {s.t_steps for s in gates if not s.seq_len} == {1, 3}
    masked = [s for s in gates if s.seq_len]
    assert {s.seq_len for s in masked} == {1, 3, 32} and {s.reverse for s in masked} == {0, 1}
    for s in masked:
        assert rm.gates_lens(s).tolist()[:3] == [0, 1, s.seq_len]      # next to each other: one 256-thread block holds all three
    for S in (3, 32):      # step 0, a row's last step, the step equal to a row's length
        steps = {s.step for s in masked if s.seq_len == S}
        assert {0, 1, S - 1} <= steps
    sat = [(k, s) for k, s in rm.cases("gates") if s.regime == "saturated"]
    for k, s in sat:
        d = rm.inputs(k, s)
        v = d["gi"][..., :2 * s.hidden] + d["gh"][:, None, :2 * s.hidden]
        assert float(v.min()) < -88.8 and float(v.abs().max()) <= 105.0 and float(d["gi"].abs().min()) >= 30.0
    step = [s for _, s in rm.cases("step")]
    assert {s.H for s in step} == {4, 96, 512, 1024} and {s.Kx for s in step} == {0, 36, 256} and {s.R for s in step} == {1, 8, 9, 17}
    assert {(s.add2, s.ld2) for s in step} == {(0, 0), (1, 0), (1, 1)} and {s.add1 for s in step} == {0, 1}
    assert {s.regime for s in step} == {"benign", "saturated"} and rm.WX_PAD > 0
    enc = [s for _, s in rm.cases("enc")]
    assert {(s.inp, s.H, s.z, s.T, s.b) for s in enc if s.enc == "chord"} == {(36, 20, 12, 64, 9), (32, 32, 32, 1, 1), (36, 100, 33, 5, 17), (36, 512, 512, 32, 8)}
    assert sum(s.with_scale for s in enc if s.enc == "chord") == 2
    assert {(s.emb, s.H, s.z, s.C, s.b, s.with_scale) for s in enc if s.enc == "texture"} == {(20, 36, 7, 1, 1, 0), (32, 64, 16, 3, 9, 0), (256, 1024, 256, 10, 2, 1)}
    assert {(s.emb, s.Hn, s.Ht, s.z, s.S, s.b) for s in enc if s.enc == "pnotree"} == {(16, 12, 20, 8, 3, 3), (32, 36, 64, 16, 32, 3), (128, 256, 512, 512, 20, 2)}


def test_chord_decoder_rows_clear_the_gap_and_the_tie_net_ties():
    dec = rm.cases("dec")
    assert {(s.zin, s.H, s.z, s.n, s.R) for _, s in dec} == {(12, 96, 20, 5, 11), (6, 4, 3, 1, 1), (256, 512, 256, 8, 17), (2048, 1024, 2048, 2, 1)}
    for key, s in dec:
        d, o = rm.oracle(key, s)
        print(f"{key}: {d['cleared']} of {rm.DRAWN} rows clear the gap; smallest gap of the rows used {o.gap:.2e}")
        assert d["cleared"] >= 17 or (s.R == 1 and d["cleared"] >= 1), key      # fewer is a failure, not a skip
        assert d["z"].shape[0] == s.R and o.gap >= rm.GAP, key
        assert rm.dec_tol_max(s, o) < 0.1 * rm.GAP, key                          # a logit's tolerance stays below a tenth of the gap
        if s.tie:
            n = rm.dec_tied_decisions(s, d, o)
            print(f"{key}: {n} tied decisions")
            assert n >= 8 and all(a < rm.TIE_B for a in d["tied"])
            assert int(o.grid[..., rm.TIE_B].sum()) == 0 and int(o.grid[..., 24 + rm.TIE_B].sum()) == 0      # the lower index wins
            assert int(o.grid[..., 12].sum()) == 0                                                           # a tied bit is 0


def test_pianotree_decoder_rows_clear_the_gap_lengths_and_ties():
    """the counts of rows that clear the 1e-3 gap in float64 (PCG64(404) rows, seed-0 weights) are the ones the matrix was designed on"""
    pn = dict(rm.cases("pn"))
    assert {(s.HD, s.R, s.eos, s.tie) for s in pn.values()} == {(16, 17, 0, 0), (64, 17, 0, 0), (16, 9, 50, 0), (64, 9, -50, 0), (16, 9, 0, 1), (64, 9, 0, 2)}
    want = {"dec pnotree S4 HD16 R17": (22, 48), "dec pnotree S4 HD64 R17": (23, 48), "dec pnotree S4 HD16 R9 eos+50": (24, 24),
            "dec pnotree S4 HD64 R9 eos-50": (15, 24)}
    for key, s in pn.items():
        d, o = rm.oracle(key, s)
        print(f"{key}: {d['cleared']} of {d['drawn']} rows clear the gap; smallest gap of the rows used {o.gap:.2e}")
        assert d["cleared"] >= (17 if s.R == 17 else 9), key                     # fewer is a failure, not a skip
        if key in want:
            assert (d["cleared"], d["drawn"]) == want[key], key
        assert d["z"].shape[0] == s.R and o.gap >= rm.GAP, key
        assert rm.pn_tol_max(s, o) < 0.1 * rm.GAP, key
        lens = set(o.lens.flatten().tolist())
        assert lens == ({1} if s.eos > 0 else {rm.PN_S - 1} if s.eos < 0 else {1, 2, 3}), (key, lens)
        assert np.array_equal(rm.pn_lengths(o.grid), o.lens.numpy()), key        # the first end token fixes the length; none: S - 1
        if s.tie:
            if s.tie == 1:
                (a1, b1), (a2, b2) = d["pairs"]
                assert b1 % 64 == a1 % 64 and b2 % 64 != a2 % 64
            n = rm.pn_tied_decisions(s, d, o)
            print(f"{key}: pairs {d['pairs']} tied decisions {n}")
            assert min(n) >= 8, n


def test_pianotree_grids_hold_the_lengths_and_pads_the_issue_names():
    for key, s in rm.cases("enc"):
        if s.enc != "pnotree":
            continue
        g = rm.inputs(key, s)["x"]
        pad = g[..., 0] == rm.PN_P
        lens = s.S - pad.sum(-1)
        assert lens[0].tolist() == [(0, 1, s.S)[t % 3] for t in range(32)], key
        notes_after_pad = (pad[1, :, :-1] & ~pad[1, :, 1:]).any()
        assert bool(notes_after_pad), key
        pitches = g[..., 0][~pad]
        assert int(pitches.min()) == 0 and int(pitches.max()) == rm.PN_P - 1, key
        assert bool((g[..., 1:][pad] == 2).all()) and bool((g[..., 1:][~pad] <= 1).all())
    for key, s in rm.cases("enc"):
        if s.enc == "texture" and s.b >= 2:
            x = rm.inputs(key, s)["x"]
            assert float(x[0].abs().max()) == 0.0 and float(x[1].min()) >= 1.0


@pytest.mark.parametrize("key,s", ALL, ids=[k for k, _ in ALL])
def test_the_emulated_kernel_is_inside_the_tolerance(key, s):
    r = rm.emulated_ratio(key, s)
    assert r <= 1.0, (key, r)
    if s.kind == "enc":     # float32 noise is below 1e-6: a tolerance above 1e-5 would mean the unit is wrong
        _, o = rm.oracle(key, s)
        assert float(rm.enc_tol(s, o)[0].max()) <= 1e-5, key


@pytest.mark.parametrize("kind,defect", [(k, df) for k in rm.KINDS for df in rm.DEFECTS[k]])
def test_every_defect_is_caught(kind, defect):
    caught = next((key for key, s in rm.cases(kind) if rm.defect_applies(s, defect) and rm.emulated_ratio(key, s, defect) > 1.0), None)
    assert caught, f"{kind}: no case rejects the defect '{defect}'"
    print(f"{kind} {defect}: rejected first by {caught}")


def test_the_defects_the_matrix_must_hold():
    have = {df for k in rm.KINDS for df in rm.DEFECTS[k]}
    assert {"rz_swapped", "bhh_outside", "masked_reverse_S", "masked_step_le", "dir1_into_half0", "pad_column", "ld2_ignored",
            "argmax_tie_high", "bit_tie_1", "last_eos", "L_unclamped"} <= have


def test_every_refusal_is_answered_before_any_launch(lib):
    for name, args in rm.refused_gates():
        assert lib.pf_gru_gates(*args, 0) == -1, name
        assert lib.pf_last_error(), name
    for name, fields in rm.refused_step():
        a = _lib.GruStepArgs(**fields)
        assert lib.pf_gru_step(C.byref(a), 0) == -1, name
        assert lib.pf_last_error(), name
    assert lib.pf_gru_step(None, 0) == -1
    for name, args in rm.REFUSED_ENCODERS:
        h = C.c_void_p()
        assert lib.pf_encoder_create_dist(*args, C.byref(h)) == -1 and not h.value, name
        assert b"1024" in lib.pf_last_error(), name
    h = C.c_void_p()
    assert lib.pf_encoder_create_dist(0, 36, 0, 1024, 64, 0, 1, C.byref(h)) == 0 and h.value      # the largest the mat-vec takes
    lib.pf_encoder_destroy(h)
    for hidden in (1028, 6):
        assert lib.pf_decoder_create(0, 0, 36, 256, hidden, 256, 8, C.byref(h)) == -1, hidden


def test_header_declares_and_both_builds_export_the_entry_points(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "pfhip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pf_[a-z0-9_]+)\s*\(", hdr))
    if not os.path.exists(_lib.lib_path("f16")):
        from polyffusion_amd.build import build
        build(verbose=False, variant="f16")
    for name in ("pf_gru_gates", "pf_gru_step"):
        assert name in declared and name in _lib.SIGNATURES
        assert hasattr(lib, name) and hasattr(_lib.load("f16"), name)
    assert "pf_gru_step_args" in hdr and C.sizeof(_lib.GruStepArgs) == 104


def test_the_recorded_constants_are_the_profile_s_and_what_the_table_measures():
    """profiles/rnn_error_model.md holds what tools/rnn_error_model.py measured; rnn_matrix.MEASURED equals it and the table's maximum"""
    sys.path.insert(0, REPO)
    from tools import rnn_error_model as tool
    text = open(tool.OUT).read()
    worst = {k: 0.0 for k in tool.SUBS}
    for key, s in ALL:
        worst[rm.sub_of(s)] = max(worst[rm.sub_of(s)], rm.measured_ratio(key, s))
    for sub in tool.SUBS:
        row = re.search(r"\| %s \| ([0-9.]+) \|" % re.escape(tool.NAMES[sub]), text)
        assert row is not None and float(row.group(1)) == rm.MEASURED[sub], sub
        assert tool.up2(worst[sub]) == rm.MEASURED[sub], (sub, worst[sub])
    assert "python tools/rnn_error_model.py" in text
    assert rm.M == {k: rm.MARGIN * v for k, v in rm.MEASURED.items()} and rm.MARGIN == 4.0 and torch.float64
