"""The attention case matrix on a machine without a GPU (-m "not gpu"; tests/attn_matrix.py): it reaches every launch path of the four
attention entry points with the edges the kernels have; its plane encoder round-trips through a decoder written on its own; its float64
oracle equals a plain torch composition; and its error budget has teeth - the float64 emulation of attention_bf3.hip's documented arithmetic
with one defect at a time leaves it, the unbroken emulation (within tol / M) and torch float32 stay inside on every case."""
import os

import pytest
import torch

import attn_matrix as am
from polyffusion_amd import _lib
from tools import attn_error_model

VARIANTS = ("", "f16")
TEETH_REGIMES = ("ramp", "late", "slices")


def _lib_of(variant):
    if not os.path.exists(_lib.lib_path(variant)):
        from polyffusion_amd.build import build
        build(verbose=False, variant=variant)
    return _lib.load(variant)


@pytest.fixture(scope="module")
def matrix():
    return am.cases()


def test_matrix_reaches_every_launch_path_with_its_edges(matrix):
    specs = [s for _, s in matrix]
    assert len({k for k, _ in matrix}) == len(matrix)
    # (entry point, form, split?, output kind, grid-size class, ldo padded?): complete both ways - no path drops out, a new one is registered
    paths = {am.path_of(s) for s in specs}
    assert paths == set(am.REQUIRED_PATHS), (sorted(set(am.REQUIRED_PATHS) - paths), sorted(paths - set(am.REQUIRED_PATHS)))

    def vals(ep, name, **where):
        return {s[name] for s in specs if s.ep == ep and all(s[k] == v for k, v in where.items())}

    assert vals(am.ATTN, "lq") >= {1, 127, 128, 129, 200} and vals(am.ATTN, "lk") >= {1, 4, 63, 64, 65, 77, 129}
    assert vals(am.ATTN, "dh") == {32, 64} and vals(am.ATTN, "h") >= {1, 3, 4} and vals(am.ATTN, "b") >= {1, 3}
    assert vals(am.ATTN, "cross") == {0, 1} and vals(am.ATTN, "ldo", cross=0) == vals(am.ATTN, "ldo", cross=1) == {0, 8}
    assert any(s.ep == am.ATTN and s.cross and s.lk == 1 for s in specs)           # the model's one condition token
    assert all(s.lq == s.lk for s in specs if not (s.ep == am.ATTN and s.cross))
    assert vals(am.X3, "lq", form=0) >= {128, 384, 512} and vals(am.X3, "lq", form=1) >= {256, 512, 768}
    assert vals(am.X3, "h", form=0) >= {1, 3, 4} and vals(am.X3, "h", form=1) >= {1, 3, 4}
    assert {am.grid_class(am.grid_of(s)) for s in specs if s.ep == am.X3 and s.form == 0} == {"1", "<8", "8k+r", "8k"}
    assert any(am.grid_of(s) == 9 for s in specs if s.ep == am.X3 and s.form == 0) and any(am.grid_of(s) == 9 for s in specs if s.ep == am.X3 and s.form == 1)
    auto = [s for s in specs if s.ep == am.X3 and s.form < 0]
    assert {am.form_of(s) for s in auto} == {"q128", "q256"} and all(am.bit_equal_partner(s).form == (am.form_of(s) == "q256") for s in auto)
    # the lazy exponent of the 256-query form: a ramp below 2^TAU per tile and one above
    assert vals(am.X3, "rate", form=1, regime="ramp") >= {"slow", "fast"}
    split = [s for s in specs if s.ep == am.SPLIT]
    assert {(s.b, s.h, s.lq) for s in split if am.splits(s)} >= {(1, 1, 512), (2, 3, 512), (1, 1, 1024)}
    assert {s.scratch for s in split} == {"full", "none", "short"} and {s.planes for s in split if am.splits(s)} == {0, 1}
    lib = _lib_of("")   # the launcher's own answer (256 compute units without a device, as on the part the list is laid out for)
    for s in split:
        need = int(lib.pf_attention_split_scratch_bytes(s.b, s.h, s.lq))
        assert need == 4 * am.scratch_floats(s) and (need > 0) == (s.scratch != "none"), am.key_of(s)
        assert am.bit_equal_partner(s) is None if am.splits(s) else am.form_of(am.bit_equal_partner(s)) == "q128"
    assert any(s.regime == "slices" for s in split if am.splits(s))
    assert vals(am.WIDE, "lq") >= {64, 128, 1024} and vals(am.WIDE, "dh") >= {16, 32, 48, 256} and vals(am.WIDE, "b") >= {1, 3}
    assert vals(am.WIDE, "ldo") == {0, 8} and {(s.b, s.dh) for s in specs if s.ep == am.WIDE and s.lq == 1024} == {(1, 16)}
    for ep in (am.ATTN, am.X3, am.WIDE):
        assert vals(ep, "regime") >= {"gauss", "ramp", "late", "first", "flat"}, ep
    assert all(s.regime != "slices" or s.ep == am.SPLIT for s in specs) and {s.regime for s in specs} == set(am.REGIMES)


def _decode(planes, B, H, L, variant):
    """written apart from am.encode_planes, by index arithmetic: the six planes -> hi + lo of q, k, v as [B][L][H][64] float64"""
    Cc = H * 64
    pl = planes.double().reshape(6, B * L * Cc)
    q, k = ((pl[i] + pl[i + 1]).reshape(B, L, H, 64) for i in (0, 2))
    vt = (pl[4] + pl[5]).reshape(B, H, 64, L)
    t = torch.arange(L)
    quad = (t >> 2) & 3
    pos = (t & ~15) + torch.where(quad == 1, 2, torch.where(quad == 2, 1, quad)) * 4 + (t & 3)   # where token t is stored
    return q, k, vt[..., pos].permute(0, 3, 1, 2)


@pytest.mark.parametrize("variant", VARIANTS)
def test_plane_encoder_round_trips_through_its_own_decoder(matrix, variant):
    n = 0
    for key, s in matrix:
        if s.ep not in (am.X3, am.SPLIT) or s.b > 3:
            continue
        d = am.inputs(key, s)
        planes, pc = am.encode_planes(d, variant)
        assert planes.dtype == _lib.x3_torch_dtype(variant) and planes.numel() == 6 * s.b * s.lq * am.channels(s)
        want = am.plane_inputs(pc)
        for name, got in zip("qkv", _decode(planes, s.b, s.h, s.lq, variant)):
            assert torch.equal(got, want[name]), (key, name)
            # hi + lo carries the input to the pair's precision (the fp16 pair: a subnormal lo piece)
            rel, ab = (2.0 ** -21, 2.0 ** -25) if variant == "f16" else (2.0 ** -16, 0.0)
            assert bool(((got - d[name].double()).abs() <= rel * d[name].double().abs() + ab).all()), (key, name)
        n += 1
    assert n > 15
    # the swap itself, on a ramp of token numbers: the two middle quads of every 16-token block change places
    v = torch.arange(32, dtype=torch.float32).reshape(1, 32, 1, 1).expand(1, 32, 1, 64).contiguous()
    planes, _ = am.encode_planes(dict(q=v, k=v, v=v), variant)
    row = planes.float().reshape(6, -1)[4][:32].tolist()
    assert row == [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15, 16, 17, 18, 19, 24, 25, 26, 27, 20, 21, 22, 23, 28, 29, 30, 31]


@pytest.fixture(scope="module")
def teeth(matrix):
    """per case, build and compared head: the largest err / tol of torch float32 (against the f32 budget), of the unbroken emulation, and
    on the ramp / late / slices regimes of every defect; the oracle against torch float64"""
    rows = []
    for key, s in matrix:
        d = am.inputs(key, s)
        for variant in VARIANTS:
            mode = am.mode_of(s, variant)
            if variant and mode == "f32":
                continue
            x, pc = attn_error_model.head_inputs(s, d, variant)
            r = dict(key=key, s=s, mode=mode, form=am.form_of(s), f32=0.0, f64=0.0, emu=0.0, **{dn: 0.0 for dn in am.DEFECTS})
            for b, h in am.heads(s):
                q, k, v = (x[n][b, :, h] for n in "qkv")
                o = am.oracle(q, k, v, am.scale_of(s))
                r["f64"] = max(r["f64"], float((am.torch_compose(q, k, v, am.scale_of(s), torch.float64) - o.ref).abs().max()) / max(float(o.ref.abs().max()), 1e-300))
                f32 = am.torch_compose(q, k, v, am.scale_of(s), torch.float32).double()
                r["f32"] = max(r["f32"], float(((f32 - o.ref).abs() / am.budget(s.but(ep=am.ATTN, planes=0), "", o)).max()))
                if mode == "f32":
                    continue
                tol = am.budget(s, variant, o)
                r["emu"] = max(r["emu"], float(((am.emulate(pc, b, h, variant, r["form"]) - o.ref).abs() / tol).max()))
                if s.regime not in TEETH_REGIMES:
                    continue
                for dn in am.DEFECTS:
                    if dn == "merge_m0" and r["form"] != "split":
                        continue
                    ratio = (am.emulate(pc, b, h, variant, r["form"], defect=dn) - o.ref).abs() / tol
                    r[dn] = max(r[dn], float(torch.nan_to_num(ratio, nan=float("inf")).max()))
            rows.append(r)
    return rows


def test_oracle_equals_the_torch_composition_in_float64(teeth):
    assert all(r["f64"] <= 1e-12 for r in teeth), max(teeth, key=lambda r: r["f64"])


def test_references_alone_stay_inside_the_budget(teeth):
    """torch float32 within the f32 budget of every case; the emulation within tol / M of every case in both builds"""
    worst = {w: max(teeth, key=lambda r: r[w]) for w in ("f32", "emu")}
    print({w: (round(r[w], 3), r["key"], r["mode"]) for w, r in worst.items()})
    assert all(r["f32"] <= 1.0 for r in teeth), worst["f32"]
    assert all(r["emu"] <= 1.0 / am.M for r in teeth), worst["emu"]
    assert worst["f32"]["f32"] > 0 and worst["emu"]["emu"] > 0
    assert {r["form"] for r in teeth if r["mode"] != "f32"} == {"q128", "q256", "split"}


@pytest.mark.parametrize("defect", am.DEFECTS)
def test_a_defective_kernel_leaves_the_budget(teeth, defect):
    """the k_lo.q_hi product left out | no lo piece of the probabilities | a row sum that misses its largest rescale | a merge relative to
    slice 0's maximum: each beyond tol on every one of the ramp, late and slices regimes, with bf16 and with fp16 pieces, in every form the
    regime runs in.  A merge relative to slice 0's maximum is the SAME sum in exact arithmetic - it differs from the correct one only where
    exp2f(m_s - m_0) leaves fp32's range, that is where a later slice's maximum lies more than 88 (natural units) above slice 0's.  The
    inputs of the split form are sharpened to have that on every regime: `slices` (+120), the L = 1024 ramp (rate "steep": +96) and `late`
    (rate "far": keys at 100).  What stays out is stated, not loosened: the slow ramp at L = 512 (+12 over its six tiles) cannot leave
    fp32's range, there the emulation cannot separate this defect from the correct arithmetic, and neither could a kernel's result."""
    forms = ("split",) if defect == "merge_m0" else ("q128", "q256", "split")
    for mode in ("bf16", "f16"):
        for regime in TEETH_REGIMES:
            for form in forms:
                rows = [r for r in teeth if r["mode"] == mode and r["s"].regime == regime and r["form"] == form]
                if defect == "merge_m0":
                    rows = [r for r in rows if r["s"].rate != "slow"]
                if not rows:
                    assert (regime, form) == ("slices", "q256"), (regime, form)   # `slices` is a regime of the split entry point (q128 when it does not split)
                    continue
                missed = [(r["key"], round(r[defect], 3)) for r in rows if not r[defect] > 1.0]
                assert not missed, (defect, mode, regime, form, missed)


def test_constants_equal_the_recorded_measurement():
    assert attn_error_model.constants_in_file() == attn_error_model.constants_in_module()
    assert am.M == 4.0 and am.UNIT == {"f32": 0.0, "bf16": 2.0 ** -18, "f16": 2.0 ** -22}
