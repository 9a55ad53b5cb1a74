"""Every attention form against the float64 oracle at its edges (-m gpu; tests/attn_matrix.py holds the cases, the oracle and the budget).

One launch per case; the split kernels (pf_attention_bf16x3, pf_attention_bf16x3_split) run on both builds (libpfhip.so and libpfhip_f16.so
in one process), the fp32 kernels (pf_attention, pf_attention_wide) once.  The inputs of the split kernels are planes written by the host
encoder of attn_matrix (not by the library's own q | k | v GEMM), the oracle sees their hi + lo.  Every owned output element must be finite
and within tol(e) of the oracle (plane outputs as hi + lo); out, o_planes and the scratch of the split and wide forms live inside larger
tensors prefilled with a sentinel bit pattern - guard rows in front and behind, ldo - C guard columns, the scratch exactly as large as the
*_scratch_bytes query said - and every guard element must keep it.  Bit-equal: the auto form and the forced form it should have picked, a
split-entry launch that does not split (the shape, too little scratch) and form 0, a second run of every launch and the first.

Largest err / tol seen on an MI355X, every head of every case compared, per entry point and form (bf16x3 | f16x3 build; 46 cases, 71
launches checked, 83 tests in 8 s): pf_attention_bf16x3 128-query 0.27 | 0.13 (equal scores with plane output | the 376-workgroup auto case),
256-query 0.21 | 0.18 (the 192-workgroup auto case); pf_attention_bf16x3_split split 0.21 | 0.09 (keys at 100 in the last slice | the steep
ramp at L = 1024), not splitting 0.07 | 0.15; pf_attention 0.16 (lk = 77, extremes in the first tile); pf_attention_wide 0.37 (L = 1024,
d = 16, a late dominating key).  No case failed: the matrix found nothing to fix in the kernels or the launchers."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_matrix as am  # noqa: E402
import conv_matrix as cm  # noqa: E402
from gpu_guard import Guarded, _dev  # noqa: E402
from polyffusion_amd import _lib  # noqa: E402


def _built(variant):
    if not os.path.exists(_lib.lib_path(variant)):
        from polyffusion_amd.build import build
        build(verbose=False, variant=variant)
    return _lib.load(variant)


_built("")
CASES = [(k, s, v) for k, s in am.cases() for v in (("", "f16") if s.ep in (am.X3, am.SPLIT) else ("",))]
_faulted = []   # the case whose launch raised: nothing more is started on the GPU after it


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _device_inputs(s, d, variant):
    """the launch's input buffers: name -> device tensor (kept alive by the caller)"""
    B, Cc = s.b, am.channels(s)
    if s.ep in (am.X3, am.SPLIT):
        return {"planes": _dev(am.encode_planes(d, variant)[0])}
    q, k, v = d["q"].reshape(B * s.lq, Cc), d["k"].reshape(B * s.lk, Cc), d["v"].reshape(B * s.lk, Cc)
    if s.ep == am.ATTN and s.cross:   # q in a buffer of its own, k | v in [B lk][2C]: the cross-attention launches of the UNet plan
        return {"q": _dev(q), "kv": _dev(torch.cat([k, v], dim=1))}
    return {"qkv": _dev(torch.cat([q, k, v], dim=1))}   # [B L][3C]


def _launch(lib, s, dev, key):
    """fresh guarded outputs, one launch, a synchronize -> (guarded buffers, the names whose whole body must stay untouched)"""
    B, H, L, Cc = s.b, s.h, s.lq, am.channels(s)
    st = _lib.current_stream()
    g, untouched = {}, set()
    if s.planes:
        g["o_planes"] = Guarded(2 * B * L, Cc, Cc, bits=16)
        g["out"] = Guarded(1, 64, 0)   # a plane store leaves fp32 `out` alone
        untouched.add("out")
    else:
        g["out"] = Guarded(B * L, Cc + s.ldo, Cc)
    ldo = Cc + (0 if s.planes else s.ldo)
    op = g["o_planes"].ptr if s.planes else None
    if s.ep == am.ATTN:
        if s.cross:
            qp, kp, ldq, ldk = dev["q"].data_ptr(), dev["kv"].data_ptr(), Cc, 2 * Cc
            vp = kp + 4 * Cc
        else:
            qp, ldq, ldk = dev["qkv"].data_ptr(), 3 * Cc, 3 * Cc
            kp, vp = qp + 4 * Cc, qp + 8 * Cc
        call = lambda: lib.pf_attention(qp, ldq, kp, ldk, vp, ldk, g["out"].ptr, ldo, B, H, s.dh, s.lq, s.lk, st)   # noqa: E731
    elif s.ep == am.WIDE:
        need = int(lib.pf_attention_wide_scratch_bytes(B, L))
        assert need == 4 * am.scratch_floats(s) and need % 4 == 0
        g["scratch"] = Guarded(1, need // 4, need // 4)
        qp = dev["qkv"].data_ptr()
        call = lambda: lib.pf_attention_wide(qp, qp + 4 * Cc, qp + 8 * Cc, 3 * Cc, g["out"].ptr, ldo, B, L, s.dh, g["scratch"].ptr, need, st)   # noqa: E731
    elif s.ep == am.X3:
        call = lambda: lib.pf_attention_bf16x3(dev["planes"].data_ptr(), g["out"].ptr, ldo, op, B, H, L, s.form, st)   # noqa: E731
    else:
        need = int(lib.pf_attention_split_scratch_bytes(B, H, L))
        assert need % 4 == 0 and (need > 0) == (s.scratch != "none"), key
        if s.scratch == "full":
            assert need > 0, key
        given = need if s.scratch == "full" else need - 4 if s.scratch == "short" else 256
        g["scratch"] = Guarded(1, given // 4, given // 4)
        if s.scratch != "full":
            untouched.add("scratch")
        call = lambda: lib.pf_attention_bf16x3_split(dev["planes"].data_ptr(), g["out"].ptr, ldo, op, B, H, L, g["scratch"].ptr, given, st)   # noqa: E731
    assert not _faulted, f"not run: the launch of {_faulted[0]} failed on the GPU"
    try:
        _lib.check(call(), s.ep, lib)
        torch.cuda.synchronize()
    except Exception:
        _faulted.append(key)
        raise
    return g, untouched


def _owned(s, g):
    """the owned output bits, on the host"""
    if s.planes:
        return g["o_planes"].body().cpu()
    return g["out"].body()[:, :am.channels(s)].cpu()


def _values(s, owned, variant):
    """owned bits -> float64 [B][lq][H][dh] (planes as hi + lo)"""
    if s.planes:
        pl = owned.reshape(-1).view(am.x3_dtype(variant)).double().reshape(2, s.b, s.lq, s.h, s.dh)
        return pl[0] + pl[1]
    return owned.contiguous().view(torch.float32).double().reshape(s.b, s.lq, s.h, s.dh)


@pytest.mark.parametrize("key,s,variant", CASES, ids=[f"{k} [{v or 'bf16'}]" if s.ep in (am.X3, am.SPLIT) else k for k, s, v in CASES])
def test_case_against_the_oracle(key, s, variant):
    assert not _faulted, f"not run: the launch of {_faulted[0]} failed on the GPU"
    lib = _built(variant)
    cus = _cus()
    d = am.inputs(key, s)
    dev = _device_inputs(s, d, variant)
    tag = f"{key} [{am.mode_of(s, variant)}]"
    g, untouched = _launch(lib, s, dev, tag)
    # ---- guards
    for name, gb in g.items():
        assert gb.guards_intact(body_too=name in untouched), f"{key}: a write outside the owned part of {name}"
    owned = _owned(s, g)
    # ---- every owned element against the oracle
    got = _values(s, owned, variant)
    x = am.plane_inputs(am.encode_planes(d, variant)[1]) if "planes" in dev else {n: d[n].double() for n in "qkv"}
    worst = 0.0
    for b, h in am.heads(s, sample=False):   # every head: every owned element is compared
        o = am.oracle(x["q"][b, :, h], x["k"][b, :, h], x["v"][b, :, h], am.scale_of(s))
        ratio = (got[b, :, h] - o.ref).abs() / am.budget(s, variant, o)
        worst = max(worst, float(torch.nan_to_num(ratio, nan=float("inf")).max()))
    print(f"attn_matrix {am.form_of(s, cus)} [{am.mode_of(s, variant)}] {key}: err/tol {worst:.3f}")
    assert worst <= 1.0, (key, worst)
    assert bool(torch.isfinite(got).all()), key
    # ---- bit-equality: a second run; the forced form an auto / non-splitting launch stands for
    g2, _ = _launch(lib, s, dev, tag + " (second run)")
    assert torch.equal(_owned(s, g2), owned), f"{key}: two runs differ"
    assert all(gb.guards_intact(body_too=name in untouched) for name, gb in g2.items()), key
    partner = am.bit_equal_partner(s, cus)
    if partner is not None:
        g3, _ = _launch(lib, partner, dev, tag + " (forced form)")
        assert torch.equal(_owned(partner, g3), owned), f"{key}: differs from {am.key_of(partner)}"
    if s.ep == am.SPLIT and s.scratch == "full":
        assert am.form_of(s, cus) == "split", key


def test_auto_cases_lie_on_both_sides_of_the_threshold_of_this_part():
    cus = _cus()
    auto = [s for _, s in am.cases() if s.ep == am.X3 and s.form < 0]
    assert {am.form_of(s, cus) for s in auto} == {"q128", "q256"}, cus
    lib = _built("")
    for _, s in am.cases():   # the split threshold: every case that is to split does on this part
        if s.ep == am.SPLIT:
            assert int(lib.pf_attention_split_scratch_bytes(s.b, s.h, s.lq)) == 4 * am.scratch_floats(s), am.key_of(s)


@pytest.mark.parametrize("variant", ["", "f16"])
def test_qkv_planes_gemm_writes_the_encoders_planes(variant):
    """producer / consumer layout: the library's q | k | v planes GEMM (pf_conv2d with qkv_planes) on an identity weight and an input that
    is exactly hi + lo must write, bit for bit, the planes the host encoder writes - a layout error shared by the GEMM and the attention
    kernels would cancel in a test that feeds one to the other, here it cannot"""
    assert not _faulted, f"not run: the launch of {_faulted[0]} failed on the GPU"
    lib = _built(variant)
    B, L, H = 2, 144, 2
    Cc = H * 64
    gen = torch.Generator().manual_seed(7)
    hi, lo = am.split_pieces(torch.randn(B, L, H, 64, generator=gen) * 1.5 + 0.3, variant)
    x = hi.float() + lo.float()   # exact: two pieces of 8 (11) bits, the lo one below half an ulp of the hi one
    assert torch.equal(x.double(), hi.double() + lo.double())
    want, _ = am.encode_planes(dict(q=x, k=x, v=x), variant)
    s = cm._lin(1, b=B, w=L, c0=Cc, n=3 * Cc, qkv=1)
    assert cm.describe(lib, s) is not None
    w = torch.eye(Cc).repeat(3, 1).contiguous()   # [3C][C]: q = k = v = x
    wp = torch.zeros(lib.pf_packed_gemm_weight_floats(3 * Cc, Cc, 1), dtype=torch.float32)
    _lib.check(lib.pf_pack_gemm_weight_bf16x3(w.data_ptr(), 3 * Cc, Cc, 1, wp.data_ptr()), "pack", lib)
    dev = {"x0": _dev(x), "w": _dev(wp)}
    g = {"qkv": Guarded(6 * B * L, Cc, Cc, bits=16), "out": Guarded(1, 64, 0)}
    a = cm.conv_args(s, lambda name: g[name].ptr if name in g else dev[name].data_ptr())
    try:
        _lib.check(lib.pf_conv2d(C.byref(a), _lib.current_stream()), "pf_conv2d", lib)
        torch.cuda.synchronize()
    except Exception:
        _faulted.append(f"qkv planes GEMM [{variant or 'bf16'}]")
        raise
    assert g["qkv"].guards_intact() and g["out"].guards_intact(body_too=True)
    got = g["qkv"].body().reshape(-1).cpu()
    assert torch.equal(got, want.view(torch.int16)), int((got != want.view(torch.int16)).sum())


def _zeros(n, dtype=torch.float32):
    return torch.zeros(n, dtype=dtype, device="cuda")


# (name, entry point, arguments the launcher must refuse); the buffers below are large enough for the launch the arguments describe
REFUSALS = ("x3 L=192", "x3 form 1 at L=384", "attn d_head=48", "attn ldq=66", "attn ldk=6", "attn ldo=66", "wide l=1088", "wide d=24",
            "wide scratch one float short")


@pytest.mark.parametrize("what", REFUSALS)
def test_refused_launch_writes_nothing(what):
    """each call must return < 0 with a message and leave every guard AND every body intact; the buffers hold what a launch that wrongly
    went ahead with these arguments would touch"""
    assert not _faulted, f"not run: the launch of {_faulted[0]} failed on the GPU"
    lib = _built("")
    st = _lib.current_stream()
    # a refusal of another kind first, so that the message read below is this call's and not one left by an earlier test
    assert lib.pf_attention(None, 4, None, 4, None, 4, None, 4, 1, 1, 32, 1, 1, st) < 0
    before = lib.pf_last_error().decode("utf-8", "replace")
    assert "null argument" in before
    if what.startswith("x3"):
        L, form = (192, 0) if "192" in what else (384, 1)
        planes = _zeros(6 * 512 * 64, am.x3_dtype(""))   # a launch would walk whole 64-key tiles and 128 / 256-query workgroups: below 512 rows
        g = {"out": Guarded(512, 64, 64)}
        rc = lib.pf_attention_bf16x3(planes.data_ptr(), g["out"].ptr, 64, None, 1, 1, L, form, st)
    elif what.startswith("attn"):
        dh, ldq, ldk, ldo = (48, 64, 64, 64) if "48" in what else (32, 66, 64, 64) if "ldq" in what else (32, 64, 6, 64) if "ldk" in what else (32, 64, 64, 66)
        q, k, v = (_zeros(128 * 72) for _ in range(3))
        g = {"out": Guarded(128, 72, 72)}
        rc = lib.pf_attention(q.data_ptr(), ldq, k.data_ptr(), ldk, v.data_ptr(), ldk, g["out"].ptr, ldo, 1, 1, dh, 64, 64, st)
    else:
        l, d = (1088, 16) if "1088" in what else (64, 24) if "24" in what else (64, 16)
        qkv = _zeros(l * 3 * 32)
        g = {"out": Guarded(l, 32, 32), "scratch": Guarded(1, l * l, l * l)}
        nbytes = 4 * l * l - (4 if "short" in what else 0)
        if "short" in what:
            assert nbytes + 4 == int(lib.pf_attention_wide_scratch_bytes(1, l))
        rc = lib.pf_attention_wide(qkv.data_ptr(), qkv.data_ptr() + 4 * d, qkv.data_ptr() + 8 * d, 3 * d, g["out"].ptr, d, 1, l, d, g["scratch"].ptr, nbytes, st)
    msg = lib.pf_last_error().decode("utf-8", "replace")
    torch.cuda.synchronize()
    names = "attention_bf3:" if what.startswith("x3") else "attention:" if what.startswith("attn") else "attention_wide:"
    assert rc < 0 and msg != before and msg.startswith(names), (what, rc, msg)
    for name, gb in g.items():
        assert gb.guards_intact(body_too=True), f"{what}: {name} was written"
