"""Every conv plan class against the float64 oracle at its edges (-m gpu; tests/conv_matrix.py holds the cases, the oracle and the budget).

One pf_conv2d launch per case and build (libpfhip.so and libpfhip_f16.so in one process).  The plan must be the class the case was built
for; every owned output element must be within tol(e) of the oracle (plane outputs as hi + lo); out, stats_out and splitk_ws live inside
larger tensors prefilled with a sentinel bit pattern - guard rows in front and behind, ld_out - n guard columns - and every guard element
must keep it; each statistics tile must equal the float64 sums of the GPU's own output over the tile's real pixels to
(n_pix + 2) * 2^-24 * sum|x| (any summation order meets that); absmax_slot must equal max |stored value| exactly.  A case above 1 GMAC is
compared on windows (conv_matrix.regions), the rest of its output must be finite, its guards are checked in full.

Largest err / tol seen on an MI355X, per form (bf16x3 | f16x3 build; 158 cases x 2 builds in 16 s): split 0.24 | 0.14, two wave groups
0.16 | 0.08, ping-pong 0.14 | 0.09, folded upsampling 0.23 | 0.11, planes GEMM 0.16 | 0.10, Winograd 0.24 | 0.12, fp32 0.45 (its q|k|v plane
store; 0.25 on fp32 outputs)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_matrix as cm  # noqa: E402
from gpu_guard import Guarded, _dev  # noqa: E402
from polyffusion_amd import _lib  # noqa: E402

EPS = cm.EPS


def _built(variant):
    if not os.path.exists(_lib.lib_path(variant)):
        from polyffusion_amd.build import build
        build(verbose=False, variant=variant)
    return _lib.load(variant)


CASES = cm.cases(_built(""))
_oracles = {}   # the last case's oracle, shared by the two builds
_faulted = []   # the case whose launch raised: nothing more is started on the GPU after it


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def _pack(lib, s, d):
    w, n, k = d["w"].contiguous(), s.n, s.c0 + s.c1
    taps = s.ks * s.ks
    out = {}
    if s.prec == 0:
        dst = torch.zeros(lib.pf_packed_gemm_weight_floats(n, k, taps), dtype=torch.float32)
        _lib.check(lib.pf_pack_gemm_weight(w.data_ptr(), n, k, taps, dst.data_ptr()), "pack", lib)
    elif s.fold:
        dst = torch.zeros(lib.pf_packed_gemm_weight_floats(n, k, 16), dtype=torch.float32)
        _lib.check(lib.pf_pack_upfold_weight_bf16x3(w.data_ptr(), n, k, dst.data_ptr()), "pack upfold", lib)
    else:
        dst = torch.zeros(lib.pf_packed_gemm_weight_floats(n, k, taps), dtype=torch.float32)
        _lib.check(lib.pf_pack_gemm_weight_bf16x3(w.data_ptr(), n, k, taps, dst.data_ptr()), "pack bf16x3", lib)
    out["w"] = _dev(dst)
    if s.wino:
        ww = torch.zeros(lib.pf_wino_weight_bytes(n, k), dtype=torch.uint8)
        _lib.check(lib.pf_pack_wino_weight_bf16x3(w.data_ptr(), n, k, ww.data_ptr()), "pack wino", lib)
        out["w_wino"] = _dev(ww)
    if s.skip[0]:
        sk = sum(s.skip)
        dst = torch.zeros(lib.pf_packed_gemm_weight_floats(n, sk, 1), dtype=torch.float32)
        _lib.check(lib.pf_pack_gemm_weight_bf16x3(d["skip_w"].contiguous().data_ptr(), n, sk, 1, dst.data_ptr()), "pack skip", lib)
        out["skip_w"] = _dev(dst)
    return out


def _decode_qkv(s, body, variant):
    """the six planes [qh|ql|kh|kl|vTh|vTl] -> hi + lo as [B][L][3C] float64 (V^T [head][d][token] with the middle token quads of every
    16-token block swapped, csrc/conv_common.h)"""
    B, L, Cc = s.b, s.w, s.n // 3
    pl = body.reshape(-1).view(cm.x3_dtype(variant)).double().cpu().reshape(6, B * L * Cc)
    q, k = (pl[0] + pl[1]).reshape(B, L, Cc), (pl[2] + pl[3]).reshape(B, L, Cc)
    vt = (pl[4] + pl[5]).reshape(B, Cc // 64, 64, L)
    t = torch.arange(L)
    qd = (t >> 2) & 3
    pos = (t & ~15) + torch.where(qd == 1, 2, torch.where(qd == 2, 1, qd)) * 4 + (t & 3)
    v = vt[..., pos].permute(0, 3, 1, 2).reshape(B, L, Cc)
    return torch.cat([q, k, v], dim=-1).reshape(B, 1, L, 3 * Cc)


@pytest.mark.parametrize("variant", ["", "f16"])
@pytest.mark.parametrize("key,s", CASES, ids=[k for k, _ in CASES])
def test_case_against_the_oracle(key, s, variant):
    assert not _faulted, f"not run: the launch of {_faulted[0]} failed on the GPU"
    lib = _lib.load(variant)
    d = cm.inputs(key, s)
    ho, wo = cm.out_hw(s)
    M_rows, nout = s.b * ho * wo, cm.n_out(s)
    # ---- buffers
    dev = {k: _dev(v) for k, v in d.items() if k not in ("w", "skip_w", "x0" if s.a_planes else "")}
    if s.a_planes:
        hi, lo = cm.split_act(d["x0"], variant)
        dev["x0"] = _dev(torch.cat([hi.reshape(-1), lo.reshape(-1)]))
    dev.update(_pack(lib, s, d))
    if s.gnfin:   # the launch writes the rows of sc / sh itself
        dev["sc"], dev["sh"] = (torch.full((s.b * (s.c0 + s.c1) + 64,), float("nan"), device="cuda") for _ in range(2))
    ld = nout + s.ldo
    guarded = {}
    if s.out_planes:
        guarded["out_planes"] = Guarded(2 * M_rows, ld, nout, bits=16)
    if s.qkv:
        guarded["qkv"] = Guarded(6 * s.b * s.w, s.n // 3, s.n // 3, bits=16)
    # a plane store leaves fp32 `out` alone
    guarded["out"] = Guarded(1, 64, 0) if (s.out_planes or s.qkv) else Guarded(M_rows, ld, nout)
    info = cm.describe(lib, s)
    assert info is not None and cm.plan_class(info) == s.cls, (key, cm.plan_class(info))
    if s.stats:
        guarded["stats"] = Guarded(s.b * info.stats_tiles * s.n, 2, 2)
    if info.splitk_ws_bytes:
        assert info.splitk_ws_bytes % 4 == 0
        guarded["splitk_ws"] = Guarded(1, info.splitk_ws_bytes // 4, info.splitk_ws_bytes // 4)
    if s.absmax:
        dev["absmax"] = torch.zeros(64, dtype=torch.int32, device="cuda")

    def ptr(name):
        return guarded[name].ptr if name in guarded else dev[name].data_ptr()

    a = cm.conv_args(s, ptr)
    if info.splitk_ws_bytes:
        a.splitk_ws, a.splitk_ws_bytes = guarded["splitk_ws"].ptr, info.splitk_ws_bytes
    live = _lib.ConvPlanInfo()
    _lib.check(lib.pf_conv_describe(C.byref(a), C.byref(live)), "pf_conv_describe", lib)
    assert cm.plan_class(live) == s.cls and live.stats_tiles == info.stats_tiles and live.ksplit == info.ksplit
    # ---- one launch
    try:
        _lib.check(lib.pf_conv2d(C.byref(a), _lib.current_stream()), "pf_conv2d", lib)
        torch.cuda.synchronize()
    except Exception:
        _faulted.append(f"{key} [{variant or 'bf16'}]")
        raise
    # ---- guards
    for name, gb in guarded.items():
        assert gb.guards_intact(body_too=name == "out" and gb.cols == 0), f"{key}: a write outside the owned part of {name}"
    # ---- every owned element against the oracle
    if s.qkv:
        got = _decode_qkv(s, guarded["qkv"].body(), variant)
    elif s.out_planes:
        pl = guarded["out_planes"].body().reshape(-1).view(cm.x3_dtype(variant)).double().cpu().reshape(2, s.b, ho, wo, ld)
        got = (pl[0] + pl[1])[..., :nout]
    else:
        stored = guarded["out"].body().view(torch.float32).cpu().reshape(s.b, ho, wo, ld)[..., :nout]
        got = stored.double()
    okey = (key, variant if s.a_planes else "")
    if okey not in _oracles:
        _oracles.clear()
        _oracles[okey] = [(b, oy, ox, cm.oracle(s, d, b, oy, ox, variant)) for b, oy, ox in cm.regions(s, info)]
    worst = 0.0
    for b, oy, ox, o in _oracles[okey]:
        err = (got[b][torch.as_tensor(oy)][:, torch.as_tensor(ox)] - o.ref).abs()
        ratio = err / cm.budget(s, variant, o)
        worst = max(worst, float(torch.nan_to_num(ratio, nan=float("inf")).max()))
    print(f"conv_matrix {_lib.CONV_FORMS[info.form]} [{cm.mode_of(s, variant)}] {key}: err/tol {worst:.3f}")
    assert worst <= 1.0, (key, worst)
    assert bool(torch.isfinite(got).all()), key
    if s.gnfin:   # the rows the finalize wrote: the host's float64 arithmetic, to an fp32 rounding
        for name in ("sc", "sh"):
            w_ = dev[name][:d[name].numel()].cpu().double().reshape(d[name].shape)
            assert bool(((w_ - d[name].double()).abs() <= 2.0 ** -22 * d[name].double().abs() + 1e-30).all()), (key, name)
    # ---- statistics: per tile (sum, sumsq) of the stored outputs, real pixels and real channels only
    if s.stats:
        tmap = torch.from_numpy(cm.stats_tile_map(s, info).reshape(-1).astype(np.int64))
        nt = info.stats_tiles
        assert int(tmap.max()) + 1 == nt
        x = got.reshape(s.b, ho * wo, s.n)
        npix = torch.bincount(tmap, minlength=nt).double()[None, :, None]
        st = guarded["stats"].body().view(torch.float32).cpu().double().reshape(s.b, nt, s.n, 2)
        for j, v in enumerate((x, x * x)):
            want = torch.zeros(s.b, nt, s.n, dtype=torch.float64).index_add_(1, tmap, v)
            mag = torch.zeros(s.b, nt, s.n, dtype=torch.float64).index_add_(1, tmap, v.abs())
            assert bool(((st[..., j] - want).abs() <= (npix + 2) * EPS * mag).all()), (key, "sum" if j == 0 else "sumsq")
    if s.absmax:
        assert dev["absmax"][:1].view(torch.float32).item() == stored.abs().max().item(), key
        assert int(dev["absmax"][1:].abs().max()) == 0
