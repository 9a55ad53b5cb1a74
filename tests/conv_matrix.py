"""The conv case matrix: one small, edge-seeking set of pf_conv2d argument sets that reaches every plan class of tests/golden/conv_plans.json
(a class = form, tile_h, tile_w, tile_n, wave_groups, K split granted), a float64 oracle of the whole launch (prologue, conv, skip
projection, epilogue), a float64 emulation of the documented operand split, and the per-element error budget both GPU builds are held to.
Used by tests/test_conv_matrix.py (no GPU), tests/test_gpu_conv_matrix.py (-m gpu) and tools/conv_error_model.py (measures the constants).

The budget of output element e (before a GeGLU or a plane store, which propagate it - see budget()):

    tol(e) = M * [ M_ACC * sqrt(K) * 2^-24 * T(e) + M_SPLIT[mode] * split_scale(mode, e) ] + 4 * 2^-24 * R(e)

T(e) = sqrt(sum (a*w)^2) over every product that feeds e (the fused skip projection's included), a = the activation AFTER the prologue,
K = the number of those products, R = |ref| + |bias| + |sbias| + |res|.  split_scale = u * T with u the unit roundoff include/pfhip.h
documents (0 / 2^-18 / 2^-22); the fp16 build adds the floor its subnormal lo pieces leave: 2^-25 * ||w||_2 (activation lo pieces below
2^-14 are quantised to 2^-24) + 2^-33 * ||a||_2 (the same for the lo pieces of the weights, stored times 2^8).  M_ACC and M_SPLIT are NOT taken
from the kernels: tools/conv_error_model.py measures them on the CPU over this matrix (torch float32 against the oracle; the emulated split
against the oracle) and writes them to profiles/conv_error_model.md; the constants below equal that file's.  M = 4 covers what neither
reference does: the MFMA's blocked accumulation order with three products per k, K-split partial sums added by a reduce kernel, __expf and
the hardware reciprocal in the prologue (a few ulp each)."""
from __future__ import annotations

import ctypes as C
import json
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from polyffusion_amd import _lib
from tools import conv_plan_table as cpt

P = cpt.P
EPS = 2.0 ** -24
UNIT = {"f32": 0.0, "bf16": 2.0 ** -18, "f16": 2.0 ** -22}
M = 4.0
# measured by tools/conv_error_model.py, recorded in profiles/conv_error_model.md (rounded up to two digits)
M_ACC = 3.17
M_SPLIT = {"bf16": 7.72, "f16": 1.97, "fold_bf16": 10.11, "fold_f16": 2.76, "wino_bf16": 32.65, "wino_f16": 6.58}

BIG_GMAC = 1.0      # above this a case is checked on windows; only BIG_CLASSES may hold such a case
CHEAP_GMAC = 0.05   # below this the oracle is compared with the torch composition on the CPU
SB_NROWS = 5        # rows of the hoisted per-sample bias table of the sbias_rows cases
GN_TILES = (3, 4)   # producer tiles per sample of the fused GroupNorm finalize cases (source 0, source 1)
GN_EPS, GN_GROUPS = 1e-5, 32
F32, SPLIT, KG2, PINGPONG, UPFOLD, PLANES, WINO = range(7)
# the classes whose cheapest member is large (fp32 8x16x64 / 8x16x128, split 16x16x64, upfold 8x16x64 / 8x16x128; the fp32 1x128x64 base found here is cheap)
BIG_CLASSES = {(F32, 8, 16, 64, 1, False), (F32, 1, 128, 64, 1, False), (F32, 8, 16, 128, 1, False), (SPLIT, 16, 16, 64, 1, False),
               (UPFOLD, 8, 16, 64, 1, False), (UPFOLD, 8, 16, 128, 1, False)}


class Spec(dict):
    __getattr__ = dict.__getitem__

    def but(self, **kw):
        s = Spec(self)
        s.update(kw)
        return s


DEFAULT = Spec(prec=1, b=1, h=1, w=16, c0=64, c1=0, n=64, ks=3, stride=1, ups=0, fold=0, pro=0, pad_br=0, wino=0, a_planes=0, out_planes=0,
               qkv=0, geglu=0, bias=0, sbias=0, res=0, ldo=0, stats=0, skip=(0, 0), gnfin=0, bmod=0, absmax=0, ft=0, fk=0, no_pp=0, no_t16=0,
               harsh=0)


def cdiv(a, b):
    return -(-a // b)


def out_hw(s):
    h, w = s.h, s.w
    if s.ups:
        h, w = 2 * h, 2 * w
    if s.stride == 2:
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return h, w


def n_out(s):
    return s.n // 2 if s.geglu else s.n


def k_products(s):
    return s.ks * s.ks * (s.c0 + s.c1) + sum(s.skip)


def gmac(s):
    ho, wo = out_hw(s)
    return s.b * ho * wo * s.n * k_products(s) / 1e9


def key_of(s):
    k = f"{'fs'[s.prec]}{s.ks} B{s.b} {s.h}x{s.w} {s.c0}+{s.c1}>{s.n}"
    for name, v in s.items():
        if name in ("prec", "ks", "b", "h", "w", "c0", "c1", "n") or v == DEFAULT[name]:
            continue
        k += f" {name}" if v == 1 else f" {name}{v[0]}+{v[1]}" if name == "skip" else f" {name}{v}"
    return k


def conv_args(s, ptr=lambda name: P) -> _lib.ConvArgs:
    """pf_conv_args of a spec; `ptr(name)` gives the address of the named buffer (a placeholder by default: pf_conv_describe reads none)"""
    a = _lib.ConvArgs()
    a.x0, a.c0 = ptr("x0"), s.c0
    if s.c1:
        a.x1, a.c1 = ptr("x1"), s.c1
    a.batch, a.hin, a.win, a.ks, a.stride, a.ups = s.b, s.h, s.w, s.ks, s.stride, s.ups
    a.w, a.n, a.prologue, a.precision = ptr("w"), s.n, s.pro, s.prec
    if s.pro:
        a.sc, a.sh = ptr("sc"), ptr("sh")
    if s.pro == 3:
        a.mean, a.rstd = ptr("mean"), ptr("rstd")
    if s.bias:
        a.bias = ptr("bias")
    if s.sbias:
        a.sbias, a.ld_sbias = ptr("sbias"), s.n + 8
    if s.sbias == 2:
        a.sbias_rows, a.sbias_nrows = ptr("sbias_rows"), SB_NROWS
    if s.res:
        a.res, a.ld_res = ptr("res"), s.n + 8
    a.geglu = s.geglu
    a.out, a.ld_out = ptr("out"), n_out(s) + s.ldo
    if s.stats:
        a.stats_out = ptr("stats")
    a.a_planes = s.a_planes
    if s.out_planes:
        a.out_planes = ptr("out_planes")
    if s.qkv:
        a.qkv_planes = ptr("qkv")
    a.ups_fold = s.fold
    if s.skip[0]:
        a.skip_x0, a.skip_c0, a.skip_w, a.skip_bias = ptr("skip_x0"), s.skip[0], ptr("skip_w"), ptr("skip_bias")
    if s.skip[1]:
        a.skip_x1, a.skip_c1 = ptr("skip_x1"), s.skip[1]
    if s.gnfin:
        a.gn_stats0, a.gn_tiles0, a.gn_gamma, a.gn_beta, a.gn_eps, a.gn_groups = ptr("gn_stats0"), GN_TILES[0], ptr("gn_gamma"), ptr("gn_beta"), GN_EPS, GN_GROUPS
        if s.c1:
            a.gn_stats1, a.gn_tiles1 = ptr("gn_stats1"), GN_TILES[1]
    a.no_t16, a.no_pp, a.force_tile, a.force_ksplit, a.x1_bmod, a.pad_mode = s.no_t16, s.no_pp, s.ft, s.fk, s.bmod, s.pad_br
    if s.wino:
        a.w_wino, a.wino = ptr("w_wino"), 1
    if s.absmax:
        a.absmax_slot = ptr("absmax")
    return a


def describe(lib, s, a=None):
    """the plan of a spec with the K-split scratch it asks for attached (None: refused)"""
    a = conv_args(s) if a is None else a
    info = _lib.ConvPlanInfo()
    if lib.pf_conv_describe(C.byref(a), C.byref(info)) != 0:
        return None
    if info.splitk_ws_bytes and not a.splitk_ws:
        a.splitk_ws, a.splitk_ws_bytes = P, info.splitk_ws_bytes
        assert lib.pf_conv_describe(C.byref(a), C.byref(info)) == 0
    return info


def plan_class(info):
    return (info.form, info.tile_h, info.tile_w, info.tile_n, info.wave_groups, info.ksplit > 1)


def recorded_classes():
    with open(cpt.GOLDEN) as f:
        return sorted({(r[0], r[1], r[2], r[3], r[4], r[6] > 1) for r in json.load(f).values()})


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def _g(**kw):
    return DEFAULT.but(**kw)


def _lin(prec, **kw):   # rows of a matrix
    return _g(prec=prec, ks=1, h=1, **kw)


def _families():
    """plan class -> geometry variants, the first the cheapest member found (searched by hand over conv_plan.hip's rules, held to the class
    by cases() through pf_conv_describe); the edges a class admits: ragged pixels, N in {32, 96, 160}, a second source, odd K chunk counts,
    B in {1, 3}, stride 2 on odd / even sizes, bottom-right padding, upsampling through the halo read and folded."""
    fam = {}
    for prec, form in ((0, F32), (1, SPLIT)):
        fam[(form, 1, 64, 64, 1, False)] = [_lin(prec, w=100), _lin(prec, b=3, w=7, c0=32, n=160, pro=3), _lin(prec, w=200, c1=32, n=96, pro=2),
                                            _lin(prec, w=64, c0=96, n=32), _lin(prec, b=3, w=20, c0=256, c1=128, n=64, pro=2)]
        # 128 px x 64 ch: 512 row tiles (two per CU) and fewer than 512 workgroups of the 128-channel tile
        fam[(form, 1, 128, 64, 1, False)] = [_lin(prec, b=4, w=16384, c0=32, n=32), _lin(prec, b=4, w=16300, c0=32, c1=32, n=32, pro=2),
                                             _lin(prec, b=1, w=21900, c0=32, n=160, pro=3), _lin(prec, b=3, w=21800, c0=96, n=64)]
        fam[(form, 1, 128, 128, 1, False)] = [_lin(prec, w=100, n=128, geglu=1, pro=3), _lin(prec, b=3, w=7, c0=96, n=64, geglu=1),
                                              _lin(prec, w=200, c1=32, n=192, geglu=1, pro=2), _lin(prec, w=128, c0=32, n=320, geglu=1, pro=3),
                                              _lin(prec, b=4, w=16384, c0=32, n=128), _lin(prec, b=4, w=16300, c0=32, n=96, pro=2)]   # without GeGLU: 512 workgroups
    fam[(F32, 4, 16, 64, 1, False)] = [_g(prec=0, h=16, pro=1), _g(prec=0, b=3, h=12, w=20, c1=32, n=96, pro=1), _g(prec=0, h=10, w=18, c0=32, n=32, stride=2),
                                       _g(prec=0, h=9, w=11, c1=32, stride=2), _g(prec=0, h=10, w=18, n=160, stride=2, pad_br=1),
                                       _g(prec=0, b=3, h=5, w=10, c0=96, n=32, ups=1), _g(prec=0, h=20, w=20, c0=96, pro=1)]
    fam[(F32, 8, 16, 64, 1, False)] = [_g(prec=0, h=256, w=256, c0=32, n=32, pro=1), _g(prec=0, h=250, w=250, c0=32, c1=32, n=32, pro=1),
                                       _g(prec=0, h=125, w=128, c0=32, n=64, ups=1)]
    fam[(F32, 8, 16, 128, 1, False)] = [_g(prec=0, h=256, w=256, c0=32, n=96, pro=1), _g(prec=0, h=250, w=250, c0=32, n=128, pro=1),
                                        _g(prec=0, h=250, w=256, c0=32, c1=32, n=128, pro=1)]
    # split 3x3 on the 64 px tile, one wave group: strided, upsampling, or an odd number of K chunks
    fam[(SPLIT, 4, 16, 64, 1, False)] = [_g(h=16, c0=96, pro=1), _g(b=3, h=12, w=20, c1=32, n=96, pro=1), _g(h=10, w=18, c0=32, n=32, stride=2),
                                         _g(h=9, w=11, c1=32, stride=2), _g(h=10, w=18, n=160, stride=2, pad_br=1), _g(b=3, h=5, w=10, n=32, ups=1),
                                         _g(h=8, w=8, c0=32, c1=32, ups=1), _g(h=20, w=20, c0=96, pro=1)]
    fam[(SPLIT, 4, 16, 64, 1, True)] = [_g(h=8, w=8, pro=1, fk=2), _g(b=3, h=16, c1=64, n=96, pro=1, fk=2), _g(h=8, w=24, c0=128, n=32, pro=1, fk=4),
                                        _g(h=2, w=32, pro=1, fk=2), _g(h=4, w=8, ups=1, fk=2), _g(h=8, w=8, c0=96, n=160, pro=1, fk=3)]
    fam[(SPLIT, 8, 16, 64, 1, False)] = [_g(h=16, pro=1, ft=2), _g(b=3, h=12, w=20, c1=32, n=96, pro=1, ft=2), _g(h=10, w=18, c0=96, n=32, pro=1, ft=2),
                                         _g(h=20, w=20, c0=32, n=160, pro=1, ft=2), _g(h=5, w=10, c0=128, pro=1, ft=2)]
    fam[(SPLIT, 8, 16, 64, 1, True)] = [_g(h=16, pro=1, ft=2, fk=2), _g(b=3, h=8, w=24, c1=64, n=96, pro=1, ft=2, fk=2),
                                        _g(h=4, w=16, c0=128, n=32, pro=1, ft=2, fk=4), _g(h=8, w=8, c0=96, n=160, pro=1, ft=2, fk=3)]
    fam[(SPLIT, 8, 16, 128, 1, False)] = [_g(h=16, n=128, pro=1, ft=1), _g(b=3, h=12, w=20, c1=32, n=96, pro=1, ft=1), _g(h=10, w=18, c0=96, n=128, pro=1, ft=1),
                                          _g(h=16, c0=256, n=128, pro=1, ft=1, no_pp=1), _g(h=20, w=20, c0=32, n=96, pro=1, ft=1)]
    fam[(SPLIT, 8, 16, 128, 1, True)] = [_g(h=16, n=128, pro=1, ft=1, fk=2), _g(b=3, h=8, w=24, c1=64, n=96, pro=1, ft=1, fk=2),
                                         _g(h=4, w=16, c0=128, n=128, pro=1, ft=1, fk=4), _g(h=8, w=8, c0=96, n=96, pro=1, ft=1, fk=3)]
    # the 16x16-pixel tile: 1024 tiles of a launch with 64 padded channels and at least 128 input channels
    fam[(SPLIT, 16, 16, 64, 1, False)] = [_g(h=512, w=512, c0=128, n=32, pro=1), _g(b=2, h=256, w=512, c1=64, n=64, pro=1)]
    fam[(KG2, 4, 16, 64, 2, False)] = [_g(h=4, w=4, pro=1), _g(b=3, h=12, w=20, c1=64, n=96, pro=1), _g(h=10, w=18, c0=128, n=32, pro=1),
                                       _g(h=5, w=10, n=160, pro=1), _g(h=20, w=20, pro=1), _g(h=16, c0=256, c1=128, pro=1)]
    fam[(PINGPONG, 8, 16, 128, 2, False)] = [_g(h=8, c0=256, n=128, pro=1, ft=1), _g(b=3, h=12, w=20, c0=256, c1=128, n=96, pro=1, ft=1),
                                             _g(h=10, w=18, c0=256, n=128, pro=1, ft=1), _g(h=20, w=20, c0=192, c1=64, n=96, pro=1, ft=1)]
    fam[(UPFOLD, 4, 16, 64, 1, False)] = [_g(h=8, w=8, ups=1, fold=1), _g(b=3, h=5, w=10, c0=32, n=96, ups=1, fold=1), _g(h=6, w=9, c1=32, n=32, ups=1, fold=1),
                                          _g(h=10, w=10, c0=96, n=160, ups=1, fold=1)]
    fam[(UPFOLD, 8, 16, 64, 1, False)] = [_g(h=128, w=128, c0=32, n=32, ups=1, fold=1), _g(h=125, w=125, c0=32, c1=32, n=64, ups=1, fold=1)]
    fam[(UPFOLD, 8, 16, 128, 1, False)] = [_g(h=64, w=128, c0=32, n=96, ups=1, fold=1), _g(h=61, w=125, c0=32, n=128, ups=1, fold=1),
                                          _g(h=64, w=125, c0=32, c1=32, n=128, ups=1, fold=1)]
    fam[(PLANES, 1, 64, 64, 1, False)] = [_lin(1, w=100, a_planes=1), _lin(1, b=3, w=7, c0=32, n=160, a_planes=1), _lin(1, w=200, c0=96, n=96, a_planes=1),
                                          _lin(1, w=64, c0=256, n=32, a_planes=1)]
    fam[(PLANES, 1, 128, 64, 1, False)] = [_lin(1, w=100, a_planes=1, ft=2), _lin(1, b=3, w=7, c0=32, n=160, a_planes=1, ft=2),
                                           _lin(1, w=200, c0=96, n=96, a_planes=1, ft=2), _lin(1, w=300, c0=256, n=32, a_planes=1, ft=2)]
    fam[(PLANES, 1, 128, 128, 1, False)] = [_lin(1, w=100, n=128, a_planes=1, ft=1), _lin(1, b=3, w=7, c0=32, n=128, a_planes=1, geglu=1),
                                            _lin(1, w=200, c0=96, n=96, a_planes=1, ft=1), _lin(1, w=300, c0=256, n=192, a_planes=1, geglu=1)]
    fam[(WINO, 16, 16, 64, 1, False)] = [_g(h=16, c0=32, pro=1, wino=1), _g(b=3, h=16, w=32, c1=32, n=128, pro=1, wino=1), _g(h=32, w=16, c0=96, pro=1, wino=1),
                                         _g(h=16, c0=256, c1=128, pro=1, wino=1)]
    return fam


OPTIONS = ("bias", "sbias", "sbias_rows", "res", "ldo", "stats", "skip1", "skip2", "gnfin", "bmod", "geglu", "out_planes", "qkv", "absmax",
           "pro0", "pro1", "pro2", "pro3")
# option bundles dealt round the variants of a class (an option a variant does not admit is left out); cases() then adds what is still missing
BUNDLES = (("bias", "res", "ldo", "stats"), ("sbias", "ldo", "absmax"), ("sbias_rows", "res", "stats", "bmod"), ("skip1", "bias", "stats", "ldo"),
           ("skip2", "sbias_rows", "bmod", "absmax"), ("gnfin", "res", "stats"), ("out_planes", "bias", "ldo"), ("bias", "sbias", "res", "stats", "ldo", "absmax"))


def has_option(s, opt):
    return {"bias": s.bias, "sbias": s.sbias == 1, "sbias_rows": s.sbias == 2, "res": s.res, "ldo": s.ldo, "stats": s.stats,
            "skip1": s.skip[0] and not s.skip[1], "skip2": s.skip[1], "gnfin": s.gnfin, "bmod": s.bmod, "geglu": s.geglu,
            "out_planes": s.out_planes, "qkv": s.qkv, "absmax": s.absmax}.get(opt, s.pro == int(opt[-1]) if opt.startswith("pro") else 0) != 0


def with_option(s, opt, tile_n=64):
    if has_option(s, opt):
        return s
    if opt == "ldo":
        return s.but(ldo=4 if s.wino else 8)
    if opt in ("bias", "res", "stats", "gnfin", "geglu", "out_planes"):
        return s.but(**{opt: 1})
    if opt == "absmax":   # exact only where the stored values can be read back: fp32 outputs
        return None if s.out_planes or s.qkv else s.but(absmax=1)
    if opt in ("sbias", "sbias_rows"):
        return s.but(sbias=1 if opt == "sbias" else 2)
    if opt in ("skip1", "skip2"):
        return s.but(skip=(64, 0) if opt == "skip1" else (32, 32))
    if opt == "bmod":
        return s.but(bmod=2, b=max(s.b, 3)) if (s.c1 or s.skip[1]) and gmac(s.but(b=max(s.b, 3))) <= 0.3 else None
    if opt == "qkv":
        return s.but(qkv=1, n=384 if tile_n == 128 else 192, w=cdiv(s.w, 16) * 16, absmax=0)
    return s.but(pro=int(opt[-1]))


def cases(lib=None):
    """[(key, spec)] in a fixed order; spec.cls is the plan class the case was built for.  Needs a built library (no device)."""
    lib = lib or _lib.load("")
    out, seen = [], set()
    for cls, variants in _families().items():
        limit = 32.0 if cls in BIG_CLASSES else 0.3

        def admit(s):
            if s is None or gmac(s) > limit:
                return False
            info = describe(lib, s)
            return info is not None and plan_class(info) == cls

        assert admit(variants[0]), (cls, key_of(variants[0]))
        members = []
        for i, v in enumerate(variants):
            if not admit(v):
                continue
            for opt in BUNDLES[(i + len(out)) % len(BUNDLES)]:
                t = with_option(v, opt, cls[3])
                if admit(t):
                    v = t
            members.append(v)
        for opt in OPTIONS:   # every option the class admits appears in it at least once
            if any(has_option(m, opt) for m in members):
                continue
            for v in variants + members:
                t = with_option(v, opt, cls[3])
                if t is not v and admit(t):
                    members.append(t)
                    break
        for i, m in enumerate(members):
            m = m.but(harsh=i % 2)
            k = key_of(m)
            if k not in seen:
                seen.add(k)
                out.append((k, m.but(cls=cls)))
    return out


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def x3_dtype(variant):
    return torch.float16 if variant == "f16" else torch.bfloat16


def split_act(x32, variant):
    """hi, lo pieces of fp32 activations, rounded to nearest (what the kernels' operand split and a producer's plane store do)"""
    dt = x3_dtype(variant)
    hi = x32.to(dt)
    return hi, (x32 - hi.float()).to(dt)


def split_weight(w32, variant):
    """(hi, lo, scale): the pieces split_hi_lo (csrc/conv_plan.hip) stores - in the fp16 build of the weight times 2^8, clamped to fp16's range"""
    if variant == "f16":
        vs = (w32 * 256.0).clamp(-65504.0, 65504.0)
        hi = vs.to(torch.float16)
        return hi, (vs - hi.float()).to(torch.float16), 256.0
    hi = w32.to(torch.bfloat16)
    return hi, (w32 - hi.float()).to(torch.bfloat16), 1.0


def inputs(key, s):
    """seeded host tensors (fp32, NHWC) of a case.  benign: the distribution of the per-op GPU tests; harsh: per-channel scales exp(2 N(0,1))
    (clipped at +-2.5 sigma: the fp16 build's range) on the activations and, independently, on the weights' input channels.  sc / sh and
    mean / rstd are plain inputs - the conv is tested alone; the fused GroupNorm finalize's statistics are made from the data."""
    rng = np.random.Generator(np.random.PCG64(zlib.crc32(key.encode())))

    def g(*shape, scale=1.0):
        return torch.from_numpy(rng.standard_normal(shape).astype(np.float32) * np.float32(scale))

    def chan(c, sigma):
        return torch.from_numpy(np.exp(sigma * np.clip(rng.standard_normal(c), -2.5, 2.5)).astype(np.float32)) if s.harsh else torch.ones(c)

    cin, B, B1 = s.c0 + s.c1, s.b, s.bmod or s.b
    ho, wo = out_hw(s)
    d = {}
    sa = chan(cin, 2.0)                      # activation scale per input channel
    d["x0"] = (g(B, s.h, s.w, s.c0) * 1.5 + 0.3) * sa[:s.c0]
    if s.c1:
        d["x1"] = (g(B1, s.h, s.w, s.c1) * 1.5 + 0.3) * sa[s.c0:]
    taps = s.ks * s.ks
    sw = chan(cin, 2.0)
    w = g(s.n, cin, s.ks, s.ks) * sw[None, :, None, None] * chan(s.n, 1.0)[:, None, None, None]
    d["w"] = w / float(np.sqrt(taps * float((sw * sw).sum())))
    if s.pro in (1, 2) and not s.gnfin:
        t = chan(cin, 1.0)
        d["sc"] = (1 + 0.1 * g(B, cin)) * (t / sa / 1.5)
        d["sh"] = (0.1 * g(B, cin) - 0.2) * t
    if s.pro == 3:
        t = chan(cin, 1.0)
        d["sc"], d["sh"] = (1 + 0.1 * g(cin)) * (t / sa), 0.1 * g(cin) * t
        d["mean"], d["rstd"] = 0.3 + 0.1 * g(B * s.h * s.w), (1 + 0.1 * g(B * s.h * s.w)).abs() / 1.5
    if s.gnfin:
        d["gn_gamma"], d["gn_beta"] = 1 + 0.1 * g(cin), 0.1 * g(cin)

        def tile_stats(x, nt):   # any split of the pixels into nt parts is a valid producer layout
            parts = x.double().reshape(x.shape[0], -1, x.shape[-1]).tensor_split(nt, dim=1)
            return torch.stack([torch.stack([p.sum(1), (p * p).sum(1)], dim=-1) for p in parts], dim=1).float().contiguous()

        d["gn_stats0"] = tile_stats(d["x0"], GN_TILES[0])
        if s.c1:
            d["gn_stats1"] = tile_stats(d["x1"], GN_TILES[1])
        d["sc"], d["sh"] = gn_finalize(s, d)
    if s.bias:
        d["bias"] = 0.1 * g(s.n)
    if s.sbias:
        d["sbias"] = g(SB_NROWS if s.sbias == 2 else B, s.n + 8)
    if s.sbias == 2:   # below 0, at / above the table's end (both clamped), inside
        d["sbias_rows"] = torch.tensor([(-1, SB_NROWS + 2, 2, SB_NROWS, 0)[(i + len(key)) % 5] for i in range(B)], dtype=torch.int64)
    if s.res:
        d["res"] = g(B, ho, wo, s.n + 8)
    if s.skip[0]:
        sk = sum(s.skip)
        d["skip_x0"] = g(B, ho, wo, s.skip[0])
        if s.skip[1]:
            d["skip_x1"] = g(B1, ho, wo, s.skip[1])
        d["skip_w"], d["skip_bias"] = g(s.n, sk, scale=sk ** -0.5), 0.1 * g(s.n)
    return d


def gn_finalize(s, d):
    """scale / shift rows the fused finalize writes (csrc/conv_common.h gn_fused_prologue): fp32 tile statistics added in float64, rounded to fp32"""
    B, cin = s.b, s.c0 + s.c1
    tot = d["gn_stats0"].double().sum(1)
    if s.c1:
        t1 = d["gn_stats1"].double().sum(1)
        tot = torch.cat([tot, t1[torch.arange(B) % t1.shape[0]]], dim=1)
    gs = cin // GN_GROUPS
    grp = tot.reshape(B, GN_GROUPS, gs, 2).sum(2)
    cnt = gs * s.h * s.w
    mean = grp[..., 0] / cnt
    rstd = 1.0 / torch.sqrt((grp[..., 1] / cnt - mean * mean).clamp_min(0.0) + GN_EPS)
    mean, rstd = mean.repeat_interleave(gs, 1), rstd.repeat_interleave(gs, 1)
    ga, be = d["gn_gamma"].double(), d["gn_beta"].double()
    return (rstd * ga).float(), (be - mean * rstd * ga).float()


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
def _source(s, d, b, variant):
    """(x of sample b as [H][W][cin] float64, or its (hi, lo) planes for a_planes)"""
    if s.a_planes:
        hi, lo = split_act(d["x0"][b], variant)
        return hi.double() + lo.double(), (hi, lo)
    x = d["x0"][b].double()
    if s.c1:
        x = torch.cat([x, d["x1"][b % d["x1"].shape[0]].double()], dim=-1)
    return x, None


def _prologue(s, d, a, b, ox):
    """a: gathered raw inputs [ny][nx][cin] float64 of sample b -> the activation the contraction sees"""
    if s.pro == 0:
        return a
    if s.pro == 3:
        rows = b * s.w + torch.as_tensor(ox)
        return (a - d["mean"].double()[rows][None, :, None]) * d["rstd"].double()[rows][None, :, None] * d["sc"].double() + d["sh"].double()
    y = a * d["sc"][b].double() + d["sh"][b].double()
    return y * torch.sigmoid(y) if s.pro == 1 else y


def _gather(s, d, src, b, oy, ox, ky, kx, replicate=False):
    """activation (after the prologue, zero where the tap reads padding) and validity mask of tap (ky, kx) at output pixels oy x ox"""
    up = 2 if s.ups else 1
    off = 0 if (s.ks == 1 or s.pad_br) else 1
    uy, ux = np.asarray(oy) * s.stride + ky - off, np.asarray(ox) * s.stride + kx - off
    vy, vx = (uy >= 0) & (uy < s.h * up), (ux >= 0) & (ux < s.w * up)
    iy, ix = np.clip(uy, 0, s.h * up - 1) // up, np.clip(ux, 0, s.w * up - 1) // up
    a = _prologue(s, d, src[torch.as_tensor(iy)][:, torch.as_tensor(ix)], b, ix)
    mask = torch.ones(len(uy), len(ux), dtype=torch.float64) if replicate else torch.as_tensor(vy[:, None] & vx[None, :]).double()
    return a * mask[..., None], mask


def _skip_source(s, d, b, oy, ox):
    x = d["skip_x0"][b]
    if s.skip[1]:
        x = torch.cat([x, d["skip_x1"][b % d["skip_x1"].shape[0]]], dim=-1)
    return x[torch.as_tensor(oy)][:, torch.as_tensor(ox)].double()


def sbias_row(s, d, b, shift=0):
    r = b
    if s.sbias == 2:
        r = min(max(int(d["sbias_rows"][b]), 0), SB_NROWS - 1)
    return (r + shift) % d["sbias"].shape[0]


def epilogue(s, d, b, oy, ox, acc, row_shift=0):
    """acc [ny][nx][n] float64 -> (stored values [ny][nx][n_out], R = |v| + |bias| + |sbias| + |res| per linear output)"""
    v = acc.clone()
    r = torch.zeros_like(acc)
    for name in ("bias", "skip_bias"):
        if name in d:
            v += d[name].double()
            r += d[name].double().abs()
    if s.sbias:
        sb = d["sbias"][sbias_row(s, d, b, row_shift), :s.n].double()
        v += sb
        r += sb.abs()
    if s.res:
        rs = d["res"][b][torch.as_tensor(oy)][:, torch.as_tensor(ox)][..., :s.n].double()
        v += rs
        r += rs.abs()
    r += v.abs()
    if s.geglu:   # value / gate rows alternate in blocks of 32 packed columns
        vg = v.reshape(*v.shape[:-1], s.n // 64, 2, 32)
        val, gate = vg[..., 0, :], vg[..., 1, :]
        return (val * 0.5 * gate * (1.0 + torch.special.erf(gate / math.sqrt(2.0)))).reshape(*v.shape[:-1], s.n // 2), r, v
    return v, r, v


class Result(dict):
    __getattr__ = dict.__getitem__


def oracle(s, d, b, oy, ox, variant=""):
    """float64 result of the launch at output pixels oy x ox of sample b, with the sums the error budget needs (`variant` matters to a_planes only)"""
    src, _ = _source(s, d, b, variant)
    ny, nx = len(oy), len(ox)
    acc = torch.zeros(ny * nx, s.n, dtype=torch.float64)
    t2, w2, a2 = torch.zeros_like(acc), torch.zeros_like(acc), torch.zeros(ny * nx, 1, dtype=torch.float64)
    for ky in range(s.ks):
        for kx in range(s.ks):
            a, mask = _gather(s, d, src, b, oy, ox, ky, kx)
            a, wt = a.reshape(ny * nx, -1), d["w"][:, :, ky, kx].double().t()
            acc += a @ wt
            t2 += (a * a) @ (wt * wt)
            w2 += mask.reshape(-1, 1) * (wt * wt).sum(0)[None]
            a2 += (a * a).sum(1, keepdim=True)
    if s.skip[0]:
        a, wt = _skip_source(s, d, b, oy, ox).reshape(ny * nx, -1), d["skip_w"].double().t()
        acc += a @ wt
        t2 += (a * a) @ (wt * wt)
        w2 += (wt * wt).sum(0)[None]
        a2 += (a * a).sum(1, keepdim=True)
    shape = (ny, nx, s.n)
    ref, r, lin = epilogue(s, d, b, oy, ox, acc.reshape(shape))
    return Result(ref=ref, lin=lin, R=r, T=t2.sqrt().reshape(shape), W=w2.sqrt().reshape(shape), A=a2.sqrt().expand(-1, s.n).reshape(shape))


# ---- the references the constants are measured on -----------------------------------------------------------------------------------
UPFOLD_TAPS = (((0, 0), (1, 2)), ((0, 1), (2, 2)))   # [parity][tap] -> the rows / columns of the 3x3 kernel the folded tap sums


def emulate(s, d, b, oy, ox, variant, defect=None):
    """float64 emulation of the documented split at output pixels oy x ox of sample b: operands rounded to nearest into hi and lo pieces,
    a_hi*w_hi + a_hi*w_lo + a_lo*w_hi accumulated in float64, the oracle's epilogue.  The folded upsampling conv contracts its folded
    weights.  `defect`: None, or one of DEFECTS - a kernel bug the budget must catch."""
    src, planes = _source(s, d, b, variant)
    oy, ox = np.asarray(oy), np.asarray(ox)
    acc = torch.zeros(len(oy), len(ox), s.n, dtype=torch.float64)

    def contract(a, w32, tap, a_pieces=None):
        ah, al = a_pieces if a_pieces is not None else split_act(a.float(), variant)
        wh, wl, ws = split_weight(w32, variant)
        ah, al, wh, wl = ah.double(), al.double(), wh.double().t(), wl.double().t()
        if defect == "wlo_tap" and tap == (4 if s.ks == 3 else 0):
            wl = torch.zeros_like(wl)
        r = ah @ wh + ah @ wl
        if defect != "drop_alo_whi":
            r = r + al @ wh
        return r / ws

    if s.fold:
        for py in range(2):
            for px in range(2):
                ys, xs = np.nonzero(oy % 2 == py)[0], np.nonzero(ox % 2 == px)[0]
                if not len(ys) or not len(xs):
                    continue
                part = torch.zeros(len(ys) * len(xs), s.n, dtype=torch.float64)
                for dy in range(2):
                    for dx in range(2):
                        (y0, y1), (x0, x1) = UPFOLD_TAPS[py][dy], UPFOLD_TAPS[px][dx]
                        wf = d["w"][:, :, y0:y1 + 1, x0:x1 + 1].double().sum((2, 3)).float()
                        a, _ = _gather(s, d, src, b, oy[ys], ox[xs], y0, x0, replicate=defect == "replicate" and (py, px, dy, dx) == (0, 0, 0, 0))
                        part += contract(a.reshape(len(ys) * len(xs), -1), wf, dy * 2 + dx)
                acc[torch.as_tensor(ys)[:, None], torch.as_tensor(xs)[None, :]] = part.reshape(len(ys), len(xs), s.n)
    else:
        flat = acc.reshape(-1, s.n)
        for ky in range(s.ks):
            for kx in range(s.ks):
                if planes is not None:
                    a, pieces = None, tuple(p[torch.as_tensor(oy)][:, torch.as_tensor(ox)].reshape(len(oy) * len(ox), -1) for p in planes)
                else:
                    a, _ = _gather(s, d, src, b, oy, ox, ky, kx, replicate=defect == "replicate" and (ky, kx) == (0, 0))
                    a, pieces = a.reshape(len(oy) * len(ox), -1), None
                flat += contract(a, d["w"][:, :, ky, kx], ky * 3 + kx, pieces)
        if s.skip[0]:
            flat += contract(_skip_source(s, d, b, oy, ox).reshape(len(oy) * len(ox), -1), d["skip_w"], -1)
    out, _, lin = epilogue(s, d, b, oy, ox, acc, row_shift=1 if defect == "sbias_row" else 0)
    return out, lin


DEFECTS = ("drop_alo_whi", "wlo_tap", "replicate", "sbias_row")


def emulate_wino(s, d, b, variant):
    """the Winograd F(2x2, 3x3) form of sample b, whole image (tools/micro/winograd_numerics.py): input tiles transformed and held in fp32, then
    split; U = G g G^T transformed in float64, rounded to fp32 and split as the packer does; products and both transforms in float64"""
    src, _ = _source(s, d, b, variant)
    h, w = s.h, s.w
    a = _gather(s, d, src, b, np.arange(-1, h + 1), np.arange(-1, w + 1), 1, 1)[0]   # the padded image (ks = 3: offset 1 - 1)
    Bt = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
    G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
    At = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)
    t = a.float().double().permute(2, 0, 1).unfold(1, 4, 2).unfold(2, 4, 2)            # [C][th][tw][4][4]
    V = torch.einsum("ij,cyxjk,lk->cyxil", Bt, t, Bt).float()
    U = torch.einsum("ij,ocjk,lk->ocil", G, d["w"].double(), G).float()
    vh, vl = (p.double() for p in split_act(V, variant))
    uh, ul, ws = split_weight(U, variant)
    uh, ul = uh.double(), ul.double()
    Mx = (torch.einsum("cyxil,ocil->oyxil", vh, uh) + torch.einsum("cyxil,ocil->oyxil", vh, ul) + torch.einsum("cyxil,ocil->oyxil", vl, uh)) / ws
    Y = torch.einsum("ij,oyxjk,lk->oyxil", At, Mx, At)                                  # [O][th][tw][2][2]
    acc = Y.permute(1, 3, 2, 4, 0).reshape(h, w, s.n)
    out, _, lin = epilogue(s, d, b, np.arange(h), np.arange(w), acc)
    return out, lin


def torch_compose(s, d, dtype, variant="", linear=False):
    """the same launch as a composition of torch's own ops in `dtype`, whole batch: [B][hout][wout][n_out] (`linear`: before the GeGLU)"""
    B = s.b
    if s.a_planes:
        hi, lo = split_act(d["x0"], variant)
        x = (hi.double() + lo.double()).to(dtype)
    else:
        x = d["x0"].to(dtype)
        if s.c1:
            x = torch.cat([x, d["x1"].to(dtype)[torch.arange(B) % d["x1"].shape[0]]], dim=-1)
    if s.pro in (1, 2):
        x = x * d["sc"].to(dtype)[:, None, None, :] + d["sh"].to(dtype)[:, None, None, :]
        x = F.silu(x) if s.pro == 1 else x
    elif s.pro == 3:
        x = (x - d["mean"].to(dtype).reshape(B, s.h, s.w, 1)) * d["rstd"].to(dtype).reshape(B, s.h, s.w, 1) * d["sc"].to(dtype) + d["sh"].to(dtype)
    w = d["w"].to(dtype)
    if s.ks == 1:
        y = F.linear(x, w[:, :, 0, 0])
    else:
        x = x.permute(0, 3, 1, 2)
        if s.ups:
            x = F.interpolate(x, scale_factor=2, mode="nearest")
        if s.pad_br:
            y = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2)
        else:
            y = F.conv2d(x, w, stride=s.stride, padding=1)
        y = y.permute(0, 2, 3, 1)
    if s.skip[0]:
        sx = d["skip_x0"].to(dtype)
        if s.skip[1]:
            sx = torch.cat([sx, d["skip_x1"].to(dtype)[torch.arange(B) % d["skip_x1"].shape[0]]], dim=-1)
        y = y + F.linear(sx, d["skip_w"].to(dtype), d["skip_bias"].to(dtype))
    if s.bias:
        y = y + d["bias"].to(dtype)
    if s.sbias:
        rows = torch.tensor([sbias_row(s, d, b) for b in range(B)])
        y = y + d["sbias"].to(dtype)[rows, :s.n][:, None, None, :]
    if s.res:
        y = y + d["res"].to(dtype)[..., :s.n]
    if s.geglu and not linear:
        idx = torch.arange(s.n).reshape(s.n // 64, 2, 32)
        y = y[..., idx[:, 0].reshape(-1)] * F.gelu(y[..., idx[:, 1].reshape(-1)])
    return y


# ---- the budget ---------------------------------------------------------------------------------------------------------------------
def mode_of(s, variant):
    return "f32" if s.prec == 0 else "f16" if variant == "f16" else "bf16"


def split_key(s, mode):
    """the Winograd form (transformed operands) and the folded upsampling conv (row / column-summed weights, T taken over the unfolded
    products) have constants of their own"""
    return ("wino_" if s.wino else "fold_" if s.fold else "") + mode


def split_scale(mode, o):
    """what M_SPLIT multiplies: u * T, and in the fp16 build the floor of its subnormal lo pieces (module text)"""
    t = UNIT[mode] * o.T
    if mode == "f16":
        t = t + 2.0 ** -25 * o.W + 2.0 ** -33 * o.A
    return t


def acc_scale(s, o):
    return math.sqrt(k_products(s)) * EPS * o.T


def budget(s, variant, o, m_acc=None, m_split=None):
    """tol per stored element.  A GeGLU output v * gelu(g) carries tol_v * |gelu(g)| + |v| * (1.13 tol_g + 2^-22 |g|) + 2 * 2^-24 |v gelu(g)|:
    first order, max |gelu'| = 1.13, the kernels' erf polynomial is within 1.5e-7 < 2^-22 / 2 * 2 of erf, two roundings of the products.  A
    plane store (hi + lo) adds the pair's representation error, two roundings to nearest of p significand bits each: 2^-2p |v|, that is
    2^-16 |v| with bf16 pieces (p = 8) and 2^-22 |v| + 2^-25 (a subnormal lo piece) with fp16 pieces (p = 11)."""
    mode = mode_of(s, variant)
    t = (M_ACC if m_acc is None else m_acc) * acc_scale(s, o)
    if mode != "f32":
        t = t + (M_SPLIT[split_key(s, mode)] if m_split is None else m_split) * split_scale(mode, o)
    tol = M * t + 4 * EPS * o.R
    if s.geglu:
        sh = (*tol.shape[:-1], s.n // 64, 2, 32)
        tv, tg = tol.reshape(sh)[..., 0, :], tol.reshape(sh)[..., 1, :]
        v, g = o.lin.reshape(sh)[..., 0, :], o.lin.reshape(sh)[..., 1, :]
        gelu = 0.5 * g * (1.0 + torch.special.erf(g / math.sqrt(2.0)))
        tol = (tv * gelu.abs() + v.abs() * (1.13 * tg + 2.0 ** -22 * g.abs()) + 2 * EPS * (v * gelu).abs()).reshape(*tol.shape[:-1], s.n // 2)
    if s.out_planes or s.qkv:
        tol = tol + ((2.0 ** -22 * (o.ref.abs() + tol) + 2.0 ** -25) if mode == "f16" else 2.0 ** -16 * (o.ref.abs() + tol))
    return tol


# ---- what is compared: whole samples, or windows of a big case ----------------------------------------------------------------------
def regions(s, info):
    """[(b, oy, ox)]: every output pixel of every sample; for a case above BIG_GMAC the first and last sample's four corners, four edge
    midpoints and two interior windows, each two workgroup tiles and two pixels wide so that it straddles tile boundaries"""
    ho, wo = out_hw(s)
    if gmac(s) <= BIG_GMAC:
        return [(b, np.arange(ho), np.arange(wo)) for b in range(s.b)]
    up = 2 if s.fold else 1   # a folded tile covers 2 th x 2 tw output pixels
    ey, ex = min(ho, 2 * up * info.tile_h + 2), min(wo, 2 * up * info.tile_w + 2)
    ys, xs = (0, (ho - ey) // 2 | 1, ho - ey), (0, (wo - ex) // 2 | 1, wo - ex)
    starts = [(y, x) for y in ys for x in xs if (y, x) != (ys[1], xs[1])]
    starts += [(up * info.tile_h * 3 - 1, up * info.tile_w * 5 - 1), (ho - up * info.tile_h * 5 - 1, wo - up * info.tile_w * 3 - 1)]
    return [(b, np.arange(y, y + ey), np.arange(x, x + ex)) for b in sorted({0, s.b - 1}) for y, x in starts]


def stats_tile_map(s, info):
    """[hout][wout] -> index of the statistics tile that counts the pixel (include/pfhip.h pf_conv_stats_tiles; csrc/conv_plan.hip)"""
    ho, wo = out_hw(s)
    yy, xx = np.mgrid[0:ho, 0:wo]
    if info.form == WINO:
        return (yy // 16) * (wo // 16) + xx // 16
    if info.ksplit > 1:
        return (yy * wo + xx) // 64
    if s.fold:
        return ((yy // 2 // info.tile_h) * cdiv(s.w, info.tile_w) + xx // 2 // info.tile_w) * 4 + (yy % 2) * 2 + xx % 2
    return (yy // info.tile_h) * cdiv(wo, info.tile_w) + xx // info.tile_w
