"""The small-kernel case matrix: the kernels around the convs - GroupNorm and LayerNorm statistics (csrc/norm_stats.hip), the stem and head
convolutions, the time embedding and the batched mat-vec (csrc/small_kernels.hip) - each with

  * a case table (cases(kind)) whose every case names the branches it exists for (`why`; branches_of() derives them from the shape),
  * a float64 oracle written from the mathematics (ref: stable_diffusion/model/unet.py:63-68 time_embed, :78-80 stem, :145-149 head,
    :151-169 sinusoid, :286-289 emb_layers, :321-336 GroupNorm32; unet_attention.py:104-110 LayerNorm, :186-212 cross attention),
  * an fp32 emulator of the kernel's own arithmetic - the order of its fused multiply-adds, for the norms the per-thread sequential fp32
    runs, the fp32 partials and the float64 finalize - with a `defect=` switch (DEFECTS), and
  * the per-element tolerance of profiles/small_error_model.md, computed from the case's own magnitudes.

Host only: imports no GPU code.  Used by tests/test_small_matrix.py (no GPU), tests/test_gpu_small_matrix.py (-m gpu) and
tools/small_error_model.py, which measures the constants M below on the CPU (emulator against oracle, times a margin of 4: the emulator has
the kernels' summation order, the hardware's exp / rcp / contraction may differ by an ulp per operation).  No constant comes from a GPU."""
from __future__ import annotations

import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24          # unit roundoff of fp32
MARGIN = 4.0
# measured by tools/small_error_model.py, recorded in profiles/small_error_model.md (largest emulator ratio, rounded up to two decimals)
MEASURED = {"gn": 1.13, "ln": 0.46, "stem": 0.74, "head": 0.22, "time": 0.12, "mv": 0.29}
M = {k: MARGIN * v for k, v in MEASURED.items()}

f32, f64 = np.float32, np.float64


class Spec(dict):
    __getattr__ = dict.__getitem__

    def but(self, **kw):
        s = Spec(self)
        s.update(kw)
        return s


class Result(dict):
    __getattr__ = dict.__getitem__


def cdiv(a, b):
    return -(-a // b)


def rng_of(key):
    return np.random.Generator(np.random.PCG64(zlib.crc32(key.encode())))


def _normal(rng):
    def g(*shape, scale=1.0):
        return torch.from_numpy(rng.standard_normal(shape).astype(f32) * f32(scale))
    return g


def fma32(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 numbers is exact in float64, one rounding of the sum to float64, then to fp32"""
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def _np(t):
    return t.detach().cpu().numpy()


def x3_dtype(variant):
    return torch.float16 if variant == "f16" else torch.bfloat16


def ratio(err, tol):
    """largest err / tol; a NaN anywhere, or an error where the tolerance is zero, is infinite"""
    err, tol = torch.as_tensor(err, dtype=torch.float64), torch.as_tensor(tol, dtype=torch.float64)
    r = torch.where((err == 0) & (tol >= 0), torch.zeros_like(err), err / tol)
    return float(torch.nan_to_num(r, nan=float("inf"), posinf=float("inf")).max()) if r.numel() else 0.0


# =====================================================================================================================================
# GroupNorm: pf_gn_scale_shift (gn_partial_kernel + gn_finalize_tiles_kernel) and pf_gn_finalize_tiles
# =====================================================================================================================================
GN_REGIMES = ("benign", "off10", "off100", "const", "outlier", "tiny", "big")
GN_DEFECTS = ("drop_last", "src0_only", "count_m1", "sqrt_plus_eps", "no_clamp")


def gn_nsplit(hw):
    return min(64, max(1, hw // 256))


def _gn(entry, b, hw, c0, c1=0, groups=32, eps=1e-5, regime="benign", t0=0, t1=0, why=()):
    s = Spec(kind="gn", entry=entry, b=b, hw=hw, c0=c0, c1=c1, groups=groups, eps=eps, regime=regime, t0=t0, t1=t1, why=tuple(why))
    key = f"gn {entry} B{b} hw{hw} {c0}+{c1} g{groups} eps{eps:g} {regime}" + (f" t{t0}+{t1}" if entry == "tiles" else "")
    return key, s


def gn_branches(s):
    C, out = s.c0 + s.c1, set()
    gs = C // s.groups
    out.add(f"regime:{s.regime}")
    out.add(f"eps:{s.eps:g}")
    out.add(f"B:{s.b}")
    if s.c1 and any(g * gs < s.c0 < (g + 1) * gs for g in range(s.groups)):
        out.add("straddle")
    if s.c1:
        out.add("two_sources")
    if s.entry == "data":
        ns, PL = gn_nsplit(s.hw), 256 // (C // 4)
        chunk = cdiv(s.hw, ns)
        out.add("one_split" if ns == 1 else "split_clamp64" if ns == 64 else "multi_split")
        if s.hw < 256:
            out.add("hw_below_256")
        if s.hw - (ns - 1) * chunk != chunk:
            out.add("ragged_chunk")
        if chunk % PL:
            out.add("ragged_lanes")
        out.add(f"pixel_lanes:{PL}")
        if PL * (C // 4) < 256:
            out.add("idle_threads")
        if gs == 1:
            out.add("group_size_1")
        if s.groups == 1:
            out.add("one_group")
    else:
        n1 = max(min((g + 1) * gs, C) - max(g * gs, s.c0) for g in range(s.groups)) if s.c1 else 0
        out.add("tiles_differ" if s.c1 and s.t0 != s.t1 else "tiles_c1_0" if not s.c1 else "tiles_equal")
        if s.c1:
            out.add("pairs_below_64" if n1 * s.t1 < 64 else "pairs_above_64")
    return out


GN_REQUIRED = {"one_split", "multi_split", "split_clamp64", "hw_below_256", "ragged_chunk", "ragged_lanes", "pixel_lanes:256", "pixel_lanes:32",
               "pixel_lanes:10", "pixel_lanes:1", "idle_threads", "group_size_1", "one_group", "straddle", "two_sources", "tiles_differ",
               "tiles_c1_0", "pairs_below_64", "pairs_above_64", "B:1", "B:3", "eps:1e-05", "eps:1e-06"} | {f"regime:{r}" for r in GN_REGIMES}


def gn_cases():
    out = []
    for i, hw in enumerate((15, 255, 256, 257, 600, 64 * 256 + 37)):      # the pixel axis: group size 1, one sample
        why = {15: ("hw_below_256", "one_split"), 255: ("one_split",), 256: ("one_split",), 257: ("one_split", "ragged_lanes"),
               600: ("multi_split",), 64 * 256 + 37: ("split_clamp64", "ragged_chunk")}[hw]
        out.append(_gn("data", 1, hw, 32, eps=(1e-5, 1e-6)[i % 2], why=why + ("group_size_1", "pixel_lanes:32")))
    out.append(_gn("data", 3, 600, 32, eps=1e-6, why=("multi_split", "B:3")))
    # the channel axis
    out.append(_gn("data", 1, 257, 4, groups=1, why=("pixel_lanes:256", "one_group")))
    out.append(_gn("data", 3, 257, 4, groups=4, eps=1e-6, why=("pixel_lanes:256", "group_size_1")))
    out.append(_gn("data", 3, 257, 96, why=("pixel_lanes:10", "idle_threads")))
    out.append(_gn("data", 1, 600, 96, eps=1e-6, why=("pixel_lanes:10", "idle_threads", "multi_split")))
    out.append(_gn("data", 1, 257, 256, 128, eps=1e-6, why=("straddle", "two_sources")))
    out.append(_gn("data", 3, 15, 256, 128, why=("straddle", "two_sources", "hw_below_256")))
    out.append(_gn("data", 3, 257, 64, 32, why=("two_sources",)))
    out.append(_gn("data", 1, 15, 1024, eps=1e-6, why=("pixel_lanes:1",)))
    out.append(_gn("data", 1, 257, 1024, why=("pixel_lanes:1",)))
    # the data regimes, on the straddling concat and on the two-split 64+32, both eps
    for i, r in enumerate(GN_REGIMES[1:]):
        out.append(_gn("data", 3, 15, 256, 128, eps=(1e-5, 1e-6)[i % 2], regime=r, why=(f"regime:{r}", "straddle")))
        out.append(_gn("data", 3, 600, 64, 32, eps=(1e-6, 1e-5)[i % 2], regime=r, why=(f"regime:{r}", "multi_split")))
    # pf_gn_finalize_tiles on fp32 tile statistics made from the data
    for i, r in enumerate(GN_REGIMES):
        out.append(_gn("tiles", 3, 45, 256, 128, eps=(1e-5, 1e-6)[i % 2], regime=r, t0=1, t1=(5, 9)[i % 2],
                       why=("tiles_differ", "straddle", "pairs_below_64" if i % 2 == 0 else "pairs_above_64", f"regime:{r}")))
        out.append(_gn("tiles", (1, 3)[i % 2], 45, 64, 0, eps=(1e-6, 1e-5)[i % 2], regime=r, t0=1, why=("tiles_c1_0", f"regime:{r}")))
    return out


def gn_inputs(key, s):
    rng = rng_of(key)
    g = _normal(rng)
    B, C = s.b, s.c0 + s.c1
    gs = C // s.groups
    x = g(B, s.hw, C)
    if s.regime in ("off10", "off100"):      # group |mean| / std = 10 or 100, the sign alternating from group to group
        sign = torch.tensor([1.0, -1.0]).repeat(s.groups)[:s.groups].repeat_interleave(gs)
        x = x + sign * float(s.regime[3:])
    else:
        x = x * 1.5 + 0.3
    if s.regime == "const":                   # sample 0: every group exactly constant, a value of its own
        v = torch.tensor([(1.5 + 0.37 * i) * (-1.0) ** i for i in range(s.groups)], dtype=torch.float32).repeat_interleave(gs)
        x[0] = v
    if s.regime == "outlier":                 # one channel of a group (the straddling one where there is one) a hundred times the rest
        grp = s.c0 // gs if s.c1 and s.c0 % gs else 1 % s.groups
        x[..., grp * gs] *= 100.0
    if s.regime == "tiny":
        x = x * 1e-4
    if s.regime == "big":
        x = x * 1e3
    d = {"x0": x[..., :s.c0].contiguous(), "gamma": 1 + 0.1 * g(C), "beta": 0.1 * g(C)}
    if s.c1:
        d["x1"] = x[..., s.c0:].contiguous()
    if s.entry == "tiles":

        def tile_stats(t, nt):   # any split of the pixels into nt parts is a valid producer layout; the producers store fp32
            parts = t.double().tensor_split(nt, dim=1)
            return torch.stack([torch.stack([p.sum(1), (p * p).sum(1)], dim=-1) for p in parts], dim=1).float().contiguous()

        d["stats0"] = tile_stats(d["x0"], s.t0)
        if s.c1:
            d["stats1"] = tile_stats(d["x1"], s.t1)
    return d


def _gn_x(s, d):
    return torch.cat([d["x0"], d["x1"]], dim=-1) if s.c1 else d["x0"]


def gn_eps(s):
    return float(f32(s.eps))      # the kernels take a float and widen it


def gn_oracle(s, d):
    """two-pass float64 GroupNorm of the data: y = x * scale + shift"""
    B, C = s.b, s.c0 + s.c1
    gs = C // s.groups
    x = _gn_x(s, d).double().reshape(B, s.hw, s.groups, gs)
    mean = x.mean((1, 3))
    var = ((x - mean[:, None, :, None]) ** 2).mean((1, 3))
    rstd = 1.0 / torch.sqrt(var + gn_eps(s))
    ga, be = d["gamma"].double(), d["beta"].double()
    scale = rstd.repeat_interleave(gs, 1) * ga
    shift = be - mean.repeat_interleave(gs, 1) * scale
    return Result(scale=scale, shift=shift, mean=mean, var=var, S=x.sum((1, 3)), Q=(x * x).sum((1, 3)), A1=x.abs().sum((1, 3)))


def gn_torch(s, d):
    """the same statement by torch: F.group_norm on double, [B][hw][C]"""
    x = _gn_x(s, d).double().permute(0, 2, 1)
    return F.group_norm(x, s.groups, d["gamma"].double(), d["beta"].double(), gn_eps(s)).permute(0, 2, 1)


def gn_partials(s, d, defect=None):
    """gn_partial_kernel: thread (pixel lane pl, channel quad) adds its pixels p0 + pl, p0 + pl + PL, ... in fp32 (sum, and sum of squares
    by fused multiply-add), the PL lanes of a channel are added in float64 and stored as fp32: [B][nsplit][C][2]"""
    x = _np(_gn_x(s, d))
    B, C = s.b, s.c0 + s.c1
    PL, ns = 256 // (C // 4), gn_nsplit(s.hw)
    chunk = cdiv(s.hw, ns)
    out = np.zeros((B, ns, C, 2), f32)
    for sp in range(ns):
        p0, p1 = sp * chunk, min(s.hw, sp * chunk + chunk)
        if defect == "drop_last":
            p1 -= 1
        seg = x[:, p0:p1]
        it = cdiv(p1 - p0, PL)
        seg = np.concatenate([seg, np.zeros((B, it * PL - (p1 - p0), C), f32)], 1).reshape(B, it, PL, C)
        sm, sq = np.zeros((B, PL, C), f32), np.zeros((B, PL, C), f32)
        for i in range(it):
            sm = sm + seg[:, i]
            sq = fma32(seg[:, i], seg[:, i], sq)
        out[:, sp, :, 0] = sm.astype(f64).sum(1).astype(f32)
        out[:, sp, :, 1] = sq.astype(f64).sum(1).astype(f32)
    return out


def gn_emulate(s, d, defect=None):
    """the launch as the kernels compute it: fp32 partials (made here for the data entry, given for the tiles entry), added per group in
    float64 over both sources, var = q / n - mean^2 clamped at 0, rstd = (var + eps)^-1/2, rows rounded to fp32"""
    B, C = s.b, s.c0 + s.c1
    gs = C // s.groups
    if s.entry == "data":
        tot = gn_partials(s, d, defect).astype(f64).sum(1)                    # [B][C][2]
    else:
        tot = _np(d["stats0"]).astype(f64).sum(1)
        if s.c1:
            tot = np.concatenate([tot, _np(d["stats1"]).astype(f64).sum(1)], 1)
    if defect == "src0_only":
        for g in range(s.groups):
            if s.c1 and g * gs < s.c0 < (g + 1) * gs:
                tot[:, s.c0:(g + 1) * gs] = 0.0
    grp = tot.reshape(B, s.groups, gs, 2).sum(2)
    cnt = float(gs * s.hw - (1 if defect == "count_m1" else 0))
    mean = grp[..., 0] / cnt
    var = grp[..., 1] / cnt - mean * mean
    if defect != "no_clamp":
        var = np.maximum(var, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        rstd = 1.0 / (np.sqrt(var) + gn_eps(s)) if defect == "sqrt_plus_eps" else 1.0 / np.sqrt(var + gn_eps(s))
    ga, be = _np(d["gamma"]).astype(f64), _np(d["beta"]).astype(f64)
    mean_c, rstd_c = np.repeat(mean, gs, 1), np.repeat(rstd, gs, 1)
    return Result(scale=torch.from_numpy((rstd_c * ga).astype(f32)), shift=torch.from_numpy((be - mean_c * rstd_c * ga).astype(f32)),
                  S=torch.from_numpy(grp[..., 0]), Q=torch.from_numpy(grp[..., 1]))


def gn_sum_units(s, o):
    """what M multiplies: the rounding of a group's sum and sum of squares.  A lane adds m numbers in sequence in fp32 (sqrt(m) roundings,
    each relative to the running sum <= sum |x|), and the lanes' float64 total is stored as fp32 (one more): U (1 + sqrt(m)) sum |x|.
    The tiles entry is given fp32 statistics of exact sums: m = 0."""
    m = 0
    if s.entry == "data":
        m = cdiv(cdiv(s.hw, gn_nsplit(s.hw)), 256 // ((s.c0 + s.c1) // 4))
    fac = U * (1.0 + math.sqrt(m))
    return fac * o.A1, fac * o.Q


def gn_tol(s, d, o, m=None):
    """(tol_scale, tol_shift) [B][C]: dS, dQ of gn_sum_units times M, through mean = S / n and var = Q / n - mean^2 to the interval of
    rstd = (max(var -+ dvar, 0) + eps)^-1/2 (to first order rstd * dvar / (2 (var + eps)); the interval stays right where dvar exceeds
    var + eps, the constant group), then scale = rstd gamma, shift = beta - mean rstd gamma; two fp32 roundings on top"""
    m = M["gn"] if m is None else m
    gs = (s.c0 + s.c1) // s.groups
    n = gs * s.hw
    uS, uQ = gn_sum_units(s, o)
    dmean = m * uS / n
    dvar = m * uQ / n + 2 * o.mean.abs() * dmean + dmean * dmean
    eps = gn_eps(s)
    rstd = 1.0 / torch.sqrt(o.var + eps)
    r_hi, r_lo = 1.0 / torch.sqrt((o.var - dvar).clamp_min(0.0) + eps), 1.0 / torch.sqrt(o.var + dvar + eps)
    drstd = torch.maximum(r_hi - rstd, rstd - r_lo)
    ga, be = d["gamma"].double().abs(), d["beta"].double().abs()
    rep = lambda t: t.repeat_interleave(gs, 1)  # noqa: E731
    tol_scale = ga * rep(drstd) + 2 * U * o.scale.abs()
    tol_shift = ga * rep(o.mean.abs() * drstd + r_hi * dmean) + 2 * U * (be + (o.shift - d["beta"].double()).abs())
    return tol_scale, tol_shift


def gn_ratio(s, d, o, got_scale, got_shift, m=None):
    ts, th = gn_tol(s, d, o, m)
    return max(ratio((got_scale.double() - o.scale).abs(), ts), ratio((got_shift.double() - o.shift).abs(), th))


# =====================================================================================================================================
# LayerNorm: pf_ln_stats, pf_ln_planes
# =====================================================================================================================================
LN_REGIMES = ("benign", "off100", "const", "tiny")
LN_DEFECTS = ("one_pass", "div256")
LN_ROWS, LN_C = (1, 3, 4, 5), (4, 64, 252, 256, 260, 1024, 2048)
LN_EPS = 1e-5


def ln_branches(s):
    out = {f"rows:{s.rows}", f"C:{s.c}", f"regime:{s.regime}", f"entry:{s.entry}"}
    out.add("partial_workgroup" if s.rows % 4 else "full_workgroup")
    if s.rows > 4:
        out.add("two_workgroups")
    out.add("idle_lanes" if s.c < 256 else "ragged_pass" if s.c % 256 else "full_passes")
    return out


LN_REQUIRED = ({f"rows:{r}" for r in LN_ROWS} | {f"C:{c}" for c in LN_C} | {f"regime:{r}" for r in LN_REGIMES}
               | {"entry:stats", "entry:planes", "partial_workgroup", "full_workgroup", "two_workgroups", "idle_lanes", "ragged_pass", "full_passes"})


def ln_cases():
    out, i = [], 0
    for entry in ("stats", "planes"):
        for c in LN_C:
            if entry == "planes" and c > 1024:
                continue
            for r in LN_REGIMES:
                rows = LN_ROWS[i % 4]
                i += 1
                s = Spec(kind="ln", entry=entry, rows=rows, c=c, regime=r, why=(f"C:{c}", f"regime:{r}", f"rows:{rows}"))
                out.append((f"ln {entry} rows{rows} C{c} {r}", s))
            i += 1      # another rotation of the rows for the next C
    return out


def ln_inputs(key, s):
    g = _normal(rng_of(key))
    x = g(s.rows, s.c)
    if s.regime == "benign":
        x = x * 1.4 + 0.2
    elif s.regime == "off100":
        x = x + 100.0
    elif s.regime == "const":
        x = torch.tensor([3.7, -100.3, 0.013, 1000.1, 7.0])[:s.rows, None].repeat(1, s.c)
    else:
        x = x * 1e-4
    return {"x": x.contiguous(), "gamma": 1 + 0.1 * g(s.c), "beta": 0.1 * g(s.c)}


def ln_oracle(s, d):
    x = d["x"].double()
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + float(f32(LN_EPS)))
    t = (x - mean[:, None]) * rstd[:, None] * d["gamma"].double()
    return Result(mean=mean, var=var, rstd=rstd, t=t, y=t + d["beta"].double(), A1=x.abs().sum(1))


def ln_torch(s, d):
    return F.layer_norm(d["x"].double(), (s.c,), d["gamma"].double(), d["beta"].double(), float(f32(LN_EPS)))


def _butterfly(v):
    """the shuffle tree of a 64-lane wave in fp32: v[..., 64] -> lane 0's total"""
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ off]
    return v[..., 0]


def ln_emulate(s, d, defect=None, variant=""):
    """ln_stats_kernel / ln_planes_kernel: lane l adds its float4s k = 4 l + 256 i as s += (x + y) + (z + w), the wave's shuffle tree,
    mu = s / C, the same order over (x - mu)^2, rstd = 1 / sqrt(q / C + eps), y = (x - mu) * rstd * gamma + beta - all fp32"""
    x = _np(d["x"])
    rows, Cc = x.shape
    it = cdiv(Cc, 256)
    pad = it * 256 - Cc
    valid = np.concatenate([np.ones(Cc, bool), np.zeros(pad, bool)]).reshape(it, 64, 4)
    xp = np.concatenate([x, np.zeros((rows, pad), f32)], 1).reshape(rows, it, 64, 4)
    div = f32(256.0 if defect == "div256" else Cc)

    def lanes(v):
        acc = np.zeros((rows, 64), f32)
        for i in range(it):
            acc = acc + ((v[:, i, :, 0] + v[:, i, :, 1]) + (v[:, i, :, 2] + v[:, i, :, 3]))
        return _butterfly(acc)

    mu = lanes(xp) / div
    if defect == "one_pass":
        qv = lanes(xp * xp) / div - mu * mu
    else:
        c = np.where(valid[None], xp - mu[:, None, None, None], f32(0.0))
        qv = lanes(c * c) / div
    with np.errstate(invalid="ignore"):
        rstd = f32(1.0) / np.sqrt(qv + f32(LN_EPS))
    y = (x - mu[:, None]) * rstd[:, None] * _np(d["gamma"]) + _np(d["beta"])
    y = torch.from_numpy(y.astype(f32))
    hi = y.to(x3_dtype(variant))
    lo = (y - hi.float()).to(x3_dtype(variant))
    return Result(mean=torch.from_numpy(mu), rstd=torch.from_numpy(rstd.astype(f32)), qv=torch.from_numpy(qv.astype(f32)), y=y,
                  planes=hi.double() + lo.double())


def ln_depth(s):
    """additions on the path of an element to the row sum: 2 inside the float4, one per pass of the lane, 6 shuffle levels, the division"""
    return 2 + cdiv(s.c, 256) + 6 + 1


def ln_mean_unit(s, o):
    return U * math.sqrt(ln_depth(s)) * o.A1 / s.c


def ln_tol(s, d, o, variant="", m=None):
    """(tol_mean, tol_rstd, tol_planes): dmu = M * ln_mean_unit.  The centred sum of squares of the kernel is that of the data plus C dmu^2
    (exactly), and is rounded like the mean: dvar = dmu^2 + M U (sqrt(depth) + 3) (var + dmu^2), to rstd through the interval of
    (var -+ dvar + eps)^-1/2, plus 4 roundings.  An output (x - mu) rstd gamma + beta moves by |gamma| (rstd dmu + |x - mu| drstd), plus 4
    roundings; a plane pair (hi + lo) adds 2^-16 |y| with bf16 pieces, 2^-22 |y| + 2^-25 with fp16 pieces (as conv_matrix.budget)."""
    m = M["ln"] if m is None else m
    eps = float(f32(LN_EPS))
    dmu = m * ln_mean_unit(s, o)
    dvar = dmu * dmu + m * U * (math.sqrt(ln_depth(s)) + 3) * (o.var + dmu * dmu)
    r_hi, r_lo = 1.0 / torch.sqrt((o.var - dvar).clamp_min(0.0) + eps), 1.0 / torch.sqrt(o.var + dvar + eps)
    drstd = torch.maximum(r_hi - o.rstd, o.rstd - r_lo) + 4 * U * o.rstd
    tol_y = d["gamma"].double().abs() * (r_hi * dmu)[:, None] + (o.t / o.rstd[:, None]).abs() * drstd[:, None] + 4 * U * (o.t.abs() + o.y.abs())
    if variant == "f16":
        tol_p = tol_y + 2.0 ** -22 * (o.y.abs() + tol_y) + 2.0 ** -25
    else:
        tol_p = tol_y + 2.0 ** -16 * (o.y.abs() + tol_y)
    return dmu + U * o.mean.abs(), drstd, tol_p


def ln_ratio(s, d, o, got, variant="", m=None):
    """got: Result with mean / rstd (stats entry) or planes (planes entry)"""
    tm, tr, tp = ln_tol(s, d, o, variant, m)
    if s.entry == "stats":
        return max(ratio((got.mean.double() - o.mean).abs(), tm), ratio((got.rstd.double() - o.rstd).abs(), tr))
    return ratio((got.planes - o.y).abs(), tp)


# =====================================================================================================================================
# Stem: pf_conv_in (conv_in_reg_kernel<1|2> with tile statistics, conv_in_kernel)
# =====================================================================================================================================
STEM_DEFECTS = ("stats_oob", "tile_transposed")
STEM_HW = ((16, 16), (12, 20), (17, 33), (1, 1))


def stem_branches(s):
    out = {f"cin:{s.cin}", f"cout:{s.cout}", f"B:{s.b}", f"hw:{s.h}x{s.w}"}
    out.add("register_kernel" if s.cin <= 2 and s.cout == 64 else "generic_kernel")
    if s.stats:
        out.add("statistics")
    if s.h % 16 or s.w % 16:
        out.add("ragged_tile")
    if cdiv(s.h, 16) > 1 and cdiv(s.w, 16) > 1 and cdiv(s.h, 16) != cdiv(s.w, 16):
        out.add("tile_grid_2d")
    return out


STEM_REQUIRED = ({"register_kernel", "generic_kernel", "statistics", "ragged_tile", "tile_grid_2d", "cin:1", "cin:2", "cin:3", "cin:4", "cout:32",
                  "cout:64", "cout:128", "B:1", "B:3"} | {f"hw:{h}x{w}" for h, w in STEM_HW})


def stem_cases():
    out = []
    for cin in (1, 2):
        for i, (h, w) in enumerate(STEM_HW):
            b = (1, 3)[(i + cin) % 2]
            for stats in (1, 0) if (h, w) == (17, 33) else (1,):
                s = Spec(kind="stem", b=b, cin=cin, cout=64, h=h, w=w, stats=stats, why=("register_kernel", f"cin:{cin}", f"hw:{h}x{w}"))
                out.append((f"stem B{b} {cin}>64 {h}x{w}" + (" stats" if stats else ""), s))
    for j, (cin, cout) in enumerate(((2, 32), (3, 64), (4, 128))):
        for i, (h, w) in enumerate(STEM_HW):
            if (i + j) % 2 and (h, w) != (17, 33):
                continue
            b = (3, 1)[(i + j) % 2] if (h, w) != (17, 33) else (1, 3)[j % 2]
            s = Spec(kind="stem", b=b, cin=cin, cout=cout, h=h, w=w, stats=0, why=("generic_kernel", f"cin:{cin}", f"cout:{cout}", f"hw:{h}x{w}"))
            out.append((f"stem B{b} {cin}>{cout} {h}x{w}", s))
    return out


def stem_inputs(key, s):
    g = _normal(rng_of(key))
    return {"x": g(s.b, s.cin, s.h, s.w), "w": g(s.cout, s.cin, 3, 3, scale=(9 * s.cin) ** -0.5), "bias": 0.2 + 0.1 * g(s.cout)}


def stem_oracle(s, d):
    """3x3 convolution, zero padding 1, NCHW in, NHWC out, float64; T = |bias| + sum |w x|"""
    xp = F.pad(d["x"].double(), (1, 1, 1, 1))
    w, b = d["w"].double(), d["bias"].double()
    ref = b.expand(s.b, s.h, s.w, s.cout).clone()
    T = ref.abs()
    for ci in range(s.cin):
        for r in range(3):
            for c in range(3):
                p = xp[:, ci, r:r + s.h, c:c + s.w, None] * w[:, ci, r, c]
                ref, T = ref + p, T + p.abs()
    return Result(ref=ref, T=T)


def stem_torch(s, d):
    return F.conv2d(d["x"].double(), d["w"].double(), d["bias"].double(), padding=1).permute(0, 2, 3, 1)


def stem_emulate(s, d, defect=None):
    """acc = bias, then fmaf(x, w, acc) over input channel, tap row, tap column (a padding tap adds nothing); the register-weight
    kernel's statistics: a thread (pixel column, channel) adds its tile column's stored values top to bottom in fp32 (squares by fused
    multiply-add), one thread per channel then adds the 16 columns left to right; tile = ty * tilesx + tx, in-image pixels only"""
    ty_n, tx_n = cdiv(s.h, 16), cdiv(s.w, 16)
    Hp, Wp = 16 * ty_n, 16 * tx_n
    xp = np.pad(_np(d["x"]), ((0, 0), (0, 0), (1, 1 + Hp - s.h), (1, 1 + Wp - s.w)))
    w, b = _np(d["w"]), _np(d["bias"])
    acc = np.broadcast_to(b, (s.b, Hp, Wp, s.cout)).astype(f32)
    for ci in range(s.cin):
        for r in range(3):
            for c in range(3):
                acc = fma32(xp[:, ci, r:r + Hp, c:c + Wp, None], w[:, ci, r, c], acc)
    out = Result(out=torch.from_numpy(acc[:, :s.h, :s.w].copy()))
    if s.stats:
        inside = np.zeros((Hp, Wp), bool)
        inside[:s.h, :s.w] = True
        stats = np.zeros((s.b, ty_n * tx_n, s.cout, 2), f32)
        for ty in range(ty_n):
            for tx in range(tx_n):
                m = inside[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16].copy()
                if defect == "stats_oob" and not m.all():
                    m.reshape(-1)[np.argmin(m.reshape(-1))] = True       # the tile's first out-of-image pixel
                v = np.where(m[None, :, :, None], acc[:, ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16], f32(0.0))
                cs, cq = np.zeros((s.b, 16, s.cout), f32), np.zeros((s.b, 16, s.cout), f32)
                for py in range(16):
                    cs = cs + v[:, py]
                    cq = fma32(v[:, py], v[:, py], cq)
                a, q = np.zeros((s.b, s.cout), f32), np.zeros((s.b, s.cout), f32)
                for px in range(16):
                    a, q = a + cs[:, px], q + cq[:, px]
                t = tx * ty_n + ty if defect == "tile_transposed" else ty * tx_n + tx
                stats[:, t, :, 0], stats[:, t, :, 1] = a, q
        out["stats"] = torch.from_numpy(stats)
    return out


def dot_unit(k, T, ref):
    """what M multiplies in the dot-product kernels: sqrt(K) U sum |w x| (K fused multiply-adds in sequence, each rounding relative to a
    partial sum <= T) and two final roundings"""
    return math.sqrt(k) * U * T + 2 * U * ref.abs()


def stem_ratio(s, o, got, m=None):
    return ratio((got.double() - o.ref).abs(), (M["stem"] if m is None else m) * dot_unit(9 * s.cin + 1, o.T, o.ref))


def stem_stats_ratio(s, out, stats):
    """each tile's (sum, sumsq) against the float64 sums of the STORED output over the tile's in-image pixels: any order of n fp32 additions
    (and the rounding of a square) stays within (n + 2) U sum |x|"""
    tx_n = cdiv(s.w, 16)
    nt = cdiv(s.h, 16) * tx_n
    yy, xx = np.mgrid[0:s.h, 0:s.w]
    tmap = torch.from_numpy(((yy // 16) * tx_n + xx // 16).reshape(-1).astype(np.int64))
    npix = torch.bincount(tmap, minlength=nt).double()[None, :, None]
    x = out.double().reshape(s.b, s.h * s.w, s.cout)
    st = stats.double().reshape(s.b, nt, s.cout, 2)
    worst = 0.0
    for j, v in enumerate((x, x * x)):
        want = torch.zeros(s.b, nt, s.cout, dtype=torch.float64).index_add_(1, tmap, v)
        mag = torch.zeros(s.b, nt, s.cout, dtype=torch.float64).index_add_(1, tmap, v.abs())
        worst = max(worst, ratio((st[..., j] - want).abs(), (npix + 2) * U * mag))
    return worst


# =====================================================================================================================================
# Head: pf_conv_out (conv_out_kernel<1..4>)
# =====================================================================================================================================
HEAD_DEFECTS = ("pad_before_act", "odd_from_pair")
HEAD_HW = ((16, 16), (12, 20), (17, 33), (5, 3))


def head_branches(s):
    out = {f"cout:{s.cout}", f"chunks:{s.cin // 16}", f"B:{s.b}", f"hw:{s.h}x{s.w}", f"regime:{s.regime}"}
    out.add("odd_channel" if s.cout & 1 else "pairs_only")
    if s.cin > 16:
        out.add("prefetch")
    if s.h % 16 or s.w % 16:
        out.add("ragged_tile")
    return out


HEAD_REQUIRED = ({f"cout:{c}" for c in (1, 2, 3, 4)} | {"chunks:1", "chunks:2", "chunks:3", "prefetch", "odd_channel", "pairs_only", "ragged_tile",
                                                       "B:1", "B:3", "regime:shift2", "regime:extreme"} | {f"hw:{h}x{w}" for h, w in HEAD_HW})


def head_cases():
    out, i = [], 0
    for cout in (1, 2, 3, 4):
        for cin in (16, 32, 48):
            h, w = HEAD_HW[i % 4]
            b = (1, 3)[(i // 2) % 2]
            i += 1
            s = Spec(kind="head", b=b, cin=cin, cout=cout, h=h, w=w, regime="shift2", why=(f"cout:{cout}", f"chunks:{cin // 16}", f"hw:{h}x{w}"))
            out.append((f"head B{b} {cin}>{cout} {h}x{w}", s))
    out.append(("head B1 32>3 12x20 extreme", Spec(kind="head", b=1, cin=32, cout=3, h=12, w=20, regime="extreme", why=("regime:extreme",))))
    return out


def head_inputs(key, s):
    g = _normal(rng_of(key))
    x = g(s.b, s.h, s.w, s.cin)
    sc, sh = 1 + 0.1 * g(s.b, s.cin), 2 + 0.1 * g(s.b, s.cin)      # per-sample rows; silu(shift) ~ 1.76: padding before the activation shows
    if s.regime == "extreme":                                      # pre-activations x sc + sh reach +-100 and beyond: exp overflows
        x, sc = x.clamp(-2.6, 2.6), 40.0 * sc
    w = g(s.cout, s.cin, 3, 3, scale=(9 * s.cin) ** -0.5)
    return {"x": x.contiguous(), "sc": sc, "sh": sh, "w": w, "wp": w.permute(2, 3, 1, 0).reshape(9, s.cin, s.cout).contiguous(),
            "bias": 0.1 * g(s.cout)}


def head_oracle(s, d):
    """out = conv3x3(zero_pad(silu(x sc + sh))) + bias, NHWC in, NCHW out, float64, from the packed weight [9][cin][cout].
    T = sum |w a|; D = sum |w| da with da the activation's own error (head_da)"""
    v = d["x"].double() * d["sc"].double()[:, None, None, :] + d["sh"].double()[:, None, None, :]
    sg = torch.sigmoid(v)
    a = v * sg
    da = U * ((sg * (1 + v * (1 - sg))).abs() * v.abs() + a.abs() * (4 + v.abs()))
    ap, dap = F.pad(a, (0, 0, 1, 1, 1, 1)), F.pad(da, (0, 0, 1, 1, 1, 1))
    wp = d["wp"].double()
    ref = torch.zeros(s.b, s.h, s.w, s.cout, dtype=torch.float64)
    T, D = torch.zeros_like(ref), torch.zeros_like(ref)
    for t in range(9):
        r, c = t // 3, t % 3
        ref += ap[:, r:r + s.h, c:c + s.w] @ wp[t]
        T += ap[:, r:r + s.h, c:c + s.w].abs() @ wp[t].abs()
        D += dap[:, r:r + s.h, c:c + s.w] @ wp[t].abs()
    ref = ref + d["bias"].double()
    return Result(ref=ref.permute(0, 3, 1, 2), T=T.permute(0, 3, 1, 2), D=D.permute(0, 3, 1, 2), vmax=float(v.abs().max()))


def head_torch(s, d):
    v = d["x"].double() * d["sc"].double()[:, None, None, :] + d["sh"].double()[:, None, None, :]
    return F.conv2d(F.silu(v).permute(0, 3, 1, 2), d["w"].double(), d["bias"].double(), padding=1)


def _silu_rcp32(v):
    """v * rcp(1 + exp(-v)) in fp32 (exp and the reciprocal correctly rounded here; an overflowing exp gives rcp(inf) = 0)"""
    with np.errstate(over="ignore"):
        e = np.exp(-v.astype(f64)).astype(f32)
        den = f32(1.0) + e
        rc = (1.0 / den.astype(f64)).astype(f32)
    return (v * rc).astype(f32)


def head_emulate(s, d, defect=None):
    """a = silu(fma(x, sc, sh)) with the reciprocal form, zero outside the image AFTER the activation; acc = 0, fmaf(a, w, acc) over
    16-channel chunk, tap, channel of the chunk; bias added last"""
    x, sc, sh = _np(d["x"]), _np(d["sc"])[:, None, None, :], _np(d["sh"])[:, None, None, :]
    a = _silu_rcp32(fma32(x, sc, sh))
    ap = np.pad(a, ((0, 0), (1, 1), (1, 1), (0, 0)))
    if defect == "pad_before_act":
        border = np.ones((s.h + 2, s.w + 2), bool)
        border[1:-1, 1:-1] = False
        ap = np.where(border[None, :, :, None], np.broadcast_to(_silu_rcp32(fma32(f32(0.0), sc, sh)), ap.shape), ap)
    wp, bias = _np(d["wp"]), _np(d["bias"])
    acc = np.zeros((s.b, s.h, s.w, s.cout), f32)
    for c0 in range(0, s.cin, 16):
        for t in range(9):
            r, c = t // 3, t % 3
            for e in range(c0, c0 + 16):
                acc = fma32(ap[:, r:r + s.h, c:c + s.w, e, None], wp[t, e], acc)
    if defect == "odd_from_pair" and s.cout & 1:      # the last channel read from a pair accumulator: channel 0's, or one never used
        acc[..., s.cout - 1] = acc[..., 0] if s.cout > 1 else f32(0.0)
    return torch.from_numpy((acc + bias).astype(f32).transpose(0, 3, 1, 2).copy())


def head_ratio(s, o, got, m=None):
    """the dot-product unit over K = 9 cin products, plus D: the SiLU's error (one rounding of x sc + sh through silu', __expf's argument
    scaling |v| U and two ulps, the hardware reciprocal and two products: U (|silu'(v)| |v| + |a| (4 + |v|))) times |w|, summed"""
    return ratio((got.double() - o.ref).abs(), (M["head"] if m is None else m) * (dot_unit(9 * s.cin, o.T, o.ref) + o.D))


# =====================================================================================================================================
# Time embedding: pf_time_embed
# =====================================================================================================================================
TIME_DEFECTS = ("swap_sincos", "freq_f64")
TIME_T = (0, 1, 500, 999)


def time_branches(s):
    out = {f"sizes:{s.channels}x{s.d_t}", "table_form" if s.table else "tensor_form", f"weights:{s.weights}"}
    if s.channels > 256:
        out.add("sinusoid_loop_strided")
    if s.d_t > 256:
        out.add("linear_loop_strided")
    return out


TIME_REQUIRED = {"sizes:32x128", "sizes:64x256", "sizes:320x1280", "table_form", "tensor_form", "sinusoid_loop_strided", "linear_loop_strided",
                 "weights:dense", "weights:probe"}


def time_cases():
    out = []
    for ch, dt in ((32, 128), (64, 256), (320, 1280)):
        for weights in ("dense", "probe"):
            out.append((f"time {ch}x{dt} t{'-'.join(map(str, TIME_T))} {weights}",
                        Spec(kind="time", channels=ch, d_t=dt, table=0, batch=len(TIME_T), weights=weights, why=(f"sizes:{ch}x{dt}", f"weights:{weights}"))))
    out.append(("time 32x128 table1000 dense", Spec(kind="time", channels=32, d_t=128, table=1, batch=1000, weights="dense", why=("table_form",))))
    out.append(("time 64x256 table1000 probe", Spec(kind="time", channels=64, d_t=256, table=1, batch=1000, weights="probe", why=("table_form",))))
    return out


def time_inputs(key, s):
    """dense: Gaussian layers.  probe: W0 has one nonzero per row (row n reads sinusoid entry n % channels) and W2 is diagonal, so every
    sinusoid entry reaches outputs of its own instead of drowning in a sum over all of them"""
    g = _normal(rng_of(key))
    ch, dt = s.channels, s.d_t
    if s.weights == "probe":
        w0 = torch.zeros(dt, ch)
        w0[torch.arange(dt), torch.arange(dt) % ch] = 1 + 0.1 * g(dt)
        w2 = torch.diag(1 + 0.1 * g(dt))
    else:
        w0, w2 = g(dt, ch, scale=ch ** -0.5), g(dt, dt, scale=dt ** -0.5)
    d = {"w0": w0.contiguous(), "b0": 0.1 * g(dt), "w2": w2.contiguous(), "b2": 0.1 * g(dt)}
    d["t"] = torch.arange(s.batch, dtype=torch.int64) if s.table else torch.tensor(TIME_T, dtype=torch.int64)
    return d


def time_freqs32(channels):
    """exp(-ln(10000) j / half) evaluated in fp32 by torch, as the reference evaluates it (unet.py:161-165): product, quotient, exp"""
    half = channels // 2
    return torch.exp(torch.arange(half, dtype=torch.float32) * float(f32(-math.log(10000.0))) / half).numpy()


def _dsilu(p):
    sg = torch.sigmoid(p)
    return (sg * (1 + p * (1 - sg))).abs()


def time_oracle(s, d):
    """float64 from the fp32 frequencies on: args = t f, [cos | sin], two linears with SiLU, and the SiLU of emb_layers"""
    f = torch.from_numpy(time_freqs32(s.channels)).double()
    arg = d["t"].double()[:, None] * f
    e = torch.cat([torch.cos(arg), torch.sin(arg)], 1)
    w0, w2 = d["w0"].double(), d["w2"].double()
    p1 = e @ w0.t() + d["b0"].double()
    h = p1 * torch.sigmoid(p1)
    p2 = h @ w2.t() + d["b2"].double()
    return Result(ref=p2 * torch.sigmoid(p2), arg2=torch.cat([arg, arg], 1).abs(), p1=p1, h=h, p2=p2,
                  T1=e.abs() @ w0.abs().t() + d["b0"].double().abs(), T2=h.abs() @ w2.abs().t() + d["b2"].double().abs())


def time_tol(s, d, o, m=None, freq=1.0):
    """M times what depends on the order and form of the arithmetic - the dot-product unit of each layer, the fp32 SiLU v / (1 + exp(-v)):
    U |silu| (4 + |v|) - plus, outside M because they are bounds and no estimates, per sinusoid entry: the one IEEE product t * f,
    U |t f|; two ulps of a cosine or sine (|value| <= 1: 2 U); and `freq` ulps of the fp32 frequency, |t f| 2^-23 (the kernel's expf
    and the reference's exp need not round alike).
    An error u of a SiLU's argument leaves |silu'(v)| u + u^2 / 4 (|silu''| <= 1/2)."""
    m = M["time"] if m is None else m
    w0a, w2a = d["w0"].double().abs(), d["w2"].double().abs()
    de = 2 * U + (U + freq * 2.0 ** -23) * o.arg2
    u1 = m * dot_unit(s.channels + 1, o.T1, o.p1) + de @ w0a.t()
    uh = _dsilu(o.p1) * u1 + 0.25 * u1 * u1 + m * U * o.h.abs() * (4 + o.p1.abs())
    u2 = m * dot_unit(s.d_t + 1, o.T2, o.p2) + uh @ w2a.t()
    return _dsilu(o.p2) * u2 + 0.25 * u2 * u2 + m * U * o.ref.abs() * (4 + o.p2.abs())


def time_torch(s, d):
    """the module as the reference composes it, on double: time_step_embedding -> Linear, SiLU, Linear -> SiLU"""
    half = s.channels // 2
    freqs = torch.exp(-math.log(10000) * torch.arange(0, half, dtype=torch.float32) / half)
    args = d["t"][:, None].double() * freqs[None].double()
    emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    return F.silu(F.linear(F.silu(F.linear(emb, d["w0"].double(), d["b0"].double())), d["w2"].double(), d["b2"].double()))


def _silu_div32(v):
    with np.errstate(over="ignore"):
        e = np.exp(-v.astype(f64)).astype(f32)
        return (v / (f32(1.0) + e)).astype(f32)


def time_emulate(s, d, defect=None):
    """fp32: arg = t * f, cos | sin, acc = bias then fmaf(w[k], e[k], acc) for k ascending, v / (1 + exp(-v)), twice"""
    t = _np(d["t"]).astype(f32)
    if defect == "freq_f64":
        half = s.channels // 2
        arg = (t.astype(f64)[:, None] * np.exp(-math.log(10000.0) * np.arange(half) / half)).astype(f32)
    else:
        arg = t[:, None] * time_freqs32(s.channels)
    c, sn = np.cos(arg.astype(f64)).astype(f32), np.sin(arg.astype(f64)).astype(f32)
    e = np.concatenate([sn, c] if defect == "swap_sincos" else [c, sn], 1)

    def layer(w, b, v):
        acc = np.broadcast_to(b, (v.shape[0], w.shape[0])).astype(f32)
        for k in range(w.shape[1]):
            acc = fma32(w[:, k], v[:, k, None], acc)
        return _silu_div32(acc)

    return torch.from_numpy(layer(_np(d["w2"]), _np(d["b2"]), layer(_np(d["w0"]), _np(d["b0"]), e)))


def time_ratio(s, d, o, got, m=None, freq=1.0):
    return ratio((got.double() - o.ref).abs(), time_tol(s, d, o, m, freq))


# =====================================================================================================================================
# Mat-vec: pf_matvec (matvec_kernel<false|true>)
# =====================================================================================================================================
MV_DEFECTS = ("drop_k_tail", "no_row_clamp", "group_unclamped")


def _mv(b, n, k, ldx_pad=0, ldy_pad=0, bias=1, npg=0, xgs=0, exp=0, why=()):
    s = Spec(kind="mv", b=b, n=n, k=k, ldx_pad=ldx_pad, ldy_pad=ldy_pad, bias=bias, npg=npg, xgs=xgs, exp=exp, why=tuple(why))
    key = f"mv B{b} N{n} K{k}" + (f" ldx+{ldx_pad}" if ldx_pad else "") + (f" ldy+{ldy_pad}" if ldy_pad else "") + ("" if bias else " nobias")
    return key + (f" npg{npg} xgs{xgs}" if npg else "") + (" exp" if exp else ""), s


def mv_groups(s):
    return cdiv(s.n, s.npg) if s.npg > 0 else 1


def mv_ldx(s):
    return (mv_groups(s) - 1) * s.xgs + s.k + s.ldx_pad


def mv_block_staged(s, blk):
    """does 32-output block `blk` run the staged vector path?"""
    npg = s.npg if s.npg > 0 else s.n
    xgs = s.xgs if s.npg > 0 else 0
    vec = s.k % 32 == 0 and mv_ldx(s) % 4 == 0 and xgs % 4 == 0
    return vec and (blk * 32) // npg == min(blk * 32 + 31, s.n - 1) // npg


def mv_branches(s):
    out = {f"B:{s.b}", f"N:{s.n}", f"K:{s.k}"}
    staged = [mv_block_staged(s, blk) for blk in range(cdiv(s.n, 32))]
    if any(staged):
        out.add("vector_path")
        if s.k > 256:
            out.add("second_k_block_ragged" if s.k % 256 else "full_k_blocks")
    if not all(staged):
        out.add("scalar_path")
        out.add("scalar_by_k" if s.k % 32 else "scalar_by_ldx" if mv_ldx(s) % 4 else "scalar_by_group_stride" if s.npg > 0 and s.xgs % 4
                else "scalar_by_straddle")
    if s.b % 8:
        out.add("partial_row_block")
    if s.b > 8:
        out.add("several_row_blocks")
    if s.n % 32:
        out.add("partial_output_block")
    if s.n % 8:
        out.add("clamped_outputs")
    if s.ldx_pad:
        out.add("ldx_gap")
    if s.ldy_pad:
        out.add("ldy_gap")
    if not s.bias:
        out.add("no_bias")
    if s.npg > 0:
        out.add(f"grouped:{s.npg}")
        out.add("group_stride_vec" if s.xgs % 4 == 0 else "group_stride_odd")
        if any(staged) and not all(staged):
            out.add("grouped_mixed_paths")
        if s.npg > 0 and (cdiv(s.n, 32) * 32 - 1) // s.npg > (s.n - 1) // s.npg:
            out.add("group_past_end")
    if s.exp:
        out.add("exp")
    return out


MV_REQUIRED = ({f"B:{b}" for b in (1, 7, 8, 9, 17)} | {f"N:{n}" for n in (1, 31, 32, 33, 100)} | {f"K:{k}" for k in (32, 256, 288, 2048, 20, 36)}
               | {"vector_path", "scalar_path", "scalar_by_k", "scalar_by_ldx", "scalar_by_group_stride", "scalar_by_straddle",
                  "second_k_block_ragged", "full_k_blocks", "partial_row_block", "several_row_blocks", "partial_output_block", "clamped_outputs",
                  "ldx_gap", "ldy_gap", "no_bias", "grouped:32", "grouped:48", "group_stride_vec", "group_stride_odd", "grouped_mixed_paths",
                  "group_past_end", "exp"})


def mv_cases():
    return [
        _mv(1, 1, 32, why=("B:1", "N:1", "K:32", "vector_path")),
        _mv(7, 31, 256, ldy_pad=5, why=("B:7", "N:31", "K:256", "ldy_gap")),
        _mv(8, 32, 288, ldx_pad=8, why=("B:8", "N:32", "K:288", "second_k_block_ragged", "ldx_gap")),
        _mv(9, 33, 2048, why=("B:9", "N:33", "K:2048", "full_k_blocks")),
        _mv(17, 100, 288, bias=0, ldx_pad=4, ldy_pad=3, why=("B:17", "N:100", "no_bias", "several_row_blocks")),
        _mv(17, 33, 20, why=("K:20", "scalar_by_k")),
        _mv(9, 100, 36, ldx_pad=3, ldy_pad=1, bias=0, why=("K:36", "scalar_by_k")),
        _mv(7, 33, 32, ldx_pad=1, why=("scalar_by_ldx",)),
        _mv(1, 31, 20, why=("B:1", "scalar_path")),
        _mv(9, 100, 32, npg=32, xgs=32, why=("grouped:32", "group_stride_vec")),
        _mv(7, 100, 256, npg=48, xgs=256, ldx_pad=4, why=("grouped:48", "scalar_by_straddle", "grouped_mixed_paths")),
        _mv(8, 100, 32, npg=32, xgs=33, ldx_pad=1, why=("group_stride_odd", "scalar_by_group_stride")),
        _mv(17, 100, 36, npg=48, xgs=37, why=("grouped:48", "group_stride_odd")),
        _mv(7, 33, 36, npg=48, xgs=36, why=("group_past_end",)),
        _mv(9, 33, 256, exp=1, why=("exp", "vector_path")),
        _mv(7, 31, 20, exp=1, bias=0, ldy_pad=2, why=("exp", "scalar_path")),
    ]


def mv_inputs(key, s):
    g = _normal(rng_of(key))
    d = {"x": g(s.b, mv_ldx(s)), "w": g(s.n, s.k, scale=s.k ** -0.5)}
    if s.bias:
        d["bias"] = 0.1 * g(s.n)
    return d


def _mv_gather(s, d):
    npg = s.npg if s.npg > 0 else s.n
    xgs = s.xgs if s.npg > 0 else 0
    idx = (torch.arange(s.n) // npg * xgs)[:, None] + torch.arange(s.k)[None]
    return d["x"][:, idx]                                                  # [B][N][K]


def mv_oracle(s, d):
    xg, w = _mv_gather(s, d).double(), d["w"].double()
    p = xg * w
    b = d["bias"].double() if s.bias else torch.zeros(s.n, dtype=torch.float64)
    lin = p.sum(-1) + b
    return Result(lin=lin, ref=torch.exp(lin) if s.exp else lin, T=p.abs().sum(-1) + b.abs())


def mv_torch(s, d):
    b = d["bias"].double() if s.bias else None
    npg = s.npg if s.npg > 0 else s.n
    xgs = s.xgs if s.npg > 0 else 0
    w, x = d["w"].double(), d["x"].double()
    parts = [F.linear(x[:, g * xgs:g * xgs + s.k], w[g * npg:min(s.n, (g + 1) * npg)], None if b is None else b[g * npg:min(s.n, (g + 1) * npg)])
             for g in range(mv_groups(s))]
    y = torch.cat(parts, 1)
    return torch.exp(y) if s.exp else y


def mv_emulate(s, d, defect=None):
    """(y, reads_in_bounds).  The 8 lanes of an output take the float4s q = j, j + 8, ... (staged path; x, y, z, w of each in turn) or the
    elements k = j, j + 8, ... (scalar path) as one fmaf chain each, then add as ((l0 + l1) + (l2 + l3)) + ((l4 + l5) + (l6 + l7)), then
    the bias, then expf.  Two of the defects change no stored value: they read outside x (rows past the batch, a group past the last),
    which the second return value reports."""
    xg, w = _np(_mv_gather(s, d)), _np(d["w"])
    B, N, K = s.b, s.n, s.k
    xz, wz = np.concatenate([xg, np.zeros((B, N, 1), f32)], -1), np.concatenate([w, np.zeros((N, 1), f32)], -1)

    def run(order):                                 # order [8][steps]: element index per lane and step (K: the appended zero)
        acc = np.zeros((B, N, 8), f32)
        for i in range(order.shape[1]):
            kk = order[:, i]
            acc = fma32(wz[None, :, kk], xz[:, :, kk], acc)
        return acc

    sc_steps = cdiv(K, 8)
    order_sc = np.full((8, sc_steps), K, np.int64)
    for j in range(8):
        ks = np.arange(j, K, 8)
        order_sc[j, :len(ks)] = ks
    acc = run(order_sc)
    staged = np.array([mv_block_staged(s, n // 32) for n in range(N)])
    if staged.any():
        kq = K // 4
        order_v = np.array([[q * 4 + e for q in range(j, kq, 8) for e in range(4)] for j in range(8)], np.int64)
        if defect == "drop_k_tail" and K > 256 and K % 256:
            order_v = np.where(order_v >= K // 256 * 256, K, order_v)
        acc = np.where(staged[None, :, None], run(order_v), acc)
    t = acc[..., 0::2] + acc[..., 1::2]
    t = t[..., 0::2] + t[..., 1::2]
    v = t[..., 0] + t[..., 1]
    if s.bias:
        v = v + _np(d["bias"])
    if s.exp:
        v = np.exp(v.astype(f64)).astype(f32)
    ok = True
    if defect == "no_row_clamp" and B % 8:
        ok = False                                  # rows b0 + r >= B of the last row block are read
    if defect == "group_unclamped" and s.npg > 0 and not staged.all():
        last = max(n for n in range(cdiv(N, 32) * 32) if not mv_block_staged(s, n // 32))
        ok = last // s.npg <= (N - 1) // s.npg      # the group of an output past N, taken from the unclamped index
    return torch.from_numpy(v.astype(f32)), ok


def mv_ratio(s, o, got, m=None):
    """linear: the dot-product unit; exp: the same relative to the value (d exp(o) = exp(o) do) plus expf's two ulps"""
    unit = dot_unit(s.k + 1, o.T, o.lin)
    m = M["mv"] if m is None else m
    if s.exp:
        return ratio((got.double() - o.ref).abs(), o.ref.abs() * (m * unit + 2 * 2.0 ** -23))
    return ratio((got.double() - o.ref).abs(), m * unit)


# =====================================================================================================================================
# The tables, and what the library must refuse
# =====================================================================================================================================
KINDS = ("gn", "ln", "stem", "head", "time", "mv")
CASES = {"gn": gn_cases, "ln": ln_cases, "stem": stem_cases, "head": head_cases, "time": time_cases, "mv": mv_cases}
INPUTS = {"gn": gn_inputs, "ln": ln_inputs, "stem": stem_inputs, "head": head_inputs, "time": time_inputs, "mv": mv_inputs}
BRANCHES = {"gn": gn_branches, "ln": ln_branches, "stem": stem_branches, "head": head_branches, "time": time_branches, "mv": mv_branches}
REQUIRED = {"gn": GN_REQUIRED, "ln": LN_REQUIRED, "stem": STEM_REQUIRED, "head": HEAD_REQUIRED, "time": TIME_REQUIRED, "mv": MV_REQUIRED}
DEFECTS = {"gn": GN_DEFECTS, "ln": LN_DEFECTS, "stem": STEM_DEFECTS, "head": HEAD_DEFECTS, "time": TIME_DEFECTS, "mv": MV_DEFECTS}


def cases(kind=None):
    """[(key, spec)] of one kernel family, or of all"""
    return CASES[kind]() if kind else [c for k in KINDS for c in CASES[k]()]


def inputs(key, s):
    return INPUTS[s.kind](key, s)


def emulated_ratio(key, s, d, defect=None, m=None):
    """err / tol of the emulator (with `defect`) against the oracle; inf where a defect reads out of bounds"""
    if s.kind == "gn":
        o, e = gn_oracle(s, d), gn_emulate(s, d, defect)
        return gn_ratio(s, d, o, e.scale, e.shift, m)
    if s.kind == "ln":
        worst = 0.0
        for variant in ("", "f16") if s.entry == "planes" else ("",):
            worst = max(worst, ln_ratio(s, d, ln_oracle(s, d), ln_emulate(s, d, defect, variant), variant, m))
        return worst
    if s.kind == "stem":
        o, e = stem_oracle(s, d), stem_emulate(s, d, defect)
        r = stem_ratio(s, o, e.out, m)
        return max(r, stem_stats_ratio(s, e.out, e.stats)) if s.stats else r
    if s.kind == "head":
        return head_ratio(s, head_oracle(s, d), head_emulate(s, d, defect), m)
    if s.kind == "time":
        return time_ratio(s, d, time_oracle(s, d), time_emulate(s, d, defect), m)
    y, ok = mv_emulate(s, d, defect)
    return mv_ratio(s, mv_oracle(s, d), y, m) if ok else float("inf")


def measured_ratio(key, s, d):
    """what tools/small_error_model.py takes the maximum of: the undefective emulator against the oracle, relative to the model at M = 1
    (the norms: at the level of the sums the model speaks of - the group's sum and sum of squares, the row mean and centred squares)"""
    if s.kind == "gn":
        o, e = gn_oracle(s, d), gn_emulate(s, d)
        uS, uQ = gn_sum_units(s, o)
        return max(ratio((e.S - o.S).abs(), uS), ratio((e.Q - o.Q).abs(), uQ))
    if s.kind == "ln":
        o, e = ln_oracle(s, d), ln_emulate(s, d)
        dm = e.mean.double() - o.mean
        var_k = o.var + dm * dm
        return max(ratio(dm.abs(), ln_mean_unit(s, o)), ratio((e.qv.double() - var_k).abs(), U * (math.sqrt(ln_depth(s)) + 3) * var_k))
    if s.kind == "time":     # the frequency allowance is not a rounding of the kernel's: it stays out of the measurement
        o = time_oracle(s, d)
        t0, t1 = time_tol(s, d, o, 0.0, freq=0.0), time_tol(s, d, o, 1.0, freq=0.0)     # the bound of the product t * f taken off first
        return ratio(((time_emulate(s, d).double() - o.ref).abs() - t0).clamp_min(0.0), t1 - t0)
    return emulated_ratio(key, s, d, m=1.0)


P = 1 << 20      # a non-null placeholder address: a refused call reads nothing


def refused(lib_ptr=lambda name: P):
    """[(name, entry point, argument tuple)]: calls the library must answer with PF_EINVAL before any launch; `lib_ptr(name)` gives the
    address of a buffer (placeholders by default - the CPU test; the GPU test passes guarded buffers and checks they stay untouched)"""
    p = lib_ptr
    big = 1 << 22      # scratch_bytes: the 2^20 floats the GPU test really passes
    return [
        ("gn C=1028", "pf_gn_scale_shift", (p("x"), 1028, 0, 0, 1, 16, 4, 1e-5, p("v"), p("v"), p("out"), p("out2"), p("scratch"), big, 0)),
        ("gn c0 % 4", "pf_gn_scale_shift", (p("x"), 30, p("x"), 34, 1, 16, 32, 1e-5, p("v"), p("v"), p("out"), p("out2"), p("scratch"), big, 0)),
        ("ln_stats C % 4", "pf_ln_stats", (p("x"), 4, 30, 1e-5, p("out"), p("out2"), 0)),
        ("ln_planes C % 4", "pf_ln_planes", (p("x"), 4, 30, 1e-5, p("v"), p("v"), p("out"), 0)),
        ("ln_planes C=2048", "pf_ln_planes", (p("x"), 4, 2048, 1e-5, p("v"), p("v"), p("out"), 0)),
        ("stem 8>256", "pf_conv_in", (p("x"), p("v"), p("v"), p("out"), 1, 8, 256, 4, 4, 0, 0)),
        ("stem stats on the generic kernel", "pf_conv_in", (p("x"), p("v"), p("v"), p("out"), 1, 3, 64, 16, 16, p("out2"), 0)),
        ("head cout=5", "pf_conv_out", (p("x"), p("v"), p("v"), p("v"), p("v"), p("out"), 1, 16, 5, 4, 4, 0)),
        ("head cin=24", "pf_conv_out", (p("x"), p("v"), p("v"), p("v"), p("v"), p("out"), 1, 24, 2, 4, 4, 0)),
        ("time odd channels", "pf_time_embed", (0, p("v"), p("v"), p("v"), p("v"), p("out"), 2, 33, 64, 0)),
        ("matvec K=2080", "pf_matvec", (p("x"), 2080, p("v"), p("v"), p("out"), 8, 2, 8, 2080, 0, 0, 0, 0)),
    ]
