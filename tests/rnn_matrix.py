"""The recurrent-kernel case matrix: the GRU cell updates of the encoders (gru_gates_kernel, gru_gates_masked_kernel: pf_gru_gates), the
fused GRU step of the decoders (gru_step_kernel: pf_gru_step), the three condition encoders end to end (csrc/encoders.hip with the embed,
length and texture kernels of csrc/small_kernels.hip) and the greedy walks of the chord and PianoTree decoders (csrc/decoders.hip), each with

  * a case table (cases(kind)) whose every case names the branches it exists for (`why`; branches() derives them from the shape),
  * a float64 oracle written from the recurrence - the whole encoders are oracle/encoders_ref.py, the decodes
    tests/test_decoders_host.restate_*, used here and not restated,
  * an fp32 emulator of the kernels' own arithmetic - the fmaf chains of matvec_kernel (8 lanes an output) and wave_dot (64 lanes), their
    fixed shuffle trees, the separately rounded gi + gh, 1 / (1 + exp(-v)) - with a `defect=` switch (DEFECTS); the PianoTree decode's
    emulator keeps the walk, the bind-time token tables, the decision rules and the lane structure of the dots, with every lane's short
    chain taken exactly and rounded once (pn_emulate says why), and
  * a per-element tolerance: a unit built from the case's own float64 magnitudes, the dot lengths and the number of steps, times the
    constant of profiles/rnn_error_model.md.

Host only: imports no GPU code.  Used by tests/test_rnn_matrix.py (no GPU), tests/test_gpu_rnn_matrix.py (-m gpu) and
tools/rnn_error_model.py, which measures the constants below on the CPU (emulator against oracle; the tests use 4 times that: the
hardware's expf, tanhf, division and contraction choices may differ from numpy's by an ulp or two per operation).  No constant comes from
a GPU."""
from __future__ import annotations

import functools
import math
import os
import sys

import numpy as np
import torch

from small_matrix import MARGIN, U, Result, Spec, _butterfly, cdiv, f32, f64, fma32, ratio, rng_of  # noqa: F401

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle import encoders_ref as eref  # noqa: E402

# measured by tools/rnn_error_model.py, recorded in profiles/rnn_error_model.md (largest emulator ratio, rounded up to two decimals)
MEASURED = {"gates": 0.62, "step": 0.46, "enc_chord": 0.12, "enc_texture": 0.29, "enc_pnotree": 0.02, "dec_chord": 0.17, "dec_pnotree": 0.12}
M = {k: MARGIN * v for k, v in MEASURED.items()}
TINY = 2.0 ** -126      # a sigmoid below fp32's normal range is 0 on the kernel's side (expf overflows, or the quotient flushes)


# =====================================================================================================================================
# The cell: r = sigmoid(a_r + c_r), z = sigmoid(a_z + c_z), n = tanh(a_n + r c_n), h' = (1 - z) n + z h   (a = gi, c = gh)
# =====================================================================================================================================
def sig32(v):
    """1.0f / (1.0f + expf(-v)): exp and the quotient correctly rounded here; an overflowing exp gives 1 / inf = 0"""
    with np.errstate(over="ignore"):
        e = np.exp(-v.astype(f64)).astype(f32)
        return (1.0 / (f32(1.0) + e).astype(f64)).astype(f32)


def tanh32(v):
    return np.tanh(v.astype(f64)).astype(f32)


def cell32(ar, az, an, cr, cz, cn, h, defect=None, bn=None):
    """the update as the kernels write it, every operation rounded to fp32.  bn: the n gate's b_hh where the caller still has it apart"""
    if defect == "rz_swapped":
        ar, az, cr, cz = az, ar, cz, cr
    r, z = sig32(ar + cr), sig32(az + cz)
    if defect == "bhh_outside" and bn is not None:
        n = tanh32(an + r * (cn - bn) + bn)
    else:
        n = tanh32(an + r * cn)
    return ((f32(1.0) - z) * n + z * h).astype(f32)


def cell64(ar, az, an, cr, cz, cn, h, d_r=0.0, d_z=0.0, d_an=0.0, d_cn=0.0):
    """(h', unit) in float64 (torch).  unit: what the constant multiplies - the first-order image of the input errors d_* of the four
    pre-activation parts and of the cell's own roundings: one per sum, three per sigmoid (exp, sum, quotient), two per tanh, and the
    products and sums of the blend.  dh'/dz = h - n."""
    vr, vz = ar + cr, az + cz
    r, z = torch.sigmoid(vr), torch.sigmoid(vz)
    arg = an + r * cn
    n = torch.tanh(arg)
    out = (1 - z) * n + z * h
    dr = r * (1 - r) * (d_r + U * vr.abs()) + 3 * U * r + TINY
    dz = z * (1 - z) * (d_z + U * vz.abs()) + 3 * U * z + TINY
    darg = d_an + r * d_cn + cn.abs() * dr + U * ((r * cn).abs() + arg.abs())
    dn = (1 - n * n) * darg + 2 * U * n.abs()
    unit = (n - h).abs() * dz + (1 - z) * dn + U * (2 * ((1 - z) * n).abs() + (z * h).abs() + out.abs())
    return out, unit


def dot_unit(depth, t2, ref):
    """the rounding of a dot product summed in fp32 over `depth` additions on an element's path (chain and shuffle tree): each relative to
    a partial sum, which for signed terms is of the size of sqrt(sum (w x)^2) = t2, and for terms of one sign of the size of the sum itself"""
    return U * (math.sqrt(depth) * (t2 + ref.abs()) + 2 * ref.abs())


def _lin64(x, w, b=None):
    """(y, t2) = (x w^T + b, sqrt(sum_k (w x)^2 + b^2)) in float64"""
    y = x @ w.t()
    t2 = (x * x) @ (w * w).t()
    if b is not None:
        y, t2 = y + b, t2 + b * b
    return y, torch.sqrt(t2)


def wave_dot32(w, x, vec):
    """wave_dot of decoders.hip, [R][N] fp32: lane l of 64 takes the float4s at k = 4 l + 256 i (x, y, z, w in turn; the vector form) or
    the elements k = l + 64 i as one fmaf chain from 0, then the shuffle tree"""
    N, K = w.shape
    R = x.shape[0]
    wz, xz = np.concatenate([w, np.zeros((N, 1), f32)], 1), np.concatenate([x, np.zeros((R, 1), f32)], 1)
    if vec:
        order = [[k + e for k in range(4 * lane, K, 256) for e in range(4)] for lane in range(64)]
    else:
        order = [list(range(lane, K, 64)) for lane in range(64)]
    steps = max(len(o) for o in order)
    idx = np.array([o + [K] * (steps - len(o)) for o in order], np.int64).reshape(64, steps)
    acc = np.zeros((R, N, 64), f32)
    for i in range(steps):
        kk = idx[:, i]
        acc = fma32(wz[None, :, kk], xz[:, None, kk], acc)
    return _butterfly(acc)


def matvec32(x, w, bias=None, exp=False):
    """matvec_kernel of small_kernels.hip, [B][N] fp32: the 8 lanes of an output take the float4s q = j, j + 8, ... (K % 32 == 0; the rows
    the encoders pass are 16-byte aligned) or the elements k = j, j + 8, ... as one fmaf chain each, then ((l0 + l1) + (l2 + l3)) +
    ((l4 + l5) + (l6 + l7)), the bias, expf"""
    N, K = w.shape
    B = x.shape[0]
    wz, xz = np.concatenate([w, np.zeros((N, 1), f32)], 1), np.concatenate([x, np.zeros((B, 1), f32)], 1)
    if K % 32 == 0:
        order = [[q * 4 + e for q in range(j, K // 4, 8) for e in range(4)] for j in range(8)]
    else:
        order = [list(range(j, K, 8)) for j in range(8)]
    steps = max(len(o) for o in order)
    idx = np.array([o + [K] * (steps - len(o)) for o in order], np.int64).reshape(8, steps)
    out = np.zeros((B, N), f32)
    rb = max(1, (1 << 22) // (N * 8))                 # rows at a time: the accumulators stay a few tens of megabytes
    for b0 in range(0, B, rb):
        acc = np.zeros((min(rb, B - b0), N, 8), f32)
        for i in range(steps):
            kk = idx[:, i]
            acc = fma32(wz[None, :, kk], xz[b0:b0 + rb, None, kk], acc)
        t = acc[..., 0::2] + acc[..., 1::2]
        t = t[..., 0::2] + t[..., 1::2]
        out[b0:b0 + rb] = t[..., 0] + t[..., 1]
    if bias is not None:
        out = out + bias
    return np.exp(out.astype(f64)).astype(f32) if exp else out.astype(f32)


def _regime_gate_inputs(rng, shape, regime):
    """a pre-activation part of the given shape: benign N(0, 1); saturated: magnitudes in [31, 99], random signs"""
    if regime == "saturated":
        return (rng.uniform(31.0, 99.0, shape) * rng.choice([-1.0, 1.0], shape)).astype(f32)
    return rng.standard_normal(shape).astype(f32)


# =====================================================================================================================================
# gates: pf_gru_gates (gru_gates_kernel, gru_gates_masked_kernel)
# =====================================================================================================================================
GATES_SHAPES = ((1, 4), (3, 20), (9, 100), (17, 512))
GATES_REGIMES = ("benign", "saturated", "hbig")
GATES_DEFECTS = ("rz_swapped", "masked_reverse_S", "masked_step_le")


def _gates(rows, hidden, regime="benign", t_steps=1, t=0, seq_len=0, step=0, reverse=0, why=()):
    s = Spec(kind="gates", rows=rows, hidden=hidden, regime=regime, t_steps=t_steps, t=t, seq_len=seq_len, step=step, reverse=reverse,
             why=tuple(why))
    key = f"gates {rows}x{hidden} {regime}" + (f" T{t_steps} t{t}" if t_steps > 1 else "")
    return key + (f" masked S{seq_len} step{step} {'rev' if reverse else 'fwd'}" if seq_len else ""), s


def gates_lens(s):
    """the lengths of a masked case: 0, 1 and seq_len next to each other (three rows of <= 85 hidden units share a 256-thread block), then
    one in between"""
    cyc = (0, 1, s.seq_len, (s.seq_len + 1) // 2)
    return np.array([cyc[i % 4] for i in range(s.rows)], np.int32)


def gates_branches(s):
    out = {f"shape:{s.rows}x{s.hidden}", f"regime:{s.regime}"}
    n = s.rows * s.hidden
    out.add("below_one_block" if n < 256 else "ragged_last_block" if n % 256 else "full_blocks")
    if s.seq_len:
        lens = gates_lens(s)
        out |= {"masked", f"S:{s.seq_len}", "reverse" if s.reverse else "forward"}
        if (lens == s.step).any():
            out.add("step_eq_len")
        if (lens - 1 == s.step).any():
            out.add("step_last")
        if s.step == 0:
            out.add("step_0")
        if (lens <= s.step).any():
            out.add("rows_kept")
        if s.rows >= 3 and 2 * s.hidden < 256:      # row 2 (length seq_len) starts inside the block of rows 0 and 1
            out.add("lens_mixed_in_a_block")
    else:
        out.add("ld_gi_step_offset" if s.t_steps > 1 else "ld_gi_3H")
    return out


GATES_REQUIRED = ({f"shape:{r}x{h}" for r, h in GATES_SHAPES} | {f"regime:{r}" for r in GATES_REGIMES}
                  | {"below_one_block", "ragged_last_block", "full_blocks", "ld_gi_3H", "ld_gi_step_offset", "masked", "S:1", "S:3", "S:32",
                     "forward", "reverse", "step_eq_len", "step_last", "step_0", "rows_kept", "lens_mixed_in_a_block"})


def gates_cases():
    out = []
    for i, (r, h) in enumerate(GATES_SHAPES):
        for j, regime in enumerate(GATES_REGIMES):
            ts, t = ((1, 0), (3, 2), (3, 1))[(i + j) % 3]
            out.append(_gates(r, h, regime, ts, t, why=(f"shape:{r}x{h}", f"regime:{regime}", "ld_gi_step_offset" if ts > 1 else "ld_gi_3H")))
    for S, steps in ((1, (0,)), (3, (0, 1, 2, 3)), (32, (0, 1, 15, 31))):
        for step in steps:
            for rev in (0, 1):
                r, h = ((9, 100), (3, 20))[(step + rev) % 2] if S != 32 else (9, 100)
                out.append(_gates(r, h, "benign", seq_len=S, step=step, reverse=rev,
                                  why=("masked", f"S:{S}", "reverse" if rev else "forward", "rows_kept")))
    out.append(_gates(17, 512, "saturated", seq_len=3, step=1, reverse=1, why=("masked", "regime:saturated", "step_eq_len")))
    return out


def gates_inputs(key, s):
    """gi [rows][T][3H] (T = seq_len, or the steps of the unmasked layout), gh [rows][3H], h [rows][H]"""
    rng = rng_of(key)
    T, H = (s.seq_len or s.t_steps), s.hidden
    gi = _regime_gate_inputs(rng, (s.rows, T, 3 * H), s.regime)
    gh = (0.5 * rng.standard_normal((s.rows, 3 * H))).astype(f32)
    h = rng.uniform(-1.0, 1.0, (s.rows, H)).astype(f32)
    if s.regime == "saturated":
        gi[:, :, 0] = f32(-95.0)          # below -88.8: expf(-v) overflows, r = 1 / inf
        gi[:, :, H] = f32(-93.0)
    if s.regime == "hbig":
        h = h * f32(1e3)
    d = {"gi": torch.from_numpy(gi), "gh": torch.from_numpy(gh), "h": torch.from_numpy(h)}
    if s.seq_len:
        d["lens"] = torch.from_numpy(gates_lens(s))
    return d


def _gates_rows(s, d, defect=None):
    """(t [rows], active [rows], ok): the element of gi each row reads, which rows take part, and whether every read stays inside gi"""
    if not s.seq_len:
        return np.full(s.rows, s.t), np.ones(s.rows, bool), True
    lens = d["lens"].numpy().astype(np.int64)
    active = s.step <= lens if defect == "masked_step_le" else s.step < lens
    if s.reverse:
        t = (np.full(s.rows, s.seq_len) if defect == "masked_reverse_S" else lens) - 1 - s.step
    else:
        t = np.full(s.rows, s.step)
    ok = bool(((t >= 0) & (t < s.seq_len))[active].all())
    return np.clip(t, 0, s.seq_len - 1), active, ok


def _thirds(a, H):
    return a[..., :H], a[..., H:2 * H], a[..., 2 * H:]


def gates_oracle(s, d):
    t, active, _ = _gates_rows(s, d)
    H = s.hidden
    a = d["gi"].double()[torch.arange(s.rows), torch.from_numpy(t)]
    h = d["h"].double()
    out, unit = cell64(*_thirds(a, H), *_thirds(d["gh"].double(), H), h)
    act = torch.from_numpy(active)[:, None]
    return Result(ref=torch.where(act, out, h), unit=torch.where(act, unit, torch.zeros_like(unit)))


def gates_emulate(s, d, defect=None):
    t, active, ok = _gates_rows(s, d, defect)
    H = s.hidden
    a, h = d["gi"].numpy()[np.arange(s.rows), t], d["h"].numpy()
    out = cell32(*_thirds(a, H), *_thirds(d["gh"].numpy(), H), h, defect)
    return torch.from_numpy(np.where(active[:, None], out, h)), ok


def gates_ratio(s, o, got, m=None):
    """a row that takes no part has tolerance 0: it keeps its bits"""
    assert bool(torch.isfinite(got).all()), "a gate update is not finite"
    return ratio((got.double() - o.ref).abs(), (M["gates"] if m is None else m) * o.unit)


# =====================================================================================================================================
# step: pf_gru_step (gru_step_kernel)
# =====================================================================================================================================
STEP_DEFECTS = ("rz_swapped", "bhh_outside", "ld2_ignored")
STEP_H, STEP_KX, STEP_R = (4, 96, 512, 1024), (0, 36, 256), (1, 8, 9, 17)
WX_PAD, WX_OFF = 8, 4       # Wx is a column slice: rows WX_PAD floats wider than Kx, the slice WX_OFF floats in


def _step(H, Kx, R, add1=1, add2=0, ld2=0, ldx0=0, regime="benign", why=()):
    s = Spec(kind="step", H=H, Kx=Kx, R=R, add1=add1, add2=add2, ld2=ld2, ldx0=ldx0, regime=regime, why=tuple(why))
    key = f"step H{H} Kx{Kx} R{R}" + (" add1" if add1 else "") + (f" add2/ld{'3H' if ld2 else '0'}" if add2 else "")
    return key + (" x-broadcast" if ldx0 else "") + ("" if regime == "benign" else f" {regime}"), s


def step_branches(s):
    out = {f"H:{s.H}", f"Kx:{s.Kx}", f"R:{s.R}", f"regime:{s.regime}"}
    out.add("add1" if s.add1 else "add1_null")
    out.add(("add2_ld3H" if s.ld2 else "add2_broadcast") if s.add2 else "add2_null")
    if s.R > 8:
        out.add("second_row_tile")
    if s.R % 8:
        out.add("partial_row_tile")
    if s.Kx:
        out.add("wx_column_slice")
        out.add("x_broadcast" if s.ldx0 else "x_per_row")
    if s.H > 64:
        out.add("vector_dot_several_lanes")
    if s.H > 256:
        out.add("vector_dot_several_passes")
    if s.R == 17:
        out.add("rows_alone")
    return out


STEP_REQUIRED = ({f"H:{h}" for h in STEP_H} | {f"Kx:{k}" for k in STEP_KX} | {f"R:{r}" for r in STEP_R}
                 | {"regime:benign", "regime:saturated", "add1", "add1_null", "add2_null", "add2_broadcast", "add2_ld3H", "second_row_tile",
                    "partial_row_tile", "wx_column_slice", "x_broadcast", "x_per_row", "vector_dot_several_lanes", "vector_dot_several_passes",
                    "rows_alone"})


def step_cases():
    return [
        _step(4, 0, 1, why=("H:4", "Kx:0", "R:1", "add2_null")),
        _step(4, 36, 9, add1=0, why=("H:4", "Kx:36", "R:9", "add1_null")),
        _step(96, 36, 8, add2=1, ld2=0, why=("H:96", "R:8", "add2_broadcast")),
        _step(96, 256, 17, add2=1, ld2=1, why=("Kx:256", "R:17", "add2_ld3H", "rows_alone")),
        _step(96, 36, 9, regime="saturated", why=("regime:saturated", "partial_row_tile")),
        _step(512, 0, 17, add2=1, ld2=0, why=("H:512", "R:17", "add2_broadcast", "rows_alone")),        # the notes GRU's first slot
        _step(512, 0, 9, add2=1, ld2=1, regime="saturated", why=("H:512", "regime:saturated", "add2_ld3H")),
        _step(1024, 256, 17, why=("H:1024", "Kx:256", "R:17", "rows_alone", "vector_dot_several_passes")),     # the time GRU
        _step(1024, 256, 9, ldx0=1, why=("H:1024", "x_broadcast", "second_row_tile")),                          # its first step
    ]


def step_inputs(key, s):
    rng = rng_of(key)
    H, Kx, R = s.H, s.Kx, s.R
    b = 1.0 / math.sqrt(H)
    u = lambda *shape: rng.uniform(-b, b, shape).astype(f32)  # noqa: E731
    d = {"wh": u(3 * H, H), "b_hh": u(3 * H), "h_in": rng.uniform(-1.0, 1.0, (R, H)).astype(f32)}
    if Kx:
        d["wx_wide"] = u(3 * H, Kx + WX_PAD)
        d["x"] = rng.uniform(0.0, 1.0, (1 if s.ldx0 else R, Kx)).astype(f32)
    if s.add1:
        d["add1"] = _regime_gate_inputs(rng, (R, 3 * H), s.regime)
        if s.regime == "saturated":
            d["add1"][:, 0] = f32(-95.0)
            d["add1"][:, H] = f32(-93.0)
    if s.add2:
        d["add2"] = (0.3 * rng.standard_normal((R if s.ld2 else 1, 3 * H))).astype(f32)
    return {k: torch.from_numpy(v) for k, v in d.items()}


def _step_wx(d, s):
    return d["wx_wide"][:, WX_OFF:WX_OFF + s.Kx]


def step_oracle(s, d):
    H, R = s.H, s.R
    h = d["h_in"].double()
    gh, th = _lin64(h, d["wh"].double(), d["b_hh"].double())
    gi, ti2 = torch.zeros(R, 3 * H, dtype=torch.float64), torch.zeros(R, 3 * H, dtype=torch.float64)
    if s.Kx:
        gi, ti = _lin64(d["x"].double().expand(R, s.Kx), _step_wx(d, s).double())
        ti2 = ti * ti
    for name in ("add1", "add2"):
        if name in d:
            a = d[name].double().expand(R, 3 * H)
            gi, ti2 = gi + a, ti2 + a * a
    dgh = dot_unit(cdiv(H, 256) * 4 + 6 + 1, th, gh)
    dgi = dot_unit((cdiv(s.Kx, 64) + 6 if s.Kx else 0) + 2, torch.sqrt(ti2), gi)
    (dhr, dhz, dhn), (dir_, diz, din) = _thirds(dgh, H), _thirds(dgi, H)
    out, unit = cell64(*_thirds(gi, H), *_thirds(gh, H), h, dhr + dir_, dhz + diz, din, dhn)
    return Result(ref=out, unit=unit)


def step_emulate(s, d, defect=None):
    """(h_out, ok): gh by the vector wave_dot over H, gi by the scalar one over Kx, add1 then add2 added to gi, b_hh to gh, the cell"""
    g = lambda n: d[n].numpy() if n in d else None  # noqa: E731
    ok = not (defect == "ld2_ignored" and s.add2 and not s.ld2 and s.R > 1)      # rows 1.. read 3H floats further on each: outside the one row
    wx = np.ascontiguousarray(_step_wx(d, s).numpy()) if s.Kx else None
    return torch.from_numpy(gru_step32(g("x"), wx, g("h_in"), g("wh"), g("b_hh"), g("add1"), g("add2"), defect)), ok


def gru_step32(x, wx, h, wh, bh, add1, add2, defect=None):
    """gru_step_kernel in fp32; x, add1, add2 may be None, and one row of x / add2 stands for every row (a stride of 0)"""
    R, H = h.shape
    gh = wave_dot32(wh, h, True)
    gi = np.zeros((R, 3 * H), f32)
    if x is not None:
        gi = wave_dot32(wx, np.broadcast_to(x, (R, x.shape[1])), False)
    if add1 is not None:
        gi = gi + add1
    if add2 is not None:
        gi = gi + np.broadcast_to(add2, (R, 3 * H))
    return cell32(*_thirds(gi, H), *_thirds(gh + bh, H), h, defect, bn=bh[2 * H:])


def step_ratio(s, o, got, m=None):
    assert bool(torch.isfinite(got).all()), "a GRU step is not finite"
    return ratio((got.double() - o.ref).abs(), (M["step"] if m is None else m) * o.unit)


# =====================================================================================================================================
# enc: the three encoders end to end (ChordEncoder, TextureEncoder, PianoTreeEncoder of polyffusion_amd.model_sdf)
# =====================================================================================================================================
ENC_DEFECTS = ("rz_swapped", "bhh_outside", "masked_reverse_S", "masked_step_le", "dir1_into_half0", "pad_column")
PN_P = 130      # pitch classes; the pad index, which has no column


def _enc(enc, b, with_scale=0, why=(), **sizes):
    s = Spec(kind="enc", enc=enc, b=b, with_scale=with_scale, why=tuple(why), **sizes)
    key = f"enc {enc} " + " ".join(f"{k}{v}" for k, v in sizes.items()) + f" B{b}" + (" scale" if with_scale else "")
    return key, s


def enc_sub(s):
    return "enc_" + s.enc


def enc_gru_shapes(s):
    """[(rows, steps, hidden, K of the input projection)] of the encoder's GRUs"""
    if s.enc == "chord":
        return [(s.b, s.T, s.H, s.inp)]
    if s.enc == "texture":
        return [(s.b, 8, s.H, s.emb)]
    return [(s.b * 32, s.S, s.Hn, s.emb), (s.b, 32, s.Ht, 2 * s.Hn)]


def enc_branches(s):
    out = {f"{s.enc}", f"{s.enc}:B{s.b}"}
    for rows, steps, H, K in enc_gru_shapes(s):
        out.add("gates_below_one_block" if rows * H < 256 else "gates_ragged_block" if rows * H % 256 else "gates_full_blocks")
        out.add("hh_scalar_path" if H % 32 else "hh_vector_path")
        out.add("ih_scalar_path" if K % 32 else "ih_vector_path")
    if s.with_scale:
        out.add("with_scale")
    if s.enc == "chord":
        out |= {f"T:{s.T}", f"input_dim:{s.inp}"}
    if s.enc == "texture":
        out |= {f"num_channel:{s.C}", "roll_zero" if s.b >= 2 else "roll_sparse_only"}
        if s.b >= 2:
            out.add("roll_dense")
    if s.enc == "pnotree":
        out |= {f"S:{s.S}", "len_0", "len_1", "len_S", "pads_between_notes", "pitch_0_and_129"}
    if s.b in (9, 17):
        out.add("rows_alone")
    return out


ENC_REQUIRED = {"chord", "texture", "pnotree", "T:1", "T:5", "T:32", "T:64", "input_dim:32", "input_dim:36", "num_channel:1", "num_channel:3",
                "num_channel:10", "S:3", "S:32", "S:20", "with_scale", "hh_scalar_path", "hh_vector_path", "ih_scalar_path", "ih_vector_path",
                "gates_below_one_block", "gates_ragged_block", "gates_full_blocks", "roll_zero", "roll_dense", "len_0", "len_1", "len_S",
                "pads_between_notes", "pitch_0_and_129", "rows_alone", "chord:B9", "chord:B1", "chord:B17", "chord:B8", "texture:B1",
                "texture:B9", "texture:B2", "pnotree:B3", "pnotree:B2"}


def enc_cases():
    return [
        _enc("chord", 9, inp=36, H=20, z=12, T=64, why=("T:64", "hh_scalar_path", "ih_scalar_path", "rows_alone", "gates_below_one_block")),
        _enc("chord", 1, inp=32, H=32, z=32, T=1, why=("T:1", "input_dim:32", "hh_vector_path", "ih_vector_path")),
        _enc("chord", 17, 1, inp=36, H=100, z=33, T=5, why=("T:5", "with_scale", "rows_alone", "gates_ragged_block")),
        _enc("chord", 8, 1, inp=36, H=512, z=512, T=32, why=("T:32", "with_scale", "gates_full_blocks")),
        _enc("texture", 1, emb=20, H=36, z=7, C=1, why=("num_channel:1", "hh_scalar_path", "gates_below_one_block")),
        _enc("texture", 9, emb=32, H=64, z=16, C=3, why=("num_channel:3", "roll_zero", "roll_dense", "rows_alone")),
        _enc("texture", 2, 1, emb=256, H=1024, z=256, C=10, why=("num_channel:10", "with_scale", "roll_zero", "roll_dense")),
        _enc("pnotree", 3, emb=16, Hn=12, Ht=20, z=8, S=3, why=("S:3", "len_0", "len_1", "len_S", "pads_between_notes", "hh_scalar_path")),
        _enc("pnotree", 3, emb=32, Hn=36, Ht=64, z=16, S=32, why=("S:32", "len_0", "len_1", "len_S", "pads_between_notes")),
        _enc("pnotree", 2, emb=128, Hn=256, Ht=512, z=512, S=20, why=("S:20", "pitch_0_and_129", "pads_between_notes")),
    ]


@functools.lru_cache(maxsize=None)
def _enc_state(key):
    from polyffusion_amd import weights
    s = dict(enc_cases())[key]
    if s.enc == "chord":
        return weights.synth_chord_encoder_state(7, s.inp, s.H, s.z)
    if s.enc == "texture":
        return weights.synth_texture_encoder_state(7, s.emb, s.H, s.z, s.C)
    return weights.synth_pianotree_encoder_state(7, PN_P + 5, s.emb, s.Hn, s.Ht, s.z)


def pnotree_grid(rng, b, S):
    """[b][32][S][6] int64.  Song 0: the lengths of its steps cycle 0, 1, S.  Song 1: pads BETWEEN notes (note, pad, note, ...).  The others:
    lengths drawn from 0..S, notes first.  Pitch indices span 0..129 (both ends forced); digits 0 / 1; a pad entry is (130, 2 2 2 2 2)."""
    g = np.zeros((b, 32, S, 6), np.int64)
    g[..., 0] = rng.integers(0, PN_P, (b, 32, S))
    g[..., 1:] = rng.integers(0, 2, (b, 32, S, 5))
    pad = np.zeros((b, 32, S), bool)
    for t in range(32):
        pad[0, t, (0, 1, S)[t % 3]:] = True
        if b > 1:
            pad[1, t, 1::2] = True
            if t % 4 == 3:
                pad[1, t, 0] = True
        for k in range(2, b):
            pad[k, t, rng.integers(0, S + 1):] = True
    g[b - 1, 5, 0, 0], g[b - 1, 6, 0, 0] = 0, PN_P - 1
    pad[b - 1, 5:7, 0] = False
    g[pad] = np.array([PN_P, 2, 2, 2, 2, 2])
    return g


def enc_inputs(key, s):
    rng = rng_of(key)
    if s.enc == "chord":
        x = (rng.random((s.b, s.T, s.inp)) < 0.3).astype(f32)
    elif s.enc == "texture":
        x = ((rng.random((s.b, 32, 128)) < 0.06) * rng.integers(1, 9, (s.b, 32, 128))).astype(f32)
        if s.b >= 2:
            x[0], x[1] = 0.0, 1.0 + (rng.random((32, 128)) < 0.5)
    else:
        x = pnotree_grid(rng, s.b, s.S)
    return {"x": torch.from_numpy(x), "state": _enc_state(key)}


def _w64(state):
    return {k: torch.from_numpy(np.asarray(v)).double() for k, v in state.items()}


def enc_oracle(s, d):
    """mu (and scale = exp(linear_var(h))) by oracle/encoders_ref.py on double; unit: see enc_unit"""
    w = _w64(d["state"])
    x = d["x"]
    if s.enc == "pnotree":
        mu = eref.pianotree_encoder_mean(w, x, PN_P)
    elif s.enc == "texture":
        mu = eref.texture_encoder_mean(w, x.double())
    else:
        mu = eref.chord_encoder_mean(w, x.double())
    o = Result(mu=mu, unit_mu=enc_unit(s, w["linear_mu.weight"], mu))
    if s.with_scale:
        # the state before linear_mu is not returned by the reference restatement: recovered through its own bigru_final
        if s.enc == "chord":
            h = eref.bigru_final(w, "gru.", x.double())
        else:
            y = torch.nn.functional.conv2d(x.double().unsqueeze(1), w["cnn.0.weight"], w["cnn.0.bias"], stride=(4, 1))
            y = torch.nn.functional.max_pool2d(torch.relu(y), (1, 4), (1, 4)).reshape(s.b, 8, -1)
            y = torch.nn.functional.linear(torch.nn.functional.linear(y, w["fc1.weight"], w["fc1.bias"]), w["fc2.weight"], w["fc2.bias"])
            h = eref.bigru_final(w, "gru.", y)
        lin = torch.nn.functional.linear(h, w["linear_var.weight"], w["linear_var.bias"])
        o["scale"] = torch.exp(lin)
        o["unit_scale"] = o["scale"] * enc_unit(s, w["linear_var.weight"], lin)
    return o


def enc_unit(s, w_out, out):
    """what the constant multiplies, per element of an output W h + b.  A GRU step leaves in every |h| <= 1 an error of the size of its
    pre-activations' rounding, U sqrt(depth of the W_hh dot); the steps' errors add in quadrature, sqrt(steps); a row of W carries them
    to the output in quadrature too, ||W row||_2.  The PianoTree encoder's note GRU feeds the time GRU: both terms.  On top, the output's
    own dot over 2H (||W row||_2 bounds sqrt(sum (w h)^2)) and its two roundings."""
    acc = 0.0
    for rows, steps, H, K in enc_gru_shapes(s):
        acc += steps * (cdiv(H, 8) + 3 + cdiv(K, 8) + 3)
    wn = torch.sqrt((w_out * w_out).sum(1))[None, :]
    d_out = cdiv(w_out.shape[1], 8) + 3
    return U * (math.sqrt(acc) * wn + math.sqrt(d_out) * (wn + out.abs()) + 2 * out.abs())


def bigru32(g, x, H, lens=None, defect=None):
    """bigru of encoders.hip in fp32: per direction the input projection of every step (one mat-vec over R T rows), then per step the W_hh
    mat-vec and the gate update; [R][2H].  lens: the masked (packed) form."""
    R, T, K = x.shape
    hcat = np.zeros((R, 2 * H), f32)
    ok = True
    for dr in (0, 1):
        sfx = "_reverse" if dr else ""
        w_ih, w_hh, b_ih, b_hh = (np.asarray(g[n + sfx], f32) for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"))
        gi = matvec32(x.reshape(R * T, K), w_ih, b_ih).reshape(R, T, 3 * H)
        half = 0 if defect == "dir1_into_half0" else dr
        for step in range(T):
            h = hcat[:, half * H:(half + 1) * H]
            gh = matvec32(hcat[:, dr * H:(dr + 1) * H], w_hh, b_hh)
            if lens is None:
                t, active = np.full(R, T - 1 - step if dr else step), np.ones(R, bool)
            else:
                active = step <= lens if defect == "masked_step_le" else step < lens
                t = ((np.full(R, T) if defect == "masked_reverse_S" else lens) - 1 - step) if dr else np.full(R, step)
                ok = ok and bool(((t >= 0) & (t < T))[active].all())
                t = np.clip(t, 0, T - 1)
            new = cell32(*_thirds(gi[np.arange(R), t], H), *_thirds(gh, H), h, defect, bn=b_hh[2 * H:])
            hcat[:, half * H:(half + 1) * H] = np.where(active[:, None], new, h)
    return hcat, ok


def _gru_of(state, prefix):
    return {k[len(prefix):]: v for k, v in state.items() if k.startswith(prefix)}


def txt_frontend32(pr, w, bias):
    """txt_frontend_kernel: acc = bias, fmaf over the 4 x 12 taps (row, then column), the maximum of 4 neighbours and 0; [B][C][8][29]"""
    B, C = pr.shape[0], w.shape[0]
    rows = pr.reshape(B, 8, 4, 128)
    acc = np.broadcast_to(bias[None, :, None, None], (B, C, 8, 116)).astype(f32)
    for r in range(4):
        for c in range(12):
            acc = fma32(rows[:, None, :, r, c:c + 116], w[None, :, 0, r, c, None, None], acc)
    return np.maximum(acc.reshape(B, C, 8, 29, 4).max(-1), f32(0.0))


def enc_emulate(s, d, defect=None):
    """(Result(mu[, scale]), ok): the launches of enc_run in order, each in its kernel's arithmetic"""
    st = {k: np.asarray(v, f32) for k, v in d["state"].items()}
    x = d["x"].numpy()
    if s.enc == "chord":
        h, ok = bigru32(_gru_of(st, "gru."), x, s.H, None, defect)
    elif s.enc == "texture":
        feat = txt_frontend32(x, st["cnn.0.weight"], st["cnn.0.bias"]).reshape(s.b * 8, s.C * 29)     # the un-permuted view
        em = matvec32(matvec32(feat, st["fc1.weight"], st["fc1.bias"]), st["fc2.weight"], st["fc2.bias"])
        h, ok = bigru32(_gru_of(st, "gru."), em.reshape(s.b, 8, s.emb), s.H, None, defect)
    else:
        g = x.reshape(-1, 6)
        we, be = st["note_embedding.weight"], st["note_embedding.bias"]
        pitch = g[:, 0]
        has = pitch <= PN_P if defect == "pad_column" else pitch < PN_P
        acc = np.broadcast_to(be, (g.shape[0], s.emb)).astype(f32)
        acc = np.where(has[:, None], acc + we[:, np.minimum(pitch, PN_P)].T, acc)
        for k in range(5):
            acc = fma32(g[:, 1 + k, None].astype(f32), we[None, :, PN_P + k], acc)
        lens = s.S - (x[..., 0] == PN_P).sum(-1).reshape(-1)
        hn, ok = bigru32(_gru_of(st, "enc_notes_gru."), acc.reshape(s.b * 32, s.S, s.emb), s.Hn, lens, defect)
        h, ok2 = bigru32(_gru_of(st, "enc_time_gru."), hn.reshape(s.b, 32, 2 * s.Hn), s.Ht, None, defect)
        ok = ok and ok2
    out = Result(mu=torch.from_numpy(matvec32(h, st["linear_mu.weight"], st["linear_mu.bias"])))
    if s.with_scale:
        out["scale"] = torch.from_numpy(matvec32(h, st["linear_var.weight"], st["linear_var.bias"], exp=True))
    return out, ok


def enc_tol(s, o, m=None):
    m = M[enc_sub(s)] if m is None else m
    return m * o.unit_mu, (m * o.unit_scale + 2 * 2.0 ** -23 * o.scale) if s.with_scale else None


def enc_ratio(s, o, got, m=None):
    tm, ts = enc_tol(s, o, m)
    r = ratio((got.mu.double() - o.mu).abs(), tm)
    return max(r, ratio((got.scale.double() - o.scale).abs(), ts)) if s.with_scale else r


# =====================================================================================================================================
# dec: the chord decoder's greedy walk (pf_decoder_forward on PF_DEC_CHORD: dec_linear_kernel, gru_step_kernel, chord_heads_kernel)
# =====================================================================================================================================
DEC_DEFECTS = ("argmax_tie_high", "bit_tie_1", "rz_swapped", "bhh_outside")
GAP = 1e-3          # a row is used when every decision of its float64 decode is at least this clear
DRAWN = 48          # rows drawn per net, PCG64(404)
TIE_B = 9           # the tie net: root and bass row 9 are copies of the most frequent lower class; chroma pair 0 has equal rows


def _dec(zin, H, z, n, R, tie=0, why=()):
    s = Spec(kind="dec", zin=zin, H=H, z=z, n=n, R=R, tie=tie, why=tuple(why))
    return f"dec chord zin{zin} H{H} z{z} n{n} R{R}" + (" tie" if tie else ""), s


def dec_branches(s):
    out = {f"net:{s.zin}/{s.H}/{s.z}", f"n_step:{s.n}", f"R:{s.R}"}
    out.add("linear_vector_path" if s.z % 4 == 0 and s.zin % 4 == 0 else "linear_scalar_path")
    if s.R > 8:
        out |= {"second_row_tile", "rows_alone"}
    if s.tie:
        out |= {"root_tie", "bass_tie", "chroma_bit_tie"}
    if s.H == 1024 and s.z == 2048 and s.zin == 2048:
        out.add("largest_accepted")
    if s.H > 256:
        out.add("heads_strided_loop")
    return out


DEC_REQUIRED = {"net:12/96/20", "net:6/4/3", "net:256/512/256", "n_step:1", "n_step:5", "n_step:8", "R:1", "R:11", "R:17", "linear_vector_path",
                "linear_scalar_path", "second_row_tile", "rows_alone", "root_tie", "bass_tie", "chroma_bit_tie", "largest_accepted",
                "heads_strided_loop"}


def dec_cases():
    return [
        _dec(12, 96, 20, 5, 11, why=("net:12/96/20", "n_step:5", "R:11", "rows_alone")),
        _dec(6, 4, 3, 1, 1, why=("net:6/4/3", "n_step:1", "R:1", "linear_scalar_path")),
        _dec(256, 512, 256, 8, 17, why=("net:256/512/256", "n_step:8", "R:17", "rows_alone", "heads_strided_loop")),
        _dec(2048, 1024, 2048, 2, 1, why=("largest_accepted",)),
        _dec(12, 96, 20, 5, 11, tie=1, why=("root_tie", "bass_tie", "chroma_bit_tie")),
    ]


def _restate():
    import test_decoders_host as tdh      # the float64 restatement of the decoders the fixture pins to the reference
    return tdh


def _chord_gap(root, chroma, bass, tie):
    """per row: the smallest top-1 / top-2 gap over every decision; the tie net's duplicate columns are merged first"""
    if tie:
        keep = [i for i in range(12) if i != TIE_B]
        root, bass, chroma = root[..., keep], bass[..., keep], chroma[:, :, 1:]
    gaps = [(t[..., 0] - t[..., 1]).flatten(1).min(1).values for t in (torch.topk(root, 2, -1).values, torch.topk(bass, 2, -1).values)]
    gaps.append((chroma[..., 0] - chroma[..., 1]).abs().flatten(1).min(1).values)
    return torch.stack(gaps).min(0).values


@functools.lru_cache(maxsize=None)
def _dec_setup(key):
    """(state, z [R][z_dim] fp32, rows cleared of DRAWN, classes tied): the first R drawn rows whose float64 decode clears the gap"""
    from polyffusion_amd import weights
    s = dict(dec_cases())[key]
    state = dict(weights.synth_chord_decoder_state(7, 36, s.zin, s.H, s.z))
    z = np.random.Generator(np.random.PCG64(404)).standard_normal((DRAWN, s.z)).astype(f32)
    tdh, tied = _restate(), None
    if s.tie:
        root, _, bass = tdh.restate_chord(state, z, s.n)
        tied = []
        for name, logits in (("root_out", root), ("bass_out", bass)):
            a = int(torch.bincount(logits.argmax(-1).flatten(), minlength=12)[:TIE_B].argmax())
            for part in ("weight", "bias"):
                t = np.array(state[f"{name}.{part}"])
                t[TIE_B] = t[a]
                state[f"{name}.{part}"] = t
            tied.append(a)
        for part in ("weight", "bias"):
            t = np.array(state[f"chroma_out.{part}"])
            t[1] = t[0]
            state[f"chroma_out.{part}"] = t
    gap = _chord_gap(*tdh.restate_chord(state, z, s.n), s.tie)
    rows = torch.nonzero(gap >= GAP).flatten()
    return state, z[rows[:s.R].numpy()], int(rows.numel()), tied


def dec_inputs(key, s):
    state, z, cleared, tied = _dec_setup(key)
    return {"state": state, "z": torch.from_numpy(z), "cleared": cleared, "tied": tied}


def dec_steps_depth(s):
    """fp32 additions on an element's path through one GRU step: the W_hh dot, the token dot, add1 and the sums of the cell"""
    return cdiv(s.H, 256) * 4 + 6 + cdiv(36, 64) + 6 + 4


def dec_oracle(s, d):
    """logits and decisions of tests/test_decoders_host.restate_chord on double, and the unit of every logit: as enc_unit, with the state's
    bound max(1, |z2dec_hid(z)|) in the place of 1 and t + 1 steps behind the logits of step t"""
    tdh = _restate()
    root, chroma, bass = tdh.restate_chord(d["state"], d["z"].numpy(), s.n)
    w = _w64(d["state"])
    h0 = d["z"].double() @ w["z2dec_hid.weight"].t() + w["z2dec_hid.bias"]
    hs = max(1.0, float(h0.abs().max()))
    depth0 = 2 * (cdiv(max(s.z, s.zin), 256) * 4 + 6)
    steps = torch.arange(1, s.n + 1, dtype=torch.float64)[None, :, None]

    def unit(name, out):
        wn = torch.sqrt((w[f"{name}.weight"] ** 2).sum(1)).reshape((1, 1) + tuple(out.shape[2:]))
        return U * (torch.sqrt(steps.reshape((1, s.n) + (1,) * (out.dim() - 2)) * dec_steps_depth(s) + depth0) * wn * hs
                    + math.sqrt(cdiv(s.H, 64) + 7) * (wn * hs + out.abs()) + 2 * out.abs())
    return Result(root=root, chroma=chroma, bass=bass, grid=tdh.chord_grid(root, chroma, bass), gap=float(_chord_gap(root, chroma, bass, s.tie).min()),
                  unit_root=unit("root_out", root), unit_chroma=unit("chroma_out", chroma), unit_bass=unit("bass_out", bass))


def dec_tied_decisions(s, d, o):
    """decisions of the used rows the tie rules settle: root / bass arg-max at the duplicated class, and chroma pair 0 (always equal)"""
    if not s.tie:
        return 0
    a_root, a_bass = d["tied"]
    assert torch.equal(o.root[..., a_root], o.root[..., TIE_B]) and torch.equal(o.bass[..., a_bass], o.bass[..., TIE_B])
    assert torch.equal(o.chroma[:, :, 0, 0], o.chroma[:, :, 0, 1])
    return int((o.root.argmax(-1) == a_root).sum() + (o.bass.argmax(-1) == a_bass).sum() + o.chroma[:, :, 0, 0].numel())


def _first_max(v, high=False):
    return v.shape[-1] - 1 - np.argmax(v[..., ::-1], -1) if high else np.argmax(v, -1)


def dec_emulate(s, d, defect=None):
    """dec_run's chord walk in fp32: three dec_linear launches (the vector wave_dot where K and the row pitch allow), then per step the
    fused GRU step on [token | hoisted z part] and the heads (a scalar wave_dot per logit; arg-max to the lowest index by a sequential
    scan, a chroma bit set only by a strictly larger logit)"""
    st = {k: np.asarray(v, f32) for k, v in d["state"].items()}
    z = d["z"].numpy()
    R = z.shape[0]
    lin = lambda x, w, b, vec: wave_dot32(np.ascontiguousarray(w), x, vec) + b  # noqa: E731
    h = lin(z, st["z2dec_hid.weight"], st["z2dec_hid.bias"], s.z % 4 == 0)
    z_in = lin(z, st["z2dec_in.weight"], st["z2dec_in.bias"], s.z % 4 == 0)
    w_ih = st["gru.weight_ih_l0"]
    gi_z = lin(z_in, w_ih[:, 36:], st["gru.bias_ih_l0"], s.zin % 4 == 0)
    wx = np.ascontiguousarray(w_ih[:, :36])
    heads_w = np.concatenate([st["root_out.weight"], st["chroma_out.weight"], st["bass_out.weight"]])
    heads_b = np.concatenate([st["root_out.bias"], st["chroma_out.bias"], st["bass_out.bias"]])
    token = st["init_input"][None, :]
    out = []
    for _ in range(s.n):
        h = gru_step32(token, wx, h, st["gru.weight_hh_l0"], st["gru.bias_hh_l0"], gi_z, None, defect)
        lg = wave_dot32(heads_w, h, False) + heads_b
        out.append(lg)
        root, chroma, bass = lg[:, :12], lg[:, 12:36].reshape(R, 12, 2), lg[:, 36:]
        bits = chroma[..., 1] >= chroma[..., 0] if defect == "bit_tie_1" else chroma[..., 1] > chroma[..., 0]
        eye = np.eye(12, dtype=f32)
        token = np.concatenate([eye[_first_max(root, defect == "argmax_tie_high")], bits.astype(f32),
                                eye[_first_max(bass, defect == "argmax_tie_high")]], 1)
    lg = torch.from_numpy(np.stack(out, 1))
    return Result(root=lg[..., :12], chroma=lg[..., 12:36].reshape(R, s.n, 12, 2), bass=lg[..., 36:])


def dec_grid(got, high=False, bit_tie_1=False):
    """the decisions the kernel's rules take on a set of logits: [R][n][36]"""
    root, chroma, bass = got.root.numpy(), got.chroma.numpy(), got.bass.numpy()
    bits = chroma[..., 1] >= chroma[..., 0] if bit_tie_1 else chroma[..., 1] > chroma[..., 0]
    eye = np.eye(12, dtype=np.int64)
    return torch.from_numpy(np.concatenate([eye[_first_max(root, high)], bits.astype(np.int64), eye[_first_max(bass, high)]], -1))


def dec_ratio(s, o, got, m=None, defect=None):
    """decisions exactly the oracle's (else infinite), logits within the unit times the constant"""
    if not torch.equal(dec_grid(got, defect == "argmax_tie_high", defect == "bit_tie_1"), o.grid):
        return float("inf")
    m = M["dec_chord"] if m is None else m
    return max(ratio((got[n].double() - o[n]).abs(), m * o["unit_" + n]) for n in ("root", "chroma", "bass"))


def dec_tol_max(s, o, m=None):
    m = M["dec_chord"] if m is None else m
    return max(float((m * o["unit_" + n]).max()) for n in ("root", "chroma", "bass"))


# =====================================================================================================================================
# pn: the PianoTree decoder's greedy decode (pf_decoder_forward on PF_DEC_PNOTREE: dec_linear_kernel, gru_step_kernel,
#     pnotree_heads_kernel<16 | 64>, pnotree_emb_gru_kernel and the bind-time token tables)
# =====================================================================================================================================
PN_DEFECTS = ("argmax_tie_high", "bit_tie_1", "last_eos", "L_unclamped", "rz_swapped")
PN_S = 4            # max_simu_note of every case: three note slots a step, embedding-GRU lengths 1..3
PN_EOS = 129


def _pn(HD, R, eos=0, tie=0, why=()):
    s = Spec(kind="pn", HD=HD, R=R, eos=eos, tie=tie, why=tuple(why))
    return f"dec pnotree S{PN_S} HD{HD} R{R}" + (f" eos{eos:+d}" if eos else "") + ("", " tie", " duration-tie")[tie], s


def pn_branches(s):
    out = {f"HD:{s.HD}", f"R:{s.R}", "second_row_tile", "rows_alone"}
    out.add("lengths_all_1" if s.eos > 0 else "lengths_all_S-1" if s.eos < 0 else "lengths_vary")
    if s.tie == 1:
        out |= {"tie_in_a_lane", "tie_across_lanes"}
    if s.tie:
        out.add(f"duration_tie_HD{s.HD}")
    return out


PN_REQUIRED = {"HD:16", "HD:64", "R:9", "R:17", "lengths_all_1", "lengths_all_S-1", "lengths_vary", "tie_in_a_lane", "tie_across_lanes",
               "duration_tie_HD16", "duration_tie_HD64", "second_row_tile", "rows_alone"}


def pn_cases():
    return [
        _pn(16, 17, why=("HD:16", "R:17", "lengths_vary")),
        _pn(64, 17, why=("HD:64", "R:17", "lengths_vary")),
        _pn(16, 9, eos=50, why=("R:9", "lengths_all_1")),
        _pn(64, 9, eos=-50, why=("HD:64", "lengths_all_S-1")),
        _pn(16, 9, tie=1, why=("tie_in_a_lane", "tie_across_lanes", "duration_tie_HD16")),
        _pn(64, 9, tie=2, why=("duration_tie_HD64",)),
    ]


def _pn_gap(tdh, pitch, dur, merged=(), dur_tied=False):
    """per row the smallest gap of a decision; duplicate pitch columns are merged first, and a tie net's two duration logits are one class"""
    if merged:
        keep = [i for i in range(PN_P) if i not in merged]
        pitch = pitch[..., keep]
    if dur_tied:
        top = torch.topk(pitch, 2, dim=-1).values
        return (top[..., 0] - top[..., 1]).flatten(1).min(1).values
    return tdh.min_margin(pitch, dur)


@functools.lru_cache(maxsize=None)
def _pn_setup(key):
    """(state, z [R][512] fp32, rows cleared, rows drawn, tie pairs): the first R drawn rows whose float64 decode clears the gap"""
    from polyffusion_amd import weights
    s = dict(pn_cases())[key]
    tdh = _restate()
    state = dict(weights.synth_pianotree_decoder_state(0, s.HD))
    drawn = DRAWN // 2 if s.eos else DRAWN
    z = np.random.Generator(np.random.PCG64(404)).standard_normal((DRAWN, 512)).astype(f32)[:drawn]
    pairs = ()
    if s.eos:
        b = np.array(state["pitch_out_linear.bias"])
        b[PN_EOS] += f32(s.eos)
        state["pitch_out_linear.bias"] = b
    if s.tie:      # the two duration logits are copies: every duration bit is a tie, and must be 0
        for part in ("weight", "bias"):
            t_ = np.array(state[f"dur_out_linear.{part}"])
            t_[1] = t_[0]
            state[f"dur_out_linear.{part}"] = t_
    if s.tie == 1:
        pitch, _, _ = tdh.restate_pianotree(state, z, PN_S)
        wins = torch.bincount(pitch.argmax(-1).flatten(), minlength=PN_P)
        a1 = int(wins[:PN_P - 64 - 1].argmax())                     # a + 64 stays a pitch class below the end token
        wins[a1] = -1
        cand = [a for a in torch.argsort(wins, descending=True).tolist() if a + 1 < PN_EOS - 1 and a not in (a1 - 1, a1 + 64, a1 + 63)]
        a2 = cand[0]
        pairs = ((a1, a1 + 64), (a2, a2 + 1))                       # the same lane of the strided scan; neighbouring lanes of the butterfly
        w, b = np.array(state["pitch_out_linear.weight"]), np.array(state["pitch_out_linear.bias"])
        for a, bb in pairs:
            w[bb], b[bb] = w[a], b[a]
        state["pitch_out_linear.weight"], state["pitch_out_linear.bias"] = w, b
    pitch, dur, _ = tdh.restate_pianotree(state, z, PN_S)
    rows = torch.nonzero(_pn_gap(tdh, pitch, dur, tuple(bb for _, bb in pairs), bool(s.tie)) >= GAP).flatten()
    return state, z[rows[:s.R].numpy()], int(rows.numel()), drawn, pairs


def pn_inputs(key, s):
    state, z, cleared, drawn, pairs = _pn_setup(key)
    return {"state": state, "z": torch.from_numpy(z), "cleared": cleared, "drawn": drawn, "pairs": pairs}


def pn_oracle(s, d):
    """tests/test_decoders_host.restate_pianotree on double: logits, the grid and the lengths; the unit of a logit of step t as the chord
    decoder's, with (t + 1) (S + 2) GRU steps behind it (the time GRU, S - 1 note slots and the embedding GRU of every step so far)"""
    tdh = _restate()
    pitch, dur, lens = tdh.restate_pianotree(d["state"], d["z"].numpy(), PN_S)
    w = _w64(d["state"])
    h0 = d["z"].double() @ w["z2dec_hid_linear.weight"].t() + w["z2dec_hid_linear.bias"]
    hs = max(1.0, float(h0.abs().max()))
    steps = (torch.arange(1, 33, dtype=torch.float64) * (PN_S + 2)).reshape(1, 32, 1, 1)
    depth = 4 * 4 + 6 + 4 + 6 + 4

    def unit(name, out, k):
        wn = torch.sqrt((w[f"{name}.weight"] ** 2).sum(1))
        st = steps.reshape((1, 32) + (1,) * (out.dim() - 2))
        return U * (torch.sqrt(st * depth) * wn * hs + math.sqrt(cdiv(k, 64) + 7) * (wn * hs + out.abs()) + 2 * out.abs())
    merged = tuple(bb for _, bb in d["pairs"])
    return Result(pitch=pitch, dur=dur, lens=lens, grid=tdh.grid_of(pitch, dur), gap=float(_pn_gap(tdh, pitch, dur, merged, bool(s.tie)).min()),
                  unit_pitch=unit("pitch_out_linear", pitch, 512), unit_dur=unit("dur_out_linear", dur, s.HD))


def pn_tied_decisions(s, d, o):
    """per pair (a, b): pitch decisions of the used rows that a wins over its copy b; last, the tied duration bits (every one, all 0)"""
    out = []
    for a, b in d["pairs"]:
        assert torch.equal(o.pitch[..., a], o.pitch[..., b]) and a < b
        assert int((o.grid[..., 0] == b).sum()) == 0
        out.append(int((o.grid[..., 0] == a).sum()))
    if s.tie:
        assert torch.equal(o.dur[..., 0], o.dur[..., 1]) and int(o.grid[..., 1:].sum()) == 0
        out.append(o.dur[..., 0].numel())
    return out


def pn_lengths(grid, defect=None):
    """the lengths the heads kernel keeps, from the decided pitches [R][32][S-1]: the first end token's slot; none: S - 1"""
    p = grid[..., 0].numpy()
    eos = p == PN_EOS
    first = np.where(eos.any(-1), eos.argmax(-1) + 1, PN_S - 1)
    if defect == "last_eos":
        first = np.where(eos.any(-1), PN_S - 1 - eos[..., ::-1].argmax(-1), PN_S - 1)
    if defect == "L_unclamped":
        first = np.where(eos.any(-1), first, PN_S)
    return first


class LaneDot:
    """x W^T in the shape of wave_dot: lane l of 64 holds k = width l + 64 width i (width 4: the vector form; 1: the scalar one); its
    partial sum is taken exactly (float64) and rounded once to fp32 - the lane's own short fmaf chain is not followed - and the 64
    partials go through the kernel's fp32 shuffle tree.  No fp32 library sum takes part, so the result does not depend on the machine."""

    def __init__(self, w, width):
        N, K = w.shape
        blk = 64 * width
        self.K, self.Kp, self.width = K, cdiv(K, blk) * blk, width
        wp = np.zeros((N, self.Kp), f64)
        wp[:, :K] = w
        self.w = np.ascontiguousarray(wp.reshape(N, -1, 64, width).transpose(2, 1, 3, 0).reshape(64, -1, N))      # [lane][c][N]

    def __call__(self, x):
        R = x.shape[0]
        xp = np.zeros((R, self.Kp), f64)
        xp[:, :self.K] = x
        xr = xp.reshape(R, -1, 64, self.width).transpose(2, 0, 1, 3).reshape(64, R, -1)                          # [lane][R][c]
        p = np.matmul(xr, self.w).astype(f32)                                                                    # [lane][R][N]
        for off in (32, 16, 8, 4, 2, 1):      # lane 0 of the xor butterfly: ((v0 + v32) + (v16 + v48)) + ...
            p = p[:off] + p[off:2 * off]
        return p[0]


def _exact32(x, w):
    """a short dot a thread runs alone, taken exactly and rounded once"""
    return (np.asarray(x, f64) @ np.asarray(w, f64).T).astype(f32)


def pn_emulate(s, d, defect=None):
    """dec_run's PianoTree walk in fp32, launch by launch, with the kernels' decision rules: the pitch arg-max to the lowest index, a
    duration bit set only by a strictly larger logit, the first end token fixes the length (none: S - 1), the embedding GRU runs over
    min(length, S - 1) entries of [start token, predicted notes...], and the next token enters through the bind-time tables W_ih[:, token
    part] . note_embedding.  The wave-wide dots have wave_dot's shape (LaneDot: exact lane partials, the fp32 shuffle tree), the short
    per-thread ones are taken exactly and rounded once: the lanes' own fmaf chains, which the `step` family follows at H 512 and 1024, are
    not followed here - the walk, the tables and the rules are what this emulator is for."""
    st = {k: np.asarray(v, f32) for k, v in d["state"].items()}
    z, S, HD = d["z"].numpy(), PN_S, s.HD
    R = z.shape[0]
    dots = {}

    def dot(x, name, width=4, cols=None):
        if (name, cols) not in dots:
            w = st[name]
            dots[(name, cols)] = LaneDot(w if cols is None else w[:, cols[0]:cols[1]], width)
        return dots[(name, cols)](x)
    lin = lambda x, name, width=4: (dot(x, name + ".weight", width) + st[name + ".bias"]).astype(f32)  # noqa: E731

    def cell(gi, gh, h, H, bn=None):
        return cell32(*_thirds(gi.astype(f32), H), *_thirds(gh.astype(f32), H), h, defect, bn)
    ew, eb = st["note_embedding.weight"], st["note_embedding.bias"]
    wn_ih, wt_ih = "dec_notes_gru.weight_ih_l0", "dec_time_gru.weight_ih_l0"
    tn, tn_b = _exact32(st[wn_ih][:, 1024:], ew.T).T, _exact32(st[wn_ih][:, 1024:], eb[None])[:, 0]
    te, te_b = [], []
    for sfx in ("", "_reverse"):
        w_e = st["dec_notes_emb_gru.weight_ih_l0" + sfx]
        te.append(_exact32(w_e, ew.T).T)
        te_b.append((_exact32(w_e, eb[None])[:, 0] + st["dec_notes_emb_gru.bias_ih_l0" + sfx]).astype(f32))
    sos = np.zeros(135, f32)
    sos[128], sos[130:] = 1.0, 2.0
    token_rows = lambda tab, bias, tok: (_exact32(tok, tab.T) + bias).astype(f32)  # noqa: E731
    ht, z_in = lin(z, "z2dec_hid_linear"), lin(z, "z2dec_in_linear")
    gi_z = (dot(z_in, wt_ih, 4, (256, 512)) + st["dec_time_gru.bias_ih_l0"]).astype(f32)
    tok_t = np.broadcast_to(st["dec_init_input"], (R, 256))
    pitch_out, dur_out = np.zeros((R, 32, S - 1, PN_P), f32), np.zeros((R, 32, S - 1, 5, 2), f32)
    eye = np.eye(PN_P, dtype=f32)
    for t in range(32):
        ht = cell(dot(tok_t, wt_ih, 1, (0, 256)) + gi_z, dot(ht, "dec_time_gru.weight_hh_l0") + st["dec_time_gru.bias_hh_l0"], ht, 1024)
        hn = lin(ht, "dec_time_to_notes_hid")
        gi_ns = (dot(ht, wn_ih, 4, (0, 1024)) + st["dec_notes_gru.bias_ih_l0"]).astype(f32)
        tok = np.broadcast_to(sos, (R, 135))
        toks = [tok]
        for sl in range(1, S):
            hn = cell(gi_ns + token_rows(tn, tn_b, tok), dot(hn, "dec_notes_gru.weight_hh_l0") + st["dec_notes_gru.bias_hh_l0"], hn, 512)
            pitch = lin(hn, "pitch_out_linear")
            dh = lin(np.concatenate([hn, pitch], 1), "dur_hid_linear", 1)
            d_tok, digits = np.broadcast_to(st["dur_sos_token"], (R, 5)), []
            for dg in range(5):
                dh = cell(_exact32(d_tok, st["dec_dur_gru.weight_ih_l0"]) + st["dec_dur_gru.bias_ih_l0"],
                          _exact32(dh, st["dec_dur_gru.weight_hh_l0"]) + st["dec_dur_gru.bias_hh_l0"], dh, HD)
                dl = (_exact32(dh, st["dur_out_linear.weight"]) + st["dur_out_linear.bias"]).astype(f32)
                dur_out[:, t, sl - 1, dg] = dl
                bit = dl[:, 1] >= dl[:, 0] if defect == "bit_tie_1" else dl[:, 1] > dl[:, 0]
                digits.append(bit.astype(f32))
                d_tok = np.eye(5, dtype=f32)[bit.astype(np.int64)]
            pitch_out[:, t, sl - 1] = pitch
            tok = np.concatenate([eye[_first_max(pitch, defect == "argmax_tie_high")], np.stack(digits, 1)], 1)
            toks.append(tok)
        if t == 31:
            break
        L = pn_lengths(torch.from_numpy(_first_max(pitch_out[:, t], defect == "argmax_tie_high")[..., None]), defect)
        seq = np.stack(toks, 1)                                        # [R][S][135]: the start token, then the predicted notes
        halves = []
        for dr, sfx in enumerate(("", "_reverse")):
            h = np.zeros((R, 128), f32)
            for i in range(S):
                idx = np.clip(L - 1 - i if dr else np.full(R, i), 0, S - 1)
                gi = token_rows(te[dr], te_b[dr], seq[np.arange(R), idx])
                new = cell(gi, _exact32(h, st["dec_notes_emb_gru.weight_hh_l0" + sfx]) + st["dec_notes_emb_gru.bias_hh_l0" + sfx], h, 128)
                h = np.where((i < L)[:, None], new, h)
            halves.append(h)
        tok_t = np.concatenate(halves, 1)
    return Result(pitch=torch.from_numpy(pitch_out), dur=torch.from_numpy(dur_out))


def pn_grid(got, defect=None):
    """the decisions the kernel's rules take on a set of logits: [R][32][S-1][6]"""
    pitch, dur = got.pitch.numpy(), got.dur.numpy()
    bits = dur[..., 1] >= dur[..., 0] if defect == "bit_tie_1" else dur[..., 1] > dur[..., 0]
    return torch.from_numpy(np.concatenate([_first_max(pitch, defect == "argmax_tie_high")[..., None], bits.astype(np.int64)], -1))


def pn_ratio(s, o, got, m=None, defect=None, est=None):
    """the grid (the library's own `est` where given, else the kernel's rules on the logits) and the lengths exactly the oracle's - else
    infinite - and the logits within the unit times the constant"""
    grid = pn_grid(got, defect) if est is None else est
    if not torch.equal(grid, o.grid) or not np.array_equal(pn_lengths(grid, defect), o.lens.numpy()):
        return float("inf")
    m = M["dec_pnotree"] if m is None else m
    return max(ratio((got.pitch.double() - o.pitch).abs(), m * o.unit_pitch), ratio((got.dur.double() - o.dur).abs(), m * o.unit_dur))


def pn_tol_max(s, o, m=None):
    m = M["dec_pnotree"] if m is None else m
    return max(float((m * o.unit_pitch).max()), float((m * o.unit_dur).max()))


# =====================================================================================================================================
# The tables, and what the library must refuse
# =====================================================================================================================================
KINDS = ("gates", "step", "enc", "dec", "pn")
CASES = {"gates": gates_cases, "step": step_cases, "enc": enc_cases, "dec": dec_cases, "pn": pn_cases}
INPUTS = {"gates": gates_inputs, "step": step_inputs, "enc": enc_inputs, "dec": dec_inputs, "pn": pn_inputs}
BRANCHES = {"gates": gates_branches, "step": step_branches, "enc": enc_branches, "dec": dec_branches, "pn": pn_branches}
REQUIRED = {"gates": GATES_REQUIRED, "step": STEP_REQUIRED, "enc": ENC_REQUIRED, "dec": DEC_REQUIRED, "pn": PN_REQUIRED}
DEFECTS = {"gates": GATES_DEFECTS, "step": STEP_DEFECTS, "enc": ENC_DEFECTS, "dec": DEC_DEFECTS, "pn": PN_DEFECTS}
SUBKINDS = {"gates": ("gates",), "step": ("step",), "enc": ("enc_chord", "enc_texture", "enc_pnotree"), "dec": ("dec_chord",), "pn": ("dec_pnotree",)}
ORACLES = {"gates": gates_oracle, "step": step_oracle, "enc": enc_oracle, "dec": dec_oracle, "pn": pn_oracle}


def sub_of(s):
    return enc_sub(s) if s.kind == "enc" else {"dec": "dec_chord", "pn": "dec_pnotree"}.get(s.kind, s.kind)


def cases(kind=None):
    """[(key, spec)] of one kernel family, or of all"""
    return CASES[kind]() if kind else [c for k in KINDS for c in CASES[k]()]


def branches(s):
    return BRANCHES[s.kind](s)


def inputs(key, s):
    return INPUTS[s.kind](key, s)


@functools.lru_cache(maxsize=None)
def _oracle_cached(key):
    s = dict(cases())[key]
    d = inputs(key, s)
    return d, ORACLES[s.kind](s, d)


def oracle(key, s):
    """(inputs, oracle) of a case, computed once and shared"""
    return _oracle_cached(key)


@functools.lru_cache(maxsize=None)
def _emulated(key, defect=None):
    """(emulator output, every read in bounds) of a case; the undefective runs are shared by the tests that need them"""
    s = dict(cases())[key]
    d, _ = oracle(key, s)
    if s.kind == "dec":
        return dec_emulate(s, d, defect), True
    if s.kind == "pn":
        return pn_emulate(s, d, defect), True
    return {"gates": gates_emulate, "step": step_emulate, "enc": enc_emulate}[s.kind](s, d, defect)


def emulated_ratio(key, s, defect=None, m=None):
    """err / tol of the emulator (with `defect`) against the oracle; inf where a defect reads out of bounds"""
    _, o = oracle(key, s)
    got, ok = _emulated(key) if defect is None else _emulated.__wrapped__(key, defect)
    if not ok:
        return float("inf")
    if s.kind in ("dec", "pn"):
        return {"dec": dec_ratio, "pn": pn_ratio}[s.kind](s, o, got, m, defect)
    return {"gates": gates_ratio, "step": step_ratio, "enc": enc_ratio}[s.kind](s, o, got, m)


def measured_ratio(key, s):
    """what tools/rnn_error_model.py takes the maximum of: the undefective emulator against the oracle, relative to the unit (constant 1)"""
    return emulated_ratio(key, s, m=1.0)


def defect_applies(s, defect):
    """cases a defect cannot touch are not emulated again"""
    if defect in ("masked_reverse_S", "masked_step_le"):
        return (s.kind == "gates" and s.seq_len > 0) or (s.kind == "enc" and s.enc == "pnotree" and s.S <= 3)
    if defect == "pad_column":
        return s.kind == "enc" and s.enc == "pnotree" and s.S <= 3
    if defect == "ld2_ignored":
        return s.kind == "step" and s.add2
    if s.kind == "dec":
        return s.H <= 96
    if s.kind == "pn":
        return s.R == 9
    if s.kind == "enc":
        return (s.enc == "chord" and s.H <= 32) or (s.enc == "pnotree" and s.S <= 3) or (s.enc == "texture" and s.C == 1)
    return True


P = 1 << 20      # a non-null, 16-byte aligned placeholder address: a refused call reads nothing


def refused_gates(p=lambda name: P):
    """[(name, argument tuple of pf_gru_gates without the stream)]: calls the library must answer with PF_EINVAL before any launch"""
    return [
        ("gates null gi", (0, 12, p("v"), p("out"), 8, 2, 4, 0, 0, 0, 0)),
        ("gates null h", (p("v"), 12, p("v"), 0, 8, 2, 4, 0, 0, 0, 0)),
        ("gates rows 0", (p("v"), 12, p("v"), p("out"), 8, 0, 4, 0, 0, 0, 0)),
        ("gates hidden 0", (p("v"), 12, p("v"), p("out"), 8, 2, 0, 0, 0, 0, 0)),
        ("gates ld_h < hidden", (p("v"), 12, p("v"), p("out"), 3, 2, 4, 0, 0, 0, 0)),
        ("gates masked seq_len 0", (p("v"), 12, p("v"), p("out"), 8, 2, 4, p("v"), 0, 0, 0)),
    ]


def refused_step(p=lambda name: P):
    """[(name, dict of pf_gru_step_args fields)]: refused with PF_EINVAL, nothing enqueued"""
    ok = dict(x=p("v"), ldx=36, Kx=36, wx=p("v"), ldwx=44, h_in=p("v"), wh=p("v"), b_hh=p("v"), add1=p("v"), ld1=288, add2=0, ld2=0,
              h_out=p("out"), R=9, H=96)
    return [
        ("step H % 4", dict(ok, H=98)),
        ("step wh unaligned", dict(ok, wh=p("v") + 4)),
        ("step h_in unaligned", dict(ok, h_in=p("v") + 8)),
        ("step 8 (H + Kx) floats above 64 KiB", dict(ok, H=1024, Kx=1028, ldx=1028, ldwx=1028)),
        ("step h_out == h_in", dict(ok, h_out=p("v"))),
        ("step null b_hh", dict(ok, b_hh=0)),
    ]


# (kind, input_dim, emb_size, hidden_dim, z_dim, num_channel, with_scale): pf_encoder_create_dist must refuse; linear_mu's K = 2 hidden
REFUSED_ENCODERS = [("chord hidden 1028", (0, 36, 0, 1028, 64, 0, 0)), ("texture hidden 2048", (1, 0, 256, 2048, 256, 10, 1)),
                    ("pnotree time hidden 1056", (2, 135, 128, 1056, 512, 256, 0))]
