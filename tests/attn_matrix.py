"""The attention case matrix: one small, edge-seeking set of launches that reaches every form of the attention kernels (csrc/attention.hip,
attention_bf3.hip, attention_wide.hip) through the four entry points pf_attention, pf_attention_bf16x3, pf_attention_bf16x3_split and
pf_attention_wide, a float64 oracle per (batch, head), a float64 emulation of the documented arithmetic of the split kernels, and the
per-element error budget both GPU builds are held to.  Used by tests/test_attn_matrix.py (no GPU), tests/test_gpu_attn_matrix.py (-m gpu)
and tools/attn_error_model.py (measures the constants).

The budget.  With p = softmax(s), o = sum_j p_j v_j and a perturbation ds of the scores, to first order
do_e = sum_j p_j (v_je - o_e) ds_j + (error of the P.V sum) / l.  So, per output element e of query row i:

    tol(e) = M * [ (M_ACC sqrt(dh) 2^-24 + M_SPLIT[mode] u) * As(e) + M_EXP 2^-24 * Ae(e)
                   + (M_ACC sqrt(Lk) 2^-24 + M_SPLIT[mode] u) * Tpv(e) + floor(mode, e) ] + 4 * 2^-24 * |ref(e)|
    As(e)  = sum_j p_j |v_je - o_e| Ts(i,j),   Ts(i,j) = scale * sqrt(sum_d (q_id k_jd)^2)
    Ae(e)  = sum_j p_j |v_je - o_e| (1 + |s_ij - max_i|)
    Tpv(e) = sqrt(sum_j (p_j v_je)^2)

(the issue's ds(i,j) = (M_ACC sqrt(dh) 2^-24 + M_SPLIT u) Ts + M_EXP 2^-24 (1 + |s - max|) multiplied out).  u is the unit roundoff
include/pfhip.h documents (0 / 2^-18 / 2^-22).  floor is zero except in the fp16 build, where probability pieces below 2^-14 are quantised
to 2^-24: 2^-25 * sum_j |v_je - o_e| / l_i with l_i = sum_j exp(s_ij - max_i) (the kernels' reference exponent is never above the row
maximum by more than the lazy form's 2^6 headroom allows - and there p >= 2^-6 p_true only shrinks the quantum relative to l).
A plane store (hi + lo) adds the pair's representation error as in the conv matrix: 2^-16 |v| (bf16), 2^-22 |v| + 2^-25 (fp16).

M_ACC, M_EXP and M_SPLIT are NOT taken from the kernels: tools/attn_error_model.py measures them on the CPU over this matrix (torch float32
against the oracle; the emulation against the oracle) and writes them to profiles/attn_error_model.md; the constants below equal that
file's.  M = 4 covers what neither reference does: the MFMA's accumulation order, the hardware exp2 and reciprocal, the merge's second
summation order."""
from __future__ import annotations

import math
import zlib

import numpy as np
import torch

from polyffusion_amd import _lib

EPS = 2.0 ** -24
UNIT = {"f32": 0.0, "bf16": 2.0 ** -18, "f16": 2.0 ** -22}
M = 4.0
# measured by tools/attn_error_model.py, recorded in profiles/attn_error_model.md (rounded up to two digits)
M_ACC = 2.97
M_EXP = 0.45
M_SPLIT = {"bf16": 2.31, "f16": 0.05}

LOG2E = 1.4426950408889634
TAU = 6.0      # attention_bf3.hip: the 256-query form moves a row's reference exponent only when the maximum grew by more than 2^TAU
KT = 64        # keys per tile of every flash form
NSPLIT = 4     # key slices of the split form
CUS = 256      # compute units of the part the auto / split thresholds of the case list are laid out for (the GPU test reads the real count)
ALL_HEADS = 12  # the CPU measurement takes the first, the last and two inner (batch, head) pairs of a case with more (heads())

ATTN, X3, SPLIT, WIDE = "attn", "x3", "split", "wide"
REGIMES = ("gauss", "ramp", "late", "first", "flat", "slices")


class Spec(dict):
    __getattr__ = dict.__getitem__

    def but(self, **kw):
        s = Spec(self)
        s.update(kw)
        return s


# ep: entry point; form: -1 auto | 0 | 1 (x3); planes: hi/lo plane output; ldo: guard columns of the fp32 output; cross: k | v in their own
# [B lk][2C] buffer (pf_attention; otherwise q | k | v interleaved in [B L][3C]); regime / rate: inputs(); scratch: split form - "full",
# "short" (four bytes less than asked) or "none" (the shape does not split)
DEFAULT = Spec(ep=ATTN, b=1, h=1, lq=128, lk=128, dh=64, form=0, planes=0, ldo=0, cross=0, regime="gauss", rate="", scratch="")


def key_of(s):
    k = f"{s.ep} B{s.b} H{s.h} {s.lq}x{s.lk} d{s.dh} {s.regime}{('-' + s.rate) if s.rate else ''}"
    if s.ep == X3:
        k += f" form{'A' if s.form < 0 else s.form}"
    for name in ("planes", "cross"):
        if s[name]:
            k += " " + name
    if s.ldo:
        k += f" ldo+{s.ldo}"
    if s.scratch:
        k += " scratch-" + s.scratch
    return k


def channels(s):
    return s.h * s.dh


def scale_of(s):
    return 0.125 if s.ep in (X3, SPLIT) else 1.0 / math.sqrt(s.dh)


def splits(s):
    """whether the split entry point splits this case (attention_bf3_split_floats; `CUS` compute units) and is given the scratch to"""
    return s.ep == SPLIT and s.lq % 512 == 0 and (s.lq // 128) * s.h * s.b * NSPLIT <= CUS and s.scratch == "full"


def scratch_floats(s):
    if s.ep == WIDE:
        return s.b * s.lq * s.lq
    if s.ep == SPLIT and s.lq % 512 == 0 and (s.lq // 128) * s.h * s.b * NSPLIT <= CUS:
        return NSPLIT * s.b * s.h * s.lq * (64 + 2)
    return 0


def form_of(s, cus=CUS):
    """the kernel a case runs: "f32" (attention.hip), "wide", "q128", "q256", "split" """
    if s.ep == ATTN:
        return "f32"
    if s.ep == WIDE:
        return "wide"
    if s.ep == SPLIT:
        return "split" if splits(s) else "q128"
    if s.form < 0:
        return "q256" if s.lq % 256 == 0 and (s.lq // 256) * s.h * s.b >= cus * 3 // 4 else "q128"
    return "q256" if s.form == 1 else "q128"


def grid_of(s, cus=CUS):
    """workgroups of the one-dimensional grid of attention_bf3.hip's kernels (the XCD remap and the FastDiv decode work on it)"""
    assert s.ep in (X3, SPLIT)
    f = form_of(s, cus)
    if f == "q256":
        return s.b * s.h * (s.lq // 256)
    return s.b * s.h * (s.lq // 128) * (NSPLIT if f == "split" else 1)


def grid_class(n):
    return "1" if n == 1 else "<8" if n < 8 else "8k" if n % 8 == 0 else "8k+r"


def path_of(s):
    """(entry point, form, split?, output kind, grid-size class, ldo padded?)"""
    return (s.ep, form_of(s), splits(s), "planes" if s.planes else "f32", grid_class(grid_of(s)) if s.ep in (X3, SPLIT) else "-", bool(s.ldo))


# every launch path the matrix must reach (tests/test_attn_matrix.py asserts the case list covers this table and nothing drops out)
REQUIRED_PATHS = (
    # pf_attention launches a (ceil(lq / 128), H, B) grid and the wide form three kernels with grids of their own: no branch of theirs depends
    # on a grid-size class, so the table has none for them ("-")
    [(ATTN, "f32", False, "f32", "-", False), (ATTN, "f32", False, "f32", "-", True)]
    # the XCD remap of attn_bf3_kernel: one workgroup, fewer than 8 (nwg >> 3 == 0), a remainder (nwg & 7 != 0), none
    + [(X3, "q128", False, "f32", g, p) for g, p in (("1", False), ("8k+r", True), ("8k", False))]
    + [(X3, "q128", False, "planes", g, False) for g in ("<8", "8k+r", "8k")]
    + [(X3, "q256", False, "f32", g, p) for g, p in (("<8", False), ("8k+r", True), ("8k+r", False), ("8k", False))]
    + [(X3, "q256", False, "planes", g, False) for g in ("8k+r", "8k")]
    # a split grid is (L / 128) * 4 * B * H workgroups with L % 512 == 0: always a multiple of 16
    + [(SPLIT, "split", True, "f32", "8k", False), (SPLIT, "split", True, "f32", "8k", True), (SPLIT, "split", True, "planes", "8k", False)]
    # the split entry point where it does not split (the shape; too little scratch)
    + [(SPLIT, "q128", False, "f32", "8k+r", False), (SPLIT, "q128", False, "f32", "<8", False)]
    + [(WIDE, "wide", False, "f32", "-", False), (WIDE, "wide", False, "f32", "-", True)]
)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def _c(**kw):
    if "l" in kw:
        kw["lq"] = kw["lk"] = kw.pop("l")
    return DEFAULT.but(**kw)


def _case_specs():
    out = []
    # pf_attention: lq in {1, 127, 128, 129, 200}, lk in {1, 4, 63, 64, 65, 77, 129}, dh in {32, 64}, H in {1, 3, 4}, B in {1, 3};
    # self-attention out of one [B L][3C] buffer, cross-attention with k | v in [B lk][2C]; ldo = C and C + 8
    out += [_c(l=1), _c(b=3, h=3, dh=32, l=127, ldo=8, regime="ramp", rate="slow"), _c(h=4, l=128, regime="late"),
            _c(b=3, dh=32, l=129, ldo=8, regime="first"), _c(h=3, l=200, regime="ramp", rate="fast"),
            _c(h=4, dh=32, l=129, regime="flat", ldo=8), _c(b=3, h=4, l=200, dh=32, regime="late")]
    out += [_c(b=3, h=4, lq=200, lk=1, cross=1), _c(h=3, dh=32, lq=129, lk=4, cross=1, ldo=8, regime="first"),
            _c(lq=127, lk=63, cross=1, regime="late"), _c(b=3, h=4, dh=32, lq=128, lk=64, cross=1, regime="ramp", rate="slow"),
            _c(h=3, lq=1, lk=65, cross=1, ldo=8, regime="late"), _c(h=4, dh=32, lq=200, lk=77, cross=1, regime="first"),
            _c(b=3, lq=129, lk=129, cross=1, ldo=8, regime="ramp", rate="fast"), _c(b=3, h=3, lq=200, lk=4, cross=1, regime="flat")]
    # pf_attention_bf16x3: form 0 at L in {128, 384, 512}, form 1 at L in {256, 512, 768}; H in {1, 3, 4}; grids of 1, < 8, 8k + r, 8k
    x = lambda **kw: _c(ep=X3, **kw)   # noqa: E731
    out += [x(l=128), x(h=3, l=128, planes=1, regime="late"), x(b=3, l=384, ldo=8, regime="ramp", rate="slow"),
            x(h=4, l=512, regime="ramp", rate="fast"), x(h=3, l=384, planes=1, regime="first"), x(h=4, l=128, planes=1, regime="flat"),
            x(b=2, h=4, l=128, planes=1), x(h=4, l=256, regime="late")]
    out += [x(form=1, b=3, h=3, l=256, ldo=8, regime="ramp", rate="slow"), x(form=1, h=4, l=512, planes=1, regime="ramp", rate="fast"),
            x(form=1, l=768, regime="late"), x(form=1, h=3, l=768, planes=1, regime="ramp", rate="slow"),
            x(form=1, b=2, h=4, l=256, regime="first"), x(form=1, h=3, l=768, regime="ramp", rate="fast"),
            x(form=1, h=4, l=512, regime="flat")]
    # auto: one shape on each side of (L / 256) H B >= 3/4 CUs
    out += [x(form=-1, b=47, h=4, l=256), x(form=-1, b=48, h=4, l=256, regime="late")]
    # pf_attention_bf16x3_split: the smallest shape that splits, B = 2 H = 3, L = 1024; one that must not split, one with too little scratch
    sp = lambda **kw: _c(ep=SPLIT, **{"scratch": "full", **kw})   # noqa: E731
    out += [sp(l=512, regime="slices"), sp(b=2, h=3, l=512, planes=1, regime="slices"), sp(l=1024, ldo=8, regime="ramp", rate="steep"),
            sp(h=2, l=512, regime="late", rate="far"), sp(l=512, planes=1, regime="ramp", rate="slow"), sp(h=2, l=512, ldo=8),
            sp(h=3, l=384, scratch="none"), sp(l=512, scratch="short", regime="slices")]
    # pf_attention_wide: L in {64, 128, 1024} (1024 at d = 16, B = 1), d in {16, 32, 48, 256}, B in {1, 3}, ld = 3 d, ldo = d and d + 8
    w = lambda **kw: _c(ep=WIDE, **kw)   # noqa: E731
    out += [w(l=1024, dh=16, regime="late"), w(b=3, l=64, dh=32, ldo=8), w(l=128, dh=48, regime="first"),
            w(b=3, l=128, dh=256, ldo=8, regime="ramp", rate="slow"), w(l=64, dh=256, regime="flat"), w(b=3, l=64, dh=48, ldo=8, regime="late")]
    return out


def cases():
    """[(key, spec)] in a fixed order"""
    out, seen = [], set()
    for s in _case_specs():
        k = key_of(s)
        assert k not in seen, k
        seen.add(k)
        out.append((k, s))
    return out


def bit_equal_partner(s, cus=CUS):
    """the forced-form launch a case must equal bit for bit: auto -> the form it should have picked; a split-entry launch that does not
    split -> form 0.  None for every other case."""
    if s.ep == X3 and s.form < 0:
        return s.but(form=1 if form_of(s, cus) == "q256" else 0)
    if s.ep == SPLIT and not splits(s):
        return s.but(ep=X3, form=0, scratch="")
    return None


def heads(s, sample=True):
    """the (batch, head) pairs of a case: all of them (the GPU test compares every one), or - `sample`, the CPU measurement and gate - at most
    ALL_HEADS, since the heads of a case are draws of one distribution"""
    n = s.b * s.h
    idx = range(n) if n <= ALL_HEADS or not sample else sorted({0, n // 3, 2 * n // 3 + 1, n - 1})
    return [(i // s.h, i % s.h) for i in idx]


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def x3_dtype(variant):
    return _lib.x3_torch_dtype(variant)


def inputs(key, s):
    """seeded fp32 q [B][lq][H][dh], k, v [B][lk][H][dh] of a case; every head and sample has its own draw.  Regimes (natural-log units):
    gauss  - scores ~ N(0, 1);
    ramp   - the scores of a row grow along the keys by `rate` per 64-key tile: "slow" 2.0 (2.9 in the exp2 domain: below the lazy form's
             2^6, so it keeps the old exponent for two tiles and p reaches 2^5.8), "fast" 6.0 (8.7: every tile moves the exponent),
             "steep" 8.0 (11.5: over the twelve tiles between the first and the last key slice of L = 1024 more than fp32's 2^128);
    late   - three keys of the last tile score 20 on one query each (first, middle, last query); rate "far": 100, which puts the last key
             slice's maximum more than 88 above the first one's (exp2f of the difference leaves fp32's range);
    first  - the first two keys score +20 and -20 on such queries;
    flat   - q = 0: all scores equal, the output is the mean of v;
    slices - the keys of the four slices of the split form are shifted by -60, -3, +60, 0: slice 2 dominates, slice 0's merge weight
             2^(-120 log2 e) underflows to zero in fp32, slice 1's does not."""
    rng = np.random.Generator(np.random.PCG64(zlib.crc32(key.encode())))

    def g(*shape):
        return torch.from_numpy(rng.standard_normal(shape).astype(np.float32))

    B, H, lq, lk, dh = s.b, s.h, s.lq, s.lk, s.dh
    scale = scale_of(s)
    q, k = g(B, lq, H, dh), g(B, lk, H, dh)
    v = g(B, lk, H, dh) + 0.5 * g(B, 1, H, 1)
    u = g(B, 1, H, dh)
    u = u / u.norm(dim=-1, keepdim=True)
    A = 4.0
    if s.regime == "ramp":
        rate = {"slow": 2.0, "fast": 6.0, "steep": 8.0}[s.rate]
        pos = torch.arange(lk, dtype=torch.float32).reshape(1, lk, 1, 1) / KT
        q = 0.5 * q + A * u
        k = k + (rate / (scale * A)) * pos * u
    elif s.regime == "slices":
        shift = torch.tensor([-60.0, -3.0, 60.0, 0.0])[torch.arange(lk) * NSPLIT // lk].reshape(1, lk, 1, 1)
        q = 0.5 * q + A * u
        k = k + (shift / (scale * A)) * u
    elif s.regime in ("late", "first"):
        targets = sorted({0, lq // 2, lq - 1})
        qt = q[:, targets]                                                   # [B][n][H][dh]
        top = 100.0 if s.rate == "far" else 20.0
        aim = top * qt / (scale * (qt * qt).sum(-1, keepdim=True))           # k with scale * q_t . k = top
        if s.regime == "late":
            rows = [max(lk - 5 - i, 0) for i in range(len(targets))]
            for i, r in enumerate(rows[:lk]):
                k[:, r] = aim[:, i]
        else:
            k[:, 0] = aim[:, 0]
            if lk > 1:
                k[:, 1] = -aim[:, -1]
    elif s.regime == "flat":
        q = torch.zeros_like(q)
    return dict(q=q.contiguous(), k=k.contiguous(), v=v.contiguous())


# ---- the q | k | v planes of attention_bf3.hip --------------------------------------------------------------------------------------
def split_pieces(x32, variant):
    dt = x3_dtype(variant)
    hi = x32.to(dt)
    return hi, (x32 - hi.float()).to(dt)


def encode_planes(d, variant):
    """host encoder of the layout the header of attention_bf3.hip documents: [qh | ql | kh | kl | vTh | vTl], each B*L*C elements; Q and K
    [B*L][C]; V^T [B][H][64][L] with the two middle token quads of every 16-token block swapped.  Returns (flat planes, the pieces as
    [B][L][H][64] tensors: qh, ql, kh, kl, vh, vl)."""
    pieces = {}
    flat = []
    for name in "qkv":
        hi, lo = split_pieces(d[name], variant)
        pieces[name + "h"], pieces[name + "l"] = hi, lo
        for p in (hi, lo):
            if name == "v":
                B, L, H, dh = p.shape
                t = p.permute(0, 2, 3, 1).reshape(B, H, dh, L // 16, 4, 4)    # [.., block, quad, token in quad]
                p = t[..., [0, 2, 1, 3], :]
            flat.append(p.reshape(-1))
    return torch.cat(flat), pieces


def plane_inputs(pieces):
    """the oracle's inputs: hi + lo of the planes in float64, so the kernel is charged for its own arithmetic only"""
    return {n: pieces[n + "h"].double() + pieces[n + "l"].double() for n in "qkv"}


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
class Result(dict):
    __getattr__ = dict.__getitem__


def oracle(q, k, v, scale):
    """float64 softmax attention of one (batch, head): q [lq][dh], k, v [lk][dh] float64, scaled after the dot product; with the sums the
    budget needs (module text), each [lq][dh]"""
    s = (q @ k.t()) * scale
    mx = s.max(1, keepdim=True).values
    e = torch.exp(s - mx)
    l = e.sum(1, keepdim=True)
    p = e / l
    o = p @ v
    ts = scale * torch.sqrt((q * q) @ (k * k).t())
    we = 1.0 + (s - mx).abs()
    lq, lk, dh = q.shape[0], k.shape[0], v.shape[1]
    As, Ae, Fl = (torch.zeros(lq, dh, dtype=torch.float64) for _ in range(3))
    step = max(1, (1 << 21) // (lk * dh))
    for r0 in range(0, lq, step):
        r = slice(r0, r0 + step)
        dv = (v[None] - o[r, None]).abs()                  # [rows][lk][dh]
        pd = p[r, :, None] * dv
        As[r] = torch.einsum("ije,ij->ie", pd, ts[r])
        Ae[r] = torch.einsum("ije,ij->ie", pd, we[r])
        Fl[r] = dv.sum(1) / l[r]
    return Result(ref=o, As=As, Ae=Ae, Tpv=torch.sqrt((p * p) @ (v * v)), Fl=Fl, p=p, s=s)


# ---- the references the constants are measured on -----------------------------------------------------------------------------------
DEFECTS = ("drop_klo_qhi", "no_plo", "l_miss_rescale", "merge_m0")


def emulate(pc, b, h, variant, form, defect=None):
    """float64 emulation of the documented arithmetic of attention_bf3.hip for head (b, h) of the pieces `pc` (encode_planes): the scores
    S = k_hi.q_hi + k_hi.q_lo + k_lo.q_hi in the exp2 domain; tiles of 64 keys; probabilities relative to the running reference of the
    form - "q128": the running maximum; "q256": the lazy one, which follows the maximum only when that grew by more than 2^TAU; "split":
    four key slices in the q128 way, merged with weights exp2f(m_s - max m_s) evaluated in fp32 as attn_merge_kernel does - rounded to
    nearest into hi and lo pieces of the build's type (fp16's subnormal quantum included: torch's conversion); O = v_hi.p_hi + v_hi.p_lo +
    v_lo.p_hi; the row sum over the unsplit probabilities.  `defect`: None or one of DEFECTS - a kernel bug the budget must catch:
    the k_lo.q_hi product left out | no lo piece of the probabilities | the row sum misses its largest rescale | the merge takes slice 0's
    maximum instead of the largest."""
    dt = x3_dtype(variant)
    qh, ql, kh, kl, vh, vl = (pc[n][b, :, h].double() for n in ("qh", "ql", "kh", "kl", "vh", "vl"))
    S = qh @ kh.t() + ql @ kh.t()
    if defect != "drop_klo_qhi":
        S = S + qh @ kl.t()
    S = S * (0.125 * LOG2E)
    L = S.shape[1]

    def walk(t0, t1, lazy):
        n = S.shape[0]
        m = torch.full((n, 1), -math.inf, dtype=torch.float64)
        l = torch.zeros(n, 1, dtype=torch.float64)
        O = torch.zeros(n, 64, dtype=torch.float64)
        steps = []
        for t in range(t0, t1):
            st = S[:, t * KT:(t + 1) * KT]
            mt = st.max(1, keepdim=True).values
            m_new = torch.where(mt > m + TAU, mt, m) if lazy else torch.maximum(m, mt)
            steps.append((m, m_new, st))
            m = m_new
        skip = None
        if defect == "l_miss_rescale":   # per row: the tile whose rescale factor is the smallest one below 1 (first tile apart: l is zero there)
            al = torch.stack([torch.exp2(a - b_) for a, b_, _ in steps[1:]] or [torch.ones(n, 1, dtype=torch.float64)])
            skip = al.argmin(0) + 1
        for i, (m_old, m_new, st) in enumerate(steps):
            alpha = torch.exp2(m_old - m_new)
            O = O * alpha
            l = l * (torch.where(skip == i, torch.ones_like(alpha), alpha) if skip is not None else alpha)
            p32 = torch.exp2(st - m_new).float()
            ph = p32.to(dt)
            pl = (p32 - ph.float()).to(dt)
            l = l + p32.double().sum(1, keepdim=True)
            t = t0 + i
            vth, vtl = vh[t * KT:(t + 1) * KT], vl[t * KT:(t + 1) * KT]
            O = O + ph.double() @ vth + ph.double() @ vtl
            if defect != "no_plo":
                O = O + pl.double() @ vth
        return O, m_new, l

    ntile = L // KT
    if form != "split":
        O, _, l = walk(0, ntile, form == "q256")
        return O / l
    parts = [walk(sl * ntile // NSPLIT, (sl + 1) * ntile // NSPLIT, False) for sl in range(NSPLIT)]
    ms = torch.cat([p[1] for p in parts], dim=1)
    m = ms[:, :1] if defect == "merge_m0" else ms.max(1, keepdim=True).values
    w = torch.exp2((ms - m).float()).double()     # exp2f: overflows to inf above 2^128, underflows to zero below 2^-149
    num = sum(w[:, i:i + 1] * parts[i][0] for i in range(NSPLIT))
    den = sum(w[:, i:i + 1] * parts[i][2] for i in range(NSPLIT))
    return num / den


def torch_compose(q, k, v, scale, dtype):
    """the same attention as a composition of torch's own ops in `dtype`, one head"""
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    return torch.softmax((q @ k.t()) * scale, dim=-1) @ v


def exp_reference(o, v):
    """the exponential alone in float32 (M_EXP): float32 exp of the oracle's own shifted scores (rounded to float32); the row sum, the
    division and P.V in float64.  Every key's probability then carries the exponential's own error, which is what the first-order term
    sum_j p_j (v_je - o_e) ds_j describes; the roundings of a float32 row sum and of each p_j are errors of sums over the keys and are
    measured with the products (M_ACC sqrt(Lk) Tpv)."""
    sh = (o.s - o.s.max(1, keepdim=True).values).float()
    e = torch.exp(sh).double()
    return (e / e.sum(1, keepdim=True)) @ v


# ---- the budget ---------------------------------------------------------------------------------------------------------------------
def mode_of(s, variant):
    return "f32" if s.ep in (ATTN, WIDE) else "f16" if variant == "f16" else "bf16"


def acc_scale(s, o):
    """what M_ACC multiplies"""
    return EPS * (math.sqrt(s.dh) * o.As + math.sqrt(s.lk) * o.Tpv)


def exp_scale(o):
    """what M_EXP multiplies"""
    return EPS * o.Ae


def split_scale(mode, o):
    """what M_SPLIT multiplies"""
    return UNIT[mode] * (o.As + o.Tpv)


def floor_of(mode, o):
    return 2.0 ** -25 * o.Fl if mode == "f16" else torch.zeros_like(o.Fl)


def budget(s, variant, o, m_acc=None, m_exp=None, m_split=None):
    """tol per stored element of one head (module text)"""
    mode = mode_of(s, variant)
    t = (M_ACC if m_acc is None else m_acc) * acc_scale(s, o) + (M_EXP if m_exp is None else m_exp) * exp_scale(o)
    if mode != "f32":
        t = t + (M_SPLIT[mode] if m_split is None else m_split) * split_scale(mode, o) + floor_of(mode, o)
    tol = M * t + 4 * EPS * o.ref.abs()
    if s.planes:
        tol = tol + ((2.0 ** -22 * (o.ref.abs() + tol) + 2.0 ** -25) if mode == "f16" else 2.0 ** -16 * (o.ref.abs() + tol))
    return tol
