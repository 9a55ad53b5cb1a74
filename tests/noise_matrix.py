"""The noise-generator case matrix: the one device function every sample, edit, morph, posterior draw and training loss is built on -
philox_normal4v of csrc/noise.h, Philox4x32-10 followed by Box-Muller - at all seven sites it is drawn (pf_randn, pf_randn_dev, the rng forms
of pf_ddpm_step and pf_ddim_step, pf_qsample_rows, pf_mse_rows and noise_at behind pf_gaussian_sample / pf_normal_rsample), with

  * an integer Philox4x32-10 written from the published definition (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2,
    3", SC'11, and the Random123 known-answer vectors KAT), not from the kernel,
  * the counter layout, as the specification (counters): counter = (g lo, g hi, draw lo, draw hi), key = (seed lo, seed hi), g = global
    element index >> 2, element 4 g + j takes normal j of the group,
  * the uniform mapping stated exactly in fp32 (uniform32 / uniform_exact),
  * a float64 Box-Muller oracle from those fp32 uniforms (oracle_groups),
  * an fp32 emulator of the kernel's own operation order with `defect=` switches (DEFECTS), and
  * the per-element tolerance of profiles/noise_error_model.md (tol).

The uniform mapping is u = ((float)(c >> 8) + 0.5f) * 2^-24 with m = c >> 8 in [0, 2^24).  For m < 2^23 the sum m + 0.5 is an fp32 number
and u = (2 m + 1) 2^-25.  For m >= 2^23 it is not: it rounds to even, to m for an even m and to m + 1 for an odd one, so in [0.5, 1] the
uniforms lie on the grid of 2^-23 and m = 2^24 - 1 gives u = 1.0 exactly.  With u0 = 1.0 the radius is 0 and both normals of the pair are
exactly (+-)0, 2^-24 of all pairs.  u is never 0: the smallest is 2^-25, the largest radius sqrt(50 ln 2) = 5.887, so no draw is infinite
or NaN.  The generator's bits are what goldens, recorded parity runs and users' seeds depend on; the mapping is recorded here, not changed.

The tolerance.  With u fixed (the oracle starts from the same fp32 uniforms) a normal z = r cos(theta) is reached by
    l = logf(u0)            one rounding: relative d1 of l, d1 / 2 of r
    t = -2 l                exact
    r = sqrtf(t)            one rounding d2
    a = 2pi_f32 * u1        one rounding d3 of the angle: cos(a) moves by theta d3 |sin(theta)|
    (s, c) = sincosf(a)     one rounding d4 of each
    z = r * c               one rounding d5
so to first order |dz| <= |z| (|d1| / 2 + |d2| + |d4| + |d5|) + r theta |sin(theta)| |d3|: in units of
    unit = U (|z| + r theta |partner|),     U = 2^-24, partner = sin(theta) for a cosine output, cos(theta) for a sine output
a kernel whose every operation is correctly rounded stays below 3.5.  MEASURED is the largest ratio the emulator (correctly rounded log,
sqrt, sin, cos: numpy's float64 functions rounded once to fp32) reaches, tools/noise_error_model.py; M = MARGIN * MEASURED allows the
device's logf and sincosf an ulp or two each.  On top, outside M, FINAL = 1 rounding of the stored value, U |z|: a bound that holds for
whatever computes z, not an estimate.  tol = M unit + FINAL U |z|.  Where the oracle is exactly 0 (u0 = 1.0: r = 0) the unit and the
tolerance are 0 and the kernel's value must be +-0.  The consumers are launched with operands that make the stored value the draw itself
(products with 1, sums with 0: exact), so they carry the same tolerance; pf_mse_rows' row sum of z^2 carries sum (2 |z| tol + tol^2) and
the float64 summation's (n + 2) 2^-53 sum z^2.  No constant comes from a GPU.

Host only: imports no GPU code.  Used by tests/test_noise_matrix.py (no GPU), tests/test_gpu_noise_matrix.py and tests/test_gpu_ops.py
(-m gpu) and tools/noise_error_model.py."""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32
MARGIN = 4.0
FINAL = 1.0             # roundings of the stored value counted outside M
# measured by tools/noise_error_model.py, recorded in profiles/noise_error_model.md (largest emulator ratio, rounded up to two decimals)
MEASURED = 2.71
M = MARGIN * MEASURED

f32, f64, u64 = np.float32, np.float64, np.uint64
M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
TWO_PI32 = f32(6.283185307179586)      # the kernel's literal 6.283185307179586f


class Spec(dict):
    __getattr__ = dict.__getitem__


class Result(dict):
    __getattr__ = dict.__getitem__


# =====================================================================================================================================
# Philox4x32-10, from the published definition
# =====================================================================================================================================
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57          # the two multipliers
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85          # the Weyl increments of the key: golden ratio, sqrt(3) - 1
# Random123's known-answer vectors for philox4x32-10: (counter, key, output)
KAT = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((M32, M32, M32, M32), (M32, M32), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def philox4x32(ctr, key, rounds=10):
    """Philox4x32-R on Python integers.  One round: (hi0, lo0) = M0 * c0, (hi1, lo1) = M1 * c2,
    c <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); the key is bumped by the Weyl increments before every round but the first."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for r in range(rounds):
        if r:
            k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
    return c0, c1, c2, c3


def counters(seed, draw, g):
    """the specification of the counter layout: group g of draw `draw` under `seed` -> (counter, key)"""
    return (g & M32, (g >> 32) & M32, draw & M32, (draw >> 32) & M32), (seed & M32, (seed >> 32) & M32)


def group_words(seed, draw, g):
    """the four 32-bit outputs of one group, on Python integers"""
    return philox4x32(*counters(seed, draw, g))


def philox_np(c, k, rounds=10, bump_first=False, swap=False):
    """the same rounds on numpy uint64 arrays holding 32-bit words (c: four arrays or scalars, k: two integers) -> uint64 [n][4]"""
    c0, c1, c2, c3 = (np.asarray(x, u64) for x in c)
    k0, k1 = int(k[0]), int(k[1])
    m0, m1 = (PHILOX_M1, PHILOX_M0) if swap else (PHILOX_M0, PHILOX_M1)
    lo, s32 = u64(M32), u64(32)
    for r in range(rounds):
        if r or bump_first:
            k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
        p0, p1 = u64(m0) * c0, u64(m1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ u64(k0), p1 & lo, (p0 >> s32) ^ c3 ^ u64(k1), p0 & lo
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), -1)


DEFECTS = ("nine_rounds", "key_bump_first", "mult_swapped", "sincos_swapped", "pairs_02", "shift9", "no_half", "g_lo_only", "draw_lo_only",
           "seed_lo_only", "elem_index", "offset_ignored", "draws_slot_32")
# the branch a defect lives on: a case that names it in `why` must reject the defect (tests/test_noise_matrix.py)
DEFECT_BRANCH = {"nine_rounds": "kat", "key_bump_first": "kat", "mult_swapped": "kat", "sincos_swapped": "whole_group", "pairs_02": "whole_group",
                 "shift9": "whole_group", "no_half": "tail:small_m", "g_lo_only": "g_hi", "draw_lo_only": "draw_hi", "seed_lo_only": "seed_hi",
                 "elem_index": "past_group_0", "offset_ignored": "offset_nonzero", "draws_slot_32": "draw_carry"}


def words(seed, draw, g, defect=None):
    """uint64 [n][4]: the Philox outputs of groups g (uint64 array) of one draw"""
    g = np.asarray(g, u64)
    (_, _, d0, d1), (k0, k1) = counters(seed, draw, 0)
    g1 = g >> u64(32)
    if defect == "g_lo_only":
        g1 = np.zeros_like(g)
    if defect == "draw_lo_only":
        d1 = 0
    if defect == "seed_lo_only":
        k1 = 0
    return philox_np((g & u64(M32), g1, d0, d1), (k0, k1), rounds=9 if defect == "nine_rounds" else 10,
                     bump_first=defect == "key_bump_first", swap=defect == "mult_swapped")


# =====================================================================================================================================
# the uniform mapping, Box-Muller in float64 and in fp32
# =====================================================================================================================================
def uniform32(m, defect=None):
    """((float)m + 0.5f) * 2^-24 in fp32 arithmetic: the conversion is exact (m < 2^24), the sum is rounded to nearest even, the product
    by a power of two is exact"""
    m = np.asarray(m, u64).astype(f32)
    if defect != "no_half":
        m = m + f32(0.5)
    return m * f32(2.0 ** -24)


def uniform_exact(m):
    """the same value from integers: (2 m + 1) / 2^25 below 2^23, the even neighbour of m + 1/2 over 2^24 from there on"""
    m = int(m)
    if m < 1 << 23:
        return (2 * m + 1) / float(1 << 25)
    return (m + (m & 1)) / float(1 << 24)


def uniforms(w, defect=None):
    return uniform32(w >> u64(9 if defect == "shift9" else 8), defect)


def _pairs(u, defect):
    """(radius uniforms [n][2], angle uniforms [n][2])"""
    if defect == "pairs_02":
        return u[:, (0, 1)], u[:, (2, 3)]
    return u[:, (0, 2)], u[:, (1, 3)]


def oracle_groups(u, defect=None):
    """float64 from the fp32 uniforms [n][4]: r = sqrt(-2 ln u), theta = fp32(2 pi) u (exact in float64: 24 x 24 bits), (r cos, r sin) of
    (u0, u1) and (u2, u3).  z and the tolerance's unit, [n][4]"""
    ur, ua = _pairs(u.astype(f64), None)
    r = np.sqrt(-2.0 * np.log(ur))
    th = f64(TWO_PI32) * ua
    c, s = np.cos(th), np.sin(th)
    z = np.stack([r * c, r * s], -1).reshape(-1, 4)                       # (z0, z1, z2, z3) = (ra ca, ra sa, rb cb, rb sb)
    partner = np.stack([np.abs(s), np.abs(c)], -1).reshape(-1, 4)
    rt = np.repeat(r * th, 2, axis=1)
    return Result(z=z, unit=U * (np.abs(z) + rt * partner))


def emulate_groups(u, defect=None):
    """the kernel's operation order in fp32, every operation correctly rounded: logf, * -2, sqrtf, the angle product, sincosf, the product"""
    ur, ua = _pairs(u, defect)
    with np.errstate(divide="ignore", invalid="ignore"):
        lg = np.log(ur.astype(f64)).astype(f32)
        r = np.sqrt(f32(-2.0) * lg)                                       # numpy's fp32 sqrt is correctly rounded
        ang = (TWO_PI32 * ua).astype(f64)
        c, s = np.cos(ang).astype(f32), np.sin(ang).astype(f32)
        pair = [r * s, r * c] if defect == "sincos_swapped" else [r * c, r * s]
    return np.stack(pair, -1).reshape(-1, 4).astype(f32)


# =====================================================================================================================================
# launches: which draw and which global elements a case's output holds
# =====================================================================================================================================
EW_CAP = 2048 * 256      # lanes of the largest elementwise launch (ew_grid); the grid-stride loop does the rest
KINDS = ("randn", "randn_dev", "ddpm", "ddim", "qsample", "mse", "gauss", "rsample")
VEC4 = ("ddpm", "ddim", "qsample", "mse")       # consumers that own whole groups: n (row_elems) and elem_offset multiples of 4


def draw_of(s, defect=None):
    """the draw index of the case's output: draws + slot in 64 bits (slot 0 and draws = the draw where no device state is involved)"""
    if defect == "draws_slot_32":
        return (s.draws & ~M32) | ((s.draws + s.slot) & M32)
    return (s.draws + s.slot) & M64


def _normals(fn, s, defect=None):
    """fn (oracle_groups or emulate_groups) over the case's elements -> its result sliced to the n elements of the launch, in order"""
    off = 0 if defect == "offset_ignored" else s.off
    draw = draw_of(s, defect)
    if defect == "elem_index":          # the group index taken from the element index itself
        e = u64(off) + np.arange(s.n, dtype=u64)
        return fn(uniforms(words(s.seed, draw, e, defect), defect), defect)[np.arange(s.n), (e & u64(3)).astype(np.int64)]
    g0 = off >> 2
    ng = ((off + s.n + 3) >> 2) - g0
    g = u64(g0) + np.arange(ng, dtype=u64)
    u = uniforms(words(s.seed, draw, g, defect), defect)
    lo = off - 4 * g0
    if fn is oracle_groups:
        o = fn(u)
        return Result(z=o.z.reshape(-1)[lo:lo + s.n], unit=o.unit.reshape(-1)[lo:lo + s.n])
    return fn(u, defect).reshape(-1)[lo:lo + s.n]


def oracle(s):
    """Result(z, unit): float64 [n], the n elements the launch stores (rows * row_elems for the row kernels), in order"""
    return _normals(oracle_groups, s)


def emulate(s, defect=None):
    """fp32 [n]: what a kernel with every operation correctly rounded stores"""
    return _normals(emulate_groups, s, defect)


def tol(o, m=None):
    return (M if m is None else m) * o.unit + FINAL * U * np.abs(o.z)


def ratio(got, o, m=None):
    """largest |got - z| / tol; a NaN or an infinity anywhere, or an error where the tolerance is zero, is infinite"""
    got = np.asarray(got, f64)
    if got.size == 0:
        return 0.0
    err, t = np.abs(got - o.z), tol(o, m)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / t)
    r = np.where(np.isfinite(got), r, np.inf)
    return float(np.nan_to_num(r, nan=np.inf, posinf=np.inf).max())


def unit_ratio(got, o):
    """what tools/noise_error_model.py measures: largest |got - z| / unit (an element whose unit is 0 must be exact)"""
    err = np.abs(np.asarray(got, f64) - o.z)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / o.unit)
    return float(np.nan_to_num(r, nan=np.inf, posinf=np.inf).max()) if r.size else 0.0


def mse_oracle(s, o):
    """pf_mse_rows with eps_theta = 0: (row sums of z^2 [rows], their tolerance): every element within its own tolerance, then a float64
    sum of row_elems exact squares in some order"""
    z, t = o.z.reshape(s.rows, s.row_elems), tol(o).reshape(s.rows, s.row_elems)
    want = np.array([math.fsum(row * row) for row in z])
    return want, (2 * np.abs(z) * t + t * t).sum(1) + (s.row_elems + 2) * 2.0 ** -53 * want


# =====================================================================================================================================
# the case table
# =====================================================================================================================================
BIG_RANDN = EW_CAP * 4 + 4 * 256 + 5       # pf_randn just over the grid cap: a second, ragged grid-stride pass
BIG_VEC4 = EW_CAP * 4 + 1024               # the ew_launch_v<4> consumers: 256 groups in the second pass
BIG_VEC1 = EW_CAP + 257                    # the ew_launch_v<1> consumers (noise_at): 257 elements in the second pass
DRAWS = (0, 1, (1 << 32) - 1, 1 << 32, (1 << 63) + 5)
SEEDS = (0, 1, (1 << 32) - 1, 1 << 32, 0x9E3779B97F4A7C15)
DEV_DRAWS, DEV_SLOTS = (0, 5, (1 << 32) - 1), (0, 1, 2)
RANDN_N = (1, 2, 3, 4, 5, 7, 8, 4097)
SEED0, DRAW0 = 1234, 7                     # the seed and draw of the cases that are about something else
# a launch addresses elements below 2^64, so a group index has 62 bits and the counter words of the second and third known-answer vector
# cannot be reached whole: their cases keep seed and draw and take the group modulo 2^61 (the first vector's is group 0).  The integer
# reference itself is held to all three vectors on the host.
KAT_GROUP_BITS = 61


def kat_triples():
    """(seed, draw, group) of the known-answer counters, the group reduced to what a launch can address"""
    out = []
    for (c0, c1, c2, c3), (k0, k1), _ in KAT:
        out.append((k0 | k1 << 32, c2 | c3 << 32, (c0 | c1 << 32) & ((1 << KAT_GROUP_BITS) - 1)))
    return out


# Found by tools/noise_error_model.py (a CPU search over the groups of seed 1234, draw 7, in index order) and re-verified against the integer
# reference by tests/test_noise_matrix.py: name -> ((group, word, m = that word >> 8), ...)
TAILS = {
    'small_m': ((1791576, 2, 7), (1812657, 2, 4), (3867054, 0, 8), (4896558, 2, 3)),
    'u_one': ((974488, 2, 16777215),),
    'm_2^23': ((2758094, 0, 8388608),),
    'm_2^23+1': ((3160723, 2, 8388609),),
    'angle_2pi': ((670733, 1, 16777215),),
}
TAIL_WANT = {"small_m": lambda j, m: j in (0, 2) and m <= 8, "u_one": lambda j, m: j in (0, 2) and m == (1 << 24) - 1,
             "m_2^23": lambda j, m: m == 1 << 23, "m_2^23+1": lambda j, m: m == (1 << 23) + 1,
             "angle_2pi": lambda j, m: j in (1, 3) and m == (1 << 24) - 1}


def _lanes(s):
    """(work items of the launch, lanes of its grid): a grid-stride pass runs when the first exceeds the second"""
    if s.kind in ("randn", "randn_dev"):
        return ((s.off + s.n + 3) >> 2) - (s.off >> 2), 256 * min(2048, (s.n // 4 + 1 + 255) // 256)
    if s.kind in ("ddpm", "ddim"):
        return s.n // 4, 256 * min(2048, (s.n // 4 + 255) // 256)
    if s.kind in ("gauss", "rsample"):
        return s.n, 256 * min(2048, (s.n + 255) // 256)
    return 0, 1          # the row kernels: one workgroup per chunk, no loop


def branches_of(s):
    out = {f"entry:{s.kind}" + (f":{s.variant}" if s.get("variant") else "")}
    off, n = s.off, s.n
    g0, g1 = off >> 2, (off + n - 1) >> 2
    out.add(f"off%4:{off % 4}")
    if s.kind == "randn":
        out.add(f"n:{n}")
    if off % 4:
        out.add("partial_first_group")
    if (off + n) % 4:
        out.add("partial_last_group")
    if g0 == g1 and off % 4 and (off + n) % 4:
        out.add("inside_group")
    if (off + 3) // 4 * 4 + 4 <= off + n:
        out.add("whole_group")
    if off:
        out.add("offset_nonzero")
    if g1 > 0:
        out.add("past_group_0")
    items, lanes = _lanes(s)
    if items > lanes:
        out.add("grid_stride")
        if items % lanes:
            out.add("ragged_stride")
    if g1 >= 1 << 32:
        out.add("g_hi")
    if g0 < 1 << 32 <= g1:
        out.add("g_crosses_2^32")
    draw = draw_of(s)
    out.add(f"draw:{draw:#x}")
    out.add(f"seed:{s.seed:#x}")
    if draw >= 1 << 32:
        out.add("draw_hi")
    if s.seed >= 1 << 32:
        out.add("seed_hi")
    if s.get("state"):
        out |= {f"draws:{s.draws:#x}", f"slot:{s.slot}"}
        if (s.draws & M32) + s.slot > M32:
            out.add("draw_carry")
    if s.kind in ("qsample", "mse"):
        out |= {f"rows:{s.rows}", f"row_elems:{s.row_elems}"}
        if s.row_elems > (1024 if s.kind == "qsample" else 2048):
            out.add("second_chunk")
    if g1 - g0 < 4:          # what the groups themselves hold: the tails and the known-answer counters
        for g in range(g0, g1 + 1):
            w = group_words(s.seed, draw, g)
            for name, want in TAIL_WANT.items():
                # (the pair of elements a word feeds, 4 g + (j & ~1) and the next, must reach into the launch)
                if any(want(j, w[j] >> 8) and 4 * g + (j & 2) < off + n and 4 * g + (j & 2) + 1 >= off for j in range(4)):
                    out.add(f"tail:{name}")
            if (s.seed, draw, g) in kat_triples():
                out |= {"kat", f"kat:{kat_triples().index((s.seed, draw, g))}"}
    return out


REQUIRED = ({f"off%4:{k}" for k in range(4)} | {f"n:{n}" for n in RANDN_N + (BIG_RANDN,)}
            | {"partial_first_group", "partial_last_group", "inside_group", "whole_group", "offset_nonzero", "past_group_0", "grid_stride",
               "ragged_stride", "g_hi", "g_crosses_2^32", "draw_hi", "seed_hi", "draw_carry", "kat", "kat:0", "kat:1", "kat:2", "second_chunk"}
            | {f"draw:{d:#x}" for d in DRAWS} | {f"seed:{v:#x}" for v in SEEDS} | {f"tail:{t}" for t in TAIL_WANT}
            | {f"draws:{d:#x}" for d in DEV_DRAWS} | {f"slot:{k}" for k in DEV_SLOTS}
            | {"entry:randn", "entry:randn_dev", "entry:ddpm:plain", "entry:ddpm:q", "entry:ddpm:p", "entry:ddpm:state_q", "entry:ddpm:state_p",
               "entry:ddim:plain", "entry:ddim:state", "entry:qsample", "entry:mse", "entry:gauss", "entry:rsample"})


def _case(kind, n, off=0, seed=SEED0, draws=DRAW0, slot=0, why=(), **kw):
    s = Spec(kind=kind, n=n, off=off, seed=seed, draws=draws, slot=slot, why=tuple(why), **kw)
    key = kind + (f":{kw['variant']}" if kw.get("variant") else "")
    key += f" rows{kw['rows']}x{kw['row_elems']}" if "rows" in kw else f" n{n}"
    key += f" off{off:#x}" if off >= 1 << 16 else f" off{off}"
    key += f" seed{seed:#x} draw{draws:#x}" + (f"+{slot}" if kw.get("state") else "")
    return key, s


def _rows(kind, rows, row_elems, off, why=(), **kw):
    return _case(kind, rows * row_elems, off, rows=rows, row_elems=row_elems, why=why, **kw)


def cases(only=None):
    out = []
    # pf_randn: every alignment of the first element with every length, each on a region of its own
    for i, n in enumerate(RANDN_N):
        for k in range(4):
            why = [f"off%4:{k}", f"n:{n}"] + (["inside_group"] if n == 1 and k in (1, 2) else [])
            why += ["whole_group"] if n >= 7 else []
            out.append(_case("randn", n, 4 * 37 * (4 * i + k) + k, why=why + (["offset_nonzero", "past_group_0"] if i + k else [])))
    out.append(_case("randn", BIG_RANDN, 3, why=("grid_stride", "ragged_stride", f"n:{BIG_RANDN}", "partial_first_group")))
    # counter words
    out.append(_case("randn", 8, (1 << 34) - 4, why=("g_crosses_2^32", "g_hi")))
    out.append(_case("randn", 5, (1 << 40) + 3, why=("g_hi", "partial_first_group")))
    for d in DRAWS:
        for sd in SEEDS:
            why = [f"draw:{d:#x}", f"seed:{sd:#x}"] + (["draw_hi"] if d >> 32 else []) + (["seed_hi"] if sd >> 32 else [])
            out.append(_case("randn", 8, 2, seed=sd, draws=d, why=why))
    for i, (sd, d, g) in enumerate(kat_triples()):
        out.append(_case("randn", 4, 4 * g, seed=sd, draws=d, why=("kat", f"kat:{i}")))
    # tails
    tails = {}
    for name, found in TAILS.items():
        for g, j, m in found:
            tails.setdefault(g, []).append(f"tail:{name}")
    for g, why in tails.items():
        out.append(_case("randn", 4, 4 * g, why=why))
    # pf_randn_dev: the draw index is the device counter plus the slot, in 64 bits
    for d in DEV_DRAWS:
        for slot in DEV_SLOTS:
            why = [f"draws:{d:#x}", f"slot:{slot}"] + (["draw_carry", "draw_hi"] if (d & M32) + slot > M32 else [])
            out.append(_case("randn_dev", 9, 5, draws=d, slot=slot, state=1, why=why))
    # the consumers that own whole groups, at 8 elements and over the grid cap
    for n, off in ((8, 12), (BIG_VEC4, 1 << 20)):
        big = ("grid_stride", "ragged_stride") if n > 8 else ()
        out.append(_case("ddpm", n, off, variant="plain", why=("entry:ddpm:plain",) + big))
        out.append(_case("ddpm", n, off, variant="q", why=("entry:ddpm:q",) + big))
        out.append(_case("ddim", n, off, variant="plain", why=("entry:ddim:plain",) + big))
    out.append(_case("ddpm", 8, 12, variant="p", why=("entry:ddpm:p",)))
    out.append(_case("ddpm", 8, (1 << 34) - 4, variant="plain", why=("entry:ddpm:plain", "g_crosses_2^32")))
    out.append(_case("ddpm", 8, 12, draws=M32, slot=0, state=1, variant="state_q", why=("entry:ddpm:state_q", f"draws:{M32:#x}")))
    out.append(_case("ddpm", 8, 12, draws=M32, slot=1, state=1, variant="state_p", why=("entry:ddpm:state_p", "draw_carry")))
    out.append(_case("ddim", 8, 12, draws=(1 << 32) + 9, slot=0, state=1, variant="state", why=("entry:ddim:state", "draw_hi")))
    # the row kernels: x_t and noise_out of pf_qsample_rows, the row sums of pf_mse_rows
    for kind in ("qsample", "mse"):
        out.append(_rows(kind, 2, 8, 16, why=(f"entry:{kind}", "row_elems:8", "rows:2")))
        out.append(_rows(kind, 2, 4 * 256 + 4, 1 << 12, why=(f"entry:{kind}", f"row_elems:{4 * 256 + 4}") + (("second_chunk",) if kind == "qsample" else ())))
    out.append(_rows("mse", 3, 2048 + 4 * 256 + 4, (1 << 34) - 2048, why=("entry:mse", "second_chunk", "g_crosses_2^32")))
    # noise_at: any n, any offset - every position of the first element in its group, and the strided pass
    for kind in ("gauss", "rsample"):
        for k in range(4):
            out.append(_case(kind, 6, 40 + k, why=(f"entry:{kind}", f"off%4:{k}")))
        out.append(_case(kind, BIG_VEC1, 3, why=(f"entry:{kind}", "grid_stride", "ragged_stride")))
        out.append(_case(kind, 5, (1 << 34) - 2, draws=(1 << 63) + 5, seed=SEEDS[4], why=(f"entry:{kind}", "g_crosses_2^32", "draw_hi", "seed_hi")))
    # the tails through the consumers: a stored -0 must come out as a zero, the largest radius unharmed
    for name in ("u_one", "small_m"):
        for g, j, m in TAILS[name][:1]:
            out.append(_case("ddpm", 4, 4 * g, variant="plain", why=(f"tail:{name}", "entry:ddpm:plain")))
            out.append(_case("gauss", 4, 4 * g, why=(f"tail:{name}", "entry:gauss")))
    return [c for c in out if only is None or c[1].kind == only]
