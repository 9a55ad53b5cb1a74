"""numpy restatement of ``pf_x0_threshold`` (include/pfhip.h), written from the definition and from nothing of the kernels: float32 arrays
for the fp32 operations (numpy rounds every elementwise operation on its own), ``np.sort`` of the ``uint32`` views for the order
statistics, Python floats (float64) for ``q``, ``s`` and ``w``."""
import math

import numpy as np

FIELDS = ("x", "x_row_stride", "eps", "eps_out", "t", "t_stride", "table", "n_table", "stats", "workspace", "workspace_bytes", "p", "s_max",
          "lo", "hi", "mode", "form", "rows", "row_elems")
F = np.float32


def table_of(alpha_bar):
    """``[n, 4]`` float32: 1/sqrt(ab), sqrt(1-ab)/sqrt(ab), 1/sqrt(1-ab), sqrt(ab)/sqrt(1-ab) of the float32 ``alpha_bar``, float64 rounded once."""
    ab = np.asarray(alpha_bar, dtype=np.float32).astype(np.float64)
    ra, rb = np.sqrt(ab), np.sqrt(1.0 - ab)
    return np.stack([1.0 / ra, rb / ra, 1.0 / rb, ra / rb], axis=1).astype(np.float32)


def order_stats(a_bits, p):
    """``(k, frac, a_k, a_k1)`` of the sorted ``uint32`` patterns: ``pos = p * (n - 1)``, ``k = floor(pos)``, ``a_(n) := a_(n-1)``."""
    n = a_bits.size
    srt = np.sort(a_bits)
    pos = float(p) * float(n - 1)
    k = int(math.floor(pos))
    return k, pos - k, srt[k], srt[min(k + 1, n - 1)]


def quantile(a_bits, p):
    """The ``p``-quantile of the non-negative floats whose patterns are ``a_bits``, ``torch.quantile``'s linear rule, each operation rounded."""
    _, frac, bk, bk1 = order_stats(a_bits, p)
    ak, ak1 = float(np.uint32(bk).view(F)), float(np.uint32(bk1).view(F))
    with np.errstate(all="ignore"):
        return float(np.float64(ak) + np.float64(frac) * (np.float64(ak1) - np.float64(ak)))


def clamp(v, lo, hi):
    """``v < lo ? lo : v > hi ? hi : v`` elementwise: a NaN stays NaN."""
    with np.errstate(invalid="ignore"):
        return np.where(v < lo, F(lo), np.where(v > hi, F(hi), v)).astype(F)


def threshold_row(x, eps, coef, mode, p=0.995, lo=0.0, hi=1.0, s_max=math.inf):
    """One row.  ``x`` / ``eps`` float32 ``[n]``, ``coef`` the row's four float32 table entries.  Returns ``(eps', [q, s, w, count])``."""
    x, eps = np.asarray(x, F), np.asarray(eps, F)
    cx, ce, kx, k0 = (F(v) for v in coef)
    lo, hi = F(lo), F(hi)
    with np.errstate(all="ignore"):
        x0 = (cx * x).astype(F) - (ce * eps).astype(F)
        q = s = math.nan
        w = 1.0
        kind = "clip"
        if mode == "dynamic":
            c = F((float(lo) + float(hi)) / 2.0)
            h = (float(hi) - float(lo)) / 2.0
            u = (x0 - c).astype(F)
            q = quantile(u.view(np.uint32) & np.uint32(0x7FFFFFFF), p)
            if not math.isfinite(q):
                kind = "copy"
            else:
                s = min(max(q, h), float(s_max) * h)
                if s != h:
                    kind, w = "scale", float(F(h / s))
        if kind == "copy":
            return eps.copy(), np.array([q, s, w, 0.0])
        if kind == "clip":
            y = clamp(x0, lo, hi)
        else:
            sf = F(s)
            y = (c + (clamp(u, -sf, sf) * F(w)).astype(F)).astype(F)
        same = y == x0
        out = np.where(same, eps, (kx * x).astype(F) - (k0 * y).astype(F)).astype(F)
    return out, np.array([q, s, w, float((~same).sum())])


def threshold(x, eps, t, table, mode, p=0.995, lo=0.0, hi=1.0, s_max=math.inf, t_stride=1):
    """All rows: ``x`` ``[rows, >= n]`` (only the first ``n`` elements of a row are the state), ``eps`` ``[rows, n]``, ``t`` int64.
    Returns ``(eps' [rows, n] float32, stats [rows, 4] float64)``."""
    x, eps = np.asarray(x, F), np.asarray(eps, F)
    rows, n = eps.shape
    out, stats = np.empty_like(eps), np.empty((rows, 4))
    for r in range(rows):
        tv = min(max(int(t[r * t_stride]), 0), table.shape[0] - 1)
        out[r], stats[r] = threshold_row(x[r, :n], eps[r], table[tv], mode, p, lo, hi, s_max)
    return out, stats
