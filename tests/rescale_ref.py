"""Guidance rescale (``pf_cfg_rescale``) restated in numpy from its definition alone; nothing here imports the package under test.

Per row of ``row_elems`` floats, with ``e_cfg`` the guidance combine of the groups in float32 - ``pf_cfg_combine``'s three or
``pf_cfg_combine3``'s five individually rounded operations, in their order - and ``e_pos`` the fully conditional (last) group::

    four sums: e_pos, e_pos^2, e_cfg, e_cfg^2        every term widened to float64 first, added with math.fsum (correctly rounded; the
                                                     kernel adds in double-double and rounds once: the same value but for near-ties)
    var = sum x^2 / n - (sum x / n)^2 ;  f = sqrt(var_pos / var_cfg)                   float64, each operation rounded
    f = 1  when var_cfg is not > 0 or the root is not finite
    w = float32(phi * f + (1 - phi)) ;  out = float32(e_cfg * w)

``FIELDS``: the members of ``pf_cfg_rescale_args`` in the header's order."""
import math

import numpy as np

FIELDS = ("epsg", "eps", "stats", "weights", "workspace", "workspace_bytes", "phi", "s1", "s2", "groups", "rows", "row_elems")


def combine_f32(groups, s1, s2=0.0):
    """``e_cfg`` of ``groups`` = ``[G, ...]`` float32, G in (2, 3): the combine step by step in float32, in ``cfg_combine_v``'s /
    ``cfg_combine3_v``'s order."""
    f = np.float32
    g = np.asarray(groups, dtype=f)
    assert g.shape[0] in (2, 3)
    s1, s2 = f(s1), f(s2)
    with np.errstate(invalid="ignore", over="ignore"):
        a1 = (g[0] + (s1 * (g[1] - g[0]).astype(f)).astype(f)).astype(f)
        if g.shape[0] == 2:
            return a1
        return (a1 + (s2 * (g[2] - g[1]).astype(f)).astype(f)).astype(f)


def row_sums(e_pos, e_cfg):
    """float64 ``[rows, 4]``: the correctly rounded sums of e_pos, e_pos^2, e_cfg, e_cfg^2 (squares of widened floats are exact), and
    ``[rows, 4]`` the sums of the terms' magnitudes - what a bound on another summation order scales with."""
    p, c = np.asarray(e_pos, dtype=np.float64), np.asarray(e_cfg, dtype=np.float64)
    p, c = p.reshape(p.shape[0], -1), c.reshape(c.shape[0], -1)
    terms = (p, p * p, c, c * c)
    sums = np.array([[math.fsum(t[r]) for t in terms] for r in range(p.shape[0])], dtype=np.float64)
    mags = np.array([[math.fsum(np.abs(t[r])) for t in terms] for r in range(p.shape[0])], dtype=np.float64)
    return sums, mags


def dd_add(x, y):
    """One double-double addition as the kernel performs it, on ``(hi, lo)`` pairs of Python floats: the rounding error of ``hi + hi`` kept
    exactly (TwoSum) and folded into ``lo``, then renormalised."""
    s = x[0] + y[0]
    bb = s - x[0]
    e = (x[0] - (s - bb)) + (y[0] - bb)
    e = e + (x[1] + y[1])
    hi = s + e
    return hi, e - (hi - s)


def chunk_order_sums(ws):
    """The four sums of every row from the workspace ``pf_cfg_rescale`` leaves, ``[rows, chunks, 4, 2]`` (hi, lo): a row's pairs added in
    chunk order in double-double, the total's ``hi`` - what the combine launch forms.  float64 ``[rows, 4]``."""
    ws = np.asarray(ws, dtype=np.float64)
    out = np.zeros((ws.shape[0], 4))
    for r in range(ws.shape[0]):
        for k in range(4):
            t = (0.0, 0.0)
            for c in range(ws.shape[1]):
                t = dd_add(t, (float(ws[r, c, k, 0]), float(ws[r, c, k, 1])))
            out[r, k] = t[0]
    return out


def factors(sums, n, phi):
    """``(var_pos, var_cfg, f, w)`` per row from the four sums of rows of ``n`` elements: float64, float64, float64, float32."""
    s = np.asarray(sums, dtype=np.float64)
    n = np.float64(n)
    mp, mc = s[:, 0] / n, s[:, 2] / n
    var_pos, var_cfg = s[:, 1] / n - mp * mp, s[:, 3] / n - mc * mc
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        f = np.sqrt(var_pos / var_cfg)
    f = np.where((var_cfg > 0.0) & np.isfinite(f), f, 1.0)
    phi = np.float64(phi)
    w = (phi * f + (np.float64(1.0) - phi)).astype(np.float32)
    return var_pos, var_cfg, f, w


def scale_rows(e_cfg, w):
    """``float32(e_cfg * w)`` with one ``w`` per row: one rounded product."""
    e = np.asarray(e_cfg, dtype=np.float32)
    w = np.asarray(w, dtype=np.float32).reshape((-1,) + (1,) * (e.ndim - 1))
    with np.errstate(invalid="ignore", over="ignore"):
        return (e * w).astype(np.float32)


def rescale(groups, s1, s2, phi):
    """The whole definition on ``groups`` = ``[G, rows, ...]``: a dict with ``out`` (float32 ``[rows, ...]``), ``e_cfg``, ``var_pos``,
    ``var_cfg``, ``f`` (float64 ``[rows]``), ``w`` (float32 ``[rows]``), ``sums`` and ``mags`` (float64 ``[rows, 4]``)."""
    g = np.asarray(groups, dtype=np.float32)
    e_cfg = combine_f32(g, s1, s2)
    sums, mags = row_sums(g[-1], e_cfg)
    n = int(np.prod(g.shape[2:])) if g.ndim > 2 else 1
    var_pos, var_cfg, f, w = factors(sums, n, phi)
    return dict(out=scale_rows(e_cfg, w), e_cfg=e_cfg, var_pos=var_pos, var_cfg=var_cfg, f=f, w=w, sums=sums, mags=mags)


def std_rows(x):
    """The population standard deviation of every row in float64, two-pass (the textbook form, not the kernel's)."""
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(x.shape[0], -1)
    return np.sqrt(np.mean((x - x.mean(axis=1, keepdims=True)) ** 2, axis=1))


def interval_from_fractions(lo, hi, n_steps):
    """``--guidance_interval LO HI``: ``(ceil(LO * (T - 1)), floor(HI * (T - 1)))``; the whole schedule is ``None``."""
    t_lo, t_hi = math.ceil(lo * (n_steps - 1)), math.floor(hi * (n_steps - 1))
    return None if (t_lo, t_hi) == (0, n_steps - 1) else (t_lo, t_hi)
