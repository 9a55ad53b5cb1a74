"""A path between two noises, restated in numpy / float64 (imports nothing from the product): the three sums per row, the slerp / lerp
weights with the fallback rule of ``pf_slerp_rows`` (include/pfhip.h), the float32 frames with individually rounded operations, and the
fractions of ``morph_fractions``."""
import math

import numpy as np

FALLBACK = 2.0 ** -20          # 1 - |cos theta| below this: the lerp weights stand in for the slerp weights
FIELDS = ("a", "b", "t", "out", "stats", "weights", "workspace", "workspace_bytes", "mode", "frames", "rows", "row_elems")


def stats(a, b) -> np.ndarray:
    """float64 ``[rows, 3]``: sum a*a, sum a*b, sum b*b per row - the float64 products are exact, ``math.fsum`` adds them exactly and rounds once."""
    a2, b2 = (np.asarray(v, dtype=np.float32).reshape(np.shape(v)[0], -1).astype(np.float64) for v in (a, b))
    return np.array([[math.fsum(p * p), math.fsum(p * q), math.fsum(q * q)] for p, q in zip(a2, b2)], dtype=np.float64).reshape(-1, 3)


def abs_terms(a, b) -> np.ndarray:
    """float64 ``[rows, 3]``: the sums of the absolute values of the same terms (what a summation error bound is relative to)."""
    a2, b2 = (np.asarray(v, dtype=np.float32).reshape(np.shape(v)[0], -1).astype(np.float64) for v in (a, b))
    return np.array([[math.fsum(p * p), math.fsum(np.abs(p * q)), math.fsum(q * q)] for p, q in zip(a2, b2)], dtype=np.float64).reshape(-1, 3)


def falls_back(st) -> np.ndarray:
    """bool ``[rows]``: the rows that take the lerp weights - a zero row, or rows (anti)parallel to within ``1 - |c| < 2^-20``."""
    st = np.asarray(st, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(len(st), dtype=bool)
    for r, (aa, ab, bb) in enumerate(st):
        out[r] = aa == 0.0 or bb == 0.0 or 1.0 - abs(ab / math.sqrt(aa * bb)) < FALLBACK
    return out


def angles(st) -> np.ndarray:
    """float64 ``[rows]``: theta = acos(ab / sqrt(aa*bb)); NaN for a zero row."""
    st = np.asarray(st, dtype=np.float64).reshape(-1, 3)
    return np.array([math.acos(max(-1.0, min(1.0, ab / math.sqrt(aa * bb)))) if aa > 0 and bb > 0 else math.nan for aa, ab, bb in st])


def weights(st, fracs, mode: str = "slerp") -> np.ndarray:
    """float64 ``[frames, rows, 2]``: ``(w0, w1)`` per frame and row, not yet rounded to float32."""
    st = np.asarray(st, dtype=np.float64).reshape(-1, 3)
    fb = np.ones(len(st), dtype=bool) if mode == "lerp" else falls_back(st)
    w = np.empty((len(fracs), len(st), 2), dtype=np.float64)
    for k, t in enumerate(fracs):
        t = float(t)
        for r, (aa, ab, bb) in enumerate(st):
            if fb[r]:
                w[k, r] = (1.0 - t, t)
                continue
            theta = math.acos(ab / math.sqrt(aa * bb))
            sn = math.sin(theta)
            w[k, r] = (math.sin((1.0 - t) * theta) / sn, math.sin(t * theta) / sn)
    return w


def frames(a, b, w32, fracs=None) -> np.ndarray:
    """float32 ``[frames, rows, ...]``: ``fl(fl(w0*a) + fl(w1*b))`` with the float32 weights ``w32 [frames, rows, 2]``; with ``fracs``, a
    frame at ``t == 0`` / ``t == 1`` is a copy of ``a`` / ``b`` (numpy's float32 ``*`` and ``+`` round once each and never contract)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    w32 = np.asarray(w32, dtype=np.float32)
    out = np.empty((w32.shape[0],) + a.shape, dtype=np.float32)
    shape = (a.shape[0],) + (1,) * (a.ndim - 1)
    for k in range(w32.shape[0]):
        p = (w32[k, :, 0].reshape(shape) * a).astype(np.float32)
        q = (w32[k, :, 1].reshape(shape) * b).astype(np.float32)
        out[k] = p + q
        if fracs is not None and float(fracs[k]) == 0.0:
            out[k] = a
        if fracs is not None and float(fracs[k]) == 1.0:
            out[k] = b
    return out


def fractions(n: int, ease: str = "linear") -> np.ndarray:
    if n == 1:
        return np.array([0.5])
    lin = np.array([k / (n - 1) for k in range(n)], dtype=np.float64)
    if ease == "linear":
        return lin
    if ease == "cosine":
        return np.array([(1.0 - math.cos(math.pi * v)) / 2.0 for v in lin])
    raise ValueError(ease)
