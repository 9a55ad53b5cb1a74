"""numpy restatements of the overlapping-window kernels (``pf_window_split`` / ``pf_window_merge`` of include/pfhip.h) and of the plan
arithmetic behind them (``sampler.WindowPlan``), written from the header's definitions and from nothing in the package.

A song is a canvas ``[S, C, canvas_h, W]`` with ``canvas_h = stride * (n_windows - 1) + win_h``; window ``j`` of song ``s`` is batch row
``s * n_windows + j`` and canvas rows ``[j * stride, j * stride + win_h)``.  ``merge32`` restates the kernel operation by operation in
float32 (every numpy float32 operation is one correctly rounded operation, as the kernel's), ``merge64`` is the same blend in float64 on
the SAME float32 weights, and ``budget`` is the error a float32 evaluation may show against it."""
import numpy as np

BLENDS = ("mean", "ramp")
MAX_COVER = 8


def canvas_h(n_windows, stride, win_h):
    return stride * (n_windows - 1) + win_h


def cover(y, n_windows, stride, win_h):
    """The windows over canvas row y, ascending - by the definition, one window at a time."""
    return [j for j in range(n_windows) if 0 <= y - j * stride < win_h]


def valid(n_windows, stride, win_h):
    return n_windows >= 1 and win_h >= 1 and 1 <= stride <= win_h and -(-win_h // stride) <= MAX_COVER


def weights(win_h, stride, blend):
    """float32 [win_h]: ones, or the ramp min(1, r / ov, (win_h - r) / ov) with ov = win_h - stride and r = row + 0.5 (ones when ov == 0)."""
    assert blend in BLENDS
    ov = win_h - stride
    if blend == "mean" or ov == 0:
        return np.ones(win_h, dtype=np.float32)
    return np.array([min(1.0, (row + 0.5) / ov, (win_h - (row + 0.5)) / ov) for row in range(win_h)], dtype=np.float64).astype(np.float32)


def split(canvas, n_windows, stride, win_h):
    """[S, C, canvas_h, W] -> [S * n_windows, C, win_h, W], song-major."""
    S = canvas.shape[0]
    assert canvas.shape[2] == canvas_h(n_windows, stride, win_h)
    return np.stack([canvas[s, :, j * stride: j * stride + win_h, :] for s in range(S) for j in range(n_windows)])


def _rows(eps, songs, n_windows, stride):
    """For every canvas row y: (y, [(j, window row, eps[:, j, :, window row, :] as [S, C, W]) for the covering j ascending])."""
    rows, C, win_h, W = eps.shape
    assert rows == songs * n_windows
    e = eps.reshape(songs, n_windows, C, win_h, W)
    for y in range(canvas_h(n_windows, stride, win_h)):
        yield y, [(j, y - j * stride, e[:, j, :, y - j * stride, :]) for j in cover(y, n_windows, stride, win_h)]


def merge32(eps, w, songs, n_windows, stride):
    """The kernel, operation by operation in float32: one covering window - the value itself; several - num = w_0*e_0, num += w_j*e_j in
    ascending j, den = w_0, den += w_j, out = num / den."""
    assert eps.dtype == np.float32 and w.dtype == np.float32
    _, C, win_h, W = eps.shape
    out = np.empty((songs, C, canvas_h(n_windows, stride, win_h), W), dtype=np.float32)
    for y, cov in _rows(eps, songs, n_windows, stride):
        if len(cov) == 1:
            out[:, :, y, :] = cov[0][2]
            continue
        num = den = None
        for _, r, e in cov:
            term = w[r] * e                                  # float32 scalar * float32 array: one rounded product per element
            num = term if num is None else num + term
            den = w[r] if den is None else np.float32(den + w[r])
        assert num.dtype == np.float32 and isinstance(den, np.float32)
        out[:, :, y, :] = num / den
    return out


def merge64(eps, w, songs, n_windows, stride):
    """The same blend in float64, on the float32 weights as they are."""
    _, C, win_h, W = eps.shape
    e64, w64 = eps.astype(np.float64), w.astype(np.float64)
    out = np.empty((songs, C, canvas_h(n_windows, stride, win_h), W), dtype=np.float64)
    for y, cov in _rows(e64, songs, n_windows, stride):
        if len(cov) == 1:
            out[:, :, y, :] = cov[0][2]
        else:
            out[:, :, y, :] = sum(w64[r] * e for _, r, e in cov) / sum(w64[r] for _, r, _ in cov)
    return out


def budget(eps, w, songs, n_windows, stride):
    """(bound, k): per canvas element, (2k + 2) * 2^-24 * (sum_j w_j |e_j| / sum_j w_j) * (1 + 2^-10) - k products and k - 1 sums on
    either side of the division, and the division, each within half an ulp of an intermediate that the weighted mean of |e| bounds; the
    last factor covers the second-order terms.  Exactly zero where k == 1 (the select).  k: [canvas_h] windows per row."""
    _, C, win_h, W = eps.shape
    e64, w64 = np.abs(eps.astype(np.float64)), w.astype(np.float64)
    hc = canvas_h(n_windows, stride, win_h)
    bound, k = np.zeros((songs, C, hc, W), dtype=np.float64), np.zeros(hc, dtype=np.int64)
    for y, cov in _rows(e64, songs, n_windows, stride):
        k[y] = len(cov)
        if len(cov) > 1:
            mean_abs = sum(w64[r] * e for _, r, e in cov) / sum(w64[r] for _, r, _ in cov)
            bound[:, :, y, :] = (2 * len(cov) + 2) * 2.0 ** -24 * mean_abs * (1 + 2.0 ** -10)
    return bound, k
