"""The definition of ``pf_roll_pack`` / ``pf_roll_match`` (include/pfhip.h) in numpy, from the float images: thresholding, the shifted
boolean images, inter / union, the exact cross-multiplied ordering, the best shift per corpus window and the top-k, with plain loops.
A second formulation on one 128-bit Python integer per row (``match_ints``) shares nothing with the first but ``shift_of``.
Not a test module; imported by tests/test_rollmatch_host.py and tests/test_gpu_rollmatch.py."""
import numpy as np


def round_(v, custom_round=False):
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        return ((v > np.float32(0.95)) & (v < np.float32(1.05))) if custom_round else (v > np.float32(0.5))


def planes(x, custom_round=False):
    """``[n, 2, steps, 128]`` float -> boolean ``[2, n * steps, 128]``: plane 0 onset, plane 1 sounding = onset | sustain"""
    x = np.asarray(x, np.float32)
    on = round_(x[:, 0], custom_round)
    snd = on | round_(x[:, 1], custom_round)
    return np.stack([on.reshape(-1, 128), snd.reshape(-1, 128)])


def pack(x, custom_round=False):
    """``[2, n * steps, 4]`` uint32: key k is bit k % 32 of word k / 32"""
    p = planes(x, custom_round)
    out = np.zeros(p.shape[:2] + (4,), np.uint32)
    for k in range(128):
        out[:, :, k // 32] |= p[:, :, k].astype(np.uint32) << np.uint32(k % 32)
    return out


def windows(rows, starts, steps):
    """``rows [R, 128]`` bool, ``starts`` -> ``[len(starts), steps, 128]``"""
    return np.stack([rows[s:s + steps] for s in starts]) if len(starts) else np.zeros((0, steps, 128), bool)


def shift_of(k):
    return -((k + 1) // 2) if k % 2 else k // 2


def shift_image(q, s):
    """qs[t][j] = q[t][j + s] where 0 <= j + s < 128, else False"""
    out = np.zeros_like(q)
    for j in range(128):
        if 0 <= j + s < 128:
            out[:, j] = q[:, j + s]
    return out


def better(ai, au, bi, bu):
    """inter / union of a strictly greater than that of b, exactly; a union of 0 is 0 / 1"""
    if au == 0:
        ai, au = 0, 1
    if bu == 0:
        bi, bu = 0, 1
    return int(ai) * int(bu) > int(bi) * int(au)


def topk_of(tab_inter, tab_union, tab_shift, topk):
    """Per query the ``topk`` best windows, descending, ties to the lowest b; slots beyond nb are -1, 0, 0, 0."""
    na, nb = tab_inter.shape
    index, shift = np.full((na, topk), -1, np.int32), np.zeros((na, topk), np.int32)
    inter, union = np.zeros((na, topk), np.int32), np.zeros((na, topk), np.int32)
    for a in range(na):
        kept = []                                   # indices, best first
        for b in range(nb):
            pos = len(kept)
            while pos > 0 and better(tab_inter[a, b], tab_union[a, b], tab_inter[a, kept[pos - 1]], tab_union[a, kept[pos - 1]]):
                pos -= 1                            # strictly better only: an equal earlier b stays in front
            if pos < topk:
                kept.insert(pos, b)
                del kept[topk:]
        for r, b in enumerate(kept):
            index[a, r], shift[a, r], inter[a, r], union[a, r] = b, tab_shift[a, b], tab_inter[a, b], tab_union[a, b]
    return dict(index=index, shift=shift, inter=inter, union=union)


def match(qwin, cwin, shifts, topk):
    """``qwin [na, steps, 128]``, ``cwin [nb, steps, 128]`` bool -> dict of index / shift / inter / union ``[na, topk]`` and the dense
    tab_inter / tab_union / tab_shift ``[na, nb]``, all int32."""
    na, nb = len(qwin), len(cwin)
    csize = cwin.reshape(nb, -1).sum(1).astype(np.int64)
    ti, tu, ts = (np.zeros((na, nb), np.int32) for _ in range(3))
    for a in range(na):
        per_k = []
        for k in range(2 * shifts + 1):
            qs = shift_image(qwin[a], shift_of(k))
            inter = (qs[None] & cwin).reshape(nb, -1).sum(1).astype(np.int64)
            per_k.append((inter, int(qs.sum()) + csize - inter))
        for b in range(nb):
            bk = 0
            for k in range(1, 2 * shifts + 1):
                if better(per_k[k][0][b], per_k[k][1][b], per_k[bk][0][b], per_k[bk][1][b]):
                    bk = k
            ti[a, b], tu[a, b], ts[a, b] = per_k[bk][0][b], per_k[bk][1][b], shift_of(bk)
    return dict(topk_of(ti, tu, ts, topk), tab_inter=ti, tab_union=tu, tab_shift=ts)


def match_images(xq, q_starts, xc, c_starts, steps, shifts, topk, plane=0, custom_round=False):
    """The whole path from float images: threshold, cut the windows, match."""
    return match(windows(planes(xq, custom_round)[plane], q_starts, steps), windows(planes(xc, custom_round)[plane], c_starts, steps), shifts, topk)


# ------------------------------------------------------------------ second formulation: a row is one Python integer of 128 bits
ALL = (1 << 128) - 1


def rows_as_ints(win):
    return [[sum(1 << j for j in range(128) if row[j]) for row in w] for w in win]


def match_ints(qwin, cwin, shifts, topk):
    """As ``match``.  The window is shifted instead of the query: sum_j q[j + s] c[j] = sum_i q[i] c[i - s]."""
    q, c = rows_as_ints(qwin), rows_as_ints(cwin)
    pop = lambda v: bin(v).count("1")
    up = lambda v, s: ((v << s) & ALL) if s >= 0 else (v >> -s)
    na, nb = len(q), len(c)
    ti, tu, ts = (np.zeros((na, nb), np.int32) for _ in range(3))
    for a in range(na):
        for b in range(nb):
            best = None
            for k in range(2 * shifts + 1):
                s = shift_of(k)
                inter = sum(pop(qr & up(cr, s)) for qr, cr in zip(q[a], c[b]))
                union = sum(pop(qr & up(ALL, s)) for qr in q[a]) + sum(pop(cr) for cr in c[b]) - inter
                num, den = (inter, union) if union else (0, 1)
                if best is None or num * best[1] > best[0] * den:
                    best = (num, den, inter, union, s)
            ti[a, b], tu[a, b], ts[a, b] = best[2], best[3], best[4]
    return dict(topk_of(ti, tu, ts, topk), tab_inter=ti, tab_union=tu, tab_shift=ts)


def jaccard(inter, union):
    inter, union = np.asarray(inter, np.float64), np.asarray(union, np.float64)
    return np.where(union > 0, inter / np.where(union > 0, union, 1), 0.0)
