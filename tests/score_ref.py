"""Roll statistics restated in numpy int64 (the rules of include/pfhip.h, pf_roll_stats, and the ratios of polyffusion_amd/score.py), for the
tests: imports nothing from the product.  Every comparison is made in float32 against a float32 constant, as the kernel makes it; everything
after the comparisons is an integer."""
import numpy as np

NAMES = ("N_ONSET", "N_SOUNDING", "N_ORPHAN", "CHORD_BEATS", "SOUND_ON_CHORD", "SOUND_IN_CHORD", "ONSET_IN_CHORD", "ONSET_ON_CHORD",
         "CHORD_CLASSES", "CHORD_HEARD", "BASS_BEATS", "BASS_HIT", "LOW_KEY", "HIGH_KEY")
IDX = {n: i for i, n in enumerate(NAMES)}
NCOUNT = 16
F = np.float32


def _round(v, custom):
    with np.errstate(invalid="ignore"):
        return ((v > F(0.95)) & (v < F(1.05))) if custom else (v > F(0.5))


def _occupied(v, custom):
    with np.errstate(invalid="ignore"):
        return _round(v, True) if custom else ((v > F(0.5)) | (v < F(-0.5)))


def argmax12(v):
    """arg-max over the last axis (12 wide), ties to the lowest index, a NaN never greater; and whether any entry is > 0"""
    with np.errstate(invalid="ignore"):
        best, idx = v[..., 0].copy(), np.zeros(v.shape[:-1], np.int64)
        for i in range(1, 12):
            up = v[..., i] > best
            best, idx = np.where(up, v[..., i], best), np.where(up, i, idx)
        return idx, (v > 0).any(-1)


def roll_stats(x, chord=None, mask=None, custom_round=False, bass_relative=False):
    """x [n, 2, S, 128], chord [n, S/4, 36] or None, mask like x or None -> (counters [n, 16], chroma [n, S/4, 12], onsets [n, S]), int64"""
    x = np.asarray(x, F)
    n, _, S, K = x.shape
    assert K == 128 and S > 0 and S % 4 == 0
    B = S // 4
    live = np.ones((n, S, K), bool) if mask is None else (np.asarray(mask, F)[:, 0] == 0)
    on, sus = _round(x[:, 0], custom_round) & live, _round(x[:, 1], custom_round) & live
    snd = on | sus
    occ = _occupied(x[:, 0], custom_round) | _occupied(x[:, 1], custom_round)          # raw values: the mask does not hide a predecessor
    prev = np.zeros_like(occ)
    prev[:, 1:] = occ[:, :-1]
    orphan = sus & ~prev
    onehot = (np.arange(K)[:, None] % 12 == np.arange(12)[None, :]).astype(np.int64)   # [128, 12]
    per_beat = lambda cells: cells.reshape(n, B, 4, K).sum(2).astype(np.int64) @ onehot    # [n, B, 12]
    chroma, on_chroma = per_beat(snd), per_beat(on)
    onsets = on.sum(-1).astype(np.int64)
    c = np.zeros((n, NCOUNT), np.int64)
    c[:, IDX["N_ONSET"]] = on.sum((1, 2))
    c[:, IDX["N_SOUNDING"]] = snd.sum((1, 2))
    c[:, IDX["N_ORPHAN"]] = orphan.sum((1, 2))
    beat_keys = snd.reshape(n, B, 4, K).any(2)                                          # [n, B, 128]
    sounds = beat_keys.any(-1)
    if chord is not None:
        chord = np.asarray(chord, F).reshape(n, B, 36)
        with np.errstate(invalid="ignore"):
            C = chord[..., 12:24] > F(0.5)
        nC = C.sum(-1)
        cb = nC > 0
        c[:, IDX["CHORD_BEATS"]] = cb.sum(-1)
        c[:, IDX["SOUND_ON_CHORD"]] = (chroma.sum(-1) * cb).sum(-1)
        c[:, IDX["SOUND_IN_CHORD"]] = (chroma * C).sum((1, 2))
        c[:, IDX["ONSET_IN_CHORD"]] = (on_chroma * C).sum((1, 2))
        c[:, IDX["ONSET_ON_CHORD"]] = (on_chroma.sum(-1) * cb).sum(-1)
        c[:, IDX["CHORD_CLASSES"]] = nC.sum(-1)
        c[:, IDX["CHORD_HEARD"]] = ((chroma > 0) & C).sum((1, 2))
        bass, has_bass = argmax12(chord[..., 24:36])
        if bass_relative:
            bass = (bass + argmax12(chord[..., 0:12])[0]) % 12
        lowest = beat_keys.argmax(-1)                                                   # first sounding key (0 where silent: excluded below)
        bb = cb & has_bass & sounds
        c[:, IDX["BASS_BEATS"]] = bb.sum(-1)
        c[:, IDX["BASS_HIT"]] = (bb & (lowest % 12 == bass)).sum(-1)
    keys = snd.any(1)                                                                   # [n, 128]
    any_key = keys.any(-1)
    c[:, IDX["LOW_KEY"]] = np.where(any_key, keys.argmax(-1), -1)
    c[:, IDX["HIGH_KEY"]] = np.where(any_key, K - 1 - keys[:, ::-1].argmax(-1), -1)
    return c, chroma, onsets


def ratio(a, b):
    """a / b in float64 on int64 arrays, 0.0 where b == 0"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return np.where(b != 0, a.astype(np.float64) / np.where(b != 0, b, 1).astype(np.float64), 0.0)


def scores(counters, steps):
    """The derived scores of counters [n, 16] (steps: per image).  chord_f1 = 2PR / (P + R) with P = chord_fit = a / b and R = chord_cover =
    c / d is evaluated as the one ratio of integers 2ac / (ad + cb)."""
    g = lambda name: np.asarray(counters, np.int64)[..., IDX[name]]
    a, b, c, d = g("SOUND_IN_CHORD"), g("SOUND_ON_CHORD"), g("CHORD_HEARD"), g("CHORD_CLASSES")
    return {
        "chord_fit": ratio(a, b),
        "chord_cover": ratio(c, d),
        "chord_f1": ratio(2 * a * c, a * d + c * b),
        "bass_fit": ratio(g("BASS_HIT"), g("BASS_BEATS")),
        "integrity": ratio(g("N_ORPHAN"), g("N_ORPHAN") + g("N_ONSET")),
        "onset_rate": ratio(g("N_ONSET"), np.full_like(g("N_ONSET"), steps)),
    }


def songs(counters, segments):
    """Counters [n, 16] of n / segments songs: sums, except the lowest / highest key (min / max over the segments that sound)."""
    c = np.asarray(counters, np.int64).reshape(-1, segments, NCOUNT)
    out = c.sum(1)
    lo, hi = c[..., IDX["LOW_KEY"]], c[..., IDX["HIGH_KEY"]]
    out[:, IDX["LOW_KEY"]] = np.where((lo >= 0).any(1), np.where(lo >= 0, lo, 128).min(1), -1)
    out[:, IDX["HIGH_KEY"]] = hi.max(1)
    return out


def texture_fit(a, b):
    """cosine of two onsets tables [n, S] per image, as dot / sqrt(|a|^2 |b|^2) on exact integers; 0.0 where either is silent"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    dot, nn = (a * b).sum(-1), (a * a).sum(-1) * (b * b).sum(-1)
    return np.where(nn != 0, dot.astype(np.float64) / np.sqrt(np.where(nn != 0, nn, 1).astype(np.float64)), 0.0)


def rank(values, keep, descending=True):
    """indices of the best `keep`, stable: ties to the lower index"""
    v = [float(s) for s in values]
    return sorted(range(len(v)), key=lambda i: ((-v[i]) if descending else v[i], i))[:keep]


def integrity(x, custom_round=False):
    c = roll_stats(x, custom_round=custom_round)[0].sum(0)
    return c[IDX["N_ORPHAN"]] / (c[IDX["N_ORPHAN"]] + c[IDX["N_ONSET"]])
