"""Rolls for the chord-recognition tests: seeded random rolls and the planted cases, shared by the host and the GPU file."""
import numpy as np

F = np.float32
# (segments, steps) x (notes per step) x (same-key overlaps allowed)
SHAPES = ((1, 16), (1, 48), (1, 128), (2, 16), (2, 128))
DENSITIES = (0.05, 0.5, 3.0)


def random_roll(seed, segments, steps, density, overlaps, songs=1):
    """``[songs * segments, 2, steps, 128]`` float32.  About ``density`` notes per step, lengths 1..12 steps (so that some run into the end of
    their segment), cell values off the exact 0 / 1 (an onset of 0.7 is a note for the plain rule and none for custom_round).  Without
    ``overlaps`` a note is only placed where its key is free from the step before its onset to the step after its end.  Every song carries a
    note that sounds in its last step."""
    rng = np.random.default_rng(seed)
    x = np.zeros((songs * segments, 2, steps, 128), F)
    x[:, :, :, :] = rng.uniform(-0.2, 0.45, x.shape).astype(F) * (rng.random(x.shape) < 0.3)
    for g in range(songs * segments):
        used = np.zeros((steps + 2, 128), bool)
        for _ in range(max(1, int(round(density * steps)))):
            k = int(rng.integers(0, 128)) if rng.random() < 0.1 else int(rng.integers(28, 92))
            t, d = int(rng.integers(steps)), int(rng.integers(1, 13))
            e = min(t + d, steps)
            if not overlaps and used[t:e + 2, k].any():
                continue
            used[t + 1:e + 1, k] = True
            x[g, 0, t, k] = rng.choice([1.0, 0.97, 1.03, 0.7]).astype(F)
            x[g, 1, t + 1:e, k] = rng.choice([1.0, 0.6, 1.4]).astype(F)
    for s in range(songs):
        x[(s + 1) * segments - 1, 0, steps - 1, 40 + s % 12] = 1.0
    return x


def random_chords(seed, songs, beats):
    """Condition rows [songs, beats, 36]: a root, a few chroma bits and a bass class per beat, some beats empty, values off 0 / 1"""
    rng = np.random.default_rng(seed)
    c = np.zeros((songs, beats, 36), F)
    for s in range(songs):
        for j in range(beats):
            if rng.random() < 0.15:
                continue
            root = int(rng.integers(12))
            c[s, j, root] = 1
            for d in ((0, 4, 7), (0, 3, 7), (0, 4, 7, 10))[int(rng.integers(3))]:
                c[s, j, 12 + (root + d) % 12] = rng.choice([1.0, 0.8]).astype(F)
            c[s, j, 24 + int(rng.integers(12))] = 1
            c[s, j, int(rng.integers(36))] += F(0.3)                      # below every threshold on its own
    return c


def empty(segments=1, steps=16):
    return np.zeros((segments, 2, steps, 128), F)


def put(x, g, t, k, d):
    """a note of d steps on key k from step t of segment g (sustain written past the segment end is dropped)"""
    x[g, 0, t, k] = 1
    x[g, 1, t + 1:t + d, k] = 1
    return x


def planted():
    """name -> (x, segments, expected label names or None)"""
    cases = {}
    # a note that would last 8 steps, clipped at the end of segment 0; segment 1 starts with sustain cells only (orphans: no note)
    x = empty(2, 16)
    put(x, 0, 12, 60, 8), put(x, 0, 12, 64, 8), put(x, 0, 12, 67, 8)
    x[1, 1, 0:4, [60, 64, 67]] = 1
    put(x, 1, 15, 48, 1)
    cases["clipped_at_segment_end"] = (x, 2, None)
    # a note from step 3 to step 5: a quarter beat in beat 0, a quarter beat in beat 1
    x = empty(1, 16)
    put(x, 0, 3, 62, 2), put(x, 0, 15, 62, 1)
    cases["quarter_beat_overlap"] = (x, 1, None)
    # only C and G sound: C:maj, C:min and C:sus4 tie (one template class missing each), the lowest index wins
    x = empty(1, 16)
    put(x, 0, 0, 48, 16), put(x, 0, 0, 55, 16)
    cases["c_g_tie"] = (x, 1, ["C:maj"] * 4)
    cases["empty"] = (empty(1, 16), 1, ["N"] * 4)
    # NaN and negative cells are silent
    x = empty(1, 16)
    put(x, 0, 0, 50, 4), put(x, 0, 15, 50, 1)
    x[0, 0, 4, 54], x[0, 1, 5, 54], x[0, 0, 8, 57], x[0, 1, 1, 50] = np.nan, np.nan, -3.0, np.nan
    cases["nan_and_negative"] = (x, 1, None)
    # the lowest and the highest key
    x = empty(1, 16)
    put(x, 0, 0, 0, 8), put(x, 0, 0, 127, 16), put(x, 0, 8, 64, 8)
    cases["keys_0_and_127"] = (x, 1, None)
    return cases
