"""Measure the constant of the noise matrix's error model on the CPU (no GPU), find its tail cases and write profiles/noise_error_model.md.

    python -m tools.noise_error_model            # measure, search, rewrite the file
    python -m tools.noise_error_model --check    # exit 1 unless MEASURED and TAILS of tests/noise_matrix.py equal what is found and the file's

m = the largest ratio of |fp32 emulator - float64 oracle| to the model's unit U (|z| + r theta |partner|) over every case of
tests/noise_matrix.py and over the first 2^22 groups of (seed 1234, draw 7), rounded up to two decimals; the tests use M = 4 m.  The tail
search walks the groups of the same seed and draw in index order, 2^22 at a time, until every kind of tail has been met."""
from __future__ import annotations

import math
import os
import re
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import noise_matrix as nm  # noqa: E402

OUT = os.path.join(REPO, "profiles", "noise_error_model.md")
RUN_GROUPS, CHUNK, SEARCH_CAP = 1 << 22, 1 << 20, 1 << 28
SMALL_KEPT = 4          # groups with a radius word <= 8 that become cases: the first ones met


def up2(v):
    return math.ceil(v * 100 - 1e-9) / 100


def measure(verbose=True):
    """(largest ratio, where) over the case table and RUN_GROUPS consecutive groups"""
    best = (0.0, "-")
    for key, s in nm.cases():
        r = nm.unit_ratio(nm.emulate(s), nm.oracle(s))
        if verbose:
            print(f"{r:8.4f}  {key}")
        if r > best[0]:
            best = (r, key)
    for g0 in range(0, RUN_GROUPS, CHUNK):
        s = nm.Spec(seed=nm.SEED0, draws=nm.DRAW0, slot=0, off=4 * g0, n=4 * CHUNK)
        r = nm.unit_ratio(nm.emulate(s), nm.oracle(s))
        if r > best[0]:
            best = (r, f"groups [{g0}, {g0 + CHUNK}) of seed {nm.SEED0}, draw {nm.DRAW0}")
    return best


def tail_search():
    """name -> ((group, word, m), ...) in group order: the first SMALL_KEPT groups with a radius word <= 8, the first group of every other
    kind; and how many groups were walked"""
    found = {name: [] for name in nm.TAIL_WANT}
    need = {name: SMALL_KEPT if name == "small_m" else 1 for name in found}
    top = (1 << 24) - 1
    g0 = 0
    while any(len(found[k]) < need[k] for k in found) and g0 < SEARCH_CAP:
        m = nm.words(nm.SEED0, nm.DRAW0, np.uint64(g0) + np.arange(1 << 22, dtype=np.uint64)) >> np.uint64(8)
        radius, angle = m[:, (0, 2)], m[:, (1, 3)]
        hits = {"small_m": (radius <= 8).any(1), "u_one": (radius == top).any(1), "m_2^23": (m == 1 << 23).any(1),
                "m_2^23+1": (m == (1 << 23) + 1).any(1), "angle_2pi": (angle == top).any(1)}
        for name, mask in hits.items():
            for i in np.nonzero(mask)[0]:
                if len(found[name]) >= need[name]:
                    break
                row = [int(v) for v in m[i]]
                j = next(j for j in range(4) if nm.TAIL_WANT[name](j, row[j]))
                found[name].append((g0 + int(i), j, row[j]))
        g0 += 1 << 22
    return {k: tuple(v) for k, v in found.items()}, g0


def tail_rows(tails):
    rows = []
    for name, found in tails.items():
        for g, j, m in found:
            s = nm.Spec(seed=nm.SEED0, draws=nm.DRAW0, slot=0, off=4 * g, n=4)
            z = nm.oracle(s).z
            rows.append(f"| {name} | {g} | c{j} >> 8 = {m} | {nm.uniform_exact(m)!r} | " + ", ".join(f"{v:.9g}" for v in z) + " |")
    return rows


def render(best, tails, walked):
    v, where = best
    lines = [
        "# Error model of the noise matrix",
        "",
        f"Written by `python -m tools.noise_error_model` (CPU only) over the {len(nm.cases())} cases of `tests/noise_matrix.py` and the first",
        f"2^22 groups of (seed {nm.SEED0}, draw {nm.DRAW0}).  `tests/noise_matrix.py` holds the measured value (rounded up to two decimals) as",
        "`MEASURED` and the tail cases as `TAILS`; the tolerance uses `M = 4 m`.  `U = 2^-24`.  No number here comes from a GPU.",
        "",
        "## The generator, as specified",
        "",
        "Philox4x32-10 (Salmon et al., SC'11; the three Random123 known-answer vectors hold) with counter = (g lo, g hi, draw lo, draw hi),",
        "key = (seed lo, seed hi), g = global element index >> 2; element 4 g + j takes normal j of (r0 cos t0, r0 sin t0, r1 cos t1, r1 sin t1)",
        "with `r = sqrt(-2 ln u)`, `t = fp32(2 pi) u`, the pairs (u0, u1) and (u2, u3), `u_i` from output word `c_i`.",
        "",
        "## The uniform mapping",
        "",
        "`u = ((float)(c >> 8) + 0.5f) * 2^-24`, m = c >> 8.  Below 2^23 the sum is exact and `u = (2 m + 1) 2^-25`.  From 2^23 on `m + 0.5` is",
        "no fp32 number and rounds to even: to m for an even m, to m + 1 for an odd one.  In [0.5, 1] the uniforms therefore lie on the grid of",
        "2^-23, and `m = 2^24 - 1` gives `u = 1.0` exactly: the radius is 0 and both normals of the pair are exactly (+-)0, 2^-24 of all pairs.",
        "u is never 0; the smallest, 2^-25, gives the largest radius `sqrt(50 ln 2) = 5.887`: no draw is infinite or NaN.  The deviation from",
        "the open interval the form suggests is harmless and the stream is what goldens, recorded parity runs and users' seeds depend on: it is",
        "recorded and tested, not changed.",
        "",
        "## The model",
        "",
        "    l = logf(u0)  d1     t = -2 l  exact     r = sqrtf(t)  d2     a = 2pi_f32 * u1  d3     (s, c) = sincosf(a)  d4     z = r * c  d5",
        "",
        "    |dz| <= |z| (|d1| / 2 + |d2| + |d4| + |d5|) + r theta |sin theta| |d3|        (first order; sine outputs with cos and sin exchanged)",
        "    unit  = U (|z| + r theta |partner|)                                           partner = sin theta for a cosine output and the other way round",
        "    tol   = M unit + 1 U |z|                                                      the last term: the rounding of the stored value, a bound outside M",
        "",
        "A kernel with every operation correctly rounded stays below 3.5 units.  Where `u0 = 1.0` the oracle, the unit and the tolerance are 0:",
        "the stored value must be +-0.  The consumers (`pf_ddpm_step`, `pf_ddim_step`, `pf_qsample_rows`, `pf_gaussian_sample`,",
        "`pf_normal_rsample`) are launched so that the stored value is the draw itself (products with 1, sums with 0) and carry the same",
        "tolerance; a sum with +0 turns a drawn -0 into +0, nothing else changes a bit.  `pf_mse_rows` with `eps_theta = 0`: the row's float64",
        "sum of z^2 within `sum (2 |z| tol + tol^2) + (n + 2) 2^-53 sum z^2`.",
        "",
        "## Measured constant",
        "",
        "| m (recorded) | measured | M = 4 m | where the maximum was met |",
        "|---|---|---|---|",
        f"| {up2(v):.2f} | {v:.4f} | {4 * up2(v):.2f} | {where} |",
        "",
        "The emulator has correctly rounded `log`, `sqrt`, `sin` and `cos` (numpy's float64 functions rounded once to fp32) in the kernel's own",
        "operation order; the device's `logf` and `sincosf` may differ by an ulp or two per operation, which the margin of 4 covers.",
        "",
        "## Tail cases",
        "",
        f"Found by walking the groups of (seed {nm.SEED0}, draw {nm.DRAW0}) in index order ({walked} groups walked): the first {SMALL_KEPT} groups whose radius word",
        "`c0 >> 8` or `c2 >> 8` is at most 8 (the largest radii), the first with a radius word of 2^24 - 1 (`u = 1.0`: an exact zero pair), the",
        "first with a word of 2^23 and of 2^23 + 1 (the first rounded uniforms) and the first with an angle word `c1 >> 8` or `c3 >> 8` of",
        "2^24 - 1 (the angle `fp32(2 pi)`).  Each is one `pf_randn` case of four elements at offset 4 g.",
        "",
        "| kind | group | word | u | float64 normals of the group |",
        "|---|---|---|---|---|",
    ] + tail_rows(tails) + [""]
    return "\n".join(lines)


def tails_literal(tails):
    return "TAILS = {\n" + "".join(f"    {k!r}: {v!r},\n" for k, v in tails.items()) + "}"


def main():
    check = "--check" in sys.argv
    tails, walked = tail_search()
    if tails != nm.TAILS and not check:
        print("tests/noise_matrix.py: TAILS differs from what the search finds; the cases measured below are the recorded ones.  Found:")
    best = measure(verbose=not check)
    if check:
        text = open(OUT).read()
        row = re.search(r"^\| ([0-9.]+) \| [0-9.]+ \| [0-9.]+ \|", text, flags=re.M)
        ok = row is not None and float(row.group(1)) == nm.MEASURED == up2(best[0]) and tails == nm.TAILS
        ok = ok and all(f"| {name} | {g} |" in text for name, found in tails.items() for g, _, _ in found)
        sys.exit(0 if ok else 1)
    with open(OUT, "w") as f:
        f.write(render(best, tails, walked))
    print(tails_literal(tails))
    print(f"m = {up2(best[0]):.2f}  (measured {best[0]:.4f} at {best[1]}; noise_matrix.MEASURED has {nm.MEASURED:.2f})")


if __name__ == "__main__":
    main()
