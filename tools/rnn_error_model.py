"""Measure the constants of the recurrent-kernel matrix's error models on the CPU (no GPU) and write profiles/rnn_error_model.md.

    python tools/rnn_error_model.py            # measure over every case of tests/rnn_matrix.py, rewrite the file
    python tools/rnn_error_model.py --check    # exit 1 unless the constants in tests/rnn_matrix.py equal the file's

Per family, m = the largest ratio of |fp32 emulator - float64 oracle| to the family's unit over the whole table
(rnn_matrix.measured_ratio), rounded up to two decimals; the tests use M = 4 m.  Also, per encoder case, the largest tolerance that
results and the emulator's own distance to the oracle."""
from __future__ import annotations

import math
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import rnn_matrix as rm  # noqa: E402

OUT = os.path.join(REPO, "profiles", "rnn_error_model.md")
NAMES = {"gates": "gate update", "step": "fused step", "enc_chord": "chord encoder", "enc_texture": "texture encoder",
         "enc_pnotree": "PianoTree encoder", "dec_chord": "chord decoder",
         "dec_pnotree": "PianoTree decoder"}
SUBS = [sub for k in rm.KINDS for sub in rm.SUBKINDS[k]]


def up2(v):
    return math.ceil(v * 100 - 1e-9) / 100


def measure(verbose=True):
    best = {k: (0.0, "-") for k in SUBS}
    for key, s in rm.cases():
        r = rm.measured_ratio(key, s)
        if verbose:
            print(f"{r:8.4f}  {key}")
        if r > best[rm.sub_of(s)][0]:
            best[rm.sub_of(s)] = (r, key)
    return best


def encoder_rows(best):
    """per encoder case: (key, emulator's largest |mu - oracle|, largest tolerance of mu at M = 4 up2(m))"""
    rows = []
    for key, s in rm.cases("enc"):
        d, o = rm.oracle(key, s)
        got, _ = rm._emulated(key)
        tol, _ = rm.enc_tol(s, o, rm.MARGIN * up2(best[rm.sub_of(s)][0]))
        rows.append((key, float((got.mu.double() - o.mu).abs().max()), float(tol.max())))
    return rows


def render(best, enc):
    lines = [
        "# Error models of the recurrent-kernel matrix",
        "",
        f"Written by `python tools/rnn_error_model.py` (CPU only) over the {len(rm.cases())} cases of `tests/rnn_matrix.py`.",
        "`tests/rnn_matrix.py` holds the measured values (rounded up to two decimals) as `MEASURED`; every tolerance uses `M = 4 m`.",
        "`U = 2^-24`.  Every tolerance is computed per element from the case's own float64 magnitudes.",
        "",
        "## The models",
        "",
        "    dot(depth, t2, ref) = U (sqrt(depth) (t2 + |ref|) + 2 |ref|)      t2 = sqrt(sum (w x)^2), depth = additions on an element's path",
        "",
        "* **cell** (every family): with `v_r = a_r + c_r`, `r = sigmoid(v_r)` (z alike), `arg = a_n + r c_n`, `n = tanh(arg)`, `h' = (1 - z) n + z h`",
        "  and input errors `d_*` of the pre-activation parts: `dr = r (1 - r) (d_r + U |v_r|) + 3 U r + 2^-126` (one sum; exp, sum and quotient of",
        "  the sigmoid; below fp32's normal range the kernel's sigmoid is 0), `darg = d_an + r d_cn + |c_n| dr + U (|r c_n| + |arg|)`,",
        "  `dn = (1 - n^2) darg + 2 U |n|`, `unit = |n - h| dz + (1 - z) dn + U (2 |(1 - z) n| + |z h| + |h'|)`.",
        "* **gate update** (`pf_gru_gates`): the cell with `d_* = 0` (gi and gh are given).  A row that takes no part (`step >= len`) has",
        "  tolerance 0: it keeps its bits.",
        "* **fused step** (`pf_gru_step`): `d` of the gh part `dot(4 ceil(H / 256) + 7, t2, gh)` (the vector `wave_dot`, its shuffle tree, `b_hh`), of",
        "  the gi part `dot(ceil(Kx / 64) + 8, t2, gi)` (the scalar `wave_dot`, `add1`, `add2`), through the cell.",
        "* **encoders** (`pf_encoder_forward`, `pf_encoder_forward_dist`): per element of `mu = W h + b`,",
        "  `unit = U (sqrt(sum over GRUs of steps (ceil(H / 8) + ceil(K / 8) + 6)) ||W row||_2 + sqrt(ceil(2H / 8) + 3) (||W row||_2 + |mu|) + 2 |mu|)`:",
        "  a GRU step leaves in `|h| <= 1` an error of the size of its pre-activations' rounding, the steps' errors add in quadrature, and a row",
        "  of W carries them to the output in quadrature.  `scale = exp(lin)`: the same unit of `lin`, relative, plus two ulps of `expf`.",
        "* **chord decoder** (`pf_decoder_forward`, greedy): decisions (root, chroma bits, bass) exactly the float64 decode's on rows whose every",
        "  decision is at least 1e-3 clear; a logit of step t as an encoder output, with `t + 1` steps of depth `4 ceil(H / 256) + 17` behind it, the",
        "  two linears in front, and `max(1, |z2dec_hid(z)|)` in the place of the bound 1 of the state.",
        "* **PianoTree decoder** (`pf_decoder_forward`, greedy, max_simu_note 4): the integer grid and the lengths it implies exactly the float64",
        "  decode's on rows that clear the same gap; a logit of time step t as the chord decoder's, with `(t + 1) (S + 2)` steps of depth 36 behind",
        "  it.  Its emulator keeps the kernels' walk, bind-time token tables and decision rules; a wave-wide dot has `wave_dot`'s shape - the 64",
        "  lanes' partial sums taken exactly and rounded once to fp32, then the fp32 shuffle tree - and a short per-thread dot is taken exactly",
        "  and rounded once.  The lanes' own fmaf chains are not followed there: the fused-step family follows them at H 512 and 1024.",
        "",
        "## Measured constants",
        "",
        "| family | m (recorded) | measured | M = 4 m | case that set the maximum |",
        "|---|---|---|---|---|",
    ]
    for k in SUBS:
        v, key = best[k]
        lines.append(f"| {NAMES[k]} | {up2(v):.2f} | {v:.4f} | {4 * up2(v):.2f} | `{key}` |")
    lines += [
        "",
        "The margin of 4 covers what the emulator does not have: the hardware's `expf`, `tanhf`, division and contraction choices, an ulp or",
        "two per operation.  No constant comes from a GPU run.",
        "",
        "## Encoder tolerances that result",
        "",
        "| case | emulator's largest distance of mu to float64 | largest tolerance of mu |",
        "|---|---|---|",
    ]
    for key, err, tol in enc:
        lines.append(f"| `{key}` | {err:.2e} | {tol:.2e} |")
    lines += ["", f"Largest tolerance of a benign encoder case: {max(t for _, _, t in enc):.2e} (the matrix requires at most 1e-5).", ""]
    dec = max(rm.dec_tol_max(s, rm.oracle(key, s)[1], rm.MARGIN * up2(best["dec_chord"][0])) for key, s in rm.cases("dec"))
    lines += [f"Largest tolerance of a chord-decoder logit: {dec:.2e} (the matrix requires less than 1e-4, a tenth of the decision gap).", ""]
    pn = max(rm.pn_tol_max(s, rm.oracle(key, s)[1], rm.MARGIN * up2(best["dec_pnotree"][0])) for key, s in rm.cases("pn"))
    lines += [f"Largest tolerance of a PianoTree-decoder logit: {pn:.2e} (the same requirement).", ""]
    return "\n".join(lines)


def main():
    best = measure(verbose="--check" not in sys.argv)
    if "--check" in sys.argv:
        text = open(OUT).read()
        ok = True
        for k in SUBS:
            row = re.search(r"\| %s \| ([0-9.]+) \|" % re.escape(NAMES[k]), text)
            ok = ok and row is not None and float(row.group(1)) == rm.MEASURED[k] and up2(best[k][0]) == rm.MEASURED[k]
        sys.exit(0 if ok else 1)
    with open(OUT, "w") as f:
        f.write(render(best, encoder_rows(best)))
    for k in SUBS:
        print(f"{NAMES[k]:18s} m = {up2(best[k][0]):.2f}  (rnn_matrix.MEASURED has {rm.MEASURED[k]:.2f})  {best[k][1]}")


if __name__ == "__main__":
    main()
