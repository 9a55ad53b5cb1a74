"""Measure the constants of the small-kernel matrix's error models on the CPU (no GPU) and write profiles/small_error_model.md.

    python tools/small_error_model.py            # measure over every case of tests/small_matrix.py, rewrite the file
    python tools/small_error_model.py --check    # exit 1 unless the constants in tests/small_matrix.py equal the file's

Per kernel family, m = the largest ratio of |fp32 emulator - float64 oracle| to the family's model at M = 1 over the whole table
(small_matrix.measured_ratio), rounded up to two decimals; the tests use M = 4 m.  Also the GroupNorm envelope: per data regime the largest
relative error of `scale` the emulated fp32-partials design makes, and the group |mean| / std at which that error passes 1e-4."""
from __future__ import annotations

import math
import os
import re
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import small_matrix as sm  # noqa: E402

OUT = os.path.join(REPO, "profiles", "small_error_model.md")
NAMES = {"gn": "GroupNorm", "ln": "LayerNorm", "stem": "stem", "head": "head", "time": "time embedding", "mv": "mat-vec"}
ENVELOPE_RATIOS = (1, 3, 10, 20, 30, 40, 50, 60, 80, 100, 150, 200, 300, 1000)


def up2(v):
    return math.ceil(v * 100 - 1e-9) / 100


def measure(verbose=True):
    best = {k: (0.0, "-") for k in sm.KINDS}
    for kind in sm.KINDS:
        for key, s in sm.cases(kind):
            r = sm.measured_ratio(key, s, sm.inputs(key, s))
            if verbose:
                print(f"{r:8.4f}  {key}")
            if r > best[kind][0]:
                best[kind] = (r, key)
    return best


def rel_scale_error(key, s, d):
    o, e = sm.gn_oracle(s, d), sm.gn_emulate(s, d)
    return float(((e.scale.double() - o.scale).abs() / o.scale.abs()).max())


def envelope():
    """(per regime: largest relative scale error over the table's GroupNorm cases, its case), (the |mean| / std sweep on 64+32 channels,
    600 pixels, three samples, eps 1e-5: relative scale error per ratio)"""
    per = {r: (0.0, "-") for r in sm.GN_REGIMES}
    for key, s in sm.cases("gn"):
        v = rel_scale_error(key, s, sm.inputs(key, s))
        if v > per[s.regime][0]:
            per[s.regime] = (v, key)
    sweep = []
    for r in ENVELOPE_RATIOS:
        key, s = sm._gn("data", 3, 600, 64, 32, regime="benign")
        d = sm.gn_inputs(f"envelope {r}", s)
        x = torch.cat([d["x0"], d["x1"]], -1)
        x = (x - 0.3) / 1.5 + float(r)          # unit variance, every group's mean r
        d["x0"], d["x1"] = x[..., :64].contiguous(), x[..., 64:].contiguous()
        sweep.append((r, rel_scale_error(key, s, d)))
    return per, sweep


def render(best, per, sweep):
    cross = next((r for r, v in sweep if v > 1e-4), None)
    lines = [
        "# Error models of the small-kernel matrix",
        "",
        f"Written by `python tools/small_error_model.py` (CPU only) over the {len(sm.cases())} cases of `tests/small_matrix.py`.",
        "`tests/small_matrix.py` holds the measured values (rounded up to two decimals) as `MEASURED`; every tolerance uses `M = 4 m`.",
        "`U = 2^-24`.  Every tolerance is computed per element from the case's own float64 magnitudes.",
        "",
        "## The models",
        "",
        "    dot(K, T, ref) = sqrt(K) U T + 2 U |ref|          T = |bias| + sum |w x| over the K products that feed the element",
        "",
        "* **stem** (`pf_conv_in`): `tol = M dot(9 cin + 1, T, ref)`.  Tile statistics are held to the float64 sums of the stored output",
        "  over the tile's in-image pixels within `(n_pix + 2) U sum |x|`: any order of n fp32 additions meets that, no constant.",
        "* **head** (`pf_conv_out`): `tol = M (dot(9 cin, T, ref) + D)`, `D = sum |w| da`, `da = U (|silu'(v)| |v| + |a| (4 + |v|))` with",
        "  `v = x sc + sh`, `a = silu(v)`: one rounding of `v` through `silu'`, `__expf`'s argument scaling (`|v| U` relative) and two ulps,",
        "  the hardware reciprocal and two products.",
        "* **mat-vec** (`pf_matvec`): `tol = M dot(K + 1, T, lin)`; the exp variant `|exp(lin)| (M dot + 2 * 2^-23)`: the linear tolerance,",
        "  relative, plus two ulps of `expf`.",
        "* **time embedding** (`pf_time_embed`): the oracle takes the fp32 frequencies as the reference's torch expression gives them.  A",
        "  sinusoid entry may move by `de = (U + 2^-23) |t f| + 2 U`: the one IEEE product `t * f`, one ulp of the fp32 frequency (the",
        "  kernel's `expf` and the reference's `exp` need not round alike; it moves the argument by `|t f| 2^-23`) and two ulps of a cosine or",
        "  sine.  These are bounds, not estimates, and stay outside M.  First layer: `u1 = M dot(channels + 1, T1, p1) + sum |w0| de`; SiLU:",
        "  `uh = |silu'(p1)| u1 + u1^2 / 4 + M U |h| (4 + |p1|)` (`|silu''| <= 1/2`; `expf`, the sum, the quotient); the second layer and the",
        "  closing SiLU the same with `uh` in place of `de`.  m is measured after the entry bounds are taken off the emulator's error.",
        "  Half of the time cases carry probe weights (one nonzero per row of W0, a diagonal W2), so that every sinusoid entry reaches",
        "  outputs of its own: only there do float64 frequencies (up to 4.6 ulps from the fp32 ones) leave the tolerance.",
        "* **LayerNorm** (`pf_ln_stats`, `pf_ln_planes`): `dmu = M U sqrt(depth) sum|x| / C`, depth = 2 + passes + 6 + 1 additions on an",
        "  element's path to the fp32 row sum.  The kernel's centred sum of squares is the data's plus `C dmu^2` exactly, rounded like the",
        "  mean: `dvar = dmu^2 + M U (sqrt(depth) + 3) (var + dmu^2)`; `drstd` = the interval of `(max(var -+ dvar, 0) + eps)^-1/2` plus",
        "  `4 U rstd`.  An output: `|gamma| rstd dmu + |x - mu| |gamma| drstd + 4 U (|t| + |y|)`; a plane pair (hi + lo) adds `2^-16 |y|`",
        "  with bf16 pieces, `2^-22 |y| + 2^-25` with fp16 pieces.  On a constant row `rstd = eps^-1/2 = 316`: the output carries `316 |gamma| dmu`.",
        "* **GroupNorm** (`pf_gn_scale_shift`, `pf_gn_finalize_tiles`): `dS = M U (1 + sqrt(m)) sum|x|`, `dQ = M U (1 + sqrt(m)) sum x^2` per",
        "  group, m = the fp32 additions one thread of `gn_partial_kernel` makes in sequence (0 for given tile statistics: one fp32 rounding",
        "  of an exact sum).  `dmean = dS / n`, `dvar = dQ / n + 2 |mean| dmean + dmean^2`, `drstd` = the interval of `(max(var -+ dvar, 0) +",
        "  eps)^-1/2` - to first order `rstd dvar / (2 (var + eps))`, and still right where `dvar > var + eps` (a constant group).  `tol_scale",
        "  = |gamma| drstd + 2 U |scale|`, `tol_shift = |gamma| (|mean| drstd + rstd_hi dmean) + 2 U (|beta| + |mean rstd gamma|)`.",
        "",
        "## Measured constants",
        "",
        "| family | m (recorded) | measured | M = 4 m | case that set the maximum |",
        "|---|---|---|---|---|",
    ]
    for k in sm.KINDS:
        v, key = best[k]
        lines.append(f"| {NAMES[k]} | {up2(v):.2f} | {v:.4f} | {4 * up2(v):.2f} | `{key}` |")
    lines += [
        "",
        "The norms are measured at the level the model speaks of: the group's fp32-partial sum and sum of squares against the float64",
        "sums, the row mean and the centred sum of squares; the other families at the output.  The margin of 4 covers what the emulator",
        "does not have: the hardware's `exp`, reciprocal and contraction choices, an ulp per operation.  No constant comes from a GPU run.",
        "",
        "## GroupNorm envelope (a recorded property of the fp32-partials design, not an assertion)",
        "",
        "Largest relative error of `scale` the emulated kernels make against the two-pass float64 GroupNorm, per data regime of the table:",
        "",
        "| regime | largest relative error of scale | case |",
        "|---|---|---|",
    ]
    for r in sm.GN_REGIMES:
        lines.append(f"| {r} | {per[r][0]:.3e} | `{per[r][1]}` |")
    lines += [
        "",
        "Unit-variance data with every group's mean at r (64+32 channels, 600 pixels, three samples, eps 1e-5):",
        "",
        "| group mean / std | " + " | ".join(str(r) for r, _ in sweep) + " |",
        "|---|" + "---|" * len(sweep),
        "| relative error of scale | " + " | ".join(f"{v:.1e}" for _, v in sweep) + " |",
        "",
        f"The error grows as (mean / std)^2 and passes 1e-4 at |mean| / std = {cross}." if cross else "The error stays below 1e-4 over the sweep.",
        "In the constant regime the variance is 0 and the error of `var` competes with eps alone: there `scale` can be off by a large factor",
        "(the float64 value is eps^-1/2 |gamma|); the tolerance interval above says by how much.  There the interval saturates (its far end",
        "tends to `rstd` itself), so an error near the tolerance (0.95 of it in `gn data B3 hw600 64+32 g32 eps1e-06 const`) is no sign of a",
        "thin margin: the emulator shows the same ratio.",
        "",
    ]
    return "\n".join(lines)


def main():
    best = measure(verbose="--check" not in sys.argv)
    if "--check" in sys.argv:
        text = open(OUT).read()
        ok = True
        for k in sm.KINDS:
            row = re.search(r"\| %s \| ([0-9.]+) \|" % re.escape(NAMES[k]), text)
            ok = ok and row is not None and float(row.group(1)) == sm.MEASURED[k] and up2(best[k][0]) == sm.MEASURED[k]
        sys.exit(0 if ok else 1)
    per, sweep = envelope()
    with open(OUT, "w") as f:
        f.write(render(best, per, sweep))
    for k in sm.KINDS:
        print(f"{NAMES[k]:16s} m = {up2(best[k][0]):.2f}  (small_matrix.MEASURED has {sm.MEASURED[k]:.2f})  {best[k][1]}")


if __name__ == "__main__":
    main()
