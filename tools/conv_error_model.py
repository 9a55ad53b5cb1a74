"""Measure the constants of the conv matrix's error budget on the CPU (no GPU) and write profiles/conv_error_model.md.

    python tools/conv_error_model.py            # measure over every case of tests/conv_matrix.py, rewrite the file
    python tools/conv_error_model.py --check    # exit 1 unless the constants in tests/conv_matrix.py equal the file's

m_acc:   largest (|torch float32 CPU composition - float64 oracle| - 4 * 2^-24 * R) / (sqrt(K) * 2^-24 * T): the reference's own arithmetic.
m_split: largest |float64 emulation of the documented split - oracle| / split_scale, per element type, the Winograd form apart; the
         emulation rounds operands to nearest into hi and lo pieces and adds a_hi*w_hi + a_hi*w_lo + a_lo*w_hi in float64.
Both are taken before a GeGLU (on the linear outputs), at the pixels the GPU test compares (tests/conv_matrix.py regions())."""
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

import conv_matrix as cm  # noqa: E402
from polyffusion_amd import _lib  # noqa: E402

OUT = os.path.join(REPO, "profiles", "conv_error_model.md")
NAMES = ("m_acc", "m_split bf16", "m_split f16", "m_split fold_bf16", "m_split fold_f16", "m_split wino_bf16", "m_split wino_f16")


def up2(v):
    return math.ceil(v * 100 - 1e-9) / 100


def measure(verbose=True):
    lib = _lib.load("")
    best = {n: (0.0, "-") for n in NAMES}
    floor_off = (0.0, "-")   # the fp16 ratio WITHOUT the subnormal floor terms, to show what they explain

    def note(name, v, key):
        if v > best[name][0]:
            best[name] = (v, key)

    for key, s in cm.cases(lib):
        d = cm.inputs(key, s)
        info = cm.describe(lib, s)
        regs = cm.regions(s, info)
        for variant in ("", "f16"):
            if variant and s.prec == 0:
                continue
            mode = cm.mode_of(s, variant)
            f32 = cm.torch_compose(s, d, torch.float32, variant, linear=True).double() if (not variant or s.a_planes) else None
            wino = {}
            for b, oy, ox in regs:
                o = cm.oracle(s, d, b, oy, ox, variant)
                if f32 is not None:
                    got = f32[b][torch.as_tensor(oy)][:, torch.as_tensor(ox)]
                    note("m_acc", float((((got - o.lin).abs() - 4 * cm.EPS * o.R).clamp_min(0) / cm.acc_scale(s, o).clamp_min(1e-300)).max()), key)
                if mode == "f32":
                    continue
                if s.wino:
                    if b not in wino:
                        wino[b] = cm.emulate_wino(s, d, b, variant)[1]
                    lin = wino[b][torch.as_tensor(oy)][:, torch.as_tensor(ox)]
                else:
                    lin = cm.emulate(s, d, b, oy, ox, variant)[1]
                name = "m_split " + cm.split_key(s, mode)
                err = (lin - o.lin).abs()
                note(name, float((err / cm.split_scale(mode, o).clamp_min(1e-300)).max()), key)
                if name == "m_split f16":
                    v = float((err / (cm.UNIT[mode] * o.T).clamp_min(1e-300)).max())
                    floor_off = max(floor_off, (v, key))
        if verbose:
            print(key, {n: round(v, 2) for n, (v, _) in best.items()}, flush=True)
    return best, floor_off


def constants_in_file():
    with open(OUT) as f:
        rows = re.findall(r"^\| (m_acc|m_split \w+) \| ([0-9.]+) \|", f.read(), re.M)
    return {n: float(v) for n, v in rows}


def constants_in_module():
    return {"m_acc": cm.M_ACC, **{"m_split " + k: v for k, v in cm.M_SPLIT.items()}}


def main(argv):
    if "--check" in argv:
        a, b = constants_in_file(), constants_in_module()
        print("equal" if a == b else f"profiles/conv_error_model.md {a} != tests/conv_matrix.py {b}")
        return 0 if a == b else 1
    best, floor_off = measure()
    n = len(cm.cases())
    with open(OUT, "w") as f:
        f.write("# Constants of the conv matrix's error budget\n\n"
                f"Written by `python tools/conv_error_model.py` (CPU only) over the {n} cases of `tests/conv_matrix.py`, both element types.\n"
                "`tests/conv_matrix.py` holds the constants (measured values rounded up to two decimals) as `M_ACC` and `M_SPLIT`.\n\n"
                "    tol(e) = M * [ m_acc * sqrt(K) * 2^-24 * T(e) + m_split(mode) * split_scale(mode, e) ] + 4 * 2^-24 * R(e)\n"
                "    split_scale = u * T,  u = 0 (f32) | 2^-18 (bf16x3) | 2^-22 (f16x3);  f16x3 adds 2^-25 * ||w||_2 + 2^-33 * ||a||_2\n\n"
                "| constant | value | measured | case that set the maximum |\n|---|---|---|---|\n")
        for name in NAMES:
            f.write(f"| {name} | {up2(best[name][0]):.2f} | {best[name][0]:.4f} | `{best[name][1]}` |\n")
        f.write("\n* `m_acc`: torch float32 on the CPU against the float64 oracle, relative to `sqrt(K) * 2^-24 * T` after the epilogue's own\n"
                "  `4 * 2^-24 * R` is taken off: the reference's arithmetic, not the kernels'.\n"
                "* `m_split`: the float64 emulation of the documented split (operands rounded to nearest into hi and lo pieces, weights as\n"
                "  `split_hi_lo` in `csrc/conv_plan.hip` splits them - times 2^8 and clamped in the fp16 build -, `a_hi*w_hi + a_hi*w_lo + a_lo*w_hi`\n"
                "  in float64; the folded upsampling conv on its folded weights; the Winograd form as `tools/micro/winograd_numerics.py` has it)\n"
                "  against the oracle, relative to `split_scale`.\n"
                f"* The fp16 floor: without the two floor terms the direct forms' f16 ratio to `2^-22 * T` reaches {floor_off[0]:.1f} (`{floor_off[1]}`): lo pieces\n"
                "  below 2^-14 fall into fp16's subnormal range and are quantised to 2^-24, an absolute error of 2^-25 per activation (times the\n"
                "  weights: `2^-25 * ||w||_2`) and of 2^-25 / 2^8 per weight (`2^-33 * ||a||_2`).  The emulation confirms the attribution: with the\n"
                "  terms in `split_scale` the ratio stays at the value in the table.\n"
                "* `M = 4`: neither reference has the MFMA's accumulation order (blocked, three products per k, K-split partial sums added by a\n"
                "  reduce kernel), and the prologue uses `__expf` and the hardware reciprocal, a few ulp each.  M is not tuned on the kernels.\n")
    print({k: v for k, v in best.items()}, floor_off)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
