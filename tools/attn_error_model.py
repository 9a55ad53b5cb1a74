"""Measure the constants of the attention matrix's error budget on the CPU (no GPU) and write profiles/attn_error_model.md.

    python tools/attn_error_model.py            # measure over every case of tests/attn_matrix.py, rewrite the file
    python tools/attn_error_model.py --check    # exit 1 unless the constants in tests/attn_matrix.py equal the file's

m_exp:   largest (|float32 exp of the oracle's shifted scores, row sum, division and P.V in float64 - oracle| - 4 * 2^-24 * |ref|) /
         (2^-24 * Ae): the exponential alone.
m_acc:   largest (|torch float32 CPU composition - float64 oracle| - 4 * 2^-24 * |ref| - m_exp * 2^-24 * Ae) / (2^-24 * (sqrt(dh) As +
         sqrt(Lk) Tpv)), with m_exp as recorded (rounded up): the two float32 products.
m_split: largest (|float64 emulation of the documented split arithmetic - oracle| - floor) / (u * (As + Tpv)), per element type, over the
         128-query, the 256-query and the key-split form."""
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

import attn_matrix as am  # noqa: E402

OUT = os.path.join(REPO, "profiles", "attn_error_model.md")
NAMES = ("m_exp", "m_acc", "m_split bf16", "m_split f16")
TINY = 1e-300


def up2(v):
    return math.ceil(v * 100 - 1e-9) / 100


def head_inputs(s, d, variant):
    """(float64 q, k, v as [B][L][H][dh], the plane pieces or None) of a case in a build"""
    if s.ep in (am.X3, am.SPLIT):
        _, pc = am.encode_planes(d, variant)
        return am.plane_inputs(pc), pc
    return {n: d[n].double() for n in "qkv"}, None


def measure(verbose=True):
    best = {n: (0.0, "-") for n in NAMES}
    floor_off = (0.0, "-")   # the fp16 ratio WITHOUT the floor, to show what it explains
    acc_rows = []

    def note(name, v, key):
        if v > best[name][0]:
            best[name] = (v, key)

    for key, s in am.cases():
        d = am.inputs(key, s)
        for variant in ("", "f16"):
            mode = am.mode_of(s, variant)
            if variant and mode == "f32":
                continue
            x, pc = head_inputs(s, d, variant)
            for b, h in am.heads(s):
                q, k, v = (x[n][b, :, h] for n in "qkv")
                o = am.oracle(q, k, v, am.scale_of(s))
                note("m_exp", float((((am.exp_reference(o, v) - o.ref).abs() - 4 * am.EPS * o.ref.abs()).clamp_min(0) / am.exp_scale(o).clamp_min(TINY)).max()), key)
                f32 = am.torch_compose(q, k, v, am.scale_of(s), torch.float32).double()
                acc_rows.append((key, (f32 - o.ref).abs() - 4 * am.EPS * o.ref.abs(), am.exp_scale(o), am.acc_scale(s, o)))
                if mode == "f32":
                    continue
                err = (am.emulate(pc, b, h, variant, am.form_of(s)) - o.ref).abs()
                fl = am.floor_of(mode, o)
                note("m_split " + mode, float(((err - fl).clamp_min(0) / am.split_scale(mode, o).clamp_min(TINY)).max()), key)
                if mode == "f16":
                    floor_off = max(floor_off, (float((err / am.split_scale(mode, o).clamp_min(TINY)).max()), key))
        if verbose:
            print(key, {n: round(v, 2) for n, (v, _) in best.items()}, flush=True)
    m_exp = up2(best["m_exp"][0])
    for key, err, es, asc in acc_rows:
        note("m_acc", float(((err - m_exp * es).clamp_min(0) / asc.clamp_min(TINY)).max()), key)
    return best, floor_off


def constants_in_file():
    with open(OUT) as f:
        rows = re.findall(r"^\| (m_acc|m_exp|m_split \w+) \| ([0-9.]+) \|", f.read(), re.M)
    return {n: float(v) for n, v in rows}


def constants_in_module():
    return {"m_acc": am.M_ACC, "m_exp": am.M_EXP, **{"m_split " + k: v for k, v in am.M_SPLIT.items()}}


def main(argv):
    if "--check" in argv:
        a, b = constants_in_file(), constants_in_module()
        print("equal" if a == b else f"profiles/attn_error_model.md {a} != tests/attn_matrix.py {b}")
        return 0 if a == b else 1
    best, floor_off = measure()
    n = len(am.cases())
    with open(OUT, "w") as f:
        f.write("# Constants of the attention matrix's error budget\n\n"
                f"Written by `python tools/attn_error_model.py` (CPU only) over the {n} cases of `tests/attn_matrix.py`, both element types.\n"
                "`tests/attn_matrix.py` holds the constants (measured values rounded up to two decimals) as `M_ACC`, `M_EXP` and `M_SPLIT`.\n\n"
                "    tol(e) = M * [ (m_acc sqrt(dh) 2^-24 + m_split(mode) u) As(e) + m_exp 2^-24 Ae(e)\n"
                "                   + (m_acc sqrt(Lk) 2^-24 + m_split(mode) u) Tpv(e) + floor(mode, e) ] + 4 * 2^-24 * |ref(e)|\n"
                "    As = sum_j p_j |v_je - o_e| Ts(i,j),  Ae = sum_j p_j |v_je - o_e| (1 + |s_ij - max_i|),  Tpv = sqrt(sum_j (p_j v_je)^2)\n"
                "    u = 0 (f32) | 2^-18 (bf16x3) | 2^-22 (f16x3);  floor = 2^-25 sum_j |v_je - o_e| / l_i in the f16x3 build, else 0\n"
                "    a plane output (hi + lo) adds 2^-16 (|ref| + tol) with bf16 pieces, 2^-22 (|ref| + tol) + 2^-25 with fp16 pieces\n\n"
                "| constant | value | measured | case that set the maximum |\n|---|---|---|---|\n")
        for name in NAMES:
            f.write(f"| {name} | {up2(best[name][0]):.2f} | {best[name][0]:.4f} | `{best[name][1]}` |\n")
        f.write("\n* `m_exp`: float32 `exp` of the oracle's own shifted scores (rounded to float32), row sum, division and `P.V` in float64, against the\n"
                "  oracle, relative to `2^-24 * Ae` after `4 * 2^-24 * |ref|` is taken off: the exponential's argument and value roundings alone.\n"
                "* `m_acc`: torch float32 on the CPU against the oracle, after `4 * 2^-24 * |ref|` and the recorded `m_exp` term are taken off,\n"
                "  relative to `2^-24 * (sqrt(dh) As + sqrt(Lk) Tpv)`: the two float32 products and the float32 row sum of the reference (a row\n"
                "  sum off by `dl` moves the output by `o dl / l`, a sum over the keys like `P.V`), not the kernels'.\n"
                "* `m_split`: the float64 emulation of `attention_bf3.hip`'s documented arithmetic (`S = k_hi.q_hi + k_hi.q_lo + k_lo.q_hi`;\n"
                "  probabilities relative to the form's running reference - per-tile maximum, lazy `TAU`, per slice and merged -, rounded to\n"
                "  nearest into hi and lo pieces of the element type; `O = v_hi.p_hi + v_hi.p_lo + v_lo.p_hi`) against the oracle on the planes'\n"
                "  own `hi + lo` values, relative to `u * (As + Tpv)` after the floor is taken off.\n"
                f"* The fp16 floor: without it the f16 ratio to `2^-22 * (As + Tpv)` reaches {floor_off[0]:.1f} (`{floor_off[1]}`): probability pieces\n"
                "  below 2^-14 fall into fp16's subnormal range and are quantised to 2^-24, an absolute error of 2^-25 per key relative to the\n"
                "  kernel's reference exponent, which never lies above the row maximum.\n"
                "* The plane-store term is not measured but derived, as in the conv matrix: the stored value v (within tol of ref, so |v| <=\n"
                "  |ref| + tol) is written as hi = rn(v), lo = rn(v - hi), two roundings to nearest of p significand bits each, which leaves\n"
                "  `|v - (hi + lo)| <= 2^-2p |v|`: 2^-16 |v| with bf16 pieces (p = 8), 2^-22 |v| with fp16 pieces (p = 11), plus 2^-25 there for a\n"
                "  lo piece that falls into fp16's subnormal range (quantum 2^-24).  It applies to `o_planes` outputs only.\n"
                "* `M = 4`: neither reference has the MFMA's accumulation order (blocked, three products per k), the hardware `exp2` and\n"
                "  reciprocal, or the merge kernel's second summation order.  M is not tuned on the kernels.\n")
    print({k: v for k, v in best.items()}, floor_off)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
