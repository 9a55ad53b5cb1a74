"""What pf_conv2d runs for a fixed grid of arguments - form, tile, wave groups, K split wanted / granted, statistics tiles, K-split
scratch - from pf_conv_describe alone; needs no GPU (a plan touches no device; the CU count falls back to the MI355X's 256).

    python tools/conv_plan_table.py            # print the table
    python tools/conv_plan_table.py --check    # compare with tests/golden/conv_plans.json (exit 1 and the differing rows on a mismatch), both builds
    python tools/conv_plan_table.py --write    # regenerate that file: only for a change that alters a conv plan ON PURPOSE
    python tools/conv_plan_table.py --write --probe DIR   # ... from a library WITHOUT pf_conv_describe, see below

The grid keeps the cases conv_validate accepts; a row is `key: [form, tile_h, tile_w, tile_n, wave_groups, ksplit_wanted, ksplit,
stats_tiles, splitk_ws_bytes]`, and a case that wants K-split scratch has a second row, `key +ws`, with the scratch granted.

The recorded file was NOT written by the code it checks.  It comes from the commit before pf_conv_describe existed: statistics tiles and
scratch bytes from that library's pf_conv_stats_tiles / pf_conv_splitk_ws_bytes (K split wanted = scratch bytes / bytes of one output),
form, tile, wave groups and the granted split from a copy of it whose launchers report their template arguments and return before any HIP
call (profiles/r08_conv_plan_probe.patch; `--probe DIR` reads DIR/libpfhip.so and DIR/libpfhip_f16.so built from that copy).
tests/test_conv_plan.py holds the plan code to this file."""
from __future__ import annotations

import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from polyffusion_amd import _lib  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden", "conv_plans.json")
COLUMNS = ("form", "tile_h", "tile_w", "tile_n", "wave_groups", "ksplit_wanted", "ksplit", "stats_tiles", "splitk_ws_bytes")
BATCHES = (1, 2, 8, 16, 32)
SQUARES = ((16, 16), (32, 32), (64, 64), (128, 128))
ODD = ((8, 8), (8, 16), (4, 4), (20, 20), (24, 40))   # hout % 16 != 0; (4, 4) and (20, 20): hw % 64 != 0 as well
# (c0, c1, n): c0 + c1 over 32 ... 1024 with and without a second source, n over 32 ... 512 with one that is no multiple of 64
WIDE = ((32, 0, 32), (64, 0, 64), (64, 64, 64), (128, 0, 64), (128, 0, 96), (128, 64, 128), (256, 0, 128), (256, 0, 256), (256, 128, 256),
        (384, 0, 384), (512, 0, 512), (512, 512, 512))
FEW = ((64, 0, 64), (128, 0, 128), (256, 128, 256), (512, 0, 512), (512, 512, 96))
P = 16   # placeholder for a pointer nothing dereferences


def _args(prec, b, h, w, c0, c1, n, ks, **kw) -> _lib.ConvArgs:
    a = _lib.ConvArgs()
    a.x0, a.c0, a.x1, a.c1 = P, c0, (P if c1 else None), c1
    a.batch, a.hin, a.win, a.ks, a.stride, a.w, a.n, a.out, a.ld_out, a.precision = b, h, w, ks, 1, P, n, P, n, prec
    for k, v in kw.items():
        setattr(a, k, v)
    if a.prologue:
        a.sc, a.sh = P, P
    if a.prologue == 3:
        a.mean, a.rstd = P, P
    return a


def cases():
    """(key, ConvArgs) over the grid, in a fixed order"""
    def emit(tag, prec, b, h, w, c0, c1, n, ks, **kw):
        return f"{'fs'[prec]}{ks} B{b} {h}x{w} {c0}+{c1}>{n}{' ' + tag if tag else ''}", _args(prec, b, h, w, c0, c1, n, ks, **kw)
    for b in BATCHES:
        for h, w in SQUARES + ODD:
            for c0, c1, n in WIDE:   # the ResBlock conv, both precisions; Winograd asked for where the shape can have it
                for prec in (0, 1):
                    yield emit("", prec, b, h, w, c0, c1, n, 3, prologue=1)
                if h % 16 == 0 or (h, w) == (8, 16):
                    yield emit("wino", 1, b, h, w, c0, c1, n, 3, prologue=1, wino=1, w_wino=P)
            for c0, c1, n in FEW:
                if c1:   # the fused skip projection of a channel-changing block
                    yield emit(f"skip{c0}+{c1}", 1, b, h, w, n, 0, n, 3, prologue=1, skip_w=P, skip_x0=P, skip_c0=c0, skip_x1=P, skip_c1=c1)
                yield emit(f"skip{c0 // 2}", 1, b, h, w, n, 0, n, 3, prologue=1, skip_w=P, skip_x0=P, skip_c0=c0 // 2)
                if (h, w) in ((16, 16), (32, 32), (64, 64), (8, 8), (4, 4), (24, 40)):
                    for prec in (0, 1) if b in (1, 16) else (1,):   # (fp32 at the two ends only: its tile rule has no other input)
                        yield emit("ups", prec, b, h, w, c0, c1, n, 3, ups=1)
                        yield emit("s2", prec, b, h, w, c0, c1, n, 3, stride=2)
                        yield emit("s2br", prec, b, h, w, c0, c1, n, 3, stride=2, pad_mode=_lib.PAD_BOTTOM_RIGHT)
                    yield emit("fold", 1, b, h, w, c0, c1, n, 3, ups=1, ups_fold=1)
                if b in (1, 8, 16) and h == w and h >= 16:   # plan options and measurement aids
                    yield emit("no_t16", 1, b, h, w, c0, c1, n, 3, prologue=1, no_t16=1)
                    yield emit("no_pp", 1, b, h, w, c0, c1, n, 3, prologue=1, no_pp=1)
                    for t in (1, 2, 3):
                        yield emit(f"ft{t}", 1, b, h, w, c0, c1, n, 3, prologue=1, force_tile=t)
                    for k in (2, 4):
                        yield emit(f"fk{k}", 1, b, h, w, c0, c1, n, 3, prologue=1, force_ksplit=k)
        for L in (256, 1024):   # the linears of the transformer block: rows of a matrix
            for c0, c1, n in WIDE + ((1024, 0, 256),):
                for prec in (0, 1) if b in (1, 16) else (1,):
                    for pro in (0, 2, 3):
                        yield emit(f"p{pro}", prec, b, 1, L, c0, c1, n, 1, prologue=pro)
                    yield emit("geglu", prec, b, 1, L, c0, c1, n, 1, prologue=3, geglu=1)
                yield emit("planes", 1, b, 1, L, c0, c1, n, 1, a_planes=1)
                yield emit("planes ft2", 1, b, 1, L, c0, c1, n, 1, a_planes=1, force_tile=2)
                yield emit("planes geglu", 1, b, 1, L, c0, c1, n, 1, a_planes=1, geglu=1, out_planes=P)
                yield emit("qkv", 1, b, 1, L, c0, c1, 3 * n, 1, prologue=3, qkv_planes=P)


class _Probe:
    """The same answers from a library without pf_conv_describe (see the module text)."""

    def __init__(self, path):
        self.lib = C.CDLL(path)
        self.lib.pf_conv_splitk_ws_bytes.restype = C.c_size_t
        self.rec = (C.c_int * 13).in_dll(self.lib, "pf_dbg_launch")

    def describe(self, a):
        rc = self.lib.pf_conv2d(C.byref(a), None)
        if rc != 77:
            assert rc == -1, rc
            return None
        fam, ks, _, _, th, tw, bn, _, _, _, kg, _, ksplit = self.rec
        form = {0: 0, 2: 5, 3: 6}.get(fam, 4 if ks == 2 else 1 if kg == 1 else 2 if bn == 64 else 3)
        grant = (a.splitk_ws, a.splitk_ws_bytes)
        a.splitk_ws, a.splitk_ws_bytes = None, 0
        ws = int(self.lib.pf_conv_splitk_ws_bytes(C.byref(a)))
        a.splitk_ws, a.splitk_ws_bytes = grant
        one = a.batch * a.hin * a.win * (4 if a.ups else 1) * a.n * 4   # bytes of one output (stride 2 never splits)
        return [form, th, tw, bn, kg, ws // one if ws else 1, ksplit, int(self.lib.pf_conv_stats_tiles(C.byref(a))), ws]


class _Describe:
    def __init__(self, variant):
        self.lib = _lib.load(variant)

    def describe(self, a):
        info = _lib.ConvPlanInfo()
        if self.lib.pf_conv_describe(C.byref(a), C.byref(info)) != 0:
            return None
        return [int(getattr(info, c)) for c in COLUMNS]


def table(src) -> dict:
    rows = {}
    for key, a in cases():
        r = src.describe(a)
        if r is None:
            continue
        assert key not in rows, key
        rows[key] = r
        if r[8]:   # the same launch with the scratch it asked for
            a.splitk_ws, a.splitk_ws_bytes = P, r[8]
            rows[key + " +ws"] = src.describe(a)
    return rows


def differences(want: dict, got: dict) -> list:
    return [f"{k}: recorded {want.get(k)}, computed {got.get(k)}" for k in sorted(set(want) | set(got)) if want.get(k) != got.get(k)]


def main(argv) -> int:
    if "--probe" in argv:
        d = argv[argv.index("--probe") + 1]
        docs = {v: table(_Probe(os.path.join(d, os.path.basename(_lib.lib_path(v))))) for v in ("", "f16")}
    else:
        docs = {v: table(_Describe(v)) for v in ("", "f16") if os.path.exists(_lib.lib_path(v))}
    doc = next(iter(docs.values()))
    assert all(d == doc for d in docs.values()), "the two builds plan differently"   # the plan does not depend on the element type
    if "--write" in argv:
        with open(GOLDEN, "w") as f:
            f.write("{\n" + ",\n".join(f"{json.dumps(k)}:{json.dumps(v, separators=(',', ':'))}" for k, v in doc.items()) + "\n}\n")
        return 0
    if "--check" in argv:
        with open(GOLDEN) as f:
            diff = differences(json.load(f), doc)
        print("\n".join(diff[:40]) if diff else f"conv plans: {len(doc)} rows equal to {os.path.relpath(GOLDEN, REPO)} ({', '.join(v or 'default' for v in docs)})")
        return 1 if diff else 0
    for k, v in doc.items():
        print(k, v)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
