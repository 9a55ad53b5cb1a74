"""The kernels around the convs against their float64 oracles at their edges (-m gpu; tests/small_matrix.py holds the cases, the oracles
and the tolerances): pf_gn_scale_shift and pf_gn_finalize_tiles against the two-pass GroupNorm of the DATA, pf_ln_stats and pf_ln_planes
(both builds; planes as hi + lo), the stem pf_conv_in with its tile statistics, the head pf_conv_out, pf_time_embed and pf_matvec.

One launch per case.  Everything a launch writes lives in a tests/gpu_guard.Guarded buffer: every owned element must be within the case's
tolerance of the oracle (profiles/small_error_model.md; no constant of it comes from a GPU), every other element must keep the sentinel, and a
second launch must leave the same bits.  A row of a 17-row mat-vec must equal, bit for bit, the same row launched alone.  Arguments the
library refuses must return PF_EINVAL and leave every buffer untouched.

Largest err / tol seen on an MI355X (173 launches in 3 s): GroupNorm 0.95 (a constant group, where the tolerance interval saturates and
the CPU emulator shows the same ratio; 0.48 elsewhere), LayerNorm 0.69, stem 0.25 (statistics 0.33), head 0.24, time embedding 0.70
(probe weights), mat-vec 0.24."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import small_matrix as sm  # noqa: E402
from gpu_guard import Guarded, _dev  # noqa: E402
from polyffusion_amd import _lib  # noqa: E402

CASES = [(k, s, v) for k, s in sm.cases() for v in (("", "f16") if s.kind == "ln" and s.entry == "planes" else ("",))]
_faulted = []   # the case whose launch raised: nothing more is started on the GPU after it


def _built(variant):
    if not os.path.exists(_lib.lib_path(variant)):
        from polyffusion_amd.build import build
        build(verbose=False, variant=variant)
    return _lib.load(variant)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def _f32(g):
    return g.body().view(torch.float32).cpu()


def _plan(lib, s, d):
    """(guarded outputs, launch(), read() -> what the ratio functions take)"""
    dev = {k: _dev(v) for k, v in d.items()}
    st = _lib.current_stream()
    p = lambda name: dev[name].data_ptr() if name in dev else 0  # noqa: E731
    if s.kind == "gn":
        C = s.c0 + s.c1
        g = {"scale": Guarded(s.b, C, C), "shift": Guarded(s.b, C, C)}
        if s.entry == "data":
            n = s.b * sm.gn_nsplit(s.hw) * C * 2
            g["scratch"] = Guarded(1, n, n)
            launch = lambda: lib.pf_gn_scale_shift(p("x0"), s.c0, p("x1"), s.c1, s.b, s.hw, s.groups, s.eps, p("gamma"), p("beta"),  # noqa: E731
                                                   g["scale"].ptr, g["shift"].ptr, g["scratch"].ptr, n * 4, st)
        else:
            launch = lambda: lib.pf_gn_finalize_tiles(p("stats0"), s.t0, s.c0, p("stats1"), s.t1, s.c1, s.b, s.hw, s.groups, s.eps,  # noqa: E731
                                                      p("gamma"), p("beta"), g["scale"].ptr, g["shift"].ptr, st)
        return g, launch, lambda: (_f32(g["scale"]), _f32(g["shift"]))
    if s.kind == "ln":
        if s.entry == "stats":
            g = {"mean": Guarded(1, s.rows, s.rows), "rstd": Guarded(1, s.rows, s.rows)}
            launch = lambda: lib.pf_ln_stats(p("x"), s.rows, s.c, sm.LN_EPS, g["mean"].ptr, g["rstd"].ptr, st)  # noqa: E731
            return g, launch, lambda: sm.Result(mean=_f32(g["mean"]).reshape(-1), rstd=_f32(g["rstd"]).reshape(-1))
        g = {"planes": Guarded(2 * s.rows, s.c, s.c, bits=16)}
        launch = lambda: lib.pf_ln_planes(p("x"), s.rows, s.c, sm.LN_EPS, p("gamma"), p("beta"), g["planes"].ptr, st)  # noqa: E731

        def read():
            pl = g["planes"].body().reshape(-1).view(sm.x3_dtype("f16" if lib.pf_x3_element() else "")).double().cpu().reshape(2, s.rows, s.c)
            return sm.Result(planes=pl[0] + pl[1])
        return g, launch, read
    if s.kind == "stem":
        g = {"out": Guarded(s.b * s.h * s.w, s.cout, s.cout)}
        nt = lib.pf_conv_in_stats_tiles(s.cin, s.cout, s.h, s.w)
        if s.stats:
            assert nt == sm.cdiv(s.h, 16) * sm.cdiv(s.w, 16)
            g["stats"] = Guarded(s.b * nt * s.cout, 2, 2)
        launch = lambda: lib.pf_conv_in(p("x"), p("w"), p("bias"), g["out"].ptr, s.b, s.cin, s.cout, s.h, s.w,  # noqa: E731
                                        g["stats"].ptr if s.stats else 0, st)
        return g, launch, lambda: (_f32(g["out"]).reshape(s.b, s.h, s.w, s.cout),
                                   _f32(g["stats"]).reshape(s.b, nt, s.cout, 2) if s.stats else None)
    if s.kind == "head":
        n = s.b * s.cout * s.h * s.w
        g = {"out": Guarded(1, n, n)}
        launch = lambda: lib.pf_conv_out(p("x"), p("sc"), p("sh"), p("wp"), p("bias"), g["out"].ptr, s.b, s.cin, s.cout, s.h, s.w, st)  # noqa: E731
        return g, launch, lambda: _f32(g["out"]).reshape(s.b, s.cout, s.h, s.w)
    if s.kind == "time":
        g = {"out": Guarded(s.batch, s.d_t, s.d_t)}
        launch = lambda: lib.pf_time_embed(0 if s.table else p("t"), p("w0"), p("b0"), p("w2"), p("b2"), g["out"].ptr, s.batch,  # noqa: E731
                                           s.channels, s.d_t, st)
        return g, launch, lambda: _f32(g["out"])
    ldy = s.n + s.ldy_pad
    g = {"y": Guarded(s.b, ldy, s.n)}
    launch = lambda: lib.pf_matvec(p("x"), sm.mv_ldx(s), p("w"), p("bias"), g["y"].ptr, ldy, s.b, s.n, s.k, s.npg, s.xgs, s.exp, st)  # noqa: E731

    def rows_alone():
        """rows of the batch launched alone: (row, its bits) - the kernel's accumulation is batch-position invariant"""
        out = []
        for r in sorted({0, 7, 8, s.b - 1}):
            y1 = Guarded(1, ldy, s.n)
            _lib.check(lib.pf_matvec(p("x") + r * sm.mv_ldx(s) * 4, sm.mv_ldx(s), p("w"), p("bias"), y1.ptr, ldy, 1, s.n, s.k, s.npg, s.xgs,
                                     s.exp, st), "pf_matvec", lib)
            torch.cuda.synchronize()
            assert y1.guards_intact()
            out.append((r, y1.body()[0, :s.n].cpu()))
        return out
    g["_rows_alone"] = rows_alone
    return g, launch, lambda: _f32(g["y"])[:, :s.n]


@pytest.mark.parametrize("key,s,variant", CASES, ids=[k + (" [f16]" if v else "") for k, _, v in CASES])
def test_case_against_the_oracle(key, s, variant):
    assert not _faulted, f"not run: the launch of {_faulted[0]} failed on the GPU"
    lib = _built(variant)
    d = sm.inputs(key, s)
    g, launch, read = _plan(lib, s, d)
    rows_alone = g.pop("_rows_alone", None)
    try:
        _lib.check(launch(), key, lib)
        torch.cuda.synchronize()
        first = {n: b.buf.clone() for n, b in g.items()}
        _lib.check(launch(), key, lib)
        torch.cuda.synchronize()
    except Exception:
        _faulted.append(key)
        raise
    for name, b in g.items():
        assert b.guards_intact(), f"{key}: a write outside the owned part of {name}"
        assert torch.equal(b.buf, first[name]), f"{key}: a second launch changed {name}"
    got = read()
    if s.kind == "gn":
        r = sm.gn_ratio(s, d, sm.gn_oracle(s, d), got[0], got[1])
    elif s.kind == "ln":
        r = sm.ln_ratio(s, d, sm.ln_oracle(s, d), got, variant)
    elif s.kind == "stem":
        out, stats = got
        r = sm.stem_ratio(s, sm.stem_oracle(s, d), out)
        if s.stats:
            rs = sm.stem_stats_ratio(s, out, stats)
            print(f"small_matrix {key}: statistics err/tol {rs:.3f}")
            assert rs <= 1.0, (key, "statistics", rs)
    elif s.kind == "head":
        assert bool(torch.isfinite(got).all()), key
        r = sm.head_ratio(s, sm.head_oracle(s, d), got)
    elif s.kind == "time":
        r = sm.time_ratio(s, d, sm.time_oracle(s, d), got)
    else:
        r = sm.mv_ratio(s, sm.mv_oracle(s, d), got)
    print(f"small_matrix {key}{' [f16]' if variant else ''}: err/tol {r:.3f}")
    assert r <= 1.0, (key, r)
    if rows_alone is not None and s.b == 17:
        whole = g["y"].body().cpu()
        for row, bits in rows_alone():
            assert torch.equal(whole[row, :s.n], bits), f"{key}: row {row} differs from the same row launched alone"


def test_refused_arguments_leave_every_buffer_untouched():
    assert not _faulted, f"not run: the launch of {_faulted[0]} failed on the GPU"
    lib = _built("")
    n = 1 << 20
    g = {name: Guarded(1, n, n) for name in ("out", "out2", "scratch")}
    dev = {"x": torch.zeros(n + 64, device="cuda"), "v": torch.ones(n + 64, device="cuda")}
    ptr = lambda name: g[name].ptr if name in g else dev[name].data_ptr()  # noqa: E731
    st = _lib.current_stream()
    for name, fn, args in sm.refused(ptr):
        rc = getattr(lib, fn)(*args[:-1], st)
        assert rc == -1, f"{name}: returned {rc}"
    torch.cuda.synchronize()
    for name, b in g.items():
        assert b.guards_intact(body_too=True), f"a refused call wrote to {name}"
