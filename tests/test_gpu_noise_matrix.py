"""The Gaussian generator against an independent Philox4x32-10 and a float64 Box-Muller, at every site it is drawn (-m gpu;
tests/noise_matrix.py holds the cases, the integer reference, the oracle and the tolerance): pf_randn and pf_randn_dev, the rng forms of
pf_ddpm_step (no known region, the q and the p draw of a known region, draw indices from the device state) and pf_ddim_step,
pf_qsample_rows (x_t and noise_out), pf_mse_rows, pf_gaussian_sample and pf_normal_rsample.

One launch per case.  Everything a launch writes lives in a tests/gpu_guard.Guarded buffer: every element must be finite and within its
tolerance of the oracle (profiles/noise_error_model.md; no constant of it comes from a GPU; exactly +-0 where the oracle is 0), every
element the launch does not own must keep the sentinel, and a second launch must leave the same bits.  The consumers are launched with
operands that make the stored value the draw itself, and must then equal pf_randn of the same (seed, draw, offset) bit for bit - but for
the sign of a zero: a sum with +0 stores a drawn -0 as +0 (pf_qsample_rows' noise_out stores the draw unchanged).

Largest err / tol seen on an MI355X (112 cases in 3 s): pf_randn 0.28 (the 2098181-element launch; at most 0.10 on the tails), pf_randn_dev 0.11,
pf_ddpm_step 0.27 (0.11 with the device state), pf_ddim_step 0.27, pf_qsample_rows 0.19 (x_t and noise_out alike), pf_mse_rows 0.03 of
the row sum's tolerance, pf_gaussian_sample and pf_normal_rsample 0.28: about 3 units of the model where a correctly rounded fp32
evaluation reaches 2.71.  Every consumer equalled pf_randn bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import noise_matrix as nm  # noqa: E402
from gpu_guard import Guarded  # noqa: E402
from polyffusion_amd import _lib  # noqa: E402

CASES = nm.cases()
_faulted = []   # the case whose launch raised: nothing more is started on the GPU after it
_shared = {}    # read-only device operands, made once: zeros, ones, the coefficient tables


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()
    yield
    _shared.clear()


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from polyffusion_amd.build import build
        build(verbose=False)
    return _lib.load()


def _const(value, n):
    """n floats of `value` on the device (16-byte aligned), grown on demand and shared by the cases: the launches only read them"""
    t = _shared.get(("const", value))
    if t is None or t.numel() < n:
        t = _shared[("const", value)] = torch.full((max(n, 4096),), float(value), device="cuda")
    return t.data_ptr()


def _coef_table(cls, good):
    """three coefficient rows on the device: row 1 is `good`, rows 0 and 2 would double every draw"""
    key = ("table", cls.__name__)
    if key not in _shared:
        rows = (cls * 3)()
        for i in range(3):
            for name, _ in cls._fields_:
                setattr(rows[i], name, getattr(good, name) * (1.0 if i == 1 else 2.0))
        host = torch.frombuffer(bytearray(bytes(rows)), dtype=torch.float32)
        _shared[key] = host.cuda()
    return _shared[key].data_ptr()


def _state(lib, s, st):
    """a device pf_step_state {index 1, draws} set through pf_step_state_set"""
    t = torch.zeros(2, dtype=torch.int64, device="cuda")
    _lib.check(lib.pf_step_state_set(t.data_ptr(), 1, s.draws, st), "pf_step_state_set", lib)
    return t


def _f32(g):
    return g.body().reshape(-1).view(torch.float32).cpu().numpy()


def _plan(lib, s):
    """(guarded outputs, keep-alive list, launch(), names of the outputs that hold the draws)"""
    st = _lib.current_stream()
    n, draw, other = s.n, nm.draw_of(s), (nm.draw_of(s) + 77) & nm.M64
    keep = []
    if s.kind in ("randn", "randn_dev"):
        g = {"out": Guarded(1, n, n)}
        if s.kind == "randn":
            return g, keep, lambda: lib.pf_randn(g["out"].ptr, n, s.seed, draw, s.off, st), ("out",)
        keep.append(_state(lib, s, st))
        return g, keep, lambda: lib.pf_randn_dev(g["out"].ptr, n, s.seed, keep[0].data_ptr(), s.slot, s.off, st), ("out",)
    if s.kind in ("ddpm", "ddim"):
        g = {"out": Guarded(1, n, n)}
        zero = _const(0.0, n)
        if s.kind == "ddpm":
            a, good = _lib.DdpmStepArgs(), _lib.DdpmCoef(sigma=1.0, sqrt_1mab=1.0)
            known = s.variant != "plain"
            if known:
                a.orig, a.mask = zero, _const(1.0 if s.variant in ("q", "state_q") else 0.0, n)
            a.draw_q, a.draw_p = (draw, other) if s.variant == "q" else (other, draw)
            fn = lib.pf_ddpm_step
        else:
            a, good = _lib.DdimStepArgs(), _lib.DdimCoef(sqrt_a=1.0, sigma=1.0)
            a.draw = draw
            fn = lib.pf_ddim_step
        a.x, a.eps, a.x_out, a.n, a.rng, a.seed, a.elem_offset = zero, zero, g["out"].ptr, n, 1, s.seed, s.off
        if s.get("state"):
            keep.append(_state(lib, s, st))
            a.table, a.state = _coef_table(type(good), good), keep[0].data_ptr()
            if s.kind == "ddpm":
                a.draw_q = a.draw_p = other         # ignored: the state supplies (draws, draws + 1)
            else:
                a.draw = other
        else:
            keep.append(good)
            a.coef = C.addressof(good)
        keep.append(a)
        return g, keep, lambda: fn(C.byref(a), st), ("out",)
    if s.kind == "qsample":
        g = {"x_t": Guarded(s.rows, s.row_elems, s.row_elems), "noise_out": Guarded(s.rows, s.row_elems, s.row_elems)}
        if "qtab" not in _shared:
            _shared["qtab"] = (torch.tensor([0.5, 0.0, 0.25], device="cuda"), torch.tensor([2.0, 1.0, 3.0], device="cuda"),
                               torch.ones(8, dtype=torch.int64, device="cuda"))
        ab, omab, t = _shared["qtab"]
        a = _lib.QsampleRowsArgs()
        a.x0, a.t, a.sqrt_ab, a.sqrt_1mab, a.n_steps, a.rng = _const(0.0, n), t.data_ptr(), ab.data_ptr(), omab.data_ptr(), 3, 1
        a.seed, a.draw, a.elem_offset, a.x_t, a.noise_out, a.rows, a.row_elems = s.seed, draw, s.off, g["x_t"].ptr, g["noise_out"].ptr, s.rows, s.row_elems
        keep.append(a)
        return g, keep, lambda: lib.pf_qsample_rows(C.byref(a), st), ("x_t", "noise_out")
    if s.kind == "mse":
        nb = lib.pf_mse_rows_workspace_bytes(s.rows, s.row_elems)
        assert nb % 8 == 0 and nb > 0
        g = {"row_sum": Guarded(1, 2 * s.rows, 2 * s.rows), "workspace": Guarded(1, nb // 4, nb // 4)}
        a = _lib.MseRowsArgs()
        a.eps_theta, a.rng, a.seed, a.draw, a.elem_offset = _const(0.0, n), 1, s.seed, draw, s.off
        a.row_sum, a.workspace, a.workspace_bytes, a.rows, a.row_elems = g["row_sum"].ptr, g["workspace"].ptr, nb, s.rows, s.row_elems
        keep.append(a)
        return g, keep, lambda: lib.pf_mse_rows(C.byref(a), st), ()
    g = {"out": Guarded(1, n, n)}
    if s.kind == "gauss":
        return g, keep, lambda: lib.pf_gaussian_sample(_const(0.0, n), _const(0.0, n), 0, s.seed, draw, s.off, 1.0, g["out"].ptr, n, st), ("out",)
    return g, keep, lambda: lib.pf_normal_rsample(_const(0.0, n), _const(1.0, n), 0, s.seed, draw, s.off, g["out"].ptr, n, st), ("out",)


@pytest.mark.parametrize("key,s", CASES, ids=[k for k, _ in CASES])
def test_case_against_the_oracle(lib, key, s):
    assert not _faulted, f"not run: the launch of {_faulted[0]} failed on the GPU"
    g, keep, launch, draws = _plan(lib, s)
    ref = None
    try:
        _lib.check(launch(), key, lib)
        torch.cuda.synchronize()
        first = {n: b.buf.clone() for n, b in g.items()}
        _lib.check(launch(), key, lib)
        if s.kind != "randn":          # what pf_randn itself writes for the same (seed, draw, offset)
            ref = torch.empty(s.n, device="cuda")
            _lib.check(lib.pf_randn(ref.data_ptr(), s.n, s.seed, nm.draw_of(s), s.off, _lib.current_stream()), key, lib)
        torch.cuda.synchronize()
    except Exception:
        _faulted.append(key)
        raise
    for name, b in g.items():
        assert b.guards_intact(), f"{key}: a write outside the owned part of {name}"
        assert torch.equal(b.buf, first[name]), f"{key}: a second launch changed {name}"
    o = nm.oracle(s)
    worst = 0.0
    for name in draws:
        got = _f32(g[name])
        assert got.shape == (s.n,) and np.isfinite(got).all(), f"{key}: {name} is not finite everywhere"
        r = nm.ratio(got, o)
        print(f"noise_matrix {key} [{name}]: err/tol {r:.3f}")
        assert r <= 1.0, (key, name, r)
        worst = max(worst, r)
        if ref is not None:
            stored_as_drawn = name == "noise_out" or s.kind == "randn_dev"
            want = ref if stored_as_drawn else ref + 0.0               # a sum with +0 stores -0 as +0; nothing else changes
            assert torch.equal(g[name].body().reshape(-1), want.view(torch.int32)), f"{key}: {name} differs from pf_randn's bits"
    if s.kind == "mse":
        got = g["row_sum"].body().reshape(-1).view(torch.float64).cpu().numpy()
        want, t = nm.mse_oracle(s, o)
        r = float((np.abs(got - want) / t).max())
        print(f"noise_matrix {key} [row_sum]: err/tol {r:.3f}")
        assert np.isfinite(got).all() and r <= 1.0, (key, r)
        z = ref.double().cpu().numpy().reshape(s.rows, s.row_elems)   # the same squares as pf_randn's draws give, in another order
        mine = (z * z).sum(1)
        assert (np.abs(got - mine) <= (s.row_elems + 2) * 2.0 ** -52 * mine).all(), key
