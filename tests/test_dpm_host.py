"""DPM-Solver++(2M) without a GPU: the C entry point is declared, exported and bound, its structs are laid out as the header says, it
refuses bad arguments before any launch; the time-step grids and the coefficient table against the float64 restatement in
``tests/dpm_ref.py``; the CLI flags; and the float64 facts the sampler's design rests on, re-derived by ``dpm_ref`` alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import dpm_ref
from polyffusion_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000          # a non-null, 16-byte aligned address that a refused call never touches


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from polyffusion_amd.build import build
        build(verbose=False)
    return _lib.load()


class Schedule:
    """What the samplers read of a LatentDiffusion: the step count and the float32 alpha_bar."""

    def __init__(self):
        self.n_steps = 1000
        self.alpha_bar = torch.from_numpy(dpm_ref.alpha_bar().astype(np.float32))
        self.eps_model = None


@pytest.fixture(scope="module")
def ab():
    return Schedule().alpha_bar.double().numpy()


def sampler(lib, *a, **kw):
    from polyffusion_amd.sampler import DPMSolverSampler
    return DPMSolverSampler(Schedule(), *a, **kw)


def test_header_declares_and_both_builds_export_the_entry_point(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "pfhip.h")).read(), flags=re.S)
    assert "pf_dpm_step" in set(re.findall(r"\b(pf_[a-z0-9_]+)\s*\(", hdr))
    assert "pf_dpm_coef" in hdr and "pf_dpm_step_args" in hdr
    assert hasattr(lib, "pf_dpm_step") and "pf_dpm_step" in _lib.SIGNATURES
    if not os.path.exists(_lib.lib_path("f16")):
        from polyffusion_amd.build import build
        build(verbose=False, variant="f16")
    assert hasattr(_lib.load("f16"), "pf_dpm_step")


def test_structs_are_laid_out_as_the_header_says():
    hdr = open(os.path.join(REPO, "include", "pfhip.h")).read()
    body = re.search(r"typedef struct pf_dpm_coef \{(.*?)\} pf_dpm_coef;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in re.findall(r"float ([^;]+);", body) for n in decl.split(",")]
    assert names == [n for n, _ in _lib.DpmCoef._fields_] == list(dpm_ref.FIELDS)
    assert C.sizeof(_lib.DpmCoef) == 28 and all(t is C.c_float for _, t in _lib.DpmCoef._fields_)
    body = re.search(r"typedef struct pf_dpm_step_args \{(.*?)\} pf_dpm_step_args;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    order = [n.strip(" *") for decl in re.findall(r"(?:const )?(?:float|pf_dpm_coef|pf_step_state|size_t)\s*\*?\s*([^;]+);", body) for n in decl.split(",")]
    assert order == [n for n, _ in _lib.DpmStepArgs._fields_]
    f = _lib.DpmStepArgs
    assert [getattr(f, n).offset for n in order] == [8 * i for i in range(12)] and C.sizeof(f) == 96


def test_bad_arguments_are_refused_before_any_launch(lib):
    """No GPU needed: the call returns before it touches HIP or any of the (fake) pointers."""
    coef = _lib.DpmCoef(0.6, 0.8, 0.9, 0.2, 0.0, 0.8, 0.6)
    second = _lib.DpmCoef(0.6, 0.8, 0.9, 0.3, -0.1, 0.8, 0.6)

    def refused(pattern, **fields):
        a = _lib.DpmStepArgs()
        kw = dict(x=FAKE, eps=FAKE, x_out=FAKE, n=8, coef=C.addressof(coef))
        kw.update(fields)
        for k, v in kw.items():
            setattr(a, k, v)
        rc = lib.pf_dpm_step(C.byref(a), None)
        msg = lib.pf_last_error().decode()
        assert rc < 0 and re.search(pattern, msg), (fields, rc, msg)

    refused("dpm_step: bad arguments", x=None)
    refused("dpm_step: bad arguments", eps=None)
    refused("dpm_step: bad arguments", x_out=None)
    refused("dpm_step: bad arguments", n=0)
    refused("both by value", table=FAKE, state=FAKE)
    refused("both by value", state=FAKE)
    refused("null coefficients", coef=None)
    refused("null coefficients", coef=None, table=FAKE)                     # a table without the state that names its row
    refused("all three or none", orig=FAKE)
    refused("all three or none", orig=FAKE, mask=FAKE)
    refused("all three or none", orig_noise=FAKE, mask=FAKE)
    refused("all three or none", mask=FAKE)
    refused("needs x0_prev", coef=C.addressof(second))
    assert lib.pf_dpm_step(None, None) < 0


def test_grids(lib, ab):
    from polyffusion_amd.sampler import DDIMSampler
    assert sampler(lib, 10).time_steps.tolist() == [1, 6, 24, 77, 195, 376, 572, 742, 882, 999]
    assert len(sampler(lib, 50).time_steps) == 49
    for n in (10, 20, 40, 50):
        assert np.array_equal(sampler(lib, n).time_steps, dpm_ref.grid_logsnr(ab, n))
        for kind in ("uniform", "quad"):
            ts = sampler(lib, n, kind).time_steps
            assert np.array_equal(ts, DDIMSampler(Schedule(), n, kind).time_steps) and np.array_equal(ts, dpm_ref.grid(ab, n, kind))
    with pytest.raises(NotImplementedError):
        sampler(lib, 10, "cosine")
    for order in (0, 3):
        with pytest.raises(ValueError):
            sampler(lib, 10, order=order)


def test_a_repeated_time_step_makes_first_order_rows_not_nan(lib):
    s = sampler(lib, 50, "quad")
    ts = s.time_steps
    assert len(set(ts.tolist())) < len(ts)                                  # quad at 50 repeats time steps
    rows = s.coef_rows()
    assert np.isfinite(rows).all()
    h0 = np.array([i for i in range(1, len(ts)) if ts[i] == ts[i - 1]])      # steps of zero length ...
    assert len(h0) and (rows[h0, 4] == 0).all() and (rows[h0 - 1, 4] == 0).all()       # ... and the steps after them
    assert (rows[h0, 2] == 1).all() and (rows[h0, 3] == 0).all()            # a zero-length step leaves x where it is
    assert (rows[:, 4] != 0).sum() > 40                                      # everything else stays second order


@pytest.mark.parametrize("kind,n", [("logsnr", 10), ("logsnr", 20), ("uniform", 50), ("quad", 50)])
@pytest.mark.parametrize("order", [1, 2])
def test_coefficient_table_is_the_float64_value_rounded_once(lib, ab, kind, n, order):
    s = sampler(lib, n, kind, order)
    for t_start in (len(s.time_steps) - 1, 3, 0):
        want = dpm_ref.rows(ab, s.time_steps, t_start, order=order)
        got = s.coef_rows(t_start)
        assert got.dtype == np.float32 and got.shape == want.shape
        # rounding to the nearest float32 moves a value by at most 2^-24 of itself; the 1e-6 on top is room for a float64 evaluation in
        # another operation order, a few 1e-16 away, to fall on the other side of a rounding boundary
        assert (np.abs(got.astype(np.float64) - want) <= 2.0 ** -24 * (1 + 1e-6) * np.abs(want)).all()
        assert ((got[:, 4] == 0) == (want[:, 4] == 0)).all()
        c = s._coef(t_start, t_start)
        assert [getattr(c, f) for f in dpm_ref.FIELDS] == got[t_start].tolist()


def test_first_row_of_a_call_and_the_lower_order_final_row(lib):
    s = sampler(lib, 10)
    full = s.coef_rows()
    assert full[9, 4] == 0 and (full[1:9, 4] != 0).all() and full[0, 4] == 0          # 10 < 15 steps: the last step is first order
    assert sampler(lib, 10, lower_order_final=False).coef_rows()[0, 4] != 0
    part = s.coef_rows(5)                                                   # a loop that starts lower: its own first row
    assert part[5, 4] == 0 and full[5, 4] != 0 and np.array_equal(part[1:5], full[1:5])
    s20 = sampler(lib, 20)
    assert len(s20.time_steps) >= 15 and s20.coef_rows()[0, 4] != 0         # 15 steps or more: second order to the end
    assert s20.coef_rows(7)[0, 4] == 0                                      # ... but not in a call of 8 steps
    assert (sampler(lib, 20, order=1).coef_rows()[:, 4] == 0).all()


def test_parser():
    from polyffusion_amd import inference_sdf
    p = inference_sdf.make_parser()
    a = p.parse_args([])
    assert (a.dpm, a.dpm_steps, a.dpm_order, a.dpm_discretize, a.ddim) == (False, 20, 2, "logsnr", False)
    a = p.parse_args(["--dpm", "--dpm_steps", "12", "--dpm_order", "1", "--dpm_discretize", "quad"])
    assert (a.dpm, a.dpm_steps, a.dpm_order, a.dpm_discretize) == (True, 12, 1, "quad")
    for bad in (["--dpm_order", "3"], ["--dpm_discretize", "cosine"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    with pytest.raises(SystemExit, match="--dpm and --ddim"):
        inference_sdf.make_sampler(None, p.parse_args(["--dpm", "--ddim"]), 0)
    with pytest.raises(SystemExit, match="--dpm and --ddim"):
        inference_sdf.main(["--dpm", "--ddim", "--synthetic_weights", "--synthetic"])


def test_make_sampler_returns_the_grid_length(lib):
    from polyffusion_amd import inference_sdf
    from polyffusion_amd.sampler import DPMSolverSampler

    class Model:
        ldm = Schedule()

    a = inference_sdf.make_parser().parse_args(["--dpm", "--dpm_steps", "50"])
    s, t_idx = inference_sdf.make_sampler(Model(), a, 3)
    assert isinstance(s, DPMSolverSampler) and t_idx == len(s.time_steps) - 1 == 48 and s.seed == 3 and s.order == 2


# ---------------------------------------------------------------------------------------------- the float64 facts, by dpm_ref alone
@pytest.mark.parametrize("s", [0.5, 1.0, 4.0])
def test_float64_2m_at_10_logsnr_steps_beats_ddim_at_50_uniform_steps(ab, s):
    assert dpm_ref.err_2m(ab, 10, s) < dpm_ref.err_ddim(ab, 50, s)


@pytest.mark.parametrize("s", [0.5, 1.0, 4.0])
def test_float64_second_order_convergence_on_the_logsnr_grid(ab, s):
    assert dpm_ref.err_2m(ab, 20, s) / dpm_ref.err_2m(ab, 40, s) >= 3


def test_float64_loop_reaches_the_exact_solution_and_the_known_region_is_kept(ab):
    """dpm_ref's own consistency: more steps come closer to the closed form; order 1 is DDIM with eta = 0; a fully known image comes back."""
    ts = dpm_ref.grid_logsnr(ab, 400)
    x = np.array([1.0, -2.0])
    gain = lambda i, v: dpm_ref.gauss_gain(ab, ts[i], 1.0) * v
    # 400 requested steps (332 after the integer rounding of the grid) must land closer than 40 do
    assert dpm_ref.rel_err(dpm_ref.loop(dpm_ref.rows(ab, ts), x, gain), dpm_ref.gauss_exact(ab, ts[-1], 1.0, x)) < dpm_ref.err_2m(ab, 40, 1.0) / 4
    ts = dpm_ref.grid_uniform(1000, 50)
    gain = lambda i, v: dpm_ref.gauss_gain(ab, ts[i], 4.0) * v
    assert np.allclose(dpm_ref.loop(dpm_ref.rows(ab, ts, order=1), x, gain), dpm_ref.ddim_loop(ab, ts, x, gain), rtol=1e-12)
    orig, noise = np.array([0.3, -0.7]), np.array([1.1, 0.2])
    out = dpm_ref.loop(dpm_ref.rows(ab, ts), x, gain, known=(orig, noise, np.array([1.0, 0.0])))
    last = dpm_ref.rows(ab, ts)[0]
    assert out[0] == last[5] * orig[0] + last[6] * noise[0] and out[1] == dpm_ref.loop(dpm_ref.rows(ab, ts), x, gain)[1]
