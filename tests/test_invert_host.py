"""Exact DDIM inversion without a GPU: the C entry points are declared, exported by both builds and bound, the structs are laid out as the
header says, bad arguments are refused before any launch; ``invert_coef_rows`` against the float64 restatement in ``tests/invert_ref.py``;
the float64 facts the design rests on (the iteration contracts by |c_e*g| per iterate on the closed-form Gaussian denoiser, and the round
trip closes geometrically), re-derived by ``invert_ref`` alone; ``invert``'s own refusals; and the CLI's."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import dpm_ref
import invert_ref
from polyffusion_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000          # a non-null, 16-byte aligned address that a refused call never touches
NAMES = ("pf_invert_step", "pf_invert_step_workspace_bytes", "pf_step_advance")


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


AB = dpm_ref.alpha_bar()


def ddim(lib, *a, **kw):
    from polyffusion_amd.sampler import DDIMSampler
    return DDIMSampler(Schedule(), *a, **kw)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_and_both_builds_export_the_entry_points(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "pfhip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pf_[a-z0-9_]+)\s*\(", hdr))
    if not os.path.exists(_lib.lib_path("f16")):
        from polyffusion_amd.build import build
        build(verbose=False, variant="f16")
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES
        assert hasattr(lib, name) and hasattr(_lib.load("f16"), name)
    assert "pf_invert_coef" in hdr and "pf_invert_step_args" in hdr


def test_structs_are_laid_out_as_the_header_says():
    hdr = open(os.path.join(REPO, "include", "pfhip.h")).read()
    body = re.search(r"typedef struct pf_invert_coef \{(.*?)\} pf_invert_coef;", hdr, flags=re.S).group(1)
    names = [n.strip() for decl in re.findall(r"float ([^;]+);", body) for n in decl.split(",")]
    assert names == [n for n, _ in _lib.InvertCoef._fields_] == list(invert_ref.FIELDS)
    assert C.sizeof(_lib.InvertCoef) == 8 and all(t is C.c_float for _, t in _lib.InvertCoef._fields_)
    body = re.search(r"typedef struct pf_invert_step_args \{(.*?)\} pf_invert_step_args;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    types = r"(?:float|double|void|pf_invert_coef|pf_step_state|size_t|int32_t|int64_t)"
    order = [n.strip(" *") for decl in re.findall(r"(?:const )?" + types + r"\s*\*?\s*([^;]+);", body) for n in decl.split(",")]
    f = _lib.InvertStepArgs
    assert order == [n for n, _ in f._fields_]
    want = dict(zip(order, [8 * i for i in range(10)] + [80, 84, 88, 96, 104, 112]))
    assert {n: getattr(f, n).offset for n in order} == want and C.sizeof(f) == 120


def test_workspace_size_is_one_pair_of_doubles_per_chunk(lib):
    ch = _lib.MSE_CHUNK
    assert lib.pf_invert_step_workspace_bytes(0, 8) == 0 and lib.pf_invert_step_workspace_bytes(3, 0) == 0
    for rows, n, chunks in ((1, 1, 1), (3, ch, 1), (3, ch + 1, 2), (2, 2 * ch + 5, 3)):
        assert lib.pf_invert_step_workspace_bytes(rows, n) == rows * chunks * 16


def test_bad_arguments_are_refused_before_any_launch(lib):
    """No GPU needed: the call returns before it touches HIP or any of the (fake) pointers."""
    coef = _lib.InvertCoef(1.01, -0.02)
    Y, E, X, R, W = FAKE, FAKE + 0x10000, FAKE + 0x20000, FAKE + 0x30000, FAKE + 0x40000

    def refused(pattern, **fields):
        a = _lib.InvertStepArgs()
        kw = dict(y=Y, eps=E, x_out=X, rows=2, row_elems=8, coef=C.addressof(coef))
        kw.update(fields)
        for k, v in kw.items():
            setattr(a, k, v)
        rc = lib.pf_invert_step(C.byref(a), None)
        msg = lib.pf_last_error().decode()
        assert rc < 0 and re.search(pattern, msg), (fields, rc, msg)

    need = int(lib.pf_invert_step_workspace_bytes(2, 8))
    res = dict(resid=R, workspace=W, workspace_bytes=need, n_slots=4, slot=1)
    refused("invert_step: bad arguments", y=None)
    refused("invert_step: bad arguments", eps=None)
    refused("invert_step: bad arguments", x_out=None)
    refused("invert_step: bad arguments", rows=0)
    refused("invert_step: bad arguments", row_elems=0)
    refused("both by value", table=FAKE, state=FAKE)
    refused("both by value", state=FAKE)
    refused("null coefficients", coef=None)
    refused("null coefficients", coef=None, table=FAKE)                     # a table without the state that names its row
    refused("y aliases x_out", x_out=Y)
    refused("y aliases x_out", x_out=Y + 16)                                # a partial overlap too
    refused("x_iter overlaps x_out", x_iter=X + 16)
    refused("without a workspace", **dict(res, workspace=None))
    refused("workspace of 32 bytes required, got 16", **dict(res, workspace_bytes=need - 16))
    refused("8-byte aligned", **dict(res, workspace=W + 4))
    refused("8-byte aligned", **dict(res, resid=R + 4))
    refused("n_slots", **dict(res, n_slots=0))
    refused("slot 4 outside", **dict(res, slot=4))
    refused("slot -1 outside", **dict(res, slot=-1))
    refused("iterate k = 3 outside", **dict(res, coef=None, table=FAKE, state=FAKE, iters=3, k=3))
    refused("iterate k = 0 outside", **dict(res, coef=None, table=FAKE, state=FAKE, iters=0, k=0))
    assert lib.pf_invert_step(None, None) < 0
    assert lib.pf_step_advance(None, 1, 0, None) < 0 and re.search("step_advance", lib.pf_last_error().decode())
    assert lib.pf_step_advance(FAKE, 1, -1, None) < 0


# ---------------------------------------------------------------------------------------------- coefficients
@pytest.mark.parametrize("kind,n", [("uniform", 50), ("uniform", 10), ("uniform", 4), ("quad", 50)])
def test_coefficient_rows_are_the_float64_value_rounded_once(lib, kind, n):
    from polyffusion_amd.sampler import invert_coef_rows
    s = ddim(lib, n, kind)
    ts = dpm_ref.grid(AB, n, kind)
    assert np.array_equal(s.time_steps, ts)
    want = invert_ref.rows(AB, ts)
    got = s.invert_rows()
    assert got.dtype == np.float32 and got.shape == want.shape == (len(ts), 2)
    # rounding to the nearest float32 moves a value by at most 2^-24 of itself; the 1e-6 on top is room for a float64 evaluation in
    # another operation order, a few 1e-16 away, to fall on the other side of a rounding boundary
    assert (np.abs(got.astype(np.float64) - want) <= 2.0 ** -24 * (1 + 1e-6) * np.abs(want)).all()
    assert np.array_equal(invert_coef_rows(s.ddim_alpha.numpy(), s.ddim_alpha_prev.numpy()).astype(np.float32), got)
    same = np.array([i > 0 and ts[i] == ts[i - 1] for i in range(len(ts))])
    assert same.any() == (kind == "quad")                                    # quad at 50 repeats time steps
    assert (got[same] == (1.0, 0.0)).all() and (want[same] == (1.0, 0.0)).all()
    assert (got[~same, 0] < 1).all() and (got[~same, 0] > 0).all() and (got[~same, 1] > 0).all()       # upwards: the signal shrinks, noise is added


def test_the_forward_step_in_the_two_forms_is_one_function(lib):
    """F(x) = sqrt(ap)*(x - sqrt(1-a)*eps)/sqrt(a) + sqrt(1-ap)*eps = (x - c_e*eps)/c_y, and one iterate from the fixed point stays there."""
    ts = dpm_ref.grid_uniform(1000, 10)
    R, D = invert_ref.rows(AB, ts), invert_ref.ddim_rows(AB, ts)
    rng = np.random.default_rng(0)
    x, eps = rng.standard_normal(16), rng.standard_normal(16)
    for i in range(len(ts)):
        y = invert_ref.forward(D[i], x, eps)
        assert np.allclose(y, (x - R[i, 1] * eps) / R[i, 0], rtol=1e-12, atol=1e-14)
        assert np.allclose(invert_ref.update(R[i], y, eps), x, rtol=1e-12, atol=1e-14)


# ---------------------------------------------------------------------------------------------- the float64 facts, by invert_ref alone
def _abs_residuals(R, gains, K):
    keep = []
    x0 = np.array([1.0, -0.5, 2.0])
    invert_ref.invert_loop(R, x0, lambda i, v: gains[i] * v, K, keep=keep)
    ys = [x0] + [k[-1] for k in keep[:-1]]
    return np.array([[np.linalg.norm(it[k] - (ys[i] if k == 0 else it[k - 1])) for k in range(K)] for i, it in enumerate(keep)])


@pytest.mark.parametrize("s", [0.5, 1.0, 4.0])
def test_float64_the_residual_shrinks_by_the_contraction_factor_per_iterate(s):
    for n, cap in ((50, 0.11), (10, 0.39)):
        ts = dpm_ref.grid_uniform(1000, n)
        R, gains = invert_ref.rows(AB, ts), dpm_ref.gauss_gain(AB, ts, s)
        q = invert_ref.contraction(R, gains)
        assert q.max() <= cap
        res = _abs_residuals(R, gains, 4)
        # exactly q per iterate; 2e-14 is float64's own noise in a norm of differences of O(1) iterates (a few ulps of |x| <= 3)
        assert (np.abs(res[:, 1:] - q[:, None] * res[:, :-1]) <= 1e-9 * q[:, None] * res[:, :-1] + 2e-14).all()
        big = q > 1e-2                                                       # where the first two residuals are far above that noise
        assert big.sum() >= n // 3 and np.allclose(res[big, 1] / res[big, 0], q[big], rtol=1e-8)


@pytest.mark.parametrize("s", [0.5, 1.0, 4.0])
def test_float64_the_round_trip_closes_geometrically(s):
    ts = dpm_ref.grid_uniform(1000, 50)
    err = {K: invert_ref.roundtrip_err(AB, ts, s, K) for K in (1, 5, 8)}
    print(f"s={s}: " + ", ".join(f"K={K} {e:.3e}" for K, e in err.items()))
    assert err[5] < 1e-3 * err[1]
    assert err[8] < 1e-9


def test_float64_bounds_are_consistent_with_the_plain_loops():
    """invert_ref's own consistency: the loops with a budget walk the same values as the plain ones, and the bound grows with the steps."""
    ts = dpm_ref.grid_uniform(1000, 10)
    R, D, gains = invert_ref.rows(AB, ts), invert_ref.ddim_rows(AB, ts), dpm_ref.gauss_gain(AB, ts, 1.0)
    x0 = np.array([1.0, -2.0])
    eps_of = lambda i, v: gains[i] * v
    x, bound, res = invert_ref.invert_gauss_with_budget(R, gains, x0, 3)
    assert np.array_equal(x, invert_ref.invert_loop(R, x0, eps_of, 3)) and res.shape == (10, 3)
    assert (bound > 0).all() and (bound < 1e-4 * np.abs(x)).all()
    low, bound_low, _ = invert_ref.invert_gauss_with_budget(R, gains, x0, 3, t_end=4)
    assert np.array_equal(low, invert_ref.invert_loop(R, x0, eps_of, 3, t_end=4)) and (bound_low < bound).all()
    back, b2 = invert_ref.paint_gauss_with_budget(D, gains, x, bound)
    assert np.array_equal(back, invert_ref.paint_loop(D, x, eps_of)) and (b2 > 0).all()
    assert np.abs(back - x0).max() < 1e-2                                    # K = 3 on 10 steps at s = 1: 9e-4 of max |x0| (roundtrip_err)


# ---------------------------------------------------------------------------------------------- invert's own refusals
def test_invert_refuses_a_stochastic_range_and_bad_indices(lib):
    x = torch.zeros(1, 2, 4, 4)
    with pytest.raises(ValueError, match="stochastic"):
        ddim(lib, 10, "uniform", 0.5).invert(x, None)
    s = ddim(lib, 10)
    for t_end in (-1, 10):
        with pytest.raises(ValueError, match="t_end"):
            s.invert(x, None, t_end)
    with pytest.raises(ValueError, match="iters"):
        s.invert(x, None, iters=0)
    from polyffusion_amd.sampler import DPMSolverSampler, SDFSampler
    assert not hasattr(DPMSolverSampler, "invert") and not hasattr(SDFSampler, "invert")


# ---------------------------------------------------------------------------------------------- the CLI
@pytest.fixture()
def npz(tmp_path):
    full, chords_only = tmp_path / "song.npz", tmp_path / "chords.npz"
    np.savez(full, chord=np.zeros((1, 32, 36), np.float32), prmat2c=np.zeros((1, 2, 128, 128), np.float32))
    np.savez(chords_only, chord=np.zeros((1, 32, 36), np.float32))
    return str(full), str(chords_only)


def test_parser_and_chord_shift():
    from polyffusion_amd import inference_sdf
    p = inference_sdf.make_parser()
    a = p.parse_args([])
    assert (a.edit, a.edit_iters, a.edit_depth, a.edit_invert_scale, a.edit_roundtrip, a.edit_chord_shift, a.edit_chords_from_midi) == \
        (False, 3, None, None, False, None, None)
    a = p.parse_args(["--edit", "--edit_iters", "5", "--edit_depth", "7", "--edit_invert_scale", "1.5", "--edit_roundtrip", "--edit_chord_shift", "-3"])
    assert (a.edit, a.edit_iters, a.edit_depth, a.edit_invert_scale, a.edit_roundtrip, a.edit_chord_shift) == (True, 5, 7, 1.5, True, -3)
    chd = torch.arange(36.0).reshape(1, 1, 36)
    got = inference_sdf.shift_chords(chd, 2)[0, 0].tolist()
    assert got == [10, 11] + list(range(10)) + [22, 23] + list(range(12, 22)) + [34, 35] + list(range(24, 34))
    assert torch.equal(inference_sdf.shift_chords(chd, 0), chd) and torch.equal(inference_sdf.shift_chords(chd, 12), chd)


def test_cli_refusals_come_before_any_weight_is_loaded(npz):
    from polyffusion_amd import inference_sdf
    full, chords_only = npz
    p = inference_sdf.make_parser()
    good = ["--edit", "--ddim", "--edit_chord_shift", "2", "--cond_npz", full]
    assert inference_sdf.check_edit_args(p.parse_args(good), "chord", 1) is True
    assert inference_sdf.check_edit_args(p.parse_args(good), "chord+txt", 1) is True
    assert inference_sdf.check_edit_args(p.parse_args([]), "txt", 4) is False

    def refused(pattern, argv, cond_type="chord", world=1):
        with pytest.raises(SystemExit, match=pattern):
            inference_sdf.check_edit_args(p.parse_args(argv), cond_type, world)

    for ct in ("txt", "pnotree", "uncond"):
        refused("cond_type chord or chord\\+txt", good, ct)
    without = lambda *flags: [v for v in good if v not in flags]
    refused("--dpm", without("--ddim") + ["--dpm"])
    refused("needs --ddim", without("--ddim"))
    refused("--ddim_eta 0", good + ["--ddim_eta", "0.5"])
    refused("--autoreg", good + ["--autoreg"])
    refused("--inpaint_type", good + ["--inpaint_type", "below"])
    refused("--from_midi2", good + ["--from_midi2", "b.mid"])
    refused("--num_generate", good + ["--num_generate", "2"])
    refused("one rank", good, world=2)
    refused("target chords", ["--edit", "--ddim", "--cond_npz", full])
    refused("give one of them", good + ["--edit_chords_from_midi", "b.mid"])
    refused("song to edit", ["--edit", "--ddim", "--edit_chord_shift", "2", "--cond_npz", chords_only])
    refused("song to edit", ["--edit", "--ddim", "--edit_chord_shift", "2", "--synthetic"])
    refused("--edit_iters", good + ["--edit_iters", "0"])
    refused("--edit_depth", good + ["--edit_depth", "50"])
    refused("belong to --edit", ["--ddim", "--edit_chord_shift", "2"])
    # through main(): what the flags alone decide is refused before the GPU, the parameters or the weights are looked at
    for pattern, argv in (("--ddim_eta 0", good + ["--ddim_eta", "1"]), ("--autoreg", good + ["--autoreg"]),
                          ("needs --ddim", without("--ddim")), ("song to edit", ["--edit", "--ddim", "--edit_chord_shift", "2", "--synthetic"])):
        with pytest.raises(SystemExit, match=pattern):
            inference_sdf.main(argv + ["--params_preset", "sdf_chd8bar", "--synthetic_weights"])
