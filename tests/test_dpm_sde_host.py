"""The stochastic DPM-Solver++(2M) without a GPU: the C entry point is declared, exported by both builds and bound, its structs are laid out
as the header says, it refuses bad arguments before any launch; ``sampler.dpm_sde_coef_rows`` against the float64 restatement in
``tests/dpm_sde_ref.py``; the three properties the form is pinned by (mean identity, variance identity, order and sign of the history
term through the closed-form variance on Gaussian data); a float32 emulation of the kernel's operation order inside the rounding budget,
with planted defects outside it; the sampler's validation and the CLI flags."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import dpm_ref
import dpm_sde_ref as ref
from polyffusion_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000          # a non-null, 16-byte aligned address that a refused call never touches
AB = dpm_ref.alpha_bar()


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
        self.alpha_bar = torch.from_numpy(AB.astype(np.float32))
        self.eps_model = None


def sampler(*a, **kw):
    from polyffusion_amd.sampler import DPMSolverSampler
    return DPMSolverSampler(Schedule(), *a, **kw)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_and_both_builds_export_the_entry_point(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "pfhip.h")).read(), flags=re.S)
    assert "pf_dpm_sde_step" in set(re.findall(r"\b(pf_[a-z0-9_]+)\s*\(", hdr))
    assert hasattr(lib, "pf_dpm_sde_step") and "pf_dpm_sde_step" in _lib.SIGNATURES
    if not os.path.exists(_lib.lib_path("f16")):
        from polyffusion_amd.build import build
        build(verbose=False, variant="f16")
    assert hasattr(_lib.load("f16"), "pf_dpm_sde_step")


def test_structs_are_laid_out_as_the_header_says():
    hdr = open(os.path.join(REPO, "include", "pfhip.h")).read()
    body = re.search(r"typedef struct pf_dpm_sde_coef \{(.*?)\} pf_dpm_sde_coef;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in re.findall(r"float ([^;]+);", body) for n in decl.split(",")]
    assert names == [n for n, _ in _lib.DpmSdeCoef._fields_] == list(ref.FIELDS) and names[:7] == [n for n, _ in _lib.DpmCoef._fields_]
    assert C.sizeof(_lib.DpmSdeCoef) == 32 and all(t is C.c_float for _, t in _lib.DpmSdeCoef._fields_)
    body = re.search(r"typedef struct pf_dpm_sde_step_args \{(.*?)\} pf_dpm_sde_step_args;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    order = [n.strip(" *") for decl in re.findall(r"(?:const )?(?:float|int|uint64_t|pf_dpm_sde_coef|pf_step_state|size_t)\s*\*?\s*([^;]+);", body)
             for n in decl.split(",")]
    f = _lib.DpmSdeStepArgs
    assert order == [n for n, _ in f._fields_]
    assert [getattr(f, n).offset for n in order] == [8 * i for i in range(17)] and C.sizeof(f) == 136
    # the fields of pf_dpm_step_args are all there
    assert {n for n, _ in _lib.DpmStepArgs._fields_} <= set(order)


def test_bad_arguments_are_refused_before_any_launch(lib):
    """No GPU needed: the call returns before it touches HIP or any of the (fake) pointers."""
    coef = _lib.DpmSdeCoef(0.6, 0.8, 0.9, 0.2, 0.0, 0.8, 0.6, 0.0)
    second = _lib.DpmSdeCoef(0.6, 0.8, 0.9, 0.3, -0.1, 0.8, 0.6, 0.0)
    noisy = _lib.DpmSdeCoef(0.6, 0.8, 0.9, 0.2, 0.0, 0.8, 0.6, 0.3)

    def refused(pattern, **fields):
        a = _lib.DpmSdeStepArgs()
        kw = dict(x=FAKE, eps=FAKE, x_out=FAKE, n=8, coef=C.addressof(coef))
        kw.update(fields)
        for k, v in kw.items():
            setattr(a, k, v)
        rc = lib.pf_dpm_sde_step(C.byref(a), None)
        msg = lib.pf_last_error().decode()
        assert rc < 0 and re.search(pattern, msg), (fields, rc, msg)

    for k in ("x", "eps", "x_out"):
        refused("dpm_sde_step: bad arguments", **{k: None})
    refused("dpm_sde_step: bad arguments", n=0)
    refused("both by value", table=FAKE, state=FAKE)
    refused("null coefficients", coef=None)
    refused("null coefficients", coef=None, table=FAKE)
    refused("all three or none", orig=FAKE)
    refused("all three or none", orig=FAKE, mask=FAKE)
    refused("all three or none", orig_noise=FAKE, mask=FAKE)
    refused("needs x0_prev", coef=C.addressof(second))
    refused("needs a noise tensor or rng", coef=C.addressof(noisy))
    refused("noise tensor must be NULL", coef=C.addressof(noisy), rng=1, noise=FAKE)
    refused("multiples of 4", coef=C.addressof(noisy), rng=1, n=6)
    refused("multiples of 4", coef=C.addressof(noisy), rng=1, elem_offset=2)
    refused("16-byte aligned", coef=C.addressof(noisy), rng=1, x=FAKE + 4)
    assert lib.pf_dpm_sde_step(None, None) < 0


# ---------------------------------------------------------------------------------------------- coefficients
@pytest.mark.parametrize("kind", ["logsnr", "uniform", "quad"])
@pytest.mark.parametrize("n", [10, 20, 50])
def test_coefficient_rows_equal_the_restatement_and_eta_0_is_the_deterministic_table(kind, n):
    from polyffusion_amd.sampler import dpm_coef_rows, dpm_sde_coef_rows
    ts = dpm_ref.grid(AB, n, kind)
    for eta in (0.0, 0.3, 1.0, 1.5):
        for order in (1, 2):
            for t_start in (len(ts) - 1, 3):
                got = dpm_sde_coef_rows(AB, ts, t_start, order, True, eta)
                want = ref.rows(AB, ts, t_start, order, True, eta)
                assert got.dtype == np.float64 and got.shape == want.shape == (t_start + 1, 8)
                assert (np.abs(got - want) <= 1e-15 * np.abs(want)).all(), (eta, order, t_start, float(np.abs(got / np.where(want == 0, 1, want) - 1).max()))
                assert ((got[:, 4] == 0) == (want[:, 4] == 0)).all()
    for order in (1, 2):
        for lof in (True, False):
            zero = dpm_sde_coef_rows(AB, ts, len(ts) - 1, order, lof, 0.0)
            assert np.array_equal(zero[:, :7], dpm_coef_rows(AB, ts, len(ts) - 1, order, lof)) and (zero[:, 7] == 0).all()


@pytest.mark.parametrize("eta", [0.0, 0.3, 1.0, 1.5])
def test_mean_and_variance_identities_hold_on_every_row(eta):
    """c_x*alpha_cur + c_0 + c_1 = alpha_tgt and c_x^2*sigma_cur^2 + sigma_n^2 = sigma_tgt^2: a step fed the true x0 maps the marginal at
    the current time step onto the marginal at the target."""
    from polyffusion_amd.sampler import dpm_sde_coef_rows
    for kind in ("logsnr", "uniform"):
        for n in (10, 20, 40, 80):
            ts = dpm_ref.grid(AB, n, kind)
            cur, tgt = ref.levels(AB, ts)
            for R in (dpm_sde_coef_rows(AB, ts, len(ts) - 1, eta=eta), ref.rows(AB, ts, eta=eta)):
                mean = np.abs(R[:, 2] * np.sqrt(cur) + R[:, 3] + R[:, 4] - np.sqrt(tgt)).max()
                var = np.abs(R[:, 2] ** 2 * (1 - cur) + R[:, 7] ** 2 - (1 - tgt)).max()
                assert mean <= 1e-13 and var <= 1e-13, (kind, n, mean, var)


@pytest.mark.parametrize("s", [0.5, 1.0])
def test_the_history_term_has_the_order_and_the_sign_that_the_variance_tells_apart(s):
    """Property 3: on Gaussian data with the optimal linear denoiser the loop's final variance is known in closed form.  The 2M form
    converges (20 -> 40 -> 80 steps, below 1e-2 at 80); the first-order loop and the loop with the sign of the 1/(2r) terms flipped are
    more than four times further off at 20 steps (measured: about 9 and 14 times)."""
    e = {n: abs(ref.var_err(AB, n, s)) for n in (20, 40, 80)}
    first, flipped = abs(ref.var_err(AB, 20, s, order=1)), abs(ref.var_err(AB, 20, s, flip_history=True))
    print(f"s={s}: 2M {e}, first order {first:.3e}, flipped {flipped:.3e}")
    assert e[20] > e[40] > e[80] and e[80] < 1e-2
    assert e[20] < first / 4 and e[20] < flipped / 4


# ---------------------------------------------------------------------------------------------- the kernel's operation order, in numpy float32
def emulate(row, x, eps, x0p, z, orig=None, on=None, m=None, defect=None):
    """pf_dpm_sde_step's individually rounded float32 operations, in its order (numpy float32 arithmetic rounds every operation)."""
    s1m, sqrt_a, c_x, c_0, c_1, q_a, q_s, sigma_n = (np.float32(v) for v in row)
    x0 = (x - s1m * eps) / sqrt_a
    xp = c_x * x + c_0 * x0
    if c_1 != 0:
        xp = xp - c_1 * x0p if defect == "history sign" else xp + c_1 * x0p
    if sigma_n != 0 and defect not in ("no noise", "noise after blend"):
        xp = xp + sigma_n * z
    if orig is not None:
        xp = (q_a * orig + q_s * on) * m + xp * (np.float32(1) - m)
    if sigma_n != 0 and defect == "noise after blend":
        xp = xp + sigma_n * z
    return xp, x0


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(11)
    d = {k: torch.randn(1028, generator=g).numpy() for k in ("x", "eps", "x0_prev", "orig", "orig_noise", "z", "z_next")}
    m = (torch.rand(1028, generator=g) > 0.3).float()
    m[::7] = 0.25
    d["mask"] = m.numpy()
    return d


def test_float32_emulation_passes_the_budget_and_planted_defects_do_not(data):
    ts = dpm_ref.grid_logsnr(AB, 20)
    R64 = ref.rows(AB, ts, eta=1.0)
    R = R64.astype(np.float32)
    pre = np.abs(R64[:, 3]) / (4 * R64[:, 1] * R64[:, 2])
    assert pre.max() < 0.5                                                   # the budget's precondition holds on these rows with margin
    d = data
    for row in (R[len(ts) - 1], R[len(ts) // 2]):                            # a first-order and a second-order row
        for known in (False, True):
            kn = dict(orig=d["orig"], orig_noise=d["orig_noise"], mask=d["mask"]) if known else {}
            want, want0 = ref.update(row, d["x"], d["eps"], d["x0_prev"], d["z"], **kn)
            bx, b0 = ref.budget(row, d["x"], d["eps"], d["x0_prev"], d["z"], **kn)
            run = lambda defect=None, z=d["z"]: emulate(row, d["x"], d["eps"], d["x0_prev"], z, kn.get("orig"), kn.get("orig_noise"), kn.get("mask"), defect)
            got, got0 = run()
            assert (np.abs(got - want) <= bx).all() and (np.abs(got0 - want0) <= b0).all()
            assert not (np.abs(run("no noise")[0] - want) <= bx).all()
            assert not (np.abs(run(z=d["z_next"])[0] - want) <= bx).all()    # the draw index off by one: another draw's values
            if row[4] != 0:
                assert not (np.abs(run("history sign")[0] - want) <= bx).all()
            if known:
                assert not (np.abs(run("noise after blend")[0] - want) <= bx).all()
    # the two defects of the coefficients break an identity
    cur, tgt = ref.levels(AB, ts)
    h = dpm_ref.lam(tgt) - dpm_ref.lam(cur)
    no_root = np.sqrt(1 - tgt) * -np.expm1(-2 * h)                           # sigma_n without the square root
    assert np.abs(R64[:, 2] ** 2 * (1 - cur) + no_root ** 2 - (1 - tgt)).max() > 1e-3
    no_exp = np.sqrt(1 - tgt) / np.sqrt(1 - cur)                             # c_x without exp(-eta*h)
    assert np.abs(no_exp * np.sqrt(cur) + R64[:, 3] + R64[:, 4] - np.sqrt(tgt)).max() > 1e-3


# ---------------------------------------------------------------------------------------------- the sampler's settings and the CLI
def test_eta_is_validated_and_decides_steering_and_morph(lib):
    from polyffusion_amd.sampler import Steering
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eta"):
            sampler(10, eta=bad)
    st = Steering(n=2, reward=lambda x0: x0.sum((1, 2, 3)).double())
    with pytest.raises(ValueError, match="deterministic.*or eta > 0"):
        sampler(10, steering=st)
    with pytest.raises(ValueError, match="deterministic"):
        sampler(10, eta=0.0, steering=st)
    s = sampler(10, eta=1.0, steering=st)
    assert s.steering is st and s.eta == 1.0 and sampler(10).eta == 0.0
    with pytest.raises(ValueError, match="graph=True"):
        sampler(10, eta=1.0, graph=True, steering=st)
    assert sampler(10)._morph_refusal() is None and "eta > 0" in sampler(10, eta=0.5)._morph_refusal()
    with pytest.raises(ValueError, match="morph"):
        sampler(10, eta=0.5).morph_from_noise([1, 2, 8, 8], torch.zeros(1, 1, 4), torch.zeros(1, 1, 4))
    rows = s.sde_coef_rows()
    assert rows.dtype == np.float32 and rows.shape == (len(s.time_steps), 8) and (rows[:, 7] > 0).all()
    want = ref.rows(AB, s.time_steps, eta=1.0)
    assert (np.abs(rows.astype(np.float64) - want) <= 2.0 ** -24 * (1 + 1e-6) * np.abs(want)).all()
    c = s._sde_coef(3, len(s.time_steps) - 1)
    assert [getattr(c, f) for f in ref.FIELDS] == rows[3].tolist()
    assert np.array_equal(sampler(10, eta=0.0).sde_coef_rows()[:, :7], sampler(10).coef_rows())


def test_cli_flags(lib):
    from polyffusion_amd import inference_sdf
    from polyffusion_amd.sampler import DPMSolverSampler
    p, check = inference_sdf.make_parser(), inference_sdf.check_steer_args
    assert p.parse_args([]).dpm_eta == 0.0 and p.parse_args(["--dpm", "--dpm_eta", "0.5"]).dpm_eta == 0.5
    got = check(p.parse_args(["--best_of", "2", "--steer", "--dpm", "--dpm_eta", "1", "--steer_every", "2", "--joint"]), "chord")
    assert got["every"] == 2
    for argv in (["--best_of", "2", "--steer", "--dpm"], ["--best_of", "2", "--steer", "--dpm", "--dpm_eta", "0"]):
        with pytest.raises(SystemExit, match="deterministic.*or eta > 0"):
            check(p.parse_args(argv), "chord")
    with pytest.raises(SystemExit, match="deterministic"):                   # through main(): before the GPU or the weights are looked at
        inference_sdf.main(["--best_of", "2", "--steer", "--dpm", "--params_preset", "sdf_chd8bar", "--synthetic_weights", "--synthetic"])
    for bad in ("-1", "nan"):
        with pytest.raises(SystemExit, match="--dpm_eta"):
            inference_sdf.main(["--dpm", "--dpm_eta", bad, "--synthetic_weights", "--synthetic"])
    with pytest.raises(SystemExit, match="belongs to --dpm"):
        inference_sdf.main(["--dpm_eta", "1", "--synthetic_weights", "--synthetic"])
    with pytest.raises(SystemExit, match="--dpm_eta 0"):
        inference_sdf.check_morph_args(p.parse_args(["--morph", "--dpm", "--dpm_eta", "1", "--synthetic"]))

    class Model:
        ldm = Schedule()

    s, t_idx = inference_sdf.make_sampler(Model(), p.parse_args(["--dpm", "--dpm_steps", "20", "--dpm_eta", "0.5", "--hip_graph"]), 3)
    assert isinstance(s, DPMSolverSampler) and s.eta == 0.5 and s.graph and t_idx == len(s.time_steps) - 1
    assert inference_sdf.make_sampler(Model(), p.parse_args(["--dpm"]), 3)[0].eta == 0.0
    # the stamp names the value only when it is set
    cut = lambda stamp: stamp[: stamp.rindex("_", 0, stamp.rindex("_"))]
    e = inference_sdf.Experiments.__new__(inference_sdf.Experiments)
    e.model_label, e.sampler = "m", s
    assert cut(e._stamp(5.0, False)) == "m[scale=5.0,dpm_eta=0.5]"
    e.sampler = sampler(10)
    assert cut(e._stamp(5.0, False)) == "m[scale=5.0]"
