"""Clipping and dynamic thresholding of the predicted x0 without a GPU: the numpy restatement in ``tests/threshold_ref.py`` against itself
(the quantile's rule, its bounds, ``np.quantile``, rows inside the range, ties), and the library and the host mirror: the C entry points are
declared, exported by both builds and bound, the struct is laid out as the header says, the workspace-size formula, every refusal before
any launch, the setting as a keyword and a validated attribute of the three families, the CLI's flags, parse errors and file stamp."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import dpm_ref
import threshold_ref as ref
from polyffusion_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x100000        # a non-null, 16-byte aligned address that a refused call never touches
NAMES = ("pf_x0_threshold", "pf_x0_threshold_workspace_bytes")
F = np.float32


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from polyffusion_amd.build import build
        build(verbose=False)
    return _lib.load()


class Schedule:
    """What the samplers read of a LatentDiffusion: the step count and the float32 schedule."""

    def __init__(self):
        self.n_steps = 1000
        self.alpha_bar = torch.from_numpy(dpm_ref.alpha_bar().astype(np.float32))
        self.beta = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000) ** 2
        self.eps_model = None


def families(**kw):
    from polyffusion_amd.sampler import DDIMSampler, DPMSolverSampler, SDFSampler
    return SDFSampler(Schedule(), **kw), DDIMSampler(Schedule(), 10, "uniform", 0.0, **kw), DPMSolverSampler(Schedule(), 10, **kw)


def bits(a):
    return (np.abs(np.asarray(a, F)).view(np.uint32)) & np.uint32(0x7FFFFFFF)


# ---------------------------------------------------------------------------------------------- the restatement against itself
def test_p_one_is_the_largest_magnitude_and_a_tiny_p_the_smallest():
    a = np.abs(np.random.default_rng(0).standard_normal(4097)).astype(F)
    assert ref.quantile(bits(a), 1.0) == float(a.max())
    assert ref.order_stats(bits(a), 1e-9)[0] == 0
    lo2 = np.sort(a)[:2].astype(np.float64)
    assert lo2[0] <= ref.quantile(bits(a), 1e-9) <= lo2[1]
    assert ref.quantile(bits(np.array([3.5], F)), 0.3) == 3.5                       # one element: a_(1) := a_(0)


def test_the_quantile_is_monotone_in_p_and_lies_between_its_two_order_statistics():
    a = np.abs(np.random.default_rng(1).standard_normal(2049)).astype(F)
    srt = np.sort(a).astype(np.float64)
    last = -1.0
    for p in np.linspace(0.001, 1.0, 173):
        k, frac, bk, bk1 = ref.order_stats(bits(a), p)
        q = ref.quantile(bits(a), p)
        assert 0.0 <= frac < 1.0 and float(np.uint32(bk).view(F)) == srt[k] and float(np.uint32(bk1).view(F)) == srt[min(k + 1, a.size - 1)]
        assert srt[k] <= q <= srt[min(k + 1, a.size - 1)] and q >= last
        last = q
    k, frac, _, _ = ref.order_stats(bits(a), 0.25)                                  # 0.25 * 2048 is integral
    assert (k, frac) == (512, 0.0) and ref.quantile(bits(a), 0.25) == srt[512]


def test_the_quantile_agrees_with_numpy_to_a_few_ulps():
    g = np.random.default_rng(2)
    for n in (5, 2047, 2048, 4100):
        a = np.abs(g.standard_normal(n)).astype(F)
        for p in (0.5, 0.995, 1.0, 0.123):
            q, want = ref.quantile(bits(a), p), float(np.quantile(a.astype(np.float64), p))
            assert abs(q - want) <= 8 * np.spacing(want), (n, p, q, want)            # numpy's lerp is another order of the same operations


def test_the_order_of_the_patterns_is_the_order_of_the_magnitudes_with_nan_on_top():
    a = np.array([0.0, -0.0, 1e-45, 1.0, np.inf, np.nan], F)
    assert list(np.argsort(bits(a), kind="stable")) == [0, 1, 2, 3, 4, 5] and bits(a)[0] == bits(a)[1] == 0


def inside_row(n=4096, seed=3):
    """A row whose x0 lies strictly inside [0, 1]: x0 chosen first, eps solved from it (the rounding of x0 is then whatever it is)."""
    g = np.random.default_rng(seed)
    tab = ref.table_of(dpm_ref.alpha_bar().astype(F))
    coef = tab[500]
    x0 = g.uniform(0.05, 0.95, n).astype(F)
    eps = g.standard_normal(n).astype(F)
    x = ((x0 + coef[1] * eps) / coef[0]).astype(F)
    return x, eps, coef


def test_a_row_inside_the_range_comes_back_bit_for_bit_in_both_modes():
    x, eps, coef = inside_row()
    x0 = (coef[0] * x).astype(F) - (coef[1] * eps).astype(F)
    assert x0.min() > 0.0 and x0.max() < 1.0
    for mode in ("clip", "dynamic"):
        out, st = ref.threshold_row(x, eps, coef, mode, p=0.995)
        assert np.array_equal(out.view(np.uint32), eps.view(np.uint32)) and st[3] == 0.0 and st[2] == 1.0
    _, st = ref.threshold_row(x, eps, coef, "dynamic", p=0.995)
    assert st[0] < 0.5 and st[1] == 0.5                                             # q below the half-width: s == h, the clip rule
    # what the rule is for: c + (x0 - c) is not x0
    c = F(0.5)
    assert ((c + (x0 - c).astype(F)).astype(F) != x0).any()


def test_tie_rows_give_the_tie_value_and_a_run_that_ends_at_k_interpolates_to_the_next_key():
    a = np.array([0.25] * 6 + [0.75] * 4, F)                                        # n = 10: p = 0.5 -> pos 4.5, k = 4 inside the run
    assert ref.quantile(bits(a), 0.5) == 0.25
    assert ref.order_stats(bits(a), 5 / 9)[0] in (4, 5)                              # (5/9 * 9 may round either way; both are stated by the rule)
    a = np.array([0.25] * 5 + [0.75] * 5, F)                                        # k = 4 is the run's last element: half-way to 0.75
    assert ref.quantile(bits(a), 0.5) == 0.5
    assert ref.quantile(bits(np.full(7, 1.5, F)), 0.3) == 1.5


def test_dynamic_thresholding_brings_the_row_into_the_range_and_s_max_binds():
    g = np.random.default_rng(5)
    tab = ref.table_of(dpm_ref.alpha_bar().astype(F))
    coef = tab[700]
    x, eps = g.standard_normal(2048).astype(F), (3.0 * g.standard_normal(2048)).astype(F)
    out, st = ref.threshold_row(x, eps, coef, "dynamic", p=0.995)
    x0n = (coef[0] * x).astype(F) - (coef[1] * out).astype(F)
    assert st[1] == st[0] > 0.5 and 0.0 < st[2] < 1.0 and st[3] > 2000
    assert x0n.min() > -1e-3 and x0n.max() < 1.0 + 1e-3                             # eps' is rounded: its x0 is the bounded one to fp32 accuracy
    _, st2 = ref.threshold_row(x, eps, coef, "dynamic", p=0.995, s_max=1.5)
    assert st2[0] == st[0] and st2[1] == 0.75 and st2[2] == float(F(0.5 / 0.75))
    row, st3 = ref.threshold_row(np.where(np.arange(2048) % 100 == 0, np.inf, x).astype(F), eps, coef, "dynamic", p=0.995)
    assert not math.isfinite(st3[0]) and math.isnan(st3[1]) and st3[3] == 0.0 and np.array_equal(row.view(np.uint32), eps.view(np.uint32))


# ---------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_and_both_builds_export_the_entry_points(lib):
    full = open(os.path.join(REPO, "include", "pfhip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    declared = set(re.findall(r"\b(pf_[a-z0-9_]+)\s*\(", hdr))
    if not os.path.exists(_lib.lib_path("f16")):
        from polyffusion_amd.build import build
        build(verbose=False, variant="f16")
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES
        assert hasattr(lib, name) and hasattr(_lib.load("f16"), name)
    assert _lib.SIGNATURES["pf_x0_threshold"] == (C.c_int, [C.POINTER(_lib.X0ThresholdArgs), C.c_void_p])
    assert _lib.SIGNATURES["pf_x0_threshold_workspace_bytes"] == (C.c_size_t, [C.c_int, C.c_size_t, C.c_int])
    assert int(re.search(r"#define PF_X0T_RESIDENT_MAX (\d+)", hdr).group(1)) == _lib.X0T_RESIDENT_MAX == 32768
    assert "Photorealistic Text-to-Image Diffusion Models" in full
    from polyffusion_amd.build import SOURCES
    assert "x0_threshold.hip" in SOURCES


def test_the_struct_is_laid_out_as_the_header_says():
    hdr = open(os.path.join(REPO, "include", "pfhip.h")).read()
    body = re.search(r"typedef struct pf_x0_threshold_args \{(.*?)\} pf_x0_threshold_args;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    types = r"(?:float|double|void|size_t|int32_t|int64_t)"
    order = [n.strip(" *") for decl in re.findall(r"(?:const )?" + types + r"\s*\*?\s*([^;]+);", body) for n in decl.split(",")]
    f = _lib.X0ThresholdArgs
    assert order == [n for n, _ in f._fields_] == list(ref.FIELDS)
    want = dict(zip(order, [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96, 104, 108, 112, 116, 120, 128]))
    assert {n: getattr(f, n).offset for n in order} == want and C.sizeof(f) == 136


def test_workspace_size_is_nothing_for_the_resident_form_and_two_histograms_per_chunk_for_the_streamed_one(lib):
    ch, ws = _lib.MSE_CHUNK, lib.pf_x0_threshold_workspace_bytes
    for form in (0, 1, 2):
        assert ws(0, 8, form) == 0 and ws(3, 0, form) == 0 and ws(-1, 8, form) == 0
    assert ws(2, 8, 3) == 0 and ws(2, 8, -1) == 0
    per_chunk, per_row = (2 * 256 + 2) * 4, 4 * 2 * 8           # two 256-bin histograms, the smallest key above, the change count; the select's state
    for rows, n, chunks in ((1, 1, 1), (3, ch, 1), (3, ch + 1, 2), (2, 2 * ch + 5, 3), (32, 32768, 16), (4, 32769, 17), (4, 2 * 128 * 512, 64)):
        assert ws(rows, n, 2) == rows * (per_row + chunks * per_chunk)
        assert ws(rows, n, 1) == 0
        assert ws(rows, n, 0) == (0 if n <= 32768 else rows * (per_row + chunks * per_chunk))


def test_bad_arguments_are_refused_before_any_launch(lib):
    """No GPU needed: the call returns before it touches HIP or any of the (fake) device pointers."""
    X, E, O, T, TB, S, K = (FAKE + i * 0x100000 for i in range(7))
    need = int(lib.pf_x0_threshold_workspace_bytes(2, 8, 2))
    base = dict(x=X, x_row_stride=8, eps=E, eps_out=O, t=T, t_stride=1, table=TB, n_table=1000, stats=S, workspace=K, workspace_bytes=need,
                p=0.995, s_max=math.inf, lo=0.0, hi=1.0, mode=1, form=2, rows=2, row_elems=8)

    def refused(pattern, **fields):
        a = _lib.X0ThresholdArgs()
        for k, v in {**base, **fields}.items():
            setattr(a, k, v)
        rc = lib.pf_x0_threshold(C.byref(a), None)
        msg = lib.pf_last_error().decode()
        assert rc == -1 and msg.startswith("x0_threshold: ") and re.search(pattern, msg), (fields, rc, msg)

    for name in ("x", "eps", "eps_out", "t", "table"):
        refused("null x, eps, eps_out, t or table", **{name: None})
    refused("0 rows", rows=0)
    refused("-1 rows", rows=-1)
    refused("of 0 elements", row_elems=0)
    refused("x_row_stride 7 below row_elems 8", x_row_stride=7)
    refused("t_stride -1", t_stride=-1)
    refused("n_table 0", n_table=0)
    for lo, hi in ((1.0, 1.0), (1.0, 0.0), (math.nan, 1.0), (0.0, math.nan), (-math.inf, 1.0), (0.0, math.inf)):
        refused("is not lo < hi, both finite", lo=lo, hi=hi)
    for bad, shown in ((0.0, "0"), (-0.5, "-0.5"), (1.0000001, "1"), (math.nan, "nan"), (math.inf, "inf")):
        refused(rf"p {shown}\S* outside \(0, 1\]", p=bad)
    for bad in (0.999, 0.0, -1.0, math.nan):
        refused("s_max .* below 1", s_max=bad)
    for bad in (-1, 2, 7):
        refused(f"unknown mode {bad}", mode=bad)
    for bad in (-1, 3):
        refused(f"unknown form {bad}", form=bad)
    refused("the resident form holds rows of at most 32768 elements, got 32769", form=1, row_elems=32769, x_row_stride=32769)
    refused("eps_out overlaps eps partially", eps_out=E + 4)
    refused("eps_out overlaps eps partially", eps_out=E + 2 * 8 * 4 - 4)
    refused("eps_out overlaps eps partially", eps_out=E - 2 * 8 * 4 + 4)
    refused("eps_out overlaps x", eps_out=X)
    refused("eps_out overlaps x", eps_out=X + (12 + 8) * 4 - 4, x_row_stride=12)            # the last state element of the second row
    refused("eps_out overlaps table", eps_out=TB + 1000 * 16 - 4)
    refused("eps_out overlaps t", eps_out=T + 3 * 8, t_stride=3)                             # row 1 reads t[3]
    refused("stats must be 8-byte aligned", stats=S + 4)
    refused("no workspace", workspace=None)
    refused(f"workspace of {need} bytes required, got {need - 1}", workspace_bytes=need - 1)
    refused("workspace must be 8-byte aligned", workspace=K + 4)
    refused("more workgroups than one launch holds", rows=2 ** 30, row_elems=2 * _lib.MSE_CHUNK, x_row_stride=2 * _lib.MSE_CHUNK, workspace_bytes=2 ** 62,
            eps_out=FAKE + 2 ** 50)
    assert lib.pf_x0_threshold(None, None) == -1 and lib.pf_last_error().decode().startswith("x0_threshold: ")


def test_the_table_is_float64_rounded_once():
    from polyffusion_amd import _steps
    ab = torch.from_numpy(dpm_ref.alpha_bar().astype(F))
    tab = _steps.x0_threshold_table(ab).numpy()
    assert tab.shape == (1000, 4) and tab.dtype == F and np.array_equal(tab.view(np.uint32), ref.table_of(ab.numpy()).view(np.uint32))
    a = ab.double().numpy()
    assert np.array_equal(tab[:, 0], (1 / np.sqrt(a)).astype(F)) and np.array_equal(tab[:, 3], (np.sqrt(a) / np.sqrt(1 - a)).astype(F))


# ---------------------------------------------------------------------------------------------- the setting
def test_the_setting_validates_its_fields_and_spells_its_label():
    from polyffusion_amd.sampler import X0Threshold
    th = X0Threshold()
    assert (th.mode, th.p, th.range, th.s_max) == ("dynamic", 0.995, (0.0, 1.0), math.inf) and th.label == "x0thr=0.995"
    assert X0Threshold("clip").label == "x0clip" and X0Threshold("clip", range=[-1, 1]).label == "x0clip,x0range=-1.0-1.0"
    assert X0Threshold(p=0.9, s_max=2).label == "x0thr=0.9,x0max=2.0" and X0Threshold(range=(-1, 1)).range == (-1.0, 1.0)
    assert hash(X0Threshold(p=0.9)) == hash(X0Threshold(p=0.9)) and X0Threshold(p=0.9) != X0Threshold(p=0.95)
    for kw in (dict(mode="static"), dict(p=0.0), dict(p=1.5), dict(p=math.nan), dict(range=(1, 1)), dict(range=(0, math.inf)), dict(range=5),
               dict(range=(0, 1, 2)), dict(s_max=0.5), dict(s_max=math.nan)):
        with pytest.raises(ValueError, match="x0_threshold"):
            X0Threshold(**kw)


def test_the_setting_is_a_keyword_and_attribute_of_all_three_families(lib):
    from polyffusion_amd.sampler import X0Threshold
    for s in families():
        assert s.x0_threshold is None and s.last_threshold is None
        s.x0_threshold = X0Threshold("clip")
        assert s.x0_threshold == X0Threshold("clip")
        for bad in (0.995, "dynamic", (0.0, 1.0)):
            with pytest.raises(ValueError, match="x0_threshold"):
                s.x0_threshold = bad
        assert s.x0_threshold == X0Threshold("clip")                                # a refused value changes nothing
        s.x0_threshold = None
        assert s.x0_threshold is None
    for s in families(x0_threshold=X0Threshold(p=0.9), guidance_interval=(10, 20)):
        assert s.x0_threshold.p == 0.9 and s.guidance_interval == (10, 20)          # independent of the interval
    assert all(s.x0_threshold.mode == "dynamic" for s in families(graph=True, x0_threshold=X0Threshold()))
    with pytest.raises(ValueError, match="x0_threshold"):
        families(x0_threshold=0.995)


# ---------------------------------------------------------------------------------------------- the CLI
def test_parser_defaults_flags_and_parse_errors(capsys):
    from polyffusion_amd import inference_sdf
    from polyffusion_amd.sampler import X0Threshold
    p, check = inference_sdf.make_parser(), inference_sdf.check_threshold_args
    a = p.parse_args([])
    assert (a.x0_clip, a.x0_threshold, a.x0_range, a.x0_threshold_max) == (False, None, None, None) and check(a) is None
    assert check(p.parse_args(["--x0_clip"])) == X0Threshold("clip")
    assert check(p.parse_args(["--x0_threshold", "0.995"])) == X0Threshold()
    assert check(p.parse_args(["--x0_threshold", "0.9", "--x0_range", "-1", "1", "--x0_threshold_max", "3"])) == X0Threshold("dynamic", 0.9, (-1.0, 1.0), 3.0)
    assert check(p.parse_args(["--x0_clip", "--x0_range", "-1", "1", "--hip_graph"])) == X0Threshold("clip", range=(-1.0, 1.0))
    for bad in (["--x0_threshold"], ["--x0_threshold", "x"], ["--x0_range", "0"], ["--x0_range", "0", "1", "2"], ["--x0_threshold_max", "a"], ["--x0_clip", "1"]):
        with pytest.raises(SystemExit) as e:
            p.parse_args(bad)
        assert e.value.code == 2
    for bad, said in ((["--x0_threshold", "0"], "P lies in (0, 1]"), (["--x0_threshold", "1.5"], "P lies in (0, 1]"), (["--x0_threshold", "nan"], "P lies in (0, 1]"),
                      (["--x0_clip", "--x0_threshold", "0.9"], "give one of them"), (["--x0_range", "0", "1"], "nothing to apply them to"),
                      (["--x0_threshold_max", "2"], "nothing to apply them to"), (["--x0_clip", "--x0_threshold_max", "2"], "no threshold to cap"),
                      (["--x0_threshold", "0.9", "--x0_threshold_max", "0.5"], "R is at least 1"), (["--x0_clip", "--x0_range", "1", "0"], "LO < HI"),
                      (["--x0_clip", "--x0_range", "0", "inf"], "LO < HI")):
        with pytest.raises(SystemExit) as e:
            check(p.parse_args(bad))
        assert e.value.code == 2 and said in capsys.readouterr().err, bad
    # through main(): refused before the GPU, the parameters or the weights are looked at
    for bad in (["--x0_threshold", "2"], ["--x0_clip", "--x0_threshold", "0.9"]):
        with pytest.raises(SystemExit) as e:
            inference_sdf.main(bad + ["--params_preset", "sdf_chd8bar", "--synthetic_weights", "--synthetic"])
        assert e.value.code == 2


def test_the_stamp_names_the_setting_only_when_set(lib):
    from polyffusion_amd.inference_sdf import Experiments
    from polyffusion_amd.sampler import X0Threshold
    cut = lambda s: s[: s.rindex("_", 0, s.rindex("_"))]                         # without the date and time
    for sampler in families():
        e = Experiments("m", dict(n_steps=1000), sampler, t_idx=3)
        assert cut(e._stamp(5.0, False)) == "m[scale=5.0]"
    for sampler in families(x0_threshold=X0Threshold(), guidance_rescale=0.7):
        e = Experiments("m", dict(n_steps=1000), sampler, t_idx=3)
        assert cut(e._stamp(5.0, False)) == "m[scale=5.0,rescale=0.7,x0thr=0.995]"
        sampler.guidance_rescale, sampler.x0_threshold = 0.0, X0Threshold("clip")
        assert cut(e._stamp(5.0, True)) == "m[scale=5.0,autoreg,x0clip]"
        assert cut(e._stamp(5.0, False, "", "mean")) == "m[scale=5.0,joint,x0clip]"
        sampler.x0_threshold = X0Threshold(p=0.9, range=(-1, 1), s_max=2)
        assert cut(e._stamp(5.0, False)) == "m[scale=5.0,x0thr=0.9,x0range=-1.0-1.0,x0max=2.0]"
