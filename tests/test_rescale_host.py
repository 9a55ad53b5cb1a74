"""Guidance rescale and the guidance interval without a GPU: the C entry points are declared, exported by both builds and bound, the struct
is laid out as the header says, bad arguments are refused before any launch; the identities of the numpy restatement in
``tests/rescale_ref.py`` (phi = 0, equal groups, phi = 1); the interval's mapping, validation and normalisation; the samplers' refusals;
the CLI's parse errors and file stamp; and ``guidance_plan``, which the feature leaves alone."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import dpm_ref
import rescale_ref
from polyffusion_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000          # a non-null, 16-byte aligned address that a refused call never touches
NAMES = ("pf_cfg_rescale", "pf_cfg_rescale_workspace_bytes")


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
    assert "pf_cfg_rescale_args" in hdr
    assert _lib.SIGNATURES["pf_cfg_rescale"] == (C.c_int, [C.POINTER(_lib.CfgRescaleArgs), C.c_void_p])
    assert _lib.SIGNATURES["pf_cfg_rescale_workspace_bytes"] == (C.c_size_t, [C.c_int, C.c_size_t])
    full = open(os.path.join(REPO, "include", "pfhip.h")).read()
    assert "Common Diffusion Noise Schedules and Sample Steps Are Flawed" in full and "Applying Guidance in a Limited Interval" in full


def test_the_struct_is_laid_out_as_the_header_says():
    hdr = open(os.path.join(REPO, "include", "pfhip.h")).read()
    body = re.search(r"typedef struct pf_cfg_rescale_args \{(.*?)\} pf_cfg_rescale_args;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    types = r"(?:float|double|void|size_t|int32_t)"
    order = [n.strip(" *") for decl in re.findall(r"(?:const )?" + types + r"\s*\*?\s*([^;]+);", body) for n in decl.split(",")]
    f = _lib.CfgRescaleArgs
    assert order == [n for n, _ in f._fields_] == list(rescale_ref.FIELDS)
    want = dict(zip(order, [0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 68, 72]))
    assert {n: getattr(f, n).offset for n in order} == want and C.sizeof(f) == 80


def test_workspace_size_is_one_quadruple_of_double_double_pairs_per_chunk(lib):
    ch = _lib.MSE_CHUNK
    assert lib.pf_cfg_rescale_workspace_bytes(0, 8) == 0 and lib.pf_cfg_rescale_workspace_bytes(3, 0) == 0
    assert lib.pf_cfg_rescale_workspace_bytes(-1, 8) == 0
    for rows, n, chunks in ((1, 1, 1), (3, ch, 1), (3, ch + 1, 2), (2, 2 * ch + 5, 3), (32, 32768, 16)):
        assert lib.pf_cfg_rescale_workspace_bytes(rows, n) == rows * chunks * 64


def test_bad_arguments_are_refused_before_any_launch(lib):
    """No GPU needed: the call returns before it touches HIP or any of the (fake) device pointers."""
    E, O, S, W, K = FAKE, FAKE + 0x10000, FAKE + 0x20000, FAKE + 0x30000, FAKE + 0x40000
    need = int(lib.pf_cfg_rescale_workspace_bytes(2, 8))
    assert need == 128

    def refused(pattern, **fields):
        a = _lib.CfgRescaleArgs()
        kw = dict(epsg=E, eps=O, stats=S, weights=W, workspace=K, workspace_bytes=need, phi=0.7, s1=5.0, s2=0.0, groups=2, rows=2, row_elems=8)
        kw.update(fields)
        for k, v in kw.items():
            setattr(a, k, v)
        rc = lib.pf_cfg_rescale(C.byref(a), None)
        msg = lib.pf_last_error().decode()
        assert rc == -1 and msg.startswith("cfg_rescale:") and re.search(pattern, msg), (fields, rc, msg)

    for name in ("epsg", "eps"):
        refused("null epsg or eps", **{name: None})
    for bad in (1, 4, 0, -1):
        refused(f"groups {bad}, expected 2 or 3", groups=bad)
    refused("0 rows", rows=0)
    refused("-1 rows", rows=-1)
    refused("of 0 elements", row_elems=0)
    for bad, shown in ((-0.25, "-0.25"), (1.5, "1.5"), (math.nan, "nan"), (math.inf, "inf")):
        refused(rf"phi {shown} outside \[0, 1\]", phi=bad)
    refused("eps overlaps epsg", eps=E)
    refused("eps overlaps epsg", eps=E + 2 * 2 * 8 * 4 - 4)                    # the last float of the second group
    refused("eps overlaps epsg", eps=E + 3 * 2 * 8 * 4 - 4, groups=3)
    refused("eps overlaps epsg", eps=E - 2 * 8 * 4 + 4)                        # the result's tail reaches into the first group
    refused("no workspace", workspace=None)
    refused("workspace of 128 bytes required, got 64", workspace_bytes=64)
    refused("workspace must be 8-byte aligned", workspace=K + 4)
    refused("stats must be 8-byte aligned", stats=S + 4)
    refused("more workgroups than one launch holds", rows=2 ** 31 - 1, row_elems=2 * _lib.MSE_CHUNK, workspace_bytes=2 ** 62)
    refused("more workgroups than one launch holds", rows=2 ** 30, row_elems=2 * _lib.MSE_CHUNK, workspace_bytes=2 ** 62)   # exactly 2^31
    assert lib.pf_cfg_rescale(None, None) == -1 and lib.pf_last_error().decode().startswith("cfg_rescale:")


# ---------------------------------------------------------------------------------------------- the restatement's identities
def groups_of(kind, G=2, rows=3, n=1000):
    g = np.random.default_rng(4).standard_normal((G, rows, n)).astype(np.float32)
    return (g + np.float32(10)).astype(np.float32) if kind == "mean10" else g


@pytest.mark.parametrize("G", [2, 3])
def test_phi_zero_is_the_plain_combine_bit_for_bit(G):
    g = groups_of("normal", G)
    r = rescale_ref.rescale(g, 5.0, 1.5, 0.0)
    assert (r["w"] == 1.0).all() and np.array_equal(r["out"].view(np.uint32), r["e_cfg"].view(np.uint32))
    assert (r["f"] < 1.0).all() and (r["f"] > 0.0).all()                         # guidance at scale 5 did widen the rows
    import guidance_ref
    want = guidance_ref.combine2_f32(g[0], g[1], 5.0) if G == 2 else guidance_ref.combine3_f32(g[0], g[1], g[2], 5.0, 1.5)
    assert np.array_equal(r["e_cfg"].view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("phi", [0.3, 0.7, 1.0])
def test_equal_groups_and_constant_rows_have_weight_one(phi):
    g = groups_of("normal")
    same = np.stack([g[1], g[1]])                                                # e_pos == e_u: e_cfg == e_pos, so var_cfg == var_pos
    r = rescale_ref.rescale(same, 5.0, 0.0, phi)
    assert (r["f"] == 1.0).all() and (r["w"] == 1.0).all() and np.array_equal(r["out"].view(np.uint32), same[1].view(np.uint32))
    const = np.full((2, 2, 37), 1.5, np.float32)
    r = rescale_ref.rescale(const, 5.0, 0.0, phi)
    assert (r["var_cfg"] == 0.0).all() and (r["f"] == 1.0).all() and (r["w"] == 1.0).all()
    flat = g.copy()
    flat[0] = 0.5                                                               # scale 0 on a constant e_u: var_cfg == 0 < var_pos
    r = rescale_ref.rescale(flat, 0.0, 0.0, phi)
    assert (r["var_cfg"] == 0.0).all() and (r["var_pos"] > 0.5).all() and (r["w"] == 1.0).all()


@pytest.mark.parametrize("kind", ["normal", "mean10"])
@pytest.mark.parametrize("G", [2, 3])
def test_phi_one_restores_the_conditional_rows_standard_deviation(G, kind):
    g = groups_of(kind, G)
    r = rescale_ref.rescale(g, 5.0, 3.0, 1.0)
    got, want = rescale_ref.std_rows(r["out"]), rescale_ref.std_rows(g[-1])
    assert (np.abs(got / want - 1.0) <= 1e-6).all(), got / want                   # w and the products round to float32: 2^-24 each and less
    assert (rescale_ref.std_rows(r["e_cfg"]) > 2.0 * want).all()                  # and there was something to restore
    half = rescale_ref.rescale(g, 5.0, 3.0, 0.5)
    assert np.allclose(half["w"], 0.5 * r["f"] + 0.5, rtol=2.0 ** -23, atol=0.0)


# ---------------------------------------------------------------------------------------------- the interval
def test_interval_from_fractions_validation_and_normalisation():
    from polyffusion_amd.sampler import guidance_interval_from_fractions as fr, normalize_guidance_interval as norm
    assert fr(0.2, 0.8, 1000) == (200, 799) == rescale_ref.interval_from_fractions(0.2, 0.8, 1000)     # ceil(199.8), floor(799.2)
    assert fr(0.25, 0.75, 5) == (1, 3) and fr(0.3, 0.3, 11) == (3, 3) and fr(0.5, 1.0, 1000) == (500, 999)
    assert fr(0.0, 1.0, 1000) is None and norm((0, 999), 1000) is None and norm(None, 1000) is None
    assert norm((0, 998), 1000) == (0, 998) and norm((1, 999), 1000) == (1, 999) and norm([np.int64(3), 7.0], 10) == (3, 7)
    for lo, hi in ((-0.1, 0.5), (0.6, 0.5), (0.5, 1.1), (math.nan, 0.5), (0.5, math.nan)):
        with pytest.raises(ValueError, match="0 <= LO <= HI <= 1"):
            fr(lo, hi, 1000)
    with pytest.raises(ValueError, match="hold no time step"):
        fr(0.3001, 0.3002, 1000)
    for bad in ((-1, 5), (6, 5), (0, 1000), (2.5, 7), "ab", (1, 2, 3), 5):
        with pytest.raises(ValueError, match="guidance_interval"):
            norm(bad, 1000)


def test_the_settings_are_keywords_and_attributes_of_all_three_families(lib):
    for s in families():
        assert s.guidance_rescale == 0.0 and s.guidance_interval is None and s.last_rescale is None
        assert s.guided_at(0) and s.guided_at(999)
        s.guidance_rescale, s.guidance_interval = 0.7, (200, 799)
        assert s.guidance_rescale == 0.7 and s.guidance_interval == (200, 799)
        assert [s.guided_at(t) for t in (199, 200, 500, 799, 800)] == [False, True, True, True, False]
        s.guidance_interval = (0, 999)
        assert s.guidance_interval is None
        for bad in (-0.1, 1.01, math.nan):
            with pytest.raises(ValueError, match="guidance_rescale"):
                s.guidance_rescale = bad
        with pytest.raises(ValueError, match="guidance_interval"):
            s.guidance_interval = (5, 1000)
        assert s.guidance_rescale == 0.7 and s.guidance_interval is None            # a refused value changes nothing
    for s in families(guidance_rescale=0.5, guidance_interval=(10, 20)):
        assert s.guidance_rescale == 0.5 and s.guidance_interval == (10, 20)
    with pytest.raises(ValueError, match="guidance_rescale"):
        families(guidance_rescale=2.0)
    with pytest.raises(ValueError, match="guidance_interval"):
        families(guidance_interval=(3, 2))


def test_an_interval_with_graph_is_refused_by_name_and_get_eps_needs_the_time_step(lib):
    from polyffusion_amd.sampler import DDIMSampler
    with pytest.raises(ValueError, match="guidance_interval.*graph=True"):
        families(graph=True, guidance_interval=(10, 20))
    assert all(s.guidance_interval is None for s in families(graph=True, guidance_interval=(0, 999)))       # the whole schedule is no interval
    s = DDIMSampler(Schedule(), 10, "uniform", 0.0, graph=True)
    s.guidance_interval = (10, 20)                                                # set afterwards: refused where the capture would start
    x, c = torch.zeros(1, 2, 4, 4), torch.zeros(1, 1, 4)
    with pytest.raises(ValueError, match="guidance_interval.*graph=True"):
        s._replay_loop("ddim", dict(x=x, cond=c), None, None, 0, 0, 1, 0, 1.0, None)
    s = DDIMSampler(Schedule(), 10, "uniform", 0.0, guidance_interval=(10, 20))
    with pytest.raises(ValueError, match="t_value"):
        s.get_eps(x, torch.zeros(1, dtype=torch.long), c, uncond_scale=5.0, uncond_cond=c)
    # the helper every loop goes through: as given inside, scale 1 and the prefix of cond alone outside
    prep = {"time_table": 1, "cross": 2, "unguided": {"time_table": 1, "cross": 3}}
    assert s._guidance_at(15, 5.0, prep) == (5.0, prep) and s._guidance_at(21, 5.0, prep) == (1.0, prep["unguided"])
    assert s._guidance_at(9, 5.0, None) == (1.0, None)
    s.guidance_interval = None
    assert s._guidance_at(None, 5.0, prep) == (5.0, prep)


def test_guidance_plan_is_untouched():
    from polyffusion_amd.sampler import DualScale, guidance_plan
    c, uc = torch.arange(8.0).reshape(2, 1, 4), -torch.ones(2, 1, 4)
    assert guidance_plan(c, 1.0, uc)[1:] == (1, ()) and guidance_plan(c, 1.0, uc)[0] is c
    assert guidance_plan(c, 0.0, uc)[0] is uc and guidance_plan(c, 5.0, None)[0] is c
    ctx, groups, scales = guidance_plan(c, 5.0, uc)
    assert groups == 2 and scales == (5.0,) and torch.equal(ctx, torch.cat([uc, c]))
    ctx, groups, scales = guidance_plan(c, DualScale(3.0, 5.0, 2), uc)
    assert groups == 3 and scales == (3.0, 5.0) and torch.equal(ctx, torch.cat([uc, DualScale(3.0, 5.0, 2).partial(c, uc), c]))
    assert guidance_plan(c, DualScale(3.0, 3.0, 2), uc)[1:] == (2, (3.0,))


# ---------------------------------------------------------------------------------------------- the CLI
def test_parser_defaults_flags_and_parse_errors(capsys):
    from polyffusion_amd import inference_sdf
    p = inference_sdf.make_parser()
    a = p.parse_args([])
    assert a.guidance_rescale == 0.0 and a.guidance_interval is None and inference_sdf.check_guidance_args(a, 1000) == (0.0, None)
    a = p.parse_args(["--guidance_rescale", "0.7", "--guidance_interval", "0.2", "0.8"])
    assert a.guidance_rescale == 0.7 and a.guidance_interval == [0.2, 0.8]
    assert inference_sdf.check_guidance_args(a) == (0.7, None) and inference_sdf.check_guidance_args(a, 1000) == (0.7, (200, 799))
    assert inference_sdf.check_guidance_args(p.parse_args(["--guidance_interval", "0", "1"]), 1000) == (0.0, None)
    for bad in (["--guidance_rescale", "x"], ["--guidance_interval", "0.2"], ["--guidance_interval", "0.2", "0.8", "0.9"], ["--guidance_interval", "a", "b"]):
        with pytest.raises(SystemExit) as e:
            p.parse_args(bad)
        assert e.value.code == 2
    for bad, said in ((["--guidance_rescale", "1.5"], "PHI lies in"), (["--guidance_rescale", "-0.1"], "PHI lies in"), (["--guidance_rescale", "nan"], "PHI lies in"),
                      (["--guidance_interval", "0.8", "0.2"], "0 <= LO <= HI <= 1"), (["--guidance_interval", "-0.1", "0.5"], "0 <= LO <= HI <= 1"),
                      (["--guidance_interval", "0.5", "1.5"], "0 <= LO <= HI <= 1"),
                      (["--guidance_interval", "0.2", "0.8", "--hip_graph"], "--guidance_interval with --hip_graph")):
        with pytest.raises(SystemExit) as e:
            inference_sdf.check_guidance_args(p.parse_args(bad))
        assert e.value.code == 2 and said in capsys.readouterr().err, bad
    with pytest.raises(SystemExit) as e:
        inference_sdf.check_guidance_args(p.parse_args(["--guidance_interval", "0.3001", "0.3002"]), 1000)
    assert e.value.code == 2 and "hold no time step" in capsys.readouterr().err
    # through main(): refused before the GPU, the parameters or the weights are looked at
    for bad in (["--guidance_interval", "0.2", "0.8", "--hip_graph"], ["--guidance_rescale", "2"]):
        with pytest.raises(SystemExit) as e:
            inference_sdf.main(bad + ["--params_preset", "sdf_chd8bar", "--synthetic_weights", "--synthetic"])
        assert e.value.code == 2
    assert inference_sdf.check_guidance_args(p.parse_args(["--guidance_rescale", "0.7", "--hip_graph"]), 1000) == (0.7, None)    # phi alone may be captured


def test_the_stamp_names_the_settings_only_when_set(lib):
    from polyffusion_amd.inference_sdf import Experiments
    from polyffusion_amd.sampler import DualScale

    class Bare:                     # a sampler that predates the settings
        time_steps = list(range(10))

    cut = lambda s: s[: s.rindex("_", 0, s.rindex("_"))]                         # without the date and time
    for sampler in (Bare(),) + families():
        e = Experiments("m", dict(n_steps=1000), sampler, t_idx=3)
        assert cut(e._stamp(5.0, False)) == "m[scale=5.0]" and cut(e._stamp(1.0, True, "_inp1_below")) == "m_inp1_below[scale=1.0,autoreg]"
        assert cut(e._stamp(DualScale(3, 1.5, 12), False, "", "ramp")) == "m[scale=chd:3.0,txt:1.5,joint-ramp]"
    for sampler in families(guidance_rescale=0.7, guidance_interval=(200, 799)):
        e = Experiments("m", dict(n_steps=1000), sampler, t_idx=3)
        assert cut(e._stamp(5.0, False)) == "m[scale=5.0,rescale=0.7,interval=200-799]"
        assert cut(e._stamp(5.0, False, "", "mean")) == "m[scale=5.0,joint,rescale=0.7,interval=200-799]"
        sampler.guidance_interval = None
        assert cut(e._stamp(5.0, True)) == "m[scale=5.0,autoreg,rescale=0.7]"
        sampler.guidance_rescale, sampler.guidance_interval = 0.0, (0, 500)
        assert cut(e._stamp(5.0, False)) == "m[scale=5.0,interval=0-500]"
