"""A path between two songs without a GPU: the C entry points are declared, exported by both builds and bound, the struct is laid out as
the header says, bad arguments are refused before any launch; the float64 facts of the restatement in ``tests/morph_ref.py`` (end
weights, unit norm on orthonormal rows, the fallback classes); ``morph_fractions``; the samplers' own refusals; and the CLI's."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import dpm_ref
import morph_ref
from polyffusion_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000          # a non-null, 16-byte aligned address that a refused call never touches
NAMES = ("pf_slerp_rows", "pf_slerp_rows_workspace_bytes")


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
    assert "pf_slerp_args" in hdr
    assert int(re.search(r"#define PF_SLERP_MAX_FRAMES (\d+)", hdr).group(1)) == _lib.SLERP_MAX_FRAMES == 64


def test_the_struct_is_laid_out_as_the_header_says():
    hdr = open(os.path.join(REPO, "include", "pfhip.h")).read()
    body = re.search(r"typedef struct pf_slerp_args \{(.*?)\} pf_slerp_args;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    types = r"(?:float|double|void|size_t|int32_t)"
    order = [n.strip(" *") for decl in re.findall(r"(?:const )?" + types + r"\s*\*?\s*([^;]+);", body) for n in decl.split(",")]
    f = _lib.SlerpArgs
    assert order == [n for n, _ in f._fields_] == list(morph_ref.FIELDS)
    want = dict(zip(order, [8 * i for i in range(8)] + [64, 68, 72, 80]))
    assert {n: getattr(f, n).offset for n in order} == want and C.sizeof(f) == 88


def test_workspace_size_is_one_triple_of_doubles_per_chunk(lib):
    ch = _lib.MSE_CHUNK
    assert lib.pf_slerp_rows_workspace_bytes(0, 8) == 0 and lib.pf_slerp_rows_workspace_bytes(3, 0) == 0
    assert lib.pf_slerp_rows_workspace_bytes(-1, 8) == 0
    for rows, n, chunks in ((1, 1, 1), (3, ch, 1), (3, ch + 1, 2), (2, 2 * ch + 5, 3)):
        assert lib.pf_slerp_rows_workspace_bytes(rows, n) == rows * chunks * 24


def test_bad_arguments_are_refused_before_any_launch(lib):
    """No GPU needed: the call returns before it touches HIP or any of the (fake) device pointers."""
    A, B, O, S, W, K = FAKE, FAKE + 0x10000, FAKE + 0x20000, FAKE + 0x40000, FAKE + 0x50000, FAKE + 0x60000
    t = (C.c_double * 64)(*([0.0, 0.5, 1.0] + [0.25] * 61))
    need = int(lib.pf_slerp_rows_workspace_bytes(2, 8))
    assert need == 48

    def refused(pattern, **fields):
        a = _lib.SlerpArgs()
        kw = dict(a=A, b=B, t=C.addressof(t), out=O, stats=S, weights=W, workspace=K, workspace_bytes=need, mode=0, frames=3, rows=2, row_elems=8)
        kw.update(fields)
        for k, v in kw.items():
            setattr(a, k, v)
        rc = lib.pf_slerp_rows(C.byref(a), None)
        msg = lib.pf_last_error().decode()
        assert rc < 0 and msg.startswith("slerp_rows:") and re.search(pattern, msg), (fields, rc, msg)

    for name in ("a", "b", "out", "t"):
        refused("null a, b, out or t", **{name: None})
    refused("0 rows", rows=0)
    refused("-1 rows", rows=-1)
    refused("of 0 elements", row_elems=0)
    refused(r"0 frames outside \[1, 64\]", frames=0)
    refused(r"65 frames outside \[1, 64\]", frames=65)
    for bad, shown in ((-0.25, "-0.25"), (1.5, "1.5"), (math.nan, "nan"), (math.inf, "inf")):
        tb = (C.c_double * 3)(0.0, bad, 1.0)
        refused(rf"t\[1\] = {shown} outside \[0, 1\]", t=C.addressof(tb))
    refused("mode 2", mode=2)
    refused("mode -1", mode=-1)
    refused("out overlaps a", out=A)
    refused("out overlaps a", out=A + 16)                                    # a partial overlap too
    refused("out overlaps a", out=A - 3 * 2 * 8 * 4 + 16)                    # the last frame's tail reaches into a
    refused("out overlaps b", out=B)
    refused("out overlaps b", out=B + 2 * 8 * 4 - 4)
    refused("without a workspace", workspace=None)
    refused("workspace of 48 bytes required, got 24", workspace_bytes=24)
    refused("workspace must be 8-byte aligned", workspace=K + 4)
    refused("stats must be 8-byte aligned", stats=S + 4)
    refused("stats must be 8-byte aligned", stats=S + 4, mode=1)
    refused("more workgroups than one launch holds", rows=2 ** 31 - 1, row_elems=2 * _lib.MSE_CHUNK, workspace_bytes=2 ** 62, out=2 ** 60)
    assert lib.pf_slerp_rows(None, None) < 0 and lib.pf_last_error().decode().startswith("slerp_rows:")


# ---------------------------------------------------------------------------------------------- the float64 facts, by morph_ref alone
def test_weights_at_the_end_points():
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal((2, 3, 50)).astype(np.float32)
    st = morph_ref.stats(a, b)
    assert not morph_ref.falls_back(st).any()
    for mode in ("slerp", "lerp"):
        w = morph_ref.weights(st, (0.0, 1.0), mode)
        assert (w[0] == (1.0, 0.0)).all() and (w[1] == (0.0, 1.0)).all()
    mid = morph_ref.weights(st, (0.5,))[0]
    assert np.allclose(mid[:, 0], mid[:, 1], rtol=1e-15) and (mid[:, 0] > 0.5).all()      # the half-way point is pushed out to the sphere


def test_on_orthonormal_rows_every_frame_has_unit_norm():
    a, b = np.zeros((1, 8), np.float32), np.zeros((1, 8), np.float32)
    a[0, 2], b[0, 5] = 1.0, 1.0
    st = morph_ref.stats(a, b)
    assert (st == [[1.0, 0.0, 1.0]]).all() and abs(morph_ref.angles(st)[0] - math.pi / 2) < 1e-15
    fr = morph_ref.fractions(33)
    w = morph_ref.weights(st, fr)[:, 0]
    # 16 * 2^-53: the two angles (1 - t)*theta and t*theta miss pi / 2 by a few 2^-53 between them (1 - t, two products, theta itself),
    # and two sines, two squares and a sum round once each - each part at most about 4 * 2^-53 of a value that is at most 1
    assert (np.abs(w[:, 0] ** 2 + w[:, 1] ** 2 - 1.0) <= 16 * 2.0 ** -53).all()
    lerp = morph_ref.weights(st, fr, "lerp")[:, 0]
    assert abs(np.hypot(*lerp[16]) - math.sqrt(0.5)) < 1e-15                              # the linear mix loses 29 % of the norm half-way


def test_the_fallback_classes_take_the_lerp_weights():
    rng = np.random.default_rng(1)
    a = rng.standard_normal((1, 40)).astype(np.float32)
    fr = (0.0, 0.3, 1.0)
    for b in (a, 2 * a, -a):
        st = morph_ref.stats(a, b)
        assert morph_ref.falls_back(st).all()
        assert np.array_equal(morph_ref.weights(st, fr), morph_ref.weights(st, fr, "lerp"))
    for p, q in ((np.zeros_like(a), a), (a, np.zeros_like(a))):
        st = morph_ref.stats(p, q)
        assert morph_ref.falls_back(st).all() and np.array_equal(morph_ref.weights(st, fr)[1], [[0.7, 0.3]])
    # just outside: an angle of 2e-3 has 1 - cos = 2e-6 > 2^-20 and is slerped; 1e-3 has 5e-7 < 2^-20 and is not
    for ang, fb in ((2e-3, False), (1e-3, True)):
        st = np.array([[1.0, math.cos(ang), 1.0]])
        assert morph_ref.falls_back(st)[0] == fb
    assert np.array_equal(morph_ref.frames(a, -a, np.float32([[[0.5, 0.5]]])), np.zeros((1, 1, 40), np.float32))


def test_frames_copy_the_end_points_bit_for_bit():
    a = np.array([[-0.0, 1e-40, 3.0]], np.float32)
    b = np.array([[np.inf, 2.0, -0.0]], np.float32)
    w = np.float32([[[1.0, 0.0]], [[0.0, 1.0]]])
    with np.errstate(invalid="ignore"):
        plain, sel = morph_ref.frames(a, b, w), morph_ref.frames(a, b, w, (0.0, 1.0))
    assert np.array_equal(sel[0].view(np.uint32), a.view(np.uint32)) and np.array_equal(sel[1].view(np.uint32), b.view(np.uint32))
    assert np.isnan(plain[0, 0, 0]) and not np.signbit(plain[1, 0, 2])                    # what arithmetic would have made of them


# ---------------------------------------------------------------------------------------------- the host side of the samplers
@pytest.mark.parametrize("ease", ["linear", "cosine"])
def test_morph_fractions_are_the_restatement(ease):
    from polyffusion_amd.sampler import morph_fractions
    for n in (1, 2, 3, 5, 9, 64):
        got = morph_fractions(n, ease)
        assert got.dtype == np.float64 and np.array_equal(got, morph_ref.fractions(n, ease))
        assert (np.diff(got) > 0).all() and (n == 1 or (got[0] == 0.0 and got[-1] == 1.0))
    assert morph_fractions(1, ease).tolist() == [0.5]
    for bad in (0, 65):
        with pytest.raises(ValueError, match="frames"):
            morph_fractions(bad, ease)
    with pytest.raises(ValueError, match="ease"):
        morph_fractions(5, "cubic")


def test_morph_from_noise_refuses_loops_that_draw_noise(lib):
    from polyffusion_amd.sampler import DDIMSampler, DPMSolverSampler, SDFSampler
    c = torch.zeros(1, 1, 4)
    with pytest.raises(ValueError, match="morph_from_noise.*draws noise"):
        SDFSampler(Schedule()).morph_from_noise((1, 2, 4, 4), c, c, 3)
    with pytest.raises(ValueError, match="morph_from_noise.*stochastic"):
        DDIMSampler(Schedule(), 10, "uniform", 0.5).morph_from_noise((1, 2, 4, 4), c, c, 3)
    assert DDIMSampler(Schedule(), 10, "uniform", 0.0)._morph_refusal() is None
    assert DPMSolverSampler(Schedule(), 10)._morph_refusal() is None
    assert not hasattr(SDFSampler, "morph") and not hasattr(DPMSolverSampler, "morph")
    # morph itself: eta != 0 is invert's refusal, bad frame counts are morph_fractions'
    x = torch.zeros(1, 2, 4, 4)
    with pytest.raises(ValueError, match="stochastic"):
        DDIMSampler(Schedule(), 10, "uniform", 0.5).morph(x, c, x, c, 3)
    with pytest.raises(ValueError, match="frames"):
        DDIMSampler(Schedule(), 10).morph(x, c, x, c, 65)
    with pytest.raises(ValueError, match="shapes"):
        DDIMSampler(Schedule(), 10).morph(x, c, torch.zeros(2, 2, 4, 4), c, 3)
    with pytest.raises(ValueError, match="how"):
        DDIMSampler(Schedule(), 10).morph_cond(c, c, (0.0, 1.0), "nearest")


# ---------------------------------------------------------------------------------------------- the CLI
@pytest.fixture()
def npz(tmp_path):
    full, other, chords_only = tmp_path / "a.npz", tmp_path / "b.npz", tmp_path / "chords.npz"
    for f in (full, other):
        np.savez(f, chord=np.zeros((1, 32, 36), np.float32), prmat2c=np.zeros((1, 2, 128, 128), np.float32))
    np.savez(chords_only, chord=np.zeros((1, 32, 36), np.float32))
    return str(full), str(other), str(chords_only)


def test_parser_defaults_and_flags():
    from polyffusion_amd import inference_sdf
    p = inference_sdf.make_parser()
    a = p.parse_args([])
    assert (a.morph, a.morph_frames, a.morph_ease, a.morph_iters, a.morph_depth, a.morph_cond, a.morph_to_midi, a.morph_to_song_index,
            a.morph_to_npz) == (False, 5, "linear", 3, None, "lerp", None, None, None)
    a = p.parse_args(["--morph", "--morph_frames", "9", "--morph_ease", "cosine", "--morph_iters", "5", "--morph_depth", "7", "--morph_cond",
                      "switch", "--morph_to_song_index", "3"])
    assert (a.morph, a.morph_frames, a.morph_ease, a.morph_iters, a.morph_depth, a.morph_cond, a.morph_to_song_index) == \
        (True, 9, "cosine", 5, 7, "switch", 3)
    for bad in (["--morph_ease", "cubic"], ["--morph_cond", "nearest"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_cli_refusals_come_before_any_weight_is_loaded(npz):
    from polyffusion_amd import inference_sdf
    full, other, chords_only = npz
    p = inference_sdf.make_parser()
    good = ["--morph", "--ddim", "--cond_npz", full, "--morph_to_npz", other]
    synth = ["--morph", "--ddim", "--synthetic"]
    check = inference_sdf.check_morph_args
    assert check(p.parse_args(good), "chord", 1) is True and check(p.parse_args(good), "chord+txt", 1) is True
    assert check(p.parse_args(synth), "chord", 1) is True and check(p.parse_args(synth), "txt", 1) is True
    assert check(p.parse_args(["--morph", "--dpm", "--synthetic"]), "chord", 1) is True
    assert check(p.parse_args(good + ["--joint", "--hip_graph", "--uncond_scale", "3", "--score"]), "chord", 1) is True
    assert check(p.parse_args([]), "txt", 4) is False

    def refused(pattern, argv, cond_type="chord", world=1):
        with pytest.raises(SystemExit, match=pattern):
            check(p.parse_args(argv), cond_type, world)

    without = lambda *flags: [v for v in good if v not in flags]
    refused("needs --ddim", without("--ddim"))
    refused("--dpm and a song image", without("--ddim") + ["--dpm"])
    refused("--ddim_eta 0", good + ["--ddim_eta", "0.5"])
    refused("--autoreg", good + ["--autoreg"])
    refused("--inpaint_type", good + ["--inpaint_type", "below"])
    refused("--edit", good + ["--edit", "--edit_chord_shift", "2"])
    refused("--best_of", good + ["--best_of", "2"])
    refused("--num_generate", good + ["--num_generate", "2"])
    refused("one rank", good, world=2)
    refused("exactly one of", ["--morph", "--ddim", "--cond_npz", full])
    refused("exactly one of", good + ["--morph_to_midi", "b.mid"])
    refused("--from_dataset", ["--morph", "--ddim", "--cond_npz", full, "--morph_to_song_index", "1"])
    refused("song A's image", ["--morph", "--ddim", "--cond_npz", chords_only, "--morph_to_npz", other])
    refused("needs song A", ["--morph", "--ddim"])
    refused("with --synthetic", synth + ["--morph_to_npz", other])
    refused("cond_type chord or chord\\+txt", good, "txt")
    for k in (1, 65):
        refused("--morph_frames", good + ["--morph_frames", str(k)])
    refused("--morph_iters", good + ["--morph_iters", "0"])
    refused("--morph_depth", good + ["--morph_depth", "50"])
    refused("--morph_depth", ["--morph", "--dpm", "--synthetic", "--morph_depth", "20"])
    for flag in (["--morph_frames", "7"], ["--morph_ease", "cosine"], ["--morph_iters", "2"], ["--morph_depth", "1"], ["--morph_cond", "switch"],
                 ["--morph_to_midi", "b.mid"], ["--morph_to_song_index", "0"], ["--morph_to_npz", other]):
        refused("belong to --morph", ["--ddim"] + flag)
    # through main(): what the flags alone decide is refused before the GPU, the parameters or the weights are looked at
    for pattern, argv in (("--ddim_eta 0", good + ["--ddim_eta", "1"]), ("--autoreg", good + ["--autoreg"]), ("needs --ddim", without("--ddim")),
                          ("exactly one of", without("--morph_to_npz", other)), ("belong to --morph", ["--ddim", "--synthetic", "--morph_frames", "3"])):
        with pytest.raises(SystemExit, match=pattern):
            inference_sdf.main(argv + ["--params_preset", "sdf_chd8bar", "--synthetic_weights"])
