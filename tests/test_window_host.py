"""Joint overlapping-window sampling without a GPU: ``pf_window_split`` / ``pf_window_merge`` are declared, exported by both builds and
bound, the argument struct is laid out as the header says, every bad call is refused before any launch; ``WindowPlan``'s arithmetic against
the restatement in ``tests/window_ref.py``; the CLI flags; and ``Experiments.predict_joint``'s window-to-condition order and canvas
stitching, seen by a stub sampler that records what it is given."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import window_ref
from polyffusion_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000         # non-null, 16-byte aligned addresses that a refused call never touches (far enough apart not to overlap)
FAKE2 = 0x4000000
FAKE3 = 0x8000000


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from polyffusion_amd.build import build
        build(verbose=False)
    return _lib.load()


def test_header_declares_both_builds_export_and_the_binding_knows_the_entry_points(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "pfhip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pf_[a-z0-9_]+)\s*\(", hdr))
    if not os.path.exists(_lib.lib_path("f16")):
        from polyffusion_amd.build import build
        build(verbose=False, variant="f16")
    for name in ("pf_window_split", "pf_window_merge"):
        assert name in declared and name in _lib.SIGNATURES
        assert hasattr(lib, name) and hasattr(_lib.load("f16"), name)
    assert "pf_window_merge_args" in hdr


def test_the_argument_struct_is_laid_out_as_the_header_says():
    hdr = open(os.path.join(REPO, "include", "pfhip.h")).read()
    body = re.search(r"typedef struct pf_window_merge_args \{(.*?)\} pf_window_merge_args;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = re.findall(r"(const float\s*\*|float\s*\*|int|float)\s*([^;]+);", body)
    order = [(kind.replace(" ", ""), n.strip()) for kind, names in decls for n in names.split(",")]
    ctype = {"constfloat*": C.c_void_p, "float*": C.c_void_p, "int": C.c_int, "float": C.c_float}
    assert [(n, ctype[k]) for k, n in order] == list(_lib.WindowMergeArgs._fields_)
    f = _lib.WindowMergeArgs
    names = [n for n, _ in f._fields_]
    assert names == ["eps", "row_weight", "groups", "s1", "s2", "songs", "channels", "win_h", "width", "n_windows", "stride", "out"]
    assert [getattr(f, n).offset for n in names] == [0, 8, 16, 20, 24, 28, 32, 36, 40, 44, 48, 56] and C.sizeof(f) == 64
    # pf_window_split: two pointers, six ints in the geometry's order, the stream
    sig = re.search(r"int pf_window_split\(([^)]*)\)", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)).group(1)
    assert [a.split()[-1].strip("*") for a in sig.split(",")] == ["canvas", "windows", "songs", "channels", "win_h", "width", "n_windows", "stride", "stream"]
    assert _lib.SIGNATURES["pf_window_split"] == (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p])


GEOM = dict(songs=2, channels=2, win_h=8, width=4, n_windows=3, stride=4)
BAD_GEOMETRY = [
    (r"stride 0 < 1", dict(stride=0)),
    (r"stride -3 < 1", dict(stride=-3)),
    (r"stride 9 > win_h 8", dict(stride=9)),
    (r"at most 8", dict(win_h=9, stride=1)),                # ceil(9 / 1) = 9 windows over a row
    (r"at most 8", dict(win_h=17, stride=2)),               # ceil(17 / 2) = 9
    (r"non-positive extent", dict(songs=0)),
    (r"non-positive extent", dict(channels=0)),
    (r"non-positive extent", dict(win_h=0)),
    (r"non-positive extent", dict(width=-1)),
    (r"non-positive extent", dict(n_windows=0)),
]


def test_split_refuses_bad_calls_before_any_launch(lib):
    """No GPU needed: the call returns before it touches HIP or any of the (fake) pointers."""
    def refused(pattern, canvas=FAKE, windows=FAKE2, **geom):
        g = dict(GEOM, **geom)
        rc = lib.pf_window_split(canvas, windows, g["songs"], g["channels"], g["win_h"], g["width"], g["n_windows"], g["stride"], None)
        msg = lib.pf_last_error().decode()
        assert rc < 0 and msg.startswith("window_split: ") and re.search(pattern, msg), (geom, rc, msg)

    for pattern, geom in BAD_GEOMETRY:
        refused(pattern, **geom)
    refused("null pointer", canvas=None)
    refused("null pointer", windows=None)
    refused("aliases", windows=FAKE)                                         # the same buffer
    refused("aliases", windows=FAKE + 16)                                    # inside the canvas
    n_win = 2 * 3 * 2 * 8 * 4 * 4                                            # bytes of the windows
    refused("aliases", windows=FAKE, canvas=FAKE + n_win - 4)                # the canvas begins in the windows' last float
    assert lib.pf_window_split(FAKE + n_win, FAKE, 0, 2, 8, 4, 3, 4, None) < 0 and "non-positive" in lib.pf_last_error().decode()
    # 8 windows over a row are the cap, not beyond it
    assert lib.pf_window_split(None, FAKE2, 1, 1, 8, 4, 7, 1, None) < 0 and "null pointer" in lib.pf_last_error().decode()


def test_merge_refuses_bad_calls_before_any_launch(lib):
    def refused(pattern, **fields):
        a = _lib.WindowMergeArgs()
        kw = dict(GEOM, eps=FAKE, row_weight=FAKE2, out=FAKE3, groups=1)
        kw.update(fields)
        for k, v in kw.items():
            setattr(a, k, v)
        rc = lib.pf_window_merge(C.byref(a), None)
        msg = lib.pf_last_error().decode()
        assert rc < 0 and msg.startswith("window_merge: ") and re.search(pattern, msg), (fields, rc, msg)

    for pattern, geom in BAD_GEOMETRY:
        refused(pattern, **geom)
    for field in ("eps", "row_weight", "out"):
        refused("null pointer", **{field: None})
    for groups in (0, 4, -1):
        refused("groups", groups=groups)
    refused("aliases", out=FAKE)
    refused("aliases", out=FAKE2)                                            # the weights
    refused("aliases", out=FAKE2 + 28, groups=2)                             # the weights' last float
    one_group = 2 * 3 * 2 * 8 * 4 * 4
    refused("aliases", out=FAKE + 3 * one_group - 4, groups=3)               # inside the third group
    refused("aliases", eps=FAKE3 + 2 * 2 * 16 * 4 * 4 - 4)                   # eps begins in out's last float
    assert lib.pf_window_merge(None, None) < 0 and lib.pf_last_error().decode().startswith("window_merge: ")


# ---------------------------------------------------------------------------------------------- WindowPlan
PLANS = [(3, 4, 8), (4, 3, 8), (2, 8, 8), (5, 4, 16), (7, 1, 8), (4, 5, 12), (1, 8, 8), (15, 64, 128), (3, 16, 32)]


@pytest.mark.parametrize("n,stride,h", PLANS)
def test_plan_arithmetic(n, stride, h):
    from polyffusion_amd.sampler import MAX_COVER, WindowPlan
    p = WindowPlan(n, stride, h)
    assert p.canvas_h == window_ref.canvas_h(n, stride, h) and MAX_COVER == window_ref.MAX_COVER == 8
    ks = []
    for y in range(p.canvas_h):                     # every row: first, last and every seam among them
        assert p.cover(y) == window_ref.cover(y, n, stride, h), y
        ks.append(len(p.cover(y)))
    assert 1 <= min(ks) and max(ks) <= 8 and max(ks) == min(n, -(-h // stride))
    assert p.cover(0) == [0] and p.cover(p.canvas_h - 1) == [n - 1]
    for y in (-1, p.canvas_h):
        with pytest.raises(IndexError):
            p.cover(y)
    for blend in window_ref.BLENDS:
        q = WindowPlan(n, stride, h, blend)
        w = q.weights()
        assert w.dtype == np.float32 and w.shape == (h,) and (w > 0).all() and (w <= 1).all()
        assert np.array_equal(w, window_ref.weights(h, stride, blend))
        assert q.key == (n, stride, h, blend) and hash(q) == hash(WindowPlan(n, stride, h, blend)) and q == WindowPlan(n, stride, h, blend)
    assert (WindowPlan(n, stride, h, "mean").weights() == 1).all()
    assert WindowPlan(n, stride, h, "mean").key != WindowPlan(n, stride, h, "ramp").key
    if stride == h:
        assert (WindowPlan(n, stride, h, "ramp").weights() == 1).all()


@pytest.mark.parametrize("h", [8, 32, 128])
def test_the_ramp_is_a_partition_of_unity_at_half_stride(h):
    from polyffusion_amd.sampler import WindowPlan
    p = WindowPlan(5, h // 2, h, "ramp")
    w = p.weights()
    for y in range(h // 2, p.canvas_h - h // 2):              # every row two windows share
        j0, j1 = p.cover(y)
        assert np.float32(w[y - j0 * p.stride] + w[y - j1 * p.stride]) == np.float32(1.0)
        assert float(w[y - j0 * p.stride]) + float(w[y - j1 * p.stride]) == 1.0       # exactly, not only after rounding
    assert np.array_equal(w, w[::-1]) and w[0] == np.float32(0.5 / (h // 2))


@pytest.mark.parametrize("bad", [(0, 4, 8), (3, 0, 8), (3, -1, 8), (3, 9, 8), (3, 1, 9), (3, 2, 17), (3, 4, 0)])
def test_bad_plans_are_refused(bad):
    from polyffusion_amd.sampler import WindowPlan
    assert not window_ref.valid(*bad)
    with pytest.raises(ValueError):
        WindowPlan(*bad)


def test_a_bad_blend_is_refused_and_the_samplers_take_the_keyword(lib):
    from polyffusion_amd.sampler import DDIMSampler, DPMSolverSampler, SDFSampler, WindowPlan
    import dpm_ref
    with pytest.raises(ValueError):
        WindowPlan(3, 4, 8, "cosine")
    assert all(window_ref.valid(*p) for p in PLANS)

    class Schedule:
        n_steps = 1000
        alpha_bar = torch.from_numpy(dpm_ref.alpha_bar().astype(np.float32))
        beta = torch.full((1000,), 0.01)
        eps_model = None

    plan = WindowPlan(3, 16, 32)
    for make in (lambda **kw: SDFSampler(Schedule(), **kw), lambda **kw: DDIMSampler(Schedule(), 20, **kw), lambda **kw: DPMSolverSampler(Schedule(), 10, **kw)):
        assert make().windows is None and make(windows=plan).windows is plan
        assert make(windows=plan)._eps_rows(torch.empty(2, 1, 64, 4)) == 6 and make()._eps_rows(torch.empty(2, 1, 64, 4)) == 2


# ---------------------------------------------------------------------------------------------- the CLI's flags
def test_parser():
    from polyffusion_amd import inference_sdf
    p = inference_sdf.make_parser()
    a = p.parse_args([])
    assert (a.joint, a.joint_blend, a.autoreg) == (False, "mean", False)
    a = p.parse_args(["--joint", "--joint_blend", "ramp", "--ddim", "--hip_graph", "--uncond_scale", "2.5", "--num_generate", "2"])
    assert (a.joint, a.joint_blend, a.autoreg, a.ddim, a.hip_graph) == (True, "ramp", False, True, True)
    assert p.parse_args(["--autoreg"]).autoreg and not p.parse_args(["--autoreg"]).joint
    with pytest.raises(SystemExit):
        p.parse_args(["--joint_blend", "cosine"])
    for pair in (["--joint", "--autoreg"], ["--autoreg", "--joint"]):
        with pytest.raises(SystemExit) as e:
            p.parse_args(pair)
        assert e.value.code == 2                                   # an argparse error, before anything is loaded
        with pytest.raises(SystemExit) as e:
            inference_sdf.main(pair + ["--synthetic_weights", "--synthetic"])
        assert e.value.code == 2


# ---------------------------------------------------------------------------------------------- predict_joint
class StubSampler:
    """Records what ``predict_joint`` hands to the sampler; ``paint`` returns the noise canvas it was given as ``orig_noise``."""

    def __init__(self):
        self.windows = None
        self.calls = []

    def randn(self, shape, device):
        self.drawn = tuple(shape)
        return torch.arange(int(np.prod(shape)), dtype=torch.float32).reshape(tuple(shape))

    def q_sample(self, orig, index, noise):
        self.q = (orig, index, noise)
        return noise + 0.5

    def paint(self, x, cond, t_start, **kw):
        self.calls.append(dict(kw, x=x, cond=cond, t_start=t_start, windows=self.windows))
        return kw["orig_noise"]


def experiments(stub):
    from polyffusion_amd import inference_sdf
    from polyffusion_amd.params import preset
    return inference_sdf.Experiments("label", preset("sdf_chd8bar"), stub, t_idx=7, repaint_n=1)


def test_predict_joint_orders_the_conditions_and_stitches_the_canvases():
    from polyffusion_amd.sampler import WindowPlan
    S, B, H, W, D = 2, 3, 128, 128, 512
    cond = torch.zeros(S, B, 1, D)
    cond_mid = torch.zeros(S, B, 1, D)
    for s in range(S):
        for b in range(B):
            cond[s, b] = 100 * s + 2 * b              # the aligned window 2b
            cond_mid[s, b] = 100 * s + 2 * b + 1      # the half-shifted window 2b + 1 (b = B - 1: the wrapped row, unused)
    tag = lambda: (torch.arange(S).view(S, 1, 1, 1, 1) * 1e6 + torch.arange(B).view(1, B, 1, 1, 1) * 1e5 + torch.arange(2).view(1, 1, 2, 1, 1) * 1e4
                   + torch.arange(H).view(1, 1, 1, H, 1) * 10 + (torch.arange(W).view(1, 1, 1, 1, W) % 10)).float()
    orig, mask, noise = tag(), (tag() % 2), tag() + 0.25
    stub = StubSampler()
    ex = experiments(stub)
    out = ex.predict_joint(cond, cond_mid, 2.5, orig, mask, None, noise, "ramp")
    assert stub.windows is None and len(stub.calls) == 1                     # the plan is set for the call and taken back
    call = stub.calls[0]
    plan = call["windows"]
    assert plan == WindowPlan(2 * B - 1, 64, 128, "ramp") and plan.canvas_h == B * H
    assert call["t_start"] == 7 and call["uncond_scale"] == 2.5 and call["repaint_n"] == 1 and call["cond_concat"] is None
    Wn = 2 * B - 1
    assert call["cond"].shape == (S * Wn, 1, D) and call["uncond_cond"].shape == (S * Wn, 1, D) and (call["uncond_cond"] == -1).all()
    for s in range(S):
        for w in range(Wn):
            assert (call["cond"][s * Wn + w] == 100 * s + w).all(), (s, w)
    canvas = lambda v: torch.cat([v[:, b] for b in range(B)], dim=2)          # segments one after the other along the time axis
    for name, src in (("orig", orig), ("mask", mask), ("orig_noise", noise)):
        assert call[name].shape == (S, 2, B * H, W) and call[name].is_contiguous() and torch.equal(call[name], canvas(src)), name
    assert stub.q[1] == 7 and torch.equal(stub.q[0], canvas(orig)) and torch.equal(stub.q[2], canvas(noise)) and torch.equal(call["x"], canvas(noise) + 0.5)
    assert out.shape == (S, B, 2, H, W) and torch.equal(out, noise)          # the canvas comes back cut into its segments


def test_predict_joint_defaults_one_segment_and_the_wrapper():
    from polyffusion_amd.sampler import WindowPlan
    S, B, D = 2, 2, 512
    stub = StubSampler()
    ex = experiments(stub)
    cond, cond_mid = torch.ones(S, B, 1, D), 2 * torch.ones(S, B, 1, D)
    cc = torch.rand(S, B, 1, 128, 128)
    out = ex.predict_joint(cond, cond_mid, cond_concat=cc)
    call = stub.calls[-1]
    assert stub.drawn == (S, 2, 256, 128) and call["windows"] == WindowPlan(3, 64, 128, "mean")
    assert (call["orig"] == 0).all() and (call["mask"] == 0).all() and call["orig"].shape == (S, 2, 256, 128)
    assert torch.equal(call["cond_concat"], torch.cat([cc[:, 0], cc[:, 1]], dim=2)) and out.shape == (S, B, 2, 128, 128)
    assert [float(v[0, 0]) for v in call["cond"]] == [1, 2, 1, 1, 2, 1]
    with pytest.raises(ValueError):
        ex.predict_joint(cond, None)
    # one segment: one window, no cond_mid needed
    ex.predict_joint(cond[:, :1], None)
    assert stub.calls[-1]["windows"] == WindowPlan(1, 64, 128) and stub.calls[-1]["cond"].shape == (S, 1, D)
    # predict(joint=True): one song
    out = ex.predict(cond[0], cond_mid[0], 1.0, joint=True, blend="ramp")
    assert out.shape == (B, 2, 128, 128) and stub.calls[-1]["windows"] == WindowPlan(3, 64, 128, "ramp") and stub.calls[-1]["cond"].shape == (3, 1, D)
    with pytest.raises(ValueError):
        ex.predict(cond[0], cond_mid[0], 1.0, True, joint=True)
    assert ",joint]" in ex._stamp(1.0, False, joint="mean") and ",joint-ramp]" in ex._stamp(1.0, False, joint="ramp")
    assert "joint" not in ex._stamp(1.0, False) and ",autoreg]" in ex._stamp(1.0, True)
