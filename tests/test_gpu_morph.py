"""A path between two songs on the GPU (-m gpu): ``pf_slerp_rows`` against the float64 restatement in ``tests/morph_ref.py`` - its three
sums, its weights, its frames bit for bit, what it must not touch, mode lerp, independence of how the rows are split into calls, vector
and element-by-element path; ``DDIMSampler.morph`` on the closed-form Gaussian denoiser against the float64 loops of ``invert_ref`` and
on a small synthetic UNet (its parts called directly, eager == captured graph, batches, window plans, dual guidance,
``morph_from_noise``), and the CLI.

Bounds.  Sums: the device adds ``row_elems`` exact float64 products in a fixed order, so each sum is within the recursive-summation bound
``row_elems * 2^-53 * sum |term|`` of the exactly rounded ``math.fsum`` value (checked on the CPU for every shape of the matrix: a plain
sequential float64 sum stays within it).  Weights: formed in float64 from the DEVICE's sums by both sides, then rounded to float32 once;
what remains between the two libms is ~1e-15 relative and can only move a value across a rounding boundary: 1 float32 ulp, and bit-equal
where no libm is involved (fallback rows, t = 0 and t = 1).  Frames: two float32 products and a float32 sum
with the device's own weights: bit-equal.  No test asserts anything about the quality of a morph on a UNet."""
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ctypes as C  # noqa: E402

import dpm_ref  # noqa: E402
import invert_ref  # noqa: E402
import morph_ref  # noqa: E402
from polyffusion_amd import _lib, _steps  # noqa: E402
from polyffusion_amd.arch import UNetConfig  # noqa: E402
from polyffusion_amd.sampler import DDIMSampler, DPMSolverSampler, DualScale, WindowPlan, morph_fractions  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AB = dpm_ref.alpha_bar()
CHUNK = _lib.MSE_CHUNK
PAD = 8                 # elements of sentinel on either side of a buffer (32 or 64 bytes: the payload keeps its 16-byte alignment)
SENTINEL = -777.25
U53 = 2.0 ** -53
ROW_ELEMS = [1, 3, 2047, 2048, 2049, 4100, 32768]
PHIS = (0.3, math.pi / 2, 2.8)
CLASSES = tuple(f"phi{i}" for i in range(len(PHIS))) + ("gauss", "same", "double", "minus", "zero")


def fracs_of(frames):
    """The fraction sets of a frame count, each holding 0 and 1 where it can: one frame cannot, so it is run at 0, at 1 and inside."""
    if frames == 1:
        return [(0.0,), (1.0,), (0.5,)]
    if frames == 2:
        return [(0.0, 1.0)]
    if frames == 5:
        return [(0.0, 0.25, 1.0, 0.6, 0.5)]
    return [tuple(np.linspace(0.0, 1.0, frames))]


@pytest.fixture(scope="module")
def lib():
    _lib.require_gpu()
    return _lib.load()


@functools.lru_cache(maxsize=None)
def inputs(n, cls):
    """(a, b) float32 ``[3, n]`` of one input class (read-only; shared by every test that needs them).  From 3 elements up row 0 of ``a``
    carries a negative zero and a denormal; they are planted before ``b`` is built, so the angles hold."""
    rng = np.random.default_rng(1000 * n + CLASSES.index(cls))
    a = rng.standard_normal((3, n)).astype(np.float32)
    if n >= 3:
        a[0, 0], a[0, 1] = -0.0, 1e-40
    g = rng.standard_normal((3, n))
    if cls.startswith("phi"):
        phi, a64 = PHIS[int(cls[3:])], a.astype(np.float64)
        if n == 1:               # no second direction: the rows are parallel or antiparallel whatever the angle asked for
            b = 1.3 * math.cos(phi) * a64
        else:                    # Gram-Schmidt in float64: u orthogonal to a, then b at the angle phi in the plane of the two
            u = g - (np.sum(g * a64, axis=1) / np.sum(a64 * a64, axis=1))[:, None] * a64
            na, nu = np.linalg.norm(a64, axis=1)[:, None], np.linalg.norm(u, axis=1)[:, None]
            b = 1.3 * na * (math.cos(phi) * a64 / na + math.sin(phi) * u / nu)
        b = b.astype(np.float32)
    elif cls == "gauss":
        b = g.astype(np.float32)
    elif cls == "same":
        b = a.copy()
    elif cls == "double":
        b = (2 * a).astype(np.float32)
    elif cls == "minus":
        b = (-a).astype(np.float32)
    else:
        b, a = g.astype(np.float32), np.zeros_like(a)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def host_stats(n, cls, rows):
    a, b = inputs(n, cls)
    return morph_ref.stats(a[:rows], b[:rows]), morph_ref.abs_terms(a[:rows], b[:rows])


def padded(values, off=0, dtype=torch.float32):
    """(whole buffer, payload view) on the device: the payload starts `off` elements past a 16-byte boundary, sentinels around it."""
    values = np.asarray(values).reshape(-1)
    n = len(values)
    whole = torch.full((n + 2 * PAD + 4,), SENTINEL, device="cuda", dtype=dtype)
    view = whole[PAD + off: PAD + off + n]
    view.copy_(torch.from_numpy(values.astype(np.float32 if dtype == torch.float32 else np.float64)))
    return whole, view


def untouched(whole, view_len, off=0):
    w = whole.cpu().numpy()
    return (w[: PAD + off] == SENTINEL).all() and (w[PAD + off + view_len:] == SENTINEL).all()


def run(lib, a, b, fracs, mode="slerp", off=0):
    """One call on the rows of the host arrays ``a`` / ``b`` ``[rows, n]``, every buffer between sentinels and ``off`` floats past a 16-byte
    boundary; returns (out [K, rows, n], stats [rows, 3] or None, weights [K, rows, 2]) as numpy after checking the sentinels and that
    the inputs are unchanged.  Fills the argument struct itself: the buffers of ``_steps.slerp_rows`` have no sentinels."""
    rows, n = a.shape
    K = len(fracs)
    aw, av = padded(a, off)
    bw, bv = padded(b, off)
    ow, ov = padded(np.zeros(K * rows * n, np.float32), off)
    ww, wv = padded(np.full(K * rows * 2, SENTINEL, np.float32))
    args = _lib.SlerpArgs()
    t = (C.c_double * K)(*fracs)
    args.a, args.b, args.t, args.out, args.weights = av.data_ptr(), bv.data_ptr(), C.addressof(t), ov.data_ptr(), wv.data_ptr()
    args.mode, args.frames, args.rows, args.row_elems = _lib.SLERP_MODES[mode], K, rows, n
    nb = int(lib.pf_slerp_rows_workspace_bytes(rows, n))
    assert nb == rows * -(-n // CHUNK) * 24
    if mode == "slerp":
        sw, sv = padded(np.full(rows * 3, SENTINEL), 0, torch.float64)
        kw, kv = padded(np.full(nb // 8, SENTINEL), 0, torch.float64)
        args.stats, args.workspace, args.workspace_bytes = sv.data_ptr(), kv.data_ptr(), nb
    _lib.check(lib.pf_slerp_rows(C.byref(args), _lib.current_stream()), "pf_slerp_rows", lib)
    torch.cuda.synchronize()
    assert untouched(ow, K * rows * n, off) and untouched(ww, K * rows * 2)
    assert untouched(aw, rows * n, off) and untouched(bw, rows * n, off)
    assert np.array_equal(av.cpu().numpy().view(np.uint32), a.reshape(-1).view(np.uint32))
    assert np.array_equal(bv.cpu().numpy().view(np.uint32), b.reshape(-1).view(np.uint32))
    st = None
    if mode == "slerp":
        assert untouched(sw, rows * 3) and untouched(kw, nb // 8)
        st = sv.cpu().numpy().reshape(rows, 3)
        assert (kv.cpu().numpy() != SENTINEL).all()                          # every partial triple was written
    return ov.cpu().numpy().reshape(K, rows, n), st, wv.cpu().numpy().reshape(K, rows, 2)


def bits(v):
    return np.ascontiguousarray(v).view(np.uint32 if v.dtype == np.float32 else np.uint64)


def expected_fallback(n, cls):
    return n == 1 or cls in ("same", "double", "minus", "zero")


# ---------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("frames", [1, 2, 5, 64])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n", ROW_ELEMS)
def test_sums_weights_and_frames_on_every_input_class(lib, n, rows, frames):
    worst = 0.0
    for cls in CLASSES:
        a, b = (v[:rows] for v in inputs(n, cls))
        want_st, abs_st = host_stats(n, cls, rows)
        # the class, by the restatement, before the matrix is trusted
        fb = morph_ref.falls_back(want_st)
        assert (fb == expected_fallback(n, cls)).all(), (cls, n, fb)
        if cls.startswith("phi") and n > 1:
            assert (np.abs(morph_ref.angles(want_st) - PHIS[int(cls[3:])]) <= 1e-3).all(), (cls, morph_ref.angles(want_st))
        for fr in fracs_of(frames):
            out, st, w = run(lib, a, b, fr)
            # 1. the sums
            err = np.abs(st - want_st)
            assert (err <= n * U53 * abs_st).all(), (cls, fr, st, want_st)
            with np.errstate(divide="ignore", invalid="ignore"):
                worst = max(worst, float(np.nanmax(np.where(abs_st > 0, err / (n * U53 * abs_st), 0.0))))
            # 2. the weights, from the device's own sums
            want_w = morph_ref.weights(st, fr).astype(np.float32)
            exact = np.zeros(w.shape[:2], dtype=bool)
            exact[:, morph_ref.falls_back(st)] = True
            exact[np.array([t in (0.0, 1.0) for t in fr], dtype=bool)] = True
            assert (morph_ref.falls_back(st) == fb).all()
            assert np.array_equal(bits(w[exact]), bits(want_w[exact])), (cls, fr)
            assert (np.abs(w.astype(np.float64) - want_w.astype(np.float64)) <= np.spacing(np.abs(want_w)).astype(np.float64)).all(), (cls, fr, w, want_w)
            for k, t in enumerate(fr):
                if t in (0.0, 1.0):
                    assert (w[k] == ((1.0, 0.0) if t == 0.0 else (0.0, 1.0))).all()
            # 3. the frames, with the device's weights
            assert np.array_equal(bits(out), bits(morph_ref.frames(a, b, w, fr))), (cls, fr)
            for k, t in enumerate(fr):
                if t in (0.0, 1.0):
                    assert np.array_equal(bits(out[k]), bits(a if t == 0.0 else b)), (cls, k)
    print(f"n={n} rows={rows} frames={frames}: largest sum error / bound {worst:.3f}")


@pytest.mark.parametrize("n", ROW_ELEMS)
def test_a_plain_sequential_float64_sum_stays_within_the_bound_of_the_sums(n):
    """The CPU side of check 1: the bound holds for the plainest order there is."""
    for cls in CLASSES:
        a, b = inputs(n, cls)
        want, abs_st = host_stats(n, cls, 3)
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        for r in range(3):
            got = [0.0, 0.0, 0.0]
            for p, q in zip(a64[r].tolist(), b64[r].tolist()):
                got[0] += p * p
                got[1] += p * q
                got[2] += q * q
            assert (np.abs(np.array(got) - want[r]) <= n * U53 * abs_st[r]).all()


@pytest.mark.parametrize("n", [3, 2049, 4100])
def test_mode_lerp_needs_no_workspace_and_is_the_restatement_bit_for_bit(lib, n):
    fr = (0.0, 0.3, 0.5, 1.0, 0.9)
    for cls in ("gauss", "minus", "zero"):
        a, b = inputs(n, cls)
        out, st, w = run(lib, a, b, fr, mode="lerp")
        assert st is None
        want_w = np.array([[(np.float32(1.0 - t), np.float32(t))] * 3 for t in fr], dtype=np.float32)
        assert np.array_equal(bits(w), bits(want_w))
        assert np.array_equal(bits(out), bits(morph_ref.frames(a, b, want_w, fr)))
        assert np.array_equal(bits(out[0]), bits(a)) and np.array_equal(bits(out[3]), bits(b))


@pytest.mark.parametrize("n", ROW_ELEMS)
def test_a_row_does_not_depend_on_how_the_rows_are_split_into_calls(lib, n):
    fr = fracs_of(5)[0]
    for cls in ("phi1", "gauss", "double"):
        a, b = inputs(n, cls)
        out3, st3, w3 = run(lib, a, b, fr)
        for lo, hi in ((0, 1), (1, 3)):
            out, st, w = run(lib, a[lo:hi], b[lo:hi], fr)
            assert np.array_equal(bits(out), bits(out3[:, lo:hi])) and np.array_equal(bits(st), bits(st3[lo:hi]))
            assert np.array_equal(bits(w), bits(w3[:, lo:hi]))
        again = run(lib, a, b, fr)
        assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(again, (out3, st3, w3)))       # from call to call


@pytest.mark.parametrize("n", [2048, 4100, 2049])
def test_vector_and_scalar_paths_give_the_same_bits(lib, n):
    """n % 4 == 0 from an aligned base moves 16-byte vectors; the same values one float further on, or an n that is no multiple of 4
    (2049, from either base), move element by element."""
    fr = fracs_of(5)[0]
    for mode in ("slerp", "lerp"):
        a, b = inputs(n, "gauss")
        p, q = run(lib, a, b, fr, mode), run(lib, a, b, fr, mode, off=1)
        assert all(u is None or np.array_equal(bits(u), bits(v)) for u, v in zip(p, q))
    if n % 4 == 0:       # a row length that is no multiple of 4 is the same computation on the rows' first n - 1 elements
        a1, b1 = (np.ascontiguousarray(v[:, : n - 1]) for v in inputs(n, "gauss"))
        out, st, w = run(lib, a1, b1, fr)
        assert np.array_equal(bits(out), bits(morph_ref.frames(a1, b1, w, fr)))


def test_the_wrapper_makes_the_same_call(lib):
    a, b = inputs(4100, "phi0")
    fr = fracs_of(5)[0]
    out, st, w = run(lib, a, b, fr)
    o2, s2, w2 = _steps.slerp_rows(lib, torch.from_numpy(a.copy()).cuda(), torch.from_numpy(b.copy()).cuda(), fr)
    assert o2.shape == (5, 3, 4100) and s2.shape == (3, 3) and w2.shape == (5, 3, 2)
    assert np.array_equal(bits(o2.cpu().numpy()), bits(out)) and np.array_equal(bits(s2.cpu().numpy()), bits(st))
    assert np.array_equal(bits(w2.cpu().numpy()), bits(w))
    o3, s3, w3 = _steps.slerp_rows(lib, torch.from_numpy(a.copy()).cuda().view(3, 2, 2050), torch.from_numpy(b.copy()).cuda().view(3, 2, 2050), fr,
                                   want_stats=False)
    assert o3.shape == (5, 3, 2, 2050) and s3 is None and w3 is None and np.array_equal(bits(o3.cpu().numpy().reshape(5, 3, 4100)), bits(out))


# ---------------------------------------------------------------------------------------------- the loop on the analytic denoiser
class GaussianDenoiser:
    """Stands in for a LatentDiffusion: the optimal denoiser of data ~ N(0, s^2), eps = gain[t] * x as ONE float32 product on the device.
    Carries what the samplers touch: n_steps, alpha_bar, and an eps_model with the two prepare hooks."""

    def __init__(self, s):
        self.n_steps = 1000
        self.alpha_bar = torch.from_numpy(AB.astype(np.float32))
        self.eps_model = self
        self.gain32 = dpm_ref.gauss_gain(AB, np.arange(1000), s).astype(np.float32)
        self.gain = torch.from_numpy(self.gain32).cuda()

    def prepare_time(self, n, out=None):
        return None

    def prepare_cond(self, ctx, out=None):
        return None

    def __call__(self, x, t, c, time_table=None, cross_bias=None):
        return x * self.gain[t].view(-1, 1, 1, 1)


def ddim_rows_of(sd):
    """The sampler's own float32 DDIM coefficients (s1m, sqrt_a, sqrt_aprev, dir_coef) per index, as float64."""
    return np.array([[getattr(sd._coef(i), f) for f in ("s1m", "sqrt_a", "sqrt_aprev", "dir_coef")] for i in range(len(sd.time_steps))], dtype=np.float64)


@pytest.mark.parametrize("s", [1.0, 4.0])
def test_gauss_morph_stays_within_the_bound_of_the_float64_loops(lib, s):
    """Invert and paint are linear on this denoiser (elementwise factors), so frame k is w0 * paint(invert(A)) + w1 * paint(invert(B)) up to
    rounding.  Against the float64 loop from the mixed noise w0*x_a + w1*x_b (x_a, x_b: the float64 inversions; w: the device's float32
    weights) a float32 frame may differ by
        |w0| * bound_a + |w1| * bound_b           the round trips' own bounds (invert_ref: every rounding of both loops, carried through
                                                  paint); paint's roundings on the mix act on |mix| <= |w0 x_a| + |w1 x_b| at every step
      + 4 * 2^-24 * (|w0 p_a| + |w1 p_b|)         the slerp's two products and one sum (3 roundings of relative size 2^-24 on the two
                                                  terms, one to spare), carried down by paint's elementwise factors: p = paint(x)."""
    g = torch.Generator().manual_seed(5)
    xa, xb = torch.randn(2, 2, 8, 8, generator=g), torch.randn(2, 2, 8, 8, generator=g)
    cond = torch.zeros(2, 1, 4, device="cuda")
    m = GaussianDenoiser(s)
    sd = DDIMSampler(m, 10, "uniform", 0.0)
    t = len(sd.time_steps) - 1
    assert t == 9
    out = sd.morph(xa.cuda(), cond, xb.cuda(), cond, 5, iters=3)
    rec = sd.last_morph
    assert out.shape == (5, 2, 2, 8, 8) and rec.weights.shape == (5, 2, 2) and rec.stats.shape == (2, 3) and rec.inversion.shape == (10, 3, 4, 2)
    assert np.array_equal(rec.fractions, morph_ref.fractions(5)) and np.isfinite(rec.angles()).all()
    got, w = out.cpu().numpy(), rec.weights.cpu().numpy().astype(np.float64)
    R, D, gains = sd.invert_rows().astype(np.float64), ddim_rows_of(sd), m.gain32[sd.time_steps].astype(np.float64)
    ends = [invert_ref.invert_gauss_with_budget(R, gains, v.numpy(), 3)[:2] for v in (xa, xb)]
    (pa, ba), (pb, bb) = (invert_ref.paint_gauss_with_budget(D, gains, x, e) for x, e in ends)
    worst = 0.0
    for k in range(5):
        w0, w1 = (w[k, :, j].reshape(2, 1, 1, 1) for j in (0, 1))
        want = invert_ref.paint_gauss_with_budget(D, gains, w0 * ends[0][0] + w1 * ends[1][0])[0]
        bound = np.abs(w0) * ba + np.abs(w1) * bb + 4 * 2.0 ** -24 * (np.abs(w0 * pa) + np.abs(w1 * pb))
        err = np.abs(got[k] - want)
        worst = max(worst, float(np.max(err / bound)))
        assert (err <= bound).all(), (k, float(np.max(err / bound)))
    print(f"s={s}: max error / bound over the 5 frames {worst:.3f}; angles {rec.angles()}")
    # the end frames are the two songs' own round trips, bit for bit
    x = sd.invert(torch.cat([xa, xb]).cuda(), torch.cat([cond, cond]), iters=3)
    assert torch.equal(x[:2], rec.end_noises[0]) and torch.equal(x[2:], rec.end_noises[1])
    assert torch.equal(sd.paint(x[:2], cond, t), out[0]) and torch.equal(sd.paint(x[2:], cond, t), out[4])


# ---------------------------------------------------------------------------------------------- a small synthetic UNet
T = 5                   # 6 steps, grid indices 0 .. 5 (the CLI's t_idx = ddim_steps - 1)


@pytest.fixture(scope="module")
def ldm():
    from polyffusion_amd.unet import LatentDiffusion, UNetModel
    from polyffusion_amd.weights import synth_unet_state
    kw = dict(in_channels=2, out_channels=2, channels=32, n_res_blocks=1, attention_levels=(1,), channel_multipliers=(1, 2), n_heads=2,
              tf_layers=1, d_cond=32)
    m = UNetModel(img_h=16, img_w=16, **kw)
    m.load_state_dict(synth_unet_state(UNetConfig(**kw), 0))
    m.set_precision("bf16x3")
    return LatentDiffusion(m, None, 0.18215, 1000, 0.00085, 0.012)


def unet_inputs():
    g = torch.Generator().manual_seed(3)
    return tuple(torch.randn(*s, generator=g).cuda() for s in ((2, 2, 16, 16), (2, 1, 32), (2, 2, 16, 16), (2, 1, 32)))


def guidance(scale, rows=2):
    return dict(uncond_scale=scale, uncond_cond=-torch.ones(rows, 1, 32).cuda())


@pytest.mark.parametrize("scale", [1.0, 5.0])
def test_unet_morph_is_its_parts_called_directly(ldm, scale):
    xa, ca, xb, cb = unet_inputs()
    g = guidance(scale)
    sd = DDIMSampler(ldm, 6, "uniform", 0.0)
    out = sd.morph(xa, ca, xb, cb, 5, t_end=T, iters=2, **g)
    rec = sd.last_morph
    assert out.shape == (5, 2, 2, 16, 16) and torch.isfinite(out).all() and rec.inversion.shape == (6, 2, 4, 2)
    ref = DDIMSampler(ldm, 6, "uniform", 0.0)
    x = ref.invert(torch.cat([xa, xb]), torch.cat([ca, cb]), T, iters=2, uncond_scale=scale, uncond_cond=torch.cat([g["uncond_cond"]] * 2))
    assert torch.equal(x[:2], rec.end_noises[0]) and torch.equal(x[2:], rec.end_noises[1])
    assert torch.equal(ref.last_inversion.table, rec.inversion.table)
    fr = morph_fractions(5)
    xs, st, w = ref.morph_noise(x[:2], x[2:], fr)
    assert torch.equal(st, rec.stats) and torch.equal(w, rec.weights)
    cs = ref.morph_cond(ca, cb, fr)
    assert torch.equal(cs[0], ca) and torch.equal(cs[4], cb) and cs.shape == (5, 2, 1, 32)
    sw = ref.morph_cond(ca, cb, fr, "switch")
    assert all(torch.equal(sw[k], ca if k < 2 else cb) for k in range(5))
    uc10 = g["uncond_cond"].repeat(5, 1, 1)
    direct = ref.paint(xs.reshape(10, 2, 16, 16), cs.reshape(10, 1, 32), T, uncond_scale=scale, uncond_cond=uc10)
    assert torch.equal(direct.reshape(5, 2, 2, 16, 16), out)
    # batches smaller than K * R: paint on the same chunks
    small = sd.morph(xa, ca, xb, cb, 5, t_end=T, iters=2, batch=4, **g)
    chunks = [ref.paint(xs.reshape(10, 2, 16, 16)[i: i + 4].contiguous(), cs.reshape(10, 1, 32)[i: i + 4].contiguous(), T, uncond_scale=scale,
                        uncond_cond=uc10[i: i + 4].contiguous()) for i in (0, 4, 8)]
    assert torch.equal(torch.cat(chunks).reshape(5, 2, 2, 16, 16), small)
    # conds= overrides the interpolated conditions
    over = sd.morph(xa, ca, xb, cb, 5, t_end=T, iters=2, conds=cs, **g)
    assert torch.equal(over, out)
    # a captured step: the same bits, and a repeat captures nothing new
    gs = DDIMSampler(ldm, 6, "uniform", 0.0, graph=True)
    a = gs.morph(xa, ca, xb, cb, 5, t_end=T, iters=2, **g)
    n = gs.graph_captures
    assert torch.equal(a, out) and n >= 2
    assert torch.equal(gs.morph(xa, ca, xb, cb, 5, t_end=T, iters=2, **g), out) and gs.graph_captures == n
    print(f"scale={scale}: angles {rec.angles()}, last-iterate residuals {rec.inversion.residuals()[:, -1].max():.3e}")


def test_unet_window_plans_and_dual_guidance(ldm):
    xa, ca, xb, cb = unet_inputs()
    plan = WindowPlan(3, 8, 16)                                              # a two-segment canvas: three half-overlapping windows
    canvas = lambda v: torch.cat([v[0], v[1]], dim=1).unsqueeze(0).contiguous()
    cw = lambda c: torch.cat([c, c[:1]]).contiguous()
    sw = DDIMSampler(ldm, 6, "uniform", 0.0, windows=plan)
    out = sw.morph(canvas(xa), cw(ca), canvas(xb), cw(cb), 3, t_end=T, iters=2, **guidance(5.0, 3))
    assert out.shape == (3, 1, 2, plan.canvas_h, 16) and torch.isfinite(out).all()
    assert sw.last_morph.stats.shape == (1, 3) and sw.last_morph.weights.shape == (3, 1, 2)             # a canvas is one row
    dual = DDIMSampler(ldm, 6, "uniform", 0.0)
    uc = -torch.ones(2, 1, 32).cuda()
    d = dual.morph(xa, ca, xb, cb, 3, t_end=T, iters=2, uncond_scale=DualScale(5.0, 2.0, 16), uncond_cond=uc)
    assert d.shape == (3, 2, 2, 16, 16) and torch.isfinite(d).all()
    same = dual.morph(xa, ca, xb, cb, 3, t_end=T, iters=2, uncond_scale=DualScale(5.0, 5.0, 16), uncond_cond=uc)
    assert torch.equal(same, DDIMSampler(ldm, 6, "uniform", 0.0).morph(xa, ca, xb, cb, 3, t_end=T, iters=2, uncond_scale=5.0, uncond_cond=uc))


def test_unet_morph_from_noise_on_the_second_order_solver(ldm):
    _, ca, _, cb = unet_inputs()
    g = guidance(5.0)
    shape = (2, 2, 16, 16)
    dp = DPMSolverSampler(ldm, 6, seed=11)
    t = len(dp.time_steps) - 1
    out = dp.morph_from_noise(shape, ca, cb, 3, batch=2, **g)               # a frame per paint call: the batches of the plain calls below
    assert out.shape == (3,) + shape and torch.isfinite(out).all() and dp.last_morph.inversion is None
    plain = DPMSolverSampler(ldm, 6, seed=11)
    na, nb = plain.randn(shape, "cuda"), plain.randn(shape, "cuda")
    assert torch.equal(na, dp.last_morph.end_noises[0]) and torch.equal(nb, dp.last_morph.end_noises[1])
    assert torch.equal(plain.paint(na, ca, t, **g), out[0]) and torch.equal(plain.paint(nb, cb, t, **g), out[2])
    dd = DDIMSampler(ldm, 6, "uniform", 0.0, seed=11).morph_from_noise(shape, ca, cb, 3, t_start=T, **g)
    assert dd.shape == (3,) + shape and torch.isfinite(dd).all()


# ---------------------------------------------------------------------------------------------- the CLI
def run_cli(out, *argv):
    cmd = [sys.executable, "-m", "polyffusion_amd.inference_sdf", "--params_preset", "sdf_chd8bar", "--synthetic_weights", "--morph", "--ddim",
           "--ddim_steps", "4", "--morph_frames", "3", "--morph_iters", "2", "--score", "--seed", "9", "--output_dir", str(out)] + list(argv)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTHONPATH=REPO), cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def check_cli_files(out, said):
    names = sorted(os.listdir(out))
    npys = [f for f in names if f.endswith("_morph.npy")]
    assert len(npys) == 1
    stamp = npys[0][: -len("_morph.npy")]
    gen = np.load(out / npys[0])
    assert gen.shape == (3, 1, 2, 128, 128) and np.isfinite(gen).all()
    for f in [f"{stamp}_morph_{k}.mid" for k in range(3)] + [f"{stamp}_morph.mid"]:
        assert f in names and os.path.getsize(out / f) > 0, f
    assert len([f for f in names if f.endswith(".mid")]) == 4
    doc = json.load(open(out / f"{stamp}_score.json"))
    assert doc["frames"] == 3 and doc["fractions"] == [0.0, 0.5, 1.0] and doc["segments"] == 1
    for col in ("chord_f1_on_a", "chord_f1_on_b"):
        assert len(doc[col]) == 3 and all(0.0 <= v <= 1.0 for v in doc[col])
    assert "angle between the two end noises" in said and "frame 2 (t = 1.000) chord_f1" in said
    return gen


def test_cli_morphs_between_two_songs(tmp_path):
    from polyffusion_amd import synth
    rng = np.random.default_rng(4)
    for name, seed in (("a", 104), ("b", 105)):
        np.savez(tmp_path / f"{name}.npz", chord=synth.chords(1, seed).astype(np.float32),
                 prmat2c=(rng.random((1, 2, 128, 128)) > 0.97).astype(np.float32))
    said = run_cli(tmp_path / "out", "--cond_npz", str(tmp_path / "a.npz"), "--morph_to_npz", str(tmp_path / "b.npz"))
    gen = check_cli_files(tmp_path / "out", said)
    assert "largest relative residual of the last iterate over all steps" in said
    assert not np.array_equal(gen[0], gen[2])


def test_cli_morphs_between_two_synthetic_conditions(tmp_path):
    said = run_cli(tmp_path / "out", "--synthetic")
    gen = check_cli_files(tmp_path / "out", said)
    assert "between two noise draws" in said and not np.array_equal(gen[0], gen[2])
