"""Steering by resampling on the GPU (-m gpu).

ABI level, against the numpy restatement in ``tests/steer_ref.py``.  ``pf_steer_resample``: the weights within 8 ulp of numpy's (both
exponentials claim <= 1 ulp on identical IEEE arguments; the largest distance seen is printed), ``u`` bit for bit against the independent
Philox, and ESS, sum, flag, ancestors and ``base`` EXACTLY equal to the restatement run on the kernel's own returned weights and ``u`` -
from there on every operation is IEEE-exact, so no case is excluded and the test counts that none is skipped.  ``pf_rows_gather`` and
``pf_x0_predict``: bit for bit, on both access paths.  Sentinels guard every output; refusals launch nothing.

Sampler level, on the small synthetic UNet of ``tests/test_gpu_threshold.py`` (32 x 32): ``steering=None`` and ``lam=0`` are today's bits,
four steered steps are the loop written by hand, copies of a survivor differ after the step that copied them, the lineage is the hand
loop's, a window plan and a ``cond_concat`` model run an event.  CLI: ``--best_of 3 --steer`` writes the ``"steer"`` object, and two
ranks that take whole groups hold the candidates of the one-rank run."""
import argparse
import ctypes as C
import functools
import glob
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dpm_ref  # noqa: E402
import steer_ref as ref  # noqa: E402
import threshold_ref  # noqa: E402
from polyffusion_amd import _lib, _steps  # noqa: E402
from polyffusion_amd.arch import UNetConfig  # noqa: E402
from polyffusion_amd.sampler import DDIMSampler, SDFSampler, Steering, WindowPlan  # noqa: E402
from polyffusion_amd.unet import LatentDiffusion, UNetModel  # noqa: E402
from polyffusion_amd.weights import synth_unet_state  # noqa: E402

PAD = 8                 # elements of sentinel on either side of a buffer (the payload keeps its alignment)
SENTINEL = -777.25
F, D = np.float32, np.float64
TABLE = threshold_ref.table_of(dpm_ref.alpha_bar().astype(F))
TABLE.setflags(write=False)
BIG = (1 << 32) + 5     # group offsets and event counts beyond 32 bits


@pytest.fixture(scope="module")
def lib():
    _lib.require_gpu()
    return _lib.load()


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    """Equality of bits, NaNs matching NaNs (IEEE 754 leaves a NaN's sign and payload to the implementation)."""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def padded(values, off=0, dtype=torch.float32):
    """(whole buffer, payload view) on the device: the payload starts `off` elements past a 16-byte boundary, sentinels around it."""
    values = np.asarray(values).reshape(-1)
    n = len(values)
    whole = torch.full((n + 2 * PAD + 4,), SENTINEL if dtype.is_floating_point else int(SENTINEL), device="cuda", dtype=dtype)
    assert whole.data_ptr() % 16 == 0
    view = whole[PAD + off: PAD + off + n]
    view.copy_(torch.from_numpy(values.copy()).to(dtype))
    return whole, view


def untouched(whole, n, off=0):
    w = whole.cpu().numpy()
    guard = SENTINEL if w.dtype.kind == "f" else int(SENTINEL)
    return bool((w[: PAD + off] == guard).all() and (w[PAD + off + n:] == guard).all())


# ---------------------------------------------------------------------------------------------- pf_steer_resample
REWARDS = ("equal", "dominant", "spread", "some_nan", "all_nan")


@functools.lru_cache(maxsize=None)
def rewards(kind, groups, n):
    g = np.random.default_rng(100 * REWARDS.index(kind) + 10 * groups + n)
    r = {"equal": np.full(groups * n, 0.625), "dominant": g.random(groups * n) * 0.1, "spread": g.random(groups * n) * 2000.0,
         "some_nan": g.random(groups * n), "all_nan": np.full(groups * n, np.nan)}[kind].astype(D)
    if kind == "dominant":
        r[:: n] += 7.0
    if kind == "some_nan":
        r[g.integers(0, groups * n, max(1, groups * n // 4))] = np.nan
        r[0] = np.inf
    base = g.random(groups * n) * (0.0 if n % 2 or kind == "equal" else 0.5)       # (equal rewards over an equal base: equal weights)
    r.setflags(write=False)
    base.setflags(write=False)
    return r, base


def resample_padded(lib, reward, base, n, lam, ess, seed=0, goff=0, event=0):
    """One call on sentinel-guarded buffers: (ancestors, weights, base', stats) as numpy, after checking every guard and the read-only input."""
    cnt, groups = reward.size, reward.size // n
    r_w, r = padded(reward, 0, torch.float64)
    b_w, b = padded(base, 0, torch.float64)
    a_w, a = padded(np.full(cnt, -9), 0, torch.int32)
    w_w, w = padded(np.full(cnt, -9.0), 0, torch.float64)
    s_w, s = padded(np.full(groups * 4, -9.0), 0, torch.float64)
    args = _lib.SteerResampleArgs(reward=r.data_ptr(), base=b.data_ptr(), lam=lam, ess_frac=ess, seed=seed, group_offset=goff, event=event,
                                  ancestors=a.data_ptr(), weights=w.data_ptr(), stats=s.data_ptr(), groups=groups, n=n)
    _lib.check(lib.pf_steer_resample(C.byref(args), _lib.current_stream()), "pf_steer_resample", lib)
    torch.cuda.synchronize()
    assert untouched(r_w, cnt) and untouched(b_w, cnt) and untouched(a_w, cnt) and untouched(w_w, cnt) and untouched(s_w, groups * 4)
    assert same(r.cpu().numpy(), reward)
    return a.cpu().numpy(), w.cpu().numpy(), b.cpu().numpy(), s.cpu().numpy().reshape(groups, 4)


WORST = {"ulp": 0.0}


@pytest.mark.parametrize("n", [1, 2, 3, 8, 64, 256])
def test_resample_is_the_restatement(lib, n):
    done, flags = 0, set()
    for groups in (1, 3):
        for kind in REWARDS:
            reward, base = rewards(kind, groups, n)
            for ess in (0.5, 1.0):
                for lam in (0.0, 5.0, 5000.0):
                    seed, goff, event = 0x9E3779B97F4A7C15 + n, BIG + groups, BIG * 3 + REWARDS.index(kind)
                    tag = (n, groups, kind, ess, lam)
                    anc, w, nb, st = resample_padded(lib, reward, base, n, lam, ess, seed, goff, event)
                    _, w_np, _, _ = ref.resample(reward, base, n, lam, ess, seed, goff, event)
                    # the weights: within 8 ulp of numpy's
                    ulp = np.abs(w - w_np) / np.spacing(np.maximum(np.abs(w_np), np.finfo(D).tiny))
                    WORST["ulp"] = max(WORST["ulp"], float(ulp.max()))
                    assert (ulp <= 8).all(), (tag, float(ulp.max()))
                    # u: bit for bit the independent Philox
                    assert [float(v) for v in st[:, 3]] == [float(ref.u_of(seed, goff + g, event)) for g in range(groups)], tag
                    # everything after the weights: exactly the restatement on the kernel's own weights and u
                    want_anc, _, want_base, want_st = ref.resample(reward, base, n, lam, ess, weights=w, u=st[:, 3])
                    assert np.array_equal(anc, want_anc), tag
                    assert same(nb, want_base) and same(st, want_st), (tag, st, want_st)
                    done += 1
                    flags |= set(st[:, 2].tolist())
                    if kind == "equal":
                        assert np.array_equal(anc, np.tile(np.arange(n), groups)) and (w == 1.0).all()
                    if kind == "all_nan":
                        assert (st[:, 2] == 2.0).all() and same(nb, base)
                    if kind == "dominant" and lam == 5.0 and n > 2:
                        assert (st[:, 2] == 1.0).all() and (anc == 0).all() and (nb == np.repeat(reward[::n], n)).all()
                    if lam == 0.0 and ess < 1.0 and kind in ("equal", "dominant", "spread"):
                        assert (st[:, 2] == 0.0).all() and same(nb, base)
                    for g in range(groups):
                        if st[g, 2] == 1.0:
                            assert (w[g * n: (g + 1) * n][anc[g * n: (g + 1) * n]] > 0).all(), (tag, g)
    assert done == 2 * len(REWARDS) * 2 * 3                                          # no case is skipped
    assert flags == {0.0, 1.0, 2.0}, flags
    print(f"n = {n}: largest distance of a weight from numpy's so far {WORST['ulp']} ulp")


def test_resample_is_the_same_from_call_to_call_and_however_the_groups_are_split(lib):
    n, groups = 8, 3
    reward, base = rewards("spread", groups, n)
    whole = resample_padded(lib, reward, base, n, 0.01, 1.0, 77, BIG, 9)
    again = resample_padded(lib, reward, base, n, 0.01, 1.0, 77, BIG, 9)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(whole, again))
    parts = [resample_padded(lib, reward[g * n: (g + 1) * n], base[g * n: (g + 1) * n], n, 0.01, 1.0, 77, BIG + g, 9) for g in range(groups)]
    for k in range(4):
        assert np.array_equal(bits(np.concatenate([p[k] for p in parts])), bits(whole[k])), k
    assert (whole[3][:, 2] == 1.0).all() and len(set(whole[3][:, 3].tolist())) == groups     # every group its own u
    other = resample_padded(lib, reward, base, n, 0.01, 1.0, 77, BIG, 10)
    assert not np.array_equal(other[3][:, 3], whole[3][:, 3])                       # and another event another one


# ---------------------------------------------------------------------------------------------- pf_rows_gather
def gather_padded(lib, srcs, anc, groups, n, per, off=0):
    rows = groups * n * per
    s_bufs = [padded(v, off) for v in srcs]
    d_bufs = [padded(np.full(v.size, -3.0, F), off) for v in srcs]
    a_w, a = padded(anc, 0, torch.int32)
    args = _lib.RowsGatherArgs()
    for k, v in enumerate(srcs):
        args.src[k], args.dst[k], args.row_elems[k] = s_bufs[k][1].data_ptr(), d_bufs[k][1].data_ptr(), v.size // rows
    args.n_tensors, args.ancestors, args.groups, args.n, args.per = len(srcs), a.data_ptr(), groups, n, per
    _lib.check(lib.pf_rows_gather(C.byref(args), _lib.current_stream()), "pf_rows_gather", lib)
    torch.cuda.synchronize()
    for v, (sw, sv), (dw, _) in zip(srcs, s_bufs, d_bufs):
        assert untouched(sw, v.size, off) and untouched(dw, v.size, off) and np.array_equal(bits(sv), bits(v.reshape(-1)))
    assert untouched(a_w, anc.size) and np.array_equal(a.cpu().numpy(), anc)
    return [d.cpu().numpy().reshape(v.shape) for v, (_, d) in zip(srcs, d_bufs)]


ANCESTORS = {"identity": [0, 1, 2, 0, 1, 2], "duplicates": [2, 2, 0, 1, 1, 1], "out_of_range": [5, -1, 1, 2 ** 31 - 1, -2 ** 31, 0]}     # built by hand: clamped


@pytest.mark.parametrize("row_elems", [4, 6, 2048, 32768, 32772])
def test_gather_is_the_numpy_gather_bit_for_bit(lib, row_elems):
    groups, n = 2, 3
    for per in (1, 3):
        rows = groups * n * per
        g = np.random.default_rng(row_elems + per)
        src = g.standard_normal((rows, row_elems)).astype(F)
        src[0, 0], src[-1, -1] = np.nan, np.inf
        for name, anc in ANCESTORS.items():
            anc = np.array(anc, np.int32)
            want = ref.gather(src, anc, n, per)
            for off in (0, 1):                                                       # one float off a 16-byte boundary: element by element
                got = gather_padded(lib, [src], anc, groups, n, per, off)[0]
                assert np.array_equal(bits(got), bits(want)), (row_elems, per, name, off)
            if name == "out_of_range":
                assert np.array_equal(bits(want), bits(ref.gather(src, np.array([2, 0, 1, 2, 0, 0]), n, per)))


def test_gather_moves_two_and_four_tensors_of_different_row_lengths_in_one_launch(lib):
    groups, n, per = 2, 3, 3
    rows = groups * n * per
    g = np.random.default_rng(4)
    srcs = [g.standard_normal((rows, re)).astype(F) for re in (2048, 6, 4100, 5)]
    anc = np.array(ANCESTORS["duplicates"], np.int32)
    for k in (2, 4):
        for off in (0, 1):
            got = gather_padded(lib, srcs[:k], anc, groups, n, per, off)
            for v, o in zip(srcs[:k], got):
                assert np.array_equal(bits(o), bits(ref.gather(v, anc, n, per))), (k, off, v.shape)


# ---------------------------------------------------------------------------------------------- pf_x0_predict
def predict_padded(lib, xs, eps, t, t_stride, off=0):
    rows, n = eps.shape
    tt = np.full((rows - 1) * t_stride + 1, 7, np.int64)
    tt[::t_stride] = t
    x_w, x = padded(xs, off)
    e_w, e = padded(eps, off)
    o_w, o = padded(np.zeros(rows * n, F), off)
    t_w, td = padded(tt, 0, torch.int64)
    tb_w, tb = padded(TABLE, 0)
    a = _lib.X0PredictArgs(x=x.data_ptr(), x_row_stride=xs.shape[1], eps=e.data_ptr(), t=td.data_ptr(), t_stride=t_stride, table=tb.data_ptr(),
                           n_table=TABLE.shape[0], x0=o.data_ptr(), rows=rows, row_elems=n)
    _lib.check(lib.pf_x0_predict(C.byref(a), _lib.current_stream()), "pf_x0_predict", lib)
    torch.cuda.synchronize()
    assert untouched(x_w, xs.size, off) and untouched(e_w, eps.size, off) and untouched(o_w, rows * n, off) and untouched(t_w, tt.size) and untouched(tb_w, TABLE.size)
    assert same(x.cpu().numpy(), xs.reshape(-1)) and same(e.cpu().numpy(), eps.reshape(-1))
    return o.cpu().numpy().reshape(rows, n)


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n", [6, 2048, 32768])
def test_x0_predict_is_the_fp32_restatement_on_both_paths(lib, rows, n):
    g = np.random.default_rng(rows * 7 + n)
    for extra, t in ((0, [0, 500, 999]), (4, [-3, 1000, 2 ** 40]), (3, [999, 1, 250])):      # x_row_stride > row_elems; t outside the table is clamped
        xs = np.full((rows, n + extra), F(123.5))
        xs[:, :n] = g.standard_normal((rows, n)).astype(F)
        eps = g.standard_normal((rows, n)).astype(F)
        if n > 6:
            eps[rows - 1, n // 2], xs[0, n // 3] = np.nan, np.inf
        t = np.array(t[:rows], np.int64)
        want = ref.x0(xs, eps, t, TABLE)
        got = {(off, ts): predict_padded(lib, xs, eps, t, ts, off) for off in (0, 1) for ts in (1, 3)}
        for key, out in got.items():
            assert same(out, want), (rows, n, extra, key)
        assert np.array_equal(bits(got[(0, 1)]), bits(got[(1, 3)]))                  # 16-byte vectors and single elements: the same bits
    # the expression pf_x0_threshold bounds: with a range nothing leaves, its eps' is eps
    xs, eps = g.standard_normal((rows, n)).astype(F), g.standard_normal((rows, n)).astype(F)
    t = np.array([300, 600, 900][:rows], np.int64)
    x0 = predict_padded(lib, xs, eps, t, 1)
    out, _ = threshold_ref.threshold(xs, eps, t, TABLE, "clip", lo=float(x0.min()), hi=float(x0.max()))
    assert np.array_equal(bits(out), bits(eps))


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(lib):
    n, groups = 8, 2
    f64 = lambda v, k: torch.full((k,), v, device="cuda", dtype=torch.float64)
    reward, base = f64(1.0, groups * n), f64(SENTINEL, groups * n)
    anc = torch.full((groups * n,), -7, device="cuda", dtype=torch.int32)
    weights, stats = f64(SENTINEL, groups * n), f64(SENTINEL, groups * 4)

    def refused(fn, prefix, pattern, a):
        rc = fn(C.byref(a), _lib.current_stream())
        msg = lib.pf_last_error().decode()
        assert rc == -1 and msg.startswith(prefix) and pattern in msg, (rc, msg)

    mk = lambda **kw: _lib.SteerResampleArgs(**{**dict(reward=reward.data_ptr(), base=base.data_ptr(), lam=5.0, ess_frac=0.5, seed=1, group_offset=0, event=0,
                                                      ancestors=anc.data_ptr(), weights=weights.data_ptr(), stats=stats.data_ptr(), groups=groups, n=n), **kw})
    for pattern, kw in (("257 particles per group", dict(n=257)), ("0 particles per group", dict(n=0)), ("0 groups", dict(groups=0)), ("lambda -1", dict(lam=-1.0)),
                        ("ess_frac 0 outside", dict(ess_frac=0.0)), ("base overlaps weights", dict(weights=base.data_ptr())), ("null reward", dict(stats=None)),
                        ("8-byte aligned", dict(base=base.data_ptr() + 4))):
        refused(lib.pf_steer_resample, "steer_resample: ", pattern, mk(**kw))
    x, eps, x0 = torch.zeros(2 * 16, device="cuda"), torch.zeros(2 * 16, device="cuda"), torch.full((2 * 16,), SENTINEL, device="cuda")
    t, table = torch.zeros(2, dtype=torch.int64, device="cuda"), torch.from_numpy(TABLE.copy()).cuda()
    mk = lambda **kw: _lib.X0PredictArgs(**{**dict(x=x.data_ptr(), x_row_stride=16, eps=eps.data_ptr(), t=t.data_ptr(), t_stride=1, table=table.data_ptr(), n_table=1000,
                                                  x0=x0.data_ptr(), rows=2, row_elems=16), **kw})
    for pattern, kw in (("0 rows", dict(rows=0)), ("x_row_stride 15 below row_elems 16", dict(x_row_stride=15)), ("x0 overlaps eps", dict(x0=eps.data_ptr() + 4)),
                        ("x0 overlaps x", dict(x0=x.data_ptr())), ("n_table 0", dict(n_table=0)), ("null x", dict(table=None))):
        refused(lib.pf_x0_predict, "x0_predict: ", pattern, mk(**kw))
    src, dst = torch.zeros(12 * 8, device="cuda"), torch.full((12 * 8,), SENTINEL, device="cuda")
    ga = torch.zeros(6, dtype=torch.int32, device="cuda")

    def gargs(**kw):
        a = _lib.RowsGatherArgs()
        a.src[0], a.dst[0], a.row_elems[0] = src.data_ptr(), dst.data_ptr(), 8
        a.n_tensors, a.ancestors, a.groups, a.n, a.per = 1, ga.data_ptr(), 2, 3, 2
        for k, v in kw.items():
            if k in ("src", "dst", "row_elems"):
                getattr(a, k)[0] = v
            else:
                setattr(a, k, v)
        return a

    for pattern, kw in (("5 tensors", dict(n_tensors=5)), ("of 0 images", dict(per=0)), ("dst of tensor 0 overlaps src of tensor 0", dict(dst=src.data_ptr() + 16)),
                        ("rows of 0 elements", dict(row_elems=0)), ("null ancestors", dict(ancestors=None)), ("null src or dst", dict(src=None))):
        refused(lib.pf_rows_gather, "rows_gather: ", pattern, gargs(**kw))
    torch.cuda.synchronize()
    assert (base == SENTINEL).all() and (weights == SENTINEL).all() and (stats == SENTINEL).all() and (anc == -7).all()
    assert (x0 == SENTINEL).all() and (dst == SENTINEL).all()


# ---------------------------------------------------------------------------------------------- the samplers
def small(in_channels=2):
    kw = dict(in_channels=in_channels, out_channels=2, channels=32, n_res_blocks=1, attention_levels=(1,), channel_multipliers=(1, 2), n_heads=2,
              tf_layers=1, d_cond=32)
    m = UNetModel(img_h=32, img_w=32, **kw)
    m.load_state_dict(synth_unet_state(UNetConfig(**kw), 0))
    return m


@pytest.fixture(scope="module")
def net():
    _lib.require_gpu()
    return small()


def inputs(rows=4, h=32, cond_rows=None):
    g = torch.Generator().manual_seed(9)
    cond_rows = rows if cond_rows is None else cond_rows
    x = torch.randn(rows, 2, h, 32, generator=g).cuda()
    c = torch.randn(1, 1, 32, generator=g).expand(cond_rows, -1, -1).contiguous().cuda()      # the particles of a group: candidates for ONE song
    return x, c, -torch.ones_like(c)


FAMILIES = {
    "ddpm": lambda ldm, **kw: SDFSampler(ldm, seed=3, **kw),
    "ddim": lambda ldm, **kw: DDIMSampler(ldm, 20, "uniform", 1.0, seed=3, **kw),
}
SCALE = 5.0


def reward_of(per=1):
    """float64 [rows / per]: the mean of the predicted image, times 10 - with lam = 50 a few hundredths decide an event"""
    return lambda x0: x0.double().reshape(x0.shape[0] // per, -1).mean(1) * 10.0


@pytest.mark.parametrize("family", list(FAMILIES))
def test_none_and_lambda_zero_are_todays_bits(net, family):
    x, c, uc = inputs()
    kw = dict(uncond_scale=SCALE, uncond_cond=uc)
    plain = FAMILIES[family](LatentDiffusion(net)).paint(x, c, 3, **kw)
    s = FAMILIES[family](LatentDiffusion(net), steering=None)
    assert torch.equal(s.paint(x, c, 3, **kw), plain) and s.last_steering is None
    for ess in (0.5, 1.0):
        s = FAMILIES[family](LatentDiffusion(net), steering=Steering(n=4, reward=reward_of(), lam=0.0, every=1, ess=ess))
        assert torch.equal(s.paint(x, c, 3, **kw), plain)
        rec = s.last_steering
        assert rec.steps == [0, 1, 2] and all((st[:, 2] == (1.0 if ess == 1.0 else 0.0)).all() for st in rec.stats)
        assert rec.lineage().tolist() == [[0, 1, 2, 3]] and all((w == 1.0).all() for w in rec.weights)
    # inpainting: the known region's draws stay where they were
    orig, mask = torch.rand(4, 2, 32, 32, generator=torch.Generator().manual_seed(1)).cuda(), torch.zeros(4, 2, 32, 32).cuda()
    mask[:, :, :16] = 1
    plain = FAMILIES[family](LatentDiffusion(net)).paint(x, c, 3, orig=orig, mask=mask, **kw)
    s = FAMILIES[family](LatentDiffusion(net), steering=Steering(n=2, reward=reward_of(), lam=0.0, every=1))
    assert torch.equal(s.paint(x, c, 3, orig=orig, mask=mask, **kw), plain) and len(s.last_steering.stats) == 3


@pytest.mark.parametrize("family", list(FAMILIES))
def test_four_steered_steps_are_the_loop_written_by_hand(net, family):
    x, c, uc = inputs()
    kw = dict(uncond_scale=SCALE, uncond_cond=uc)
    st = Steering(n=4, reward=reward_of(), lam=50.0, every=1, ess=1.0)
    s = FAMILIES[family](LatentDiffusion(net), steering=st)
    after = {}
    s.on_step = lambda step, xs: after.setdefault(len(after), xs.clone())
    got = s.paint(x, c, 3, **kw)
    rec = s.last_steering
    want, ancs, flags = ref.hand_loop(FAMILIES[family](LatentDiffusion(net)), _steps, x, c, 3, st, reward_of(), **kw)
    assert torch.equal(got, want)
    assert len(rec.ancestors) == 3 and rec.steps == [0, 1, 2] and all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(rec.ancestors, ancs))
    assert all(np.array_equal(s_.cpu().numpy()[:, 2], f) for s_, f in zip(rec.stats, flags)) and all((f == 1.0).all() for f in flags)
    assert np.array_equal(rec.lineage(), ref.lineage(ancs, 4))
    rep = rec.report()
    assert rep["steps"] == [0, 1, 2] and rep["resampled"] == [[1], [1], [1]] and len(rep["ess"]) == 3
    plain = FAMILIES[family](LatentDiffusion(net)).paint(x, c, 3, **kw)
    assert not torch.equal(got, plain) and torch.isfinite(got).all()
    # an event that duplicates a particle: its copies differ after the very step that copied them - every row draws its own noise
    first = ancs[0]
    dup = [(j, k) for j in range(4) for k in range(j + 1, 4) if first[j] == first[k]]
    assert dup, first
    for j, k in dup:
        assert not torch.equal(after[0][j], after[0][k])
    # a second paint continues the event counter, as the draw counter: another u
    s.paint(x, c, 3, **kw)
    assert s._steer_events == 6 and not torch.equal(s.last_steering.stats[0][:, 3], rec.stats[0][:, 3])


def test_groups_of_several_images_and_the_window_of_time_steps(net):
    x, c, uc = inputs(8)
    kw = dict(uncond_scale=SCALE, uncond_cond=uc)
    st = Steering(n=2, per=2, reward=reward_of(2), lam=50.0, every=1, ess=1.0, window=(0.001, 0.002))     # time-step values 1 .. 1 of 1000
    s = SDFSampler(LatentDiffusion(net), seed=3, sample_offset=8, steering=st)
    got = s.paint(x, c, 3, **kw)
    rec = s.last_steering
    assert st.window_values(1000) == (1, 1) and rec.steps == [2] and rec.t_values == [1] and rec.ancestors[0].shape == (4,)
    want, ancs, _ = ref.hand_loop(SDFSampler(LatentDiffusion(net), seed=3, sample_offset=8), _steps, x, c, 3, st, reward_of(2), **kw)
    assert torch.equal(got, want) and np.array_equal(rec.ancestors[0].cpu().numpy(), ancs[0])
    assert [float(v) for v in rec.stats[0][:, 3].cpu()] == [float(ref.u_of(3, 2 + g, 0)) for g in range(2)]      # group_offset = sample_offset // (n * per)


def test_a_window_plan_canvas_and_a_cond_concat_model_each_run_an_event(net):
    wp = WindowPlan(2, 16, 32)
    x, c, uc = inputs(2, wp.canvas_h, 4)                                           # two canvases of two windows each: one condition row per window
    kw = dict(uncond_scale=SCALE, uncond_cond=uc)
    st = Steering(n=2, reward=reward_of(), lam=50.0, every=1, ess=1.0)
    s = DDIMSampler(LatentDiffusion(net), 20, "uniform", 1.0, seed=3, windows=wp, steering=st)
    got = s.paint(x, c, 1, **kw)
    want, ancs, _ = ref.hand_loop(DDIMSampler(LatentDiffusion(net), 20, "uniform", 1.0, seed=3, windows=wp), _steps, x, c, 1, st, reward_of(), **kw)
    assert len(s.last_steering.ancestors) == 1 and torch.equal(got, want) and np.array_equal(s.last_steering.ancestors[0].cpu().numpy(), ancs[0])
    ldm = LatentDiffusion(small(in_channels=4))
    x, c, uc = inputs(4)
    cc = torch.randn(1, 2, 32, 32, generator=torch.Generator().manual_seed(5)).expand(4, -1, -1, -1).contiguous().cuda()
    kw = dict(uncond_scale=SCALE, uncond_cond=uc, cond_concat=cc)
    s = SDFSampler(ldm, seed=3, steering=Steering(n=4, reward=reward_of(), lam=50.0, every=1, ess=1.0))
    got = s.paint(x, c, 1, **kw)
    want, ancs, _ = ref.hand_loop(SDFSampler(ldm, seed=3), _steps, x, c, 1, s.steering, reward_of(), **kw)
    assert len(s.last_steering.ancestors) == 1 and torch.equal(got, want) and np.array_equal(s.last_steering.ancestors[0].cpu().numpy(), ancs[0])


# ---------------------------------------------------------------------------------------------- the CLI
BASE = ["--params_preset", "sdf_chd8bar", "--synthetic_weights", "--synthetic", "--length", "1", "--ddim", "--ddim_steps", "4", "--ddim_eta", "1", "--seed", "5",
        "--precision", "bf16x3", "--uncond_scale", "2"]


def test_cli_best_of_with_steer_writes_the_steer_object(tmp_path):
    from polyffusion_amd import inference_sdf
    out = tmp_path / "s"
    assert inference_sdf.main(BASE + ["--output_dir", str(out), "--num_generate", "2", "--best_of", "3", "--steer", "--steer_every", "1", "--steer_ess", "1"]) == 0
    npys = sorted(glob.glob(os.path.join(str(out), "*.npy")))
    doc = json.load(open(glob.glob(os.path.join(str(out), "*_score.json"))[0]))
    assert len(npys) == 2 and all("steer=chord,lam=10.0,every=1,ess=1.0]" in f for f in npys)
    assert doc["best_of"] == 3 and doc["rank_by"] == "chord" and len(doc["candidates"]) == 6
    sd = doc["steer"]
    assert (sd["by"], sd["lambda"], sd["every"], sd["window"], sd["ess"], sd["n"]) == ("chord", 10.0, 1, [0.0, 1.0], 1.0, 3)
    ev = sd["ranks"][0]["events"]
    assert sd["ranks"][0]["groups"] == [0, 2] and ev["steps"] == [0, 1, 2] and all(len(e) == 2 for e in ev["ess"]) and all(f == [1, 1] for f in ev["resampled"])
    assert [l["candidate"] for l in sd["lineage"]] == [s["candidate"] for s in doc["songs"]]
    assert all(l["descends_from"] // 3 == l["candidate"] // 3 for l in sd["lineage"])            # a song descends from a candidate of its own group
    # without --steer nothing changes, file names included
    plain = tmp_path / "p"
    assert inference_sdf.main(BASE + ["--output_dir", str(plain), "--num_generate", "2", "--best_of", "3"]) == 0
    assert all("steer" not in f and "[scale=2.0]" in f for f in os.listdir(plain))
    assert "steer" not in json.load(open(glob.glob(os.path.join(str(plain), "*_score.json"))[0]))


def steered_runs(num_generate, best_of=2):
    from polyffusion_amd import inference_sdf, synth
    from polyffusion_amd.params import preset
    p = preset("sdf_chd8bar")
    model = inference_sdf.load_model(p, argparse.Namespace(synthetic_weights=True, precision="bf16x3", chkpt_path=None, chkpt_name=None), 0, 1)
    model.ldm.eps_model.set_precision("bf16x3")
    chd = torch.from_numpy(synth.chords(1, 21)).cuda()
    cond, cond_mid = inference_sdf.encode_conditions(model, p, chd, None, False)
    records = {}

    def run(r, w, songs=num_generate):
        args = inference_sdf.make_parser().parse_args(BASE + ["--num_generate", str(songs), "--best_of", str(best_of), "--steer", "--steer_every", "1", "--steer_ess", "1",
                                                              "--steer_lambda", "50"])
        steer = inference_sdf.check_steer_args(args, p.cond_type)
        gen, ex = inference_sdf.generate_songs(model, p, args, cond, cond_mid, None, None, 99, r, w, steer=steer, chd=chd)
        records[(r, w, songs)] = ex.sampler.last_steering
        return gen

    return run, records


def test_a_rank_that_holds_whole_groups_reproduces_the_one_rank_run_of_those_groups():
    """Rank 0 of two holds group 0, and so does the one-rank run of one song - through another shard path."""
    run, records = steered_runs(2)
    a, b = run(0, 2), run(0, 1, songs=1)
    assert a.shape == (2, 1, 2, 128, 128) and torch.equal(a, b)
    assert all(torch.equal(x, y) for x, y in zip(records[(0, 2, 2)].ancestors, records[(0, 1, 1)].ancestors))
    assert torch.equal(run(1, 2), run(1, 2)) and not torch.equal(run(1, 2), a)      # the other rank: its own groups, reproducibly


def test_two_ranks_taken_by_groups_hold_the_candidates_of_the_one_rank_run():
    """Every steering decision of the two-rank run is the one-rank run's - each group draws the ``u`` of its GLOBAL index, the lineages
    agree - and so are the candidates, bit for bit.  The denoiser picks its tiles by the per-launch batch, so two launches of different
    batch differ in their last bits (about 2.5e-4 here between 4 rows and 2, with or without steering; tests/test_gpu_checkpoint_cli.py
    holds the unsteered sharding to 2e-4 for that reason): under --steer every group is a launch of its own, the same launch on any rank."""
    run, records = steered_runs(2)
    full = run(0, 1)
    halves = torch.cat([run(0, 2), run(1, 2)])
    assert full.shape == (4, 1, 2, 128, 128) and halves.shape == full.shape
    u = lambda key: torch.cat([s[:, 3] for s in records[key].stats]).tolist()
    assert u((0, 1, 2))[0::2] == u((0, 2, 2)) and u((0, 1, 2))[1::2] == u((1, 2, 2))  # every group draws the u of its global index
    assert np.array_equal(records[(0, 1, 2)].lineage(), np.concatenate([records[(0, 2, 2)].lineage(), records[(1, 2, 2)].lineage()]))
    print("two ranks by groups against one rank: largest |difference|", float((halves - full).abs().max()))
    assert torch.equal(halves, full)
