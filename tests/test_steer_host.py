"""Steering by resampling without a GPU: the numpy restatement in ``tests/steer_ref.py`` against the properties the rule promises (equal
weights give the identity for every u; every ancestor has a positive weight; copy counts are floor or ceil of the expected number;
``lambda = 0`` never resamples below ``ess = 1``; rewards that are all NaN give the identity with flag 2; the largest u at n = 256 never
selects a zero-weight last particle) and against planted defects, and the library and the host mirror: the entry points are declared,
exported by both builds and bound, the structs are laid out as the header says, every refusal comes before any launch, the ``Steering``
dataclass validates its fields, the samplers and the CLI refuse what they must, the stamp names the setting, and sharding by groups gives
every candidate the global index of the one-rank run."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import dpm_ref
import noise_matrix
import steer_ref as ref
from polyffusion_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x100000        # a non-null, 16-byte aligned address that a refused call never touches
NAMES = ("pf_x0_predict", "pf_steer_resample", "pf_rows_gather")
D = np.float64


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from polyffusion_amd.build import build
        build(verbose=False)
    return _lib.load()


def seeded_cases():
    """(reward, base, n, lam, ess) over seeds, sizes and spreads - shared by the property tests."""
    for seed in range(40):
        g = np.random.default_rng(seed)
        n = (1, 2, 3, 8, 64, 256)[seed % 6]
        groups = 1 + seed % 3
        reward = g.random(groups * n) * (1.0, 10.0, 1e3)[seed % 3]
        base = g.random(groups * n) if seed % 2 else np.zeros(groups * n)
        if seed % 5 == 4 and n > 2:
            reward[g.integers(0, reward.size, 2)] = np.nan
        yield reward, base, n, (0.5, 5.0, 50.0)[seed % 3], (0.5, 1.0)[seed % 2], seed


# ---------------------------------------------------------------------------------------------- the restatement against its properties
def test_the_philox_word_is_the_published_generator_under_a_tagged_key():
    for ctr, key, out in noise_matrix.KAT:                                           # the independent Philox reproduces Random123's vectors
        assert noise_matrix.philox4x32(ctr, key) == out
    seed, g, ev = 0x9E3779B97F4A7C15, (1 << 40) + 3, (1 << 33) + 1
    want = noise_matrix.philox4x32((g & 0xFFFFFFFF, g >> 32, ev & 0xFFFFFFFF, ev >> 32), (seed & 0xFFFFFFFF, (seed >> 32) ^ 0x53544552))[0]
    assert ref.u_word(seed, g, ev) == want and ref.u_of(seed, g, ev) == want / 2.0 ** 32
    assert ref.u_word(seed, g, ev) != noise_matrix.group_words(seed, ev, g)[0]       # the noise stream of the same (seed, counter) is another
    assert 0.0 <= ref.u_of(seed, g, ev) < 1.0 and (ref.u_of(seed, g, ev) * 2.0 ** 32).is_integer()


def test_equal_weights_give_the_identity_for_every_u():
    for n in (1, 2, 3, 8, 64, 256):
        for u in (0.0, 2.0 ** -32, 0.5, 0.999, 1.0 - 2.0 ** -32):
            for r0 in (0.0, 0.37, -5.0):
                anc, w, nb, st = ref.resample(np.full(n, r0), np.zeros(n), n, 7.0, 1.0, u=[u])
                assert st[0, 2] == 1.0 and np.array_equal(anc, np.arange(n)) and (w == 1.0).all() and st[0, 0] == n and st[0, 1] == n


def test_every_ancestor_has_a_positive_weight_and_copy_counts_are_floor_or_ceil():
    seen = 0
    for reward, base, n, lam, ess, seed in seeded_cases():
        anc, w, nb, st = ref.resample(reward, base, n, lam, ess, seed, seed, seed)
        for g in range(reward.size // n):
            a, wg = anc[g * n: (g + 1) * n], w[g * n: (g + 1) * n]
            assert ((0 <= a) & (a < n)).all()
            if st[g, 2] == 1.0:
                seen += 1
                assert (wg[a] > 0).all(), (seed, g)
                assert ref.copy_counts_ok(a, wg, n), (seed, g)
                assert np.array_equal(nb[g * n: (g + 1) * n], reward[g * n: (g + 1) * n][a])
                assert (np.diff(a) >= 0).all()                                       # systematic resampling keeps the order
            else:
                assert np.array_equal(a, np.arange(n)) and np.array_equal(nb[g * n: (g + 1) * n], base[g * n: (g + 1) * n], equal_nan=True)
    assert seen >= 20


def test_lambda_zero_never_resamples_below_ess_one():
    for reward, base, n, _, _, seed in seeded_cases():
        reward = np.nan_to_num(reward)
        for ess in (0.5, 0.99):
            anc, w, nb, st = ref.resample(reward, base, n, 0.0, ess, seed)
            assert (st[:, 2] == 0.0).all() and (w == 1.0).all() and np.array_equal(anc, np.tile(np.arange(n), reward.size // n))
            assert np.array_equal(nb, base) and (st[:, 0] == n).all()


def test_rewards_that_are_all_nan_give_the_identity_with_flag_two():
    for n in (1, 3, 256):
        base = np.arange(2 * n, dtype=D)
        anc, w, nb, st = ref.resample(np.full(2 * n, np.nan), base, n, 5.0, 1.0)
        assert (st[:, 2] == 2.0).all() and (w == 0.0).all() and np.isnan(st[:, 0]).all() and (st[:, 1] == 0.0).all()
        assert np.array_equal(anc, np.tile(np.arange(n), 2)) and np.array_equal(nb, base)
    # infinite rewards and an overflowing log weight count as not finite; one finite particle takes everything
    r = np.array([np.inf, 1.0, -np.inf, 1e308])
    anc, w, nb, st = ref.resample(r, np.zeros(4), 4, 5000.0, 1.0, u=[0.3])
    assert list(w) == [0.0, 1.0, 0.0, 0.0] and st[0, 2] == 1.0 and list(anc) == [1, 1, 1, 1] and (nb == 1.0).all()


def test_the_largest_u_at_n_256_never_selects_a_zero_weight_last_particle():
    n, u = 256, 1.0 - 2.0 ** -32
    g = np.random.default_rng(11)
    for trial in range(20):
        w = np.exp(-g.random(n) * (1, 30, 700)[trial % 3])
        w[-1] = 0.0
        if trial % 4 == 3:
            w[-5:] = 0.0
        S, _, c = ref.serial_sums(w)
        anc, _, st = ref.decide(w, True, np.arange(n, dtype=D), np.zeros(n), 1.0, u)
        p_last = (D(n - 1) + D(u)) * (S / D(n))
        assert p_last < S and st[2] == 1.0                                           # p_j < S strictly: the clamp never acts
        assert anc.max() < n - 1 and (w[anc] > 0).all() and c[anc[-1]] > p_last
    assert D(n - 1) + D(u) == (n - 1) + u and ((D(n - 1) + D(u)) * 2.0 ** 32).is_integer()      # j + u is exact: u has 32 bits


def check_rule(resample):
    """What any implementation of the rule must pass; returns the name of the first property it fails, or None."""
    # the serial sum: weights whose tree sum and serial sum differ in the last bit
    w = np.array([1.0] + [2.0 ** -53] * 3 + [2.0 ** -52] * 4)
    S = D(0.0)
    for x in w:
        S = S + D(x)
    got = resample(np.zeros(w.size), np.zeros(w.size), w.size, 1.0, 1.0, weights=w, u=[0.25])
    if got[3][0, 1] != S:
        return "serial_sum"
    # <=, not <: equal weights have ESS == n == 1.0 * n exactly and resample (to the identity, and base moves)
    anc, _, nb, st = resample(np.full(4, 2.0), np.zeros(4), 4, 3.0, 1.0, u=[0.5])
    if st[0, 2] != 1.0 or not (nb == 2.0).all():
        return "ess_le"
    # u has 32 bits
    st = resample(np.arange(8.0), np.zeros(8), 8, 1.0, 1.0, seed=5, group_offset=9, event=2)[3]
    if not (st[0, 3] * 2.0 ** 32).is_integer() or st[0, 3] != ref.u_word(5, 9, 2) / 2.0 ** 32:
        return "u32"
    # flag 0 leaves base alone
    base = np.array([0.5, 0.25, 0.125, 0.0625])
    anc, _, nb, st = resample(np.array([1.0, 1.01, 1.02, 1.03]), base, 4, 0.1, 0.5)
    if st[0, 2] != 0.0 or not np.array_equal(nb, base) or not np.array_equal(anc, np.arange(4)):
        return "base_kept"
    return None


def test_planted_defects_are_caught():
    assert check_rule(ref.resample) is None
    caught = {d: check_rule(lambda *a, _d=d, **k: ref.resample(*a, defect=_d, **k)) for d in ref.DEFECTS}
    assert caught == {"tree_sum": "serial_sum", "strict_ess": "ess_le", "u53": "u32", "base_on_keep": "base_kept"}, caught


def test_gather_and_lineage():
    src = np.arange(2 * 3 * 2 * 5, dtype=np.float32).reshape(12, 5)                  # 2 groups of 3 particles of 2 images
    anc = np.array([2, 2, 0, 1, 7, -4], np.int32)                                    # (out of range: clamped)
    out = ref.gather(src, anc, 3, 2)
    rows = [4, 5, 4, 5, 0, 1, 8, 9, 10, 11, 6, 7]
    assert np.array_equal(out, src[rows])
    assert np.array_equal(ref.gather(src, np.tile(np.arange(3), 2), 3, 2), src)
    lin = ref.lineage([np.array([0, 0, 2]), np.array([1, 2, 2])], 3)
    assert lin.tolist() == [[0, 2, 2]]                                               # final 0 <- particle 1 of event 2 <- particle 0 of event 1


def test_x0_is_the_threshold_restatements_x0():
    import threshold_ref
    tab = threshold_ref.table_of(dpm_ref.alpha_bar().astype(np.float32))
    g = np.random.default_rng(2)
    x, eps = g.standard_normal((3, 9)).astype(np.float32), g.standard_normal((3, 6)).astype(np.float32)
    t = np.array([5, 7, 7, 2000, 7, 7, -3], np.int64)
    got = ref.x0(x, eps, t, tab, 3)
    for r, tv in enumerate((5, 999, 0)):
        want = (tab[tv, 0] * x[r, :6]).astype(np.float32) - (tab[tv, 1] * eps[r]).astype(np.float32)
        assert np.array_equal(got[r].view(np.uint32), want.view(np.uint32))


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
    assert _lib.SIGNATURES["pf_steer_resample"] == (C.c_int, [C.POINTER(_lib.SteerResampleArgs), C.c_void_p])
    assert int(re.search(r"#define PF_STEER_MAX_N (\d+)", hdr).group(1)) == _lib.STEER_MAX_N == ref.MAX_N == 256
    assert int(re.search(r"#define PF_GATHER_MAX_TENSORS (\d+)", hdr).group(1)) == _lib.GATHER_MAX_TENSORS == 4
    assert "0x53544552" in full and "a zero-weight particle is never chosen" in full and "Singhal" in full
    from polyffusion_amd.build import SOURCES
    assert "steer.hip" in SOURCES
    # one device function for the predicted x0, in a header both kernels include
    csrc = os.path.join(REPO, "polyffusion_amd", "csrc")
    for f in ("steer.hip", "x0_threshold.hip"):
        src = open(os.path.join(csrc, f)).read()
        assert '#include "x0_predict.h"' in src and "x0_of(" in src


def test_the_structs_are_laid_out_as_the_header_says():
    hdr = open(os.path.join(REPO, "include", "pfhip.h")).read()
    types = r"(?:float|double|void|size_t|int32_t|int64_t|uint64_t)"

    def order_of(name):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return [re.sub(r"\[.*\]", "", n).strip(" *") for decl in re.findall(r"(?:const )?" + types + r"\s*\*?\s*([^;]+);", body) for n in decl.split(",")]

    f = _lib.X0PredictArgs
    assert order_of("pf_x0_predict_args") == [n for n, _ in f._fields_]
    assert [getattr(f, n).offset for n, _ in f._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72] and C.sizeof(f) == 80
    f = _lib.SteerResampleArgs
    names = order_of("pf_steer_resample_args")
    assert [("lam" if n == "lambda" else n) for n in names] == [n for n, _ in f._fields_]
    assert [getattr(f, n).offset for n, _ in f._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 84] and C.sizeof(f) == 88
    f = _lib.RowsGatherArgs
    assert order_of("pf_rows_gather_args") == [n for n, _ in f._fields_]
    assert [getattr(f, n).offset for n, _ in f._fields_] == [0, 32, 64, 96, 104, 112, 116, 120] and C.sizeof(f) == 128


def test_bad_arguments_are_refused_before_any_launch(lib):
    """No GPU needed: the calls return before they touch HIP or any of the (fake) device pointers."""
    P = [FAKE + i * 0x100000 for i in range(12)]

    def refused(fn, struct, prefix, defaults, pattern, **fields):
        a = struct()
        for k, v in {**defaults, **fields}.items():
            if isinstance(v, (list, tuple)):
                for i, e in enumerate(v):
                    getattr(a, k)[i] = e
            else:
                setattr(a, k, v)
        rc = fn(C.byref(a), None)
        msg = lib.pf_last_error().decode()
        assert rc == -1 and msg.startswith(prefix) and re.search(pattern, msg), (fields, rc, msg)

    base = dict(x=P[0], x_row_stride=8, eps=P[1], t=P[2], t_stride=1, table=P[3], n_table=1000, x0=P[4], rows=2, row_elems=8)
    no = lambda pattern, **kw: refused(lib.pf_x0_predict, _lib.X0PredictArgs, "x0_predict: ", base, pattern, **kw)
    for name in ("x", "eps", "t", "table", "x0"):
        no("null x, eps, t, table or x0", **{name: None})
    no("0 rows", rows=0)
    no("of 0 elements", row_elems=0)
    no("x_row_stride 7 below row_elems 8", x_row_stride=7)
    no("t_stride -1", t_stride=-1)
    no("n_table 0", n_table=0)
    no("x0 overlaps eps", x0=P[1] + 4)
    no("x0 overlaps x", x0=P[0] + (12 + 8) * 4 - 4, x_row_stride=12)
    no("x0 overlaps table", x0=P[3] + 1000 * 16 - 4)
    no("x0 overlaps t", x0=P[2] + 3 * 8, t_stride=3)
    assert lib.pf_x0_predict(None, None) == -1 and lib.pf_last_error().decode().startswith("x0_predict: ")

    base = dict(reward=P[0], base=P[1], lam=5.0, ess_frac=0.5, seed=1, group_offset=0, event=0, ancestors=P[2], weights=P[3], stats=P[4], groups=2, n=8)
    no = lambda pattern, **kw: refused(lib.pf_steer_resample, _lib.SteerResampleArgs, "steer_resample: ", base, pattern, **kw)
    for name in ("reward", "base", "ancestors", "weights", "stats"):
        no("null reward, base, ancestors, weights or stats", **{name: None})
    no("0 groups", groups=0)
    for bad in (0, -1, 257):
        no(rf"{bad} particles per group outside \[1, 256\]", n=bad)
    for bad in (-1.0, math.nan, math.inf):
        no("lambda .* is not finite and >= 0", lam=bad)
    for bad in (0.0, -0.5, 1.0000001, math.nan):
        no(r"ess_frac .* outside \(0, 1\]", ess_frac=bad)
    no("must be 8-byte aligned", reward=P[0] + 4)
    no("must be 8-byte aligned", stats=P[4] + 4)
    no("ancestors 4-byte aligned", ancestors=P[2] + 2)
    no("reward overlaps base", base=P[0] + 8)
    no("base overlaps weights", weights=P[1] + 15 * 8)
    no("ancestors overlaps stats", stats=P[2] + 8 * 7)
    assert lib.pf_steer_resample(None, None) == -1 and lib.pf_last_error().decode().startswith("steer_resample: ")

    base = dict(src=[P[0], P[1]], dst=[P[2], P[3]], row_elems=[8, 6], n_tensors=2, ancestors=P[4], groups=2, n=3, per=2)
    no = lambda pattern, **kw: refused(lib.pf_rows_gather, _lib.RowsGatherArgs, "rows_gather: ", base, pattern, **kw)
    no("null ancestors", ancestors=None)
    for bad in (0, 5):
        no(rf"{bad} tensors outside \[1, 4\]", n_tensors=bad)
    no("0 groups of 3 particles of 2 images", groups=0)
    no("2 groups of 0 particles", n=0)
    no("of 0 images", per=0)
    no("null src or dst of tensor 1", src=[P[0], None])
    no("null src or dst of tensor 0", dst=[None, P[3]])
    no("rows of 0 elements in tensor 1", row_elems=[8, 0])
    no("src and dst of tensor 0 must be 4-byte aligned", src=[P[0] + 2, P[1]])
    no("dst of tensor 0 overlaps src of tensor 0", dst=[P[0] + 12 * 8 * 4 - 4, P[3]])
    no("dst of tensor 1 overlaps src of tensor 0", dst=[P[2], P[0]])
    no("dst of tensor 0 overlaps dst of tensor 1", dst=[P[3] + 4, P[3]])
    no("dst of tensor 0 overlaps ancestors", ancestors=P[2] + 8)
    no("more workgroups than one launch holds", groups=2 ** 20, n=256, per=4, row_elems=[2 * _lib.MSE_CHUNK + 1, 6], dst=[FAKE + 2 ** 50, FAKE + 2 ** 52])
    assert lib.pf_rows_gather(None, None) == -1 and lib.pf_last_error().decode().startswith("rows_gather: ")


# ---------------------------------------------------------------------------------------------- the setting and the samplers
class Schedule:
    """What the samplers read of a LatentDiffusion: the step count and the float32 schedule."""

    def __init__(self):
        self.n_steps = 1000
        self.alpha_bar = torch.from_numpy(dpm_ref.alpha_bar().astype(np.float32))
        self.beta = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000) ** 2
        self.eps_model = None


def test_the_dataclass_validates_its_fields_and_spells_its_label():
    from polyffusion_amd.sampler import STEER_REWARDS, Steering
    fn = lambda x0: x0.sum((1, 2, 3)).double()
    st = Steering(n=4, reward=fn)
    assert (st.per, st.lam, st.every, st.window, st.ess) == (1, 10.0, 5, (0.0, 1.0), 0.5) and st.label == "steer=fn,lam=10.0"
    assert sorted(STEER_REWARDS) == ["bass", "chord", "integrity", "texture"] and STEER_REWARDS["integrity"][1] < 0
    st = Steering(n=3, reward="integrity", per=2, lam=0, every=1, window=(0.25, 0.75), ess=1)
    assert st.label == "steer=integrity,lam=0.0,every=1,win=0.25-0.75,ess=1.0" and st.window_values(1000) == (250, 749)
    assert Steering(n=256, reward=fn).n == 256 and Steering(n=1, reward=fn).window_values(1000) == (0, 999)
    chord = torch.zeros(1, 32, 36)
    assert Steering(n=2, reward="chord", chord=chord).reward == "chord" and Steering(n=2, reward="texture", onsets=torch.zeros(1, 128)).per == 1
    for kw in (dict(n=0), dict(n=257), dict(n=2.5), dict(per=0), dict(every=0), dict(lam=-1), dict(lam=math.inf), dict(lam=math.nan), dict(ess=0), dict(ess=1.5),
               dict(ess=math.nan), dict(window=(0.5, 0.25)), dict(window=(-0.1, 1)), dict(window=3), dict(reward="extracted"), dict(reward="chord"),
               dict(reward="bass"), dict(reward="texture")):
        with pytest.raises(ValueError, match="steering"):
            Steering(**{**dict(n=4, reward=fn), **kw})


def test_the_samplers_take_the_setting_and_refuse_what_cannot_be_steered(lib):
    from polyffusion_amd.sampler import DDIMSampler, DPMSolverSampler, SDFSampler, Steering
    st = Steering(n=2, reward=lambda x0: x0.sum((1, 2, 3)).double())
    s = SDFSampler(Schedule(), steering=st)
    assert s.steering is st and s.last_steering is None and SDFSampler(Schedule()).steering is None
    assert DDIMSampler(Schedule(), 10, "uniform", 1.0, steering=st).steering is st
    for make, said in ((lambda: SDFSampler(Schedule(), graph=True, steering=st), "graph=True"),
                       (lambda: DDIMSampler(Schedule(), 10, "uniform", 0.0, steering=st), "ddim_eta == 0"),
                       (lambda: DPMSolverSampler(Schedule(), 10, steering=st), "deterministic"),
                       (lambda: SDFSampler(Schedule(), noise_fn=lambda shape: torch.zeros(shape), steering=st), "noise_fn"),
                       (lambda: SDFSampler(Schedule(), steering=0.5), "expected None or a Steering")):
        with pytest.raises(ValueError, match="steering"):
            make()
        try:
            make()
        except ValueError as e:
            assert said in str(e)
    for s in (DDIMSampler(Schedule(), 10, "uniform", 0.0), DPMSolverSampler(Schedule(), 10)):
        with pytest.raises(ValueError, match="steering"):
            s.steering = st
        assert s.steering is None                                                   # a refused value changes nothing
    s = SDFSampler(Schedule(), steering=st, sample_offset=4)
    x = torch.zeros(3, 2, 8, 8)
    with pytest.raises(ValueError, match="not whole groups of 2 particles"):
        s._steer_begin(x)
    with pytest.raises(ValueError, match="repaint_n 2"):
        s._steer_begin(torch.zeros(4, 2, 8, 8), 2)
    with pytest.raises(ValueError, match="not whole groups"):
        SDFSampler(Schedule(), steering=st, sample_offset=3)._steer_begin(torch.zeros(4, 2, 8, 8))
    ctx = s._steer_begin(torch.zeros(4, 2, 8, 8))
    assert ctx["group_offset"] == 2 and ctx["window"] == (0, 999) and s.last_steering.lineage().tolist() == [[0, 1], [0, 1]]
    # the host's decision: the every-th step of the loop, inside the window, not the last
    ctx = dict(st=Steering(n=2, reward=st.reward, every=3), window=(100, 500))
    got = [i for i in range(12) if SDFSampler._steered_at(ctx, i, 600 - 50 * i, i == 11)]
    assert got == [2, 5, 8]


# ---------------------------------------------------------------------------------------------- the CLI
def test_cli_flags_defaults_and_refusals():
    from polyffusion_amd import inference_sdf
    p, check = inference_sdf.make_parser(), inference_sdf.check_steer_args
    a = p.parse_args([])
    assert (a.steer, a.steer_by, a.steer_lambda, a.steer_every, a.steer_window, a.steer_ess) == (False, None, 10.0, 5, None, 0.5) and check(a) is None
    assert check(p.parse_args(["--best_of", "3", "--steer"]), "chord") == dict(reward="chord", lam=10.0, every=5, window=(0.0, 1.0), ess=0.5)
    got = check(p.parse_args(["--best_of", "4", "--steer", "--rank_by", "integrity", "--steer_lambda", "3", "--steer_every", "2", "--steer_window", "0.1", "0.9",
                              "--steer_ess", "1", "--ddim", "--ddim_eta", "1", "--joint"]), "chord")
    assert got == dict(reward="integrity", lam=3.0, every=2, window=(0.1, 0.9), ess=1.0)
    assert check(p.parse_args(["--best_of", "2", "--steer", "--rank_by", "extracted", "--steer_by", "bass"]), "chord")["reward"] == "bass"
    assert check(p.parse_args(["--best_of", "2", "--steer", "--inpaint_type", "below"]), "chord")["reward"] == "chord"
    for bad, said in ((["--steer"], "--best_of N with N > 1"), (["--steer_lambda", "3"], "belong to --steer"), (["--best_of", "2", "--steer_by", "bass"], "belong to --steer"),
                      (["--best_of", "2", "--steer", "--autoreg"], "--autoreg"), (["--best_of", "2", "--steer", "--dpm"], "--dpm"),
                      (["--best_of", "2", "--steer", "--ddim"], "eta 0"), (["--best_of", "2", "--steer", "--hip_graph"], "--hip_graph"),
                      (["--best_of", "2", "--steer", "--rank_by", "extracted"], "no steering reward"),
                      (["--best_of", "2", "--steer", "--rank_by", "novelty", "--novelty_corpus", "x"], "no steering reward"),
                      (["--best_of", "2", "--steer", "--steer_lambda", "-1"], "finite and >= 0"), (["--best_of", "2", "--steer", "--steer_lambda", "nan"], "finite and >= 0"),
                      (["--best_of", "2", "--steer", "--steer_every", "0"], "at least 1"), (["--best_of", "2", "--steer", "--steer_ess", "0"], "in (0, 1]"),
                      (["--best_of", "2", "--steer", "--steer_window", "0.6", "0.5"], "0 <= LO <= HI <= 1"), (["--best_of", "300", "--steer"], "at most 256"),
                      (["--best_of", "2", "--steer", "--repaint_n", "2"], "--repaint_n")):
        with pytest.raises(SystemExit) as e:
            check(p.parse_args(bad), "chord")
        assert said in str(e.value), bad
    with pytest.raises(SystemExit, match="texture song of a chord\\+txt model"):
        check(p.parse_args(["--best_of", "2", "--steer", "--steer_by", "texture"]), "chord")
    with pytest.raises(SystemExit, match="needs the chords of the run"):
        check(p.parse_args(["--best_of", "2", "--steer"]), "txt")
    # through main(): refused before the GPU, the parameters or the weights are looked at
    with pytest.raises(SystemExit, match="--hip_graph"):
        inference_sdf.main(["--best_of", "2", "--steer", "--hip_graph", "--params_preset", "sdf_chd8bar", "--synthetic_weights", "--synthetic"])


def test_the_stamp_names_the_setting_only_when_set(lib):
    from polyffusion_amd.inference_sdf import Experiments
    from polyffusion_amd.sampler import SDFSampler, Steering
    cut = lambda s: s[: s.rindex("_", 0, s.rindex("_"))]                         # without the date and time
    s = SDFSampler(Schedule())
    e = Experiments("m", dict(n_steps=1000), s, t_idx=3)
    assert cut(e._stamp(5.0, False)) == "m[scale=5.0]"
    s.steering = Steering(n=3, reward="integrity", lam=2.5, every=2)
    assert cut(e._stamp(5.0, False)) == "m[scale=5.0,steer=integrity,lam=2.5,every=2]"
    assert cut(e._stamp(5.0, False, "", "mean")) == "m[scale=5.0,joint,steer=integrity,lam=2.5,every=2]"
    s.steering = None
    assert cut(e._stamp(5.0, False)) == "m[scale=5.0]"


def test_sharding_by_groups_keeps_every_candidates_global_index():
    from polyffusion_amd import dist as pfdist
    from polyffusion_amd.inference_sdf import steer_shard
    for num in (1, 2, 3, 5, 8):
        for n in (2, 3, 4):
            for world in (1, 2, 3, 4, 8):
                got = []
                for rank in range(world):
                    lo, hi = steer_shard(num, n, rank, world)
                    assert lo % n == 0 and hi % n == 0 and (lo // n, hi // n) == pfdist.shard_range(num, rank, world)
                    got += list(range(lo, hi))                                       # candidate lo + k of rank `rank` is global candidate lo + k
                assert got == list(range(num * n))
    # where the plain split would cut a group in two
    assert pfdist.shard_range(3 * 2, 0, 2) == (0, 3) and steer_shard(3, 2, 0, 2) == (0, 4) and steer_shard(3, 2, 1, 2) == (4, 6)
