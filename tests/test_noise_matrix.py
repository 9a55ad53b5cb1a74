"""The noise matrix without a GPU (tests/noise_matrix.py): the integer Philox4x32-10 reproduces the Random123 known-answer vectors, the fp32
uniform mapping is what the module says it is (u = 1.0 at m = 2^24 - 1, u >= 2^-25 always), the float64 oracle agrees with an independent
statement of Box-Muller, the table reaches every branch it lists, the undefective fp32 emulator is inside the measured constant on every
case and every listed defect, switched on in the emulator, leaves the tolerance on a case that names the defect's branch - so the tolerance
tests/test_gpu_noise_matrix.py holds the kernels to passes a correct generator and rejects a subtly wrong one.  The committed tail constants
are true of the integer reference, the oracle's own normals have a Gaussian's moments, and the recorded constant equals
profiles/noise_error_model.md and what the table measures."""
import math
import os
import re
import sys

import numpy as np
import pytest

import noise_matrix as nm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = nm.cases()
SMALL = [(k, s) for k, s in ALL if s.n <= 1 << 16]
_measured = {}


def measured(key, s):
    """the undefective emulator's largest error in units, once per case"""
    if key not in _measured:
        _measured[key] = nm.unit_ratio(nm.emulate(s), nm.oracle(s))
    return _measured[key]


def test_philox_reproduces_the_known_answer_vectors():
    for ctr, key, want in nm.KAT:
        assert nm.philox4x32(ctr, key) == want
        assert tuple(int(v) for v in nm.philox_np(ctr, key)) == want
    assert nm.philox4x32(*nm.KAT[0][:2], rounds=9) != nm.KAT[0][2]
    assert nm.counters(0x1122334455667788, 0x99AABBCCDDEEFF00, 0x0123456789ABCDEF) == (
        (0x89ABCDEF, 0x01234567, 0xDDEEFF00, 0x99AABBCC), (0x55667788, 0x11223344))


def test_the_vectorised_philox_is_the_integer_reference():
    rng = np.random.Generator(np.random.PCG64(11))
    for _ in range(6):
        seed, draw = (int(v) for v in rng.integers(0, 1 << 64, 2, dtype=np.uint64))
        g = rng.integers(0, 1 << 62, 64, dtype=np.uint64)
        w = nm.words(seed, draw, g)
        assert w.dtype == np.uint64 and w.shape == (64, 4) and int(w.max()) <= nm.M32
        for i in (0, 31, 63):
            assert tuple(int(v) for v in w[i]) == nm.group_words(seed, draw, int(g[i]))


def test_the_uniform_mapping_is_the_fp32_one():
    top = (1 << 24) - 1
    ms = [0, 1, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, top - 1, top]
    got = nm.uniform32(np.array(ms, np.uint64))
    assert got.dtype == np.float32
    assert [float(v) for v in got] == [nm.uniform_exact(m) for m in ms]
    assert float(got[0]) == 2.0 ** -25 and float(got[1]) == 3 * 2.0 ** -25 and float(got[2]) == 0.5 - 2.0 ** -25
    assert float(got[3]) == 0.5                              # 2^23 + 1/2 is a tie: to the even 2^23
    assert float(got[4]) == 0.5 + 2.0 ** -23                 # 2^23 + 1 + 1/2: to the even 2^23 + 2
    assert float(got[5]) == 1.0 - 2.0 ** -23 and float(got[6]) == 1.0
    rng = np.random.Generator(np.random.PCG64(5))
    m = np.concatenate([rng.integers(0, 1 << 24, 4096, dtype=np.uint64), np.arange((1 << 23) - 8, (1 << 23) + 8, dtype=np.uint64)])
    u = nm.uniform32(m)
    assert [float(v) for v in u] == [nm.uniform_exact(int(v)) for v in m]
    assert float(u.min()) >= 2.0 ** -25 and float(u.max()) <= 1.0
    hi = u[m >= 1 << 23].astype(np.float64) * 2.0 ** 23
    assert np.array_equal(hi, np.round(hi))                  # the grid of 2^-23 in [0.5, 1]
    # the largest radius, and the exact zero
    o = nm.oracle_groups(np.array([[2.0 ** -25, 0.0, 1.0, 0.25]], np.float32))
    assert abs(o.z[0, 0] - math.sqrt(50 * math.log(2))) < 1e-14 and o.z[0, 2] == 0 and o.z[0, 3] == 0
    assert o.unit[0, 2] == 0 and o.unit[0, 3] == 0


def _independent(u0, u1):
    """(r cos, r sin) of one pair by another route: mpmath at 40 digits where it is installed, else Python's math on doubles"""
    try:
        import mpmath
    except ImportError:
        r, th = math.sqrt(-2.0 * math.log(u0)), float(nm.TWO_PI32) * u1
        return r * math.cos(th), r * math.sin(th)
    with mpmath.workdps(40):
        r, th = mpmath.sqrt(-2 * mpmath.log(mpmath.mpf(u0))), mpmath.mpf(float(nm.TWO_PI32)) * mpmath.mpf(u1)
        return float(r * mpmath.cos(th)), float(r * mpmath.sin(th))


def test_the_oracle_agrees_with_an_independent_float64_statement():
    groups = list(range(48)) + [g for found in nm.TAILS.values() for g, _, _ in found] + [(1 << 32) - 1, 1 << 32, (1 << 61) + 12345]
    for seed, draw in ((nm.SEED0, nm.DRAW0), (nm.SEEDS[4], nm.DRAWS[4])):
        for g in groups:
            u = [nm.uniform_exact(w >> 8) for w in nm.group_words(seed, draw, g)]
            want = _independent(u[0], u[1]) + _independent(u[2], u[3])
            s = nm.Spec(seed=seed, draws=draw, slot=0, off=4 * g, n=4)
            o = nm.oracle(s)
            for j in range(4):
                # float64 log, sqrt, cos / sin and two products: a few ulps of the value; a cosine next to its zero is as good (the
                # angle is exact), an exact zero is exact
                assert abs(o.z[j] - want[j]) <= 16 * 2.0 ** -53 * abs(want[j]), (seed, draw, g, j)
                assert o.unit[j] >= nm.U * abs(o.z[j])


def test_keys_are_unique_and_every_case_says_why_it_exists():
    keys = [k for k, _ in ALL]
    assert len(keys) == len(set(keys))
    reached, named = set(), set()
    for key, s in ALL:
        assert s.why, key
        b = nm.branches_of(s)
        assert set(s.why) <= b, (key, set(s.why) - b)
        reached |= b
        named |= set(s.why)
        if s.kind in nm.VEC4:
            assert s.off % 4 == 0 and s.get("row_elems", s.n) % 4 == 0, key
    assert nm.REQUIRED <= reached, nm.REQUIRED - reached
    assert set(nm.DEFECT_BRANCH) == set(nm.DEFECTS) and set(nm.DEFECT_BRANCH.values()) <= named


def test_the_cases_are_the_issue_s():
    """the sizes and counter words the table must hold, spelled out once more against the specs themselves"""
    rn = [s for _, s in ALL if s.kind == "randn"]
    assert {(s.off % 4, s.n) for s in rn} >= {(k, n) for k in range(4) for n in (1, 2, 3, 4, 5, 7, 8, 4097)}
    assert any(s.n == 2048 * 256 * 4 + 4 * 256 + 5 and s.off % 2 for s in rn)
    assert any(s.off == (1 << 34) - 4 and s.n == 8 for s in rn) and any(s.off == (1 << 40) + 3 for s in rn)
    assert {(s.draws, s.seed) for s in rn} >= {(d, sd) for d in (0, 1, (1 << 32) - 1, 1 << 32, (1 << 63) + 5) for sd in nm.SEEDS}
    assert nm.SEEDS[:4] == (0, 1, (1 << 32) - 1, 1 << 32) and nm.SEEDS[4] >> 32 and nm.SEEDS[4] & nm.M32
    for (ctr, key, _), (seed, draw, g) in zip(nm.KAT, nm.kat_triples()):
        got_ctr, got_key = nm.counters(seed, draw, g)
        assert got_key == key and got_ctr[2:] == ctr[2:] and got_ctr[0] == ctr[0] and got_ctr[1] == ctr[1] & ((1 << (nm.KAT_GROUP_BITS - 32)) - 1)
        assert any(s.off == 4 * g and s.seed == seed and s.draws == draw for s in rn)
    dev = [s for _, s in ALL if s.kind == "randn_dev"]
    assert {(s.draws, s.slot) for s in dev} == {(d, k) for d in (0, 5, (1 << 32) - 1) for k in (0, 1, 2)}
    variants = {(s.kind, s.get("variant")) for _, s in ALL}
    assert variants >= {("ddpm", "plain"), ("ddpm", "q"), ("ddpm", "p"), ("ddpm", "state_q"), ("ddpm", "state_p"), ("ddim", "plain")}
    for kind in ("ddpm", "ddim"):
        assert {s.n for _, s in ALL if s.kind == kind} >= {8, 2048 * 256 * 4 + 1024}
    for kind in ("qsample", "mse"):
        assert {(s.rows, s.row_elems) for _, s in ALL if s.kind == kind} >= {(2, 8), (2, 4 * 256 + 4)}
        assert all(s.off for _, s in ALL if s.kind == kind)
    for kind in ("gauss", "rsample"):
        assert {s.off % 4 for _, s in ALL if s.kind == kind} == {0, 1, 2, 3}


@pytest.mark.parametrize("key,s", ALL, ids=[k for k, _ in ALL])
def test_the_emulated_kernel_is_inside_the_measured_constant(key, s):
    e, o = nm.emulate(s), nm.oracle(s)
    assert e.dtype == np.float32 and e.shape == (s.n,) and o.z.shape == (s.n,) and o.z.dtype == np.float64
    assert np.isfinite(e).all() and np.isfinite(o.z).all()
    r = _measured[key] = nm.unit_ratio(e, o)
    assert r <= nm.M / nm.MARGIN, (key, r)
    assert nm.ratio(e, o) <= 1.0 / nm.MARGIN
    if s.kind == "mse":
        want, t = nm.mse_oracle(s, o)
        got = (e.astype(np.float64) ** 2).reshape(s.rows, s.row_elems).sum(1)
        assert (np.abs(got - want) <= t).all() and (t < 1e-4 * want).all()


@pytest.mark.parametrize("defect", nm.DEFECTS)
def test_every_defect_is_caught_by_a_case_that_names_its_branch(defect):
    branch = nm.DEFECT_BRANCH[defect]
    named = [(k, s) for k, s in SMALL if branch in s.why]
    assert named, f"no case names the branch '{branch}'"
    caught = [k for k, s in named if nm.ratio(nm.emulate(s, defect), nm.oracle(s)) > 1.0]
    assert caught, f"no case that names '{branch}' rejects the defect '{defect}'"
    print(f"{defect}: rejected by {len(caught)} of {len(named)} case(s) that name {branch}, first {caught[0]}")


def test_the_committed_tail_constants_are_true():
    assert set(nm.TAILS) == set(nm.TAIL_WANT)
    top = (1 << 24) - 1
    for name, found in nm.TAILS.items():
        assert found, name
        for g, j, m in found:
            assert nm.group_words(nm.SEED0, nm.DRAW0, g)[j] >> 8 == m and nm.TAIL_WANT[name](j, m), (name, g)
            assert any(s.kind == "randn" and s.off == 4 * g and s.n == 4 and f"tail:{name}" in s.why for _, s in ALL), (name, g)
    assert all(m <= 8 and j in (0, 2) for _, j, m in nm.TAILS["small_m"]) and len(nm.TAILS["small_m"]) >= 4
    assert all(m == top and j in (0, 2) for _, j, m in nm.TAILS["u_one"])
    assert all(m == top and j in (1, 3) for _, j, m in nm.TAILS["angle_2pi"])
    # what they are for: an exact zero pair (the emulator's is +-0 too), the largest radii, the angle fp32(2 pi)
    g, j, _ = nm.TAILS["u_one"][0]
    s = nm.Spec(seed=nm.SEED0, draws=nm.DRAW0, slot=0, off=4 * g, n=4)
    o, e = nm.oracle(s), nm.emulate(s)
    assert o.z[j] == 0 and o.z[j + 1] == 0 and e[j] == 0 and e[j + 1] == 0 and nm.tol(o)[j] == 0 and o.z[2 - j] != 0
    for g, j, m in nm.TAILS["small_m"]:
        z = nm.oracle(nm.Spec(seed=nm.SEED0, draws=nm.DRAW0, slot=0, off=4 * g, n=4)).z
        assert abs(math.hypot(z[j], z[j + 1]) - math.sqrt(-2 * math.log((2 * m + 1) * 2.0 ** -25))) < 1e-12 and math.hypot(z[j], z[j + 1]) > 5.38
    g, j, _ = nm.TAILS["angle_2pi"][0]
    z = nm.oracle(nm.Spec(seed=nm.SEED0, draws=nm.DRAW0, slot=0, off=4 * g, n=4)).z
    assert 0 < z[j] < 2e-7 * abs(z[j - 1])                   # sin(fp32(2 pi)) = fp32(2 pi) - 2 pi = 1.75e-7


def test_the_oracle_s_own_normals_have_a_gaussian_s_moments():
    """the reference, not the kernel: 2^20 normals of one draw within 5 sigma of the sampling error of a true Gaussian"""
    n = 1 << 20
    z = nm.oracle(nm.Spec(seed=nm.SEED0, draws=nm.DRAW0, slot=0, off=0, n=n)).z
    five = 5.0 / math.sqrt(n)
    assert abs(z.mean()) < five                              # Var z = 1
    assert abs((z ** 2).mean() - 1) < five * math.sqrt(2)    # Var z^2 = 2
    assert abs((z ** 3).mean()) < five * math.sqrt(15)       # Var z^3 = 15
    assert abs((z ** 4).mean() - 3) < five * math.sqrt(96)   # Var z^4 = 105 - 9
    for lag in (1, 2, 3, 4):                                 # neighbours, the partner of a pair, the next group: Var z z' = 1
        assert abs((z[:-lag] * z[lag:]).mean()) < five
    assert abs(z).max() < math.sqrt(50 * math.log(2)) + 1e-9


def test_the_recorded_constant_is_the_profile_s_and_what_the_table_measures():
    """profiles/noise_error_model.md holds what tools/noise_error_model.py measured; noise_matrix.MEASURED equals it and the table's maximum
    (the tool's run of 2^22 consecutive groups stays below the table's largest launch)"""
    sys.path.insert(0, REPO)
    from tools import noise_error_model as tool
    text = open(tool.OUT).read()
    row = re.search(r"^\| ([0-9.]+) \| [0-9.]+ \| [0-9.]+ \|", text, flags=re.M)
    assert row is not None and float(row.group(1)) == nm.MEASURED
    worst = max(measured(k, s) for k, s in ALL)
    assert tool.up2(worst) == nm.MEASURED, worst
    for name, found in nm.TAILS.items():
        for g, _, _ in found:
            assert f"| {name} | {g} |" in text
    assert nm.M == nm.MARGIN * nm.MEASURED and nm.MARGIN == 4.0 and nm.FINAL == 1.0
    assert "No number here comes from a GPU" in text and "u = 1.0" in text
