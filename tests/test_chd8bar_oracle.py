"""tests/chd8bar_ref.py (the numpy float64 restatement of ``Chord_8Bar``) against tests/golden/chd8bar.npz, the arrays
tools/make_goldens_chd8bar.py recorded from the reference's own modules - and what of the product needs no GPU: the teacher-forcing
schedule and the order in which ``get_loss_dict`` draws its coin flips.

Measured when the fixture was made (float64 restatement against the reference's float64 run, both nets): Normal mean 1.4e-16, scale
2.2e-16, z 8.9e-16; logits 1.8e-15 (row by row, three masks, and the batch of 4); losses 1.8e-15.  The bounds below are ten times
those, far under the cap of 1e-9.
"""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chd8bar_ref as R  # noqa: E402

TOL_DIST, TOL_LOGITS, TOL_LOSS = 1e-14, 2e-14, 2e-14
MASKS = ("m0", "mh", "m1")
LOGITS = ("root", "chroma", "bass")
KEYS = ("loss", "root", "chroma", "bass")


@pytest.fixture(scope="module")
def g():
    return R.fixture()


@pytest.fixture(scope="module", params=sorted(R.NETS))
def net(request, g):
    """One net's states, chords and the float64 z of the whole pool from the restated encoder (shared; never modified)."""
    tag = request.param
    est, dst = R.states(R.NETS[tag], int(g["seed_w"]))
    chord = g[f"{tag}_chord"].astype(np.float64)
    mean, scale = R.encoder_dist(est, chord)
    return dict(tag=tag, est=est, dst=dst, chord=chord, mean=mean, scale=scale, z=mean + scale * g[f"{tag}_noise"].astype(np.float64))


def test_fixture_is_what_the_generator_promises(g):
    assert float(g["min_gap"]) == 1e-3
    assert float(g["ref_f32_f64_logits"]) < 1e-6 and float(g["ref_f32_f64_loss"]) < 2e-6
    for tag, n in (("s", 8), ("c", 32)):
        assert g[f"{tag}_chord"].shape == (32, n, 36) and g[f"{tag}_noise"].dtype == np.float32
        for mk in MASKS:
            assert float(g[f"{tag}_{mk}_margin"]) >= 1e-3 and g[f"{tag}_{mk}_rows"].shape == (8,)
            assert g[f"{tag}_{mk}_root64"].shape == (8, n, 12) and g[f"{tag}_{mk}_chroma32"].shape == (8, n, 12, 2)
            assert g[f"{tag}_{mk}_flips"].shape == (n - 1,)
        assert not g[f"{tag}_m0_flips"].any() and g[f"{tag}_m1_flips"].all()
        assert g[f"{tag}_mh_flips"].any() and not g[f"{tag}_mh_flips"].all()
        assert float(g[f"{tag}_b4_margin"]) >= 1e-3 and g[f"{tag}_b4_root64"].shape == (4, n, 12)
    assert os.path.getsize(R.GOLDEN) <= 1_000_000


def test_restated_normal_equals_the_reference(g, net):
    tag = net["tag"]
    e = [np.abs(net[k][:4] - g[f"{tag}_{n}"]).max() for k, n in (("mean", "mean64"), ("scale", "scale64"), ("z", "z64_head"))]
    print(f"net {tag}: restated Normal vs reference float64: mean {e[0]:.2e} scale {e[1]:.2e} z {e[2]:.2e}")
    assert max(e) <= TOL_DIST
    assert np.abs(net["z"] - g[f"{tag}_z32"]).max() <= 1e-5          # the float32 z of the whole pool is the same sample


@pytest.mark.parametrize("mk", MASKS)
def test_restated_forced_decode_and_loss_equal_the_reference_row_by_row(g, net, mk):
    tag = net["tag"]
    rows, flips = g[f"{tag}_{mk}_rows"], g[f"{tag}_{mk}_flips"]
    logits = R.decode_forced(net["dst"], net["z"][rows], net["chord"][rows], flips, "row")
    e = max(np.abs(a - g[f"{tag}_{mk}_{n}64"]).max() for a, n in zip(logits, LOGITS))
    loss = np.array([[R.chord_loss(net["chord"][r:r + 1], *[a[i:i + 1] for a in logits])[k] for k in KEYS] for i, r in enumerate(rows)])
    e_loss = np.abs(loss - g[f"{tag}_{mk}_loss64"]).max()
    print(f"net {tag} mask {mk}: restatement vs reference float64: logits {e:.2e} loss {e_loss:.2e}")
    assert e <= TOL_LOGITS and e_loss <= TOL_LOSS
    assert R.min_margin(*logits).min() >= 1e-3
    # batch feedback at batch 1 is row feedback
    one = R.decode_forced(net["dst"], net["z"][rows[:1]], net["chord"][rows[:1]], flips, "batch")
    assert all(np.array_equal(a, b[:1]) for a, b in zip(one, R.decode_forced(net["dst"], net["z"][rows[:1]], net["chord"][rows[:1]], flips, "row")))


def test_restated_batch_feedback_equals_the_reference_batch_of_4(g, net):
    tag = net["tag"]
    rows, flips = g[f"{tag}_b4_rows"], g[f"{tag}_mh_flips"]
    logits = R.decode_forced(net["dst"], net["z"][rows], net["chord"][rows], flips, "batch")
    e = max(np.abs(a - g[f"{tag}_b4_{n}64"]).max() for a, n in zip(logits, LOGITS))
    d = R.chord_loss(net["chord"][rows], *logits)
    e_loss = np.abs(np.array([d[k] for k in KEYS]) - g[f"{tag}_b4_loss64"]).max()
    print(f"net {tag} batch of 4: restatement vs reference float64: logits {e:.2e} loss {e_loss:.2e}")
    assert e <= TOL_LOGITS and e_loss <= TOL_LOSS
    # and the union is not a detail: the same rows decoded one by one differ by far more than any tolerance here
    row = R.decode_forced(net["dst"], net["z"][rows], net["chord"][rows], flips, "row")
    assert max(np.abs(a - b).max() for a, b in zip(logits, row)) > 1e-3
    # an all-ones mask feeds nothing back: both forms are the same arithmetic
    ones = [True] * len(flips)
    assert all(np.array_equal(a, b) for a, b in zip(R.decode_forced(net["dst"], net["z"][rows], net["chord"][rows], ones, "batch"),
                                                    R.decode_forced(net["dst"], net["z"][rows], net["chord"][rows], ones, "row")))


def test_ce_rows_targets_and_hits():
    """The reference's targets: arg-max with ties to the lowest index (an all-zero chord row targets 0), chroma truncated to long."""
    c = np.zeros((1, 2, 36))
    c[0, 1, [3, 5]] = 1.0            # a tie between 3 and 5: 3
    c[0, 1, 12:24] = 1.0
    t_root, t_chroma, t_bass = R.targets(c)
    assert t_root.tolist() == [[0, 3]] and t_bass.tolist() == [[0, 0]] and t_chroma[0, 1].tolist() == [1] * 12
    root = np.zeros((1, 2, 12))
    root[0, 1, 3] = 2.0
    ce, hit = R.ce_rows(c, root, np.zeros((1, 2, 12, 2)), np.zeros((1, 2, 12)))
    assert hit.tolist() == [[2, 12, 2]]                                   # chroma: arg-max of a tie is 0, the target of step 0
    want = np.log(12.0) + (np.log(11.0 + np.exp(2.0)) - 2.0)
    assert abs(ce[0, 0] - want) <= 1e-15 * want and abs(ce[0, 1] - 24 * np.log(2.0)) <= 1e-14 and abs(ce[0, 2] - 2 * np.log(12.0)) <= 1e-14


def test_teacher_forcing_rate_is_the_reference_schedule(g):
    from polyffusion_amd.chd8bar import CHD_8BAR, teacher_forcing_rate
    high, low = CHD_8BAR["tfr_chd"]
    got = np.array([teacher_forcing_rate(int(s), high, low) for s in g["sched_steps"]])
    assert np.array_equal(got, g["sched_tfr"])
    assert np.array_equal(np.array([teacher_forcing_rate(int(s)) for s in g["sched_steps"]]), g["sched_default"])
    assert teacher_forcing_rate(20000, 0.5, 0.0) == 0.25


@pytest.mark.parametrize("tag", sorted(R.NETS))
@pytest.mark.parametrize("rate,mk", [(0.0, "m0"), (0.5, "mh"), (1.0, "m1")])
def test_get_loss_dict_draws_the_flips_in_the_reference_order(g, tag, rate, mk, monkeypatch):
    """``n_step - 1`` draws from ``random`` per call, also at rate 0, each compared with the rate as the reference does: under the
    fixture's seed the product hands the fixture's flips to the decoder and leaves ``random`` where the reference left it."""
    from polyffusion_amd import chd8bar
    n_step = R.NETS[tag]["n_step"]
    seen = {}

    class Enc:
        with_scale = True

        def encode_dist(self, chord):
            return torch.zeros(2, 4), torch.ones(2, 4)

    class Dec:
        _lib = None

        def __init__(self):
            self.n_step = n_step

        def forward_forced(self, z, gt, force, feedback):
            seen.update(force=list(force), feedback=feedback)
            return None, None, None

    monkeypatch.setattr(chd8bar, "normal_rsample", lambda mean, std, noise, **kw: mean)
    model = chd8bar.Chord_8Bar(Enc(), Dec())
    monkeypatch.setattr(model, "chord_loss", lambda c, *logits, detail=False: {"loss": 0.0})
    random.seed(int(g["seed_flip"]))
    out = model.get_loss_dict((None, None, torch.zeros(2, n_step, 36), None), 0, rate, detail=True, feedback="batch")
    assert seen["force"] == g[f"{tag}_{mk}_flips"].tolist() == out["flips"] and seen["feedback"] == "batch"
    assert len(seen["force"]) == int(g[f"{tag}_random_calls"]) == n_step - 1
    assert random.random() == float(g[f"{tag}_random_next"])
