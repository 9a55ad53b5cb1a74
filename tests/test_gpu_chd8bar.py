"""The chd_8bar objective on the GPU: the teacher-forced chord decode (``pf_decoder_forward_forced``), the cross-entropy
(``pf_chord_ce_rows``), ``pf_normal_rsample``, ``chd8bar.Chord_8Bar`` and ``validate --model chd_8bar`` - against the reference fixture
tests/golden/chd8bar.npz and the float64 restatement tests/chd8bar_ref.py (pinned to that fixture in tests/test_chd8bar_oracle.py).

Tolerances.  Logits: 1e-4 absolute, the decoders' existing bound (tests/test_gpu_decoders.py) - 200 times the reference's own float32
noise and ten times below the smallest top-1 / top-2 gap of any row used here (1e-3), so within it no arg-max can flip; rows drawn
here are used only where the float64 restatement clears that gap, and a case fails outright if fewer than half of its rows do.
Cross-entropy on given logits: relative 1e-12 (float64 exp / log on the device plus at most 32 * 25 ordered additions).  Losses:
a cross-entropy item moves by at most twice the largest logit error e (log-sum-exp and the target logit each by at most e), so each of
the three means moves by at most 2 e and their sum by 6 e.

Observed on an MI355X when the tests were written: logits within 4.8e-7 of the reference's float32 run and 3.8e-7 of the float64
restatement in every case (both nets, every mask, both feedback forms, the off-size net); ``pf_chord_ce_rows`` relative 3.4e-16; batch
losses within 1.6e-8 of the restatement; per-row losses within 7.6e-7 of the reference's float32 values; ``pf_normal_rsample`` at 0.67
of its per-element bound.
"""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chd8bar_ref as R  # noqa: E402
from polyffusion_amd import _lib, chd8bar, synth, validate  # noqa: E402
from polyffusion_amd.decoders import ChordDecoder  # noqa: E402
from polyffusion_amd.weights import synth_chord_decoder_state  # noqa: E402

TOL = 1e-4
GAP = 1e-3
MASKS = {"m0": 0.0, "mh": 0.5, "m1": 1.0}
LOGITS = ("root", "chroma", "bass")
KEYS = ("loss", "root", "chroma", "bass")


@pytest.fixture(scope="module")
def g():
    return R.fixture()


@pytest.fixture(scope="module")
def nets(g):
    """Per net: the model on the GPU, the states, the pool's chords / noise and the float64 z of the restated encoder (never modified)."""
    out = {}
    for tag, net in R.NETS.items():
        est, dst = R.states(net, int(g["seed_w"]))
        p = dict(chd_n_step=net["n_step"], chd_z_input_dim=net["z_input_dim"], chd_hidden_dim=net["hidden_dim"], chd_z_dim=net["z_dim"])
        model = chd8bar.Chord_8Bar.from_params(p)
        model.chord_enc.load_state_dict(est)
        model.chord_dec.load_state_dict(dst)
        chord = g[f"{tag}_chord"].astype(np.float32)
        mean, scale = R.encoder_dist(est, chord)
        out[tag] = dict(model=model, est=est, dst=dst, chord=chord, noise=g[f"{tag}_noise"], z64=mean + scale * g[f"{tag}_noise"].astype(np.float64))
    return out


def _err(got, want):
    return max(float(np.abs(a.detach().cpu().numpy().astype(np.float64) - np.asarray(b, np.float64)).max()) for a, b in zip(got, want))


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _clearing(dst, z, gt, flips, n_step):
    """Float64 logits of the pool under ``flips`` (row feedback) and the indices of the rows that clear the gap: at least half must."""
    want = R.decode_forced(dst, z, gt, flips, "row", n_step=n_step)
    ok = np.nonzero(R.min_margin(*want) >= GAP)[0]
    assert len(ok) * 2 >= z.shape[0], f"only {len(ok)} of {z.shape[0]} rows clear the gap"
    return want, ok


# ------------------------------------------------------------------------------------------------ logits
@pytest.mark.parametrize("mk", sorted(MASKS))
@pytest.mark.parametrize("tag", sorted(R.NETS))
def test_forced_logits_against_the_fixture_and_the_restatement(g, nets, tag, mk):
    n = nets[tag]
    rows, flips = g[f"{tag}_{mk}_rows"], g[f"{tag}_{mk}_flips"].tolist()
    z32 = g[f"{tag}_z32"][rows]
    got = n["model"].chord_dec.forward_forced(_cuda(z32), _cuda(n["chord"][rows]), flips, "row")
    e_ref = _err(got, [g[f"{tag}_{mk}_{name}32"] for name in LOGITS])
    e_orc = _err(got, R.decode_forced(n["dst"], z32, n["chord"][rows], flips, "row"))
    print(f"net {tag} mask {mk}: logits vs reference float32 {e_ref:.3e}, vs float64 restatement {e_orc:.3e}")
    assert e_ref <= TOL and e_orc <= TOL
    # an int mask is the same call
    assert _equal(got, n["model"].chord_dec.forward_forced(_cuda(z32), _cuda(n["chord"][rows]), R.mask_of(flips), "row"))


@pytest.mark.parametrize("tag", sorted(R.NETS))
def test_batch_feedback_against_the_reference_batch_of_4(g, nets, tag):
    n = nets[tag]
    rows, flips = g[f"{tag}_b4_rows"], g[f"{tag}_mh_flips"].tolist()
    z32 = g[f"{tag}_z32"][rows]
    got = n["model"].chord_dec.forward_forced(_cuda(z32), _cuda(n["chord"][rows]), flips, "batch")
    e_ref = _err(got, [g[f"{tag}_b4_{name}32"] for name in LOGITS])
    e_orc = _err(got, R.decode_forced(n["dst"], z32, n["chord"][rows], flips, "batch"))
    print(f"net {tag} batch of 4, batch feedback: logits vs reference float32 {e_ref:.3e}, vs float64 restatement {e_orc:.3e}")
    assert e_ref <= TOL and e_orc <= TOL
    row = n["model"].chord_dec.forward_forced(_cuda(z32), _cuda(n["chord"][rows]), flips, "row")
    assert _err(got, [t.cpu().numpy() for t in row]) > GAP               # the union is what makes the reference's number


@pytest.mark.parametrize("rows", [1, 3, 9, 17])
@pytest.mark.parametrize("n_step", [2, 8])
def test_masks_and_row_counts_off_the_tile(g, nets, n_step, rows):
    """Only-first, only-last and a mixed mask at R = 1, 3, 9, 17 (the mat-vec kernels hold 8 rows) and n_step 2 and 8 (32: the fixture
    tests), on the "s" weights; rows are the first that clear the gap in float64."""
    n = nets["s"]
    dec = n["model"].chord_dec if n_step == 8 else ChordDecoder(36, 256, 512, 256, n_step).load_state_dict(n["dst"])
    gt = n["chord"][:, :n_step]
    z = g["s_z32"]
    masks = {"first": [True] + [False] * (n_step - 2), "last": [False] * (n_step - 2) + [True]}
    if n_step > 2:
        masks["mixed"] = [t % 3 == 1 for t in range(n_step - 1)]
    for name, flips in masks.items():
        want, ok = _clearing(n["dst"], z, gt, flips, n_step)
        assert len(ok) >= rows
        pick = ok[:rows]
        got = dec.forward_forced(_cuda(z[pick]), _cuda(gt[pick]), flips, "row")
        e = _err(got, [w[pick] for w in want])
        print(f"n_step {n_step} rows {rows} mask {name}: {len(ok)} of 32 rows clear; logits vs restatement {e:.3e}")
        assert tuple(got[1].shape) == (rows, n_step, 12, 2) and e <= TOL


def test_off_size_net():
    """hidden 96, z 20, z_input 12, n_step 5: no dimension a multiple of a wave or of the row tile."""
    net = dict(input_dim=36, z_input_dim=12, hidden_dim=96, z_dim=20, n_step=5)
    dst = synth_chord_decoder_state(3, 36, 12, 96, 20)
    dec = ChordDecoder(**net).load_state_dict(dst)
    z = np.random.Generator(np.random.PCG64(77)).standard_normal((32, 20)).astype(np.float32)
    gt = synth.chords(32, 78, 5)
    flips = [False, True, False, False]
    want, ok = _clearing(dst, z, gt, flips, 5)
    pick = ok[:11]
    got = dec.forward_forced(_cuda(z[pick]), _cuda(gt[pick]), flips, "row")
    e = _err(got, [w[pick] for w in want])
    print(f"off-size net: {len(ok)} of 32 rows clear; logits vs restatement {e:.3e}")
    assert len(pick) == 11 and e <= TOL
    # batch feedback on the first window of 5 rows whose BATCHED float64 run clears the gap as a whole
    for start in range(28):
        sl = slice(start, start + 5)
        wb = R.decode_forced(dst, z[sl], gt[sl], flips, "batch")
        if R.min_margin(*wb).min() >= GAP:
            break
    else:
        pytest.fail("no window of 5 rows clears the gap under batch feedback")
    e = _err(dec.forward_forced(_cuda(z[sl]), _cuda(gt[sl]), flips, "batch"), wb)
    print(f"off-size net, batch feedback rows {start}..{start + 4}: logits vs restatement {e:.3e}")
    assert e <= TOL


# ------------------------------------------------------------------------------------------------ bit identity
@pytest.mark.parametrize("tag", sorted(R.NETS))
def test_bit_identity(g, nets, tag):
    n = nets[tag]
    dec, n_step = n["model"].chord_dec, R.NETS[tag]["n_step"]
    z, gt = _cuda(g[f"{tag}_z32"][:9]), _cuda(n["chord"][:9])
    greedy = dec(z, True, 0.0)
    zero = dec.forward_forced(z, gt, 0, "row")
    assert _equal(zero, greedy)                                            # mask 0, row feedback: pf_decoder_forward bit for bit
    flips = g[f"{tag}_mh_flips"].tolist()
    for fb in ("row", "batch"):
        a, b = dec.forward_forced(z, gt, flips, fb), dec.forward_forced(z, gt, flips, fb)
        assert _equal(a, b)                                                # two identical calls
    nine = dec.forward_forced(z, gt, flips, "row")
    alone = dec.forward_forced(z[:1], gt[:1], flips, "row")
    assert _equal([t[:1] for t in nine], alone)                            # row 0 alone is row 0 among others
    tail = dec.forward_forced(z[5:], gt[5:], flips, "row")
    assert _equal([t[5:] for t in nine], tail)
    assert _equal(alone, dec.forward_forced(z[:1], gt[:1], flips, "batch"))   # a batch of one has nothing to unite
    ones = (1 << (n_step - 1)) - 1
    assert _equal(dec.forward_forced(z, gt, ones, "row"), dec.forward_forced(z, gt, ones, "batch"))   # nothing is fed back
    assert not _equal(dec.forward_forced(z, gt, ones, "row"), zero)


# ------------------------------------------------------------------------------------------------ pf_chord_ce_rows
@pytest.fixture(scope="module")
def ce_case():
    rng = np.random.Generator(np.random.PCG64(5))
    rows, n_step = 17, 32
    gt = synth.chords(rows, 6, n_step)
    gt[2, 3] = 0.0                                                         # an all-zero chord row: targets 0 / all 0 / 0
    gt[4, 5, 12:24] = 0.7                                                  # .long() truncates: 0
    gt[6, 7, [1, 9]] = 1.0                                                 # a tie with the row's own root: lowest index wins
    logits = [(3.0 * rng.standard_normal(s)).astype(np.float32) for s in ((rows, n_step, 12), (rows, n_step, 12, 2), (rows, n_step, 12))]
    logits[0][2, 3] = 0.0
    logits[0][2, 3, 0] = 1.0                                               # the all-zero row's target 0 is the arg-max: a hit
    logits[2][1, 1, 4] = logits[2][1, 1, 8] = 9.0                          # tied logits: the arg-max is the lower index
    return gt, logits, R.ce_rows(gt, *logits)


def _ce(lib, gt, logits, guard=4):
    """pf_chord_ce_rows into the middle of sentinel-filled buffers: (ce [rows][3], hits [rows][3], the two whole buffers)"""
    rows, n_step = gt.shape[0], gt.shape[1]
    ce = torch.full((rows + 2 * guard, 3), -7.5, dtype=torch.float64, device="cuda")
    hit = torch.full((rows + 2 * guard, 3), -77, dtype=torch.int32, device="cuda")
    t = [_cuda(a) for a in logits] + [_cuda(gt)]
    _lib.check(lib.pf_chord_ce_rows(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), rows, n_step,
                                    ce[guard:].data_ptr(), hit[guard:].data_ptr(), _lib.current_stream()), "pf_chord_ce_rows")
    torch.cuda.synchronize()
    return ce[guard:guard + rows].cpu(), hit[guard:guard + rows].cpu(), ce.cpu(), hit.cpu()


def test_chord_ce_rows(ce_case):
    lib = _lib.load()
    gt, logits, (want_ce, want_hit) = ce_case
    ce, hit, ce_all, hit_all = _ce(lib, gt, logits)
    rel = float((np.abs(ce.numpy() - want_ce) / np.abs(want_ce)).max())
    print(f"pf_chord_ce_rows vs float64 numpy on the same logits: relative {rel:.3e}")
    assert rel <= 1e-12
    assert np.array_equal(hit.numpy(), want_hit)
    assert (ce_all[:4] == -7.5).all() and (ce_all[-4:] == -7.5).all() and (hit_all[:4] == -77).all() and (hit_all[-4:] == -77).all()
    # the all-zero chord row targets index 0: with logit 0 the largest there, step (2, 3) is a root hit, and moving the peak loses it
    moved = [a.copy() for a in logits]
    moved[0][2, 3, 0], moved[0][2, 3, 5] = 0.0, 1.0
    assert _ce(lib, gt, moved)[1][2, 0] == hit[2, 0] - 1
    # the split 17 = 9 + 8, and without the optional hits
    a, b = _ce(lib, gt[:9], [x[:9] for x in logits]), _ce(lib, gt[9:], [x[9:] for x in logits])
    assert torch.equal(torch.cat([a[0], b[0]]), ce) and torch.equal(torch.cat([a[1], b[1]]), hit)
    got, none = chd8bar.chord_ce_rows(_cuda(gt), *[_cuda(x) for x in logits], hits=False)
    assert none is None and torch.equal(got.cpu(), ce)


# ------------------------------------------------------------------------------------------------ losses
def _loss_run(n, rows, rate, seed_flip, feedback):
    """get_loss_dict on pool rows with the stored noise, and the logits of that very run (the same launches again: same bits)"""
    model, chord, noise = n["model"], _cuda(n["chord"][rows]), _cuda(n["noise"][rows])
    random.seed(seed_flip)
    d = model.get_loss_dict((None, None, chord, None), 0, rate, detail=True, feedback=feedback, noise=noise)
    mean, std = model.chord_enc.encode_dist(chord)
    logits = model.chord_dec.forward_forced(chd8bar.normal_rsample(mean, std, noise), chord, d["flips"], feedback)
    return d, logits


@pytest.mark.parametrize("mk", sorted(MASKS))
@pytest.mark.parametrize("tag", sorted(R.NETS))
def test_loss_against_the_restatement_and_the_reference(g, nets, tag, mk):
    n = nets[tag]
    rows = g[f"{tag}_{mk}_rows"]
    d, logits = _loss_run(n, rows, MASKS[mk], int(g["seed_flip"]), "row")
    assert d["flips"] == g[f"{tag}_{mk}_flips"].tolist()
    want_logits = R.decode_forced(n["dst"], n["z64"][rows], n["chord"][rows], d["flips"], "row")
    e = _err(logits, want_logits)
    want = R.chord_loss(n["chord"][rows], *want_logits)
    got = {"loss": float(d["loss64"]), **{k: float(d["loss_rows"][:, i].mean()) for i, k in enumerate(KEYS[1:])}}
    diff = {k: abs(got[k] - want[k]) for k in KEYS}
    print(f"net {tag} mask {mk}: logit error {e:.3e}; loss {got['loss']:.6f} vs restatement {want['loss']:.6f}: " +
          " ".join(f"{k} {diff[k]:.3e}" for k in KEYS))
    assert e <= TOL
    assert diff["loss"] <= 6 * e + 1e-12 and all(diff[k] <= 2 * e + 1e-12 for k in KEYS[1:])
    for k in KEYS:                                                         # the float32 scalars the reference's call shape returns
        assert abs(float(d[k]) - got[k]) <= 1e-6 * max(1.0, abs(got[k]))
    # every row against the real reference's float32 run of that row alone: the same bound plus the reference's own float32 distance
    ref = g[f"{tag}_{mk}_loss32"].astype(np.float64)
    rows3 = d["loss_rows"].cpu().numpy()
    slack = float(g["ref_f32_f64_loss"])
    d_sum, d_part = np.abs(rows3.sum(1) - ref[:, 0]).max(), np.abs(rows3 - ref[:, 1:]).max()
    print(f"net {tag} mask {mk}: per-row losses vs reference float32: sum {d_sum:.3e} parts {d_part:.3e}")
    assert d_sum <= 6 * e + 1e-12 + slack and d_part <= 2 * e + 1e-12 + slack
    acc = d["acc"].cpu().numpy()
    _, hits = R.ce_rows(n["chord"][rows], *want_logits)
    n_step = R.NETS[tag]["n_step"]
    assert np.array_equal(d["hit_rows"].cpu().numpy(), hits) and np.allclose(acc, hits.sum(0) / (len(rows) * np.array([n_step, 12 * n_step, n_step])))


@pytest.mark.parametrize("tag", sorted(R.NETS))
def test_batch_feedback_loss_is_the_reference_number(g, nets, tag):
    n = nets[tag]
    rows = g[f"{tag}_b4_rows"]
    d, logits = _loss_run(n, rows, 0.5, int(g["seed_flip"]), "batch")
    e = _err(logits, R.decode_forced(n["dst"], n["z64"][rows], n["chord"][rows], d["flips"], "batch"))
    got = np.array([float(d["loss64"])] + [float(d["loss_rows"][:, i].mean()) for i in range(3)])
    d64, d32 = np.abs(got - g[f"{tag}_b4_loss64"]), np.abs(got - g[f"{tag}_b4_loss32"].astype(np.float64))
    print(f"net {tag} batch of 4, batch feedback: logit error {e:.3e}; loss {got[0]:.6f}; vs reference float64 {d64.max():.3e} float32 {d32.max():.3e}")
    slack = float(g["ref_f32_f64_loss"])
    assert e <= TOL and d64[0] <= 6 * e + 1e-12 and (d64[1:] <= 2 * e + 1e-12).all()
    assert d32[0] <= 6 * e + 1e-12 + slack and (d32[1:] <= 2 * e + 1e-12 + slack).all()


def test_get_loss_dict_is_invariant_to_the_batch_split_in_row_mode(nets):
    n = nets["s"]
    model, chord, zd = n["model"], _cuda(n["chord"][:17]), R.NETS["s"]["z_dim"]
    run = lambda sl, off: model.get_loss_dict((None, None, chord[sl], None), 0, 0.0, detail=True, seed=11, draw=2, elem_offset=off)
    whole, a, b = run(slice(0, 17), 40), run(slice(0, 9), 40), run(slice(9, 17), 40 + 9 * zd)
    assert torch.equal(whole["loss_rows"], torch.cat([a["loss_rows"], b["loss_rows"]]))
    assert torch.equal(whole["hit_rows"], torch.cat([a["hit_rows"], b["hit_rows"]]))
    assert not torch.equal(whole["loss_rows"], run(slice(0, 17), 44)["loss_rows"])     # the offset is what keys the noise
    assert len(whole["flips"]) == 7 and not any(whole["flips"])


# ------------------------------------------------------------------------------------------------ pf_normal_rsample
def test_normal_rsample():
    lib = _lib.load()
    n, seed, draw, off = 1003, 9, 3, 6                                     # no multiple of four anywhere
    rng = np.random.Generator(np.random.PCG64(8))
    mean, std = rng.standard_normal(n).astype(np.float32), np.exp(rng.standard_normal(n)).astype(np.float32)
    noise = torch.empty(n, dtype=torch.float32, device="cuda")
    _lib.check(lib.pf_randn(noise.data_ptr(), n, seed, draw, off, _lib.current_stream()), "pf_randn")
    from_rng = chd8bar.normal_rsample(_cuda(mean), _cuda(std), None, seed=seed, draw=draw, elem_offset=off)
    from_tensor = chd8bar.normal_rsample(_cuda(mean), _cuda(std), noise)
    assert torch.equal(from_rng, from_tensor)                              # the rng form is pf_randn + the tensor form, bit for bit
    nz = noise.cpu().numpy().astype(np.float64)
    want = mean.astype(np.float64) + std.astype(np.float64) * nz
    bound = 2 * 2.0 ** -24 * (np.abs(mean) + np.abs(std.astype(np.float64) * nz))
    err = np.abs(from_tensor.cpu().numpy().astype(np.float64) - want)
    print(f"pf_normal_rsample vs float64: worst error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    assert 0.9 < float(nz.std()) < 1.1


# ------------------------------------------------------------------------------------------------ workspace, capture
def test_workspace_canaries_rows_9(g, nets):
    n = nets["c"]
    dec, lib = n["model"].chord_dec, _lib.load()
    z, gt = _cuda(g["c_z32"][:9]), _cuda(n["chord"][:9])
    flips = g["c_mh_flips"].tolist()
    want = dec.forward_forced(z, gt, flips, "batch")
    need, guard = lib.pf_decoder_forced_workspace_bytes(dec._h, 9), 64 * 1024
    buf = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    outs = [torch.full_like(t, float("nan")) for t in want]
    a = _lib.ChordForcedArgs(z=z.data_ptr(), gt=gt.data_ptr(), rows=9, feedback=1, force_mask=R.mask_of(flips), root=outs[0].data_ptr(),
                             chroma=outs[1].data_ptr(), bass=outs[2].data_ptr(), workspace=buf.data_ptr() + guard, workspace_bytes=need)
    _lib.check(lib.pf_decoder_forward_forced(dec._h, C.byref(a), _lib.current_stream()), "pf_decoder_forward_forced")
    torch.cuda.synchronize()
    assert _equal(outs, want)
    assert bool((buf[:guard] == 0xA5).all()) and bool((buf[guard + need:] == 0xA5).all())


def test_forced_decode_and_cross_entropy_are_capturable(g, nets):
    """One capture of forward_forced + the cross-entropy (a linear graph: one stream, no branches), replayed: the eager bits."""
    n = nets["s"]
    model = n["model"]
    z, gt = _cuda(g["s_z32"][:3]), _cuda(n["chord"][:3])
    flips = g["s_mh_flips"].tolist()

    def step():
        logits = model.chord_dec.forward_forced(z, gt, flips, "batch")
        return logits + chd8bar.chord_ce_rows(gt, *logits)

    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _equal(eager, captured)


# ------------------------------------------------------------------------------------------------ validate, checkpoints
def test_validate_cli(capsys):
    import json
    base = ["--model", "chd_8bar", "--synthetic_weights", "--synthetic"]
    r2 = validate.main(base + ["--batch_num", "2", "--batch_size", "8"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["model"] == "chd_8bar" and line["feedback"] == "row" and line["tfr_chd"] == 0.0 and line["n_samples"] == 16
    for k in ("val/loss", "val/root", "val/chroma", "val/bass", "acc/root", "acc/chroma", "acc/bass"):
        assert np.isfinite(line[k]) and line[k] == r2[k]
    assert len(line["batch_losses"]) == 2 and abs(line["val/loss"] - (line["val/root"] + line["val/chroma"] + line["val/bass"])) < 1e-12
    assert 1.0 < line["val/loss"] < 10.0 and 0.0 <= line["acc/root"] <= 1.0          # untrained weights: about log 12 + log 2 + log 12
    r1 = validate.main(base + ["--batch_num", "1", "--batch_size", "16"])
    capsys.readouterr()
    assert r1["n_samples"] == 16 and r1["loss_rows"].shape == (16, 3)
    # the same 16 samples; where the seeds line up - batch 0 is draw 0 in both runs - the rows are the same bits, whatever the batch size
    assert np.array_equal(r1["loss_rows"][:8], r2["loss_rows"][:8])
    assert not np.array_equal(r1["loss_rows"][8:], r2["loss_rows"][8:])              # batch 1 took draw 1: other noise, same samples
    rb = validate.main(base + ["--batch_num", "1", "--batch_size", "16", "--feedback", "batch", "--global_step", "20000"])
    capsys.readouterr()
    assert rb["feedback"] == "batch" and rb["tfr_chd"] == 0.25 and np.isfinite(rb["val/loss"]) and rb["val/loss"] != r1["val/loss"]
    assert any(rb["flips"][0]) and not all(rb["flips"][0])


def test_weights_pt_round_trips_through_load_trained(nets, tmp_path):
    import ckpt_fixture
    n = nets["s"]
    state = {f"chord_enc.{k}": torch.as_tensor(np.asarray(v)) for k, v in n["est"].items()}
    state.update({f"chord_dec.{k}": torch.as_tensor(np.asarray(v)) for k, v in n["dst"].items()})
    ckpt_fixture.write_legacy_pt(str(tmp_path / "weights.pt"), state)
    net = R.NETS["s"]
    p = dict(chd_n_step=net["n_step"], chd_z_input_dim=net["z_input_dim"], chd_hidden_dim=net["hidden_dim"], chd_z_dim=net["z_dim"])
    fresh = chd8bar.Chord_8Bar.from_params(p)
    chord = _cuda(n["chord"][:3])
    for where in (tmp_path, tmp_path / "weights.pt"):
        loaded = chd8bar.Chord_8Bar.load_trained(fresh.chord_enc, fresh.chord_dec, where)
        a = loaded.get_loss_dict((None, None, chord, None), 0, 0.0, detail=True, seed=1)
        b = n["model"].get_loss_dict((None, None, chord, None), 0, 0.0, detail=True, seed=1)
        assert torch.equal(a["loss_rows"], b["loss_rows"]) and torch.equal(a["loss"], b["loss"])
    with pytest.raises(RuntimeError, match="chord_enc"):
        ckpt_fixture.write_legacy_pt(str(tmp_path / "other.pt"), {"ldm.alpha": torch.zeros(3)})
        chd8bar.Chord_8Bar.load_trained(fresh.chord_enc, fresh.chord_dec, tmp_path / "other.pt")
