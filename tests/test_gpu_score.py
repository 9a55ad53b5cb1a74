"""Roll statistics on the GPU (-m gpu): ``pf_roll_stats`` must equal the numpy restatement in ``tests/score_ref.py`` EXACTLY on all three
outputs - every counter, every per-beat pitch-class count, every per-step onset count - at the smallest shapes that can go wrong (one beat,
two beats with a sustain across the boundary, more beats than the workgroup has waves, fewer, a canvas), with the values the rounding
rules hinge on planted at the keys of the wave seam, silent and full images, chords with an empty / full chroma, a tied / zero bass block,
both bass conventions, both rounding modes, with and without a mask; it writes every output word and nothing beside them, repeats bit
for bit, does not depend on how the batch is split, and replays from a captured graph.  Then ``score.roll_stats`` and its ratios on the
device, and ``inference_sdf --score / --best_of / --edit --score`` end to end against ``score_ref`` on the files they write."""
import ctypes as C
import glob
import json
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import score_ref  # noqa: E402
from polyffusion_amd import _lib, synth  # noqa: E402

I = score_ref.IDX
PAD = 16                              # int32 words of sentinel on either side of an output
SENTINEL, GARBAGE = -1234567, 0x5A5A5A5
SPECIAL = np.array([0.5, -0.5, -0.6, 0.95, 1.05, np.nan, np.inf, -np.inf, 1.0, 0.96, 0.51, -0.51], np.float32)
SEAM = (0, 63, 64, 127)
SHAPES = [(1, 4), (1, 8), (3, 128), (2, 64), (17, 12), (1, 256)]
MODES = [(False, False, False), (True, True, False), (False, True, True), (True, False, True)]      # custom_round, bass_relative, mask


@pytest.fixture(scope="module")
def lib():
    _lib.require_gpu()
    return _lib.load()


def make_case(n, steps, seed):
    """(x [n, 2, steps, 128], chord [n, steps / 4, 36], mask like x), float32 numpy, read-only."""
    rng = np.random.default_rng(seed)
    B = steps // 4
    x = (rng.standard_normal((n, 2, steps, 128)) * 0.6 + 0.3).astype(np.float32)
    flat = x.reshape(-1)
    where = rng.choice(flat.size, size=max(flat.size // 6, 24), replace=False)
    flat[where] = SPECIAL[rng.integers(len(SPECIAL), size=where.size)]
    for k, key in enumerate(SEAM):                               # every special value on every key of the wave seam, both channels
        for j, v in enumerate(SPECIAL):
            x[(j + k) % n, j % 2, (3 * j + k) % steps, key] = v
    x[0, 1, 0, 5] = 1.0                                          # an orphan at step 0
    if steps >= 8:                                               # a sustain across a beat boundary, held and not held by its predecessor
        x[0, 0, 4, 70:73] = 0.0
        x[0, :, 3, 70], x[0, 1, 4, 70] = (1.0, 0.0), 1.0
        x[0, :, 3, 71], x[0, 1, 4, 71] = (0.0, -0.6), 1.0        # -0.6 occupies by the default rule only
        x[0, :, 3, 72], x[0, 1, 4, 72] = (0.2, 0.1), 1.0
    if n >= 3:
        x[1] = 0.0                                               # a silent image
        x[2] = 1.0                                               # every cell sounding (in both rounding modes)
    if n >= 5:                                                   # the lowest / highest key away from the ends and on either side of the seam
        x[3, :, :, :66], x[3, :, :, 91:] = 0.0, 0.0
        x[4, :, :, :10], x[4, :, :, 64:] = 0.0, 0.0
    chord = np.zeros((n, B, 36), np.float32)
    chord[..., 12:24] = rng.random((n, B, 12)) < 0.35
    np.put_along_axis(chord[..., 0:12], rng.integers(12, size=(n, B, 1)), 1.0, axis=-1)
    np.put_along_axis(chord[..., 24:36], rng.integers(12, size=(n, B, 1)), 1.0, axis=-1)
    rows = chord.reshape(-1, 36)
    pick = lambda i: rows[(i * 7) % len(rows)]
    pick(0)[12:24] = 0.0                                         # an empty chroma: a no-chord beat
    if len(rows) > 1:
        pick(1)[12:24] = 1.0                                     # a full chroma
    if len(rows) > 2:
        pick(2)[24:36] = 0.0
        pick(2)[[24 + 9, 24 + 3]] = 0.7                          # a tie in the bass block: class 3
    if len(rows) > 3:
        pick(3)[24:36] = 0.0                                     # no bass
    if len(rows) > 4:
        pick(4)[12:24] = 0.5                                     # exactly 0.5 is not in the chord
        pick(4)[13] = 0.51
    if len(rows) > 5:
        pick(5)[0:12] = 0.25                                     # a tie in the root block: class 0
    mask = (rng.random((n, 2, steps, 128)) < 0.4).astype(np.float32)
    mask[:, 1] = 1.0 - mask[:, 0]                                # channel 1 is not read
    if steps >= 8:
        mask[0, :, 3, 70] = 1.0                                  # hides the predecessor of a sustain cell, which stays a predecessor
        mask[0, :, 4, 70] = 0.0
    for a in (x, chord, mask):
        a.setflags(write=False)
    return x, chord, mask


@pytest.fixture(scope="module")
def cases():
    """(n, steps) -> (x, chord, mask); and the restatement's answer per mode, computed once and shared."""
    data = {s: make_case(*s, seed=11 + i) for i, s in enumerate(SHAPES)}
    ref = {}
    for s, (x, chord, mask) in data.items():
        for mode in MODES:
            custom, rel, masked = mode
            ref[s, mode] = score_ref.roll_stats(x, chord, mask if masked else None, custom, rel)
    return data, ref


def guarded(shape):
    """(whole buffer, payload view): an int32 output pre-filled with garbage between two runs of sentinels."""
    size = int(np.prod(shape))
    whole = torch.full((size + 2 * PAD,), SENTINEL, device="cuda", dtype=torch.int32)
    whole[PAD: PAD + size] = GARBAGE
    return whole, whole[PAD: PAD + size].view(*shape)


def untouched(whole):
    return bool((whole[:PAD] == SENTINEL).all()) and bool((whole[-PAD:] == SENTINEL).all())


def launch(lib, x, chord, mask, custom, rel, outs=None):
    """One pf_roll_stats call on device tensors; returns (counters, chroma, onsets) views and their guarded buffers."""
    n, steps = x.shape[0], x.shape[2]
    bufs = outs or [guarded((n, 16)), guarded((n, steps // 4, 12)), guarded((n, steps))]
    a = _lib.RollStatsArgs(prmat2c=x.data_ptr(), chord=None if chord is None else chord.data_ptr(), mask=None if mask is None else mask.data_ptr(),
                           n=n, steps=steps, custom_round=int(custom), bass_relative=int(rel),
                           counters=bufs[0][1].data_ptr(), chroma=bufs[1][1].data_ptr(), onsets=bufs[2][1].data_ptr())
    _lib.check(lib.pf_roll_stats(C.byref(a), _lib.current_stream()), "pf_roll_stats", lib)
    return bufs


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def assert_equal(bufs, want, what):
    for (whole, got), ref, name in zip(bufs, want, ("counters", "chroma", "onsets")):
        g = got.cpu().numpy().astype(np.int64)
        assert untouched(whole), (what, name, "sentinel overwritten")
        bad = np.argwhere(g != ref)
        assert bad.size == 0, (what, name, bad[:8].tolist(), g[tuple(bad[0])], ref[tuple(bad[0])])


@pytest.mark.parametrize("mode", MODES, ids=lambda m: "custom%d-rel%d-mask%d" % m)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-steps%d" % s)
def test_every_word_equals_the_restatement(lib, cases, shape, mode):
    data, ref = cases
    x, chord, mask = data[shape]
    custom, rel, masked = mode
    want = ref[shape, mode]
    print(f"{shape} {mode}: counters summed over the batch {dict(zip(score_ref.NAMES, want[0][:, :12].sum(0).tolist()))}")
    bufs = launch(lib, dev(x), dev(chord), dev(mask) if masked else None, custom, rel)
    torch.cuda.synchronize()
    assert_equal(bufs, want, (shape, mode))
    assert (want[0][:, 14:] == 0).all()                                         # (the unused slots are written as 0: GARBAGE would show)


def test_the_planted_cases_are_really_in_the_data(cases):
    """The restatement's own answers show that the edges the kernel is compared at exist: orphans at step 0 and across the beat boundary,
    a mask that changes the counts, both bass conventions and both rounding modes giving different numbers, silent and full images."""
    data, ref = cases
    plain, custom, rel_mask, custom_mask = (ref[(3, 128), m] for m in MODES)
    c = plain[0]
    assert c[1, :3].tolist() == [0, 0, 0] and c[1, I["LOW_KEY"]] == -1 and c[1, I["HIGH_KEY"]] == -1
    assert c[2, I["N_SOUNDING"]] == 128 * 128 and c[2, I["N_ORPHAN"]] == 128 and (c[2, I["LOW_KEY"]], c[2, I["HIGH_KEY"]]) == (0, 127)
    assert (plain[1][2] > 0).all() and (plain[2][2] == 128).all()
    assert c[0, I["N_ORPHAN"]] > 0 and not np.array_equal(c, custom[0]) and not np.array_equal(c[:, :3], rel_mask[0][:, :3])
    x, chord, mask = data[(3, 128)]
    assert not np.array_equal(score_ref.roll_stats(x, chord, None, False, True)[0][:, I["BASS_HIT"]], c[:, I["BASS_HIT"]])
    x, chord, mask = data[(1, 8)]

    def first3(key, m=None, custom=False):
        """N_ONSET, N_SOUNDING, N_ORPHAN of steps 3 and 4 of one key alone"""
        y = np.zeros_like(x)
        y[:, :, 3:5, key] = x[:, :, 3:5, key]
        return score_ref.roll_stats(y, None, m, custom)[0][0, :3].tolist()

    assert first3(70) == [1, 2, 0]                         # a sustain held across the beat boundary
    assert first3(71) == [0, 1, 0]                         # -0.6 below it occupies ...
    assert first3(71, custom=True) == [0, 1, 1]            # ... but not under custom_round
    assert first3(72) == [0, 1, 1]                         # nothing below it
    assert first3(70, mask) == [0, 1, 0]                   # the onset hidden by the mask is silent and still a predecessor


def test_without_chords_the_chord_counters_are_written_as_zero(lib, cases):
    data, _ = cases
    x, chord, mask = data[(2, 64)]
    want = score_ref.roll_stats(x, None, None)
    assert (want[0][:, 3:12] == 0).all()
    assert_equal(launch(lib, dev(x), None, None, False, False), want, "no chords")


def test_two_calls_agree_and_a_split_batch_equals_the_whole(lib, cases):
    data, ref = cases
    for shape, cut in (((3, 128), 1), ((17, 12), 9)):
        x, chord, mask = (dev(a) for a in data[shape])
        mode = MODES[2]
        first, second = launch(lib, x, chord, mask, *mode[:2]), launch(lib, x, chord, mask, *mode[:2])
        for (_, a), (_, b) in zip(first, second):
            assert torch.equal(a, b)
        parts = [launch(lib, x[s].contiguous(), chord[s].contiguous(), mask[s].contiguous(), *mode[:2]) for s in (slice(0, cut), slice(cut, None))]
        for k in range(3):
            assert torch.equal(torch.cat([parts[0][k][1], parts[1][k][1]]), first[k][1])
        assert_equal(first, ref[shape, mode], shape)


def test_a_captured_launch_replays_the_same_words(lib, cases):
    data, ref = cases
    shape, mode = (3, 128), MODES[3]
    x, chord, mask = (dev(a) for a in data[shape])
    bufs = launch(lib, x, chord, mask, *mode[:2])                               # eager first: the module is loaded outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch(lib, x, chord, mask, *mode[:2], outs=bufs)
    for _, view in bufs:
        view.fill_(GARBAGE)
    g.replay()
    torch.cuda.synchronize()
    assert_equal(bufs, ref[shape, mode], "graph replay")
    x.copy_(torch.roll(x, 1, 0))                                                # the graph reads its inputs where they are
    g.replay()
    torch.cuda.synchronize()
    want = score_ref.roll_stats(np.roll(data[shape][0], 1, 0), data[shape][1], data[shape][2], mode[0], mode[1])
    assert_equal(bufs, want, "graph replay on new values")


# ---------------------------------------------------------------------------------------------- score.roll_stats and its ratios
def test_roll_stats_flattens_leading_shapes_and_its_scores_equal_the_restatement():
    from polyffusion_amd import score
    rng = np.random.default_rng(2)
    S, B = 2, 3
    gen = (rng.random((S, B, 2, 128, 128)) > 0.93).astype(np.float32)
    chd = synth.chords(B, 7)
    st = score.roll_stats(torch.from_numpy(gen).cuda(), torch.from_numpy(chd).cuda().unsqueeze(0).expand(S, B, 32, 36))
    want = score_ref.roll_stats(gen.reshape(S * B, 2, 128, 128), np.broadcast_to(chd, (S, B, 32, 36)).reshape(S * B, 32, 36))
    assert st.counters.dtype == torch.int32 and st.counters.is_cuda
    for got, ref in zip((st.counters, st.chroma, st.onsets), want):
        assert np.array_equal(got.cpu().numpy(), ref)
    songs = st.songs(B)
    sc, ref = songs.scores(), score_ref.scores(score_ref.songs(want[0], B), B * 128)
    for k in ref:
        assert sc[k].is_cuda and sc[k].dtype == torch.float64 and np.array_equal(sc[k].cpu().numpy(), ref[k]), k
    assert 0 < float(sc["chord_f1"][0]) < 1
    # the --autoreg halves [2B, 2, 64, 128] against the same chord tensor: the same song sums
    from polyffusion_amd.inference_sdf import autoreg_halves
    halves = autoreg_halves(torch.from_numpy(gen[0]).cuda())
    assert halves.shape == (2 * B, 2, 64, 128) and torch.equal(halves[1, :, :, :], torch.from_numpy(gen[0, 0, :, 64:, :]).cuda())
    h = score.roll_stats(halves, torch.from_numpy(chd).cuda())
    same = [i for n, i in I.items() if n != "N_ORPHAN"]                          # a half's step 0 has no predecessor: orphans may differ
    assert torch.equal(h.songs(2 * B).counters[:, same], st.songs(B).counters[:1, same])
    # texture_fit of a roll with itself is 1, with a silent roll 0
    silent = score.roll_stats(torch.zeros(S * B, 2, 128, 128, device="cuda"))
    assert torch.equal(score.texture_fit(st, st), torch.ones(S * B, dtype=torch.float64, device="cuda"))
    assert torch.equal(score.texture_fit(st, silent), torch.zeros(S * B, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="chord rows"):
        score.roll_stats(torch.from_numpy(gen).cuda(), torch.from_numpy(chd).cuda())
    with pytest.raises(ValueError, match="whole number of beats"):
        score.roll_stats(torch.zeros(1, 2, 6, 128, device="cuda"))


# ---------------------------------------------------------------------------------------------- end to end
BASE = ["--params_preset", "sdf_chd8bar", "--synthetic_weights", "--ddim", "--ddim_steps", "2", "--seed", "5", "--precision", "bf16x3"]
SEED = 5


def run_main(out, argv, capsys=None):
    from polyffusion_amd import inference_sdf
    assert inference_sdf.main(BASE + ["--output_dir", str(out)] + argv) == 0
    said = capsys.readouterr().out if capsys is not None else ""
    files = {}
    for f in glob.glob(os.path.join(str(out), "*.npy")):
        m = re.search(r"_\d{6}_(\d+)\.npy$", f)
        files[int(m.group(1)) if m else 0] = np.load(f)
    docs = glob.glob(os.path.join(str(out), "*_score.json"))
    return files, (json.load(open(docs[0])) if docs else None), said


def song_counters(files, chord, mask=None):
    """score_ref's per-song counters of the written songs [B, 2, 128, 128], in file order"""
    out = []
    for i in sorted(files):
        c = score_ref.roll_stats(files[i], chord, None if mask is None else mask)[0]
        out.append(score_ref.songs(c, files[i].shape[0])[0])
    return np.stack(out)


def check_best_of(tmp_path, capsys, extra, chord, mask=None):
    plain, none, _ = run_main(tmp_path / "plain", ["--num_generate", "6"] + extra)
    kept, doc, said = run_main(tmp_path / "best", ["--num_generate", "2", "--best_of", "3"] + extra, capsys)
    assert none is None and sorted(plain) == list(range(6)) and sorted(kept) == [0, 1]
    counters = song_counters(plain, chord, mask)
    steps = plain[0].shape[0] * 128
    ref = score_ref.scores(counters, steps)
    order = score_ref.rank(ref["chord_f1"], 2)
    print("chord_f1 of the six candidates:", ref["chord_f1"].tolist(), "kept:", order)
    for r, cand in enumerate(order):
        assert np.array_equal(kept[r].view(np.uint32), plain[cand].view(np.uint32)), (r, cand)
    assert doc["best_of"] == 3 and doc["rank_by"] == "chord" and doc["masked"] == (mask is not None) and doc["steps"] == steps
    assert [s["candidate"] for s in doc["songs"]] == order and len(doc["candidates"]) == 6
    for i, c in enumerate(doc["candidates"]):
        assert [c["counters"][n] for n in score_ref.NAMES] == counters[i, :14].tolist(), i
        for k in ref:
            assert c[k] == ref[k][i], (i, k)
    assert all(s["chord_f1"] == ref["chord_f1"][order[r]] for r, s in enumerate(doc["songs"]))
    assert "best of 3: 6 candidates" in said and f"(candidate {order[0]} of 6)" in said
    return ref


def test_best_of_keeps_the_candidates_the_restatement_ranks_first(tmp_path, capsys):
    check_best_of(tmp_path, capsys, ["--synthetic", "--length", "1"], synth.chords(1, SEED + 100))


def test_best_of_on_a_joint_canvas(tmp_path, capsys):
    check_best_of(tmp_path, capsys, ["--synthetic", "--length", "2", "--joint"], synth.chords(2, SEED + 100))


def test_best_of_when_inpainting_scores_the_invented_cells(tmp_path, capsys):
    rng = np.random.default_rng(8)
    chord, image = synth.chords(1, 41), (rng.random((1, 2, 128, 128)) > 0.95).astype(np.float32)
    np.savez(tmp_path / "song.npz", chord=chord, prmat2c=image)
    mask = np.ones_like(image)
    mask[:, :, 32:64] = 0                                                       # --bar_list 2,3: bars of 16 steps
    check_best_of(tmp_path, capsys, ["--cond_npz", str(tmp_path / "song.npz"), "--inpaint_type", "bars", "--bar_list", "2,3"], chord, mask)


def test_edit_score_prints_the_four_numbers_of_the_restatement(tmp_path, capsys):
    from polyffusion_amd.inference_sdf import shift_chords
    rng = np.random.default_rng(9)
    chord, image = synth.chords(1, 42), (rng.random((1, 2, 128, 128)) > 0.95).astype(np.float32)
    np.savez(tmp_path / "song.npz", chord=chord, prmat2c=image)
    files, doc, said = run_main(tmp_path / "edit", ["--cond_npz", str(tmp_path / "song.npz"), "--edit", "--edit_iters", "1", "--edit_chord_shift", "2",
                                                    "--score"], capsys)
    target = shift_chords(torch.from_numpy(chord), 2).numpy()
    f1 = lambda img, chd: float(score_ref.scores(score_ref.songs(score_ref.roll_stats(img, chd)[0], 1), 128)["chord_f1"][0])
    want = {"source_on_source_chords": f1(image, chord), "source_on_target_chords": f1(image, target),
            "edited_on_source_chords": f1(files[0], chord), "edited_on_target_chords": f1(files[0], target)}
    print("edit chord_f1:", want)
    assert {k: doc[k]["chord_f1"] for k in want} == want
    line = [ln for ln in said.splitlines() if ln.startswith("edit score (chord_f1)")]
    assert len(line) == 1 and [float(v) for v in re.findall(r"chords ([0-9.e+-]+)", line[0])] == list(want.values())
    assert want["source_on_source_chords"] != want["source_on_target_chords"]


def test_score_of_autoreg_halves_and_of_a_model_without_chords(tmp_path, capsys):
    files, doc, said = run_main(tmp_path / "autoreg", ["--synthetic", "--length", "2", "--autoreg", "--score"], capsys)
    assert files[0].shape == (4, 2, 64, 128) and doc["best_of"] == 1 and doc["rank_by"] is None and doc["chords"] and doc["steps"] == 256
    want = score_ref.songs(score_ref.roll_stats(files[0], synth.chords(2, SEED + 100).reshape(4, 16, 36))[0], 4)
    assert [doc["songs"][0]["counters"][n] for n in score_ref.NAMES] == want[0, :14].tolist() and doc["songs"][0]["candidate"] == 0
    assert doc["songs"][0]["chord_f1"] == score_ref.scores(want, 256)["chord_f1"][0] and "song 0 score: chord_f1" in said
    # cond_type txt: the run conditions on no chords, so the chord-free numbers
    files, doc, _ = run_main(tmp_path / "txt", ["--params_preset", "sdf_txt", "--synthetic", "--length", "1", "--score"], capsys)
    want = score_ref.roll_stats(files[0], None)[0]
    got = doc["songs"][0]
    assert doc["chords"] is False and [got["counters"][n] for n in score_ref.NAMES] == want[0, :14].tolist() and want[0, I["N_ONSET"]] > 0
    assert (got["chord_f1"], got["bass_fit"]) == (0.0, 0.0) and got["integrity"] == score_ref.scores(want, 128)["integrity"][0]
