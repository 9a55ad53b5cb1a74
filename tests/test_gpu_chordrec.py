"""Chord recognition on the GPU (-m gpu): ``pf_chord_recognize`` must equal the numpy restatement in ``tests/chordrec_ref.py`` EXACTLY on
every output word - labels, segment bounds, rows, counters, both feature tables, and the path score bit for bit as float64 - at the smallest
shapes that can go wrong (one bar, bars that are no multiple of the waves, several songs, songs of several images), with and without a
condition, in both rounding modes and both bass conventions; it writes every output word and nothing beside them, repeats bit for bit, does
not depend on how the batch is split, and replays from a captured graph.  Then ``chordrec.recognize_rolls`` against the file path, and
``inference_sdf --score --score_chords / --rank_by extracted / --edit`` end to end against the restatement on the files they write."""
import ctypes as C
import glob
import json
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import chordrec_cases  # noqa: E402
import chordrec_ref as ref  # noqa: E402
from polyffusion_amd import _lib, chordrec, synth  # noqa: E402

I = ref.IDX
PAD = 16                              # int32 words of sentinel on either side of an output
SENTINEL, GARBAGE = -1234567, 0x5A5A5A5
SPECIAL = np.array([0.5, -0.5, 0.95, 1.05, np.nan, np.inf, -np.inf, 0.96, 0.51, 1.04], np.float32)
SHAPES = [(1, 1, 16), (3, 1, 48), (5, 1, 128), (2, 2, 16), (2, 3, 128)]          # songs, segments, steps
MODES = [(False, False, False), (True, False, False), (True, True, True), (True, False, True), (False, True, False)]  # chord, custom, relative
OUTPUTS = ("labels", "bounds", "rows", "counters", "path_score", "chroma_q", "bass_q")
DTYPES = dict(labels=torch.int32, bounds=torch.int32, rows=torch.float32, counters=torch.int32, path_score=torch.float64, chroma_q=torch.int32,
              bass_q=torch.int32)


@pytest.fixture(scope="module")
def lib():
    _lib.require_gpu()
    return _lib.load()


def make_case(songs, segments, steps, seed):
    """(x [songs * segments, 2, steps, 128], chord [songs, beats, 36]) float32 numpy, read-only: every song another density, with and
    without same-key overlaps, the values the rounding rules hinge on sprinkled over both channels."""
    rng = np.random.default_rng(seed)
    x = np.concatenate([chordrec_cases.random_roll(seed * 100 + s, segments, steps, chordrec_cases.DENSITIES[s % 3], s % 2 == 1) for s in range(songs)])
    flat = x.reshape(-1)
    where = rng.choice(flat.size, size=flat.size // 300, replace=False)
    flat[where] = SPECIAL[rng.integers(len(SPECIAL), size=where.size)]
    x[0, 0, 0, 0], x[-1, 0, steps - 1, 127] = 1.0, 1.0                       # the lowest key at the first step, the highest at the last
    chord = chordrec_cases.random_chords(seed + 50, songs, segments * steps // 4)
    # every other beat of the condition is the row the restatement recognises (plain rounding): the hit counters have something to count
    rows = ref.recognize_rolls(x, segments)["rows"]
    chord[:, ::2] = rows[:, ::2]
    chord[0, 0, 12:24] = np.where(chord[0, 0, 12:24] > 0.5, np.float32(0.51), np.float32(0.5))     # exactly 0.5 is not set
    for a in (x, chord):
        a.setflags(write=False)
    return x, chord


@pytest.fixture(scope="module")
def cases():
    """shape -> (x, chord); and the restatement's answer per (shape, custom_round), computed once and shared."""
    data = {s: make_case(*s, seed=21 + i) for i, s in enumerate(SHAPES)}
    base = {(s, custom): ref.recognize_rolls(x, s[1], custom_round=custom) for s, (x, _) in data.items() for custom in (False, True)}
    return data, base


def expected(cases, shape, mode):
    data, base = cases
    with_chord, custom, rel = mode
    want = {k: v.copy() for k, v in base[shape, custom].items()}
    if with_chord:
        for s in range(shape[0]):
            c = ref.compare(want["rows"][s], data[shape][1][s], rel)
            c[I["BEATS"]], c[I["SEGMENTS"]] = want["counters"][s, I["BEATS"]], want["counters"][s, I["SEGMENTS"]]
            want["counters"][s] = c
    want["bounds"] = want.pop("starts")
    return want


def guarded(shape, dtype):
    """(whole int32 buffer, payload view of `dtype`): an output pre-filled with garbage between two runs of sentinels."""
    words = int(np.prod(shape)) * (2 if dtype == torch.float64 else 1)
    whole = torch.full((words + 2 * PAD,), SENTINEL, device="cuda", dtype=torch.int32)
    whole[PAD: PAD + words] = GARBAGE
    return whole, whole[PAD: PAD + words].view(dtype).view(*shape)


def untouched(whole):
    return bool((whole[:PAD] == SENTINEL).all()) and bool((whole[-PAD:] == SENTINEL).all())


def launch(lib, x, segments, chord, custom, rel, outs=None):
    """One pf_chord_recognize call on device tensors; returns name -> (guarded buffer, view)."""
    n, steps = x.shape[0], x.shape[2]
    songs, beats = n // segments, segments * steps // 4
    shapes = dict(labels=(songs, beats), bounds=(songs, beats), rows=(songs, beats, 36), counters=(songs, 8), path_score=(songs,),
                  chroma_q=(songs, beats, 12), bass_q=(songs, beats, 12))
    bufs = outs or {k: guarded(shapes[k], DTYPES[k]) for k in OUTPUTS}
    bits, const, rows, consts = chordrec._device_tables(x.device)
    host = chordrec.vocabulary_tables()
    a = _lib.ChordRecognizeArgs(prmat2c=x.data_ptr(), chord=None if chord is None else chord.data_ptr(), cls_bits=bits.data_ptr(),
                                cls_const=const.data_ptr(), cls_rows=rows.data_ptr(), consts=consts.data_ptr(), songs=songs, segments=segments,
                                steps=steps, n_classes=len(host["names"]), max_template=host["max_template"], custom_round=int(custom),
                                bass_relative=int(rel), reserved=0, **{k: bufs[k][1].data_ptr() for k in OUTPUTS})
    _lib.check(lib.pf_chord_recognize(C.byref(a), _lib.current_stream()), "pf_chord_recognize", lib)
    return bufs


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def assert_equal(bufs, want, what):
    for name in OUTPUTS:
        whole, got = bufs[name]
        assert untouched(whole), (what, name, "sentinel overwritten")
        g, w = got.cpu().numpy(), want[name]
        if name == "path_score":
            g, w = g.view(np.int64), np.asarray(w, np.float64).view(np.int64)                  # bit for bit
        elif name == "rows":
            g, w = g.view(np.uint32), np.asarray(w, np.float32).view(np.uint32)
        else:
            g = g.astype(np.int64)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (what, name, len(bad), bad[:8].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


@pytest.mark.parametrize("mode", MODES, ids=lambda m: "chord%d-custom%d-rel%d" % m)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "songs%d-seg%d-steps%d" % s)
def test_every_word_equals_the_restatement(lib, cases, shape, mode):
    x, chord = cases[0][shape]
    want = expected(cases, shape, mode)
    print(f"{shape} {mode}: counters summed over the songs {dict(zip(ref.NAMES, want['counters'].sum(0).tolist()))}, path scores "
          f"{want['path_score'].tolist()}, distinct labels {len(np.unique(want['labels']))}")
    bufs = launch(lib, dev(x), shape[1], dev(chord) if mode[0] else None, mode[1], mode[2])
    torch.cuda.synchronize()
    assert_equal(bufs, want, (shape, mode))
    if not mode[0]:
        assert (want["counters"][:, 1:7] == 0).all()                                           # written as zeros: GARBAGE would show


def test_the_cases_hold_what_they_are_meant_to(cases):
    """The restatement's own answers show that the comparison has something to bite on: hits and misses, both rounding modes and both bass
    conventions giving different words, several labels, several segments per song."""
    data, base = cases
    shape = (5, 1, 128)
    plain, custom = base[shape, False], base[shape, True]
    assert not np.array_equal(plain["chroma_q"], custom["chroma_q"]) and not np.array_equal(plain["labels"], custom["labels"])
    assert len(np.unique(plain["labels"])) > 10 and (plain["counters"][:, I["SEGMENTS"]] >= 8).all()
    absolute, relative = expected(cases, shape, (True, False, False))["counters"], expected(cases, shape, (True, False, True))["counters"]
    assert (absolute[:, I["FULL_HIT"]] >= 16).all() and (absolute[:, I["FULL_HIT"]] < 32).all()
    assert not np.array_equal(absolute[:, I["BASS_HIT"]], relative[:, I["BASS_HIT"]])
    x = data[shape][0]
    assert x[0, 0, 0, 0] == 1.0 and x[-1, 0, 127, 127] == 1.0 and np.isnan(x).any()
    assert plain["bass_q"][0, 0, 0] >= 2 and plain["chroma_q"][-1, -1, 127 % 12] >= 1            # keys 0 and 127 reach the features


def test_planted_cases(lib):
    names = ref.vocabulary().names
    for name, (x, segments, labels) in chordrec_cases.planted().items():
        want = ref.recognize_rolls(x, segments)
        want["bounds"] = want.pop("starts")
        bufs = launch(lib, dev(x), segments, None, False, False)
        torch.cuda.synchronize()
        assert_equal(bufs, want, name)
        if labels is not None:
            assert [names[i] for i in bufs["labels"][1][0].tolist()] == labels, name
    x = chordrec_cases.planted()["keys_0_and_127"][0]
    assert x[0, 0, 0, 0] == 1 and x[0, 0, 0, 127] == 1                                          # really in the data


def test_two_calls_agree_and_a_split_batch_equals_the_whole(lib, cases):
    for shape, cut in (((5, 1, 128), 2), ((2, 3, 128), 1)):
        x, chord = (dev(a) for a in cases[0][shape])
        mode = (True, True, True)
        first, second = launch(lib, x, shape[1], chord, *mode[1:]), launch(lib, x, shape[1], chord, *mode[1:])
        for k in OUTPUTS:
            assert torch.equal(first[k][1].view(torch.int32), second[k][1].view(torch.int32)), k
        seg = shape[1]
        parts = [launch(lib, x[a * seg: b * seg].contiguous(), seg, chord[a:b].contiguous(), *mode[1:]) for a, b in ((0, cut), (cut, shape[0]))]
        for k in OUTPUTS:
            assert torch.equal(torch.cat([parts[0][k][1], parts[1][k][1]]).view(torch.int32), first[k][1].view(torch.int32)), k
        assert_equal(first, expected(cases, shape, mode), shape)


def test_a_captured_launch_replays_the_same_words(lib, cases):
    shape, mode = (3, 1, 48), (True, False, False)
    x, chord = (dev(a) for a in cases[0][shape])
    bufs = launch(lib, x, shape[1], chord, *mode[1:])                              # eager first: the module and the tables are loaded outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch(lib, x, shape[1], chord, *mode[1:], outs=bufs)
    for _, view in bufs.values():
        view.view(torch.int32).fill_(GARBAGE)
    g.replay()
    torch.cuda.synchronize()
    assert_equal(bufs, expected(cases, shape, mode), "graph replay")
    x.copy_(torch.roll(x, 1, 0))                                                   # the graph reads its inputs where they are
    g.replay()
    torch.cuda.synchronize()
    want = ref.recognize_rolls(np.roll(cases[0][shape][0], 1, 0), shape[1], cases[0][shape][1])
    want["bounds"] = want.pop("starts")
    assert_equal(bufs, want, "graph replay on new values")


# ---------------------------------------------------------------------------------------------- the Python layer
def file_rows(x, tmp_path):
    from oracle import notes_ref
    from polyffusion_amd import chord_extractor, midi
    origin, _ = notes_ref.note_lists(x)
    midi.write_smf(str(tmp_path / "roll.mid"), [origin])
    return chord_extractor.recognize(chord_extractor.PrettyMIDI(str(tmp_path / "roll.mid")))


def test_recognize_rolls_flattens_leading_shapes_and_its_lab_rows_are_the_file_paths(tmp_path, cases):
    x, chord = cases[0][(2, 3, 128)]
    want = expected(cases, (2, 3, 128), (True, False, False))
    rec = chordrec.recognize_rolls(dev(x.reshape(2, 3, 2, 128, 128)), 3, dev(chord.reshape(2 * 96, 36)))
    assert rec.labels.is_cuda and rec.labels.dtype == torch.int32 and rec.path_score.dtype == torch.float64 and rec.rows.shape == (2, 96, 36)
    for k in OUTPUTS:
        assert np.array_equal(getattr(rec, k).cpu().numpy(), want[k].astype(getattr(rec, k).cpu().numpy().dtype)), k
    sc, want_sc = rec.scores(), ref.scores(want["counters"])
    for k in want_sc:
        assert sc[k].is_cuda and sc[k].dtype == torch.float64 and np.array_equal(sc[k].cpu().numpy(), want_sc[k]), k
    assert 0 < float(sc["chord_acc"][0]) < 1
    for song in range(2):                                                          # two rolls through the real file path
        assert rec.lab_rows(song) == file_rows(x[3 * song: 3 * song + 3], tmp_path)
    assert rec.names()[1] == [ref.vocabulary().names[i] for i in want["labels"][1]] and rec.report()[0]["counters"]["BEATS"] == 96
    with pytest.raises(ValueError, match="chord rows"):
        chordrec.recognize_rolls(dev(x), 3, dev(chord[:1]))
    with pytest.raises(ValueError, match="whole number of bars"):
        chordrec.recognize_rolls(torch.zeros(1, 2, 20, 128, device="cuda"))
    with pytest.raises(ValueError, match="whole songs"):
        chordrec.recognize_rolls(dev(x), 4)


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


def recognized(song, chord):
    """the restatement's report of one written song [B, 2, 128, 128] against chord [B, 32, 36]"""
    got = ref.recognize_rolls(song, song.shape[0], None if chord is None else chord.reshape(1, -1, 36))
    sc = ref.scores(got["counters"])
    names = ref.vocabulary().names
    return dict({k: float(v[0]) for k, v in sc.items()}, counters={n: int(got["counters"][0, i]) for n, i in I.items()},
                labels=[names[i] for i in got["labels"][0]])


def test_score_chords_adds_the_recognition_and_without_the_flag_nothing_changes(tmp_path, capsys):
    chord = synth.chords(2, SEED + 100)
    files, doc, said = run_main(tmp_path / "with", ["--synthetic", "--length", "2", "--num_generate", "2", "--score", "--score_chords"], capsys)
    assert sorted(files) == [0, 1] and len(doc["recognized"]) == 2
    for i in (0, 1):
        want = recognized(files[i], chord)
        assert doc["recognized"][i] == dict(want, candidate=i), i
        assert all(doc["songs"][i][k] == want[k] for k in chordrec.SCORES)
        assert f"song {i} chords: chord_acc {want['chord_acc']:.4f}" in said
    plain, none, _ = run_main(tmp_path / "without", ["--synthetic", "--length", "2", "--num_generate", "2", "--score"], capsys)
    assert "recognized" not in none and "chord_acc" not in none["songs"][0] and "chords:" not in _
    assert all(np.array_equal(plain[i].view(np.uint32), files[i].view(np.uint32)) for i in (0, 1))
    assert {k: v for k, v in doc.items() if k != "recognized"}["candidates"][0].keys() - none["candidates"][0].keys() == set(chordrec.SCORES)


def test_rank_by_extracted_keeps_the_candidates_the_restatement_ranks_first(tmp_path, capsys):
    import score_ref
    chord = synth.chords(1, SEED + 100)
    plain, none, _ = run_main(tmp_path / "plain", ["--synthetic", "--length", "1", "--num_generate", "4"])
    kept, doc, said = run_main(tmp_path / "best", ["--synthetic", "--length", "1", "--num_generate", "2", "--best_of", "2", "--rank_by", "extracted"], capsys)
    assert none is None and sorted(plain) == [0, 1, 2, 3] and sorted(kept) == [0, 1]
    want = [recognized(plain[i], chord) for i in range(4)]
    order = score_ref.rank([w["chord_acc"] for w in want], 2)
    print("chord_acc of the four candidates:", [w["chord_acc"] for w in want], "kept:", order)
    for r, cand in enumerate(order):
        assert np.array_equal(kept[r].view(np.uint32), plain[cand].view(np.uint32)), (r, cand)
    assert doc["rank_by"] == "extracted" and [s["candidate"] for s in doc["songs"]] == order
    assert [c["chord_acc"] for c in doc["candidates"]] == [w["chord_acc"] for w in want]
    assert doc["recognized"] == [dict(want[c], candidate=c) for c in order] and "by chord_acc are kept" in said


def chordful_song(bars):
    """(chord [1, 32, 36], image [1, 2, 128, 128]): eight bars, each beat its bar's chord as a block - the bass class lowest, the other template
    classes an octave above, struck on the beat and held for it"""
    v = ref.vocabulary()
    chord, image = np.zeros((1, 32, 36), np.float32), np.zeros((1, 2, 128, 128), np.float32)
    for bar, name in enumerate(bars):
        i = v.names.index(name)
        keys = [36 + int(v.bass[i])] + [48 + k for k in range(12) if v.tpl[i, k] and k != v.bass[i]]
        for j in range(4 * bar, 4 * bar + 4):
            chord[0, j] = v.rows[i]
            image[0, 0, 4 * j, keys] = 1
            image[0, 1, 4 * j + 1: 4 * j + 4, keys] = 1
    return chord, image


def test_rank_by_extracted_when_inpainting_a_song_that_plays_its_chords(tmp_path, capsys):
    """The kept bars of the source play the conditioning chords, so chord_acc is far from 0 here, unlike in the run above.  (On synthetic
    weights the invented bars give none of their chords back, so the candidates tie at 6 bars of 8 and the stable ranking keeps the first
    ones: that the ranking orders distinct values is test_score_host's business.)"""
    import score_ref
    chord, image = chordful_song(["C:maj", "G:maj", "A:min", "F:maj", "D:min", "G:7", "C:maj/3", "C:maj"])
    assert recognized(image, chord)["chord_acc"] == 1.0                                          # the source itself gives its chords back
    np.savez(tmp_path / "song.npz", chord=chord, prmat2c=image)
    extra = ["--cond_npz", str(tmp_path / "song.npz"), "--inpaint_type", "bars", "--bar_list", "2,3"]
    plain, none, _ = run_main(tmp_path / "plain", ["--num_generate", "4"] + extra)
    kept, doc, said = run_main(tmp_path / "best", ["--num_generate", "2", "--best_of", "2", "--rank_by", "extracted"] + extra, capsys)
    want = [recognized(plain[i], chord) for i in range(4)]
    acc = [w["chord_acc"] for w in want]
    order = score_ref.rank(acc, 2)
    print("chord_acc of the four inpainted candidates:", acc, "kept:", order)
    assert min(acc) >= 0.5                                                                       # six of the eight bars are the source's
    for r, cand in enumerate(order):
        assert np.array_equal(kept[r].view(np.uint32), plain[cand].view(np.uint32)), (r, cand)
    assert [s["candidate"] for s in doc["songs"]] == order and [c["chord_acc"] for c in doc["candidates"]] == acc
    assert doc["recognized"] == [dict(want[c], candidate=c) for c in order]


def test_edit_score_chords_prints_the_four_accuracies_of_the_restatement(tmp_path, capsys):
    from polyffusion_amd.inference_sdf import shift_chords
    rng = np.random.default_rng(9)
    chord, image = synth.chords(1, 42), (rng.random((1, 2, 128, 128)) > 0.95).astype(np.float32)
    np.savez(tmp_path / "song.npz", chord=chord, prmat2c=image)
    files, doc, said = run_main(tmp_path / "edit", ["--cond_npz", str(tmp_path / "song.npz"), "--edit", "--edit_iters", "1", "--edit_chord_shift", "2",
                                                    "--score", "--score_chords"], capsys)
    target = shift_chords(torch.from_numpy(chord), 2).numpy()
    want = {"source_on_source_chords": recognized(image, chord), "source_on_target_chords": recognized(image, target),
            "edited_on_source_chords": recognized(files[0], chord), "edited_on_target_chords": recognized(files[0], target)}
    assert {k: doc[k]["recognized"] for k in want} == want and all("chord_f1" in doc[k] for k in want)
    line = [ln for ln in said.splitlines() if ln.startswith("edit score (chord_acc)")]
    assert len(line) == 1 and [float(v) for v in re.findall(r"chords ([0-9.e+-]+)", line[0])] == [w["chord_acc"] for w in want.values()]


def test_morph_score_chords_gives_every_frame_its_accuracy_on_both_songs(tmp_path, capsys):
    a, b = chordful_song(["C:maj"] * 8), chordful_song(["A:min", "F:maj"] * 4)
    for name, (chord, image) in (("a", a), ("b", b)):
        np.savez(tmp_path / f"{name}.npz", chord=chord, prmat2c=image)
    from polyffusion_amd import inference_sdf
    argv = ["--params_preset", "sdf_chd8bar", "--synthetic_weights", "--morph", "--ddim", "--ddim_steps", "2", "--morph_frames", "3", "--morph_iters", "1",
            "--score", "--score_chords", "--seed", "9", "--output_dir", str(tmp_path / "out"), "--cond_npz", str(tmp_path / "a.npz"), "--morph_to_npz",
            str(tmp_path / "b.npz")]
    assert inference_sdf.main(argv) == 0
    said = capsys.readouterr().out
    gen = np.load(glob.glob(str(tmp_path / "out" / "*_morph.npy"))[0])
    doc = json.load(open(glob.glob(str(tmp_path / "out" / "*_score.json"))[0]))
    assert gen.shape == (3, 1, 2, 128, 128)
    for col, (chord, _) in (("chord_acc_on_a", a), ("chord_acc_on_b", b)):
        assert doc[col] == [recognized(gen[k], chord)["chord_acc"] for k in range(3)], col
    assert doc["recognized"] == [recognized(gen[k], None)["labels"] for k in range(3)] and len(doc["chord_f1_on_a"]) == 3
    print("morph chord_acc on A:", doc["chord_acc_on_a"], "on B:", doc["chord_acc_on_b"])
    assert f"chord_acc: on A's chords {doc['chord_acc_on_a'][0]:.4f}, on B's chords {doc['chord_acc_on_b'][0]:.4f}" in said
