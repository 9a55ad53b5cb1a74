"""Chord recognition without a GPU: ``tests/chordrec_ref.py`` (the numpy restatement the GPU tests compare against) equals the real path
``oracle.notes_ref.note_lists -> midi.write_smf -> chord_extractor.recognize`` label for label on seeded random rolls, and does what it
should on planted cases; the vocabulary tables equal ``chd_to_onehot(chord_matrix_from_labels(...))``; ``pf_chord_recognize`` is declared,
exported by both builds and bound, its struct and enum are laid out as the header says, bad arguments are refused before any launch; the
comparison counters and scores on hand-made rows; and the CLI's refusals and defaults."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import chordrec_cases as cases
import chordrec_ref as ref
from oracle import notes_ref
from polyffusion_amd import _lib, chord_extractor, chordrec, midi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000          # a non-null, 8-byte aligned address that a refused call never touches
I = ref.IDX


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from polyffusion_amd.build import build
        build(verbose=False)
    return _lib.load()


def header():
    return open(os.path.join(REPO, "include", "pfhip.h")).read()


def file_path_rows(x, tmp_path, custom_round=False):
    """[start, end, label] rows of the real path: the reference's note lists, the product's file writer, the restated extractor"""
    origin, _ = notes_ref.note_lists(x, None, custom_round)
    path = str(tmp_path / "roll.mid")
    midi.write_smf(path, [origin])
    return chord_extractor.recognize(chord_extractor.PrettyMIDI(path))


def per_beat(rows):
    out = []
    for start, end, label in rows:
        assert start * 2 == int(start * 2) and end * 2 == int(end * 2)
        out += [label] * (int(end * 2) - int(start * 2))
    return out


# ---------------------------------------------------------------------------------------------- the restatement is the real path
@pytest.mark.parametrize("custom_round", [False, True])
def test_restatement_equals_the_file_path_on_every_beat(tmp_path, custom_round):
    names = ref.vocabulary().names
    beats = differing = overlapping = 0
    seed = 1000 * custom_round
    for segments, steps in cases.SHAPES:
        for density in cases.DENSITIES:
            for overlaps in (False, True):
                seed += 1
                x = cases.random_roll(seed, segments, steps, density, overlaps)
                want = file_path_rows(x, tmp_path, custom_round)
                got = ref.recognize_rolls(x, segments, custom_round=custom_round)
                got_names = [names[i] for i in got["labels"][0]]
                want_names = per_beat(want)
                assert len(want_names) == len(got_names) == segments * steps // 4            # the note in the last step: the file has every beat
                beats += len(got_names)
                differing += sum(a != b for a, b in zip(want_names, got_names))
                assert ref.lab_rows(got["labels"][0], got["starts"][0]) == want, (segments, steps, density, overlaps)
                on = (x[:, 0] > 0.5)
                overlapping += int((on[:, 1:] & (x[:, 1, 1:] > 0.5) & ((x[:, 0, :-1] > 0.5) | (x[:, 1, :-1] > 0.5))).sum()) if overlaps else 0
    assert beats == 2 * 3 * (4 + 12 + 32 + 8 + 64) and differing == 0
    assert overlapping > 0                                                                   # same-key overlaps are really in the data


# ---------------------------------------------------------------------------------------------- planted cases
def test_planted_cases(tmp_path):
    names = ref.vocabulary().names
    planted = cases.planted()
    for name, (x, segments, expected) in planted.items():
        got = ref.recognize_rolls(x, segments)
        got_names = [names[i] for i in got["labels"][0]]
        if expected is not None:
            assert got_names == expected, name
        if name != "empty":
            assert ref.lab_rows(got["labels"][0], got["starts"][0]) == file_path_rows(x, tmp_path), name
    q = lambda name: ref.features(planted[name][0])
    # clipped at the segment end: the three notes cover beat 3 only, the orphan sustains of segment 1 are no notes
    chroma, bass = q("clipped_at_segment_end")
    assert chroma[3].tolist() == [4, 0, 0, 0, 4, 0, 0, 4, 0, 0, 0, 0] and chroma[4:7].sum() == 0 and chroma[7, 0] == 1
    assert [n for n in ref.notes(planted["clipped_at_segment_end"][0]) if n[0] == 60] == [(60, 12, 16)]
    # a quarter beat on either side of the beat line
    chroma, bass = q("quarter_beat_overlap")
    assert chroma[0, 2] == 1 and chroma[1, 2] == 1 and bass[0, 2] == 2 and bass[1, 2] == 2
    # C and G: the three triads on C with a fifth tie, the lowest index wins
    v = ref.vocabulary()
    sc = ref.class_scores(*[t[0] for t in q("c_g_tie")])
    tie = [v.names.index(n) for n in ("C:maj", "C:min", "C:sus4")]
    assert sc[tie[0]] == sc[tie[1]] == sc[tie[2]] == sc.max() and int(np.argmax(sc)) == tie[0] == min(tie)
    # empty: all N, one segment per ... the DP still cuts it; every feature zero
    got = ref.recognize_rolls(planted["empty"][0], 1)
    assert got["chroma_q"].sum() == 0 and got["bass_q"].sum() == 0 and (got["labels"] == 0).all()
    # NaN and negative cells are silent: only key 50 sounds, and its NaN sustain ends the first note after one step
    chroma, bass = q("nan_and_negative")
    assert chroma.sum() == 2 and chroma[0, 2] == 1 and chroma[3, 2] == 1 and bass.sum() == 4
    # keys 0 and 127 are really in the data: key 0 is the bass of the first two beats, key 127 sounds throughout
    x = planted["keys_0_and_127"][0]
    assert x[0, 0, 0, 0] == 1 and x[0, 0, 0, 127] == 1
    chroma, bass = q("keys_0_and_127")
    assert bass[:2, 0].tolist() == [8, 8] and chroma[:, 127 % 12].tolist() == [4, 4, 4, 4] and bass[2:, 64 % 12].tolist() == [8, 8]


def test_refusals_of_the_definition():
    with pytest.raises(AssertionError):
        ref.recognize_rolls(np.zeros((1, 2, 20, 128), np.float32))
    with pytest.raises(AssertionError):
        ref.recognize_rolls(np.zeros((3, 2, 16, 128), np.float32), segments=2)


# ---------------------------------------------------------------------------------------------- vocabulary
def test_vocabulary_tables_are_the_label_functions():
    from polyffusion_amd.datasample import chd_to_onehot
    t = chordrec.vocabulary_tables()
    cc = chord_extractor.ChordClass()
    v = ref.vocabulary()
    assert t["names"] == cc.chord_list == v.names and len(t["names"]) == 529
    for i, name in enumerate(cc.chord_list):
        row = chd_to_onehot(chord_extractor.chord_matrix_from_labels([[0, .5, name]]))
        assert row.shape == (1, 36) and np.array_equal(t["cls_rows"][i], row[0]), name
        tpl = cc.chroma_templates[i] > 0
        assert t["cls_bits"][i] & 0xFFF == sum(1 << k for k in range(12) if tpl[k]) == v.template[i]
        assert (t["cls_bits"][i] >> 16) & 15 == tpl.sum() == v.size[i]
        if i:
            assert (t["cls_bits"][i] >> 12) & 15 == int(np.argmax(cc.bass_templates[i])) == v.bass[i]
        assert t["cls_const"][i, 0] == tpl.sum() * 0.1 == v.c_size[i] and t["cls_const"][i, 1] == ("/" in name) * 0.05 == v.c_slash[i]
    assert np.array_equal(t["cls_rows"], v.rows)
    assert sorted({int(s) for s in (t["cls_bits"] >> 16) & 15}) == [0, 3, 4, 5, 6, 7] and t["max_template"] == 7
    assert len({tuple(r) for r in t["cls_rows"].tolist()}) == 325
    assert t["names"][0] == "N" and np.flatnonzero(t["cls_rows"][0]).tolist() == [34, 35]        # the root = -1 indexing of the --from_midi path
    assert t["consts"].tolist() == [j * 0.7 for j in range(12)] + [0.15, 0.2, 0.2, 0.0]
    assert t["cls_bits"].dtype == np.int32 and t["cls_const"].dtype == np.float64 and t["cls_rows"].dtype == np.float32
    assert len(t["names"]) <= _lib.CHORDREC_MAX_CLASSES


# ---------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_and_both_builds_export_the_entry_point(lib):
    hdr = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    declared = set(re.findall(r"\b(pf_[a-z0-9_]+)\s*\(", hdr))
    if not os.path.exists(_lib.lib_path("f16")):
        from polyffusion_amd.build import build
        build(verbose=False, variant="f16")
    assert "pf_chord_recognize" in declared and "pf_chord_recognize" in _lib.SIGNATURES
    assert hasattr(lib, "pf_chord_recognize") and hasattr(_lib.load("f16"), "pf_chord_recognize")
    assert _lib.SIGNATURES["pf_chord_recognize"] == (C.c_int, [C.POINTER(_lib.ChordRecognizeArgs), C.c_void_p])


def test_struct_and_enum_are_laid_out_as_the_header_says():
    hdr = header()
    body = re.search(r"typedef struct pf_chord_recognize_args \{(.*?)\} pf_chord_recognize_args;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    order = [n.strip(" *") for decl in re.findall(r"(?:const )?(?:float|double|int32_t)\s*\*?\s*([^;]+);", body) for n in decl.split(",")]
    f = _lib.ChordRecognizeArgs
    assert order == [n for n, _ in f._fields_] == ["prmat2c", "chord", "cls_bits", "cls_const", "cls_rows", "consts", "songs", "segments", "steps",
                                                   "n_classes", "max_template", "custom_round", "bass_relative", "reserved", "labels", "bounds",
                                                   "rows", "counters", "path_score", "chroma_q", "bass_q"]
    offsets = [0, 8, 16, 24, 32, 40, 48, 52, 56, 60, 64, 68, 72, 76, 80, 88, 96, 104, 112, 120, 128]
    assert {n: getattr(f, n).offset for n in order} == dict(zip(order, offsets)) and C.sizeof(f) == 136
    enum = re.findall(r"PF_CHORDREC_([A-Z_]+) = (\d+)", hdr)
    assert [n for n, _ in enum] == list(_lib.CHORDREC_COUNTERS) == list(ref.NAMES) and [int(v) for _, v in enum] == list(range(8))
    define = lambda name: int(re.search(rf"#define {name} (\d+)", hdr).group(1))
    assert define("PF_CHORDREC_NCOUNT") == _lib.CHORDREC_NCOUNT == ref.NCOUNT == 8
    assert define("PF_CHORDREC_MAX_BEATS") == _lib.CHORDREC_MAX_BEATS >= 16 * 128 // 4
    assert define("PF_CHORDREC_MAX_CLASSES") == _lib.CHORDREC_MAX_CLASSES >= 529


def test_bad_arguments_are_refused_before_any_launch(lib):
    """No GPU needed: the call returns before it touches HIP or any of the (fake) pointers."""
    pointers = ("prmat2c", "chord", "cls_bits", "cls_const", "cls_rows", "consts", "labels", "bounds", "rows", "counters", "path_score", "chroma_q",
                "bass_q")

    def refused(pattern, **fields):
        a = _lib.ChordRecognizeArgs()
        kw = dict({n: FAKE + 0x10000 * i for i, n in enumerate(pointers)}, songs=2, segments=1, steps=16, n_classes=529, max_template=7)
        kw.update(fields)
        for k, v in kw.items():
            setattr(a, k, v)
        rc = lib.pf_chord_recognize(C.byref(a), None)
        msg = lib.pf_last_error().decode()
        assert rc < 0 and re.search(pattern, msg), (fields, rc, msg)

    refused("chord_recognize: bad arguments.*prmat2c", prmat2c=None)
    for name in ("songs", "segments", "steps"):
        refused(f"chord_recognize: bad arguments.*{name} = 0", **{name: 0})
        refused(f"chord_recognize: bad arguments.*{name} = -3", **{name: -3})
    for steps in (20, 4, 8, 127):
        refused(f"steps = {steps} is not a whole number of bars", steps=steps)
    refused("more than 512 beats", segments=17, steps=128)
    refused("more than 512 beats", segments=1, steps=2064)
    for name in ("cls_bits", "cls_const", "cls_rows", "consts"):
        refused(f"null vocabulary table.*{name}", **{name: None})
    for n in (0, -1, 577):
        refused("n_classes = -?\\d+ outside 1..576", n_classes=n)
    for n in (0, 13):
        refused("max_template = \\d+ outside 1..12", max_template=n)
    for name in pointers[6:]:
        refused(f"null output.*{name}", **{name: None})
    for name in pointers:
        refused("aligned", **{name: FAKE + 0x200002})
    for name in ("cls_const", "consts", "path_score"):
        refused("8-byte", **{name: FAKE + 0x200004})
    assert lib.pf_chord_recognize(None, None) < 0 and re.search("pf_chord_recognize: null arguments", lib.pf_last_error().decode())


# ---------------------------------------------------------------------------------------------- comparison counters and scores
def row(root=None, chroma=(), bass=None):
    r = np.zeros(36, np.float32)
    if root is not None:
        r[root] = 1
    r[[12 + k for k in chroma]] = 1
    if bass is not None:
        r[24 + bass] = 1
    return r


def test_comparison_counters_and_scores_on_hand_made_rows():
    v = ref.vocabulary()
    cmaj, gseven, none = v.rows[v.names.index("C:maj")], v.rows[v.names.index("G:7")], v.rows[0]
    cmaj_e = v.rows[v.names.index("C:maj/3")]
    assert np.array_equal(cmaj, row(0, (0, 4, 7), 0)) and np.array_equal(gseven, row(7, (7, 11, 2, 5), 7)) and np.array_equal(cmaj_e, row(0, (0, 4, 7), 4))
    rec = np.stack([cmaj, cmaj, gseven, none, cmaj_e, cmaj])
    cond = np.stack([row(0, (0, 4, 7), 0),          # all three
                     row(0, (0, 3, 7), 0),          # root and bass, not the chroma: 2 of 4 in common
                     row(7, (7, 11, 2, 5), 2),      # root and chroma, another bass
                     np.zeros(36, np.float32),      # the N row against an empty row: root and chroma agree (both lack), the bass bits of N do not
                     row(0, (0, 4, 7), 4),          # the inversion, bass absolute
                     row(5, (5, 9, 0), 5)])         # nothing but one common class
    c = ref.compare(rec, cond)
    assert [int(c[I[k]]) for k in ("ROOT_HIT", "CHROMA_HIT", "BASS_HIT", "FULL_HIT")] == [5, 4, 3, 2]
    assert c[I["CHROMA_INTER"]] == 3 + 2 + 4 + 0 + 3 + 1 and c[I["CHROMA_UNION"]] == 3 + 4 + 4 + 0 + 3 + 5
    # the bass_relative reading: a condition whose bass block holds the offset from the root
    rel = cond.copy()
    rel[:, 24:36] = 0
    rel[0, 24 + 0] = rel[1, 24 + 0] = rel[4, 24 + 4] = rel[5, 24 + 0] = 1
    rel[2, 24 + (2 - 7) % 12] = 1
    assert np.array_equal(ref.compare(rec, rel, bass_relative=True), c)
    # read as absolute, the offsets give other answers: beat 5's offset 0 is C, the recognised bass, though the condition's bass is F
    assert ref.compare(rec[5:6], rel[5:6])[I["BASS_HIT"]] == 1 and ref.compare(rec[5:6], rel[5:6], bass_relative=True)[I["BASS_HIT"]] == 0
    assert ref.compare(rec, rel)[I["BASS_HIT"]] == 5
    # ties go to the lowest index, values at 0.5 are not set, a NaN never wins
    t = row(3, (3,), 3)
    t[5], t[1] = 1, np.nan
    assert ref.compare(row(3, (3,), 3)[None], t[None])[I["ROOT_HIT"]] == 1
    half = row(0, (0, 4, 7), 0)
    half[12 + 9] = 0.5
    assert ref.compare(cmaj[None], half[None])[I["CHROMA_HIT"]] == 1
    # the ratios, 0 / 0 = 0, and the product's torch form of them
    import torch
    counters = np.zeros((3, 8), np.int64)
    counters[0] = [6, 5, 4, 3, 2, 13, 19, 4]
    counters[1] = [32, 32, 32, 32, 32, 96, 96, 8]
    sc = ref.scores(counters)
    assert sc["chord_acc"].tolist() == [2 / 6, 1.0, 0.0] and sc["root_acc"].tolist() == [5 / 6, 1.0, 0.0] and sc["chroma_acc"][0] == 4 / 6
    assert sc["bass_acc"][0] == 3 / 6 and sc["chroma_iou"].tolist() == [13 / 19, 1.0, 0.0]
    got = chordrec.scores_of(torch.from_numpy(counters).to(torch.int32))
    assert set(got) == set(sc) == set(chordrec.SCORES)
    for k in sc:
        assert got[k].dtype == torch.float64 and np.array_equal(got[k].numpy(), sc[k]), k


def test_lab_rows_and_report_of_the_python_layer_need_no_gpu():
    import torch
    v = ref.vocabulary()
    x = cases.random_roll(7, 2, 16, 0.5, True)
    got = ref.recognize_rolls(x, 2)
    z = torch.zeros(0)
    rec = chordrec.ChordRecognition(torch.from_numpy(got["labels"]).int(), torch.from_numpy(got["starts"]).int(), z,
                                    torch.from_numpy(got["counters"]).int(), z, z, z)
    assert rec.lab_rows(0) == ref.lab_rows(got["labels"][0], got["starts"][0])
    assert rec.names() == [[v.names[i] for i in got["labels"][0]]]
    rep = rec.report()[0]
    assert rep["labels"] == rec.names()[0] and rep["counters"]["BEATS"] == 8 and rep["counters"]["SEGMENTS"] == int(got["starts"].sum())
    assert rep["chord_acc"] == 0.0 and set(rep) == set(chordrec.SCORES) | {"counters", "labels"}


# ---------------------------------------------------------------------------------------------- the CLI
def test_parser_defaults_and_refusals(tmp_path):
    from polyffusion_amd import inference_sdf, score
    p = inference_sdf.make_parser()
    a = p.parse_args([])
    assert a.score_chords is False and a.rank_by == "chord" and inference_sdf.recognizing(a) is False
    assert score.RANK_BY["extracted"] == ("chord_acc", True)
    assert "chord_acc" not in score.SCORES                                                    # the key set of the roll statistics stays
    assert inference_sdf.check_score_args(p.parse_args(["--score", "--score_chords"]), "chord") is True
    assert inference_sdf.check_score_args(p.parse_args(["--best_of", "2", "--rank_by", "extracted"]), "chord+txt") is True
    assert inference_sdf.recognizing(p.parse_args(["--score", "--score_chords"])) and inference_sdf.recognizing(p.parse_args(["--best_of", "2", "--rank_by", "extracted"]))
    assert not inference_sdf.recognizing(p.parse_args(["--best_of", "2"]))

    def refused(pattern, argv, cond_type=None):
        with pytest.raises(SystemExit, match=pattern):
            inference_sdf.check_score_args(p.parse_args(argv), cond_type)

    refused("--score_chords: these belong to --score", ["--score_chords"])
    refused("belong to --score", ["--rank_by", "extracted"])
    refused("needs the chords", ["--best_of", "2", "--rank_by", "extracted"], "txt")
    refused("needs the chords", ["--best_of", "2", "--rank_by", "extracted"], "pnotree")
    with pytest.raises(SystemExit):
        p.parse_args(["--rank_by", "key"])
    # the stand-alone scorer
    np.save(tmp_path / "roll.npy", np.zeros((1, 2, 128, 128), np.float32))
    with pytest.raises(SystemExit, match="--lab belongs to --chords"):
        score.main(["--npy", str(tmp_path / "roll.npy"), "--lab", str(tmp_path / "out.lab")])
    # songs longer than the recogniser holds are refused with a message, not a traceback
    import torch
    with pytest.raises(SystemExit, match="at most 512 beats"):
        inference_sdf.recognize_songs(torch.zeros(1, 17, 2, 128, 128), None, p.parse_args(["--score", "--score_chords"]))
    line = inference_sdf.chords_line({**{k: 0.5 for k in chordrec.SCORES}, "counters": {"BEATS": 4}, "labels": ["C:maj", "C:maj", "N", "G:7"]})
    assert line.endswith("chords: C:maj*2 N G:7") and "chord_acc 0.5000" in line and "BEATS 4" in line
