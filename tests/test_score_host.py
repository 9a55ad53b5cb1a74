"""Roll statistics without a GPU: ``pf_roll_stats`` is declared, exported by both builds and bound, its struct and enum are laid out as the
header says, bad arguments are refused before any launch; ``tests/score_ref.py`` (the numpy restatement the GPU tests compare against) on
hand-built rolls with known answers and against ``midi.check_prmat2c_integrity``; the product's ratios, song sums, texture cosine and
ranking (torch code that runs where its tensors live) against ``score_ref``; and the CLI's refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import score_ref
from polyffusion_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000          # a non-null, aligned address that a refused call never touches
I = score_ref.IDX


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from polyffusion_amd.build import build
        build(verbose=False)
    return _lib.load()


def header():
    return open(os.path.join(REPO, "include", "pfhip.h")).read()


# ---------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_and_both_builds_export_the_entry_point(lib):
    hdr = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    declared = set(re.findall(r"\b(pf_[a-z0-9_]+)\s*\(", hdr))
    if not os.path.exists(_lib.lib_path("f16")):
        from polyffusion_amd.build import build
        build(verbose=False, variant="f16")
    assert "pf_roll_stats" in declared and "pf_roll_stats" in _lib.SIGNATURES
    assert hasattr(lib, "pf_roll_stats") and hasattr(_lib.load("f16"), "pf_roll_stats")
    assert _lib.SIGNATURES["pf_roll_stats"] == (C.c_int, [C.POINTER(_lib.RollStatsArgs), C.c_void_p])


def test_struct_and_enum_are_laid_out_as_the_header_says():
    hdr = header()
    body = re.search(r"typedef struct pf_roll_stats_args \{(.*?)\} pf_roll_stats_args;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    order = [n.strip(" *") for decl in re.findall(r"(?:const )?(?:float|int32_t)\s*\*?\s*([^;]+);", body) for n in decl.split(",")]
    f = _lib.RollStatsArgs
    assert order == [n for n, _ in f._fields_] == ["prmat2c", "chord", "mask", "n", "steps", "custom_round", "bass_relative", "counters", "chroma", "onsets"]
    assert {n: getattr(f, n).offset for n in order} == dict(zip(order, [0, 8, 16, 24, 28, 32, 36, 40, 48, 56])) and C.sizeof(f) == 64
    enum = re.findall(r"PF_ROLL_([A-Z_]+) = (\d+)", hdr)
    assert [n for n, _ in enum] == list(_lib.ROLL_COUNTERS) == list(score_ref.NAMES) and [int(v) for _, v in enum] == list(range(14))
    assert int(re.search(r"#define PF_ROLL_NCOUNT (\d+)", hdr).group(1)) == _lib.ROLL_NCOUNT == score_ref.NCOUNT == 16


def test_bad_arguments_are_refused_before_any_launch(lib):
    """No GPU needed: the call returns before it touches HIP or any of the (fake) pointers."""
    def refused(pattern, **fields):
        a = _lib.RollStatsArgs()
        kw = dict(prmat2c=FAKE, chord=FAKE + 0x10000, mask=None, n=2, steps=8, counters=FAKE + 0x20000, chroma=FAKE + 0x30000, onsets=FAKE + 0x40000)
        kw.update(fields)
        for k, v in kw.items():
            setattr(a, k, v)
        rc = lib.pf_roll_stats(C.byref(a), None)
        msg = lib.pf_last_error().decode()
        assert rc < 0 and re.search(pattern, msg), (fields, rc, msg)

    refused("roll_stats: bad arguments", prmat2c=None)
    refused("roll_stats: bad arguments", n=0)
    refused("roll_stats: bad arguments", n=-3)
    refused("roll_stats: bad arguments", steps=0)
    refused("roll_stats: bad arguments", steps=-4)
    for steps in (1, 6, 127):
        refused("not a whole number of beats", steps=steps)
    for out in ("counters", "chroma", "onsets"):
        refused("null output", **{out: None})
        refused("4-byte aligned", **{out: FAKE + 0x50002})
    refused("4-byte aligned", prmat2c=FAKE + 1)
    refused("4-byte aligned", chord=FAKE + 2)
    refused("4-byte aligned", mask=FAKE + 3)
    assert lib.pf_roll_stats(None, None) < 0 and re.search("roll_stats", lib.pf_last_error().decode())


# ---------------------------------------------------------------------------------------------- score_ref on hand-built rolls
MAJOR, MINOR = (0, 4, 7), (0, 3, 7)


def triad_song(n=2, steps=128, seed=3, bass_zero_beats=(), empty_beats=()):
    """A roll made only of each beat's triad: onset on the beat's first step, sustain on the other three, the bass class lowest (octave 3,
    the other two classes an octave above).  Returns (x [n, 2, steps, 128], chord [n, steps / 4, 36]) with absolute bass."""
    rng = np.random.default_rng(seed)
    B = steps // 4
    x, chord = np.zeros((n, 2, steps, 128), np.float32), np.zeros((n, B, 36), np.float32)
    for i in range(n):
        for j in range(B):
            root = int(rng.integers(12))
            classes = [(root + d) % 12 for d in (MAJOR if rng.integers(2) else MINOR)]
            bass = classes[int(rng.integers(3))]
            if j not in empty_beats:
                chord[i, j, root] = 1
                chord[i, j, [12 + k for k in classes]] = 1
                if j not in bass_zero_beats:
                    chord[i, j, 24 + bass] = 1
            keys = [36 + bass] + [48 + k for k in classes if k != bass]
            x[i, 0, 4 * j, keys] = 1
            x[i, 1, 4 * j + 1: 4 * j + 4, keys] = 1
    return x, chord


def shift(chord, s):
    return np.concatenate([np.roll(chord[..., 12 * b: 12 * b + 12], s, axis=-1) for b in range(3)], axis=-1)


def test_a_roll_of_each_beats_triad_fits_its_chords_perfectly():
    x, chord = triad_song()
    c, chroma, onsets = score_ref.roll_stats(x, chord)
    B = 32
    assert (c[:, I["N_ONSET"]] == 3 * B).all() and (c[:, I["N_SOUNDING"]] == 12 * B).all() and (c[:, I["N_ORPHAN"]] == 0).all()
    assert (c[:, I["CHORD_BEATS"]] == B).all() and (c[:, I["CHORD_CLASSES"]] == 3 * B).all() and (c[:, I["CHORD_HEARD"]] == 3 * B).all()
    assert (c[:, I["SOUND_ON_CHORD"]] == 12 * B).all() and (c[:, I["SOUND_IN_CHORD"]] == 12 * B).all()
    assert (c[:, I["ONSET_ON_CHORD"]] == 3 * B).all() and (c[:, I["ONSET_IN_CHORD"]] == 3 * B).all()
    assert (c[:, I["BASS_BEATS"]] == B).all() and (c[:, I["BASS_HIT"]] == B).all()
    assert (c[:, I["LOW_KEY"]] >= 36).all() and (c[:, I["HIGH_KEY"]] <= 59).all() and (c[:, 14:] == 0).all()
    assert (chroma.sum(-1) == 12).all() and ((chroma == 4) == (chord[..., 12:24] > 0.5)).all()
    assert (onsets.reshape(2, B, 4) == np.array([3, 0, 0, 0])).all()
    s = score_ref.scores(c, 128)
    for k in ("chord_fit", "chord_cover", "chord_f1", "bass_fit"):
        assert (s[k] == 1.0).all(), k
    assert (s["integrity"] == 0.0).all() and (s["onset_rate"] == 3 * B / 128).all()


def test_the_same_roll_against_the_chords_a_semitone_up_is_out_of_chord():
    x, chord = triad_song()
    c = score_ref.roll_stats(x, shift(chord, 1))[0]
    # major and minor triads share no class with their semitone transposition ({0,4,7} / {1,5,8}; {0,3,7} / {1,4,8})
    assert (c[:, I["SOUND_IN_CHORD"]] == 0).all() and (c[:, I["ONSET_IN_CHORD"]] == 0).all() and (c[:, I["CHORD_HEARD"]] == 0).all()
    assert (c[:, I["BASS_HIT"]] == 0).all() and (c[:, I["BASS_BEATS"]] == 32).all() and (c[:, I["SOUND_ON_CHORD"]] == 12 * 32).all()
    s = score_ref.scores(c, 128)
    assert (s["chord_f1"] == 0.0).all() and (s["chord_fit"] == 0.0).all() and (s["bass_fit"] == 0.0).all()
    # a relative bass block: the interval from the root, scored with bass_relative, is the same statement
    x, chord = triad_song(n=1)
    root, bass = chord[..., 0:12].argmax(-1), chord[..., 24:36].argmax(-1)
    rel = chord.copy()
    rel[..., 24:36] = np.eye(12, dtype=np.float32)[(bass - root) % 12]
    assert np.array_equal(score_ref.roll_stats(x, rel, bass_relative=True)[0], score_ref.roll_stats(x, chord)[0])
    assert score_ref.roll_stats(x, rel)[0][0, I["BASS_HIT"]] < 32                 # read as absolute it misses wherever the bass is not the root


def test_no_chord_beats_and_a_bass_block_of_zeros():
    x, chord = triad_song(n=1, empty_beats=(0, 5, 31), bass_zero_beats=(1, 2))
    c = score_ref.roll_stats(x, chord)[0][0]
    assert c[I["CHORD_BEATS"]] == 29 and c[I["SOUND_ON_CHORD"]] == 12 * 29 and c[I["SOUND_IN_CHORD"]] == 12 * 29
    assert c[I["CHORD_CLASSES"]] == 3 * 29 and c[I["ONSET_ON_CHORD"]] == 3 * 29
    assert c[I["BASS_BEATS"]] == 27 and c[I["BASS_HIT"]] == 27                   # a beat without a bass entry > 0 is no bass beat
    assert c[I["N_SOUNDING"]] == 12 * 32                                         # the chord-free counters see every beat
    none = score_ref.roll_stats(x, None)[0][0]
    assert (none[3:12] == 0).all() and (none[[0, 1, 2, 12, 13]] == c[[0, 1, 2, 12, 13]]).all()
    allzero = score_ref.roll_stats(x, np.zeros_like(chord))[0][0]
    assert np.array_equal(allzero, none)
    s = score_ref.scores(none[None], 128)
    assert all(float(s[k][0]) == 0.0 for k in ("chord_fit", "chord_cover", "chord_f1", "bass_fit"))      # 0 / 0 is 0.0
    # a tie in the bass block goes to the lowest index; a silent beat is no bass beat
    x1, ch1 = np.zeros((1, 2, 4, 128), np.float32), np.zeros((1, 1, 36), np.float32)
    ch1[0, 0, [12, 16, 19]] = 1
    ch1[0, 0, [24 + 4, 24 + 7]] = 0.5
    assert score_ref.roll_stats(x1, ch1)[0][0, I["BASS_BEATS"]] == 0 and score_ref.roll_stats(x1, ch1)[0][0, I["LOW_KEY"]] == -1
    x1[0, 0, 2, 40] = 1                                                           # key 40: class 4
    got = score_ref.roll_stats(x1, ch1)[0][0]
    assert (got[I["BASS_BEATS"]], got[I["BASS_HIT"]], got[I["LOW_KEY"]], got[I["HIGH_KEY"]]) == (1, 1, 40, 40)
    x1[0, 1, 3, 31] = 1                                                           # a lower key of class 7: the tie still names class 4
    got = score_ref.roll_stats(x1, ch1)[0][0]
    assert (got[I["BASS_BEATS"]], got[I["BASS_HIT"]], got[I["LOW_KEY"]], got[I["N_ORPHAN"]]) == (1, 0, 31, 1)


def test_the_mask_silences_cells_but_not_predecessors():
    x = np.zeros((1, 2, 8, 128), np.float32)
    x[0, 0, 3, 60] = 1
    x[0, 1, 4, 60] = 1                                                            # sustained across the beat boundary: no orphan
    x[0, 1, 6, 10] = 1                                                            # an orphan
    mask = np.zeros_like(x)
    assert score_ref.roll_stats(x)[0][0, :3].tolist() == [1, 3, 1]
    assert np.array_equal(score_ref.roll_stats(x, mask=mask)[0], score_ref.roll_stats(x)[0])
    mask[0, :, 3, 60] = 1                                                         # the onset is kept (not generated): silent, still a predecessor
    assert score_ref.roll_stats(x, mask=mask)[0][0, :3].tolist() == [0, 2, 1]
    x[0, 0, 3, 60] = 0.2                                                          # without the onset below it the sustain is an orphan
    assert score_ref.roll_stats(x, mask=mask)[0][0, :3].tolist() == [0, 2, 2]


@pytest.mark.parametrize("custom", [False, True])
def test_integrity_is_check_prmat2c_integrity(custom):
    from polyffusion_amd.midi import check_prmat2c_integrity
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 2, 32, 128, generator=g) * 0.6 + 0.3
    flat = x.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:1200]
    flat[idx] = torch.tensor([0.5, -0.7, -0.5, 0.95, 1.05, 1.0, 1.0, 1.0])[torch.arange(1200) % 8]
    x[1, 1, 0, :] = 1.0                                                           # an orphan row at step 0
    got = score_ref.integrity(x.numpy(), custom)
    assert got == check_prmat2c_integrity(x, custom) and 0 < got < 1


# ---------------------------------------------------------------------------------------------- the product's host-side arithmetic
def random_counters(n, seed=0):
    rng = np.random.default_rng(seed)
    x = (rng.random((n, 2, 32, 128)) > 0.9).astype(np.float32)
    x[0] = 0
    chord = (rng.random((n, 8, 36)) > 0.6).astype(np.float32)
    chord[1] = 0
    return score_ref.roll_stats(x, chord)


def test_scores_songs_and_texture_fit_equal_the_restatement():
    from polyffusion_amd import score
    c, chroma, onsets = random_counters(12)
    st = score.RollStats(torch.from_numpy(c).int(), torch.from_numpy(chroma).int(), torch.from_numpy(onsets).int())
    for steps, stats, want in ((32, st, c), (96, st.songs(3), score_ref.songs(c, 3))):
        assert np.array_equal(stats.counters.numpy(), want) and stats.steps == steps
        ref = score_ref.scores(want, steps)
        got = stats.scores()
        assert set(got) == set(ref) == set(score.SCORES)
        for k in ref:
            assert got[k].dtype == torch.float64 and np.array_equal(got[k].numpy(), ref[k]), k
    assert st.songs(3).chroma.shape == (4, 24, 12) and np.array_equal(st.songs(3).onsets.numpy(), onsets.reshape(4, 96))
    rep = st.report()
    assert rep[2]["counters"]["N_ONSET"] == c[2, I["N_ONSET"]] and rep[2]["chord_f1"] == score_ref.scores(c, 32)["chord_f1"][2]
    other = score.RollStats(st.counters, st.chroma, torch.from_numpy(np.roll(onsets, 5, axis=0).copy()).int())
    got = score.texture_fit(st, other).numpy()
    assert np.array_equal(got, score_ref.texture_fit(onsets, np.roll(onsets, 5, axis=0))) and got[0] == 0.0
    assert np.allclose(score.texture_fit(st, st).numpy()[1:], 1.0, rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match="whole songs"):
        st.songs(5)


def test_rank_is_stable_and_keeps_the_first():
    from polyffusion_amd import score
    for rank in (score.rank, score_ref.rank):
        assert rank([0.5, 0.9, 0.5, 0.9, 0.1], 3) == [1, 3, 0]
        assert rank([0.5, 0.9, 0.5, 0.9, 0.1], 3, descending=False) == [4, 0, 2]
        assert rank([0.0, 0.0, 0.0], 2) == [0, 1] and rank([0.0, 0.0, 0.0], 2, False) == [0, 1]
        assert rank([1.0, 2.0], 0) == [] and rank([1.0, 2.0], 2) == [1, 0]
    with pytest.raises(ValueError, match="keep"):
        score.rank([1.0], 2)
    assert score.RANK_BY["integrity"] == ("integrity", False) and score.RANK_BY["chord"] == ("chord_f1", True)


# ---------------------------------------------------------------------------------------------- the CLI
def test_parser_defaults_and_refusals_come_before_any_weight_is_loaded(tmp_path):
    from polyffusion_amd import inference_sdf
    p = inference_sdf.make_parser()
    a = p.parse_args([])
    assert (a.score, a.best_of, a.rank_by, a.score_bass_relative) == (False, 1, "chord", False)
    assert inference_sdf.check_score_args(a, "chord") is False
    assert inference_sdf.check_score_args(p.parse_args(["--score"]), "txt") is True
    assert inference_sdf.check_score_args(p.parse_args(["--best_of", "3"]), "chord") is True
    assert inference_sdf.check_score_args(p.parse_args(["--best_of", "3", "--rank_by", "texture"]), "chord+txt") is True
    assert inference_sdf.check_score_args(p.parse_args(["--best_of", "2", "--rank_by", "integrity"]), "txt") is True

    def refused(pattern, argv, cond_type=None):
        with pytest.raises(SystemExit, match=pattern):
            inference_sdf.check_score_args(p.parse_args(argv), cond_type)

    refused("--edit is deterministic", ["--best_of", "2", "--edit"])
    refused("--best_of 0", ["--best_of", "0"])
    for ct in ("chord", "txt", "pnotree"):
        refused("--rank_by texture", ["--best_of", "2", "--rank_by", "texture"], ct)
        refused("--rank_by texture", ["--score", "--rank_by", "texture"], ct)
    refused("needs the chords", ["--best_of", "2"], "txt")
    refused("needs the chords", ["--best_of", "2", "--rank_by", "bass"], "pnotree")
    refused("belong to --score", ["--score_bass_relative"])
    refused("belong to --score", ["--rank_by", "bass"])
    with pytest.raises(SystemExit):
        p.parse_args(["--rank_by", "key"])
    # through main(): refused before the GPU, the parameters or the weights are looked at
    with pytest.raises(SystemExit, match="--edit is deterministic"):
        np.savez(tmp_path / "song.npz", chord=np.zeros((1, 32, 36), np.float32), prmat2c=np.zeros((1, 2, 128, 128), np.float32))
        inference_sdf.main(["--best_of", "2", "--edit", "--ddim", "--edit_chord_shift", "2", "--cond_npz", str(tmp_path / "song.npz"),
                            "--params_preset", "sdf_chd8bar", "--synthetic_weights"])
    # generate_songs counts candidates as songs: the same shards as that many plain generations
    from polyffusion_amd import dist as pfdist
    assert [pfdist.shard_range(2 * 3, r, 4) for r in range(4)] == [pfdist.shard_range(6, r, 4) for r in range(4)]
