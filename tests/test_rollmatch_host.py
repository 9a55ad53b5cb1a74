"""Roll matching without a GPU (-m "not gpu"): the numpy restatement (tests/rollmatch_ref.py) on planted cases, its second formulation on
128-bit integers against the first, the C ABI of pf_roll_pack / pf_roll_match (declared, exported by both builds, laid out as the header
says, every misuse refused before any launch), the ``Corpus`` (windows, where(), save / load, version refusal, from_dataset), the
exclusion rule of ``pairwise``, the ranking key and the CLI's refusals and defaults."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dataset_fixture
import rollmatch_ref as ref
from polyffusion_amd import _lib, rollmatch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000         # a non-null, 16-byte aligned address that a refused call never touches
SEAM = (0, 31, 32, 63, 64, 95, 96, 127)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from polyffusion_amd.build import build
        build(verbose=False)
    return _lib.load()


def header():
    return open(os.path.join(REPO, "include", "pfhip.h")).read()


def window(cells, steps=4):
    """A boolean window [steps, 128] with notes at (step, key) pairs"""
    w = np.zeros((steps, 128), bool)
    for t, k in cells:
        w[t, k] = True
    return w


def transposed(w, s):
    out = np.zeros_like(w)
    for j in range(128):
        if 0 <= j + s < 128:
            out[:, j + s] = w[:, j]
    return out


# ---------------------------------------------------------------------------------------------- the restatement on planted cases
def test_shift_order_and_thresholds():
    assert [ref.shift_of(k) for k in range(7)] == [0, -1, 1, -2, 2, -3, 3]
    v = np.array([0.5, 0.51, 0.95, 0.96, 1.0, 1.05, np.nan, np.inf, -np.inf, -0.6], np.float32)
    assert ref.round_(v).tolist() == [False, True, True, True, True, True, False, True, False, False]
    assert ref.round_(v, True).tolist() == [False, False, False, True, True, False, False, False, False, False]
    x = np.zeros((1, 2, 2, 128), np.float32)
    x[0, 0, 0, 3], x[0, 1, 0, 40], x[0, 1, 1, 127], x[0, 0, 1, 127] = 1.0, 1.0, 0.7, np.nan
    on, snd = ref.planes(x)
    assert np.argwhere(on).tolist() == [[0, 3]] and np.argwhere(snd).tolist() == [[0, 3], [0, 40], [1, 127]]     # sounding = onset | sustain
    bits = ref.pack(x)
    assert bits.shape == (2, 2, 4) and bits[0, 0].tolist() == [8, 0, 0, 0] and bits[1, 0].tolist() == [8, 256, 0, 0]
    assert bits[1, 1].tolist() == [0, 0, 0, 1 << 31] and not bits[0, 1].any()
    assert np.array_equal(rollmatch.pack_host(x), bits) and np.array_equal(rollmatch.pack_host(x, True), ref.pack(x, True))


def test_planted_cases():
    base = window([(0, 40), (0, 44), (1, 47), (2, 52), (3, 40), (3, 64)])
    other = window([(0, 10), (1, 90), (2, 100)])
    corpus = np.stack([other, base, base])                       # window 2 duplicates window 1
    # an identical window: J = 1 at s = 0, and the duplicate goes to the lower index
    m = ref.match(base[None], corpus, 3, 3)
    assert (m["index"][0].tolist(), m["shift"][0].tolist()) == ([1, 2, 0], [0, 0, 0])
    assert m["inter"][0].tolist() == [6, 6, 0] and m["union"][0].tolist() == [6, 6, 9]
    # the corpus window transposed up by 3, nothing leaving the keyboard: J = 1 at s = 3
    m = ref.match(transposed(base, 3)[None], corpus, 3, 1)
    assert (m["index"][0, 0], m["shift"][0, 0], m["inter"][0, 0], m["union"][0, 0]) == (1, 3, 6, 6)
    m = ref.match(transposed(base, -2)[None], corpus, 3, 1)
    assert (m["index"][0, 0], m["shift"][0, 0], m["inter"][0, 0]) == (1, -2, 6)
    assert ref.match(transposed(base, 3)[None], corpus, 2, 1)["inter"][0, 0] < 6                     # out of reach with S = 2
    # a transposition that pushes notes off either end: the query's lost notes are dropped from |qs|, the window keeps all of its own
    edge = window([(0, 0), (0, 1), (1, 64), (2, 126), (2, 127)])
    up = transposed(edge, 2)                                     # keys 126, 127 left the keyboard: 3 notes remain
    m = ref.match(up[None], edge[None], 2, 1)
    assert up.sum() == 3 and (m["shift"][0, 0], m["inter"][0, 0], m["union"][0, 0]) == (2, 3, 5)
    down = transposed(edge, -1)                                  # key 0 left
    m = ref.match(down[None], edge[None], 2, 1)
    assert down.sum() == 4 and (m["shift"][0, 0], m["inter"][0, 0], m["union"][0, 0]) == (-1, 4, 5)
    # the query's own notes leave when shifted: q at key 127 against a window at key 126 needs s = +1 (qs[j] = q[j + 1])
    m = ref.match(window([(0, 127), (1, 127)])[None], window([(0, 126)])[None], 1, 1)
    assert (m["shift"][0, 0], m["inter"][0, 0], m["union"][0, 0]) == (1, 1, 2)
    # disjoint rolls: 0, and the tie of all shifts goes to k = 0
    m = ref.match(window([(0, 5)])[None], window([(3, 100)])[None], 4, 1)
    assert (m["shift"][0, 0], m["inter"][0, 0], m["union"][0, 0]) == (0, 0, 2)
    # an empty query and an empty window count as 0 / 1: ties to k = 0 and the lowest b; slots beyond nb are -1, 0, 0, 0
    empty = window([])
    m = ref.match(empty[None], np.stack([base, empty, other]), 2, 8)
    assert m["index"][0].tolist() == [0, 1, 2, -1, -1, -1, -1, -1] and not m["shift"].any() and not m["inter"].any()
    assert m["union"][0].tolist() == [6, 0, 3, 0, 0, 0, 0, 0] and m["tab_union"][0].tolist() == [6, 0, 3]
    m = ref.match(base[None], np.stack([empty, other, empty]), 0, 2)
    assert m["index"][0].tolist() == [0, 1] and m["union"][0].tolist() == [6, 9]
    # exact ordering: 2 / 3 beats 3 / 5 although float32 would still tell them apart; 1 / 3 ties 2 / 6
    assert ref.better(2, 3, 3, 5) and not ref.better(3, 5, 2, 3) and not ref.better(1, 3, 2, 6) and not ref.better(2, 6, 1, 3)
    assert not ref.better(0, 0, 0, 5) and not ref.better(0, 5, 0, 0) and ref.better(1, 100, 0, 0)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_integer_formulation_equals_the_boolean_one(seed):
    rng = np.random.default_rng(seed)
    steps, na, nb, S, topk = (3, 4, 9, 15, 4) if seed else (2, 3, 5, 6, 8)
    q, c = rng.random((na, steps, 128)) < 0.15, rng.random((nb, steps, 128)) < 0.15
    q[:, :, SEAM] |= rng.random((na, steps, len(SEAM))) < 0.5    # notes on the word seams
    c[:, :, SEAM] |= rng.random((nb, steps, len(SEAM))) < 0.5
    q[1], c[2] = transposed(c[0], 1 + seed), c[1]                # a transposed copy and a duplicate
    q[2] = False
    a, b = ref.match(q, c, S, topk), ref.match_ints(q, c, S, topk)
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert (a["tab_shift"] != 0).any() and (a["tab_inter"] > 0).any()


# ---------------------------------------------------------------------------------------------- the C ABI
SYMBOLS = ("pf_roll_pack", "pf_roll_match", "pf_roll_match_workspace_bytes")


def test_header_declares_and_both_builds_export_the_entry_points(lib):
    hdr = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    declared = set(re.findall(r"\b(pf_[a-z0-9_]+)\s*\(", hdr))
    if not os.path.exists(_lib.lib_path("f16")):
        from polyffusion_amd.build import build
        build(verbose=False, variant="f16")
    for name in SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES, name
        assert hasattr(lib, name) and hasattr(_lib.load("f16"), name), name
    assert _lib.SIGNATURES["pf_roll_match"] == (C.c_int, [C.POINTER(_lib.RollMatchArgs), C.c_void_p])
    assert _lib.SIGNATURES["pf_roll_match_workspace_bytes"][0] is C.c_size_t


def test_struct_and_constants_are_laid_out_as_the_header_says(lib):
    hdr = header()
    body = re.search(r"typedef struct pf_roll_match_args \{(.*?)\} pf_roll_match_args;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    order = [n.strip(" *") for decl in re.findall(r"(?:const )?(?:uint32_t|int32_t|void|size_t)\s*\*?\s*([^;]+);", body) for n in decl.split(",")]
    f = _lib.RollMatchArgs
    assert order == [n for n, _ in f._fields_] == ["a_bits", "a_starts", "b_bits", "b_starts", "na", "nb", "steps", "shifts", "topk", "reserved",
                                                   "top_index", "top_shift", "top_inter", "top_union", "tab_inter", "tab_union", "tab_shift",
                                                   "workspace", "workspace_bytes"]
    offsets = [0, 8, 16, 24, 32, 36, 40, 44, 48, 52, 56, 64, 72, 80, 88, 96, 104, 112, 120]
    assert {n: getattr(f, n).offset for n in order} == dict(zip(order, offsets)) and C.sizeof(f) == 128
    define = lambda name: int(re.search(rf"#define {name} (\d+)", hdr).group(1))
    assert define("PF_ROLL_MATCH_CHUNK") == _lib.ROLL_MATCH_CHUNK
    assert define("PF_ROLL_MATCH_MAX_SHIFTS") == _lib.ROLL_MATCH_MAX_SHIFTS == 15
    assert define("PF_ROLL_MATCH_MAX_TOPK") == _lib.ROLL_MATCH_MAX_TOPK == 8
    # the workspace: a per-chunk list per query plus the |qs| table; 0 for arguments the call would refuse
    ws = lib.pf_roll_match_workspace_bytes
    chunk = _lib.ROLL_MATCH_CHUNK
    assert ws(1, 1, 1) > 0 and ws(3, chunk, 8) == ws(3, 1, 8) < ws(3, chunk + 1, 8)
    assert ws(3, chunk + 1, 8) - ws(3, chunk, 8) == 3 * 8 * 16 and ws(2, 5, 3) % 16 == 0
    assert [ws(0, 1, 1), ws(1, 0, 1), ws(1, 1, 0), ws(1, 1, 9), ws(-1, 1, 1)] == [0] * 5
    assert ws(16, 2 ** 31 - 1, 8) > 2 ** 32                                                             # formed in 64 bits


def test_bad_arguments_are_refused_before_any_launch(lib):
    """No GPU needed: the calls return before they touch HIP or any of the (fake) pointers."""
    inputs, tops, tabs = ("a_bits", "a_starts", "b_bits", "b_starts"), ("top_index", "top_shift", "top_inter", "top_union"), ("tab_inter", "tab_union", "tab_shift")
    pointers = inputs + tops + tabs + ("workspace",)

    def refused(pattern, **fields):
        a = _lib.RollMatchArgs()
        kw = dict({n: FAKE + 0x10000 * i for i, n in enumerate(pointers)}, na=2, nb=300, steps=128, shifts=6, topk=3, reserved=0,
                  workspace_bytes=1 << 20)
        kw.update(fields)
        for k, v in kw.items():
            setattr(a, k, v)
        rc = lib.pf_roll_match(C.byref(a), None)
        msg = lib.pf_last_error().decode()
        assert rc < 0 and re.search(pattern, msg), (fields, rc, msg)

    for name in inputs:
        refused(f"roll_match: null input.*{name}", **{name: None})
    for name in ("na", "nb", "steps"):
        refused(f"roll_match: bad shape.*{name} = 0", **{name: 0})
        refused(f"roll_match: bad shape.*{name} = -3", **{name: -3})
    for v in (-1, 16):
        refused(f"shifts = {v} outside 0..15", shifts=v)
    for v in (0, 9, -2):
        refused(f"topk = {v} outside 1..8", topk=v)
    refused("reserved = 1 must be 0", reserved=1)
    for name in tops:
        refused(f"roll_match: null output.*{name}", **{name: None})
    for missing in [("tab_inter",), ("tab_union",), ("tab_shift",), ("tab_inter", "tab_union"), ("tab_union", "tab_shift"), ("tab_inter", "tab_shift")]:
        refused("dense tables go together", **{n: None for n in missing})
    refused("null workspace", workspace=None)
    refused("workspace of 64 bytes, \\d+ needed", workspace_bytes=64)
    for name in pointers:
        refused("aligned", **{name: FAKE + 0x200002})
    for name in ("a_bits", "b_bits", "workspace"):
        refused("16-byte aligned", **{name: FAKE + 0x200004})
    assert lib.pf_roll_match(None, None) < 0 and re.search("pf_roll_match: null arguments", lib.pf_last_error().decode())

    def pack_refused(pattern, x=FAKE, n=1, steps=4, bits=FAKE * 2):
        rc = lib.pf_roll_pack(x, n, steps, 0, bits, None)
        assert rc < 0 and re.search(pattern, lib.pf_last_error().decode()), (pattern, rc, lib.pf_last_error().decode())

    pack_refused("roll_pack: null pointer", x=None)
    pack_refused("roll_pack: null pointer", bits=None)
    pack_refused("roll_pack: bad shape.*n = 0", n=0)
    pack_refused("roll_pack: bad shape.*steps = -1", steps=-1)
    pack_refused("4-byte aligned", x=FAKE + 2)
    pack_refused("4-byte aligned", bits=FAKE + 1)


# ---------------------------------------------------------------------------------------------- the corpus
def hand_made_songs():
    rng = np.random.default_rng(4)
    a = (rng.random((2, 2, 128, 128)) < 0.03).astype(np.float32)          # 256 rows
    b = (rng.random((1, 2, 128, 128)) < 0.03).astype(np.float32)          # 128 rows: exactly one window
    short = (rng.random((1, 2, 40, 128)) < 0.03).astype(np.float32)       # 40 rows: zero-padded to one window
    return [a, b, short], ["a.npz", "b.npz", "short.npz"]


def test_corpus_windows_where_and_round_trip(tmp_path):
    songs, names = hand_made_songs()
    c = rollmatch.Corpus.from_songs(songs, names, steps=128, hop=16)
    assert c.bits.shape == (2, 256 + 128 + 128, 4) and c.bits.dtype == np.uint32
    assert c.starts.tolist() == list(range(0, 129, 16)) + [256, 384]          # none spans two songs
    assert c.song_of_window.tolist() == [0] * 9 + [1, 2] and c.row_in_song.tolist() == list(range(0, 129, 16)) + [0, 0]
    assert [c.where(i) for i in (0, 3, 8, 9, 10)] == [("a.npz", 0), ("a.npz", 3), ("a.npz", 8), ("b.npz", 0), ("short.npz", 0)] and c.where(-1) is None
    assert np.array_equal(c.bits[:, :256], ref.pack(songs[0])) and np.array_equal(c.bits[:, 384:424], ref.pack(songs[2])) and not c.bits[:, 424:].any()
    one = rollmatch.Corpus.from_songs(songs, names, hop=1)
    assert len(one) == 129 + 1 + 1 and one.where(5) == ("a.npz", 0) and one.where(16) == ("a.npz", 1) and one.where(129) == ("b.npz", 0)
    assert np.array_equal(one.bits, c.bits)
    custom = rollmatch.Corpus.from_songs([s * 0.7 for s in songs], names, custom_round=True)                 # 0.7 is a note by the default rule only
    assert not custom.bits.any() and custom.custom_round
    c.save(str(tmp_path / "corpus.npz"))
    back = rollmatch.Corpus.load(str(tmp_path / "corpus.npz"))
    for k in ("bits", "starts", "song_of_window", "row_in_song"):
        assert np.array_equal(getattr(back, k), getattr(c, k)) and getattr(back, k).dtype == getattr(c, k).dtype, k
    assert (back.names, back.steps, back.hop, back.custom_round) == (names, 128, 16, False)
    with np.load(str(tmp_path / "corpus.npz")) as z:
        assert sorted(z.files) == sorted(["bits", "starts", "song_of_window", "row_in_song", "names", "steps", "hop", "custom_round", "version"])
        fields = {k: z[k] for k in z.files}
    fields["version"] = np.int32(rollmatch.FORMAT_VERSION + 1)
    np.savez(str(tmp_path / "future.npz"), **fields)
    with pytest.raises(ValueError, match="format version 2"):
        rollmatch.Corpus.load(str(tmp_path / "future.npz"))
    del fields["version"]
    np.savez(str(tmp_path / "old.npz"), **fields)
    with pytest.raises(ValueError, match="format version None"):
        rollmatch.Corpus.load(str(tmp_path / "old.npz"))
    with pytest.raises(ValueError, match="songs"):
        rollmatch.Corpus.from_songs(songs, names[:2])
    with pytest.raises(ValueError, match="leaves the stored rows"):
        rollmatch.Corpus(c.bits, c.starts + 400, c.song_of_window, c.row_in_song, names, 128, 16, False)


def test_corpus_from_dataset_and_the_build_command(tmp_path, capsys):
    from polyffusion_amd import datasample
    pop, mus, split = (str(tmp_path / d) for d in ("pop", "mus", "split"))
    dataset_fixture.write_all(pop, mus, split)
    c = rollmatch.Corpus.from_dataset("pop909", "val", pop, split)
    files = [fn for fn, v in dataset_fixture.SONGS.items() if v[0] == "pop909"]
    want = [datasample.DataSampleNpz(fn, (0, 1, 2), pop).get_whole_song_data()[0].numpy() for fn in files]
    assert c.names == files and c.steps == 128 and c.hop == 16
    assert np.array_equal(c.bits, np.concatenate([ref.pack(w) for w in want], axis=1))
    assert len(c) == sum((w.shape[0] * 128 - 128) // 16 + 1 for w in want)
    m = rollmatch.Corpus.from_dataset("musicalion", "val", mus, split, hop=128)
    assert m.names == ["mus_a.npz"] and len(m) == m.bits.shape[1] // 128
    with pytest.raises(FileNotFoundError):
        rollmatch.Corpus.from_dataset("pop909", "train", pop, split)                                         # the fixture's train half names no file
    with pytest.raises(ValueError, match="part"):
        rollmatch.Corpus.from_dataset("pop909", "test", pop, split)
    out = str(tmp_path / "c.npz")
    assert rollmatch.main(["build", "--from_dataset", "pop909", "--part", "val", "--dataset_dir", pop, "--split_dir", split, "--out", out]) == 0
    assert '"windows": %d' % len(c) in capsys.readouterr().out
    assert np.array_equal(rollmatch.Corpus.load(out).bits, c.bits)
    np.save(str(tmp_path / "song.npy"), want[0])
    assert rollmatch.main(["build", "--from_npy", str(tmp_path / "song.npy"), "--out", out, "--hop", "64", "--custom_round"]) == 0
    back = rollmatch.Corpus.load(out)
    assert (back.hop, back.custom_round, back.names) == (64, True, [str(tmp_path / "song.npy")])
    with pytest.raises(SystemExit, match="exactly one of"):
        rollmatch.main(["build", "--out", out])
    with pytest.raises(SystemExit, match="exactly one of"):
        rollmatch.main(["build", "--from_npy", "x.npy", "--from_midi", "y.mid", "--out", out])
    with pytest.raises(SystemExit, match="--hop 0"):
        rollmatch.main(["build", "--from_npy", str(tmp_path / "song.npy"), "--out", out, "--hop", "0"])


# ---------------------------------------------------------------------------------------------- results on the host
def test_pairwise_exclusion_and_diversity_on_hand_made_tables():
    j = np.array([[1.0, 0.9, 0.2, 0.1],
                  [0.9, 1.0, 0.3, 0.0],
                  [0.2, 0.3, 1.0, 0.8],
                  [0.4, 0.0, 0.8, 1.0]])
    assert rollmatch.nearest_other_of(j, 1).tolist() == [0.9, 0.9, 0.8, 0.8]                                 # the diagonal is excluded
    other = rollmatch.nearest_other_of(j, 2)                                                                 # songs of two images: their own images too
    assert other.tolist() == [0.3, 0.4] and rollmatch.diversity_of(other) == 1.0 - 0.35
    assert rollmatch.nearest_other_of(j, 4).tolist() == [0.0] and rollmatch.diversity_of(np.zeros(1)) == 1.0
    with pytest.raises(ValueError, match="whole songs"):
        rollmatch.nearest_other_of(j, 3)


def test_songs_report_and_windows_need_no_gpu():
    import torch
    songs, names = hand_made_songs()
    c = rollmatch.Corpus.from_songs(songs, names)
    rep = rollmatch.songs_report(torch.tensor([1.0, 0.25, 0.0]), torch.tensor([[9, 0, 0], [3, -2, 1], [-1, 0, 0]], dtype=torch.int32), c)
    assert rep[0] == dict(copy_score=1.0, nearest=dict(song="b.npz", bar=0, shift=0, image=0, window=9))
    assert rep[1] == dict(copy_score=0.25, nearest=dict(song="a.npz", bar=3, shift=-2, image=1, window=3)) and rep[2]["nearest"] is None
    p = rollmatch.PackedRolls(torch.zeros(2, 6 * 64, 4, dtype=torch.int32), 6, 64)
    assert p.windows().tolist() == [0, 64, 128, 192, 256, 320] and p.windows(128, 128).tolist() == [0, 128, 256]
    assert p.windows(128, 16).tolist() == list(range(0, 257, 16))
    m = rollmatch.MatchResult(*(torch.tensor(v, dtype=torch.int32) for v in ([[9, 3], [1, -1]], [[0, -2], [1, 0]], [[6, 1], [0, 0]], [[6, 4], [0, 0]])), c)
    assert m.jaccard.tolist() == [[1.0, 0.25], [0.0, 0.0]] and m.jaccard.dtype == torch.float64                # 0 where the union is 0
    assert m.where() == [[("b.npz", 0), ("a.npz", 3)], [("a.npz", 1), None]]
    assert m.songs(2) == [dict(copy_score=1.0, nearest=dict(song="b.npz", bar=0, shift=0, image=0, window=9))]
    assert [len(r) for r in m.report()] == [2, 1] and m.report()[0][1] == dict(jaccard=0.25, inter=1, union=4, shift=-2, window=3, song="a.npz", bar=3)
    with pytest.raises(ValueError, match="plane"):
        rollmatch.nearest(None, c, plane="pitch")


# ---------------------------------------------------------------------------------------------- the CLI
def test_parser_defaults_rank_key_and_refusals(tmp_path):
    from polyffusion_amd import inference_sdf, score
    p = inference_sdf.make_parser()
    a = p.parse_args([])
    assert (a.novelty_corpus, a.novelty_shifts, a.novelty_topk, a.novelty_plane, a.diversity) == (None, 6, 3, "onset", False)
    assert score.RANK_BY["novelty"] == ("copy_score", False) and "copy_score" not in score.SCORES
    assert score.rank([0.5, 0.1, 1.0, 0.1], 2, descending=False) == [1, 3]                                   # the least copied first, ties to the earlier
    assert inference_sdf.check_score_args(p.parse_args([])) is False                                         # nothing changes without the flags
    assert inference_sdf.check_score_args(p.parse_args(["--score", "--novelty_corpus", "c.npz", "--diversity"]), "chord") is True
    assert inference_sdf.check_score_args(p.parse_args(["--best_of", "2", "--rank_by", "novelty", "--novelty_corpus", "c.npz"]), "txt") is True
    assert inference_sdf.check_score_args(p.parse_args(["--score", "--diversity", "--novelty_plane", "sounding"])) is True
    assert inference_sdf.check_score_args(p.parse_args(["--edit", "--score", "--novelty_corpus", "c.npz"])) is True
    assert inference_sdf.check_score_args(p.parse_args(["--morph", "--score", "--novelty_corpus", "c.npz", "--diversity"])) is True

    def refused(pattern, argv):
        with pytest.raises(SystemExit, match=pattern):
            inference_sdf.check_score_args(p.parse_args(argv))

    refused("--novelty_corpus: these belong to --score", ["--novelty_corpus", "c.npz"])
    refused("--diversity: these belong to --score", ["--diversity"])
    refused("--novelty_shifts, --novelty_topk: these belong to --score", ["--novelty_shifts", "2", "--novelty_topk", "1"])
    refused("belong to --score", ["--novelty_plane", "sounding"])
    refused("--rank_by novelty ranks by copy_score, which needs --novelty_corpus", ["--best_of", "2", "--rank_by", "novelty"])
    refused("--novelty_shifts: these belong to --novelty_corpus", ["--score", "--novelty_shifts", "2"])
    refused("--novelty_shifts 16: 0..15", ["--score", "--novelty_corpus", "c.npz", "--novelty_shifts", "16"])
    refused("--novelty_topk 0: 1..8", ["--score", "--novelty_corpus", "c.npz", "--novelty_topk", "0"])
    with pytest.raises(SystemExit):
        p.parse_args(["--novelty_plane", "pitch"])
    # a corpus the run cannot be compared with
    songs, names = hand_made_songs()
    load = lambda path: inference_sdf.load_novelty_corpus(p.parse_args(["--score", "--novelty_corpus", str(path)]))
    assert inference_sdf.load_novelty_corpus(p.parse_args(["--score"])) is None
    rollmatch.Corpus.from_songs(songs, names).save(str(tmp_path / "good.npz"))
    assert len(load(tmp_path / "good.npz")) == 11
    rollmatch.Corpus.from_songs(songs, names, steps=64).save(str(tmp_path / "steps64.npz"))
    with pytest.raises(SystemExit, match="windows of 64 steps"):
        load(tmp_path / "steps64.npz")
    rollmatch.Corpus.from_songs(songs, names, custom_round=True).save(str(tmp_path / "custom.npz"))
    with pytest.raises(SystemExit, match="built with --custom_round"):
        load(tmp_path / "custom.npz")
    with pytest.raises(SystemExit, match="--novelty_corpus"):
        load(tmp_path / "missing.npz")
    line = inference_sdf.novelty_text(dict(copy_score=0.5, nearest=dict(song="a.npz", bar=3, shift=-2, image=0, window=3)))
    assert line == "copy_score 0.5000 (nearest a.npz bar 3 shift -2)"
    # the stand-alone scorer
    np.save(tmp_path / "roll.npy", np.zeros((1, 2, 128, 128), np.float32))
    with pytest.raises(SystemExit, match="belong to --novelty_corpus"):
        score.main(["--npy", str(tmp_path / "roll.npy"), "--novelty_shifts", "2"])
    with pytest.raises(SystemExit, match="--novelty_topk 1..8"):
        score.main(["--npy", str(tmp_path / "roll.npy"), "--novelty_corpus", "c.npz", "--novelty_topk", "9"])
