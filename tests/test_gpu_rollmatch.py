"""Roll packing and matching on the GPU (-m gpu): ``pf_roll_pack`` and ``pf_roll_match`` must equal the numpy restatement in
``tests/rollmatch_ref.py`` EXACTLY - every packed word, every index, shift, intersection and union of the top-k lists and of the dense
tables.  All values are integers, so no tolerance exists.  Shapes are the smallest at which the kernels can go wrong: one row, rows that
do not fill a workgroup, an odd row count (the scan takes two rows at a time), corpora of one window, fewer windows than ``topk``, one
below / at / one above a multiple of the corpus chunk, several chunks, more queries than a workgroup takes, every shift range, both
planes, overlapping windows in a non-monotone order.  Then ``rollmatch.nearest`` / ``pairwise`` on the device and ``inference_sdf
--novelty_corpus --diversity --rank_by novelty`` (plain generation, ``--edit``, ``--morph``, ``--autoreg``) and ``polyffusion_amd.score
--novelty_corpus`` end to end against the restatement on the files the runs write."""
import ctypes as C
import glob
import json
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rollmatch_ref as ref  # noqa: E402
from polyffusion_amd import _lib  # noqa: E402

PAD = 16                              # int32 words of sentinel on either side of a buffer
SENTINEL, GARBAGE = -1234567, 0x5A5A5A5
SPECIAL = np.array([0.5, -0.5, -0.6, 0.95, 1.05, np.nan, np.inf, -np.inf, 1.0, 0.96, 0.51, -0.51], np.float32)   # as tests/test_gpu_score.py
SEAM = (0, 31, 32, 63, 64, 95, 96, 127)
CHUNK = _lib.ROLL_MATCH_CHUNK
PACK_SHAPES = [(1, 1), (1, 4), (3, 128), (17, 12)]
#            steps, na,  nb,           S, topk, plane
MATCH_CASES = [(1, 1, 1, 0, 1, 0),
               (4, 3, 2, 1, 3, 1),
               (4, 17, CHUNK - 1, 15, 8, 0),
               (4, 3, CHUNK, 12, 3, 0),
               (4, 17, CHUNK + 1, 1, 8, 1),
               (1, 17, 2 * CHUNK + 1, 15, 8, 0),
               (4, 3, 4100, 1, 3, 0),
               (128, 3, 7, 12, 8, 0),
               (128, 17, 40, 1, 3, 1),
               (130, 1, 2, 15, 1, 0),
               (130, 3, CHUNK + 44, 0, 3, 1)]
OUTS = ("index", "shift", "inter", "union")
TABS = ("tab_inter", "tab_union", "tab_shift")


@pytest.fixture(scope="module")
def lib():
    _lib.require_gpu()
    return _lib.load()


def guarded(shape):
    """(whole buffer, payload view): an int32 buffer pre-filled with garbage between two runs of sentinels."""
    size = int(np.prod(shape))
    whole = torch.full((size + 2 * PAD,), SENTINEL, device="cuda", dtype=torch.int32)
    whole[PAD: PAD + size] = GARBAGE
    return whole, whole[PAD: PAD + size].view(*shape)


def untouched(whole):
    return bool((whole[:PAD] == SENTINEL).all()) and bool((whole[-PAD:] == SENTINEL).all())


def dev_bits(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int32)).cuda()


# ---------------------------------------------------------------------------------------------- pf_roll_pack
def make_images(n, steps, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, 2, steps, 128)) * 0.6 + 0.3).astype(np.float32)
    flat = x.reshape(-1)
    where = rng.choice(flat.size, size=max(flat.size // 6, 24), replace=False)
    flat[where] = SPECIAL[rng.integers(len(SPECIAL), size=where.size)]
    for k, key in enumerate(SEAM):                               # every special value on every seam key of both channels
        for j, v in enumerate(SPECIAL):
            x[(j + k) % n, j % 2, (3 * j + k) % steps, key] = v
            x[(j + k + 1) % n, (j + 1) % 2, (5 * j + k) % steps, key] = v
    if n >= 3:
        x[1] = 0.0                                               # a silent image
        x[2] = 1.0                                               # a full one (in both rounding modes)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("custom_round", [False, True])
@pytest.mark.parametrize("shape", PACK_SHAPES, ids=lambda s: "n%d-steps%d" % s)
def test_pack_writes_the_words_of_the_restatement(lib, shape, custom_round):
    from polyffusion_amd import rollmatch
    n, steps = shape
    x = make_images(n, steps, 3 + n)
    want = ref.pack(x, custom_round)
    assert want.shape == (2, n * steps, 4)
    if n >= 3:
        assert not want[:, steps:2 * steps].any() and (want[:, 2 * steps:3 * steps] == 0xFFFFFFFF).all()
    whole, bits = guarded((2, n * steps, 4))
    xd = torch.from_numpy(np.array(x)).cuda()
    _lib.check(lib.pf_roll_pack(xd.data_ptr(), n, steps, int(custom_round), bits.data_ptr(), _lib.current_stream()), "pf_roll_pack", lib)
    got = bits.cpu().numpy().view(np.uint32)
    assert untouched(whole)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (bad[:8].tolist(), hex(got[tuple(bad[0])]), hex(want[tuple(bad[0])]))
    assert np.array_equal(rollmatch.pack_host(x, custom_round), want)             # the corpus builder's host packing is the same words
    p = rollmatch.pack_rolls(xd.reshape(1, n, 2, steps, 128), custom_round)
    assert (p.images, p.steps) == (n, steps) and np.array_equal(p.bits.cpu().numpy().view(np.uint32), want)


# ---------------------------------------------------------------------------------------------- pf_roll_match
def make_match_case(steps, na, nb, S, topk, plane, seed):
    """Float images of one corpus song (windows at every row, visited in a shuffled order) and of ``na`` query windows (in reverse order)
    with planted relations; returns (xq, a_starts, xc, b_starts), read-only."""
    rng = np.random.default_rng(seed)
    dens = 0.2 if steps <= 4 else 0.03
    R = nb + steps - 1
    c = rng.random((R, 128)) < dens
    c[:, SEAM] |= rng.random((R, len(SEAM))) < 0.3
    if nb >= 3:
        c[1:1 + steps] = False                                   # an empty window (start 1)
    if nb > 3 * steps + 8:
        d = 2 * steps + 3
        c[d + steps + 1: d + 2 * steps + 1] = c[d: d + steps]    # window d + steps + 1 duplicates window d
    q = rng.random((na * steps, 128)) < dens
    clear = nb > 4 * steps + 5                                   # room beyond the rows the empty and the duplicated window own
    kinds = [i % 4 if i < 8 else 1 for i in range(na)]           # 0 random, 1 exact transposed copy, 2 noisy copy, 3 empty
    sources = [int(rng.integers(4 * steps + 5, nb)) if clear else int(rng.integers(nb)) for _ in range(na)]
    for kind, b in zip(kinds, sources):                          # first every change to the corpus, then the copies
        if kind == 1 and clear:
            c[b:b + steps, :16], c[b:b + steps, 112:] = False, False     # nothing leaves the keyboard: the copy is exact
    for i, (kind, b) in enumerate(zip(kinds, sources)):
        rows = slice(i * steps, (i + 1) * steps)
        if kind == 1 or kind == 2:                               # corpus window b transposed up by s: q[t][j + s] = c[t][j]
            s = ref.shift_of(i % (2 * S + 1)) if kind == 1 else (S if i % 8 == 2 else -S)
            src, dst = c[b:b + steps], np.zeros((steps, 128), bool)
            for j in range(128):
                if 0 <= j + s < 128:
                    dst[:, j + s] = src[:, j]
            if kind == 2:                                        # a noisy copy: 0.3 % of the cells flipped
                dst ^= rng.random(dst.shape) < 0.003
            q[rows] = dst
        elif kind == 3:
            q[rows] = False                                      # an empty query
    plan = list(zip(kinds, sources))
    if na >= 5:                                                  # notes on the word seams only: shifted across them and off both ends
        q[4 * steps:5 * steps] = False
        q[4 * steps:5 * steps, SEAM] = True
    def images(cells):
        x = np.zeros((1, 2, len(cells), 128), np.float32)
        if plane == 0:
            x[0, 0] = cells
            x[0, 1] = rng.random(cells.shape) < 0.5              # the sustain channel is not part of the onset plane
        else:
            half = rng.random(cells.shape) < 0.5                 # sounding = onset | sustain
            x[0, 0], x[0, 1] = cells & half, cells & ~half
        x.setflags(write=False)
        return x
    a_starts = (np.arange(na, dtype=np.int32)[::-1] * steps).copy()
    b_starts = rng.permutation(nb).astype(np.int32)
    return images(q), a_starts, images(c), b_starts, plan


_CACHE = {}


def case_and_reference(case):
    """The case's data, its packed words (packed by the restatement: these tests do not lean on pf_roll_pack) and the restatement's answer,
    computed once and shared, never modified."""
    if case not in _CACHE:
        steps, na, nb, S, topk, plane = case
        xq, a_starts, xc, b_starts, plan = make_match_case(*case, seed=100 + MATCH_CASES.index(case))
        want = ref.match_images(xq, a_starts, xc, b_starts, steps, S, topk, plane)
        for v in want.values():
            v.setflags(write=False)
        _CACHE[case] = dict(xq=xq, xc=xc, a_starts=a_starts, b_starts=b_starts, plan=plan, want=want,
                            a_bits=ref.pack(xq)[plane], b_bits=ref.pack(xc)[plane])
    return _CACHE[case]


def run_match(lib, a_bits, a_starts, b_bits, b_starts, steps, S, topk, tables, bufs=None):
    """One pf_roll_match call on device tensors into guarded buffers; returns {name: (whole, view)} including the workspace."""
    na, nb = int(a_starts.numel()), int(b_starts.numel())
    if bufs is None:
        bufs = {k: guarded((na, topk)) for k in OUTS}
        if tables:
            bufs.update({k: guarded((na, nb)) for k in TABS})
        need = int(lib.pf_roll_match_workspace_bytes(na, nb, topk))
        assert need > 0 and need % 4 == 0
        bufs["workspace"] = guarded((need // 4,))
    p = lambda k: bufs[k][1].data_ptr() if k in bufs else None
    a = _lib.RollMatchArgs(a_bits=a_bits.data_ptr(), a_starts=a_starts.data_ptr(), b_bits=b_bits.data_ptr(), b_starts=b_starts.data_ptr(),
                           na=na, nb=nb, steps=steps, shifts=S, topk=topk, reserved=0, top_index=p("index"), top_shift=p("shift"),
                           top_inter=p("inter"), top_union=p("union"), tab_inter=p("tab_inter"), tab_union=p("tab_union"),
                           tab_shift=p("tab_shift"), workspace=p("workspace"), workspace_bytes=bufs["workspace"][1].numel() * 4)
    _lib.check(lib.pf_roll_match(C.byref(a), _lib.current_stream()), "pf_roll_match", lib)
    return bufs


def assert_equal(bufs, want, what):
    for name, (whole, got) in bufs.items():
        assert untouched(whole), (what, name, "sentinel overwritten")
        if name == "workspace":
            continue
        g = got.cpu().numpy()
        assert not (g == GARBAGE).any(), (what, name, "a word was not written")
        bad = np.argwhere(g != want[name])
        assert bad.size == 0, (what, name, bad[:8].tolist(), g[tuple(bad[0])], want[name][tuple(bad[0])])


def on_device(d):
    return dev_bits(d["a_bits"]), torch.from_numpy(d["a_starts"]).cuda(), dev_bits(d["b_bits"]), torch.from_numpy(d["b_starts"]).cuda()


@pytest.mark.parametrize("case", MATCH_CASES, ids=lambda c: "steps%d-na%d-nb%d-S%d-top%d-plane%d" % c)
def test_every_word_equals_the_restatement_with_and_without_tables(lib, case):
    steps, na, nb, S, topk, plane = case
    d = case_and_reference(case)
    args = on_device(d)
    with_tables = run_match(lib, *args, steps, S, topk, True)
    assert_equal(with_tables, d["want"], (case, "tables"))
    without = run_match(lib, *args, steps, S, topk, False)
    assert_equal(without, d["want"], (case, "no tables"))
    for k in OUTS:
        assert torch.equal(with_tables[k][1], without[k][1]), k
    if nb < topk:                                                # slots beyond nb
        assert (d["want"]["index"][:, nb:] == -1).all() and not d["want"]["union"][:, nb:].any()


def test_the_planted_cases_are_really_in_the_data():
    # exact copies at every shift come back with J = 1 at that shift (S = 12: nothing wide enough to leave the keyboard is not asserted, only
    # that the restatement finds a full overlap wherever the transposed window kept all its notes)
    d = case_and_reference((4, 17, CHUNK - 1, 15, 8, 0))
    w = d["want"]
    shifts_found = set()
    for i, (kind, b) in enumerate(d["plan"]):
        row = d["a_starts"].tolist().index(i * 4)
        if kind == 1 and w["inter"][row, 0] == w["union"][row, 0] > 0:
            shifts_found.add(int(w["shift"][row, 0]))
    assert len(shifts_found) >= 3 and any(s < 0 for s in shifts_found) and any(s > 0 for s in shifts_found)
    empty_q = [d["a_starts"].tolist().index(i * 4) for i, (kind, _) in enumerate(d["plan"]) if kind == 3]
    assert empty_q
    for r in empty_q:                                           # an empty query: every fraction is 0, ties go to the lowest b and to s = 0
        assert w["index"][r].tolist() == list(range(8)) and not w["shift"][r].any() and not w["inter"][r].any()
    pos_of_empty = d["b_starts"].tolist().index(1)               # the empty corpus window against the empty query: 0 / 0 counts as 0 / 1
    assert w["tab_union"][empty_q[0], pos_of_empty] == 0 and w["tab_shift"][empty_q[0], pos_of_empty] == 0
    assert d["xq"][0, 0, 16:20].sum() == 4 * len(SEAM)            # the seam-only query: its notes cross words and leave both ends when shifted
    # the noisy copy among distractors: the restatement itself separates them
    d = case_and_reference((128, 17, 40, 1, 3, 1))
    w = d["want"]
    j = ref.jaccard(w["inter"], w["union"])
    noisy = [d["a_starts"].tolist().index(i * 128) for i, (kind, _) in enumerate(d["plan"]) if kind == 2]
    plain = [d["a_starts"].tolist().index(i * 128) for i, (kind, _) in enumerate(d["plan"]) if kind == 0 and i != 4]
    print("noisy copies:", j[noisy, 0].tolist(), "their runners-up:", j[noisy, 1].tolist(), "random queries:", j[plain, 0].tolist())
    assert (j[noisy, 0] > 0.7).all() and (j[noisy, 1] < 0.1).all() and (j[plain, 0] < 0.1).all()
    # a duplicated corpus window: the one visited first (the lower b) is listed first
    d = case_and_reference((4, 3, 4100, 1, 3, 0))
    first, second = (d["b_starts"].tolist().index(s) for s in (11, 16))
    ti, tu = d["want"]["tab_inter"], d["want"]["tab_union"]
    assert (ti[:, first] == ti[:, second]).all() and (tu[:, first] == tu[:, second]).all()


def merge_lists(parts, topk):
    """Two top-k results over disjoint corpus halves (indices already global) -> the top-k of the whole, by the stated order."""
    out = {k: [] for k in OUTS}
    for a in range(parts[0]["index"].shape[0]):
        cands = [(p["inter"][a, r], p["union"][a, r], p["index"][a, r], p["shift"][a, r]) for p in parts for r in range(topk) if p["index"][a, r] >= 0]
        kept = []
        for c in sorted(cands, key=lambda c: c[2]):
            pos = len(kept)
            while pos > 0 and ref.better(c[0], c[1], kept[pos - 1][0], kept[pos - 1][1]):
                pos -= 1
            kept.insert(pos, c)
        kept = (kept + [(0, 0, -1, 0)] * topk)[:topk]
        for k, col in zip(("inter", "union", "index", "shift"), range(4)):
            out[k].append([c[col] for c in kept])
    return {k: np.array(v, np.int32) for k, v in out.items()}


def test_repeats_and_split_calls_give_the_same_rows(lib):
    case = (4, 17, CHUNK + 1, 1, 8, 1)
    steps, na, nb, S, topk, plane = case
    d = case_and_reference(case)
    a_bits, a_starts, b_bits, b_starts = on_device(d)
    first = run_match(lib, a_bits, a_starts, b_bits, b_starts, steps, S, topk, True)
    again = run_match(lib, a_bits, a_starts, b_bits, b_starts, steps, S, topk, True)
    for k in OUTS + TABS:
        assert torch.equal(first[k][1], again[k][1]), k
    # the queries over two calls
    cut = 5
    parts = [run_match(lib, a_bits, s.contiguous(), b_bits, b_starts, steps, S, topk, True) for s in (a_starts[:cut], a_starts[cut:])]
    for k in OUTS + TABS:
        assert torch.equal(torch.cat([parts[0][k][1], parts[1][k][1]]), first[k][1]), k
    # the corpus over two calls (not at a chunk boundary), merged on the host by the stated order
    cut = 100
    halves = []
    for lo, hi in ((0, cut), (cut, nb)):
        r = run_match(lib, a_bits, a_starts, b_bits, b_starts[lo:hi].contiguous(), steps, S, topk, False)
        h = {k: r[k][1].cpu().numpy().copy() for k in OUTS}
        h["index"][h["index"] >= 0] += lo
        halves.append(h)
    merged = merge_lists(halves, topk)
    for k in OUTS:
        assert np.array_equal(merged[k], d["want"][k]), k


def test_a_captured_call_replays_the_same_words(lib):
    case = (4, 3, CHUNK, 12, 3, 0)
    steps, na, nb, S, topk, plane = case
    d = case_and_reference(case)
    args = on_device(d)
    bufs = run_match(lib, *args, steps, S, topk, True)                           # eager first: the module is loaded outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run_match(lib, *args, steps, S, topk, True, bufs=bufs)
    for name, (_, view) in bufs.items():
        view.fill_(GARBAGE)
    g.replay()
    torch.cuda.synchronize()
    assert_equal(bufs, d["want"], "graph replay")


# ---------------------------------------------------------------------------------------------- the host layer on the device
def test_nearest_and_pairwise_equal_the_restatement():
    from polyffusion_amd import rollmatch
    rng = np.random.default_rng(8)
    songs = [(rng.random((s, 2, 128, 128)) < 0.03).astype(np.float32) for s in (2, 1, 3)]
    songs.append((rng.random((1, 2, 40, 128)) < 0.03).astype(np.float32))        # shorter than a window: zero-padded
    songs[2][..., 126:] = 0                                                      # nothing of song c leaves the keyboard when moved up by 2
    corpus = rollmatch.Corpus.from_songs(songs, ["a", "b", "c", "short"], hop=16)
    q = (rng.random((2, 2, 2, 128, 128)) < 0.03).astype(np.float32)              # two songs of two images
    src = songs[2].transpose(1, 0, 2, 3).reshape(2, -1, 128)[:, 48:48 + 128]      # rows 48.. of song c: bar 3, transposed up by 2 below
    q[1, 0, :, :, 2:] = src[:, :, :-2]
    q[1, 0, :, :, :2] = 0
    for plane in ("onset", "sounding"):
        m = rollmatch.nearest(torch.from_numpy(q).cuda(), corpus, shifts=3, topk=2, plane=plane)
        pl = rollmatch.PLANES[plane]
        parts = []
        for s in songs:
            r = ref.planes(s)[pl]
            parts.append(r if len(r) >= 128 else np.concatenate([r, np.zeros((128 - len(r), 128), bool)]))
        rows = np.concatenate(parts)
        want = ref.match(ref.windows(ref.planes(q.reshape(4, 2, 128, 128))[pl], [0, 128, 256, 384], 128),
                         ref.windows(rows, corpus.starts, 128), 3, 2)
        for k in OUTS:
            assert np.array_equal(getattr(m, k).cpu().numpy(), want[k]), (plane, k)
        assert m.jaccard.dtype == torch.float64 and m.jaccard.is_cuda
        assert np.array_equal(m.jaccard.cpu().numpy(), ref.jaccard(want["inter"], want["union"]))
        assert m.where()[2][0] == ("c", 3) and int(m.shift[2, 0]) == 2 and int(m.inter[2, 0]) == int(m.union[2, 0]) > 0
        per_song = m.songs(2)
        assert per_song[1]["copy_score"] == 1.0 and per_song[1]["nearest"] == dict(song="c", bar=3, shift=2, image=0, window=int(m.index[2, 0]))
        assert per_song[0]["copy_score"] == float(max(m.jaccard[0, 0], m.jaccard[1, 0])) < 0.2
    # pairwise: the dense tables of a set against itself
    imgs = q.reshape(4, 2, 128, 128).copy()
    imgs[3] = imgs[0]                                                             # song 1's second image repeats song 0's first
    pw = rollmatch.pairwise(torch.from_numpy(imgs).cuda(), segments=2, shifts=1)
    win = ref.windows(ref.planes(imgs)[0], [0, 128, 256, 384], 128)
    want = ref.match(win, win, 1, 1)
    jac = ref.jaccard(want["tab_inter"], want["tab_union"])
    assert np.array_equal(pw["jaccard"], jac) and np.array_equal(pw["shift"], want["tab_shift"])
    assert pw["nearest_other"].tolist() == [1.0, 1.0] and pw["diversity"] == 0.0 and (np.diag(jac) == 1.0).all()
    one = rollmatch.pairwise(torch.from_numpy(imgs[:2]).cuda(), segments=2)
    assert one["nearest_other"].tolist() == [0.0] and one["diversity"] == 1.0


# ---------------------------------------------------------------------------------------------- end to end
BASE = ["--params_preset", "sdf_chd8bar", "--synthetic_weights", "--synthetic", "--ddim", "--ddim_steps", "2", "--seed", "5", "--precision", "bf16x3",
        "--length", "1"]


def run_main(out, argv, capsys):
    from polyffusion_amd import inference_sdf
    assert inference_sdf.main(BASE + ["--output_dir", str(out)] + argv) == 0
    said = capsys.readouterr().out
    files = {}
    for f in glob.glob(os.path.join(str(out), "*.npy")):
        m = re.search(r"_\d{6}_(\d+)\.npy$", f)
        files[int(m.group(1)) if m else 0] = f
    docs = glob.glob(os.path.join(str(out), "*_score.json"))
    return files, (json.load(open(docs[0])) if docs else None), said


def test_cli_reports_copy_score_diversity_and_ranks_by_novelty(tmp_path, capsys):
    from polyffusion_amd import rollmatch
    first, _, _ = run_main(tmp_path / "first", ["--num_generate", "4"], capsys)
    assert sorted(first) == [0, 1, 2, 3]
    rng = np.random.default_rng(21)
    synthetic = [(rng.random((2, 2, 128, 128)) < 0.03).astype(np.float32) for _ in range(3)]
    for i, s in enumerate(synthetic):
        np.save(tmp_path / f"syn{i}.npy", s)
    corpus_file = str(tmp_path / "corpus.npz")
    sources = [str(tmp_path / f"syn{i}.npy") for i in range(3)] + [first[1]]       # ... plus one of the run's own outputs
    assert rollmatch.main(["build", "--from_npy"] + sources + ["--out", corpus_file]) == 0
    capsys.readouterr()
    kept, doc, said = run_main(tmp_path / "second", ["--num_generate", "2", "--best_of", "2", "--rank_by", "novelty", "--novelty_corpus", corpus_file,
                                                      "--diversity", "--score"], capsys)
    # the four candidates are the four songs of the first run (same keys and shards as that many plain generations)
    cands = [np.load(first[i]) for i in range(4)]
    corpus = rollmatch.Corpus.load(corpus_file)
    rows = np.concatenate([ref.planes(np.load(f))[0] for f in sources])
    cwin = ref.windows(rows, corpus.starts, 128)
    want = ref.match(np.stack([ref.planes(c)[0] for c in cands]), cwin, 6, 3)
    jac = ref.jaccard(want["inter"], want["union"])
    assert len(doc["candidates"]) == 4
    for i, c in enumerate(doc["candidates"]):
        assert c["copy_score"] == jac[i, 0], i
        song, bar = corpus.where(int(want["index"][i, 0]))
        assert c["nearest"] == dict(song=song, bar=bar, shift=int(want["shift"][i, 0]), image=0, window=int(want["index"][i, 0])), i
    re_fed = doc["candidates"][1]
    assert re_fed["copy_score"] == 1.0 and re_fed["nearest"]["song"] == first[1] and re_fed["nearest"]["shift"] == 0 and re_fed["nearest"]["bar"] == 0
    order = sorted(range(4), key=lambda i: (jac[i, 0], i))[:2]                    # least copied first, ties to the earlier candidate
    assert [s["candidate"] for s in doc["songs"]] == order and 1 not in order and doc["rank_by"] == "novelty"
    for r, cand in enumerate(order):
        assert np.array_equal(np.load(kept[r]).view(np.uint32), cands[cand].view(np.uint32)), (r, cand)
    win = np.stack([ref.planes(cands[i])[0] for i in order])
    pw = ref.match(win, win, 0, 1)
    pj = ref.jaccard(pw["tab_inter"], pw["tab_union"])
    other = [float(pj[0, 1]), float(pj[1, 0])]
    assert [s["nearest_other"] for s in doc["songs"]] == other and doc["diversity"] == 1.0 - float(np.mean(other))
    assert "copy_score" in said and "diversity" in said and "nearest_other" in said


def song_novelty(roll, corpus, corpus_rows, shifts=6, topk=3):
    """What ``MatchResult.songs`` must give for one written song: the restatement on its rows cut into windows of 128 steps"""
    rows = ref.planes(roll.reshape(-1, 2, roll.shape[-2], 128))[0]
    want = ref.match(ref.windows(rows, list(range(0, len(rows), 128)), 128), ref.windows(corpus_rows, corpus.starts, 128), shifts, topk)
    jac = ref.jaccard(want["inter"], want["union"])[:, 0]
    i = int(np.argmax(jac))
    song, bar = corpus.where(int(want["index"][i, 0]))
    return dict(copy_score=float(jac[i]), nearest=dict(song=song, bar=bar, shift=int(want["shift"][i, 0]), image=i, window=int(want["index"][i, 0])))


def test_edit_morph_autoreg_and_the_scorer_report_novelty(tmp_path, capsys):
    from polyffusion_amd import inference_sdf, rollmatch, score, synth
    rng = np.random.default_rng(9)
    a = (synth.chords(1, 42), (rng.random((1, 2, 128, 128)) > 0.95).astype(np.float32))
    b = (synth.chords(1, 43), (rng.random((1, 2, 128, 128)) > 0.95).astype(np.float32))
    other = (rng.random((2, 2, 128, 128)) > 0.95).astype(np.float32)
    for name, (chord, image) in (("a", a), ("b", b)):
        np.savez(tmp_path / f"{name}.npz", chord=chord, prmat2c=image)
    corpus = rollmatch.Corpus.from_songs([a[1], other], ["a", "other"])
    corpus_rows = np.concatenate([ref.planes(s)[0] for s in (a[1], other)])
    cfile = str(tmp_path / "corpus.npz")
    corpus.save(cfile)
    core = ["--params_preset", "sdf_chd8bar", "--synthetic_weights", "--ddim", "--ddim_steps", "2", "--seed", "9", "--precision", "bf16x3"]
    # --edit: the source is in the corpus, the edited image is scored as the restatement scores the written file
    out = tmp_path / "edit"
    assert inference_sdf.main(core + ["--output_dir", str(out), "--cond_npz", str(tmp_path / "a.npz"), "--edit", "--edit_iters", "1",
                                      "--edit_chord_shift", "2", "--score", "--novelty_corpus", cfile]) == 0
    said = capsys.readouterr().out
    doc = json.load(open(glob.glob(str(out / "*_score.json"))[0]))
    edited = np.load([f for f in glob.glob(str(out / "*.npy")) if "roundtrip" not in f][0])
    assert doc["source_novelty"] == dict(copy_score=1.0, nearest=dict(song="a", bar=0, shift=0, image=0, window=0))
    assert doc["edited_novelty"] == song_novelty(edited, corpus, corpus_rows) and "edit score (novelty): source image copy_score 1.0000 (nearest a bar 0 shift +0)" in said
    # --morph: every frame, and the frames' diversity
    out = tmp_path / "morph"
    assert inference_sdf.main(core + ["--output_dir", str(out), "--morph", "--morph_frames", "3", "--morph_iters", "1", "--score", "--novelty_corpus", cfile,
                                      "--novelty_shifts", "2", "--diversity", "--cond_npz", str(tmp_path / "a.npz"), "--morph_to_npz",
                                      str(tmp_path / "b.npz")]) == 0
    said = capsys.readouterr().out
    gen = np.load(glob.glob(str(out / "*_morph.npy"))[0])
    doc = json.load(open(glob.glob(str(out / "*_score.json"))[0]))
    assert doc["novelty"] == [song_novelty(gen[k], corpus, corpus_rows, shifts=2) for k in range(3)] and "frame 2 novelty: copy_score" in said
    win = np.stack([ref.planes(gen[k])[0] for k in range(3)])
    pw = ref.match(win, win, 0, 1)
    pj = ref.jaccard(pw["tab_inter"], pw["tab_union"])
    other_best = [float(max(pj[k, j] for j in range(3) if j != k)) for k in range(3)]
    assert doc["nearest_other"] == other_best and doc["diversity"] == float(1.0 - np.mean(other_best))
    # --autoreg: the two halves of a segment are one window of 128 steps
    files, doc, said = run_main(tmp_path / "autoreg", ["--autoreg", "--num_generate", "1", "--score", "--novelty_corpus", cfile, "--diversity"], capsys)
    roll = np.load(files[0])
    assert roll.shape == (2, 2, 64, 128) and {k: doc["candidates"][0][k] for k in ("copy_score", "nearest")} == song_novelty(roll, corpus, corpus_rows)
    assert doc["songs"][0]["nearest_other"] == 0.0 and doc["diversity"] == 1.0 and doc["novelty"]["masked"] is False
    # the stand-alone scorer on a written roll
    np.save(tmp_path / "roll.npy", edited)
    assert score.main(["--npy", str(tmp_path / "roll.npy"), "--novelty_corpus", cfile, "--novelty_topk", "2"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert {k: line[k] for k in ("copy_score", "nearest")} == song_novelty(edited, corpus, corpus_rows, topk=2)
    assert len(line["novelty"]["matches"]) == 1 and len(line["novelty"]["matches"][0]) == 2
