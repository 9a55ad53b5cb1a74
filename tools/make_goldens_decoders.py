#!/usr/bin/env python
"""tests/golden/decoders.npz: the reference's two frozen decoders on synthetic weights (build container only).

Loads ``weights.synth_pianotree_decoder_state`` / ``synth_chord_decoder_state`` into the REAL ``dl_modules.PianoTreeDecoder`` /
``ChordDecoder`` and decodes through the real ``Polyffusion_SDF._decode_pnotree`` / ``_decode_chord`` and ``utils.estx_to_midi_file``
(pretty_midi replaced by the recording stand-in of make_goldens_notes.py).  Arrays only, never reference source.

A decode is a chain of arg-maxes, so a row is only usable as a fixture if no decision in it is a near-tie.  Candidate rows are
z ~ N(0, 1) from a seeded pool; each is decoded in float64 and in float32 and kept only if every top-1 / top-2 gap of the float64 run
is at least MIN_GAP and the float32 grid equals the float64 grid.  The pool is widened until enough rows are found; the gap never moves.
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from make_goldens import import_reference  # noqa: E402
from make_goldens_notes import import_utils  # noqa: E402
from polyffusion_amd.weights import synth_chord_decoder_state, synth_pianotree_decoder_state  # noqa: E402

MIN_GAP = 1e-3
KEEP = 4
S = 20                      # max_simu_note of the sdf_pnotree variant
CHD = dict(input_dim=36, z_input_dim=256, hidden_dim=512, z_dim=256, n_step=8)
SEED_W, SEED_Z_PN, SEED_Z_CHD = 0, 101, 201


def gap_top2(x, dim=-1):
    top = torch.topk(x, 2, dim=dim).values
    return top[..., 0] - top[..., 1]


def build(cls, state, dtype, **kw):
    torch.set_default_dtype(dtype)
    try:
        m = cls(**kw)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in state.items()}, strict=True)
    finally:
        torch.set_default_dtype(torch.float32)
    return m.eval()


def run(fn, dtype, *args):
    torch.set_default_dtype(dtype)
    try:
        with torch.no_grad():
            return fn(*[a.to(dtype) for a in args])
    finally:
        torch.set_default_dtype(torch.float32)


def lengths_of(est):
    """Predicted length per (row, step): the slot (1-based) of the first end token, else the number of slots."""
    eos = (est[..., 0] == 129)
    first = torch.where(eos.any(-1), eos.float().argmax(-1) + 1, torch.full(eos.shape[:-1], est.shape[2], dtype=torch.long))
    return first


def main():
    utils, PM = import_utils()          # recording pretty_midi first: utils and dl_modules bind to it
    R = import_reference()
    from dl_modules import ChordDecoder, PianoTreeDecoder
    SDF = R["Polyffusion_SDF"]
    out = {"min_gap": MIN_GAP, "seed_w": SEED_W, "max_simu_note": S}
    out.update({f"chd_{k}": v for k, v in CHD.items()})

    # ---- PianoTree
    st = synth_pianotree_decoder_state(SEED_W)
    d32, d64 = build(PianoTreeDecoder, st, torch.float32, max_simu_note=S), build(PianoTreeDecoder, st, torch.float64, max_simu_note=S)
    names = list(d32.state_dict().keys())
    out["pn_param_names"] = np.array(names)
    out["pn_param_shapes"] = np.array([list(d32.state_dict()[k].shape) + [0] * (4 - d32.state_dict()[k].dim()) for k in names])
    # The first KEEP clearing rows of a pool must also exercise the variable-length embedding GRU (asserted below); where they do not,
    # the next pool seed is tried.  Neither the gap nor "the first KEEP rows" moves.
    seed_z, pool, found = SEED_Z_PN, 32, False
    while not found:
        z = torch.from_numpy(np.random.Generator(np.random.PCG64(seed_z)).standard_normal((pool, 512)).astype(np.float32))
        p64, u64 = run(lambda a: d64(a, True, None, None, 0.0, 0.0), torch.float64, z)
        p32, u32 = run(lambda a: d32(a, True, None, None, 0.0, 0.0), torch.float32, z)
        e64 = torch.cat([p64.max(-1)[1].unsqueeze(-1), u64.max(-1)[1]], -1)
        e32 = torch.cat([p32.max(-1)[1].unsqueeze(-1), u32.max(-1)[1]], -1)
        margin = torch.minimum(gap_top2(p64).flatten(1).min(1).values, (u64[..., 0] - u64[..., 1]).abs().flatten(1).min(1).values)
        ok = (margin >= MIN_GAP) & (e32 == e64).flatten(1).all(1)
        keep = torch.nonzero(ok).flatten()[:KEEP]
        print(f"pianotree: seed {seed_z}, pool {pool}, {int(ok.sum())} rows clear the gap; lengths seen {sorted(set(lengths_of(e64).flatten().tolist()))}")
        if len(keep) < KEEP:
            pool *= 2
            assert pool <= 1024, "no usable PianoTree rows: check the synthetic weights"
            continue
        lens = set(lengths_of(e64[keep]).flatten().tolist())
        found = len(lens) >= 3 and (S - 1) in lens and min(lens) <= 2
        if not found:
            print("  the kept rows do not exercise the variable lengths:", sorted(lens))
            seed_z, pool = seed_z + 1, 32
            assert seed_z < SEED_Z_PN + 16
    lens = set(lengths_of(e64[keep]).flatten().tolist())
    assert len(lens) >= 3 and (S - 1) in lens and min(lens) <= 2, lens
    out["pn_pool"], out["pn_seed_z"], out["pn_rows"] = pool, seed_z, keep.numpy()
    out["pn_z"] = z[keep].numpy()
    out["pn_est"] = e64[keep].numpy().astype(np.int16)
    out["pn_lengths"] = lengths_of(e64[keep]).numpy().astype(np.int16)
    out["pn_logit_rows"] = np.array([0, 1])
    out["pn_pitch"] = p32[keep[:2]].numpy()
    out["pn_dur"] = u32[keep[:2]].numpy()
    out["pn_min_margin"] = float(margin[keep].min())
    out["pn_ref_f32_f64"] = float(max((p32[keep].double() - p64[keep]).abs().max(), (u32[keep].double() - u64[keep]).abs().max()))
    out["pn_logit_scale"] = float(p64[keep].std())
    # _decode_pnotree at B = 2: eight slices built from the kept rows
    b2 = np.array([[0, 1, 2, 3], [3, 1, 0, 2]])
    zb = z[keep][torch.from_numpy(b2)].reshape(2, 1, 4 * 512)
    sdf = SDF(None, "pnotree", pnotree_dec=d32, chord_dec=None)
    with torch.no_grad():
        grid = sdf._decode_pnotree(zb)
    assert tuple(grid.shape) == (2, 128, S - 1, 6) and torch.equal(grid[0, :32], e32[keep[0]])
    out["pn_b2_rows"], out["pn_b2_grid"] = b2, grid.numpy().astype(np.int16)
    # utils.estx_to_midi_file on the kept grids, with labels
    labels = ["seg0", "seg1", "seg2", "seg3"]
    utils.estx_to_midi_file(e32[keep], "unused.mid", labels)
    midi = PM.last
    assert len(midi.instruments) == 1
    out["midi_notes"] = np.array([(n.pitch, n.start, n.end, n.velocity) for n in midi.instruments[0].notes], dtype=np.float64).reshape(-1, 4)
    out["midi_lyric_text"] = np.array([ly.text for ly in midi.lyrics])
    out["midi_lyric_time"] = np.array([ly.time for ly in midi.lyrics], dtype=np.float64)

    # ---- chord
    st = synth_chord_decoder_state(SEED_W, CHD["input_dim"], CHD["z_input_dim"], CHD["hidden_dim"], CHD["z_dim"])
    c32, c64 = build(ChordDecoder, st, torch.float32, **CHD), build(ChordDecoder, st, torch.float64, **CHD)
    names = list(c32.state_dict().keys())
    out["chd_param_names"] = np.array(names)
    out["chd_param_shapes"] = np.array([list(c32.state_dict()[k].shape) + [0] * (4 - c32.state_dict()[k].dim()) for k in names])
    pool = 32
    while True:
        z = torch.from_numpy(np.random.Generator(np.random.PCG64(SEED_Z_CHD)).standard_normal((pool, CHD["z_dim"])).astype(np.float32))
        # one row per call: the reference's feedback token indexes t_root[arange(bs), 0, idx] with idx of shape (bs, 1), which
        # broadcasts to (bs, bs) and sets every row's root / bass token to the union over the batch (chord_dec.py:59-63).  At batch 1 it
        # is the one-hot it means to be, and that is what the product computes for every row of a batch.
        per_row = lambda m: (lambda a: tuple(torch.cat(t) for t in zip(*[m(a[i:i + 1], True, 0.0) for i in range(a.shape[0])])))
        r64, c64o, b64 = run(per_row(c64), torch.float64, z)
        r32, c32o, b32 = run(per_row(c32), torch.float32, z)
        margin = torch.stack([gap_top2(r64).flatten(1).min(1).values, gap_top2(b64).flatten(1).min(1).values,
                              (c64o[..., 0] - c64o[..., 1]).abs().flatten(1).min(1).values]).min(0).values
        same = ((r32.max(-1)[1] == r64.max(-1)[1]).flatten(1).all(1) & (b32.max(-1)[1] == b64.max(-1)[1]).flatten(1).all(1) &
                (c32o.max(-1)[1] == c64o.max(-1)[1]).flatten(1).all(1))
        ok = (margin >= MIN_GAP) & same
        keep = torch.nonzero(ok).flatten()[:KEEP]
        print(f"chord: pool {pool}, {int(ok.sum())} rows clear the gap")
        if len(keep) == KEEP:
            break
        pool *= 2
        assert pool <= 1024
    out["chd_pool"], out["chd_seed_z"], out["chd_rows"] = pool, SEED_Z_CHD, keep.numpy()
    out["chd_z"] = z[keep].numpy()
    out["chd_root"], out["chd_chroma"], out["chd_bass"] = r32[keep].numpy(), c32o[keep].numpy(), b32[keep].numpy()
    out["chd_min_margin"] = float(margin[keep].min())
    out["chd_ref_f32_f64"] = float(max((r32[keep].double() - r64[keep]).abs().max(), (c32o[keep].double() - c64o[keep]).abs().max(),
                                       (b32[keep].double() - b64[keep]).abs().max()))
    sdf = SDF(None, "chord", chord_dec=c32)
    with torch.no_grad():
        out["chd_decoded"] = torch.cat([sdf._decode_chord(z[i:i + 1]) for i in keep.tolist()]).numpy().astype(np.int16)

    path = os.path.join(OUT, "decoders.npz")
    np.savez_compressed(path, **out)
    print("decoders.npz", os.path.getsize(path) // 1024, "KiB; pianotree min margin", out["pn_min_margin"], "f32-f64", out["pn_ref_f32_f64"],
          "lengths", sorted(set(out["pn_lengths"].flatten().tolist())), "; chord min margin", out["chd_min_margin"], "f32-f64",
          out["chd_ref_f32_f64"])
    assert os.path.getsize(path) <= 1_000_000


if __name__ == "__main__":
    main()
