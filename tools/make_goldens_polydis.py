#!/usr/bin/env python
"""tests/golden/polydis.npz: the reference's Polydis model on synthetic weights (build container only).

Loads ``weights.synth_polydis_state`` into the REAL ``polydis.model.DisentangleVAE.init_model()`` and records what its inference
methods compute, plus the note lists ``PolydisAftertouch.reconstruct`` and ``utils.prmat_to_midi_file`` hand to pretty_midi (replaced by
the recording stand-in of make_goldens_notes.py).  Arrays only, never reference source.

Row selection is the rule of make_goldens_decoders.py, unchanged: a candidate is decoded in float64 and in float32 and kept only if
every top-1 / top-2 gap of the float64 run is at least MIN_GAP and the float32 grid equals the float64 grid.  Two groups of KEEP rows:
"encoded" rows (prmat, chd) taken from ``synth`` and run through both encoders, and "direct" rows z ~ N(0, 1).  The pool is widened
until KEEP rows are found; the gap never moves.  For the encoded rows a pool of 1024 that yields fewer than KEEP keeps what cleared,
provided that is at least 2 (asserted).
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from make_goldens_decoders import gap_top2, lengths_of, run  # noqa: E402
from make_goldens_notes import import_utils  # noqa: E402
from polyffusion_amd import synth  # noqa: E402
from polyffusion_amd.weights import synth_polydis_state  # noqa: E402

MIN_GAP = 1e-3
KEEP = 4
SEED_W, SEED_PR, SEED_CHD, SEED_Z = 0, 301, 401, 501
LOGIT_STEPS = (0, 15, 31)


def build_model(cls, state, dtype):
    torch.set_default_dtype(dtype)
    try:
        m = cls.init_model()
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in state.items()}, strict=True)
    finally:
        torch.set_default_dtype(torch.float32)
    return m.eval()


def decode_logits(m, dtype, z):
    return run(lambda a: m.decoder(a, True, None, None, 0.0, 0.0), dtype, z)


def grid(p, u):
    return torch.cat([p.max(-1)[1].unsqueeze(-1), u.max(-1)[1]], -1)


def clear(p64, u64, p32, u32):
    margin = torch.minimum(gap_top2(p64).flatten(1).min(1).values, (u64[..., 0] - u64[..., 1]).abs().flatten(1).min(1).values)
    ok = (margin >= MIN_GAP) & (grid(p32, u32) == grid(p64, u64)).flatten(1).all(1)
    return ok, margin


def encode(m, dtype, pr, c):
    def f(pr_, c_):
        d_c, d_r = m.inference_encode(pr_, c_)
        return d_c.mean, d_c.scale, d_r.mean, d_r.scale
    return run(f, dtype, pr, c)


def notes_of(midi):
    assert len(midi.instruments) == 1
    return np.array([(n.pitch, n.start, n.end, n.velocity) for n in midi.instruments[0].notes], dtype=np.float64).reshape(-1, 4)


def main():
    utils, PM = import_utils()          # recording pretty_midi first: ptvae.py and utils bind to it
    from polydis.model import DisentangleVAE
    from polydis_aftertouch import PolydisAftertouch
    st = synth_polydis_state(SEED_W)
    m32, m64 = build_model(DisentangleVAE, st, torch.float32), build_model(DisentangleVAE, st, torch.float64)
    sd = m32.state_dict()
    out = {"min_gap": MIN_GAP, "seed_w": SEED_W, "max_simu_note": int(m32.decoder.max_simu_note)}
    out["param_names"] = np.array(list(sd.keys()))
    out["param_shapes"] = np.array([list(sd[k].shape) + [0] * (4 - sd[k].dim()) for k in sd])
    S = out["max_simu_note"]

    # ---- encoded rows
    pool = 32
    while True:
        pr = torch.from_numpy(synth.prmat(pool // 4, SEED_PR)).reshape(-1, 32, 128)
        c = torch.from_numpy(synth.chords(pool // 4, SEED_CHD)).reshape(-1, 8, 36)
        enc64, enc32 = encode(m64, torch.float64, pr, c), encode(m32, torch.float32, pr, c)
        p64, u64 = decode_logits(m64, torch.float64, torch.cat([enc64[0], enc64[2]], -1))
        p32, u32 = decode_logits(m32, torch.float32, torch.cat([enc32[0], enc32[2]], -1))
        ok, margin = clear(p64, u64, p32, u32)
        keep = torch.nonzero(ok).flatten()[:KEEP]
        print(f"encoded: pool {pool}, {int(ok.sum())} rows clear the gap; mean rms chd {float(enc64[0].pow(2).mean().sqrt()):.3f} "
              f"rhy {float(enc64[2].pow(2).mean().sqrt()):.3f}")
        if len(keep) == KEEP or pool >= 1024:
            break
        pool *= 2
    assert len(keep) >= 2, "fewer than two encoded rows clear the gap in a pool of 1024: check the synthetic weights"
    e64 = grid(p64, u64)
    out["enc_pool"], out["enc_seed_pr"], out["enc_seed_chd"], out["enc_rows"] = pool, SEED_PR, SEED_CHD, keep.numpy()
    out["enc_prmat"], out["enc_chd"] = pr[keep].numpy().astype(np.int8), c[keep].numpy().astype(np.int8)
    assert np.array_equal(out["enc_prmat"].astype(np.float32), pr[keep].numpy()) and np.array_equal(out["enc_chd"].astype(np.float32), c[keep].numpy())
    for i, name in enumerate(("chd_mean", "chd_scale", "rhy_mean", "rhy_scale")):
        out[f"{name}_f32"], out[f"{name}_f64"] = enc32[i][keep].numpy(), enc64[i][keep].numpy()
    out["enc_ref_f32_f64"] = float(max((enc32[i][keep].double() - enc64[i][keep]).abs().max() for i in range(4)))
    out["enc_scale_ref_rel_f32_f64"] = float(max(((enc32[i][keep].double() - enc64[i][keep]).abs() / enc64[i][keep]).max() for i in (1, 3)))
    est = torch.from_numpy(run(lambda a, b: m32.inference(a, b, False), torch.float32, pr[keep], c[keep]))
    assert torch.equal(est, e64[keep]) and tuple(est.shape) == (len(keep), 32, S - 1, 6) and est.dtype == torch.int64
    out["enc_est"] = est.numpy().astype(np.int16)
    out["enc_lengths"] = lengths_of(e64[keep]).numpy().astype(np.int16)
    out["enc_min_margin"] = float(margin[keep].min())
    out["dec_ref_f32_f64"] = float(max((p32[keep].double() - p64[keep]).abs().max(), (u32[keep].double() - u64[keep]).abs().max()))
    out["logit_scale"] = float(p64[keep].std())
    # one row's logits at three time steps (a full row at 32 slots is 555 KB)
    r0 = int(keep[0])
    out["logit_steps"] = np.array(LOGIT_STEPS)
    out["logit_pitch"], out["logit_dur"] = p32[r0, list(LOGIT_STEPS)].numpy(), u32[r0, list(LOGIT_STEPS)].numpy()

    # ---- one swap call: texture of one kept row, chords of another; the pair must clear the gap like any other row
    pairs = [(i, j) for i in range(len(keep)) for j in range(len(keep)) if i != j]
    pi, ci = keep[[a for a, _ in pairs]], keep[[b for _, b in pairs]]
    sp64, su64 = decode_logits(m64, torch.float64, torch.cat([enc64[0][ci], enc64[2][pi]], -1))
    sp32, su32 = decode_logits(m32, torch.float32, torch.cat([enc32[0][ci], enc32[2][pi]], -1))
    sok, smargin = clear(sp64, su64, sp32, su32)
    good = torch.nonzero(sok).flatten()[:2].tolist()
    assert len(good) == 2, "no two (texture row, chord row) pairs clear the gap"
    a_rows, b_rows = [pairs[g][0] for g in good], [pairs[g][1] for g in good]          # indices into the kept rows
    sw = run(lambda p1, p2, c1, c2: m32.swap(p1, p2, c1, c2, True, False), torch.float32, pr[keep[a_rows]], pr[keep[b_rows]],
             c[keep[a_rows]], c[keep[b_rows]])                                          # = inference(pr[a], c[b])
    assert np.array_equal(sw, grid(sp64, su64)[good].numpy())
    out["swap_rows_pr"], out["swap_rows_chd"], out["swap_est"] = np.array(a_rows), np.array(b_rows), sw.astype(np.int16)
    out["swap_min_margin"] = float(smargin[good].min())

    # ---- direct rows z ~ N(0, 1)
    pool_z = 32
    while True:
        z = torch.from_numpy(np.random.Generator(np.random.PCG64(SEED_Z)).standard_normal((pool_z, 512)).astype(np.float32))
        zp64, zu64 = decode_logits(m64, torch.float64, z)
        zp32, zu32 = decode_logits(m32, torch.float32, z)
        zok, zmargin = clear(zp64, zu64, zp32, zu32)
        zkeep = torch.nonzero(zok).flatten()[:KEEP]
        print(f"direct: pool {pool_z}, {int(zok.sum())} rows clear the gap; lengths seen {sorted(set(lengths_of(grid(zp64, zu64)).flatten().tolist()))}")
        if len(zkeep) == KEEP:
            break
        pool_z *= 2
        assert pool_z <= 1024, "no usable direct rows: check the synthetic weights"
    zest = run(lambda a, b: m32.inference_decode(a, b), torch.float32, z[zkeep][:, :256], z[zkeep][:, 256:])
    assert np.array_equal(zest, grid(zp64, zu64)[zkeep].numpy())
    out["z_pool"], out["z_seed"], out["z_rows"], out["z"] = pool_z, SEED_Z, zkeep.numpy(), z[zkeep].numpy()
    out["z_est"] = zest.astype(np.int16)
    out["z_lengths"] = lengths_of(grid(zp64, zu64)[zkeep]).numpy().astype(np.int16)
    out["z_min_margin"] = float(zmargin[zkeep].min())
    lens = set(out["enc_lengths"].flatten().tolist()) | set(out["z_lengths"].flatten().tolist())
    assert len(lens) >= 2, lens

    # ---- the note lists of the two writers
    aft = PolydisAftertouch.__new__(PolydisAftertouch)      # its constructor reads the trained checkpoint; the model is the one above
    aft.model = m32
    aft.reconstruct(pr[keep], c[keep], "unused.mid")
    out["recon_notes"] = notes_of(PM.last)
    utils.prmat_to_midi_file(pr[keep], "unused.mid")
    out["prmat_notes"] = notes_of(PM.last)
    out["notes"] = np.array(f"encoded rows kept: {len(keep)} of a pool of {pool} (rule: {KEEP}, or what cleared in 1024 if at least 2); direct rows: "
                            f"{len(zkeep)} of {pool_z}; gap {MIN_GAP}; lengths {sorted(lens)}")

    path = os.path.join(OUT, "polydis.npz")
    np.savez_compressed(path, **out)
    print("polydis.npz", os.path.getsize(path) // 1024, "KiB;", str(out["notes"]), "; margins", out["enc_min_margin"], out["swap_min_margin"],
          out["z_min_margin"], "; ref f32-f64: encoders", out["enc_ref_f32_f64"], "decoder", out["dec_ref_f32_f64"])
    assert os.path.getsize(path) <= 981751 // 2


if __name__ == "__main__":
    main()
