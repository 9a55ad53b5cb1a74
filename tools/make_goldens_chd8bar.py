#!/usr/bin/env python
"""tests/golden/chd8bar.npz: the reference's ``Chord_8Bar`` objective on synthetic weights (build container only).

Loads ``weights.synth_chord_encoder_state`` / ``synth_chord_decoder_state`` into the REAL ``dl_modules.ChordEncoder`` / ``ChordDecoder``
/ ``models.model_chd_8bar.Chord_8Bar`` and records, in float32 and float64, the encoder's Normal, the teacher-forced logits and the
losses.  Arrays only, never reference source.

What the reference leaves to global generators is recorded: the ``eps`` of ``rsample()`` is a stored array (``rsample`` is
``loc + eps * scale``; one real ``get_loss_dict`` under a seeded torch generator is checked against that form below), and the
teacher-forcing flips are Python's ``random`` under a stored seed (rate 0 gives mask 0, rate 1 the all-ones mask, rate 0.5 a mixed one).

Two nets: "s" (36, 256, 512, 256, n_step 8) and "c", chd_8bar's (36, 512, 512, 512, n_step 32).  Per net a pool of 32 samples
(``synth.chords``, z noise from PCG64).  The masks are run ROW BY ROW (the reference's fed-back token is only the one-hot it means to be
at batch 1, ``chord_dec.py:59-63``); one batch of 4 is run as a batch and gives the ``feedback="batch"`` case.  A decode is a chain of
arg-maxes, so a row is kept only if every top-1 / top-2 gap of its float64 run is at least MIN_GAP and its float32 decisions equal the
float64 ones (the method of make_goldens_decoders.py); the batch of 4 must clear the gap as a whole.  The gap never moves.
"""
import os
import random
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from make_goldens import import_reference  # noqa: E402
from make_goldens_decoders import build, gap_top2, run  # noqa: E402
from polyffusion_amd import synth  # noqa: E402
from polyffusion_amd.weights import synth_chord_decoder_state, synth_chord_encoder_state  # noqa: E402

MIN_GAP = 1e-3
KEEP, POOL = 8, 32
NETS = {"s": dict(input_dim=36, z_input_dim=256, hidden_dim=512, z_dim=256, n_step=8),
        "c": dict(input_dim=36, z_input_dim=512, hidden_dim=512, z_dim=512, n_step=32)}
SEED_W, SEED_CHD, SEED_NOISE, SEED_FLIP = 0, 301, 401, 501
RATES = {"m0": 0.0, "mh": 0.5, "m1": 1.0}
STEPS = np.array([0, 1, 1000, 19999, 20000, 20001, 40000, 123456], dtype=np.int64)


def flips_of(rate, n):
    random.seed(SEED_FLIP)
    return [random.random() < rate for _ in range(n)]


def margin_and_decisions(root, chroma, bass):
    m = torch.stack([gap_top2(root).flatten(1).min(1).values, gap_top2(bass).flatten(1).min(1).values,
                     (chroma[..., 0] - chroma[..., 1]).abs().flatten(1).min(1).values]).min(0).values
    dec = torch.cat([root.argmax(-1).flatten(1), chroma.argmax(-1).flatten(1), bass.argmax(-1).flatten(1)], 1)
    return m, dec


def main():
    import_reference()
    from dl_modules import ChordDecoder, ChordEncoder
    from models.model_chd_8bar import Chord_8Bar
    import importlib.util
    from make_goldens import REF
    spec = importlib.util.spec_from_file_location("pf_ref_scheduler", os.path.join(REF, "train", "scheduler.py"))   # train/__init__ needs Lightning
    sched = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sched)
    scheduled_sampling = sched.scheduled_sampling
    out = {"min_gap": MIN_GAP, "seed_w": SEED_W, "seed_flip": SEED_FLIP, "sched_steps": STEPS,
           "sched_tfr": np.array([scheduled_sampling(float(s), 0.5, 0.0) for s in STEPS], dtype=np.float64),
           "sched_default": np.array([scheduled_sampling(float(s)) for s in STEPS], dtype=np.float64)}
    worst = {"logits": 0.0, "loss": 0.0}
    for tag, net in NETS.items():
        n, zd = net["n_step"], net["z_dim"]
        est, dst = (synth_chord_encoder_state(SEED_W, 36, net["hidden_dim"], zd),
                    synth_chord_decoder_state(SEED_W, 36, net["z_input_dim"], net["hidden_dim"], zd))
        models = {}
        for dtype in (torch.float32, torch.float64):
            enc = build(ChordEncoder, est, dtype, input_dim=36, hidden_dim=net["hidden_dim"], z_dim=zd)
            dec = build(ChordDecoder, dst, dtype, **net)
            models[dtype] = Chord_8Bar(enc, dec)
        chord = torch.from_numpy(synth.chords(POOL, SEED_CHD, n))
        noise = torch.from_numpy(np.random.Generator(np.random.PCG64(SEED_NOISE)).standard_normal((POOL, zd)).astype(np.float32))
        out[f"{tag}_chord"], out[f"{tag}_noise"] = chord.numpy().astype(np.int8), noise.numpy()

        def dist(dtype):
            d = run(lambda c: models[dtype].chord_enc(c), dtype, chord)
            return d.mean, d.scale

        def decode(dtype, z, gt, rate, rows=None):
            """The real decoder and chord_loss, one call per row (rows=None) or one call on the rows given."""
            m = models[dtype]

            def call(zz, cc):
                random.seed(SEED_FLIP)
                logits = m.chord_dec(zz, False, rate, cc)
                return logits, m.chord_loss(cc, *logits)
            if rows is not None:
                logits, loss = run(call, dtype, z[rows], gt[rows])
                return logits, torch.stack([loss[k] for k in ("loss", "root", "chroma", "bass")])
            res = [run(call, dtype, z[i:i + 1], gt[i:i + 1]) for i in range(z.shape[0])]
            logits = tuple(torch.cat(t) for t in zip(*[r[0] for r in res]))
            return logits, torch.stack([torch.stack([r[1][k] for k in ("loss", "root", "chroma", "bass")]) for r in res])

        (mu32, sc32), (mu64, sc64) = dist(torch.float32), dist(torch.float64)
        z32, z64 = mu32 + noise * sc32, mu64 + noise.double() * sc64
        # the Normal of the first four pool rows only (the file has a size limit); z for the whole pool in float32
        out[f"{tag}_mean32"], out[f"{tag}_scale32"], out[f"{tag}_mean64"], out[f"{tag}_scale64"] = (t[:4].numpy() for t in (mu32, sc32, mu64, sc64))
        out[f"{tag}_z32"], out[f"{tag}_z64_head"] = z32.numpy(), z64[:4].numpy()
        with torch.no_grad():
            for mk, rate in RATES.items():
                flips = flips_of(rate, n - 1)
                assert mk != "m0" or not any(flips)
                assert mk != "m1" or all(flips)
                assert mk != "mh" or (any(flips) and not all(flips))
                l64, loss64 = decode(torch.float64, z64, chord, rate)
                l32, loss32 = decode(torch.float32, z32, chord, rate)
                m64, d64 = margin_and_decisions(*l64)
                _, d32 = margin_and_decisions(*l32)
                ok = (m64 >= MIN_GAP) & (d32 == d64).all(1)
                keep = torch.nonzero(ok).flatten()[:KEEP]
                print(f"net {tag} mask {mk}: {int(ok.sum())} of {POOL} rows clear the gap")
                assert len(keep) == KEEP, "widen the pool (the gap does not move)"
                out[f"{tag}_{mk}_flips"], out[f"{tag}_{mk}_rows"] = np.array(flips), keep.numpy()
                for name, a32, a64 in zip(("root", "chroma", "bass"), l32, l64):
                    out[f"{tag}_{mk}_{name}32"], out[f"{tag}_{mk}_{name}64"] = a32[keep].numpy(), a64[keep].numpy()
                    worst["logits"] = max(worst["logits"], float((a32[keep].double() - a64[keep]).abs().max()))
                out[f"{tag}_{mk}_loss32"], out[f"{tag}_{mk}_loss64"] = loss32[keep].numpy(), loss64[keep].numpy()   # [KEEP][loss, root, chroma, bass]
                out[f"{tag}_{mk}_margin"] = float(m64[keep].min())
                worst["loss"] = max(worst["loss"], float((loss32[keep].double() - loss64[keep]).abs().max()))
            # the batch of 4 under the mixed mask: four consecutive pool rows whose BATCHED run clears the gap as a whole
            found = None
            for start in range(POOL - 3):
                rows = torch.arange(start, start + 4)
                l64, loss64 = decode(torch.float64, z64, chord, RATES["mh"], rows)
                l32, loss32 = decode(torch.float32, z32, chord, RATES["mh"], rows)
                m64, d64 = margin_and_decisions(*l64)
                _, d32 = margin_and_decisions(*l32)
                if bool((m64 >= MIN_GAP).all()) and torch.equal(d32, d64):
                    found = start
                    break
            assert found is not None, "no batch of 4 clears the gap: widen the pool"
            # it must differ from the row-by-row decode, or it shows nothing
            lrow, _ = decode(torch.float64, z64[rows], chord[rows], RATES["mh"])
            diff = max(float((a - b).abs().max()) for a, b in zip(l64, lrow))
            print(f"net {tag} batch of 4 at pool rows {found}..{found + 3}: margin {float(m64.min()):.3e}, batch vs row logits differ by {diff:.3e}")
            assert diff > 1e-3
            out[f"{tag}_b4_rows"] = rows.numpy()
            for name, a32, a64 in zip(("root", "chroma", "bass"), l32, l64):
                out[f"{tag}_b4_{name}32"], out[f"{tag}_b4_{name}64"] = a32.numpy(), a64.numpy()
                worst["logits"] = max(worst["logits"], float((a32.double() - a64).abs().max()))
            out[f"{tag}_b4_loss32"], out[f"{tag}_b4_loss64"] = loss32.numpy(), loss64.numpy()                       # [loss, root, chroma, bass]
            out[f"{tag}_b4_margin"] = float(m64.min())
            worst["loss"] = max(worst["loss"], float((loss32.double() - loss64).abs().max()))
            # one REAL get_loss_dict under seeded generators: the recorded-noise form above is what it computes, and it draws n_step - 1
            # numbers from `random` also at rate 0
            rows = out[f"{tag}_b4_rows"]
            batch = (None, None, chord[rows], None)
            for rate in (0.0, 0.5):
                torch.manual_seed(77)
                eps = torch.empty(4, zd).normal_()
                torch.manual_seed(77)
                random.seed(SEED_FLIP)
                real = models[torch.float32].get_loss_dict(batch, 0, rate)
                after = random.random()
                random.seed(SEED_FLIP)
                d4 = models[torch.float32].chord_enc(chord[rows])          # (at its own batch size: float32 GEMMs are not batch-invariant)
                logits = models[torch.float32].chord_dec(d4.mean + eps * d4.scale, False, rate, chord[rows])
                mine = models[torch.float32].chord_loss(chord[rows], *logits)
                assert all(torch.equal(real[k], mine[k]) for k in real), "rsample is not loc + eps * scale under this torch"
                random.seed(SEED_FLIP)
                for _ in range(n - 1):
                    random.random()
                assert random.random() == after
            out[f"{tag}_random_calls"], out[f"{tag}_random_next"] = n - 1, after
    out["ref_f32_f64_logits"], out["ref_f32_f64_loss"] = worst["logits"], worst["loss"]
    path = os.path.join(OUT, "chd8bar.npz")
    np.savez_compressed(path, **out)
    print("chd8bar.npz", os.path.getsize(path) // 1024, "KiB; reference float32 vs float64: logits", worst["logits"], "loss", worst["loss"])
    assert os.path.getsize(path) <= 1_000_000


if __name__ == "__main__":
    main()
