"""Score a checkpoint: the reference's ``val/loss`` on the HIP path.

``LightningLearner.validation_step`` (``lightning_learner.py:41-52``) calls ``model.get_loss_dict(batch, step)`` on every validation
batch and Lightning logs the mean over the epoch as ``val/loss`` - the number ``ModelCheckpoint(monitor="val/loss")``
(``train/__init__.py:85-92``) ranks checkpoints by.  ``validation_loss`` is that loop over any iterable of reference-layout batches
``(prmat2c, pnotree, chord, prmat)`` - the contract of ``expr.py``'s drivers - for a ``Polyffusion_SDF`` or a ``Polyffusion_DDPM``.

What is pinned that the reference leaves to global generators: the time steps come, batch after batch, from ONE CPU generator
seeded with ``seed``; batch ``k`` takes its noise as draw ``k`` of the library's counter-based generator under ``seed``, every sample's
noise keyed by the sample's GLOBAL index (``elem_offset``).  The ``mix`` / ``mix2`` condition dropout uses Python's ``random`` as the
reference does; seed it to pin it.

``--model chd_8bar`` scores the chord VAE (``chd8bar.Chord_8Bar``) instead: ``validation_loss_chd8bar`` is the same loop over its
``get_loss_dict(batch, step, tfr_chd)``, with the noise of ``rsample`` pinned in the same way and the teacher-forcing flips taken from
the seeded ``random``.

CLI: ``python -m polyffusion_amd.validate`` prints one JSON line.
"""
from __future__ import annotations

import json
import math
import os
import random
import sys
from argparse import ArgumentParser
from typing import Iterable, Iterator, Optional

import numpy as np
import torch

N_BUCKETS = 10


def t_buckets(t, loss, n_steps: int, n: int = N_BUCKETS):
    """The per-sample losses averaged inside ``n`` equal ranges of ``t``: bucket ``i`` holds ``i * n_steps / n <= t < (i + 1) * n_steps / n``.
    Returns a list of ``{"t_lo", "t_hi", "count", "loss"}`` (``loss`` is ``None`` for an empty bucket); the buckets partition the samples."""
    t, loss = np.asarray(t, np.int64), np.asarray(loss, np.float64)
    idx = np.minimum(t * n // n_steps, n - 1)
    out = []
    for i in range(n):
        m = idx == i
        out.append({"t_lo": -(-i * n_steps // n), "t_hi": -(-(i + 1) * n_steps // n), "count": int(m.sum()),
                    "loss": float(loss[m].mean()) if m.any() else None})
    return out


def validation_loss(model, batches: Iterable, num: Optional[int] = None, *, seed: int = 0) -> dict:
    """The loop of ``validation_step`` over the first ``num`` batches (all of them for ``None``).  ``model``: anything with the
    ``get_loss_dict(batch, step, detail=True, seed=, draw=, elem_offset=)`` of ``Polyffusion_SDF`` / ``Polyffusion_DDPM``.

    Returns ``{"val/loss": mean of the batch losses (Lightning's epoch mean), "n_samples", "n_batches", "batch_losses",
    "t": int64 [n_samples], "loss": float64 [n_samples] (the per-sample (t, loss) pairs), "t_buckets": t_buckets(...)}``.
    Raises on a non-finite loss, as the reference's learner does in training (``lightning_learner.py:28-33``)."""
    n_steps = model.ldm.n_steps if hasattr(model, "ldm") else model.ddpm.n_steps
    batch_losses, ts, rows = [], [], []
    offset = 0
    gen = torch.Generator().manual_seed(int(seed))
    for k, batch in enumerate(batches):
        if num is not None and k >= num:
            break
        t = torch.randint(0, n_steps, (batch[0].shape[0],), generator=gen, dtype=torch.int64)
        d = model.get_loss_dict(batch, k, detail=True, t=t, seed=seed, draw=k, elem_offset=offset)
        loss = float(d["loss"])
        if not math.isfinite(loss):
            raise RuntimeError(f"Detected non-finite loss {loss} at validation batch {k}")
        batch_losses.append(loss)
        ts.append(d["t"].cpu())
        rows.append(d["loss_rows"].cpu())
        offset += batch[0].numel()
    if not batch_losses:
        raise RuntimeError("validation_loss: no batches")
    t, loss_rows = torch.cat(ts).numpy(), torch.cat(rows).numpy()
    return {"val/loss": float(np.mean(batch_losses)), "n_samples": int(t.shape[0]), "n_batches": len(batch_losses),
            "batch_losses": batch_losses, "t": t, "loss": loss_rows, "t_buckets": t_buckets(t, loss_rows, n_steps)}


def validation_loss_chd8bar(model, batches: Iterable, num: Optional[int] = None, *, seed: int = 0, tfr_chd: float = 0.0,
                            feedback: str = "row") -> dict:
    """The loop of ``validation_step`` for a ``chd8bar.Chord_8Bar``: batch ``k`` takes its noise as draw ``k`` under ``seed`` with the
    sample's GLOBAL index as element offset, and its ``n_step - 1`` flips from Python's ``random``.

    Returns ``{"val/loss", "val/root", "val/chroma", "val/bass"`` (means of the batch values), ``"acc/root", "acc/chroma", "acc/bass"``
    (correct arg-maxes over all samples), ``"n_samples", "n_batches", "batch_losses", "loss_rows"`` (float64 ``[n_samples, 3]``: every
    sample's own three means), ``"flips"`` (per batch)``}``.  Raises on a non-finite loss."""
    keys = ("loss", "root", "chroma", "bass")
    per_batch = {k: [] for k in keys}
    rows, hits, flips = [], [], []
    offset, z_dim, n_step = 0, model.chord_enc.z_dim, model.chord_dec.n_step
    for k, batch in enumerate(batches):
        if num is not None and k >= num:
            break
        d = model.get_loss_dict(batch, k, tfr_chd, detail=True, feedback=feedback, seed=seed, draw=k, elem_offset=offset)
        loss = float(d["loss64"])
        if not math.isfinite(loss):
            raise RuntimeError(f"Detected non-finite loss {loss} at validation batch {k}")
        per_batch["loss"].append(loss)
        for key in keys[1:]:
            per_batch[key].append(float(d["loss_rows"][:, keys.index(key) - 1].mean()))
        rows.append(d["loss_rows"].cpu())
        hits.append(d["hit_rows"].cpu())
        flips.append(d["flips"])
        offset += batch[2].shape[0] * z_dim
    if not per_batch["loss"]:
        raise RuntimeError("validation_loss_chd8bar: no batches")
    loss_rows, hit = torch.cat(rows).numpy(), torch.cat(hits).numpy().astype(np.int64)
    n = loss_rows.shape[0]
    out = {f"val/{key}": float(np.mean(per_batch[key])) for key in keys}
    for i, (key, per_row) in enumerate((("root", n_step), ("chroma", 12 * n_step), ("bass", n_step))):
        out[f"acc/{key}"] = float(hit[:, i].sum() / (n * per_row))
    out.update(n_samples=int(n), n_batches=len(per_batch["loss"]), batch_losses=per_batch["loss"], loss_rows=loss_rows, flips=flips)
    return out


# ---- batch sources ---------------------------------------------------------------------------------------------------------------
def synthetic_batches(batch_size: int, num: int, seed: int = 0, device="cuda", pnotree: bool = False) -> Iterator:
    """``num`` seeded reference-layout batches: a generated-sample-like piano-roll image, chords and a texture matrix."""
    from . import synth
    for k in range(num):
        s = seed + 1000 * k
        p2c = torch.from_numpy(synth.prmat2c_image(s + 1, batch_size)).float().to(device)
        pt = torch.from_numpy(synth.pnotree(batch_size, s + 300)).to(device) if pnotree else None
        yield (p2c, pt, torch.from_numpy(synth.chords(batch_size, s + 100)).to(device), torch.from_numpy(synth.prmat(batch_size, s + 200)).to(device))


def synthetic_chord_batches(batch_size: int, num: int, seed: int = 0, device="cuda", n_step: int = 32) -> Iterator:
    """``num`` batches that carry chords only, sample ``g`` of the epoch seeded by ``g`` itself: the same samples however the epoch is
    cut into batches."""
    from . import synth
    for k in range(num):
        chd = np.concatenate([synth.chords(1, seed + 100 + g, n_step) for g in range(k * batch_size, (k + 1) * batch_size)])
        yield (None, None, torch.from_numpy(chd).to(device), None)


def song_batches(samples: Iterable, batch_size: int, device="cuda") -> Iterator:
    """The 8-bar segments of ``DataSample`` objects, ``batch_size`` at a time, with the piano-tree grid kept (``expr.song_batches``
    drops it); a dataset without chords (Musicalion) yields ``chord = None``."""
    buf = []

    def stack(buf):
        cols = list(zip(*buf))
        return tuple(None if c[0] is None else torch.stack(c).to(device) for c in cols)

    for sample in samples:
        p2c, pt, chd, prmat = sample.get_whole_song_data()
        for i in range(p2c.shape[0]):
            buf.append((p2c[i], pt[i], None if chd is None else chd[i], prmat[i]))
            if len(buf) == batch_size:
                yield stack(buf)
                buf = []
    if buf:
        yield stack(buf)


def dataset_samples(dataset: str, data_dir: Optional[str], split_dir: str) -> Iterator:
    """Every song of the validation half of the dataset's split (``inference_sdf.py:95-118`` picks one of them)."""
    from . import datasample
    n = len(datasample.load_split(os.path.join(split_dir, f"{dataset}.pickle"))[1])
    for i in range(n):
        yield datasample.choose_song_from_val_dl(dataset, i, (0, 1, 2), data_dir, split_dir)[0]


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------
def make_parser() -> ArgumentParser:
    from . import datasample
    p = ArgumentParser(description="validation loss (val/loss) of a Polyffusion checkpoint on the MI355X-native path")
    p.add_argument("--model", choices=["sdf", "ddpm", "chd_8bar"], default="sdf")
    p.add_argument("--tfr_chd", type=float, default=0.0, help="chd_8bar: teacher-forcing rate of the decode (default 0: every step feeds its arg-max back)")
    p.add_argument("--global_step", type=int, help="chd_8bar: take the rate the training schedule hands out at this step (the params' tfr_chd pair)")
    p.add_argument("--feedback", choices=["row", "batch"], default="row",
                   help="chd_8bar: fed-back token per row (batch-invariant) or the reference's union over the batch (its logged number at the same batch size)")
    p.add_argument("--chkpt_path", help="the checkpoint (.pt / .ckpt, or a run directory holding chkpts/)")
    p.add_argument("--chkpt_name", default="weights_best.pt")
    p.add_argument("--custom_params_path", help="params yaml/json; default <chkpt>/../../params.yaml")
    p.add_argument("--params_preset", help="a built-in params preset instead of a params.yaml (e.g. sdf_chd8bar)")
    p.add_argument("--precision", choices=["f32", "bf16x3", "f16x3"], default="bf16x3", help="arithmetic of the denoiser's contractions")
    p.add_argument("--seed", type=int, default=0, help="keys the time steps, the noise and the condition dropout")
    p.add_argument("--from_dataset", help="validation half of a dataset's split {pop909, musicalion}")
    p.add_argument("--dataset_dir", help="directory of the dataset's song .npz files")
    p.add_argument("--split_dir", default=datasample.TRAIN_SPLIT_DIR, help="directory of the <dataset>.pickle split files")
    p.add_argument("--from_song_npz", nargs="+", help="quantised songs in the reference's data-dictionary format")
    p.add_argument("--synthetic", action="store_true", help="seeded synthetic batches")
    p.add_argument("--synthetic_weights", action="store_true", help="deterministic synthetic weights instead of a checkpoint")
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--batch_num", type=int, help="number of batches to evaluate (default: all; required with --synthetic)")
    return p


def _load_sdf(args):
    from . import inference_sdf
    from .params import find_params, load_params, preset
    if args.params_preset is not None:
        params = preset(args.params_preset)
    elif args.chkpt_path is not None or args.custom_params_path is not None:
        params = load_params(find_params(args.chkpt_path or ".", args.custom_params_path))
    elif args.synthetic_weights:
        params = preset("sdf_chd8bar")
    else:
        raise SystemExit("give --chkpt_path, --custom_params_path or --params_preset")
    model = inference_sdf.load_model(params, args)
    model.concat_blurry, model.concat_ratio = bool(params.get("concat_blurry", False)), params.get("concat_ratio", 1 / 8)
    model.ldm.eps_model.set_precision(args.precision)
    return model, params.model_name, params.cond_type == "pnotree"


def _load_ddpm(args):
    from . import ddpm
    from .weights import synth_ddpm_state
    x3 = "f16" if args.precision == "f16x3" else None
    if args.synthetic_weights:
        p = ddpm.params_from_dir(None)
        unet = ddpm.DDPMUNet(ddpm.DDPMConfig.from_params(p), x3=x3)
        unet.load_state_dict(synth_ddpm_state(unet.cfg, 0))
        diff = ddpm.DenoiseDiffusion(unet, int(p["n_steps"]))
    else:
        path = args.chkpt_path
        if path and os.path.exists(f"{path}/chkpts/{args.chkpt_name}"):
            path = f"{path}/chkpts/{args.chkpt_name}"
        if not path or not os.path.exists(path):
            raise SystemExit("--chkpt_path must name a ddpm checkpoint (or a run directory holding chkpts/)")
        diff = ddpm.load_trained(path, x3=x3)
    diff.eps_model.set_precision(args.precision)
    return ddpm.Polyffusion_DDPM(diff), "ddpm", False


def _load_chd8bar(args):
    from . import chd8bar
    from .params import load_params
    from .weights import synth_chord_decoder_state, synth_chord_encoder_state
    p = dict(chd8bar.CHD_8BAR)
    if args.custom_params_path is not None:
        p.update(load_params(args.custom_params_path))
    model = chd8bar.Chord_8Bar.from_params(p)
    if args.synthetic_weights:
        model.chord_enc.load_state_dict(synth_chord_encoder_state(0, p["chd_input_dim"], p["chd_hidden_dim"], p["chd_z_dim"]))
        model.chord_dec.load_state_dict(synth_chord_decoder_state(0, p["chd_input_dim"], p["chd_z_input_dim"], p["chd_hidden_dim"], p["chd_z_dim"]))
    else:
        path = args.chkpt_path
        if path and os.path.exists(f"{path}/chkpts/{args.chkpt_name}"):
            path = f"{path}/chkpts/{args.chkpt_name}"
        if not path or not os.path.exists(path):
            raise SystemExit("--chkpt_path must name a chd_8bar checkpoint (a file, a directory holding weights.pt, or a run directory holding chkpts/)")
        model = chd8bar.Chord_8Bar.load_trained(model.chord_enc, model.chord_dec, path)
    return model, p


def _batches(args, synthetic):
    """The batch source the flags name; ``synthetic()`` makes the model's seeded synthetic batches."""
    if args.synthetic:
        if args.batch_num is None:
            raise SystemExit("--synthetic needs --batch_num")
        return synthetic()
    if args.from_song_npz:
        from .datasample import DataSample
        return song_batches((DataSample.from_npz(p) for p in args.from_song_npz), args.batch_size)
    if args.from_dataset:
        try:
            return song_batches(dataset_samples(args.from_dataset, args.dataset_dir, args.split_dir), args.batch_size)
        except FileNotFoundError as e:
            raise SystemExit(f"--from_dataset {args.from_dataset}: {e} (give --dataset_dir / --split_dir)")
    raise SystemExit("no batch source: use --from_dataset, --from_song_npz or --synthetic")


def _main_chd8bar(args) -> dict:
    from . import chd8bar
    model, p = _load_chd8bar(args)
    tfr = chd8bar.teacher_forcing_rate(args.global_step, *p["tfr_chd"]) if args.global_step is not None else args.tfr_chd
    batches = _batches(args, lambda: synthetic_chord_batches(args.batch_size, args.batch_num, args.seed, n_step=p["chd_n_step"]))
    r = validation_loss_chd8bar(model, batches, args.batch_num, seed=args.seed, tfr_chd=tfr, feedback=args.feedback)
    line = {"model": "chd_8bar", "seed": args.seed, "tfr_chd": tfr, "feedback": args.feedback}
    line.update({k: r[k] for k in ("val/loss", "val/root", "val/chroma", "val/bass", "acc/root", "acc/chroma", "acc/bass", "n_samples",
                                   "n_batches", "batch_losses")})
    print(json.dumps(line))
    r.update(tfr_chd=tfr, feedback=args.feedback)
    return r


def main(argv=None) -> dict:
    args = make_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("validate needs an AMD GPU (no CPU fallback on this path)")
    random.seed(args.seed)
    if args.model == "chd_8bar":
        return _main_chd8bar(args)
    model, label, need_pnotree = (_load_sdf if args.model == "sdf" else _load_ddpm)(args)
    batches = _batches(args, lambda: synthetic_batches(args.batch_size, args.batch_num, args.seed, pnotree=need_pnotree))
    r = validation_loss(model, batches, args.batch_num, seed=args.seed)
    eps_model = model.ldm.eps_model if args.model == "sdf" else model.ddpm.eps_model
    line = {"model": label, "precision": eps_model.precision, "seed": args.seed, "val/loss": r["val/loss"], "n_samples": r["n_samples"],
            "n_batches": r["n_batches"], "batch_losses": r["batch_losses"], "t_buckets": r["t_buckets"]}
    print(json.dumps(line))
    return r


if __name__ == "__main__":
    main(sys.argv[1:])
