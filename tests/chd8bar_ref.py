"""A numpy restatement of ``Chord_8Bar`` (``ref:models/model_chd_8bar.py``) in float64, nothing of the product imported: the encoder's
Normal (``ref:dl_modules/chord_enc.py``), the teacher-forced decode of ``ref:dl_modules/chord_dec.py:27-70`` in both feedback forms, and
``chord_loss``.  tests/test_chd8bar_oracle.py pins it to tests/golden/chd8bar.npz (recorded from the reference's own modules); the GPU
tests use it as their oracle for the shapes the fixture does not hold.
"""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chd8bar.npz")
NETS = {"s": dict(input_dim=36, z_input_dim=256, hidden_dim=512, z_dim=256, n_step=8),
        "c": dict(input_dim=36, z_input_dim=512, hidden_dim=512, z_dim=512, n_step=32)}


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(GOLDEN))


def states(net: dict, seed: int = 0):
    """The synthetic encoder / decoder tensors of a net (``polyffusion_amd.weights``: pure numpy generators)."""
    from polyffusion_amd.weights import synth_chord_decoder_state, synth_chord_encoder_state
    return (synth_chord_encoder_state(seed, net["input_dim"], net["hidden_dim"], net["z_dim"]),
            synth_chord_decoder_state(seed, net["input_dim"], net["z_input_dim"], net["hidden_dim"], net["z_dim"]))


def _w(state, dtype):
    return {k: np.asarray(v).astype(dtype) for k, v in state.items()}


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _gru_cell(x, h, w, name="gru", sfx=""):
    gi = x @ w[f"{name}.weight_ih_l0{sfx}"].T + w[f"{name}.bias_ih_l0{sfx}"]
    gh = h @ w[f"{name}.weight_hh_l0{sfx}"].T + w[f"{name}.bias_hh_l0{sfx}"]
    H = h.shape[-1]
    r = _sigmoid(gi[..., :H] + gh[..., :H])
    z = _sigmoid(gi[..., H:2 * H] + gh[..., H:2 * H])
    n = np.tanh(gi[..., 2 * H:] + r * gh[..., 2 * H:])
    return (1 - z) * n + z * h


def _lin(x, w, name):
    return x @ w[f"{name}.weight"].T + w[f"{name}.bias"]


def encoder_dist(enc_state, chord, dtype=np.float64):
    """``RnnEncoder.forward``: ``(mean, scale)`` of the Normal, each ``[B, z_dim]``."""
    w, x = _w(enc_state, dtype), np.asarray(chord).astype(dtype)
    B, T, H = x.shape[0], x.shape[1], w["gru.weight_hh_l0"].shape[1]
    hf = hb = np.zeros((B, H), dtype)
    for t in range(T):
        hf = _gru_cell(x[:, t], hf, w)
        hb = _gru_cell(x[:, T - 1 - t], hb, w, sfx="_reverse")
    h = np.concatenate([hf, hb], -1)
    return _lin(h, w, "linear_mu"), np.exp(_lin(h, w, "linear_var"))


def _one_hot(idx, n, dtype):
    return np.eye(n, dtype=dtype)[idx]


def decode_forced(dec_state, z, gt, flips, feedback="row", n_step=None, dtype=np.float64):
    """``ChordDecoder.forward(z, False, tfr, gt)`` with the coin flips handed in (``flips[t]``: ``gt[:, t]`` is fed to step ``t + 1``).
    ``feedback="row"``: every row feeds back its own arg-max token (the reference at batch 1).  ``"batch"``: the reference at batch > 1,
    whose fancy-indexed assignment gives every row the union of the batch's root and bass arg-maxes (``chord_dec.py:59-63``)."""
    w, z, gt = _w(dec_state, dtype), np.asarray(z).astype(dtype), np.asarray(gt).astype(dtype)
    n_step = gt.shape[1] if n_step is None else n_step
    R = z.shape[0]
    h, z_in = _lin(z, w, "z2dec_hid"), _lin(z, w, "z2dec_in")
    token = np.broadcast_to(w["init_input"], (R, 36))
    roots, chromas, basses = [], [], []
    for t in range(n_step):
        h = _gru_cell(np.concatenate([token, z_in], -1), h, w)
        root, chroma, bass = _lin(h, w, "root_out"), _lin(h, w, "chroma_out").reshape(R, 12, 2), _lin(h, w, "bass_out")
        roots.append(root), chromas.append(chroma), basses.append(bass)
        if t == n_step - 1:
            break
        if flips[t]:
            token = gt[:, t]
        else:
            t_root, t_bass = _one_hot(root.argmax(-1), 12, dtype), _one_hot(bass.argmax(-1), 12, dtype)
            if feedback == "batch":
                t_root, t_bass = np.broadcast_to(t_root.max(0), (R, 12)), np.broadcast_to(t_bass.max(0), (R, 12))
            token = np.concatenate([t_root, chroma.argmax(-1).astype(dtype), t_bass], -1)
    return np.stack(roots, 1), np.stack(chromas, 1), np.stack(basses, 1)


def _nll(logits, target):
    """``-log_softmax(logits)[target]`` along the last axis."""
    m = logits.max(-1, keepdims=True)
    lse = m[..., 0] + np.log(np.exp(logits - m).sum(-1))
    return lse - np.take_along_axis(logits, target[..., None], -1)[..., 0]


def targets(c):
    c = np.asarray(c)
    return c[..., 0:12].argmax(-1), c[..., 12:24].astype(np.int64), c[..., 24:36].argmax(-1)


def ce_rows(c, root, chroma, bass):
    """Per-row sums ``[B, 3]`` of the three cross-entropies (float64) and per-row hit counts ``[B, 3]``."""
    t_root, t_chroma, t_bass = targets(c)
    root, chroma, bass = (np.asarray(a).astype(np.float64) for a in (root, chroma, bass))
    B = root.shape[0]
    chroma = chroma.reshape(B, -1, 12, 2)
    ce = np.stack([_nll(root, t_root).sum(1), _nll(chroma, t_chroma).sum((1, 2)), _nll(bass, t_bass).sum(1)], 1)
    hit = np.stack([(root.argmax(-1) == t_root).sum(1), (chroma.argmax(-1) == t_chroma).sum((1, 2)), (bass.argmax(-1) == t_bass).sum(1)], 1)
    return ce, hit


def chord_loss(c, root, chroma, bass):
    """``Chord_8Bar.chord_loss``: ``{"loss", "root", "chroma", "bass"}`` as float64 (means over all items of the batch)."""
    ce, _ = ce_rows(c, root, chroma, bass)
    B, n = root.shape[0], root.shape[1]
    r, ch, b = ce[:, 0].sum() / (B * n), ce[:, 1].sum() / (B * n * 12), ce[:, 2].sum() / (B * n)
    return {"loss": r + ch + b, "root": r, "chroma": ch, "bass": b}


def get_loss(enc_state, dec_state, chord, noise, flips, feedback="row", dtype=np.float64):
    """``get_loss_dict`` with the noise and the flips handed in: ``(loss dict, (root, chroma, bass), z)``."""
    mean, scale = encoder_dist(enc_state, chord, dtype)
    z = mean + scale * np.asarray(noise).astype(dtype)
    logits = decode_forced(dec_state, z, chord, flips, feedback, dtype=dtype)
    return chord_loss(chord, *logits), logits, z


def min_margin(root, chroma, bass):
    """Smallest top-1 / top-2 gap over every decision of each row."""
    def top2(x):
        s = np.sort(x, -1)
        return (s[..., -1] - s[..., -2]).reshape(x.shape[0], -1).min(1)
    return np.minimum(np.minimum(top2(root), top2(bass)), np.abs(chroma[..., 0] - chroma[..., 1]).reshape(chroma.shape[0], -1).min(1))


def mask_of(flips):
    return sum(1 << t for t, f in enumerate(flips) if f)
