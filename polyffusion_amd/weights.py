"""Deterministic synthetic weights in the reference checkpoint key namespace.

No trained checkpoint ships with the reference, so parity and
benchmarks run on synthetic weights.  Every tensor is drawn from its own
PCG64 stream keyed by ``seed`` and ``crc32(key)``, so the *same* weights are
regenerated bit-for-bit in the build container (where they are loaded into
the imported reference to make golden vectors) and on the GPU box.
"""
from __future__ import annotations

import zlib
from collections import OrderedDict
from typing import Dict, Tuple

import numpy as np

from .arch import (
    UNetConfig,
    chord_encoder_param_shapes,
    pianotree_encoder_param_shapes,
    texture_encoder_param_shapes,
    unet_param_shapes,
)


def _draw(key: str, shape: Tuple[int, ...], seed: int) -> np.ndarray:
    rng = np.random.Generator(np.random.PCG64([seed, zlib.crc32(key.encode())]))
    if len(shape) == 1:
        if key.endswith(".weight"):  # normalisation gain
            return (1.0 + 0.1 * rng.standard_normal(shape)).astype(np.float32)
        return (0.02 * rng.standard_normal(shape)).astype(np.float32)
    fan_in = int(np.prod(shape[1:]))
    std = (1.0 / fan_in) ** 0.5
    return (std * rng.standard_normal(shape)).astype(np.float32)


def synth_tensors(shapes: Dict[str, Tuple[int, ...]], seed: int = 0, prefix: str = "") -> "OrderedDict[str, np.ndarray]":
    return OrderedDict((prefix + k, _draw(prefix + k, s, seed)) for k, s in shapes.items())


def synth_unet_state(cfg: UNetConfig, seed: int = 0) -> "OrderedDict[str, np.ndarray]":
    """UNet tensors keyed relative to ``eps_model`` (e.g. ``input_blocks.0.0.weight``)."""
    return synth_tensors(unet_param_shapes(cfg), seed)


def synth_chord_encoder_state(seed: int = 0, input_dim=36, hidden_dim=512, z_dim=512):
    # GRU weights use U(-1/sqrt(H), 1/sqrt(H))-like scale so the recurrence stays bounded
    shapes = chord_encoder_param_shapes(input_dim, hidden_dim, z_dim)
    return _synth_rnn(shapes, seed, "chord_enc.", hidden_dim)


def synth_texture_encoder_state(seed: int = 0, emb_size=256, hidden_dim=1024, z_dim=256, num_channel=10):
    shapes = texture_encoder_param_shapes(emb_size, hidden_dim, z_dim, num_channel)
    return _synth_rnn(shapes, seed, "txt_enc.", hidden_dim)


def _synth_rnn(shapes, seed, prefix, hidden_dim):
    out = OrderedDict()
    for k, s in shapes.items():
        rng = np.random.Generator(np.random.PCG64([seed, zlib.crc32((prefix + k).encode())]))
        if k.startswith("gru."):
            b = 1.0 / hidden_dim ** 0.5
            out[k] = rng.uniform(-b, b, size=s).astype(np.float32)
        else:
            out[k] = _draw(prefix + k, s, seed)
    return out


def synth_pianotree_encoder_state(seed: int = 0, note_size=135, note_emb_size=128, enc_notes_hid_size=256, enc_time_hid_size=512, z_size=512):
    """PianoTreeEncoder tensors (dl_modules/pianotree_enc.py); GRU weights at torch's U(-1/sqrt(H), 1/sqrt(H)) scale."""
    shapes = pianotree_encoder_param_shapes(note_size, note_emb_size, enc_notes_hid_size, enc_time_hid_size, z_size)
    out = OrderedDict()
    for k, s in shapes.items():
        if "_gru." in k:
            hid = enc_notes_hid_size if k.startswith("enc_notes") else enc_time_hid_size
            rng = np.random.Generator(np.random.PCG64([seed, zlib.crc32(("pnotree_enc." + k).encode())]))
            out[k] = rng.uniform(-1.0 / hid ** 0.5, 1.0 / hid ** 0.5, size=s).astype(np.float32)
        else:
            out[k] = _draw("pnotree_enc." + k, s, seed)
    return out


def synth_ddpm_state(cfg, seed: int = 0) -> "OrderedDict[str, np.ndarray]":
    """Vanilla DDPM UNet tensors (ddpm.DDPMConfig) keyed relative to ``eps_model`` (e.g. ``down.0.res.conv1.weight``)."""
    from .ddpm import ddpm_param_shapes
    return synth_tensors(ddpm_param_shapes(cfg), seed)


def _synth_decoder(shapes, seed, prefix, gru_hidden, rand_keys):
    out = OrderedDict()
    for k, s in shapes.items():
        rng = np.random.Generator(np.random.PCG64([seed, zlib.crc32((prefix + k).encode())]))
        if ".weight_" in k or ".bias_ih_" in k or ".bias_hh_" in k:      # GRU tensors: torch's U(-1/sqrt(H), 1/sqrt(H))
            b = 1.0 / gru_hidden(k) ** 0.5
            out[k] = rng.uniform(-b, b, size=s).astype(np.float32)
        elif k in rand_keys:                                             # nn.Parameter(torch.rand(...)): U(0, 1)
            out[k] = rng.uniform(0.0, 1.0, size=s).astype(np.float32)
        else:
            out[k] = _draw(prefix + k, s, seed)
    return out


def synth_pianotree_decoder_state(seed: int = 0, dec_dur_hid_size: int = 16):
    """PianoTreeDecoder tensors at its default sizes (dl_modules/pianotree_dec.py); ``dec_dur_hid_size`` is the width of the duration
    GRU (16, or 64 as Polydis builds it).  ``note_embedding.*`` is the encoder's (the trained model shares it); the end-token bias is
    raised so that end tokens occur and the predicted lengths vary."""
    from .arch import pianotree_decoder_param_shapes
    hid = {"dec_notes_emb_gru": 128, "dec_time_gru": 1024, "dec_notes_gru": 512, "dec_dur_gru": dec_dur_hid_size}
    out = _synth_decoder(pianotree_decoder_param_shapes(dec_dur_hid_size=dec_dur_hid_size), seed, "pnotree_dec.",
                         lambda k: hid[k.split(".")[0]], ("dec_init_input", "dur_sos_token"))
    enc = synth_pianotree_encoder_state(seed)
    out["note_embedding.weight"], out["note_embedding.bias"] = enc["note_embedding.weight"], enc["note_embedding.bias"]
    out["pitch_out_linear.bias"] = out["pitch_out_linear.bias"].copy()
    out["pitch_out_linear.bias"][129] += np.float32(0.3)
    return out


def synth_chord_decoder_state(seed: int = 0, input_dim=36, z_input_dim=256, hidden_dim=512, z_dim=256):
    """ChordDecoder tensors (dl_modules/chord_dec.py)."""
    from .arch import chord_decoder_param_shapes
    return _synth_decoder(chord_decoder_param_shapes(input_dim, z_input_dim, hidden_dim, z_dim), seed, "chord_dec.", lambda k: hidden_dim,
                          ("init_input",))


# The synthetic linear_mu (rows of std 1/sqrt(2048) on the final GRU state) gives encoded means of rms 0.044 (chord encoder) and 0.32
# (texture encoder) on synth.chords / synth.prmat rows: below about 0.5 every row decodes to the same notes.  A constant gain on
# linear_mu.weight brings the rms of the means into [0.5, 2] (measured: about 0.9 and 1.0).  The two encoders' rms differ by a factor of
# 7.4, more than the band is wide, so there is one constant per encoder - chosen once, never per row or per input.
POLYDIS_MU_GAIN = {"chd_encoder.": 24.0, "rhy_encoder.": 3.0}


def synth_polydis_state(seed: int = 0):
    """A ``DisentangleVAE.init_model()`` state_dict (polydis/model.py:303-319) in its key order: ``chd_encoder.*`` RnnEncoder(36, 1024,
    256), ``rhy_encoder.*`` TextureEncoder(256, 1024, 256, 10), ``decoder.*`` PtvaeDecoder(dec_dur_hid_size=64), ``chd_decoder.*``
    RnnDecoder(z_dim=256) - the existing encoder / decoder generators under the four prefixes, the encoders' ``linear_mu.weight`` times
    ``POLYDIS_MU_GAIN``."""
    parts = (("chd_encoder.", synth_chord_encoder_state(seed, 36, 1024, 256)),
             ("rhy_encoder.", synth_texture_encoder_state(seed, 256, 1024, 256, 10)),
             ("decoder.", synth_pianotree_decoder_state(seed, 64)),
             ("chd_decoder.", synth_chord_decoder_state(seed, 36, 256, 512, 256)))
    out = OrderedDict()
    for prefix, st in parts:
        for k, v in st.items():
            out[prefix + k] = v * np.float32(POLYDIS_MU_GAIN[prefix]) if prefix in POLYDIS_MU_GAIN and k == "linear_mu.weight" else v
    return out


AUTOENCODER_BRANCH_GAIN = 0.5


def synth_autoencoder_state(cfg, seed: int = 0) -> "OrderedDict[str, np.ndarray]":
    """First-stage autoencoder tensors (autoencoder.AutoencoderConfig) keyed as the reference ``Autoencoder`` state_dict
    (``encoder.conv_in.weight`` ...).  Every conv is drawn at 1 / sqrt(fan_in), which keeps a layer's output at its input's scale;
    the convs that close a residual branch (``conv2`` of a ResnetBlock, ``proj_out`` of the AttnBlock) get AUTOENCODER_BRANCH_GAIN on
    top, so each of the up to 15 blocks in a row adds a quarter of a unit of variance to the stream instead of a whole one and the
    activations stay O(1) through the depth - which is what keeps an absolute tolerance on the outputs meaningful."""
    from .autoencoder import autoencoder_param_shapes
    out = synth_tensors(autoencoder_param_shapes(cfg), seed, "")
    for k in out:
        if k.endswith((".conv2.weight", ".proj_out.weight")):
            out[k] = (out[k] * np.float32(AUTOENCODER_BRANCH_GAIN)).astype(np.float32)
    return out
