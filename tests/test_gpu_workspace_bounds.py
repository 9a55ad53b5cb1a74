"""No launch of pf_encoder_forward / _forward_dist / pf_decoder_forward writes past the workspace the library asks for.

Every handle family, at the smallest shapes that still go through every buffer and an off-tile row count.  The C entry point gets exactly
``<prefix>_workspace_bytes`` bytes at the head of an allocation that is 64 KiB longer and whose tail carries a byte pattern: an overrun
lands in the tail (nothing faults) and is seen there.  The outputs must equal the ordinary Python call's bit for bit, and one byte less
must be refused ("workspace too small") with nothing enqueued."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from polyffusion_amd import _lib, synth  # noqa: E402
from polyffusion_amd import weights as W  # noqa: E402
from polyffusion_amd.model_sdf import ChordDecoder, ChordEncoder, PianoTreeDecoder, PianoTreeEncoder, TextureEncoder  # noqa: E402

TAIL, PATTERN, PF_EINVAL = 64 * 1024, 0xA5, -1


def _pnotree_grid(B: int, S: int) -> torch.Tensor:
    """[B,32,S,6]: per step sos, 0..S-2 notes, eos, pad (pitch 130, duration digits 2) - lengths 2..S, the reference's layout"""
    rng = np.random.Generator(np.random.PCG64(4))
    grid = np.full((B, 32, S, 6), 2, np.int64)
    grid[..., 0] = 130
    for b in range(B):
        for t in range(32):
            k = int(rng.integers(0, S - 1))
            grid[b, t, 0, 0] = 128
            grid[b, t, 1:1 + k, 0] = np.sort(rng.integers(36, 96, k))
            grid[b, t, 1:1 + k, 1:] = rng.integers(0, 2, (k, 5))
            grid[b, t, 1 + k, 0] = 129
    return torch.from_numpy(grid)


def _encoder(enc, x, n_step, dist):
    """(workspace bytes, call(ws_ptr, ws_bytes, outs) -> rc, the Python call's outputs, fresh outputs)"""
    x = x.cuda().float().contiguous()
    B = x.shape[0]
    want = enc.encode_dist(x) if dist else (enc.encode_mean(x),)
    outs = [torch.full_like(w, float("nan")) for w in want]
    nbytes = enc._lib.pf_encoder_workspace_bytes(enc._h, B)

    def call(ws_ptr, ws_bytes):
        if dist:
            return enc._lib.pf_encoder_forward_dist(enc._h, x.data_ptr(), B, n_step, outs[0].data_ptr(), outs[1].data_ptr(), ws_ptr, ws_bytes,
                                                    _lib.current_stream())
        return enc._lib.pf_encoder_forward(enc._h, x.data_ptr(), B, n_step, outs[0].data_ptr(), ws_ptr, ws_bytes, _lib.current_stream())
    return nbytes, call, want, outs


def _decoder(dec, z, pnotree):
    z = z.cuda().float().contiguous()
    R = z.shape[0]
    if pnotree:
        pitch, dur, est = dec.decode(z)
        want = [pitch, dur, est.int()]
    else:
        want = list(dec(z, True, 0.0))
    outs = [torch.full_like(w, -7) if w.dtype == torch.int32 else torch.full_like(w, float("nan")) for w in want]
    nbytes = dec._lib.pf_decoder_workspace_bytes(dec._h, R)

    def call(ws_ptr, ws_bytes):
        o2, est = (None, outs[2]) if pnotree else (outs[2], None)
        return dec._lib.pf_decoder_forward(dec._h, z.data_ptr(), R, outs[0].data_ptr(), outs[1].data_ptr(), _lib.ptr(o2), _lib.ptr(est), ws_ptr,
                                           ws_bytes, _lib.current_stream())
    return nbytes, call, want, outs


def _pn_decoder(hd):
    return PianoTreeDecoder(max_simu_note=4, dec_dur_hid_size=hd).load_state_dict(W.synth_pianotree_decoder_state(0, hd))


def _z(rows, width):
    return torch.from_numpy(np.random.Generator(np.random.PCG64(11)).standard_normal((rows, width)).astype(np.float32))


CASES = {
    "chord_encoder_B9_T8": lambda: _encoder(ChordEncoder(36, 512, 512).load_state_dict(W.synth_chord_encoder_state(0)),
                                            torch.from_numpy(synth.chords(9, 1, 8)), 8, False),
    "texture_encoder_B2": lambda: _encoder(TextureEncoder(256, 1024, 256, 10).load_state_dict(W.synth_texture_encoder_state(0)),
                                           torch.from_numpy(synth.prmat(2, 2, 32, 128)), 8, False),
    "pianotree_encoder_B1_S4": lambda: _encoder(PianoTreeEncoder(max_simu_note=4).load_state_dict(W.synth_pianotree_encoder_state(0)),
                                                _pnotree_grid(1, 4), 4, False),
    "chord_encoder_with_scale_B9": lambda: _encoder(ChordEncoder(36, 1024, 256, with_scale=True).load_state_dict(
        W.synth_chord_encoder_state(0, 36, 1024, 256)), torch.from_numpy(synth.chords(9, 3, 8)), 8, True),
    "chord_decoder_R9": lambda: _decoder(ChordDecoder(36, 256, 512, 256, 8).load_state_dict(W.synth_chord_decoder_state(0)), _z(9, 256), False),
    "pianotree_decoder_S4_R9_hd16": lambda: _decoder(_pn_decoder(16), _z(9, 512), True),
    "pianotree_decoder_S4_R9_hd64": lambda: _decoder(_pn_decoder(64), _z(9, 512), True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_forward_stays_inside_the_workspace_it_asked_for(case):
    nbytes, call, want, outs = CASES[case]()
    lib = _lib.load()
    assert nbytes > 0
    buf = torch.empty(nbytes + TAIL, dtype=torch.uint8, device="cuda")
    buf[nbytes:] = PATTERN
    # one byte short: refused, nothing enqueued
    assert call(buf.data_ptr(), nbytes - 1) == PF_EINVAL
    assert "workspace too small" in lib.pf_last_error().decode()
    torch.cuda.synchronize()
    for o in outs:
        assert bool(torch.isnan(o).all()) if o.is_floating_point() else bool((o == -7).all())
    # exactly what was asked for
    assert call(buf.data_ptr(), nbytes) == 0, lib.pf_last_error().decode()
    torch.cuda.synchronize()
    assert bool((buf[nbytes:] == PATTERN).all()), "a launch wrote past the workspace"
    for o, w in zip(outs, want):
        assert o.dtype == w.dtype and np.array_equal(o.cpu().numpy().view(np.uint8), w.cpu().numpy().view(np.uint8))
