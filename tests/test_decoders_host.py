"""The PianoTree and chord decoders without a GPU: the ``pf_decoder`` handle's parameter tables, packing messages and launch accounting,
the MIDI writer of the reconstruction, the Python surface, and a plain-torch RESTATEMENT of both decoders (this module, nothing of the
product imported) pinned against tests/golden/decoders.npz - the fixture tools/make_goldens_decoders.py recorded from the reference's
own modules.  tests/test_gpu_decoders.py uses the restatement as its oracle for the shapes the fixture does not hold.

The restatement runs in float64: the fixture's logits are the reference's float32 ones, whose own distance to its float64 run the
generator recorded (about 1e-6), so "logits within 1e-6" pins the float64 oracle to the reference within the reference's own noise.
"""
import functools
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoders.npz")


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(GOLDEN))


# ------------------------------------------------------------------------------------------------ restatement (plain torch)
def _t(state, dtype):
    return {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in state.items()}


def _gru_cell(x, h, w, name, sfx=""):
    gi = x @ w[f"{name}.weight_ih_l0{sfx}"].T + w[f"{name}.bias_ih_l0{sfx}"]
    gh = h @ w[f"{name}.weight_hh_l0{sfx}"].T + w[f"{name}.bias_hh_l0{sfx}"]
    H = h.shape[-1]
    r = torch.sigmoid(gi[..., :H] + gh[..., :H])
    z = torch.sigmoid(gi[..., H:2 * H] + gh[..., H:2 * H])
    n = torch.tanh(gi[..., 2 * H:] + r * gh[..., 2 * H:])
    return (1 - z) * n + z * h


def _lin(x, w, name):
    return x @ w[f"{name}.weight"].T + w[f"{name}.bias"]


def restate_pianotree(state, z, max_simu_note=20, dtype=torch.float64):
    """Greedy PianoTree decode: ``(recon_pitch [R,32,S-1,130], recon_dur [R,32,S-1,5,2], lengths [R,32])`` in ``dtype``."""
    w, S = _t(state, dtype), max_simu_note
    z = torch.as_tensor(z).to(dtype)
    R = z.shape[0]
    one_hot = lambda i, n: torch.nn.functional.one_hot(i, n).to(dtype)
    sos = torch.zeros(135, dtype=dtype)
    sos[128], sos[130:] = 1.0, 2.0
    h_time, z_in = _lin(z, w, "z2dec_hid_linear"), _lin(z, w, "z2dec_in_linear")
    tok_time = w["dec_init_input"].expand(R, -1)
    pitch_out, dur_out, len_out = [], [], []
    for _t_step in range(32):
        h_time = _gru_cell(torch.cat([tok_time, z_in], -1), h_time, w, "dec_time_gru")
        h_notes = _lin(h_time, w, "dec_time_to_notes_hid")
        token = _lin(sos, w, "note_embedding").expand(R, -1)
        notes, lens = [token], torch.zeros(R, dtype=torch.long)
        p_t, d_t = [], []
        for s in range(1, S):
            h_notes = _gru_cell(torch.cat([h_time, token], -1), h_notes, w, "dec_notes_gru")
            pitch = _lin(h_notes, w, "pitch_out_linear")
            h_dur = _lin(torch.cat([h_notes, pitch], -1), w, "dur_hid_linear")
            d_tok, durs = w["dur_sos_token"].expand(R, -1), []
            for _d in range(5):
                h_dur = _gru_cell(d_tok, h_dur, w, "dec_dur_gru")
                durs.append(_lin(h_dur, w, "dur_out_linear"))
                d_tok = one_hot(durs[-1].argmax(-1), 5)
            durs = torch.stack(durs, 1)
            p_idx = pitch.argmax(-1)
            token = _lin(torch.cat([one_hot(p_idx, 130), durs.argmax(-1).to(dtype)], -1), w, "note_embedding")
            notes.append(token)
            lens = torch.where((p_idx == 129) & (lens == 0), torch.full_like(lens, s), lens)
            p_t.append(pitch)
            d_t.append(durs)
        lens = torch.where(lens == 0, torch.full_like(lens, S - 1), lens)
        seq = torch.stack(notes, 1)                      # [R, S, 128]: start token, then the predicted notes
        h_f = h_b = torch.zeros(R, 128, dtype=dtype)
        for i in range(S):                               # final hidden state of each direction at the row's own length
            h_f = torch.where((i < lens)[:, None], _gru_cell(seq[:, i], h_f, w, "dec_notes_emb_gru"), h_f)
        for i in reversed(range(S)):
            h_b = torch.where((i < lens)[:, None], _gru_cell(seq[:, i], h_b, w, "dec_notes_emb_gru", "_reverse"), h_b)
        tok_time = torch.cat([h_f, h_b], -1)
        pitch_out.append(torch.stack(p_t, 1))
        dur_out.append(torch.stack(d_t, 1))
        len_out.append(lens)
    return torch.stack(pitch_out, 1), torch.stack(dur_out, 1), torch.stack(len_out, 1)


def grid_of(pitch, dur):
    return torch.cat([pitch.argmax(-1).unsqueeze(-1), dur.argmax(-1)], -1)


def min_margin(pitch, dur):
    """Smallest top-1 / top-2 gap over every pitch and duration decision of each row."""
    top = torch.topk(pitch, 2, dim=-1).values
    return torch.minimum((top[..., 0] - top[..., 1]).flatten(1).min(1).values, (dur[..., 0] - dur[..., 1]).abs().flatten(1).min(1).values)


def restate_chord(state, z, n_step=8, dtype=torch.float64):
    """Greedy chord decode: ``(root [R,n,12], chroma [R,n,12,2], bass [R,n,12])``."""
    w = _t(state, dtype)
    z = torch.as_tensor(z).to(dtype)
    R = z.shape[0]
    one_hot = lambda i, n: torch.nn.functional.one_hot(i, n).to(dtype)
    h, z_in = _lin(z, w, "z2dec_hid"), _lin(z, w, "z2dec_in")
    token = w["init_input"].expand(R, -1)
    roots, chromas, basses = [], [], []
    for _step in range(n_step):
        h = _gru_cell(torch.cat([token, z_in], -1), h, w, "gru")
        root, chroma, bass = _lin(h, w, "root_out"), _lin(h, w, "chroma_out").view(R, 12, 2), _lin(h, w, "bass_out")
        roots.append(root), chromas.append(chroma), basses.append(bass)
        token = torch.cat([one_hot(root.argmax(-1), 12), chroma.argmax(-1).to(dtype), one_hot(bass.argmax(-1), 12)], -1)
    return torch.stack(roots, 1), torch.stack(chromas, 1), torch.stack(basses, 1)


def chord_grid(root, chroma, bass):
    one_hot = torch.nn.functional.one_hot
    return torch.cat([one_hot(root.argmax(-1), 12), chroma.argmax(-1), one_hot(bass.argmax(-1), 12)], -1)


@functools.lru_cache(maxsize=None)
def pianotree_oracle():
    """The float64 restatement on the four fixture rows (computed once, shared)."""
    from polyffusion_amd.weights import synth_pianotree_decoder_state
    g = fixture()
    return restate_pianotree(synth_pianotree_decoder_state(int(g["seed_w"])), g["pn_z"], int(g["max_simu_note"]))


@functools.lru_cache(maxsize=None)
def chord_oracle():
    from polyffusion_amd.weights import synth_chord_decoder_state
    g = fixture()
    st = synth_chord_decoder_state(int(g["seed_w"]), int(g["chd_input_dim"]), int(g["chd_z_input_dim"]), int(g["chd_hidden_dim"]),
                                   int(g["chd_z_dim"]))
    return restate_chord(st, g["chd_z"], int(g["chd_n_step"]))


def _recorded_table(g, prefix):
    return [(str(n), tuple(int(v) for v in s if v)) for n, s in zip(g[f"{prefix}_param_names"], g[f"{prefix}_param_shapes"])]


# ------------------------------------------------------------------------------------------------ tests
def test_fixture_rows_clear_the_gap_and_vary_in_length():
    g = fixture()
    assert g["pn_est"].shape == (4, 32, 19, 6) and g["pn_pitch"].shape == (2, 32, 19, 130) and g["pn_dur"].shape == (2, 32, 19, 5, 2)
    assert float(g["min_gap"]) == 1e-3 and float(g["pn_min_margin"]) >= 1e-3 and float(g["chd_min_margin"]) >= 1e-3
    assert float(g["pn_ref_f32_f64"]) < 2e-6 and float(g["chd_ref_f32_f64"]) < 2e-6
    lens = set(g["pn_lengths"].flatten().tolist())
    assert len(lens) >= 3 and 19 in lens and min(lens) <= 2


def test_restatement_equals_the_reference_fixture():
    g = fixture()
    pitch, dur, lens = pianotree_oracle()
    assert torch.equal(grid_of(pitch, dur), torch.from_numpy(g["pn_est"]).long())
    assert torch.equal(lens, torch.from_numpy(g["pn_lengths"]).long())
    assert float(min_margin(pitch, dur).min()) >= 1e-3
    rows = g["pn_logit_rows"]
    e_p = (pitch[rows] - torch.from_numpy(g["pn_pitch"]).double()).abs().max().item()
    e_d = (dur[rows] - torch.from_numpy(g["pn_dur"]).double()).abs().max().item()
    print(f"restatement vs reference float32 logits: pitch {e_p:.3e} dur {e_d:.3e}")
    assert e_p <= 1e-6 and e_d <= 1e-6
    root, chroma, bass = chord_oracle()
    for got, name in ((root, "chd_root"), (chroma, "chd_chroma"), (bass, "chd_bass")):
        e = (got - torch.from_numpy(g[name]).double()).abs().max().item()
        print(f"restatement vs reference float32 logits: {name} {e:.3e}")
        assert e <= 1e-6
    assert torch.equal(chord_grid(root, chroma, bass), torch.from_numpy(g["chd_decoded"]).long())


def test_decoder_handles_build_without_gpu_and_carry_the_reference_tables():
    from polyffusion_amd.arch import chord_decoder_param_shapes, pianotree_decoder_param_shapes
    from polyffusion_amd.model_sdf import ChordDecoder, PianoTreeDecoder
    g = fixture()
    pn = PianoTreeDecoder(max_simu_note=20)
    assert list(pn.param_shapes().items()) == _recorded_table(g, "pn") == list(pianotree_decoder_param_shapes().items())
    chd = ChordDecoder(36, 256, 512, 256, 8)
    assert list(chd.param_shapes().items()) == _recorded_table(g, "chd") == list(chord_decoder_param_shapes(36, 256, 512, 256).items())
    assert pn.weight_bytes() > 4 * sum(int(np.prod(s)) for s in pn.param_shapes().values())     # + the bind-time tables
    with pytest.raises(ValueError, match="max_simu_note"):
        PianoTreeDecoder(max_simu_note=33)
    with pytest.raises(RuntimeError, match="input_dim 36"):
        ChordDecoder(35, 256, 512, 256, 8)
    for dec, args in ((pn, (None, False, None, None, 0.5, 0.5)), (chd, (None, False, 0.5))):
        with pytest.raises(NotImplementedError, match="teacher forcing"):
            dec.forward(*args)


def test_decoder_pack_messages():
    from polyffusion_amd.model_sdf import ChordDecoder, PianoTreeDecoder
    from polyffusion_amd.weights import synth_chord_decoder_state, synth_pianotree_decoder_state, synth_pianotree_encoder_state
    st = synth_pianotree_decoder_state(0)
    enc = synth_pianotree_encoder_state(0)
    assert np.array_equal(st["note_embedding.weight"], enc["note_embedding.weight"]) and np.array_equal(st["note_embedding.bias"], enc["note_embedding.bias"])
    assert 0.0 <= st["dec_init_input"].min() and st["dec_init_input"].max() <= 1.0 and st["dec_init_input"].mean() > 0.3
    assert np.abs(st["dec_notes_gru.weight_hh_l0"]).max() <= 1 / 512 ** 0.5
    blob = PianoTreeDecoder(max_simu_note=20).pack_state_dict(st)
    assert float(blob.abs().sum()) > 0
    bad = dict(st); bad["pitch_out_linear.bias"] = np.zeros(128, np.float32)
    with pytest.raises(RuntimeError, match=r"size mismatch for 'pitch_out_linear.bias': expected \[130,\] got \[128,\]"):
        PianoTreeDecoder(max_simu_note=20).pack_state_dict(bad)
    bad = dict(st); bad["enc_notes_gru.weight_ih_l0"] = np.zeros((768, 128), np.float32)
    with pytest.raises(RuntimeError, match="unexpected key"):
        PianoTreeDecoder(max_simu_note=20).pack_state_dict(bad)
    bad = dict(st); del bad["dur_sos_token"]
    with pytest.raises(RuntimeError, match=r"1 missing key\(s\), first: dur_sos_token"):
        PianoTreeDecoder(max_simu_note=20).pack_state_dict(bad)
    cst = synth_chord_decoder_state(0)
    bad = dict(cst); del bad["init_input"]
    with pytest.raises(RuntimeError, match=r"1 missing key\(s\), first: init_input"):
        ChordDecoder(36, 256, 512, 256, 8).pack_state_dict(bad)
    bad = dict(cst); bad["gru.weight_ih_l0"] = np.zeros((1536, 36), np.float32)
    with pytest.raises(RuntimeError, match=r"size mismatch for 'gru.weight_ih_l0': expected \[1536,292,\] got \[1536,36,\]"):
        ChordDecoder(36, 256, 512, 256, 8).pack_state_dict(bad)


def test_launch_counts_respect_the_structural_bound():
    """At most 3 launches per note slot and 2100 per PianoTree decode (32 x (19 x 3 + 7) + setup), at most 3 per step + 4 for the
    chord decoder; computed on the host, the same for every batch size.  Exactly 3 + 32 (3 + 2 (S - 1)) + 31 and 3 + 2 n_step (DESIGN.md
    section 3)."""
    from polyffusion_amd.model_sdf import ChordDecoder, PianoTreeDecoder
    for S in (20, 4, 2):
        pn = PianoTreeDecoder(max_simu_note=S)
        n = pn.n_launches(1)
        assert n == {20: 1346, 4: 322, 2: 194}[S]
        assert [pn.n_launches(r) for r in (1, 8, 64)] == [n] * 3
        assert 32 * (S - 1) <= n <= 32 * ((S - 1) * 3 + 7) + 8
        if S == 20:
            assert n <= 2100
    for n_step in (8, 32):
        chd = ChordDecoder(36, 256, 512, 256, n_step)
        n = chd.n_launches(1)
        assert n == {8: 19, 32: 67}[n_step]
        assert [chd.n_launches(r) for r in (1, 8, 64)] == [n] * 3 and n_step <= n <= 3 * n_step + 4


def test_estx_to_midi_file_reproduces_the_reference_note_list(tmp_path):
    from polyffusion_amd import midi
    g = fixture()
    est = g["pn_est"].astype(np.int64)
    labels = [str(s) for s in g["midi_lyric_text"]]
    want = g["midi_notes"]
    assert len(want) > 0 and set(want[:, 3]) == {80.0}
    got = midi.estx_note_list(est)
    assert [(p, s, e) for p, s, e in got] == [(int(p), float(s), float(e)) for p, s, e, _ in want]
    path = str(tmp_path / "recon.mid")
    midi.estx_to_midi_file(torch.from_numpy(est), path, labels)
    tracks, lyrics, division, tempo = midi.read_smf(path)
    assert len(tracks) == 1 and division == midi.RESOLUTION and midi.VELOCITY == 80
    tick = lambda v: int(round(v * midi.TICKS_PER_SECOND))
    assert sorted(tracks[0]) == sorted((int(p), tick(s), tick(e)) for p, s, e, _ in want)
    assert [t for t, _ in lyrics] == labels and [s for _, s in lyrics] == [float(v) for v in g["midi_lyric_time"]]
    # an end token (129) in the middle of a step does not end the step: the reference writes the valid slots after it too
    grid = np.full((1, 32, 3, 6), 0, np.int64)
    grid[..., 0] = 130
    grid[0, 30] = [[60, 0, 0, 0, 1, 1], [129, 0, 0, 0, 0, 0], [64, 1, 1, 1, 1, 1]]
    assert midi.estx_note_list(grid) == [(60, 30 / 8, 32 / 8), (64, 30 / 8, 32 / 8)]      # durations 4 and 32, clipped to the segment end
    grid[0, 2, 1] = [127, 0, 0, 0, 0, 0]
    assert midi.estx_note_list(grid)[0] == (127, 2 / 8, 3 / 8)


def test_python_surface_without_gpu():
    from polyffusion_amd.checkpoint import split_state_decoders, split_state_full
    from polyffusion_amd.model_sdf import (ChordDecoder, PianoTreeDecoder, PianoTreeEncoder, Polyffusion_SDF, split_pnotree_vae_state)
    from polyffusion_amd.weights import synth_chord_decoder_state, synth_pianotree_decoder_state, synth_pianotree_encoder_state
    dec = PianoTreeDecoder(max_simu_note=20)
    model = Polyffusion_SDF(None, "pnotree", pnotree_dec=dec, chord_dec=ChordDecoder(36, 256, 512, 256, 8))
    assert model.pnotree_dec is dec and model.chord_dec is not None
    z = torch.zeros(2, 256)
    assert Polyffusion_SDF(None, "chord")._decode_chord(z) is z
    # a PianoTree VAE checkpoint holds both halves under bare keys; the embedding is shared
    enc_st, dec_st = synth_pianotree_encoder_state(0), synth_pianotree_decoder_state(0)
    combined = dict(enc_st)
    combined.update({k: v for k, v in dec_st.items() if not k.startswith("note_embedding.")})
    to_enc, to_dec = split_pnotree_vae_state(combined)
    assert set(to_enc) == set(enc_st) and set(to_dec) == set(dec_st)
    assert to_enc["note_embedding.weight"] is to_dec["note_embedding.weight"]
    PianoTreeEncoder(max_simu_note=20).pack_state_dict(to_enc)
    assert torch.equal(PianoTreeDecoder(max_simu_note=20).pack_state_dict(to_dec), PianoTreeDecoder(max_simu_note=20).pack_state_dict(dec_st))
    # a full-model checkpoint: split_state_full keeps its four parts and drops decoder keys of any shape; the new helper returns them
    full = {"ldm.eps_model.x": torch.zeros(1), "pnotree_enc.note_embedding.bias": torch.zeros(128), "ldm.alpha": torch.zeros(3),
            "pnotree_dec.dur_sos_token": torch.zeros(5), "pnotree_dec.anything": torch.zeros(7, 7), "chord_dec.init_input": torch.zeros(36)}
    parts = split_state_full(full)
    assert set(parts) == {"unet", "chord_enc", "txt_enc", "pnotree_enc"}
    assert set(parts["unet"]) == {"x"} and set(parts["pnotree_enc"]) == {"note_embedding.bias"} and not parts["chord_enc"] and not parts["txt_enc"]
    decs = split_state_decoders(full)
    assert set(decs) == {"chord_dec", "pnotree_dec"} and set(decs["pnotree_dec"]) == {"dur_sos_token", "anything"} and set(decs["chord_dec"]) == {"init_input"}
    assert synth_chord_decoder_state(0)["init_input"].shape == (36,)
