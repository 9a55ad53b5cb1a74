"""Polydis (``polyffusion_amd.polydis``) without a GPU: a plain-torch float64 RESTATEMENT of ``DisentangleVAE.inference`` /
``inference_decode`` / ``swap`` (the two encoders restated here, the decoder by ``test_decoders_host.restate_pianotree``) pinned against
tests/golden/polydis.npz - what tools/make_goldens_polydis.py recorded from the reference's own ``polydis.model.DisentangleVAE`` - plus
the handles' parameter tables, packing messages, launch accounting, the two MIDI writers and the Python / CLI surface.
tests/test_gpu_polydis.py uses the restatement as its oracle for the shapes the fixture does not hold.

Grids must be exactly equal; ``mean`` and ``scale`` are compared with the reference's float64 run, to 1e-9.
"""
import functools
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_decoders_host as H  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "polydis.npz")
# sha256 over (key, dtype, shape, bytes) of synth_pianotree_decoder_state(0) before it took the duration width: committed fixtures
# (decoders.npz) were recorded from exactly these tensors
PN_DEC_STATE_SHA256 = "8ce729dbeb4ffc082130b241488306f042054a56f76ab7256be7b6e8b54b2696"


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def state():
    from polyffusion_amd.weights import synth_polydis_state
    return synth_polydis_state(int(fixture()["seed_w"]))


def sub(st, prefix):
    return {k[len(prefix):]: v for k, v in st.items() if k.startswith(prefix)}


# ------------------------------------------------------------------------------------------------ restatement (plain torch)
def _bigru_final(seq, w):
    """Final hidden state of each direction of a bidirectional GRU over ``seq`` [R,T,in] -> [R, 2H]."""
    R, T, _ = seq.shape
    hf = hb = torch.zeros(R, w["gru.weight_hh_l0"].shape[1], dtype=seq.dtype)
    for t in range(T):
        hf = H._gru_cell(seq[:, t], hf, w, "gru")
        hb = H._gru_cell(seq[:, T - 1 - t], hb, w, "gru", "_reverse")
    return torch.cat([hf, hb], -1)


def restate_chd_encoder(st, c, dtype=torch.float64):
    """polydis/ptvae.py RnnEncoder: ``(mean, scale)`` of chords [R,8,36]."""
    w = H._t(st, dtype)
    h = _bigru_final(torch.as_tensor(c).to(dtype), w)
    return H._lin(h, w, "linear_mu"), H._lin(h, w, "linear_var").exp()


def restate_rhy_encoder(st, pr, dtype=torch.float64):
    """polydis/ptvae.py TextureEncoder: ``(mean, scale)`` of a texture [R,32,128]."""
    w = H._t(st, dtype)
    pr = torch.as_tensor(pr).to(dtype)
    x = torch.nn.functional.conv2d(pr[:, None], w["cnn.0.weight"], w["cnn.0.bias"], stride=(4, 1))
    x = torch.nn.functional.max_pool2d(torch.relu(x), (1, 4), (1, 4)).reshape(pr.shape[0], 8, -1)
    h = _bigru_final(H._lin(H._lin(x, w, "fc1"), w, "fc2"), w)
    return H._lin(h, w, "linear_mu"), H._lin(h, w, "linear_var").exp()


@functools.lru_cache(maxsize=None)
def encoder_oracle():
    """``(chd_mean, chd_scale, rhy_mean, rhy_scale)`` in float64 on the fixture's encoded rows (computed once, shared)."""
    g, st = fixture(), state()
    return (restate_chd_encoder(sub(st, "chd_encoder."), g["enc_chd"].astype(np.float32)) +
            restate_rhy_encoder(sub(st, "rhy_encoder."), g["enc_prmat"].astype(np.float32)))


@functools.lru_cache(maxsize=None)
def decode_oracle():
    """One float64 decode of every z the fixture pins: the encoded rows (``inference``), the swap pairs and the direct rows.
    -> dict of ``(pitch, dur, lengths)`` slices."""
    g = fixture()
    mc, _, mr, _ = encoder_oracle()
    a, b = g["swap_rows_pr"], g["swap_rows_chd"]
    z = torch.cat([torch.cat([mc, mr], -1), torch.cat([mc[b], mr[a]], -1), torch.from_numpy(g["z"]).double()])
    p, d, lens = H.restate_pianotree(sub(state(), "decoder."), z, int(g["max_simu_note"]))
    n, s = len(mc), len(a)
    cut = lambda lo, hi: (p[lo:hi], d[lo:hi], lens[lo:hi])
    return {"enc": cut(0, n), "swap": cut(n, n + s), "z": cut(n + s, len(z))}


def _recorded_table(g):
    return [(str(n), tuple(int(v) for v in s if v)) for n, s in zip(g["param_names"], g["param_shapes"])]


def _state_hash(st):
    m = hashlib.sha256()
    for k, v in st.items():
        m.update(k.encode()); m.update(str(v.dtype).encode()); m.update(str(v.shape).encode()); m.update(v.tobytes())
    return m.hexdigest()


# ------------------------------------------------------------------------------------------------ tests
def test_fixture_rows_clear_the_gap():
    g = fixture()
    n = len(g["enc_rows"])
    assert 2 <= n <= 4 and len(g["z_rows"]) == 4 and int(g["max_simu_note"]) == 32
    assert g["enc_est"].shape == (n, 32, 31, 6) and g["z_est"].shape == (4, 32, 31, 6) and g["swap_est"].shape == (2, 32, 31, 6)
    assert g["logit_pitch"].shape == (3, 31, 130) and g["logit_dur"].shape == (3, 31, 5, 2) and list(g["logit_steps"]) == [0, 15, 31]
    assert float(g["min_gap"]) == 1e-3
    assert min(float(g["enc_min_margin"]), float(g["swap_min_margin"]), float(g["z_min_margin"])) >= 1e-3
    assert float(g["enc_ref_f32_f64"]) < 1e-5 and float(g["dec_ref_f32_f64"]) < 1e-5
    assert len(set(g["enc_lengths"].flatten().tolist()) | set(g["z_lengths"].flatten().tolist())) >= 2
    for name in ("chd_mean", "rhy_mean"):          # the documented gain: encoded means of rms in [0.5, 2]
        assert 0.5 <= float(np.sqrt((g[name + "_f64"] ** 2).mean())) <= 2.0
    assert os.path.getsize(GOLDEN) <= 981751 // 2
    # every row of the restatement clears the gap too (recomputed, not only recorded)
    for key, (p, d, _) in decode_oracle().items():
        assert float(H.min_margin(p, d).min()) >= 1e-3, key


def test_restatement_equals_the_reference_fixture():
    g = fixture()
    for got, name in zip(encoder_oracle(), ("chd_mean", "chd_scale", "rhy_mean", "rhy_scale")):
        e = (got - torch.from_numpy(g[name + "_f64"])).abs().max().item()
        print(f"restatement vs reference float64 {name}: {e:.3e}")
        assert e <= 1e-9
    o = decode_oracle()
    for key, est, lens in (("enc", "enc_est", "enc_lengths"), ("swap", "swap_est", None), ("z", "z_est", "z_lengths")):
        p, d, ln = o[key]
        assert torch.equal(H.grid_of(p, d), torch.from_numpy(g[est]).long()), key
        if lens:
            assert torch.equal(ln, torch.from_numpy(g[lens]).long())
    steps = list(g["logit_steps"])
    e_p = (o["enc"][0][0, steps] - torch.from_numpy(g["logit_pitch"]).double()).abs().max().item()
    e_d = (o["enc"][1][0, steps] - torch.from_numpy(g["logit_dur"]).double()).abs().max().item()
    print(f"restatement vs reference float32 logits at steps {steps}: pitch {e_p:.3e} dur {e_d:.3e}")
    assert e_p <= 1e-5 and e_d <= 1e-5          # the reference's own float32 noise (recorded: about 1e-6)


def test_handles_build_without_gpu_and_carry_the_reference_tables():
    from polyffusion_amd.arch import pianotree_decoder_param_shapes, polydis_param_shapes
    from polyffusion_amd.model_sdf import ChordEncoder, TextureEncoder
    from polyffusion_amd.polydis import DisentangleVAE, PtvaeDecoder
    g = fixture()
    table = _recorded_table(g)
    assert table == [(k, tuple(s)) for k, s in polydis_param_shapes().items()]
    assert table == [(k, tuple(v.shape)) for k, v in state().items()]
    m = DisentangleVAE.init_model()
    assert m.num_step == 32 and m.decoder.max_simu_note == 32 and m.decoder.dec_dur_hid_size == 64
    dec_table = [(k[len("decoder."):], s) for k, s in table if k.startswith("decoder.")]
    assert list(m.decoder.param_shapes().items()) == dec_table == list(pianotree_decoder_param_shapes(dec_dur_hid_size=64).items())
    assert [("chd_decoder." + k, tuple(s)) for k, s in m.chd_decoder_shapes.items()] == [t for t in table if t[0].startswith("chd_decoder.")]
    blobs = m.pack_state_dict(state())
    assert set(blobs) == {"chd_encoder", "rhy_encoder", "decoder"} and all(float(b.abs().sum()) > 0 for b in blobs.values())
    # PtvaeDecoder's defaults; the 16-wide decoder's blob and table do not change with the new argument
    pt = PtvaeDecoder()
    assert pt.max_simu_note == 32 and pt.dec_dur_hid_size == 16
    assert list(pt.param_shapes().items()) == list(pianotree_decoder_param_shapes().items())
    assert m.decoder.weight_bytes() > pt.weight_bytes()
    # an encoder created the existing way keeps its blob size and layout; linear_var.* is appended only when asked for
    for mk, st in ((lambda **kw: ChordEncoder(36, 1024, 256, **kw), sub(state(), "chd_encoder.")),
                   (lambda **kw: TextureEncoder(256, 1024, 256, 10, **kw), sub(state(), "rhy_encoder."))):
        plain, dist = mk(), mk(with_scale=True)
        assert dist.weight_bytes() == plain.weight_bytes() + 4 * (256 * 2048 + 256)
        b0, b1 = plain.pack_state_dict(st), dist.pack_state_dict(st)
        assert torch.equal(b0, b1[:b0.numel()])
        assert torch.equal(b1[b0.numel():b0.numel() + 256 * 2048], torch.from_numpy(st["linear_var.weight"]).flatten())
        no_var = {k: v for k, v in st.items() if not k.startswith("linear_var.")}
        plain.pack_state_dict(no_var)                                    # optional without the scale head ...
        with pytest.raises(RuntimeError, match=r"missing key\(s\), first: linear_var.weight"):
            mk(with_scale=True).pack_state_dict(no_var)                  # ... required with it (a fresh handle: it remembers what it packed)


def test_dist_entry_refuses_encoders_without_scale():
    import ctypes as C
    from polyffusion_amd import _lib
    from polyffusion_amd.model_sdf import ChordEncoder, PianoTreeEncoder
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    lib = _lib.load()
    for enc, msg in ((ChordEncoder(36, 64, 32), "created without the scale head"), (PianoTreeEncoder(), "PianoTree encoder has no scale head")):
        rc = lib.pf_encoder_forward_dist(enc._h, p, 1, 8, p, p, p, 256, None)
        assert rc < 0 and msg in lib.pf_last_error().decode()
    h = C.c_void_p()
    assert lib.pf_encoder_create_dist(2, 135, 128, 512, 512, 256, 1, C.byref(h)) < 0 and "chord and texture encoders only" in lib.pf_last_error().decode()


def test_pack_messages():
    from polyffusion_amd.polydis import DisentangleVAE
    st = state()
    fresh = DisentangleVAE.init_model          # a handle remembers what it packed: every case gets its own model
    m = fresh()
    want = m.pack_state_dict(st)
    got = m.pack_state_dict({"module." + k: v for k, v in st.items()})           # DataParallel checkpoints: the prefix is stripped
    assert all(torch.equal(want[k], got[k]) for k in want)
    for key in ("decoder.dur_sos_token", "chd_encoder.linear_var.bias", "rhy_encoder.fc1.weight", "chd_decoder.init_input"):
        bad = dict(st); del bad[key]
        part, rest = key.split(".", 1)
        with pytest.raises(RuntimeError, match=part + r": load_state_dict: 1 missing key\(s\), first: " + rest.replace(".", r"\.") + "$"):
            fresh().pack_state_dict(bad)
    for key in ("pt_encoder.linear_mu.weight", "decoder.enc_notes_gru.weight_ih_l0", "chd_decoder.extra.weight", "name"):
        bad = dict(st); bad[key] = np.zeros((2, 2), np.float32)
        with pytest.raises(RuntimeError, match="unexpected key"):
            fresh().pack_state_dict(bad)
    bad = dict(st); bad["decoder.dur_out_linear.weight"] = np.zeros((2, 16), np.float32)
    with pytest.raises(RuntimeError, match=r"^decoder: .*size mismatch for 'dur_out_linear.weight': expected \[2,64,\] got \[2,16,\]"):
        fresh().pack_state_dict(bad)
    bad = dict(st); bad["chd_decoder.root_out.bias"] = np.zeros(13, np.float32)
    with pytest.raises(RuntimeError, match=r"^chd_decoder: .*size mismatch for 'root_out.bias': expected \[12,\] got \[13,\]"):
        fresh().pack_state_dict(bad)
    bad = dict(st); bad["rhy_encoder.linear_var.bias"] = np.zeros(255, np.float32)
    with pytest.raises(RuntimeError, match=r"^rhy_encoder: .*size mismatch for 'linear_var.bias': expected \[256,\] got \[255,\]"):
        fresh().pack_state_dict(bad)


def test_duration_width_32_is_refused():
    from polyffusion_amd import _lib
    from polyffusion_amd.decoders import PianoTreeDecoder
    from polyffusion_amd.polydis import PtvaeDecoder
    import ctypes as C
    for cls in (PianoTreeDecoder, PtvaeDecoder):
        with pytest.raises(ValueError, match="dec_dur_hid_size must be 16 or 64"):
            cls(dec_dur_hid_size=32)
    lib, h = _lib.load(), C.c_void_p()
    assert lib.pf_decoder_create(1, 32, 0, 0, 32, 0, 0, C.byref(h)) < 0 and "must be 16 or 64" in lib.pf_last_error().decode()
    for hd in (0, 16, 64):
        assert lib.pf_decoder_create(1, 32, 0, 0, hd, 0, 0, C.byref(h)) == 0
        lib.pf_decoder_destroy(h)


def test_synth_pianotree_decoder_state_is_unchanged():
    from polyffusion_amd.weights import synth_pianotree_decoder_state
    d = H.fixture()
    st = synth_pianotree_decoder_state(0)
    assert [(k, tuple(v.shape)) for k, v in st.items()] == H._recorded_table(d, "pn")
    assert _state_hash(st) == PN_DEC_STATE_SHA256
    st16, st64 = synth_pianotree_decoder_state(0, 16), synth_pianotree_decoder_state(0, 64)
    for key in ("dec_dur_gru.weight_hh_l0", "dur_hid_linear.weight"):
        assert np.array_equal(st[key], st16[key]) and st64[key].shape[0] == 4 * st[key].shape[0]
    for key in ("dec_time_gru.weight_hh_l0", "pitch_out_linear.bias"):              # the width touches the duration tensors only
        assert np.array_equal(st[key], st64[key])
    assert np.abs(st64["dec_dur_gru.weight_hh_l0"]).max() <= 1 / 8


def test_launch_counts_at_32_slots():
    from polyffusion_amd.polydis import PtvaeDecoder
    for hd in (16, 64):
        dec = PtvaeDecoder(dec_dur_hid_size=hd)
        n = dec.n_launches(1)
        assert n == 2114                                      # 3 + 32 (3 + 2 * 31) + 31
        assert [dec.n_launches(r) for r in (1, 8, 64)] == [n] * 3 and 32 * 31 <= n <= 32 * (31 * 3 + 7) + 8
    assert PtvaeDecoder(dec_dur_hid_size=64).n_launches(1) == PtvaeDecoder().n_launches(1)       # the count does not depend on the width


def test_midi_writers_reproduce_the_reference_note_lists(tmp_path):
    from polyffusion_amd import midi
    g = fixture()
    tick = lambda v: int(round(v * midi.TICKS_PER_SECOND))
    # synthetic textures hold overlapping notes of one pitch, whose note-offs a reader may pair either way: compare the note-on and the
    # note-off events as multisets
    ons = lambda notes: sorted((int(p), s) for p, s, _ in notes)
    offs = lambda notes: sorted((int(p), e) for p, _, e in notes)
    ref = lambda want: [(p, tick(s), tick(e)) for p, s, e, _ in want]
    prmat = g["enc_prmat"].astype(np.int64)
    want = g["prmat_notes"]
    assert len(want) > 0 and set(want[:, 3]) == {80.0}
    assert midi.prmat_note_list(prmat) == [(int(p), float(s), float(e)) for p, s, e, _ in want]
    path = str(tmp_path / "prmat.mid")
    midi.prmat_to_midi_file(torch.from_numpy(prmat), path, labels=["a", "b"])
    tracks, lyrics, division, _ = midi.read_smf(path)
    assert len(tracks) == 1 and division == midi.RESOLUTION and lyrics == [("a", 0.0), ("b", 4.0)]
    assert ons(tracks[0]) == ons(ref(want)) and offs(tracks[0]) == offs(ref(want))
    # reconstruct's writer: estx_to_midi_file on the grid inference returns
    want = g["recon_notes"]
    path = str(tmp_path / "recon.mid")
    midi.estx_to_midi_file(g["enc_est"].astype(np.int64), path)
    tracks, lyrics, _, _ = midi.read_smf(path)
    assert len(want) > 0 and lyrics == [] and ons(tracks[0]) == ons(ref(want)) and offs(tracks[0]) == offs(ref(want))
    # a duration past the end of its bar group is clipped; truncation like the reference's int()
    one = np.zeros((2, 32, 128)); one[1, 30, 60] = 5.9
    assert midi.prmat_note_list(one) == [(60, 4 + 30 / 8, 8.0)]


def test_cli_parser_and_python_surface():
    from polyffusion_amd.inference_sdf import make_parser
    from polyffusion_amd.polydis import MODEL_PATH, DisentangleVAE, PolydisAftertouch
    a = make_parser().parse_args([])
    assert (a.polydis, a.polydis_recon, a.polydis_chd_resample, a.polydis_path) == (False, False, False, MODEL_PATH)
    a = make_parser().parse_args(["--polydis", "--polydis_recon", "--polydis_chd_resample", "--polydis_path", "x.pt"])
    assert a.polydis and a.polydis_recon and a.polydis_chd_resample and a.polydis_path == "x.pt"
    m = DisentangleVAE.init_model()
    for fn, args in ((m.run, (None,) * 6), (m.loss, (None,) * 4), (m.loss_function, ()), (m.chord_loss, ()), (m.kl_loss, ()), (m.confuse_prmat, (None,))):
        with pytest.raises(NotImplementedError, match="training"):
            fn(*args)
    with pytest.raises(RuntimeError, match="no Polydis checkpoint"):
        PolydisAftertouch(model_path="/nonexistent/model.pt")
    # the host-side paths of interp: end points, norms interpolated log-linearly
    z1, z2 = np.array([3.0, 0.0, 0.0], np.float32), np.array([0.0, 12.0, 0.0], np.float32)
    path = m.interp_path(z1, z2, 5)
    assert tuple(path.shape) == (5, 3) and torch.allclose(path[0], torch.from_numpy(z1), atol=1e-6) and torch.allclose(path[-1], torch.from_numpy(z2), atol=1e-5)
    assert torch.allclose(path.norm(dim=1), torch.tensor([3.0, 3 * 2 ** 0.5, 6.0, 6 * 2 ** 0.5, 12.0]), atol=1e-4)
    assert tuple(m.interp_z(torch.ones(2, 4), torch.arange(8.0).reshape(2, 4) + 1, 3).shape) == (2, 3, 4)
    assert m.gt_sample(torch.zeros(2, 32, 5, 6)).shape == (2, 32, 4, 6)
