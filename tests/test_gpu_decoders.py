"""The PianoTree and chord decoders on the GPU (``pf_decoder`` of libpfhip.so) against the reference fixture
tests/golden/decoders.npz and, for shapes the fixture does not hold, against the float64 restatement of tests/test_decoders_host.py
(itself pinned to the fixture there).

Tolerances: integer grids must be EXACTLY equal; logits within 1e-4 absolute - the project's encoder tolerance, about 80x the reference's
own float32 noise (recorded in the fixture, ~1e-6) and 10x below the smallest top-1 / top-2 gap of any fixture row (1e-3, enforced by the
generator), so within it no arg-max can flip.
"""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_decoders_host as H  # noqa: E402
from polyffusion_amd import inference_sdf, midi  # noqa: E402
from polyffusion_amd.model_sdf import ChordDecoder, PianoTreeDecoder, Polyffusion_SDF  # noqa: E402
from polyffusion_amd.weights import synth_chord_decoder_state, synth_pianotree_decoder_state  # noqa: E402

TOL = 1e-4


@pytest.fixture(scope="module")
def g():
    return H.fixture()


@pytest.fixture(scope="module")
def pn_dec(g):
    return PianoTreeDecoder(max_simu_note=int(g["max_simu_note"])).load_state_dict(synth_pianotree_decoder_state(int(g["seed_w"])))


@pytest.fixture(scope="module")
def chd_dec(g):
    st = synth_chord_decoder_state(int(g["seed_w"]), int(g["chd_input_dim"]), int(g["chd_z_input_dim"]), int(g["chd_hidden_dim"]), int(g["chd_z_dim"]))
    return ChordDecoder(int(g["chd_input_dim"]), int(g["chd_z_input_dim"]), int(g["chd_hidden_dim"]), int(g["chd_z_dim"]),
                        int(g["chd_n_step"])).load_state_dict(st)


@pytest.fixture(scope="module")
def pn_all(g, pn_dec):
    """The four fixture rows decoded in one call (shared; never modified)."""
    return tuple(t.cpu() for t in pn_dec.decode(torch.from_numpy(g["pn_z"]).cuda()))


def _err(a, b):
    return (a.double() - torch.as_tensor(b).double()).abs().max().item()


def test_pianotree_fixture_rows(g, pn_dec, pn_all):
    pitch, dur, est = pn_all
    assert est.dtype == torch.int64 and tuple(est.shape) == (4, 32, 19, 6)
    assert torch.equal(est, torch.from_numpy(g["pn_est"]).long())
    assert torch.equal(est, H.grid_of(pitch, dur))                       # the device arg-max is the max(-1)[1] of the logits it returns
    rows = g["pn_logit_rows"]
    e_p, e_d = _err(pitch[rows], g["pn_pitch"]), _err(dur[rows], g["pn_dur"])
    print(f"pianotree logits vs reference: pitch {e_p:.3e} dur {e_d:.3e} (reference float32 noise {float(g['pn_ref_f32_f64']):.2e})")
    assert e_p <= TOL and e_d <= TOL
    # the rows without recorded logits: against the float64 restatement (pinned to the fixture on the host)
    o_p, o_d, _ = H.pianotree_oracle()
    e_p, e_d = _err(pitch, o_p), _err(dur, o_d)
    print(f"pianotree logits vs float64 restatement, all rows: pitch {e_p:.3e} dur {e_d:.3e}")
    assert e_p <= TOL and e_d <= TOL
    # the reference call shape
    p2, d2 = pn_dec(torch.from_numpy(g["pn_z"][:1]).cuda(), True, None, None, 0.0, 0.0)
    assert torch.equal(p2.cpu(), pitch[:1]) and torch.equal(d2.cpu(), dur[:1])


def test_chord_fixture_rows(g, chd_dec):
    z = torch.from_numpy(g["chd_z"]).cuda()
    root, chroma, bass = chd_dec(z, inference=True, tfr=0.0)
    assert tuple(root.shape) == (4, 8, 12) and tuple(chroma.shape) == (4, 8, 12, 2) and tuple(bass.shape) == (4, 8, 12)
    for got, name in ((root, "chd_root"), (chroma, "chd_chroma"), (bass, "chd_bass")):
        e = _err(got.cpu(), g[name])
        print(f"chord {name} vs reference: {e:.3e}")
        assert e <= TOL
    out = Polyffusion_SDF(None, "chord", chord_dec=chd_dec)._decode_chord(z)
    assert out.dtype == torch.int64 and torch.equal(out.cpu(), torch.from_numpy(g["chd_decoded"]).long())


def test_decode_pnotree_batches_the_four_segments(g, pn_dec):
    model = Polyffusion_SDF(None, "pnotree", pnotree_dec=pn_dec)
    rows = torch.from_numpy(g["pn_b2_rows"])
    z = torch.from_numpy(g["pn_z"])[rows].reshape(2, 1, 4 * 512).cuda()
    grid = model._decode_pnotree(z)
    assert grid.dtype == torch.int64 and tuple(grid.shape) == (2, 128, 19, 6)
    assert torch.equal(grid.cpu(), torch.from_numpy(g["pn_b2_grid"]).long())
    # B = 1 is one sample (the reference's squeeze() would collapse it)
    one = model._decode_pnotree(z[1:])
    assert tuple(one.shape) == (1, 128, 19, 6) and torch.equal(one, grid[1:])


@pytest.mark.parametrize("rows", [1, 3])
def test_row_counts_off_the_tile(g, pn_dec, chd_dec, rows):
    """R = 1 and R = 3 (no multiple of the 8-row tile of the mat-vec kernels), last fixture rows, against the restatement."""
    o_p, o_d, _ = H.pianotree_oracle()
    pitch, dur, est = pn_dec.decode(torch.from_numpy(g["pn_z"][4 - rows:]).cuda())
    assert torch.equal(est.cpu(), H.grid_of(o_p, o_d)[4 - rows:])
    assert _err(pitch.cpu(), o_p[4 - rows:]) <= TOL and _err(dur.cpu(), o_d[4 - rows:]) <= TOL
    o = H.chord_oracle()
    got = chd_dec(torch.from_numpy(g["chd_z"][4 - rows:]).cuda(), True, 0.0)
    for a, b in zip(got, o):
        assert _err(a.cpu(), b[4 - rows:]) <= TOL
    assert torch.equal(H.chord_grid(*[t.cpu() for t in got]), H.chord_grid(*o)[4 - rows:])


def test_batch_invariance_and_repeatability(g, pn_dec, chd_dec, pn_all):
    z = torch.from_numpy(g["pn_z"]).cuda()
    alone = [t.cpu() for t in pn_dec.decode(z[:1])]
    for a, b in zip(alone, pn_all):
        assert torch.equal(a, b[:1])                   # row 0 alone is bit-identical to row 0 with three others
    again = [t.cpu() for t in pn_dec.decode(z)]
    for a, b in zip(again, pn_all):
        assert torch.equal(a, b)                       # two identical calls
    zc = torch.from_numpy(g["chd_z"]).cuda()
    c4, c1, c4b = chd_dec(zc, True, 0.0), chd_dec(zc[:1], True, 0.0), chd_dec(zc, True, 0.0)
    for a, b, c in zip(c4, c1, c4b):
        assert torch.equal(a[:1], b) and torch.equal(a, c)


def test_smallest_slot_loop_max_simu_note_4():
    """Three note slots per step.  Rows are drawn here and kept only where the float64 restatement clears the 1e-3 gap."""
    st = synth_pianotree_decoder_state(0)
    z = torch.from_numpy(np.random.Generator(np.random.PCG64(404)).standard_normal((16, 512)).astype(np.float32))
    o_p, o_d, o_len = H.restate_pianotree(st, z, 4)
    ok = torch.nonzero(H.min_margin(o_p, o_d) >= 1e-3).flatten()
    print(f"max_simu_note 4: {len(ok)} of 16 rows clear the gap; lengths {sorted(set(o_len[ok].flatten().tolist()))}")
    assert len(ok) >= 2
    ok = ok[:2]
    dec = PianoTreeDecoder(max_simu_note=4).load_state_dict(st)
    pitch, dur, est = dec.decode(z[ok].cuda())
    assert tuple(est.shape) == (2, 32, 3, 6)
    assert torch.equal(est.cpu(), H.grid_of(o_p, o_d)[ok])
    assert _err(pitch.cpu(), o_p[ok]) <= TOL and _err(dur.cpu(), o_d[ok]) <= TOL


def test_chord_decode_is_capturable(g, chd_dec):
    """Captured with torch.cuda.graph and replayed: no synchronisation, allocation or host read on the path."""
    z = torch.from_numpy(g["chd_z"][:2]).cuda()
    eager = [t.clone() for t in chd_dec(z, True, 0.0)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = chd_dec(z, True, 0.0)
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)


def test_cli_writes_pnotree_recon_and_leaves_the_songs_alone(tmp_path):
    """The sdf_pnotree invocation of test_gpu_checkpoint_cli.test_cli_sdf_pnotree_variant: a parsable pnotree_recon.mid appears, and the
    generated .npy is bit-identical to the same run with the reconstruction switched off (it draws no random numbers)."""
    params = dict(model_name="small_pnotree", in_channels=2, out_channels=2, channels=32, attention_levels=[1], n_res_blocks=1,
                  channel_multipliers=[1, 2], n_heads=2, tf_layers=1, d_cond=2048, linear_start=0.00085, linear_end=0.012, n_steps=1000,
                  latent_scaling_factor=0.18215, img_h=128, img_w=128, cond_type="pnotree", cond_mode="mix", use_enc=True,
                  chd_n_step=32, chd_input_dim=36, chd_z_input_dim=32, chd_hidden_dim=64, chd_z_dim=32)
    (tmp_path / "params.yaml").write_text(yaml.safe_dump(params))
    song = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chord_example.mid")
    outs = []
    for name, extra in (("with", []), ("without", ["--no_pnotree_recon"])):
        out = tmp_path / name
        argv = ["--custom_params_path", str(tmp_path / "params.yaml"), "--synthetic_weights", "--from_midi", song, "--length", "2", "--autoreg",
                "--ddim", "--ddim_steps", "4", "--uncond_scale", "2.0", "--seed", "9", "--output_dir", str(out)] + extra
        assert inference_sdf.main(argv) == 0
        outs.append(out)
    recon = outs[0] / "pnotree_recon.mid"
    assert recon.exists() and not (outs[1] / "pnotree_recon.mid").exists()
    tracks, lyrics, division, _tempo = midi.read_smf(str(recon))
    assert len(tracks) == 1 and division == midi.RESOLUTION and lyrics == []
    assert all(0 <= p <= 127 and 0 <= s < e and e - s <= 32 * 55 for p, s, e in tracks[0])     # at most 32 steps of 55 ticks
    npy = [sorted(f for f in os.listdir(o) if f.endswith(".npy")) for o in outs]
    assert len(npy[0]) == 1 and len(npy[1]) == 1          # (the names carry a time stamp: they need not match)
    assert np.array_equal(np.load(outs[0] / npy[0][0]), np.load(outs[1] / npy[1][0]))


def test_pretrained_loaders_and_state_dict_routing(g, pn_all):
    """load_pretrained_pnotree_enc_dec (ref:utils.py:19-45: bare keys, note_embedding.* to both halves), load_pretrained_chd_enc_dec
    (ref:utils.py:48-69: chord_enc. / chord_dec. prefixes, {"model": ...} unwrapped) and the decoder routing of
    Polyffusion_SDF.load_state_dict: each loaded decoder reproduces the fixture, each loaded encoder equals one loaded directly."""
    from types import SimpleNamespace

    from polyffusion_amd import synth
    from polyffusion_amd.model_sdf import (ChordEncoder, PianoTreeEncoder, load_pretrained_chd_enc_dec, load_pretrained_pnotree_enc_dec)
    from polyffusion_amd.weights import synth_chord_encoder_state, synth_pianotree_encoder_state
    enc_st, dec_st = synth_pianotree_encoder_state(0), synth_pianotree_decoder_state(0)
    vae = dict(enc_st)
    vae.update({k: v for k, v in dec_st.items() if not k.startswith("note_embedding.")})     # one shared embedding, as in the checkpoint
    enc, dec = load_pretrained_pnotree_enc_dec(vae, 20)
    z = torch.from_numpy(g["pn_z"]).cuda()
    assert torch.equal(dec.decode(z)[2].cpu(), pn_all[2])
    grid = torch.from_numpy(synth.pnotree(1, 5)).cuda().view(4, 32, 20, 6)
    assert torch.equal(enc.encode_mean(grid), PianoTreeEncoder(max_simu_note=20).load_state_dict(enc_st).encode_mean(grid))
    # chord pair from a full-model checkpoint
    ce_st, cd_st = synth_chord_encoder_state(0, 36, 512, 256), synth_chord_decoder_state(0, 36, 256, 512, 256)
    full = {"chord_enc." + k: v for k, v in ce_st.items()}
    full.update({"chord_dec." + k: v for k, v in cd_st.items()})
    full.update({"pnotree_dec." + k: v for k, v in dec_st.items()})
    full["ldm.alpha"] = np.zeros(3, np.float32)
    c_enc, c_dec = load_pretrained_chd_enc_dec({"model": full}, 36, 256, 512, 256, 8)
    zc = torch.from_numpy(g["chd_z"]).cuda()
    want = torch.from_numpy(g["chd_decoded"]).long()
    assert torch.equal(Polyffusion_SDF(None, "chord", chord_dec=c_dec)._decode_chord(zc).cpu(), want)
    chd = torch.from_numpy(synth.chords(2, 7)).cuda()
    assert torch.equal(c_enc.encode_mean(chd), ChordEncoder(36, 512, 256).load_state_dict(ce_st).encode_mean(chd))
    # Polyffusion_SDF.load_state_dict: decoder keys reach attached decoders, and are dropped without them
    ldm = SimpleNamespace(eps_model=SimpleNamespace(load_state_dict=lambda state: None))
    model = Polyffusion_SDF(ldm, "pnotree", pnotree_dec=PianoTreeDecoder(max_simu_note=20), chord_dec=ChordDecoder(36, 256, 512, 256, 8))
    model.load_state_dict(full)
    assert torch.equal(model._decode_chord(zc).cpu(), want)
    assert torch.equal(model.pnotree_dec.decode(z[:1])[2].cpu(), pn_all[2][:1])
    bare = Polyffusion_SDF(ldm, "pnotree").load_state_dict(full)
    assert bare.pnotree_dec is None and bare.chord_dec is None and bare._decode_chord(zc) is zc
