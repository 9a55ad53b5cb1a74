"""Polydis on the GPU (``polyffusion_amd.polydis``: the encoders' scale head ``pf_encoder_forward_dist`` and the PianoTree heads at a
64-wide duration GRU) against the reference fixture tests/golden/polydis.npz and, for shapes the fixture does not hold, against the
float64 restatement of tests/test_polydis_host.py (itself pinned to the fixture there).

Tolerances are those of tests/test_gpu_decoders.py: integer grids EXACTLY equal; logits, ``mean`` and ``scale`` within 1e-4 - the
project's encoder tolerance, 10x below the 1e-3 gap the generator enforces on every fixture row, so within it no arg-max can flip -
absolute for logits and ``mean``, relative for ``scale`` (an exponential).  The reference's own float32 noise is printed beside each.
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
import test_polydis_host as P  # noqa: E402
from polyffusion_amd import inference_sdf, midi  # noqa: E402
from polyffusion_amd.model_sdf import ChordEncoder, TextureEncoder  # noqa: E402
from polyffusion_amd.polydis import DisentangleVAE, PtvaeDecoder  # noqa: E402
from polyffusion_amd.weights import synth_pianotree_decoder_state  # noqa: E402

TOL = 1e-4


@pytest.fixture(scope="module")
def g():
    return P.fixture()


@pytest.fixture(scope="module")
def model():
    return DisentangleVAE.init_model().load_state_dict(P.state())


@pytest.fixture(scope="module")
def inputs(g):
    return torch.from_numpy(g["enc_prmat"].astype(np.float32)).cuda(), torch.from_numpy(g["enc_chd"].astype(np.float32)).cuda()


@pytest.fixture(scope="module")
def z_all(g, model):
    """Every fixture z decoded once: ``(pitch, dur, est)`` on the host for the direct rows (shared; never modified)."""
    return tuple(t.cpu() for t in model.decoder.decode(torch.from_numpy(g["z"]).cuda()))


def _err(a, b):
    return (a.double().cpu() - torch.as_tensor(b).double()).abs().max().item()


def test_encoders_mean_and_scale(g, model, inputs):
    pr, c = inputs
    d_chd, d_rhy = model.inference_encode(pr, c)
    noise, noise_rel = float(g["enc_ref_f32_f64"]), float(g["enc_scale_ref_rel_f32_f64"])
    for dist, name in ((d_chd, "chd"), (d_rhy, "rhy")):
        assert dist.mean.is_cuda and tuple(dist.mean.shape) == tuple(dist.scale.shape) == (len(g["enc_rows"]), 256)
        e_m = _err(dist.mean, g[f"{name}_mean_f64"])
        want = torch.from_numpy(g[f"{name}_scale_f64"])
        e_s = ((dist.scale.double().cpu() - want).abs() / want).max().item()
        print(f"{name} encoder vs reference float64: mean {e_m:.3e} abs (reference float32 noise {noise:.2e}), scale {e_s:.3e} rel ({noise_rel:.2e})")
        assert e_m <= TOL and e_s <= TOL
    # an encoder created without the scale head: the same mean, bit for bit
    st = P.state()
    chd0 = ChordEncoder(36, 1024, 256).load_state_dict(P.sub(st, "chd_encoder."))
    rhy0 = TextureEncoder(256, 1024, 256, 10).load_state_dict(P.sub(st, "rhy_encoder."))
    assert torch.equal(chd0.encode_mean(c), d_chd.mean) and torch.equal(rhy0.encode_mean(pr), d_rhy.mean)
    assert torch.equal(model.chd_encoder.encode_mean(c), d_chd.mean)          # and the mean-only entry on the encoder that has the head
    with pytest.raises(RuntimeError, match="created without the scale head"):
        chd0.encode_dist(c)


def test_inference_decode_and_swap_equal_the_fixture(g, model, inputs, z_all):
    pr, c = inputs
    est = model.inference(pr, c, sample=False)
    assert isinstance(est, np.ndarray) and est.dtype == np.int64 and est.shape == (len(g["enc_rows"]), 32, 31, 6)
    assert np.array_equal(est, g["enc_est"])
    z = torch.from_numpy(g["z"]).cuda()
    assert np.array_equal(model.inference_decode(z[:, :256], z[:, 256:]), g["z_est"])
    a, b = torch.from_numpy(g["swap_rows_pr"]).cuda(), torch.from_numpy(g["swap_rows_chd"]).cuda()
    assert np.array_equal(model.swap(pr[a], pr[b], c[a], c[b], fix_rhy=True, fix_chd=False), g["swap_est"])
    assert np.array_equal(model.swap(pr[b], pr[a], c[b], c[a], fix_rhy=False, fix_chd=True), g["swap_est"])
    # logits: the recorded steps of the first encoded row, and every direct row against the float64 restatement
    d_chd, d_rhy = model.inference_encode(pr[:1], c[:1])
    pitch, dur, e0 = model.decoder.decode(torch.cat([d_chd.mean, d_rhy.mean], -1))
    steps = list(g["logit_steps"])
    e_p, e_d = _err(pitch[0, steps], g["logit_pitch"]), _err(dur[0, steps], g["logit_dur"])
    print(f"logits vs reference at steps {steps}: pitch {e_p:.3e} dur {e_d:.3e} (reference float32 noise {float(g['dec_ref_f32_f64']):.2e})")
    assert e_p <= TOL and e_d <= TOL and np.array_equal(e0.cpu().numpy(), g["enc_est"][:1])
    o_p, o_d, _ = P.decode_oracle()["z"]
    e_p, e_d = _err(z_all[0], o_p), _err(z_all[1], o_d)
    print(f"logits vs float64 restatement, direct rows: pitch {e_p:.3e} dur {e_d:.3e}")
    assert e_p <= TOL and e_d <= TOL and torch.equal(z_all[2], H.grid_of(z_all[0], z_all[1]))


def test_wide_duration_gru_at_the_smallest_slot_loop():
    """HD = 64, max_simu_note = 4.  Rows are drawn here and kept only where the float64 restatement clears the 1e-3 gap (on the CPU
    10 of these 16 do, with lengths 1, 2 and 3)."""
    st = synth_pianotree_decoder_state(0, 64)
    z = torch.from_numpy(np.random.Generator(np.random.PCG64(464)).standard_normal((16, 512)).astype(np.float32))
    o_p, o_d, o_len = H.restate_pianotree(st, z, 4)
    ok = torch.nonzero(H.min_margin(o_p, o_d) >= 1e-3).flatten()
    print(f"HD 64, max_simu_note 4: {len(ok)} of 16 rows clear the gap; lengths {sorted(set(o_len[ok].flatten().tolist()))}")
    assert len(ok) >= 2
    ok = ok[:2]
    dec = PtvaeDecoder(max_simu_note=4, dec_dur_hid_size=64).load_state_dict(st)
    pitch, dur, est = dec.decode(z[ok].cuda())
    assert tuple(est.shape) == (2, 32, 3, 6)
    assert torch.equal(est.cpu(), H.grid_of(o_p, o_d)[ok])
    assert _err(pitch, o_p[ok]) <= TOL and _err(dur, o_d[ok]) <= TOL


@pytest.mark.parametrize("rows", [1, 3])
def test_row_counts_off_the_tile(g, model, inputs, z_all, rows):
    """R = 1 and R = 3 (no multiple of the 8-row tile), last fixture rows: the decode, and the encoders with their scale heads."""
    z = torch.from_numpy(g["z"][4 - rows:]).cuda()
    pitch, dur, est = model.decoder.decode(z)
    assert np.array_equal(est.cpu().numpy(), g["z_est"][4 - rows:])
    for a, b in zip((pitch, dur), z_all):
        assert torch.equal(a.cpu(), b[4 - rows:])
    pr, c = inputs
    n = pr.shape[0]
    d_chd, d_rhy = model.inference_encode(pr[n - rows:], c[n - rows:])
    for dist, name in ((d_chd, "chd"), (d_rhy, "rhy")):
        want = torch.from_numpy(g[f"{name}_scale_f64"][n - rows:])
        assert _err(dist.mean, g[f"{name}_mean_f64"][n - rows:]) <= TOL
        assert ((dist.scale.double().cpu() - want).abs() / want).max().item() <= TOL


def test_batch_invariance_and_repeatability(g, model, inputs, z_all):
    z = torch.from_numpy(g["z"]).cuda()
    for a, b in zip(model.decoder.decode(z[:1]), z_all):
        assert torch.equal(a.cpu(), b[:1])                 # row 0 alone is bit-identical to row 0 among four
    for a, b in zip(model.decoder.decode(z), z_all):
        assert torch.equal(a.cpu(), b)                     # two identical calls
    pr, c = inputs
    all4, one, again = model.inference_encode(pr, c), model.inference_encode(pr[:1], c[:1]), model.inference_encode(pr, c)
    for d4, d1, d4b in zip(all4, one, again):
        assert torch.equal(d4.mean[:1], d1.mean) and torch.equal(d4.scale[:1], d1.scale)
        assert torch.equal(d4.mean, d4b.mean) and torch.equal(d4.scale, d4b.scale)


def test_seeded_draws(g, model, inputs):
    pr, c = inputs
    R = pr.shape[0]
    d_chd, d_rhy = model.inference_encode(pr, c)
    gen = lambda: torch.Generator().manual_seed(77)
    draw = lambda gg: torch.randn((R, 256), generator=gg, dtype=torch.float32).cuda()
    # chd_sample: z_chd ~ N(0, 1) from the generator, z_rhy untouched (the encoder mean)
    got = model.inference(pr, c, sample=False, chd_sample=True, generator=gen())
    assert np.array_equal(got, model.inference_decode(draw(gen()), d_rhy.mean))
    assert np.array_equal(got, model.inference(pr, c, sample=False, chd_sample=True, generator=gen()))
    assert not np.array_equal(got, model.inference(pr, c, sample=False))
    # posterior_sample: mean + scale * randn, z_chd drawn first
    g2 = gen()
    z_chd, z_rhy = d_chd.mean + d_chd.scale * draw(g2), d_rhy.mean + d_rhy.scale * draw(g2)
    got = model.posterior_sample(pr, c, generator=gen())
    assert np.array_equal(got, model.inference_decode(z_chd, z_rhy))
    assert np.array_equal(got, model.posterior_sample(pr, c, generator=gen()))
    # scale = 0 collapses the posterior onto its mean; sample_txt=False keeps the texture mean
    assert np.array_equal(model.posterior_sample(pr, c, scale=0.0, generator=gen()), g["enc_est"])
    assert np.array_equal(model.posterior_sample(pr, c, sample_txt=False, generator=gen()), model.inference_decode(z_chd, d_rhy.mean))
    # prior_sample with both posteriors replaced by N(0, scale) at scale 0 decodes z = 0
    zero = torch.zeros(R, 256).cuda()
    assert np.array_equal(model.prior_sample(pr, c, True, True, scale=0.0, generator=gen()), model.inference_decode(zero, zero))
    # a device generator works too, and is repeatable
    dg = lambda: torch.Generator(device="cuda").manual_seed(5)
    assert np.array_equal(model.posterior_sample(pr, c, generator=dg()), model.posterior_sample(pr, c, generator=dg()))


def test_cli_polydis_flags(tmp_path):
    """The small chord model of test_gpu_checkpoint_cli on synthetic weights and conditions: --polydis writes two parsable files,
    --polydis_recon writes <stamp>_recon.mid, and the generated .npy is bit-identical to the run without the flags."""
    params = dict(model_name="small_chd", in_channels=2, out_channels=2, channels=32, attention_levels=[1], n_res_blocks=1,
                  channel_multipliers=[1, 2], n_heads=2, tf_layers=1, d_cond=32, linear_start=0.00085, linear_end=0.012, n_steps=1000,
                  latent_scaling_factor=0.18215, img_h=128, img_w=128, cond_type="chord", cond_mode="mix", use_enc=True,
                  chd_n_step=32, chd_input_dim=36, chd_z_input_dim=32, chd_hidden_dim=64, chd_z_dim=32)
    (tmp_path / "params.yaml").write_text(yaml.safe_dump(params))
    outs = []
    for name, extra in (("with", ["--polydis", "--polydis_recon"]), ("without", [])):
        out = tmp_path / name
        argv = ["--custom_params_path", str(tmp_path / "params.yaml"), "--synthetic_weights", "--synthetic", "--length", "1", "--ddim",
                "--ddim_steps", "2", "--seed", "9", "--output_dir", str(out)] + extra
        assert inference_sdf.main(argv) == 0
        outs.append(out)
    files = sorted(os.listdir(outs[0]))
    recon = [f for f in files if f.endswith("_recon.mid")]
    assert len(recon) == 1 and "polydis_prmat.mid" in files and "polydis_gen.mid" in files
    assert not [f for f in os.listdir(outs[1]) if "polydis" in f or f.endswith("_recon.mid")]
    assert recon[0][:-len("_recon.mid")] + ".mid" in files                   # next to the song it reconstructs, which stays
    for f in ("polydis_prmat.mid", "polydis_gen.mid", recon[0]):
        tracks, lyrics, division, _tempo = midi.read_smf(str(outs[0] / f))
        assert len(tracks) == 1 and division == midi.RESOLUTION and lyrics == []
        assert all(0 <= p <= 127 and 0 <= s < e <= 4 * 4 * 440 for p, s, e in tracks[0])      # 4 two-bar rows of 4 s
    assert len(midi.read_smf(str(outs[0] / "polydis_prmat.mid"))[0][0]) > 0
    npy = [sorted(f for f in os.listdir(o) if f.endswith(".npy")) for o in outs]
    assert len(npy[0]) == 1 and len(npy[1]) == 1          # (the names carry a time stamp: they need not match)
    assert np.array_equal(np.load(outs[0] / npy[0][0]), np.load(outs[1] / npy[1][0]))
