"""CPU-side checks of the first-stage autoencoder (-m "not gpu"): the new exports, the reference key namespace in Python and in the
pf_autoenc table against the golden's state_dict, weight packing (loss.* dropped, unknown / mis-shaped keys refused), the dry-walk plans
against the launch counts DESIGN.md records, params/autoencoder.yaml, checkpoints, and what LatentDiffusion does with and without it."""
import os
import re

import numpy as np
import pytest
import torch

from polyffusion_amd import _lib
from polyffusion_amd.autoencoder import (Autoencoder, AutoencoderConfig, GaussianDistribution, Polyffusion_Autoencoder,
                                         autoencoder_param_shapes)
from polyffusion_amd.params import AUTOENCODER_PARAMS, load_autoencoder_params
from polyffusion_amd.weights import synth_autoencoder_state

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(REPO, "tests", "golden", "autoencoder.npz"))
SMALL = AutoencoderConfig(in_channels=3, out_channels=3, channels=32, channel_multipliers=(1, 2), n_resnet_blocks=1, z_channels=4,
                          emb_channels=4)
FULL = AutoencoderConfig()


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from polyffusion_amd.build import build
        build(verbose=False)
    return _lib.load()


def test_library_exports_every_autoencoder_symbol_of_the_header(lib):
    hdr = open(os.path.join(REPO, "include", "pfhip.h")).read()
    names = sorted(set(re.findall(r"\b(pf_autoenc_\w+|pf_gaussian_sample)\s*\(", hdr)))
    assert len(names) == 19, names
    for name in names:
        assert hasattr(lib, name), f"{name} declared in pfhip.h but not exported"
        assert name in _lib.SIGNATURES, f"{name} has no prototype in _lib.SIGNATURES"
    assert "int32_t pad_mode;" in hdr and [f for f, _ in _lib.ConvArgs._fields_][-1] == "pad_mode"


def test_param_table_is_the_reference_state_dict(lib):
    ref = {str(k): tuple(int(v) for v in str(s).split(",") if v) for k, s in zip(G["keys"], G["key_shapes"])}
    assert len(ref) == 248
    py = autoencoder_param_shapes(FULL)
    assert list(py) == [str(k) for k in G["keys"]] and dict(py) == ref
    assert Autoencoder(FULL).param_shapes() == py
    assert Autoencoder(SMALL).param_shapes() == autoencoder_param_shapes(SMALL)


def test_pack_state_drops_loss_keys_and_refuses_unknown_or_misshaped_ones(lib):
    u = Autoencoder(SMALL)
    st = dict(synth_autoencoder_state(SMALL, 0))
    st["loss.logvar"] = np.zeros((), np.float32)
    st["loss.discriminator.main.0.weight"] = np.zeros((64, 3, 4, 4), np.float32)
    blob = u.pack_state_dict(st)               # strict: the loss.* keys pass silently
    assert blob.numel() * 4 == u.weight_bytes() and u.pack_missing() == (0, "")
    with pytest.raises(RuntimeError, match=r"unexpected key 'encoder\.bogus\.weight'"):
        Autoencoder(SMALL).pack_state_dict(dict(st, **{"encoder.bogus.weight": np.zeros(3, np.float32)}))
    with pytest.raises(RuntimeError, match=r"size mismatch for 'quant_conv\.weight'"):
        Autoencoder(SMALL).pack_state_dict(dict(st, **{"quant_conv.weight": np.zeros((8, 8), np.float32)}))
    st.pop("post_quant_conv.bias")
    with pytest.raises(RuntimeError, match=r"1 missing key\(s\), first: post_quant_conv\.bias"):
        Autoencoder(SMALL).pack_state_dict(st)
    with pytest.raises(RuntimeError):          # weights not bound: no fallback
        u.decode(torch.zeros(1, 4, 16, 8))


def _design_counts():
    text = open(os.path.join(REPO, "DESIGN.md")).read()
    m = re.search(r"`pf_autoenc` launches[^\n]*?encode (\d+) \(f32\) / (\d+) \(split\), decode (\d+) \(f32\) / (\d+) \(split\)", text)
    assert m, "DESIGN.md does not record the pf_autoenc launch counts"
    return [int(v) for v in m.groups()]


def test_dry_walk_sizes_and_launch_counts(lib):
    u = Autoencoder(FULL)
    ef, es, df, ds = _design_counts()
    for mode, e, d in (("f32", ef, df), ("bf16x3", es, ds)):
        u.set_precision(mode)
        assert u.precision == mode
        enc = [u.encode_workspace_bytes(b, 128, 128) for b in (1, 2, 3, 16)]
        dec = [u.decode_workspace_bytes(b, 16, 16) for b in (1, 2, 3, 16)]
        assert enc[0] > 0 and dec[0] > 0 and enc == sorted(enc) and dec == sorted(dec)
        for b in (1, 16):
            assert u.encode_launches(b, 128, 128) == e and u.decode_launches(b, 16, 16) == d
        assert u.encode_flops(1, 128, 128) > 1e9 and u.decode_flops(1, 16, 16) > u.encode_flops(1, 128, 128)
    with pytest.raises(ValueError):
        u.set_precision("f16x3")
    # shapes the plans cannot run: sides not multiples of 8, a latent that is no multiple of 64 tokens or beyond 1024
    assert u.encode_workspace_bytes(1, 100, 128) == 0 and u.encode_workspace_bytes(1, 24, 24) == 0
    assert u.decode_workspace_bytes(1, 64, 32) == 0 and u.decode_launches(1, 3, 3) == 0
    s = Autoencoder(SMALL)
    assert s.encode_workspace_bytes(3, 32, 16) > 0 and s.decode_workspace_bytes(3, 16, 8) > 0


def test_params_yaml_round_trips_into_the_config(tmp_path):
    import yaml
    assert AutoencoderConfig.from_params(AUTOENCODER_PARAMS) == FULL
    p = dict(AUTOENCODER_PARAMS, batch_size=16, learning_rate=5e-5, disc_start=50001, channels=32, channel_multipliers=[1, 2], n_res_blocks=1)
    path = tmp_path / "params.yaml"
    path.write_text(yaml.safe_dump(p))
    assert AutoencoderConfig.from_params(load_autoencoder_params(str(path))) == SMALL
    p.pop("z_channels")
    path.write_text(yaml.safe_dump(p))
    with pytest.raises(KeyError, match="z_channels"):
        load_autoencoder_params(str(path))


def test_checkpoint_prefix_is_stripped_and_foreign_keys_refused():
    st = {"autoencoder." + k: v for k, v in synth_autoencoder_state(SMALL, 0).items()}
    assert list(Polyffusion_Autoencoder.strip_prefix(st)) == list(autoencoder_param_shapes(SMALL))
    with pytest.raises(RuntimeError, match="unexpected key 'ldm.beta'"):
        Polyffusion_Autoencoder.strip_prefix(dict(st, **{"ldm.beta": 0}))


def test_load_trained_needs_a_gpu_only_to_bind(tmp_path, lib):
    st = {"autoencoder." + k: torch.from_numpy(v) for k, v in synth_autoencoder_state(SMALL, 0).items()}
    st["autoencoder.loss.logvar"] = torch.zeros(())
    torch.save({"model": st}, tmp_path / "weights.pt")
    if torch.cuda.is_available():
        m = Polyffusion_Autoencoder.load_trained(str(tmp_path), SMALL)
        assert m.autoencoder.pack_missing() == (0, "")
    else:
        with pytest.raises(RuntimeError, match="needs an AMD GPU"):
            Polyffusion_Autoencoder.load_trained(str(tmp_path), SMALL)


def test_forward_without_posterior_sample_and_training_loss_raise(lib):
    u = Autoencoder(SMALL)
    with pytest.raises(RuntimeError):
        u.forward(torch.zeros(1, 3, 32, 16), sample_posterior=False)
    with pytest.raises(RuntimeError):
        u(torch.zeros(1, 3, 32, 16), False)
    with pytest.raises(NotImplementedError):
        u.get_loss_dict(None, 0)
    with pytest.raises(NotImplementedError):
        Polyffusion_Autoencoder(u).get_loss_dict(None, 0)


def test_gaussian_distribution_mirrors_the_reference_fields():
    mean, lv = torch.from_numpy(G["small_mean"]), torch.from_numpy(G["small_log_var"])
    d = GaussianDistribution(mean, lv, lib=object())
    assert d.mean is mean and d.log_var is lv and torch.equal(d.std, torch.exp(0.5 * lv)) and d.scale == 1.0


def test_latent_diffusion_without_an_autoencoder_is_unchanged(lib):
    from polyffusion_amd.unet import LatentDiffusion, UNetModel
    unet = UNetModel(in_channels=2, out_channels=2, channels=64, n_res_blocks=1, attention_levels=[1], channel_multipliers=[1, 2], n_heads=4,
                     tf_layers=1, d_cond=128, img_h=32, img_w=32)
    ldm = LatentDiffusion(unet, autoencoder=None)
    assert ldm.first_stage_model is None and ldm.latent_scaling_factor == 0.18215
    x = torch.arange(6.0).reshape(1, 2, 3, 1)
    assert ldm.autoencoder_encode(x) is x and ldm.autoencoder_decode(x) is x
    ae = Autoencoder(SMALL)
    assert LatentDiffusion(unet, ae).first_stage_model is ae
    with pytest.raises(TypeError):
        LatentDiffusion(unet, autoencoder=torch.nn.Identity())
