"""CPU-side checks of the vanilla DDPM model (-m "not gpu"): the reference key namespace in Python and in the pf_ddpm plan against the
golden's state_dict, weight packing, the parity-folded ConvTranspose packings evaluated in numpy, the schedule tables, the CLI surface,
checkpoint round trips, and the new kernels' register budget."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from polyffusion_amd import _lib
from polyffusion_amd.ddpm import (DDPMConfig, DDPMUNet, ddpm_model_state, ddpm_param_shapes, ddpm_tables, params_from_dir,
                                  state_from_checkpoint)
from polyffusion_amd.weights import synth_ddpm_state

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(REPO, "tests", "golden", "ddpm.npz"))
SMALL = DDPMConfig(image_channels=2, n_channels=32, ch_mults=(1, 2), is_attn=(False, True), n_blocks=2, img_h=32, img_w=32)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from polyffusion_amd.build import build
        build(verbose=False)
    return _lib.load()


def _golden_shapes():
    out = {}
    for k, s in zip(G["keys"], G["key_shapes"]):
        out[str(k)] = tuple(int(v) for v in str(s).split(",") if v)
    return out


def test_param_table_is_the_reference_state_dict(lib):
    ref = _golden_shapes()
    assert len(ref) == 309 and ref.pop("ddpm.beta") == (1000,)
    ref = {k[len("ddpm.eps_model."):]: v for k, v in ref.items()}
    py = ddpm_param_shapes(DDPMConfig())
    assert list(py) == list(ref) and dict(py) == ref
    assert sum(int(np.prod(s)) for s in py.values()) == 167776834
    assert DDPMUNet(DDPMConfig()).param_shapes() == py
    assert DDPMUNet(SMALL).param_shapes() == ddpm_param_shapes(SMALL)


def test_pack_synthetic_state_and_unknown_keys(lib):
    u = DDPMUNet(SMALL)
    st = synth_ddpm_state(SMALL, 0)
    blob = torch.zeros(u.weight_bytes() // 4)
    for k, v in st.items():
        assert u.pack_param(k, v, blob) == 0
    assert u.pack_missing() == (0, "")
    assert u.pack_param("down.0.res.bogus.weight", np.zeros(3, np.float32), blob) == -2     # PF_ENOTFOUND
    assert u.pack_param("down.0.res.conv1.weight", np.zeros((3, 3), np.float32), blob) == -1  # shape mismatch
    assert u.n_launches(2) > 0 and u.flops(2) > 0
    assert lib.pf_ddpm_workspace_bytes(u._h, 2) > 0
    with pytest.raises(RuntimeError):
        u.forward(torch.zeros(2, 2, 32, 32), torch.zeros(2, dtype=torch.int64))   # weights not bound: no fallback


def test_attention_norm_keys_are_required(lib):
    """AttentionBlock.norm is saved by the reference but never applied: its keys are accepted and dropped, yet a state without them
    is refused like any other incomplete one."""
    st = synth_ddpm_state(SMALL, 0)
    norm = [k for k in st if ".attn.norm." in k]
    assert norm
    with pytest.raises(RuntimeError, match=rf"{len(norm)} missing key\(s\), first: {re.escape(norm[0])}"):
        DDPMUNet(SMALL).pack_state_dict({k: v for k, v in st.items() if k not in norm})


def _piece(lib):
    if lib.pf_x3_element() == 0:
        return (lambda u: (u.astype(np.uint32) << 16).view(np.float32)), 1.0
    return (lambda u: u.view(np.float16).astype(np.float32)), 1.0 / 256.0


def _convT_via_fold(x, fold):
    """Evaluate the 4 parity-folded 2x2 convs: fold [Cout][Cin][parity*4 + dy*2 + dx]; tap (dy, dx) of parity (py, px) reads source
    pixel (y - 1 + py + dy, x - 1 + px + dx)."""
    Cin, H, W = x.shape
    xp = np.zeros((Cin, H + 2, W + 2)); xp[:, 1:-1, 1:-1] = x
    out = np.zeros((fold.shape[0], 2 * H, 2 * W))
    for py in range(2):
        for px in range(2):
            acc = np.zeros((fold.shape[0], H, W))
            for dy in range(2):
                for dx in range(2):
                    win = xp[:, py + dy:py + dy + H, px + dx:px + dx + W]
                    acc += np.einsum("oc,chw->ohw", fold[:, :, (py * 2 + px) * 4 + dy * 2 + dx], win)
            out[:, py::2, px::2] = acc
    return out


def test_convT_fold_packings_reproduce_the_transposed_convolution(lib):
    rng = np.random.default_rng(3)
    Cin, Cout, H, W = 32, 64, 5, 6
    w = (rng.standard_normal((Cin, Cout, 4, 4)) * 0.1).astype(np.float32)
    x = rng.standard_normal((Cin, H, W)).astype(np.float32)
    ref = F.conv_transpose2d(torch.from_numpy(x[None]).double(), torch.from_numpy(w).double(), stride=2, padding=1)[0].numpy()
    # fp32 packing [parity][tap][Cin][Cout]: exact
    f32 = np.zeros(lib.pf_convt_weight_floats(Cin, Cout), np.float32)
    assert lib.pf_pack_convt_weight_f32(w.ctypes.data, Cin, Cout, f32.ctypes.data) == 0
    fold = f32.reshape(4, 4, Cin, Cout).transpose(3, 2, 0, 1).reshape(Cout, Cin, 16).astype(np.float64)
    assert np.abs(_convT_via_fold(x.astype(np.float64), fold) - ref).max() < 1e-5
    # split packing: the 16-tap layout of pf_pack_upfold_weight_bf16x3, [tap][Cin/8][plane][Npad][8]
    npad = (Cout + 63) // 64 * 64
    dst = np.zeros(lib.pf_packed_gemm_weight_floats(Cout, Cin, 16) * 2, np.uint16)
    assert lib.pf_pack_convt_weight_bf16x3(w.ctypes.data, Cin, Cout, dst.ctypes.data) == 0
    piece, scale = _piece(lib)
    d = dst.reshape(16, Cin // 8, 2, npad, 8)
    hi = piece(d[:, :, 0, :Cout, :]).astype(np.float64)
    lo = piece(d[:, :, 1, :Cout, :]).astype(np.float64)
    fold3 = ((hi + lo) * scale).transpose(2, 1, 3, 0).reshape(Cout, Cin, 16)   # [tap][k8][n][e] -> [n][k][tap]
    assert np.abs(_convT_via_fold(x.astype(np.float64), fold3) - ref).max() < 1e-4 * np.abs(ref).max()


def test_schedule_tables_are_bit_equal_to_the_reference():
    beta, alpha, alpha_bar = ddpm_tables(1000)
    assert beta.dtype == torch.float32
    for name, t in (("beta", beta), ("alpha", alpha), ("alpha_bar", alpha_bar)):
        assert np.array_equal(t.numpy().view(np.int32), G[name].view(np.int32)), name


def test_cli_parses_the_reference_flags():
    from polyffusion_amd.inference_ddpm import make_parser
    a = make_parser().parse_args(["--model_dir", "m", "--length", "3", "--num_generate", "2", "--output_dir", "o", "--show_progress",
                                  "--chkpt_name", "w.pt", "--seed", "7", "--precision", "f32"])
    assert (a.model_dir, a.length, a.num_generate, a.output_dir, a.show_progress, a.chkpt_name, a.seed, a.precision) == \
        ("m", 3, 2, "o", True, "w.pt", 7, "f32")
    d = make_parser().parse_args([])
    assert (d.length, d.num_generate, d.output_dir, d.chkpt_name, d.synthetic_weights) == (1, 1, "exp", "weights_best.pt", False)


def test_params_come_from_model_dir_or_the_builtin_yaml(tmp_path):
    assert params_from_dir(None)["channel_multipliers"] == [1, 2, 2, 4]
    (tmp_path / "params.yaml").write_text("model_name: ddpm\nn_channels: 32\nchannel_multipliers:\n- 1\n- 2\nis_attention:\n- false\n- true\n")
    p = params_from_dir(str(tmp_path))
    assert DDPMConfig.from_params(p) == DDPMConfig(2, 32, (1, 2), (False, True), 2, 128, 128)


@pytest.mark.parametrize("fmt", [".pt", ".ckpt"])
def test_checkpoint_round_trip(tmp_path, fmt):
    eps = synth_ddpm_state(SMALL, 1)
    full = ddpm_model_state(eps)
    path = str(tmp_path / ("w" + fmt))
    if fmt == ".pt":
        torch.save({"model": full}, path)
    else:
        torch.save({"state_dict": {"model." + k: v for k, v in full.items()}}, path)
    state, beta, _ = state_from_checkpoint(path)
    assert list(state) == list(eps) and torch.equal(beta, ddpm_tables(1000)[0])
    for k in eps:
        assert np.array_equal(state[k].numpy(), eps[k])
    u = DDPMUNet(SMALL)
    u.pack_state_dict(state)          # every key (the never-applied attn.norm ones included) is accepted


def test_new_kernels_have_no_scratch_spills(tmp_path):
    """The DDPM translation units compiled for gfx950 report no private-segment (scratch) use in any kernel."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(REPO, "polyffusion_amd", "csrc", "attention_wide.hip")
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", src, "-o", str(tmp_path / "a.o"),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    sizes = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)
    assert len(sizes) >= 4 and all(int(s) == 0 for s in sizes), out.stderr[-3000:]
