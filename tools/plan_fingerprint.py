"""Fingerprint of the host-side plans of pf_unet, pf_ddpm, pf_encoder and pf_decoder, from the C ABI alone; needs no GPU.

A dry-run plan touches no device (the CU count falls back to the MI355X's 256), so the document computed on a CPU-only machine describes
what the GPU runs: per model the parameter table (count, a sha256 over its `key:shape` rows IN ORDER, blob size), the sha256 of the blob
packed from the synthetic state (seed 0) for the models whose blob is small enough, and per batch / precision / n_cond / plan option /
telemetry binding the workspace sizes and launch counts (pf_ddpm: workspace, launches, operations).  The encoders and decoders keep
what a refactor of their host code must not move under "table" (blob size, the decoders' parameter table, the packed blob, the decoders'
launch counts) and their workspace sizes, which may move by rounding, under "workspace".  Both builds of the library.

    python tools/plan_fingerprint.py            # print the document
    python tools/plan_fingerprint.py --check    # compare with tests/golden/plan_fingerprint.json (exit 1 and the differing keys on a mismatch)
    python tools/plan_fingerprint.py --write    # regenerate that file: only for a change that alters a plan ON PURPOSE

tests/test_plan_fingerprint.py holds a refactor of the plan code to this file."""
from __future__ import annotations

import ctypes as C
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from polyffusion_amd import _lib  # noqa: E402
from polyffusion_amd.arch import UNetConfig  # noqa: E402
from polyffusion_amd.ddpm import DDPMConfig, DDPMUNet  # noqa: E402
from polyffusion_amd._handle import ModelHandle  # noqa: E402
from polyffusion_amd.params import preset  # noqa: E402
from polyffusion_amd.unet import UNetModel  # noqa: E402
from polyffusion_amd import weights as W  # noqa: E402
from polyffusion_amd.weights import synth_ddpm_state, synth_unet_state  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden", "plan_fingerprint.json")
BATCHES = (1, 2, 8, 16, 32)
PRECISIONS = (("f32", 0), ("split", 1))   # PF_PREC_F32, PF_PREC_BF16X3
UNET_SMALL = UNetConfig(channels=32, n_res_blocks=1, attention_levels=(1,), channel_multipliers=(1, 2), n_heads=2, d_cond=32)   # tests/test_cpu_host.py
DDPM_SMALL = DDPMConfig(image_channels=2, n_channels=32, ch_mults=(1, 2), is_attn=(False, True), n_blocks=2, img_h=32, img_w=32)   # tests/test_ddpm_host.py
# (name, config, image side, hash the packed blob)
UNETS = (("sdf_chd8bar", None, 128, True), ("sdf_txt", None, 128, False), ("sdf_concat", None, 128, False), ("unet_small", UNET_SMALL, 32, True))
DDPMS = (("ddpm", DDPMConfig(), False), ("ddpm_small", DDPM_SMALL, True))   # the default config's blob is over a gigabyte
# (name, create arguments of the C ABI, synthetic state): the encoders at the sizes tests/test_gpu_encoders.py builds, the two Polydis
# encoders (with the scale head), the chord decoder, and the PianoTree decoder at three (max_simu_note, dec_dur_hid_size)
# pf_encoder_create_dist(kind, input_dim, emb_size, hidden_dim, z_dim, num_channel, with_scale)
ENCODERS = (("enc_chord", (0, 36, 0, 512, 512, 0, 0), lambda: W.synth_chord_encoder_state(0)),
            ("enc_texture", (1, 0, 256, 1024, 256, 10, 0), lambda: W.synth_texture_encoder_state(0)),
            ("enc_pnotree", (2, 135, 128, 512, 512, 256, 0), lambda: W.synth_pianotree_encoder_state(0)),
            ("enc_polydis_chord", (0, 36, 0, 1024, 256, 0, 1), lambda: W.synth_chord_encoder_state(0, 36, 1024, 256)),
            ("enc_polydis_texture", (1, 0, 256, 1024, 256, 10, 1), lambda: W.synth_texture_encoder_state(0, 256, 1024, 256, 10)))
# pf_decoder_create(kind, max_simu_note, input_dim, z_input_dim, hidden_dim, z_dim, n_step)
DECODERS = (("dec_chord", (0, 0, 36, 256, 512, 256, 8), lambda: W.synth_chord_decoder_state(0)),) + tuple(
    (f"dec_pnotree_s{s}_hd{hd}", (1, s, 0, 0, hd, 0, 0), lambda hd=hd: W.synth_pianotree_decoder_state(0, hd)) for s, hd in ((20, 16), (32, 64), (4, 16)))
ROWS = (1, 8, 9, 64)   # workspace sizes; the decoders' launch counts at 1, 8 and 64


def _table(model) -> dict:
    rows = "".join(f"{k}:{','.join(map(str, s))}\n" for k, s in model.param_shapes().items())
    return {"n_params": len(model.param_shapes()), "params_sha256": hashlib.sha256(rows.encode()).hexdigest(), "weight_bytes": model.weight_bytes()}


def _blob_sha(model, state) -> str:
    return hashlib.sha256(model.pack_state_dict(state).numpy().tobytes()).hexdigest()


def _unet_plans(lib, h) -> dict:
    """[workspace, workspace_cfg, launches, launches prepared (time, cross) = 00 01 10 11, launches_cfg prepared 11]; cfg: even batches"""
    out = {}
    for pname, prec in PRECISIONS:
        lib.pf_unet_set_precision(h, prec)
        for b in BATCHES:
            for nc in (1, 4):
                even = b % 2 == 0
                out[f"{pname} B{b} nc{nc}"] = (
                    [int(lib.pf_unet_workspace_bytes(h, b, nc)), int(lib.pf_unet_workspace_bytes_cfg(h, b, nc)) if even else 0,
                     int(lib.pf_unet_n_launches(h, b, nc))]
                    + [int(lib.pf_unet_n_launches_prepared(h, b, nc, t, c)) for t in (0, 1) for c in (0, 1)]
                    + [int(lib.pf_unet_n_launches_cfg(h, b, nc, 1, 1)) if even else 0])
    lib.pf_unet_set_precision(h, 0)
    return out


def _unet(lib, variant, name, cfg, side, blob) -> dict:
    cfg = cfg or UNetConfig.from_params(preset(name))
    m = UNetModel(in_channels=cfg.in_channels, out_channels=cfg.out_channels, channels=cfg.channels, n_res_blocks=cfg.n_res_blocks,
                  attention_levels=cfg.attention_levels, channel_multipliers=cfg.channel_multipliers, n_heads=cfg.n_heads,
                  tf_layers=cfg.tf_layers, d_cond=cfg.d_cond, img_h=side, img_w=side, x3=variant)
    r = _table(m)
    if blob:
        r["blob_sha256"] = _blob_sha(m, synth_unet_state(cfg, 0))
    r["plan"] = _unet_plans(lib, m._h)
    for o in range(_lib.OPT_COUNT):
        for v in (0, 1):
            lib.pf_unet_set_option(m._h, o, v)
            r[f"plan opt{o}={v}"] = _unet_plans(lib, m._h)
            lib.pf_unet_set_option(m._h, o, -1)
    word = (C.c_uint32 * 1)()   # telemetry bound: nothing dereferences the word in a dry run
    lib.pf_unet_track_absmax(m._h, C.addressof(word))
    r["plan absmax"] = _unet_plans(lib, m._h)
    lib.pf_unet_track_absmax(m._h, None)
    return r


def _ddpm(lib, variant, cfg, blob) -> dict:
    u = DDPMUNet(cfg, x3=variant)
    r = _table(u)
    if blob:
        r["blob_sha256"] = _blob_sha(u, synth_ddpm_state(cfg, 0))
    r["plan"] = {}
    for pname, prec in PRECISIONS:
        lib.pf_ddpm_set_precision(u._h, prec)
        for b in BATCHES:   # [workspace, launches, operations]
            r["plan"][f"{pname} B{b}"] = [int(lib.pf_ddpm_workspace_bytes(u._h, b)), int(lib.pf_ddpm_n_launches(u._h, b)), int(lib.pf_ddpm_flops(u._h, b))]
    return r


class _Coder(ModelHandle):
    """A pf_encoder / pf_decoder handle in the library of one build (the model classes live in the process's default library)."""

    def __init__(self, lib, prefix, create, args):
        self.PREFIX, self._create = prefix, create
        super().__init__(lib, *args)

    def _fn(self, name: str):
        return super()._fn(self._create if name == "create" else name)


def _coder(lib, args, state, decoder: bool) -> dict:
    m = _Coder(lib, "pf_decoder", "create", args) if decoder else _Coder(lib, "pf_encoder", "create_dist", args)
    t = _table(m) if decoder else {"weight_bytes": m.weight_bytes()}
    t["blob_sha256"] = _blob_sha(m, state())
    if decoder:
        t["launches"] = {f"R{r}": int(lib.pf_decoder_launches(m._h, r)) for r in ROWS if r != 9}
    return {"table": t, "workspace": {f"R{r}": int(m._fn("workspace_bytes")(m._h, r)) for r in ROWS}}


def fingerprint(variant: str = "") -> dict:
    """The document of one build of the library ("" or "f16")."""
    lib = _lib.load(variant)
    doc = {name: _unet(lib, variant, name, cfg, side, blob) for name, cfg, side, blob in UNETS}
    doc.update({name: _ddpm(lib, variant, cfg, blob) for name, cfg, blob in DDPMS})
    doc.update({name: _coder(lib, args, state, False) for name, args, state in ENCODERS})
    doc.update({name: _coder(lib, args, state, True) for name, args, state in DECODERS})
    return doc


def build_key(variant: str) -> str:
    return variant or "default"


def differences(want, got, path="") -> list:
    if isinstance(want, dict) and isinstance(got, dict):
        return [d for k in sorted(set(want) | set(got)) for d in differences(want.get(k), got.get(k), f"{path}/{k}")]
    return [] if want == got else [f"{path}: recorded {want}, computed {got}"]


def dumps(doc: dict) -> str:
    """one line per leaf dict: small diffs, small file"""
    def enc(v, depth):
        if isinstance(v, dict) and depth < 3:
            pad = " " * depth
            return "{\n" + ",\n".join(f"{pad} {json.dumps(k)}: {enc(x, depth + 1)}" for k, x in v.items()) + "\n" + pad + "}"
        return json.dumps(v, separators=(",", ":"))
    return enc(doc, 0) + "\n"


def main(argv) -> int:
    doc = {build_key(v): fingerprint(v) for v in ("", "f16") if os.path.exists(_lib.lib_path(v))}
    if "--write" in argv:
        with open(GOLDEN, "w") as f:
            f.write(dumps(doc))
        return 0
    if "--check" in argv:
        with open(GOLDEN) as f:
            want = json.load(f)
        diff = differences({k: want[k] for k in doc}, doc)
        print("\n".join(diff[:40]) if diff else f"plan fingerprint: equal to {os.path.relpath(GOLDEN, REPO)} ({', '.join(doc)})")
        return 1 if diff else 0
    sys.stdout.write(dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
