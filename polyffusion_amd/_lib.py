"""ctypes binding of libpfhip.so (the C ABI in include/pfhip.h).

There is no fallback: if the shared library is missing or a call fails, a RuntimeError
is raised.  ``load()`` itself needs no GPU (the library dlopens on a CPU-only box, which
the ``-m "not gpu"`` tests use to check the exported symbols); launching needs one.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

HERE = os.path.dirname(os.path.abspath(__file__))
# The library exists in two builds of the same sources (csrc/pf_internal.h): libpfhip.so splits operands into bf16 pieces ("bf16x3"),
# libpfhip_f16.so (`python -m polyffusion_amd.build --variant=f16`) into fp16 pieces ("f16x3": fp32-class error, ~3 % slower, fp16's range).
# load() returns the process default - libpfhip.so unless PF_X3=f16 is set, which makes everything named "bf16x3" run as f16x3 (how the
# whole GPU suite is run against the fp16 build); load("f16") returns the fp16 build explicitly (UNetModel.set_precision("f16x3")).
X3_VARIANT = {"": "", "bf16": "", "f16": "f16"}.get(os.environ.get("PF_X3", ""), None)
if X3_VARIANT is None:
    raise RuntimeError(f"PF_X3={os.environ['PF_X3']!r}: expected 'bf16' (default) or 'f16'")


def lib_path(variant: str = "") -> str:
    return os.path.join(HERE, f"libpfhip_{variant}.so" if variant else "libpfhip.so")


LIB_PATH = lib_path(X3_VARIANT)
X3_WEIGHT_SCALE = 256.0 if X3_VARIANT == "f16" else 1.0     # what the default library's split packing multiplies weights by (PF_X3_WS)


def x3_torch_dtype(variant: Optional[str] = None):
    """Element type of the hi / lo planes the split-precision kernels exchange (tests decode planes with it)."""
    import torch
    return torch.float16 if (X3_VARIANT if variant is None else variant) == "f16" else torch.bfloat16


c_float_p = C.POINTER(C.c_float)
c_i64_p = C.POINTER(C.c_int64)


class UNetCfg(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int32), ("out_channels", C.c_int32), ("channels", C.c_int32), ("n_res_blocks", C.c_int32),
        ("n_attention_levels", C.c_int32), ("attention_levels", C.c_int32 * 8),
        ("n_levels", C.c_int32), ("channel_multipliers", C.c_int32 * 8),
        ("n_heads", C.c_int32), ("tf_layers", C.c_int32), ("d_cond", C.c_int32),
        ("img_h", C.c_int32), ("img_w", C.c_int32),
    ]


class DdpmCoef(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("c_recip", "c_recipm1", "c_x0", "c_xt", "sigma", "sqrt_ab", "sqrt_1mab")]


class DdimCoef(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("s1m", "sqrt_a", "sqrt_aprev", "dir_coef", "sigma", "q_sqrt_a", "q_s1m")]


class DpmCoef(C.Structure):
    """pf_dpm_coef (include/pfhip.h): one DPM-Solver++(2M) step; ``c_1 == 0`` marks a first-order step."""
    _fields_ = [(n, C.c_float) for n in ("s1m", "sqrt_a", "c_x", "c_0", "c_1", "q_sqrt_a", "q_s1m")]


_STEP_COMMON = [("rng", C.c_int), ("coef", C.c_void_p), ("table", C.c_void_p), ("state", C.c_void_p)]


class DdpmStepArgs(C.Structure):
    """pf_ddpm_step_args (include/pfhip.h); filled by ``_steps.ddpm_step`` only."""
    _fields_ = ([(n, C.c_void_p) for n in ("x", "eps", "orig", "mask", "noise_p", "noise_q")] + _STEP_COMMON
                + [(n, C.c_uint64) for n in ("seed", "draw_q", "draw_p", "elem_offset")] + [("x_out", C.c_void_p), ("n", C.c_size_t)])


class DdimStepArgs(C.Structure):
    """pf_ddim_step_args (include/pfhip.h); filled by ``_steps.ddim_step`` only."""
    _fields_ = ([(n, C.c_void_p) for n in ("x", "eps", "orig", "orig_noise", "mask", "noise")] + _STEP_COMMON
                + [(n, C.c_uint64) for n in ("seed", "draw", "elem_offset")] + [("x_out", C.c_void_p), ("n", C.c_size_t)])


class DpmStepArgs(C.Structure):
    """pf_dpm_step_args (include/pfhip.h); filled by ``_steps.dpm_step`` only."""
    _fields_ = ([(n, C.c_void_p) for n in ("x", "eps", "x0_prev", "x0_out", "orig", "orig_noise", "mask", "coef", "table", "state", "x_out")]
                + [("n", C.c_size_t)])


class DpmSdeCoef(C.Structure):
    """pf_dpm_sde_coef (include/pfhip.h): one step of the stochastic DPM-Solver++(2M) - ``DpmCoef``'s fields and ``sigma_n``, the standard
    deviation of the step's fresh noise (``0``: no noise term)."""
    _fields_ = DpmCoef._fields_ + [("sigma_n", C.c_float)]


class DpmSdeStepArgs(C.Structure):
    """pf_dpm_sde_step_args (include/pfhip.h); filled by ``_steps.dpm_sde_step`` only."""
    _fields_ = ([(n, C.c_void_p) for n in ("x", "eps", "x0_prev", "x0_out", "orig", "orig_noise", "mask", "noise")] + _STEP_COMMON
                + [(n, C.c_uint64) for n in ("seed", "draw", "elem_offset")] + [("x_out", C.c_void_p), ("n", C.c_size_t)])


class InvertCoef(C.Structure):
    """pf_invert_coef (include/pfhip.h): one upward step of exact DDIM inversion, ``x = c_y*y + c_e*eps``."""
    _fields_ = [("c_y", C.c_float), ("c_e", C.c_float)]


class InvertStepArgs(C.Structure):
    """pf_invert_step_args (include/pfhip.h); filled by ``_steps.invert_step`` only."""
    _fields_ = ([(n, C.c_void_p) for n in ("y", "eps", "x_iter", "coef", "table", "state", "x_out", "resid", "workspace")]
                + [("workspace_bytes", C.c_size_t), ("iters", C.c_int32), ("k", C.c_int32), ("slot", C.c_int64), ("n_slots", C.c_int64),
                   ("rows", C.c_int32), ("row_elems", C.c_size_t)])


class SlerpArgs(C.Structure):
    """pf_slerp_args (include/pfhip.h); filled by ``_steps.slerp_rows`` only."""
    _fields_ = ([(n, C.c_void_p) for n in ("a", "b", "t", "out", "stats", "weights", "workspace")]
                + [("workspace_bytes", C.c_size_t), ("mode", C.c_int32), ("frames", C.c_int32), ("rows", C.c_int32), ("row_elems", C.c_size_t)])


class CfgRescaleArgs(C.Structure):
    """pf_cfg_rescale_args (include/pfhip.h); filled by ``_steps.cfg_rescale`` only."""
    _fields_ = ([(n, C.c_void_p) for n in ("epsg", "eps", "stats", "weights", "workspace")]
                + [("workspace_bytes", C.c_size_t), ("phi", C.c_double), ("s1", C.c_float), ("s2", C.c_float), ("groups", C.c_int32),
                   ("rows", C.c_int32), ("row_elems", C.c_size_t)])


class X0ThresholdArgs(C.Structure):
    """pf_x0_threshold_args (include/pfhip.h); filled by ``_steps.x0_threshold`` only."""
    _fields_ = [("x", C.c_void_p), ("x_row_stride", C.c_size_t), ("eps", C.c_void_p), ("eps_out", C.c_void_p), ("t", C.c_void_p),
                ("t_stride", C.c_int32), ("table", C.c_void_p), ("n_table", C.c_int32), ("stats", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t), ("p", C.c_double), ("s_max", C.c_double), ("lo", C.c_float), ("hi", C.c_float),
                ("mode", C.c_int32), ("form", C.c_int32), ("rows", C.c_int32), ("row_elems", C.c_size_t)]


class X0PredictArgs(C.Structure):
    """pf_x0_predict_args (include/pfhip.h); filled by ``_steps.x0_predict`` only."""
    _fields_ = [("x", C.c_void_p), ("x_row_stride", C.c_size_t), ("eps", C.c_void_p), ("t", C.c_void_p), ("t_stride", C.c_int32),
                ("table", C.c_void_p), ("n_table", C.c_int32), ("x0", C.c_void_p), ("rows", C.c_int32), ("row_elems", C.c_size_t)]


class SteerResampleArgs(C.Structure):
    """pf_steer_resample_args (include/pfhip.h); filled by ``_steps.steer_resample`` only."""
    _fields_ = [("reward", C.c_void_p), ("base", C.c_void_p), ("lam", C.c_double), ("ess_frac", C.c_double), ("seed", C.c_uint64),
                ("group_offset", C.c_uint64), ("event", C.c_uint64), ("ancestors", C.c_void_p), ("weights", C.c_void_p), ("stats", C.c_void_p),
                ("groups", C.c_int32), ("n", C.c_int32)]


GATHER_MAX_TENSORS = 4     # PF_GATHER_MAX_TENSORS: tensors one pf_rows_gather launch moves
STEER_MAX_N = 256          # PF_STEER_MAX_N: particles of one group of pf_steer_resample


class RowsGatherArgs(C.Structure):
    """pf_rows_gather_args (include/pfhip.h); filled by ``_steps.rows_gather`` only."""
    _fields_ = [("src", C.c_void_p * GATHER_MAX_TENSORS), ("dst", C.c_void_p * GATHER_MAX_TENSORS), ("row_elems", C.c_size_t * GATHER_MAX_TENSORS),
                ("n_tensors", C.c_int32), ("ancestors", C.c_void_p), ("groups", C.c_int32), ("n", C.c_int32), ("per", C.c_int32)]


class WindowMergeArgs(C.Structure):
    """pf_window_merge_args (include/pfhip.h); filled by ``_steps.window_merge`` only."""
    _fields_ = ([("eps", C.c_void_p), ("row_weight", C.c_void_p), ("groups", C.c_int), ("s1", C.c_float), ("s2", C.c_float)]
                + [(n, C.c_int) for n in ("songs", "channels", "win_h", "width", "n_windows", "stride")] + [("out", C.c_void_p)])


class QsampleRowsArgs(C.Structure):
    """pf_qsample_rows_args (include/pfhip.h); filled by ``_steps.qsample_rows`` only."""
    _fields_ = ([(n, C.c_void_p) for n in ("x0", "noise", "t", "sqrt_ab", "sqrt_1mab")] + [("n_steps", C.c_int32), ("rng", C.c_int)]
                + [(n, C.c_uint64) for n in ("seed", "draw", "elem_offset")] + [("x_t", C.c_void_p), ("noise_out", C.c_void_p)]
                + [("rows", C.c_int32), ("row_elems", C.c_size_t)])


class MseRowsArgs(C.Structure):
    """pf_mse_rows_args (include/pfhip.h); filled by ``_steps.mse_rows`` only."""
    _fields_ = ([("eps_theta", C.c_void_p), ("noise", C.c_void_p), ("rng", C.c_int)] + [(n, C.c_uint64) for n in ("seed", "draw", "elem_offset")]
                + [("row_sum", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("rows", C.c_int32),
                   ("row_elems", C.c_size_t)])


class ChordForcedArgs(C.Structure):
    """pf_chord_forced_args (include/pfhip.h); filled by ``decoders.ChordDecoder.forward_forced`` only."""
    _fields_ = [("z", C.c_void_p), ("gt", C.c_void_p), ("rows", C.c_int32), ("feedback", C.c_int), ("force_mask", C.c_uint64),
                ("root", C.c_void_p), ("chroma", C.c_void_p), ("bass", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class GruStepArgs(C.Structure):
    """pf_gru_step_args (include/pfhip.h); filled by the recurrent-kernel matrix (tests/test_gpu_rnn_matrix.py) only."""
    _fields_ = [("x", C.c_void_p), ("ldx", C.c_int), ("Kx", C.c_int), ("wx", C.c_void_p), ("ldwx", C.c_int), ("h_in", C.c_void_p),
                ("wh", C.c_void_p), ("b_hh", C.c_void_p), ("add1", C.c_void_p), ("ld1", C.c_int), ("add2", C.c_void_p), ("ld2", C.c_int),
                ("h_out", C.c_void_p), ("R", C.c_int), ("H", C.c_int)]


class RollStatsArgs(C.Structure):
    """pf_roll_stats_args (include/pfhip.h); filled by ``score.roll_stats`` only."""
    _fields_ = ([(n, C.c_void_p) for n in ("prmat2c", "chord", "mask")] + [(n, C.c_int32) for n in ("n", "steps", "custom_round", "bass_relative")]
                + [(n, C.c_void_p) for n in ("counters", "chroma", "onsets")])


# PF_ROLL_*, in the enum's order; PF_ROLL_NCOUNT slots per image (the rest are written as 0)
ROLL_COUNTERS = ("N_ONSET", "N_SOUNDING", "N_ORPHAN", "CHORD_BEATS", "SOUND_ON_CHORD", "SOUND_IN_CHORD", "ONSET_IN_CHORD", "ONSET_ON_CHORD",
                 "CHORD_CLASSES", "CHORD_HEARD", "BASS_BEATS", "BASS_HIT", "LOW_KEY", "HIGH_KEY")
ROLL_NCOUNT = 16


class ChordRecognizeArgs(C.Structure):
    """pf_chord_recognize_args (include/pfhip.h); filled by ``chordrec.recognize_rolls`` only."""
    _fields_ = ([(n, C.c_void_p) for n in ("prmat2c", "chord", "cls_bits", "cls_const", "cls_rows", "consts")]
                + [(n, C.c_int32) for n in ("songs", "segments", "steps", "n_classes", "max_template", "custom_round", "bass_relative", "reserved")]
                + [(n, C.c_void_p) for n in ("labels", "bounds", "rows", "counters", "path_score", "chroma_q", "bass_q")])


# PF_CHORDREC_*, in the enum's order
CHORDREC_COUNTERS = ("BEATS", "ROOT_HIT", "CHROMA_HIT", "BASS_HIT", "FULL_HIT", "CHROMA_INTER", "CHROMA_UNION", "SEGMENTS")
CHORDREC_NCOUNT = 8
CHORDREC_MAX_BEATS = 512       # PF_CHORDREC_MAX_BEATS: beats of one song
CHORDREC_MAX_CLASSES = 576     # PF_CHORDREC_MAX_CLASSES


class RollMatchArgs(C.Structure):
    """pf_roll_match_args (include/pfhip.h); filled by ``rollmatch.match_windows`` only."""
    _fields_ = ([(n, C.c_void_p) for n in ("a_bits", "a_starts", "b_bits", "b_starts")]
                + [(n, C.c_int32) for n in ("na", "nb", "steps", "shifts", "topk", "reserved")]
                + [(n, C.c_void_p) for n in ("top_index", "top_shift", "top_inter", "top_union", "tab_inter", "tab_union", "tab_shift", "workspace")]
                + [("workspace_bytes", C.c_size_t)])


ROLL_MATCH_CHUNK = 256         # PF_ROLL_MATCH_CHUNK: corpus windows one workgroup of pf_roll_match scans
ROLL_MATCH_MAX_SHIFTS = 15     # PF_ROLL_MATCH_MAX_SHIFTS
ROLL_MATCH_MAX_TOPK = 8        # PF_ROLL_MATCH_MAX_TOPK


FEEDBACK = {"row": 0, "batch": 1}   # PF_FEEDBACK_ROW / PF_FEEDBACK_BATCH
MSE_CHUNK = 2048           # PF_MSE_CHUNK: elements of a row one workgroup of pf_mse_rows reduces
SLERP_MAX_FRAMES = 64      # PF_SLERP_MAX_FRAMES: frames one pf_slerp_rows call writes
SLERP_MODES = {"slerp": 0, "lerp": 1}
X0T_RESIDENT_MAX = 32768   # PF_X0T_RESIDENT_MAX: elements of a row the resident form of pf_x0_threshold holds in LDS
X0T_MODES = {"clip": 0, "dynamic": 1}
X0T_FORMS = {"auto": 0, "resident": 1, "streamed": 2}


class UNetPrepared(C.Structure):
    """pf_unet_prepared (include/pfhip.h): the step-invariant prefix a sampler computes once per loop."""
    _fields_ = [("time_table", C.c_void_p), ("n_time_rows", C.c_int32), ("cross_bias", C.c_void_p)]


class DDPMCfg(C.Structure):
    _fields_ = [
        ("image_channels", C.c_int32), ("n_channels", C.c_int32), ("n_levels", C.c_int32),
        ("ch_mults", C.c_int32 * 8), ("is_attn", C.c_int32 * 8), ("n_blocks", C.c_int32), ("img_h", C.c_int32), ("img_w", C.c_int32),
    ]


OPT_MLP_FUSED, OPT_ATTN_WIDE, OPT_CONV_T16, OPT_CONV_PP, OPT_CONV_WINO = 0, 1, 2, 3, 4
OPT_COUNT = 5              # PF_OPT_COUNT
OPT_AUTO, OPT_OFF, OPT_ON = -1, 0, 1


class ConvArgs(C.Structure):
    _fields_ = [
        ("x0", C.c_void_p), ("c0", C.c_int32), ("x1", C.c_void_p), ("c1", C.c_int32),
        ("batch", C.c_int32), ("hin", C.c_int32), ("win", C.c_int32),
        ("ks", C.c_int32), ("stride", C.c_int32), ("ups", C.c_int32),
        ("w", C.c_void_p), ("n", C.c_int32),
        ("prologue", C.c_int32), ("sc", C.c_void_p), ("sh", C.c_void_p), ("mean", C.c_void_p), ("rstd", C.c_void_p),
        ("bias", C.c_void_p), ("sbias", C.c_void_p), ("ld_sbias", C.c_int32), ("res", C.c_void_p), ("ld_res", C.c_int32),
        ("geglu", C.c_int32),
        ("out", C.c_void_p), ("ld_out", C.c_int32),
        ("precision", C.c_int32),
        ("stats_out", C.c_void_p),
        ("splitk_ws", C.c_void_p), ("splitk_ws_bytes", C.c_size_t),
        ("a_planes", C.c_int32), ("out_planes", C.c_void_p),
        ("qkv_planes", C.c_void_p),
        ("ups_fold", C.c_int32),
        ("skip_x0", C.c_void_p), ("skip_c0", C.c_int32), ("skip_x1", C.c_void_p), ("skip_c1", C.c_int32),
        ("skip_w", C.c_void_p), ("skip_bias", C.c_void_p),
        ("gn_stats0", C.c_void_p), ("gn_tiles0", C.c_int32), ("gn_stats1", C.c_void_p), ("gn_tiles1", C.c_int32),
        ("gn_gamma", C.c_void_p), ("gn_beta", C.c_void_p), ("gn_eps", C.c_float), ("gn_groups", C.c_int32),
        ("sbias_rows", C.c_void_p), ("sbias_nrows", C.c_int32), ("no_t16", C.c_int32), ("no_pp", C.c_int32),
        ("force_tile", C.c_int32), ("force_ksplit", C.c_int32), ("x1_bmod", C.c_int32),
        ("w_wino", C.c_void_p), ("wino", C.c_int32), ("absmax_slot", C.c_void_p),
        ("pad_mode", C.c_int32),
    ]


PAD_SAME, PAD_BOTTOM_RIGHT = 0, 1   # pf_conv_args.pad_mode


class ConvPlanInfo(C.Structure):   # pf_conv_plan_info: what pf_conv_describe says a pf_conv2d launch runs
    _fields_ = [
        ("form", C.c_int32), ("tile_h", C.c_int32), ("tile_w", C.c_int32), ("tile_n", C.c_int32), ("wave_groups", C.c_int32),
        ("ksplit_wanted", C.c_int32), ("ksplit", C.c_int32), ("stats_tiles", C.c_int32),
        ("splitk_ws_bytes", C.c_size_t), ("flops", C.c_double),
    ]


# PF_CONV_FORM_*, in the enum's order
CONV_FORMS = ("f32", "split", "split_kg2", "split_pingpong", "upfold", "planes", "wino")


def conv_form(lib, a: ConvArgs) -> str:
    """'form THxTWxBN[ ks=S]': what pf_conv_describe says a pf_conv2d launch with these arguments runs ('refused' if it would not)"""
    i = ConvPlanInfo()
    if lib.pf_conv_describe(C.byref(a), C.byref(i)) != 0:
        return "refused"
    return f"{CONV_FORMS[i.form]} {i.tile_h}x{i.tile_w}x{i.tile_n}" + (f" ks={i.ksplit}" if i.ksplit > 1 else "")


class AutoencCfg(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int32), ("out_channels", C.c_int32), ("channels", C.c_int32), ("n_levels", C.c_int32),
        ("channel_multipliers", C.c_int32 * 8), ("n_resnet_blocks", C.c_int32), ("z_channels", C.c_int32), ("emb_channels", C.c_int32),
    ]


# name -> (restype, argtypes); this table is also what tests/test_abi.py checks against include/pfhip.h
SIGNATURES = {
    "pf_version": (C.c_int, []),
    "pf_last_error": (C.c_char_p, []),
    "pf_unet_create": (C.c_int, [C.POINTER(UNetCfg), C.POINTER(C.c_void_p)]),
    "pf_unet_destroy": (None, [C.c_void_p]),
    "pf_unet_weight_bytes": (C.c_size_t, [C.c_void_p]),
    "pf_unet_n_params": (C.c_int, [C.c_void_p]),
    "pf_unet_param_info": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, c_i64_p, C.POINTER(C.c_int)]),
    "pf_unet_pack_param": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, c_i64_p, C.c_int, C.c_void_p]),
    "pf_unet_pack_missing": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "pf_unet_bind_weights": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pf_unet_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "pf_unet_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                  C.c_void_p, C.c_size_t, C.c_void_p]),
    "pf_unet_forward_prepared": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(UNetPrepared),
                                           C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pf_unet_forward_cfg": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(UNetPrepared),
                                           C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pf_unet_forward_cfgn": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(UNetPrepared),
                                       C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pf_unet_time_bias_width": (C.c_int, [C.c_void_p]),
    "pf_unet_cross_bias_width": (C.c_int, [C.c_void_p]),
    "pf_unet_prepare_time": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pf_unet_prepare_cond": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pf_unet_n_launches_prepared": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "pf_unet_workspace_bytes_cfg": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "pf_unet_n_launches_cfg": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "pf_unet_workspace_bytes_cfgn": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "pf_unet_n_launches_cfgn": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "pf_unet_set_option": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "pf_unet_get_option": (C.c_int, [C.c_void_p, C.c_int]),
    "pf_unet_set_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "pf_unet_track_absmax": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pf_unet_profile_read_direct": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int]),
    "pf_unet_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), c_float_p, C.POINTER(C.c_double), C.c_int]),
    "pf_unet_n_launches": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "pf_cfg_combine": (C.c_int, [C.c_void_p, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pf_cfg_combine3": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pf_cfg_rescale_workspace_bytes": (C.c_size_t, [C.c_int, C.c_size_t]),
    "pf_cfg_rescale": (C.c_int, [C.POINTER(CfgRescaleArgs), C.c_void_p]),
    "pf_x0_threshold_workspace_bytes": (C.c_size_t, [C.c_int, C.c_size_t, C.c_int]),
    "pf_x0_threshold": (C.c_int, [C.POINTER(X0ThresholdArgs), C.c_void_p]),
    "pf_x0_predict": (C.c_int, [C.POINTER(X0PredictArgs), C.c_void_p]),
    "pf_steer_resample": (C.c_int, [C.POINTER(SteerResampleArgs), C.c_void_p]),
    "pf_rows_gather": (C.c_int, [C.POINTER(RowsGatherArgs), C.c_void_p]),
    "pf_window_split": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]),
    "pf_window_merge": (C.c_int, [C.POINTER(WindowMergeArgs), C.c_void_p]),
    "pf_ddpm_step": (C.c_int, [C.POINTER(DdpmStepArgs), C.c_void_p]),
    "pf_axpby": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pf_ddim_step": (C.c_int, [C.POINTER(DdimStepArgs), C.c_void_p]),
    "pf_dpm_step": (C.c_int, [C.POINTER(DpmStepArgs), C.c_void_p]),
    "pf_dpm_sde_step": (C.c_int, [C.POINTER(DpmSdeStepArgs), C.c_void_p]),
    "pf_invert_step_workspace_bytes": (C.c_size_t, [C.c_int, C.c_size_t]),
    "pf_invert_step": (C.c_int, [C.POINTER(InvertStepArgs), C.c_void_p]),
    "pf_slerp_rows_workspace_bytes": (C.c_size_t, [C.c_int, C.c_size_t]),
    "pf_slerp_rows": (C.c_int, [C.POINTER(SlerpArgs), C.c_void_p]),
    "pf_step_advance": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "pf_randn": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]),
    "pf_clock_probe": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pf_mfma_probe": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_void_p]),
    "pf_step_state_set": (C.c_int, [C.c_void_p, C.c_int64, C.c_uint64, C.c_void_p]),
    "pf_step_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "pf_step_end": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "pf_randn_dev": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p]),
    "pf_qsample_rows": (C.c_int, [C.POINTER(QsampleRowsArgs), C.c_void_p]),
    "pf_mse_rows_workspace_bytes": (C.c_size_t, [C.c_int, C.c_size_t]),
    "pf_mse_rows": (C.c_int, [C.POINTER(MseRowsArgs), C.c_void_p]),
    "pf_chord_ce_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pf_normal_rsample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pf_comm_unique_id": (C.c_int, [C.c_void_p]),
    "pf_comm_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "pf_comm_bcast": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "pf_comm_destroy": (C.c_int, [C.c_void_p]),
    "pf_prmat2c_durations": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pf_roll_stats": (C.c_int, [C.POINTER(RollStatsArgs), C.c_void_p]),
    "pf_chord_recognize": (C.c_int, [C.POINTER(ChordRecognizeArgs), C.c_void_p]),
    "pf_roll_pack": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pf_roll_match_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "pf_roll_match": (C.c_int, [C.POINTER(RollMatchArgs), C.c_void_p]),
    "pf_encoder_create": (C.c_int, [C.c_int] * 6 + [C.POINTER(C.c_void_p)]),
    "pf_encoder_create_dist": (C.c_int, [C.c_int] * 7 + [C.POINTER(C.c_void_p)]),
    "pf_encoder_destroy": (None, [C.c_void_p]),
    "pf_encoder_weight_bytes": (C.c_size_t, [C.c_void_p]),
    "pf_encoder_pack_param": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, c_i64_p, C.c_int, C.c_void_p]),
    "pf_encoder_pack_missing": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "pf_encoder_bind_weights": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pf_encoder_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "pf_encoder_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pf_encoder_forward_dist": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                          C.c_void_p]),
    "pf_decoder_create": (C.c_int, [C.c_int] * 7 + [C.POINTER(C.c_void_p)]),
    "pf_decoder_destroy": (None, [C.c_void_p]),
    "pf_decoder_weight_bytes": (C.c_size_t, [C.c_void_p]),
    "pf_decoder_n_params": (C.c_int, [C.c_void_p]),
    "pf_decoder_param_info": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, c_i64_p, C.POINTER(C.c_int)]),
    "pf_decoder_pack_param": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, c_i64_p, C.c_int, C.c_void_p]),
    "pf_decoder_pack_missing": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "pf_decoder_bind_weights": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pf_decoder_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "pf_decoder_launches": (C.c_int, [C.c_void_p, C.c_int]),
    "pf_decoder_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_size_t, C.c_void_p]),
    "pf_decoder_forced_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "pf_decoder_forced_launches": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "pf_decoder_forward_forced": (C.c_int, [C.c_void_p, C.POINTER(ChordForcedArgs), C.c_void_p]),
    "pf_packed_gemm_weight_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "pf_pack_gemm_weight": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "pf_pack_gemm_weight_bf16x3": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "pf_pack_upfold_weight_bf16x3": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "pf_wino_weight_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "pf_pack_wino_weight_bf16x3": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "pf_unet_set_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "pf_unet_get_precision": (C.c_int, [C.c_void_p]),
    "pf_x3_element": (C.c_int, []),
    "pf_gn_scale_shift": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pf_ln_stats": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pf_conv_in": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p, C.c_void_p]),
    "pf_conv_in_stats_tiles": (C.c_int, [C.c_int] * 4),
    "pf_conv_out": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 5 + [C.c_void_p]),
    "pf_time_embed": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 3 + [C.c_void_p]),
    "pf_matvec": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p]),
    "pf_gru_gates": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p]),
    "pf_gru_step": (C.c_int, [C.POINTER(GruStepArgs), C.c_void_p]),
    "pf_ln_planes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pf_mlp_geglu_fused": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pf_mlp_geglu_proj_fused": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float] + [C.c_void_p] * 10),
    "pf_conv2d": (C.c_int, [C.POINTER(ConvArgs), C.c_void_p]),
    "pf_conv_stats_tiles": (C.c_int, [C.POINTER(ConvArgs)]),
    "pf_conv_splitk_ws_bytes": (C.c_size_t, [C.POINTER(ConvArgs)]),
    "pf_conv_describe": (C.c_int, [C.POINTER(ConvArgs), C.POINTER(ConvPlanInfo)]),
    "pf_gn_finalize_tiles": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pf_attention_bf16x3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "pf_attention_split_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "pf_attention_bf16x3_split": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pf_attention": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                               C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "pf_ddpm_create": (C.c_int, [C.POINTER(DDPMCfg), C.POINTER(C.c_void_p)]),
    "pf_ddpm_destroy": (None, [C.c_void_p]),
    "pf_ddpm_weight_bytes": (C.c_size_t, [C.c_void_p]),
    "pf_ddpm_n_params": (C.c_int, [C.c_void_p]),
    "pf_ddpm_param_info": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, c_i64_p, C.POINTER(C.c_int)]),
    "pf_ddpm_pack_param": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, c_i64_p, C.c_int, C.c_void_p]),
    "pf_ddpm_pack_missing": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "pf_ddpm_bind_weights": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pf_ddpm_set_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "pf_ddpm_get_precision": (C.c_int, [C.c_void_p]),
    "pf_ddpm_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "pf_ddpm_n_launches": (C.c_int, [C.c_void_p, C.c_int]),
    "pf_ddpm_flops": (C.c_double, [C.c_void_p, C.c_int]),
    "pf_ddpm_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pf_autoenc_create": (C.c_int, [C.POINTER(AutoencCfg), C.POINTER(C.c_void_p)]),
    "pf_autoenc_destroy": (None, [C.c_void_p]),
    "pf_autoenc_weight_bytes": (C.c_size_t, [C.c_void_p]),
    "pf_autoenc_n_params": (C.c_int, [C.c_void_p]),
    "pf_autoenc_param_info": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, c_i64_p, C.POINTER(C.c_int)]),
    "pf_autoenc_pack_param": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, c_i64_p, C.c_int, C.c_void_p]),
    "pf_autoenc_pack_missing": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "pf_autoenc_bind_weights": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pf_autoenc_set_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "pf_autoenc_get_precision": (C.c_int, [C.c_void_p]),
    "pf_autoenc_encode_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "pf_autoenc_decode_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "pf_autoenc_encode_launches": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "pf_autoenc_decode_launches": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "pf_autoenc_encode_flops": (C.c_double, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "pf_autoenc_decode_flops": (C.c_double, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "pf_autoenc_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pf_autoenc_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pf_gaussian_sample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_float, C.c_void_p, C.c_size_t,
                                     C.c_void_p]),
    "pf_attention_wide_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "pf_attention_wide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_void_p, C.c_size_t, C.c_void_p]),
    "pf_convt_weight_floats": (C.c_size_t, [C.c_int, C.c_int]),
    "pf_pack_convt_weight_bf16x3": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "pf_pack_convt_weight_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "pf_conv_transpose_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
}

_libs: dict = {}


def load(variant: Optional[str] = None) -> C.CDLL:
    """dlopen the library (default build, or the named variant) and attach prototypes.  Raises if it has not been built.
    Both builds can live in one process: they are opened RTLD_LOCAL and share nothing but the HIP runtime."""
    v = X3_VARIANT if variant is None else variant
    if v in _libs:
        return _libs[v]
    path = lib_path(v)
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: the HIP extension is not built. Run `python -m polyffusion_amd.build{' --variant=' + v if v else ''}` "
            "(or __graft_entry__.build()). There is no CPU fallback for this path.")
    lib = C.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_NOW)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.pf_x3_element() != (1 if v == "f16" else 0):
        raise RuntimeError(f"{path}: built with the wrong split element type (pf_x3_element() = {lib.pf_x3_element()})")
    _libs[v] = lib
    return lib


def check(rc: int, what: str = "", lib: Optional[C.CDLL] = None) -> int:
    """Raise on a negative return code, with the message of the library that produced it (`lib`: default build if omitted)."""
    if rc < 0:
        msg = (lib or load()).pf_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"libpfhip {what}: error {rc}: {msg}")
    return rc


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("polyffusion_amd needs an AMD GPU (gfx950); no CPU fallback exists for the denoising path")


def ptr(t) -> int:
    """Raw device/host address of a torch tensor (None -> NULL)."""
    return 0 if t is None else t.data_ptr()


def current_stream() -> int:
    import torch
    return torch.cuda.current_stream().cuda_stream
