"""The chd_8bar objective without a GPU: the new C entry points are declared, exported and bound; the launch accounting of the
teacher-forced chord walk; what it refuses before it enqueues anything; the Python surface and the ``validate`` flags."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from polyffusion_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pf_decoder_forward_forced", "pf_decoder_forced_workspace_bytes", "pf_decoder_forced_launches", "pf_chord_ce_rows", "pf_normal_rsample")
FAKE = 0x1000          # a non-null address that a refused call never touches


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from polyffusion_amd.build import build
        build(verbose=False)
    return _lib.load()


def _dec(n_step=8, **kw):
    from polyffusion_amd.decoders import ChordDecoder
    return ChordDecoder(36, kw.get("z_input_dim", 256), kw.get("hidden_dim", 512), kw.get("z_dim", 256), n_step)


def _args(rows=3, ws_bytes=1 << 20, **kw):
    a = _lib.ChordForcedArgs(z=FAKE, gt=FAKE, rows=rows, feedback=0, force_mask=0, root=FAKE, chroma=FAKE, bass=FAKE, workspace=FAKE,
                             workspace_bytes=ws_bytes)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_header_declares_and_library_exports_the_new_symbols(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "pfhip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pf_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} not declared in pfhip.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.SIGNATURES
    assert "pf_chord_forced_args" in hdr and "PF_FEEDBACK_ROW = 0" in hdr and "PF_FEEDBACK_BATCH = 1" in hdr
    if os.path.exists(_lib.lib_path("f16")):
        assert all(hasattr(_lib.load("f16"), name) for name in NEW)
    # the struct as C lays it out: pointers, two ints sharing eight bytes, the mask, pointers, size
    f = _lib.ChordForcedArgs
    assert (f.rows.offset, f.feedback.offset, f.force_mask.offset, f.root.offset, f.workspace_bytes.offset) == (16, 20, 24, 32, 64)
    assert C.sizeof(f) == 72


@pytest.mark.parametrize("n_step", [2, 8, 32])
def test_forced_walk_launch_counts(lib, n_step):
    """From the dry walks: row feedback enqueues what the greedy decode enqueues, batch feedback at most n_step - 1 launches more, and
    neither depends on the number of rows."""
    d = _dec(n_step)
    greedy = d.n_launches(1)
    assert greedy == 3 + 2 * n_step
    for rows in (1, 3, 9, 128):
        assert d.n_launches(rows) == greedy                               # unchanged by this walk's existence
        assert d.n_launches_forced(rows, "row") == greedy
        assert greedy <= d.n_launches_forced(rows, "batch") <= greedy + n_step - 1
    assert d.n_launches_forced(4, "batch") == greedy + n_step - 1         # mask 0: every step but the last feeds back
    assert lib.pf_decoder_forced_launches(d._h, 4, 7) == 0 and lib.pf_decoder_forced_launches(d._h, 0, 0) == 0
    for rows in (1, 9, 128):
        assert lib.pf_decoder_forced_workspace_bytes(d._h, rows) == lib.pf_decoder_workspace_bytes(d._h, rows) > 0


def test_forced_walk_refusals_come_before_any_launch(lib):
    """None of these needs a GPU: the call returns before it touches HIP or any of the (fake) pointers."""
    d = _dec(8)

    def refused(dec, a, pattern):
        rc = lib.pf_decoder_forward_forced(dec._h, C.byref(a), None)
        msg = lib.pf_last_error().decode()
        assert rc < 0 and re.search(pattern, msg), (rc, msg)

    refused(d, _args(gt=None), "gt .* is null")
    refused(d, _args(feedback=2), "unknown feedback 2")
    refused(d, _args(feedback=-1), "unknown feedback -1")
    refused(d, _args(rows=0), "bad arguments")
    refused(d, _args(root=None), "bad arguments")
    need = lib.pf_decoder_forced_workspace_bytes(d._h, 3)
    refused(d, _args(ws_bytes=need - 1), f"workspace too small \\({need - 1} < {need}\\)")
    refused(d, _args(workspace=FAKE + 4, ws_bytes=need), "16-byte aligned")
    refused(d, _args(ws_bytes=need), "weights not bound")                 # everything else in order: only the weights are missing
    refused(_dec(66), _args(), "n_step - 1 = 65")                         # the mask holds 64 steps
    d65 = _dec(65)
    refused(d65, _args(ws_bytes=lib.pf_decoder_forced_workspace_bytes(d65._h, 3)), "weights not bound")
    from polyffusion_amd.decoders import PianoTreeDecoder
    pn = PianoTreeDecoder(max_simu_note=4)
    refused(pn, _args(), "chord decoder only")
    assert lib.pf_decoder_forced_workspace_bytes(pn._h, 3) == 0 and lib.pf_decoder_forced_launches(pn._h, 3, 0) == 0
    assert lib.pf_decoder_forward_forced(d._h, None, None) < 0


def test_loss_entry_points_refuse_bad_arguments(lib):
    assert lib.pf_chord_ce_rows(None, FAKE, FAKE, FAKE, 1, 8, FAKE, None, None) < 0
    assert lib.pf_chord_ce_rows(FAKE, FAKE, FAKE, FAKE, 0, 8, FAKE, None, None) < 0
    assert lib.pf_chord_ce_rows(FAKE, FAKE, FAKE, FAKE, 1, 0, FAKE, None, None) < 0
    assert lib.pf_chord_ce_rows(FAKE, FAKE, FAKE, FAKE, 1, 8, FAKE + 4, None, None) < 0 and b"aligned" in lib.pf_last_error()
    assert lib.pf_normal_rsample(None, FAKE, None, 0, 0, 0, FAKE, 4, None) < 0
    assert lib.pf_normal_rsample(FAKE, FAKE, None, 0, 0, 0, FAKE, 0, None) < 0


def test_python_surface():
    from polyffusion_amd import chd8bar
    from polyffusion_amd.decoders import ChordDecoder
    from polyffusion_amd.model_sdf import ChordEncoder
    from polyffusion_amd.params import PRESETS
    d = _dec(8)
    with pytest.raises(NotImplementedError, match="teacher forcing.*forward_forced"):
        d.forward(None, False, 0.5)
    assert d.force_mask([True, False, False, True, False, False, True]) == 0b1001001 and d.force_mask(0b1111111) == 127
    assert d.force_mask([False] * 7) == 0
    with pytest.raises(ValueError, match="n_step - 1 = 7"):
        d.force_mask([True] * 8)
    with pytest.raises(ValueError, match="bits past"):
        d.force_mask(1 << 7)
    with pytest.raises(ValueError, match="feedback"):
        d.forward_forced(torch.zeros(1, 256), torch.zeros(1, 8, 36), 0, "union")
    assert _dec(65).force_mask((1 << 64) - 1) == (1 << 64) - 1
    # the chd_8bar sizes live in the module, not in the UNet preset table
    assert chd8bar.CHD_8BAR["chd_n_step"] == 32 and chd8bar.CHD_8BAR["chd_z_dim"] == 512 and tuple(chd8bar.CHD_8BAR["tfr_chd"]) == (0.5, 0.0)
    assert "chd_8bar" not in PRESETS
    m = chd8bar.Chord_8Bar.from_params()
    assert isinstance(m.chord_enc, ChordEncoder) and m.chord_enc.with_scale and isinstance(m.chord_dec, ChordDecoder)
    assert (m.chord_dec.n_step, m.chord_dec.z_dim, m.chord_dec.hidden_dim) == (32, 512, 512)
    with pytest.raises(ValueError, match="with_scale"):
        chd8bar.Chord_8Bar(ChordEncoder(36, 64, 32), _dec(8))
    with pytest.raises(RuntimeError, match="chord_enc"):
        m.load_state_dict({"model": {"ldm.alpha": np.zeros(3, np.float32)}})
    # Polydis' training entry points keep raising
    from polyffusion_amd import polydis
    for name in ("loss", "loss_function"):
        if hasattr(polydis.DisentangleVAE, name):
            with pytest.raises(NotImplementedError):
                getattr(polydis.DisentangleVAE, name)(None)


def test_validate_parser_accepts_the_new_flags():
    from polyffusion_amd import validate
    p = validate.make_parser()
    a = p.parse_args(["--model", "chd_8bar", "--synthetic_weights", "--synthetic", "--batch_num", "2", "--batch_size", "8"])
    assert (a.model, a.tfr_chd, a.global_step, a.feedback) == ("chd_8bar", 0.0, None, "row")
    a = p.parse_args(["--model", "chd_8bar", "--tfr_chd", "0.25", "--feedback", "batch", "--global_step", "20000"])
    assert (a.tfr_chd, a.feedback, a.global_step) == (0.25, "batch", 20000)
    with pytest.raises(SystemExit):
        p.parse_args(["--model", "chd_8bar", "--feedback", "union"])
    assert p.parse_args([]).model == "sdf"                                 # the default and the other paths are as they were
    # the chord-only synthetic source: sample g is the same sample however the epoch is cut
    one = next(validate.synthetic_chord_batches(4, 1, 3, device="cpu"))
    two = list(validate.synthetic_chord_batches(2, 2, 3, device="cpu"))
    assert one[0] is None and tuple(one[2].shape) == (4, 32, 36)
    assert torch.equal(one[2], torch.cat([two[0][2], two[1][2]]))
