"""The recurrent kernels against their float64 oracles at their edges (-m gpu; tests/rnn_matrix.py holds the cases, the oracles and the
tolerances): pf_gru_gates (plain and masked), pf_gru_step, the chord, texture and PianoTree encoders and the greedy decodes of the chord and
PianoTree decoders through the library handles their Python classes hold.

One launch, forward or decode per case.  Everything it writes lives in a tests/gpu_guard.Guarded buffer: every owned element must be within the
case's tolerance of the oracle (profiles/rnn_error_model.md; no constant of it comes from a GPU), every other element must keep the
sentinel - the first half of the [rows][2H] state a gate update owns the second half of included - and a second launch must leave the same
bits.  A masked row with step >= len keeps its bits.  Rows of a 17-row (or 9-row) batch launched alone equal the batch's rows bit for
bit.  A decode's decisions - the PianoTree decoder's integer grid, and the lengths it implies - equal the float64 decode's exactly, its
logits are within the tolerance, and duplicated classes carry equal logits and decide for the lower index (a tied duration or chroma bit
is 0).  Arguments the library refuses must return PF_EINVAL and leave every buffer untouched.

Largest err / tol seen on an MI355X (102 cases in 9 s; the two builds agree): gate update 0.24, fused step 0.25, chord encoder 0.22,
texture encoder 0.24, PianoTree encoder 0.31, chord decoder 0.24, PianoTree decoder 0.25; every saturated case 0.00 (the gates are
exactly 0 or 1 on both sides)."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import rnn_matrix as rm  # noqa: E402
from gpu_guard import SENTINEL32, Guarded, _dev  # noqa: E402
from polyffusion_amd import _lib  # noqa: E402

# the two per-launch entry points run in both builds (the kernels are plain fp32 in either); the model handles live in the default one
CASES = [(k, s, v) for k, s in rm.cases() for v in (("", "f16") if s.kind in ("gates", "step") else ("",))]
_faulted = []   # the case whose launch raised: nothing more is started on the GPU after it


def _built(variant):
    if not os.path.exists(_lib.lib_path(variant)):
        from polyffusion_amd.build import build
        build(verbose=False, variant=variant)
    return _lib.load(variant)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def _f32(g):
    return g.body().view(torch.float32).cpu()


def _encoder(s, state):
    from polyffusion_amd.model_sdf import ChordEncoder, PianoTreeEncoder, TextureEncoder
    if s.enc == "chord":
        e = ChordEncoder(s.inp, s.H, s.z, with_scale=bool(s.with_scale))
    elif s.enc == "texture":
        e = TextureEncoder(s.emb, s.H, s.z, s.C, with_scale=bool(s.with_scale))
    else:
        e = PianoTreeEncoder(max_simu_note=s.S, note_emb_size=s.emb, enc_notes_hid_size=s.Hn, enc_time_hid_size=s.Ht, z_size=s.z)
    return e.load_state_dict(state)


def _enc_forward(lib, e, s, x, rows, mu, scale):
    n_step = {"chord": s.get("T", 0), "texture": 8, "pnotree": s.get("S", 0)}[s.enc]
    ws = e.workspace_for(lib.pf_encoder_workspace_bytes(e._h, rows), x.device)
    if scale is not None:
        return lib.pf_encoder_forward_dist(e._h, x.data_ptr(), rows, n_step, mu.ptr, scale.ptr, ws.data_ptr(), ws.numel(), _lib.current_stream())
    return lib.pf_encoder_forward(e._h, x.data_ptr(), rows, n_step, mu.ptr, ws.data_ptr(), ws.numel(), _lib.current_stream())


def _plan(lib, s, d):
    """(guarded outputs, launch(), read(), rows_alone() or None)"""
    st = _lib.current_stream()
    if s.kind == "gates":
        H, rows = s.hidden, s.rows
        dev = {k: _dev(v) for k, v in d.items()}
        g = {"h": Guarded(rows, 2 * H, 2 * H)}      # the update owns the second half of every row; the first must keep the sentinel
        T = s.seq_len or s.t_steps
        gi = dev["gi"].data_ptr() + (0 if s.seq_len else s.t * 3 * H * 4)

        def launch():
            g["h"].body()[:, H:] = dev["h"][:rows * H].view(torch.int32).view(rows, H)      # in place: every launch starts from h
            return lib.pf_gru_gates(gi, T * 3 * H, dev["gh"].data_ptr(), g["h"].ptr + H * 4, 2 * H, rows, H,
                                    dev["lens"].data_ptr() if s.seq_len else 0, s.seq_len, s.step, s.reverse, st)

        def read():
            assert bool((g["h"].body()[:, :H] == SENTINEL32).all()), "a gate update wrote into the other direction's half"
            return _f32(g["h"])[:, H:]
        return g, launch, read, None
    if s.kind == "step":
        H, R = s.H, s.R
        dev = {k: _dev(v) for k, v in d.items()}
        g = {"h_out": Guarded(R, H, H)}
        p = lambda name: dev[name].data_ptr() if name in dev else 0  # noqa: E731
        ldx, ld2 = (0 if s.ldx0 else s.Kx), (3 * H if s.ld2 else 0)

        def args(r0, rows, out):
            return _lib.GruStepArgs(x=p("x") + r0 * ldx * 4 if s.Kx else 0, ldx=ldx, Kx=s.Kx, wx=p("wx_wide") + rm.WX_OFF * 4 if s.Kx else 0,
                                    ldwx=s.Kx + rm.WX_PAD if s.Kx else 0, h_in=p("h_in") + r0 * H * 4, wh=p("wh"), b_hh=p("b_hh"),
                                    add1=p("add1") + r0 * 3 * H * 4 if s.add1 else 0, ld1=3 * H, add2=p("add2") + r0 * ld2 * 4 if s.add2 else 0,
                                    ld2=ld2, h_out=out.ptr, R=rows, H=H)

        def rows_alone():
            out = []
            for r in (0, 7, 8, 16):
                one = Guarded(1, H, H)
                a = args(r, 1, one)
                _lib.check(lib.pf_gru_step(C.byref(a), st), "pf_gru_step", lib)
                torch.cuda.synchronize()
                assert one.guards_intact()
                out.append((r, one.body()[0].cpu()))
            return out
        whole = args(0, R, g["h_out"])

        def launch(keep=dev):      # the struct holds raw addresses: the closure keeps the input tensors alive
            return lib.pf_gru_step(C.byref(whole), st)
        return g, launch, lambda: _f32(g["h_out"]), (rows_alone if R == 17 else None)
    if s.kind == "dec":
        from polyffusion_amd.decoders import ChordDecoder
        dec = ChordDecoder(36, s.zin, s.H, s.z, s.n).load_state_dict(d["state"])
        z = d["z"].cuda().contiguous()
        g = {"root": Guarded(s.R, s.n * 12, s.n * 12), "chroma": Guarded(s.R, s.n * 24, s.n * 24), "bass": Guarded(s.R, s.n * 12, s.n * 12)}

        def forward(zz, out):
            ws = dec.workspace_for(lib.pf_decoder_workspace_bytes(dec._h, zz.shape[0]), zz.device)
            return lib.pf_decoder_forward(dec._h, zz.data_ptr(), zz.shape[0], out["root"].ptr, out["chroma"].ptr, out["bass"].ptr, 0,
                                          ws.data_ptr(), ws.numel(), st)

        def rows_alone():
            out = []
            for r in sorted({0, 8, s.R - 1}):
                one = {n: Guarded(1, b.ld, b.ld) for n, b in g.items()}
                _lib.check(forward(z[r:r + 1].contiguous(), one), "pf_decoder_forward", lib)
                torch.cuda.synchronize()
                assert all(b.guards_intact() for b in one.values())
                out.append((r, {n: b.body()[0].cpu() for n, b in one.items()}))
            return out
        read = lambda: rm.Result(root=_f32(g["root"]).reshape(s.R, s.n, 12), chroma=_f32(g["chroma"]).reshape(s.R, s.n, 12, 2),  # noqa: E731
                                 bass=_f32(g["bass"]).reshape(s.R, s.n, 12))
        return g, lambda: forward(z, g), read, (rows_alone if s.R > 8 else None)
    if s.kind == "pn":
        from polyffusion_amd.decoders import PianoTreeDecoder
        dec = PianoTreeDecoder(max_simu_note=rm.PN_S, dec_dur_hid_size=s.HD).load_state_dict(d["state"])
        z = d["z"].cuda().contiguous()
        n = 32 * (rm.PN_S - 1)
        g = {"pitch": Guarded(s.R, n * 130, n * 130), "dur": Guarded(s.R, n * 10, n * 10), "est": Guarded(s.R, n * 6, n * 6)}

        def forward(zz, out):
            ws = dec.workspace_for(lib.pf_decoder_workspace_bytes(dec._h, zz.shape[0]), zz.device)
            return lib.pf_decoder_forward(dec._h, zz.data_ptr(), zz.shape[0], out["pitch"].ptr, out["dur"].ptr, 0, out["est"].ptr,
                                          ws.data_ptr(), ws.numel(), st)

        def rows_alone():
            out = []
            for r in sorted({0, 8, s.R - 1}):
                one = {name: Guarded(1, b.ld, b.ld) for name, b in g.items()}
                _lib.check(forward(z[r:r + 1].contiguous(), one), "pf_decoder_forward", lib)
                torch.cuda.synchronize()
                assert all(b.guards_intact() for b in one.values())
                out.append((r, {name: b.body()[0].cpu() for name, b in one.items()}))
            return out
        read = lambda: rm.Result(pitch=_f32(g["pitch"]).reshape(s.R, 32, rm.PN_S - 1, 130), dur=_f32(g["dur"]).reshape(s.R, 32, rm.PN_S - 1, 5, 2),  # noqa: E731
                                 est=g["est"].body().cpu().long().reshape(s.R, 32, rm.PN_S - 1, 6))
        return g, lambda: forward(z, g), read, rows_alone
    e = _encoder(s, d["state"])
    x = d["x"].to(torch.float32).cuda().contiguous()
    g = {"mu": Guarded(s.b, s.z, s.z)}
    if s.with_scale:
        g["scale"] = Guarded(s.b, s.z, s.z)

    def rows_alone():
        out = []
        for r in sorted({0, 7, 8, s.b - 1}):
            one = {n: Guarded(1, s.z, s.z) for n in g}
            _lib.check(_enc_forward(lib, e, s, x[r:r + 1].contiguous(), 1, one["mu"], one.get("scale")), "pf_encoder_forward", lib)
            torch.cuda.synchronize()
            assert all(b.guards_intact() for b in one.values())
            out.append((r, {n: b.body()[0].cpu() for n, b in one.items()}))
        return out
    read = lambda: rm.Result(mu=_f32(g["mu"]), **({"scale": _f32(g["scale"])} if s.with_scale else {}))  # noqa: E731
    return g, lambda: _enc_forward(lib, e, s, x, s.b, g["mu"], g.get("scale")), read, (rows_alone if s.b in (9, 17) else None)


@pytest.mark.parametrize("key,s,variant", CASES, ids=[k + (" [f16]" if v else "") for k, _, v in CASES])
def test_case_against_the_oracle(key, s, variant):
    assert not _faulted, f"not run: the launch of {_faulted[0]} failed on the GPU"
    lib = _built(variant)
    d, o = rm.oracle(key, s)
    try:
        g, launch, read, rows_alone = _plan(lib, s, d)
        _lib.check(launch(), key, lib)
        torch.cuda.synchronize()
        first = {n: b.buf.clone() for n, b in g.items()}
        _lib.check(launch(), key, lib)
        torch.cuda.synchronize()
    except Exception:
        _faulted.append(key)
        raise
    for name, b in g.items():
        assert b.guards_intact(), f"{key}: a write outside the owned part of {name}"
        assert torch.equal(b.buf, first[name]), f"{key}: a second launch changed {name}"
    got = read()
    if s.kind == "gates":
        r = rm.gates_ratio(s, o, got)
        if s.seq_len:      # a row that takes no part keeps its bits
            kept = torch.from_numpy(rm.gates_lens(s)) <= s.step
            assert torch.equal(got[kept].view(torch.int32), d["h"][kept].view(torch.int32)), key
    elif s.kind == "step":
        r = rm.step_ratio(s, o, got)
    elif s.kind == "dec":      # decisions exactly the float64 decode's (a tie to the lower index, a tied bit 0), logits within the tolerance
        assert torch.equal(rm.dec_grid(got), o.grid), f"{key}: a decision differs from the float64 decode"
        if s.tie:
            a_root, a_bass = d["tied"]
            assert torch.equal(got.root[..., a_root], got.root[..., rm.TIE_B]) and torch.equal(got.bass[..., a_bass], got.bass[..., rm.TIE_B])
            assert torch.equal(got.chroma[:, :, 0, 0], got.chroma[:, :, 0, 1]), key
        r = rm.dec_ratio(s, o, got)
    elif s.kind == "pn":       # the library's own integer grid, and the lengths it implies, exactly the float64 decode's
        assert torch.equal(got.est, o.grid), f"{key}: the decoded grid differs from the float64 decode"
        assert torch.equal(rm.pn_grid(got), got.est), f"{key}: est is not the arg-max of the logits, ties to the lowest index"
        for a, b in d["pairs"]:
            assert torch.equal(got.pitch[..., a], got.pitch[..., b]) and int((got.est[..., 0] == b).sum()) == 0, (key, a, b)
        if s.tie:      # a tied duration bit is 0
            assert torch.equal(got.dur[..., 0], got.dur[..., 1]) and int(got.est[..., 1:].sum()) == 0, key
        r = rm.pn_ratio(s, o, got, est=got.est)
    else:
        assert bool(torch.isfinite(got.mu).all()), key
        r = rm.enc_ratio(s, o, got)
    print(f"rnn_matrix {key}{' [f16]' if variant else ''}: err/tol {r:.3f}")
    assert r <= 1.0, (key, r)
    if rows_alone is not None:
        try:
            alone = rows_alone()
        except Exception:
            _faulted.append(key)
            raise
        for row, bits in alone:
            if s.kind == "step":
                assert torch.equal(g["h_out"].body()[row].cpu(), bits), f"{key}: row {row} differs from the same row launched alone"
            else:
                for n, b in bits.items():
                    assert torch.equal(g[n].body()[row].cpu(), b), f"{key}: {n} of row {row} differs from the same row encoded alone"


def test_refused_arguments_leave_every_buffer_untouched():
    assert not _faulted, f"not run: the launch of {_faulted[0]} failed on the GPU"
    lib = _lib.load()
    n = 1 << 16
    out = Guarded(1, n, n)
    v = torch.ones(n + 64, device="cuda")
    ptr = lambda name: out.ptr if name == "out" else v.data_ptr()  # noqa: E731
    st = _lib.current_stream()
    for name, args in rm.refused_gates(ptr):
        assert lib.pf_gru_gates(*args, st) == -1, name
    for name, fields in rm.refused_step(ptr):
        a = _lib.GruStepArgs(**fields)
        assert lib.pf_gru_step(C.byref(a), st) == -1, name
    # a sequence longer than the workspace plan is sized for: 65 chord steps, 33 simultaneous notes
    for key, n_step in (("enc chord inp32 H32 z32 T1 B1", 65), ("enc pnotree emb16 Hn12 Ht20 z8 S3 B3", 33)):
        s = dict(rm.cases("enc"))[key]
        e = _encoder(s, rm.inputs(key, s)["state"])
        x = torch.zeros(s.b * 32 * 65 * 36, device="cuda")
        ws = e.workspace_for(lib.pf_encoder_workspace_bytes(e._h, s.b), x.device)
        rc = lib.pf_encoder_forward(e._h, x.data_ptr(), s.b, n_step, out.ptr, ws.data_ptr(), ws.numel(), st)
        assert rc == -1, (key, n_step, rc)
    torch.cuda.synchronize()
    assert out.guards_intact(body_too=True), "a refused call wrote to its output"
