"""What finding the nearest corpus windows of a batch of rolls costs: ``pf_roll_match`` against the same result from torch alone.

    python tools/bench_rollmatch.py [--reps 7] [--nb 65536]

prints ONE JSON line.  Workload: ``na = 16`` queries, ``shifts = 6`` (13 transpositions), ``steps = 128``, ``nb`` corpus windows of random
rows of density 0.03, ``topk = 3``.  The corpus is stored as a ``Corpus`` is: one run of rows with a window every ``hop`` rows
(``--hop 16``, so neighbouring windows share rows; ``--hop 128`` stores every window on its own).
  * ``kernel_ms``: milliseconds per ``pf_roll_match`` call (three launches), the median of ``--reps`` windows of ``--calls`` calls each
    between two device events, after a warm-up; ``word_pairs_per_s``: na * 13 * nb * 512 word pairs over that time;
  * ``vector_bound_frac``: that rate as a fraction of the vector bound - 2 lane-ops (AND, accumulating popcount) per word pair against
    CUs * 4 SIMDs * 32 lanes per clock at the measured shader clock (``sclk_mhz``);
  * ``corpus_bytes_per_s``: the bytes of the windows (nb * steps * 16, each counted once per call) over the call's time, and
    ``stored_bytes`` what is actually resident; ``hbm_frac`` against 6.29e12 B/s, the measured copy rate of the part;
  * ``torch_ms``: the same top-k lists from torch alone on the same GPU - rolls unpacked to 0/1 bf16, one ``matmul`` per shift with fp32
    accumulation (exact: counts stay below 2^24), the ordering as float64 fractions (exact for counts this small: distinct fractions of
    integers below 2^14 differ by more than 2^-28) - and ``torch_equal`` whether its lists equal the kernel's; ``speedup_vs_torch``;
  * ``numpy_ms_scaled``: the numpy restatement (tests/rollmatch_ref.py) on ``--numpy_nb`` windows and 2 queries, scaled linearly to the
    workload (``numpy_scaled: true``).
Nothing is asserted and no threshold is set; the line is copied to profiles/rollmatch_bench.json and quoted in DESIGN.md."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from polyffusion_amd import _lib, rollmatch  # noqa: E402
from tools.bench_invert import ClockProbe  # noqa: E402

HBM_MEASURED = 6.29e12


def windows_ms(fn, reps: int, calls: int) -> float:
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    return statistics.median(ms)


def unpack(plane: torch.Tensor) -> torch.Tensor:
    """int32 ``[rows, 4]`` -> bool ``[rows, 128]``"""
    bit = torch.arange(32, device=plane.device, dtype=torch.int32)
    return ((plane.unsqueeze(-1) >> bit) & 1).bool().reshape(plane.shape[0], 128)


FORMULATION = {"name": "bf16 operands, fp32 result (torch.mm out_dtype)"}


def mm_f32(a_bf16: torch.Tensor, b_bf16: torch.Tensor) -> torch.Tensor:
    """a @ b.T of 0/1 bf16 operands with an fp32 result (a bf16 result would round counts above 256); where this torch has no such GEMM,
    fp32 operands - recorded in the line as ``torch_formulation``."""
    if FORMULATION["name"].startswith("bf16"):
        try:
            return torch.mm(a_bf16, b_bf16.t(), out_dtype=torch.float32)
        except (TypeError, RuntimeError, NotImplementedError):
            FORMULATION["name"] = "fp32 operands (this torch has no bf16 GEMM with an fp32 result)"
    return torch.mm(a_bf16.float(), b_bf16.float().t())


def torch_match(q_rows: torch.Tensor, c_rows: torch.Tensor, a_starts, b_starts, steps: int, shifts: int, topk: int):
    """The top-k lists from torch alone: 0/1 bf16 matmul per shift.  ``q_rows`` / ``c_rows`` bool ``[rows, 128]``."""
    t = torch.arange(steps, device=q_rows.device)
    q = q_rows[(a_starts.long()[:, None] + t)]                               # [na, steps, 128]
    c = c_rows[(b_starts.long()[:, None] + t)].reshape(len(b_starts), -1)     # [nb, steps * 128]
    cb = c.to(torch.bfloat16)
    csize = c.sum(1, dtype=torch.int64)
    best_j = best_i = best_u = best_s = None
    for k in range(2 * shifts + 1):
        s = -((k + 1) // 2) if k % 2 else k // 2
        qs = torch.zeros_like(q)
        if s >= 0:
            qs[:, :, :128 - s] = q[:, :, s:]
        else:
            qs[:, :, -s:] = q[:, :, :128 + s]
        qs = qs.reshape(len(a_starts), -1)
        inter = mm_f32(qs.to(torch.bfloat16), cb).long()
        union = qs.sum(1, dtype=torch.int64)[:, None] + csize[None] - inter
        j = torch.where(union > 0, inter.double() / union.clamp(min=1).double(), torch.zeros((), dtype=torch.float64, device=q.device))
        if best_j is None:
            best_j, best_i, best_u, best_s = j, inter, union, torch.full_like(inter, s)
        else:
            up = j > best_j
            best_j, best_i, best_u = torch.where(up, j, best_j), torch.where(up, inter, best_i), torch.where(up, union, best_u)
            best_s = torch.where(up, torch.full_like(inter, s), best_s)
    order = torch.sort(best_j, dim=1, descending=True, stable=True).indices[:, :topk]
    return order.int(), best_s.gather(1, order).int(), best_i.gather(1, order).int(), best_u.gather(1, order).int()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--na", type=int, default=16)
    ap.add_argument("--nb", type=int, default=65536)
    ap.add_argument("--shifts", type=int, default=6)
    ap.add_argument("--hop", type=int, default=16)
    ap.add_argument("--numpy_nb", type=int, default=256)
    ap.add_argument("--seed", type=int, default=1234)
    a = ap.parse_args(argv)
    _lib.require_gpu()
    lib = _lib.load()
    steps, topk, dens = 128, 3, 0.03
    rng = np.random.default_rng(a.seed)
    rows_b = (a.nb - 1) * a.hop + steps
    c_rows = rng.random((rows_b, 128)) < dens
    q_rows = rng.random((a.na * steps, 128)) < dens
    pack = lambda r: np.ascontiguousarray(np.packbits(r, axis=-1, bitorder="little")).view("<u4").view(np.int32)
    b_bits, a_bits = torch.from_numpy(pack(c_rows)).cuda(), torch.from_numpy(pack(q_rows)).cuda()
    b_starts = torch.arange(a.nb, dtype=torch.int32, device="cuda") * a.hop
    a_starts = torch.arange(a.na, dtype=torch.int32, device="cuda") * steps
    out = rollmatch.match_windows(a_bits, a_starts, b_bits, b_starts, steps, a.shifts, topk)
    ws = torch.empty(int(lib.pf_roll_match_workspace_bytes(a.na, a.nb, topk)), dtype=torch.uint8, device="cuda")
    kernel = lambda: rollmatch.match_windows(a_bits, a_starts, b_bits, b_starts, steps, a.shifts, topk, out=out, workspace=ws)
    probe = ClockProbe(lib)
    probe.begin()
    ms = windows_ms(kernel, a.reps, a.calls)
    mhz = probe.end_mhz()
    pairs = a.na * (2 * a.shifts + 1) * a.nb * steps * 4
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"what": "pf_roll_match: nearest corpus windows under transposition, against torch alone (0/1 bf16 matmul per shift) and numpy",
           "device": torch.cuda.get_device_properties(0).name, "cus": cus, "na": a.na, "nb": a.nb, "shifts": a.shifts, "steps": steps, "topk": topk,
           "hop": a.hop, "density": dens, "reps": a.reps, "calls_per_window": a.calls, "sclk_mhz": mhz,
           "kernel_ms": round(ms, 4), "word_pairs": pairs, "word_pairs_per_s": round(pairs / (ms * 1e-3), 1)}
    if mhz:
        res["vector_bound_frac"] = round(2 * pairs / (ms * 1e-3) / (cus * 4 * 32 * mhz * 1e6), 4)
    win_bytes = a.nb * steps * 16
    res.update(corpus_bytes_per_s=round(win_bytes / (ms * 1e-3), 1), stored_bytes=int(b_bits.numel() * 4),
               hbm_frac=round(win_bytes / (ms * 1e-3) / HBM_MEASURED, 4))
    # torch alone
    qb, cbool = unpack(a_bits), unpack(b_bits)
    tfn = lambda: torch_match(qb, cbool, a_starts, b_starts, steps, a.shifts, topk)
    tout = tfn()
    res["torch_equal"] = all(bool(torch.equal(x, y)) for x, y in zip(tout, (out.index, out.shift, out.inter, out.union)))
    tms = windows_ms(tfn, max(3, a.reps // 2), 1)
    res.update(torch_ms=round(tms, 3), speedup_vs_torch=round(tms / ms, 2), torch_formulation=FORMULATION["name"])
    # numpy restatement, scaled
    import rollmatch_ref as ref
    nq, nbs = 2, min(a.numpy_nb, a.nb)
    qw = ref.windows(q_rows, [0, steps], steps)
    cw = ref.windows(c_rows, [i * a.hop for i in range(nbs)], steps)
    t0 = time.perf_counter()
    want = ref.match(qw, cw, a.shifts, topk)
    sec = time.perf_counter() - t0
    small = rollmatch.match_windows(a_bits, a_starts[:nq].contiguous(), b_bits, b_starts[:nbs].contiguous(), steps, a.shifts, topk)
    res.update(numpy_ms_scaled=round(sec * 1e3 * (a.na / nq) * (a.nb / nbs), 1), numpy_scaled=True, numpy_windows=nbs, numpy_queries=nq,
               numpy_equal=all(np.array_equal(getattr(small, k).cpu().numpy(), want[k]) for k in ("index", "shift", "inter", "union")))
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
