"""Sentinel-guarded device buffers shared by the GPU matrices (tests/test_gpu_conv_matrix.py, tests/test_gpu_attn_matrix.py): what a launch
writes lives inside a larger tensor prefilled with a NaN bit pattern, and every element the launch does not own must keep it."""
import torch

GUARD = 4096            # guard elements in front of and behind every guarded buffer (a multiple of 64: 16-byte stores stay aligned)
SENTINEL32 = 0x7FC0BEEF  # a NaN: an owned element the launch leaves out fails its comparison
SENTINEL16 = 0x7E5B      # fp16: a NaN; bf16: 4.5e37


class Guarded:
    """rows x ld elements of which the first `cols` of every row are the launch's; sentinel everywhere, guards on both sides"""

    def __init__(self, rows, ld, cols, bits=32):
        self.rows, self.ld, self.cols = rows, ld, cols
        self.dt, self.sentinel = (torch.int32, SENTINEL32) if bits == 32 else (torch.int16, SENTINEL16)
        self.buf = torch.full((2 * GUARD + rows * ld,), self.sentinel, dtype=self.dt, device="cuda")

    @property
    def ptr(self):
        return self.buf.data_ptr() + GUARD * self.buf.element_size()

    def body(self):
        return self.buf[GUARD:GUARD + self.rows * self.ld].view(self.rows, self.ld)

    def guards_intact(self, body_too=False):
        ok = bool((self.buf[:GUARD] == self.sentinel).all()) and bool((self.buf[GUARD + self.rows * self.ld:] == self.sentinel).all())
        if self.cols < self.ld:
            ok = ok and bool((self.body()[:, self.cols:] == self.sentinel).all())
        return ok and (not body_too or bool((self.body() == self.sentinel).all()))


def _dev(t):
    """a host tensor on the device, with 256 bytes of slack behind it"""
    flat = t.contiguous().reshape(-1)
    buf = torch.zeros(flat.numel() + 256 // flat.element_size(), dtype=flat.dtype, device="cuda")
    buf[:flat.numel()] = flat.cuda()
    return buf
