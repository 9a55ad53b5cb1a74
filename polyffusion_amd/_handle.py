"""The part every model handle of libpfhip.so shares: creation and destruction of the ``<prefix>_*`` handle, and its weights - the
reference ``state_dict`` packed on the host into ONE blob (``<prefix>_pack_param`` / ``_pack_missing``), then bound on the GPU."""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import Mapping, Optional, Tuple

import numpy as np
import torch

from . import _lib


class ModelHandle:
    PREFIX = ""   # "pf_unet", "pf_ddpm", "pf_encoder", "pf_decoder"

    def __init__(self, lib: C.CDLL, *create_args, device=None):
        self._lib = lib
        h = C.c_void_p()
        self._check(self._fn("create")(*create_args, C.byref(h)), f"{self.PREFIX}_create")
        self._h = h
        self.device = torch.device(device) if device is not None else (
            torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None)
        self._blob_dev: Optional[torch.Tensor] = None
        self._ws: Optional[torch.Tensor] = None

    def _fn(self, name: str):
        return getattr(self._lib, f"{self.PREFIX}_{name}")

    def _check(self, rc: int, what: str = "") -> int:
        return _lib.check(rc, what, self._lib)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._fn("destroy")(self._h)
                self._h = None
        except Exception:
            pass

    def workspace_for(self, nbytes: int, device) -> torch.Tensor:
        """The cached workspace, at least ``nbytes`` long and on ``device``: grown, or moved to another device, by dropping the old
        buffer before the new one is allocated."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != device:
            self._ws = None
            self._ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        return self._ws

    def param_shapes(self) -> "OrderedDict[str, Tuple[int, ...]]":
        """The parameter table in state_dict order (models with a ``<prefix>_param_info``)."""
        out: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
        buf = C.create_string_buffer(256)
        shape = (C.c_int64 * 4)()
        nd = C.c_int()
        for i in range(self._fn("n_params")(self._h)):
            self._check(self._fn("param_info")(self._h, i, buf, 256, shape, C.byref(nd)))
            out[buf.value.decode()] = tuple(int(shape[d]) for d in range(nd.value))
        return out

    def pack_param(self, key: str, val, blob: torch.Tensor) -> int:
        """Pack one tensor into the host blob; returns the library's code (PF_ENOTFOUND = -2 for a key this model does not have)."""
        t = torch.as_tensor(np.asarray(val) if not isinstance(val, torch.Tensor) else val).detach().to("cpu", torch.float32).contiguous()
        shape = (C.c_int64 * max(1, t.dim()))(*t.shape)
        return self._fn("pack_param")(self._h, key.encode(), t.data_ptr(), shape, t.dim(), blob.data_ptr())

    def pack_missing(self) -> Tuple[int, str]:
        buf = C.create_string_buffer(256)
        n = self._fn("pack_missing")(self._h, buf, 256)
        return n, buf.value.decode()

    def pack_state_dict(self, state: Mapping[str, object], strict: bool = True) -> torch.Tensor:
        """Repack reference-named tensors into the kernel-friendly host blob (no GPU needed).  ``strict=False`` skips unknown keys."""
        blob = torch.zeros(self.weight_bytes() // 4, dtype=torch.float32)
        for key, val in state.items():
            rc = self.pack_param(key, val, blob)
            if rc == -2 and not strict:
                continue
            self._check(rc, f"load_state_dict({key})")
        n, first = self.pack_missing()
        if n:
            raise RuntimeError(f"load_state_dict: {n} missing key(s), first: {first}")
        return blob

    def weight_bytes(self) -> int:
        return int(self._fn("weight_bytes")(self._h))

    def bind_packed(self, blob_dev: torch.Tensor):
        """Attach a packed blob that already lives on the GPU (e.g. received by RCCL broadcast)."""
        assert blob_dev.is_cuda and blob_dev.dtype == torch.float32 and blob_dev.numel() * 4 == self.weight_bytes()
        self._blob_dev = blob_dev
        self.device = blob_dev.device
        self._check(self._fn("bind_weights")(self._h, blob_dev.data_ptr()), f"{self.PREFIX}_bind_weights")

    def load_state_dict(self, state: Mapping[str, object], strict: bool = True):
        """Reference-compatible weight ingestion: pack on the host, copy to the GPU, bind."""
        _lib.require_gpu()
        self.bind_packed(self.pack_state_dict(state, strict).to(self.device))
        return self
