"""ctypes binding of libriggs_hip.so.  Every signature, struct and constant is read from include/riggs_hip.h (riggs_amd/_abi.py):
a function added to the header and to the library is callable from here with no further edit.

The product path has NO fallback: if the HIP library is missing or fails to load,
every op raises.  PyTorch is used only for device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os

from ._abi import CONSTANTS, STRUCTS
from ._abi import FUNCTIONS as _SIGS  # name -> (restype, argtypes)

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "lib", "libriggs_hip.so")

# the header's enumerators of the arena layouts under their short names: RIGGS_GEOM_XYD -> GEOM_XYD, RIGGS_GEOM_NFIELDS_ -> GEOM_NFIELDS
globals().update({k[len("RIGGS_"):].rstrip("_"): v for k, v in CONSTANTS.items() if k.startswith(("RIGGS_GEOM_", "RIGGS_IMG_", "RIGGS_BIN_"))})
ABI_VERSION = CONSTANTS["RIGGS_ABI_VERSION"]

RasterCfg, Frame, FrameGrads = STRUCTS["riggs_raster_cfg"], STRUCTS["riggs_frame"], STRUCTS["riggs_frame_grads"]
MlpEpilogue, GateStruct = STRUCTS["riggs_mlp_epilogue"], STRUCTS["riggs_gate"]
NodeMlp, NodeMlpGrads = STRUCTS["riggs_node_mlp"], STRUCTS["riggs_node_mlp_grads"]
ViewerProjection, ViewerFrame = STRUCTS["riggs_viewer_projection"], STRUCTS["riggs_viewer_frame"]


class Watch:
    """A non-blocking look at one 32-bit device word, for callers that must not synchronise (an eagerly issued training
    iteration is bound by the host: a blocking read per iteration would expose the whole queue's latency).  Every ``period``-th
    ``poll`` enqueues an asynchronous copy of the word into pinned host memory behind the work issued so far; a poll returns the
    most recent value whose copy has landed (0 until then).  Never call it while the current stream is being captured."""

    def __init__(self, period: int = 16):
        self.period, self.n, self.event, self.host, self.value = int(period), 0, None, None, 0

    def poll(self, tensor, index: int) -> int:
        import torch
        if self.event is not None and self.event.query():
            self.value, self.event = int(self.host[0]), None
        self.n += 1
        if self.event is None and self.n % self.period == 0:
            if self.host is None:
                self.host = torch.zeros(1, dtype=tensor.dtype).pin_memory()
            self.host.copy_(tensor[index:index + 1], non_blocking=True)
            self.event = torch.cuda.Event()
            self.event.record()
        return self.value


class FrameGate:
    """A frame's "valid" gate (include/riggs_hip.h: riggs_gate): up to RIGGS_GATE_MAX (device word, mask) pairs — the sticky status word
    of the one-launch PoseMLP kernels, the rasterizer's overflow / sort-barrier flags, the gradient-row exchange's status —
    that the consumers of the frame's gradients (the fused Adam, the exchange's pack) read ON THE DEVICE: a frame that went
    wrong is a skipped step, also inside a hipGraph where the host cannot look first.  ``sources``: callables returning
    ``(int32 / uint32 device tensor, word index, mask)`` or None, resolved at every launch (the rasterizer's counters are a
    new tensor per frame until a capture pins them).  ``skipped`` counts the steps the gate turned into no-ops."""

    def __init__(self, sources=(), device=None):
        import torch
        self.sources = list(sources)
        self.skipped = torch.zeros(1, dtype=torch.int32, device=device or "cuda")
        self._keep = []

    def struct(self):
        g = GateStruct()
        keep, n = [], 0
        for src in self.sources:
            got = src()
            if got is None:
                continue
            t, index, mask = got
            if not (t.is_cuda and t.element_size() == 4 and t.is_contiguous() and 0 <= index < t.numel()):
                raise RiggsHipError("a gate word must be an element of a contiguous 32-bit device tensor")
            if n >= len(g.word):
                raise RiggsHipError("at most %d gate words" % len(g.word))
            g.word[n] = t.data_ptr() + 4 * int(index)
            g.mask[n] = int(mask) & 0xFFFFFFFF
            keep.append(t)
            n += 1
        g.n = n
        self._keep = keep  # the words outlive the launches that were handed their addresses
        return g

    def read_skipped(self, clear=True) -> int:
        n = int(self.skipped.item())
        if clear and n:
            self.skipped.zero_()
        return n


_lib = None


class RiggsHipError(RuntimeError):
    pass


def lib():
    """Load libriggs_hip.so; raise loudly when it is absent (no CPU/eager fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise RiggsHipError(
                "libriggs_hip.so not found at %s — build it with `python -m riggs_amd.build` "
                "(or __graft_entry__.build()).  There is no fallback path." % SO_PATH)
        # (torch's HIP runtime first: a process whose first HIP activity is this library's load — its kernels register with
        # the runtime from static initialisers — and which initialises torch.cuda afterwards ends with the library's launches
        # failing "no ROCm-capable device is detected"; the other order is the one every caller that allocates a tensor
        # before its first call takes anyway)
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
        L = C.CDLL(SO_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)  # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if L.riggs_version() != ABI_VERSION:
            raise RiggsHipError("%s was built for ABI version %d, include/riggs_hip.h declares %d: rebuild it (`python -m riggs_amd.build`)"
                                % (SO_PATH, L.riggs_version(), ABI_VERSION))
        _lib = L
    return _lib


def set_option(name: str, value: int):
    """riggs_set_option: the option names, their defaults and meanings are listed in include/riggs_hip.h; unknown names fail."""
    check(lib().riggs_set_option(name.encode(), int(value)), "riggs_set_option")
    OPTIONS_SET[name] = int(value)


OPTIONS_SET = {}  # what this process set through set_option (host-side decisions that follow an option read it here: no C call per frame)


def get_option(name: str) -> int:
    v = C.c_int32()
    check(lib().riggs_get_option(name.encode(), C.byref(v)), "riggs_get_option")
    return int(v.value)


def exported_symbols():
    return sorted(_SIGS.keys())


def check(rc: int, what: str):
    if rc != 0:
        msg = lib().riggs_last_error().decode(errors="replace")
        raise RiggsHipError("%s failed (rc=%d): %s" % (what, rc, msg))


def ptr(t):
    """Device pointer of a tensor (or None -> NULL)."""
    return None if t is None else t.data_ptr()


def stream_ptr():
    """The current HIP stream of the current device as an integer handle (torch._C's raw accessor: ~0.3 us instead of the
    ~15 us of building a torch.cuda.Stream object — three of those per eager frame were 7 % of its host time)."""
    import torch
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    if raw is not None:
        return raw(torch._C._cuda_getDevice())
    return torch.cuda.current_stream().cuda_stream


_F32 = None


def require_cuda_f32(name, t, shape=None):
    global _F32
    if t is None:
        return None
    if _F32 is None:
        import torch
        _F32 = torch.float32
    if not t.is_cuda:
        raise RiggsHipError("%s must be a CUDA(HIP) tensor — the product path is GPU-only" % name)
    if t.dtype is not _F32:
        raise RiggsHipError("%s must be float32, got %s" % (name, t.dtype))
    if shape is not None:
        ts = t.shape
        ok = len(shape) == len(ts)
        if ok:
            for s, d in zip(shape, ts):
                if s is not None and s != d:
                    ok = False
                    break
        if not ok:
            raise RiggsHipError("%s has shape %s, expected %s" % (name, tuple(ts), shape))
    return t if t.is_contiguous() else t.contiguous()
