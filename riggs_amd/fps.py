"""Farthest-point sampling on csrc/fps.hip (utils/time_utils.py:461-482 of the reference, bit for bit — see the kernel's header
for the arithmetic and the tie rule): one launch per picked point, no host synchronisation, the start index read on the device."""
from __future__ import annotations

import torch

from . import _lib as L


def farthest_point_sample(xyz, npoint, start=None):
    """(B, N, 3) fp32 on the device -> (B, npoint) int64 indices, the start index first.  ``start`` (B,) fixes the first index
    (a tensor on the device is not synchronised on); ``None`` draws it with ``torch.randint`` as the reference does.  Batches
    run one after the other (the kernel takes one cloud)."""
    if xyz.dim() != 3 or xyz.shape[-1] != 3:
        raise L.RiggsHipError("farthest_point_sample takes (B, N, 3) points, got %s" % (tuple(xyz.shape),))
    if not xyz.is_cuda or xyz.dtype is not torch.float32:
        raise L.RiggsHipError("farthest_point_sample: xyz must be a float32 CUDA(HIP) tensor — there is no CPU path")
    B, N, _ = xyz.shape
    npoint = int(npoint)
    if N < 1 or npoint < 0:
        raise L.RiggsHipError("farthest_point_sample needs at least one point and npoint >= 0")
    dev = xyz.device
    xyz = xyz.detach()
    if xyz.stride(2) != 1 or (N > 1 and xyz.stride(1) < 3):
        xyz = xyz.contiguous()
    if start is None:
        cur = torch.randint(0, N, (B,), dtype=torch.long, device=dev)
    else:
        cur = torch.as_tensor(start, dtype=torch.long).to(dev).reshape(B).contiguous()
    out = torch.empty(B, npoint, dtype=torch.long, device=dev)
    if npoint == 0:
        return out
    lib = L.lib()
    ws = torch.empty(int(lib.riggs_fps_workspace_bytes(N)), dtype=torch.uint8, device=dev)
    row = xyz.stride(1) if N > 1 else 3
    with torch.cuda.device(dev):
        for b in range(B):
            L.check(lib.riggs_fps_sample(N, npoint, xyz[b].data_ptr(), row, cur[b:b + 1].data_ptr(), ws.data_ptr(),
                                         out[b].data_ptr(), L.stream_ptr()), "riggs_fps_sample")
    return out
