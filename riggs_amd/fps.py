"""Farthest-point sampling on csrc/fps.hip (utils/time_utils.py:461-482 of the reference, bit for bit — see the kernel's header
for the arithmetic and the tie rule): one launch per picked point, no host synchronisation, the start index read on the device.
``farthest_point_sample`` takes clouds of 3-vectors, ``farthest_point_sample_rows`` rows of 1 to 64 floats (the stage-1 node
sampling over trajectories)."""
from __future__ import annotations

import torch

from . import _lib as L

MAX_WIDTH = 64  # FPS_MAX_WIDTH of csrc/fps.hip


def _sweep(name, x, npoint, start, rows):
    """The checks and the launch loop both samplers share; ``rows``: the wide entry (any width) instead of the 3-column one."""
    if not x.is_cuda or x.dtype is not torch.float32:
        raise L.RiggsHipError("%s: the points must be a float32 CUDA(HIP) tensor — there is no CPU path" % name)
    B, N, D = x.shape
    npoint = int(npoint)
    if N < 1 or npoint < 0:
        raise L.RiggsHipError("%s needs at least one point and npoint >= 0" % name)
    dev = x.device
    x = x.detach()
    if x.stride(2) != 1 or (N > 1 and x.stride(1) < D):
        x = x.contiguous()
    if start is None:
        cur = torch.randint(0, N, (B,), dtype=torch.long, device=dev)
    else:
        cur = torch.as_tensor(start, dtype=torch.long).to(dev).reshape(B).contiguous()
    out = torch.empty(B, npoint, dtype=torch.long, device=dev)
    if npoint == 0:
        return out
    lib = L.lib()
    nbytes = lib.riggs_fps_rows_workspace_bytes(N, D) if rows else lib.riggs_fps_workspace_bytes(N)
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    row = x.stride(1) if N > 1 else D
    with torch.cuda.device(dev):
        for b in range(B):
            tail = (x[b].data_ptr(), row, cur[b:b + 1].data_ptr(), ws.data_ptr(), out[b].data_ptr(), L.stream_ptr())
            if rows:
                L.check(lib.riggs_fps_sample_rows(N, D, npoint, *tail), "riggs_fps_sample_rows")
            else:
                L.check(lib.riggs_fps_sample(N, npoint, *tail), "riggs_fps_sample")
    return out


def farthest_point_sample(xyz, npoint, start=None):
    """(B, N, 3) fp32 on the device -> (B, npoint) int64 indices, the start index first.  ``start`` (B,) fixes the first index
    (a tensor on the device is not synchronised on); ``None`` draws it with ``torch.randint`` as the reference does.  Batches
    run one after the other (the kernel takes one cloud)."""
    if xyz.dim() != 3 or xyz.shape[-1] != 3:
        raise L.RiggsHipError("farthest_point_sample takes (B, N, 3) points, got %s" % (tuple(xyz.shape),))
    return _sweep("farthest_point_sample", xyz, npoint, start, rows=False)


def farthest_point_sample_rows(rows, npoint, start=None):
    """(B, N, D) fp32 on the device, 1 <= D <= 64 -> (B, npoint) int64 indices, the start index first: the same sweep with the
    squared distance summed over the D columns in ascending order (at D = 3 the indices of ``farthest_point_sample``).  ``start``,
    strides (rows that are a view of wider ones are read in place), batches and ``npoint == 0`` as there."""
    if rows.dim() != 3 or not 1 <= rows.shape[-1] <= MAX_WIDTH:
        raise L.RiggsHipError("farthest_point_sample_rows takes (B, N, D) rows with 1 <= D <= %d, got %s" % (MAX_WIDTH, tuple(rows.shape)))
    return _sweep("farthest_point_sample_rows", rows, npoint, start, rows=True)
