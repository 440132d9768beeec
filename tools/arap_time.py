"""Time riggs_amd.arap (one launch of csrc/arap.hip per drag or per batch of drags) against the SAME iteration written in torch ops on
the device as the reference writes it: ``torch.linalg.lstsq`` on the N x (N - M) matrix per solve (four per drag), a batched 3 x 3
``torch.linalg.svd`` with the Kabsch flip per round.  Shapes (N, M) = (512, 4) and (1024, 8), K = 16, one drag and 60 batched drags
(the torch form solves the 60 as 180 right-hand-side columns of one lstsq).  The two forms' results are compared first.  The
per-click cost — the float64 pseudo-inverse of a new handle set — is timed once, apart.  Device events around repeated calls, after
a warm-up; milliseconds per call.  A measurement to record, not a bar.  Needs the GPU.
Writes profiles/arap_times.json (or the path after --out)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from riggs_amd import arap as AR  # noqa: E402
from pose_solve_common import timed  # noqa: E402  (tools/ is the script's directory)


def torch_drag(d, handles, handle_pos, iterations=3):
    """``handle_pos`` (B, M, 3) -> positions (B, N, 3): the reference's deform() in batched torch ops on the device."""
    N, K, B = d.N, d.K, handle_pos.shape[0]
    A = d.laplacian(torch.float32)
    h = torch.tensor(handles, device=A.device)
    free = torch.ones(N, dtype=torch.bool, device=A.device)
    free[h] = False
    Au, Ah = A[:, free], A[:, h]
    kept = (d.nn_idx >= 0)
    j = d.nn_idx.long().clamp_min(0)
    w = d.weight
    p0 = d.verts

    def solve(b):  # (B, N, 3) -> (B, N, 3): lstsq_with_handles
        rhs = (b - torch.einsum("nm,bmc->bnc", Ah, handle_pos)).permute(1, 0, 2).reshape(N, B * 3)
        xu = torch.linalg.lstsq(Au, rhs).solution.reshape(-1, B, 3).permute(1, 0, 2)
        x = torch.empty(B, N, 3, device=A.device)
        x[:, free] = xu
        x[:, h] = handle_pos
        return x

    P = (p0[:, None] - p0[j]) * kept[..., None]
    x = solve((A @ p0)[None].expand(B, N, 3))
    for _ in range(iterations):
        Q = (x[:, :, None] - x[:, j]) * kept[None, ..., None]
        S = torch.einsum("nk,nka,bnkc->bnac", w, P, Q)
        U, sig, Vh = torch.linalg.svd(S)
        R = Vh.transpose(-1, -2) @ U.transpose(-1, -2)
        flip = torch.linalg.det(R) <= 0
        Um = U.clone()
        col = torch.nn.functional.one_hot(sig.argmin(-1), 3).bool() & flip[..., None]
        Um = torch.where(col[..., None, :], -Um, Um)
        R = Vh.transpose(-1, -2) @ Um.transpose(-1, -2)
        b = 0.5 * torch.einsum("nk,bnkrc,nkc->bnr", w, (R[:, :, None] + R[:, j]) * kept[None, ..., None, None], P)
        x = solve(b)
    return x


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "arap_times.json"))
    ap.add_argument("--reps", type=int, default=50, help="timed calls of the library (the torch-op form takes a tenth)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "arap_time.py measures on the GPU"
    dev = torch.device("cuda")
    rows = []
    for N, M in ((512, 4), (1024, 8)):
        g = torch.Generator().manual_seed(N)
        verts = (0.3 * torch.randn(N, 3, generator=g)).to(dev)
        tool = AR.LapDeform(verts)
        d = tool.arap_deformer
        handles = torch.randperm(N, generator=g)[:M].tolist()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, null_dims = d.operator(handles)
        torch.cuda.synchronize()
        click_ms = (time.perf_counter() - t0) * 1e3
        for B in (1, 60):
            hp = (verts[handles][None] + 0.1 * torch.randn(B, M, 3, generator=g).to(dev)).contiguous()
            out = d.deform_batch(handles, hp)
            row = {"N": N, "M": M, "K": d.K, "B": B, "dropped_edges": int((d.nn_idx < 0).sum()), "null_dims": null_dims,
                   "new_handle_set_ms": click_ms, "arap_ms": timed(lambda: d.deform_batch(handles, hp, return_R=True), args.reps)}
            try:
                ref = torch_drag(d, handles, hp)
                row["max_abs_diff"] = float((out - ref).abs().max())
                row["torch_ops_ms"] = timed(lambda: torch_drag(d, handles, hp), max(3, args.reps // 10))
                row["speedup"] = row["torch_ops_ms"] / row["arap_ms"]
            except RuntimeError as e:  # (a device without lstsq / svd kernels: say so instead of a number)
                row["torch_ops_ms"], row["torch_ops_error"] = None, str(e).splitlines()[0][:200]
            print(json.dumps(row), flush=True)
            rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f_:
        json.dump({"device": torch.cuda.get_device_name(0), "what": "ms per call, device events around repeated calls after a warm-up; arap = one "
                   "launch of csrc/arap.hip (plus torch's allocations) for B drags with rotations, torch_ops = the reference's iteration in "
                   "torch ops on the device (torch.linalg.lstsq per solve, batched torch.linalg.svd per round); new_handle_set_ms = the "
                   "float64 pseudo-inverse of a new handle set, host clock, once per click", "rows": rows}, f_, indent=1)


if __name__ == "__main__":
    main()
