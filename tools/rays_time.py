"""Time riggs_amd.pose_edit.fit_rays (one launch of csrc/rays.hip for all iterations) against fit_pose on the same rigs (targets: the
points the rays run through) and against the SAME iteration written in torch ops on the device (tools/fit_time.py's TorchFit with
the 3 x 3 metric per joint; no early stop of the CG, that would be a read-back).  Both forms of the kernel are timed: the rays in
registers (the default) and read again in every iteration (riggs_set_option("rays_reread", 1)).
Sizes: 24 joints with 2 and 8 cameras, 256 joints with 8 cameras; 32 iterations of 8 CG steps; batches B = 1 and B = 60.  The two
forms' results are compared first.  Device events around repeated calls, after a warm-up; milliseconds per call.  Needs the GPU.
Writes profiles/rays_times.json (or the path after --out)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from riggs_amd import _lib as L  # noqa: E402
from riggs_amd import pose_edit as PE  # noqa: E402
from pose_solve_common import make_problem, timed  # noqa: E402  (tools/ is the script's directory)
from fit_time import TorchFit  # noqa: E402


class TorchRays(TorchFit):
    """The iteration of include/riggs_hip.h (riggs_fit_rays) in torch ops: all weights 1, no pins, no locked joint, no translation."""

    def solve(self, q, gt, origins, d, iterations, cg_steps):
        cross = torch.linalg.cross
        eye = torch.eye(3, device=q.device)
        N = (eye - d[..., :, None] * d[..., None, :]).sum(2)          # (B, J, 3, 3)
        n = (N[..., 0, 0] + N[..., 1, 1] + N[..., 2, 2])[..., None] / 3.0
        for _ in range(iterations):
            GR, posed = self.fk(q, gt)
            pc = posed - posed[:, :1]
            pv = pc[:, self.vp]
            v = origins - posed[:, :, None]
            f = self.clamped(v - (v * d).sum(-1, keepdim=True) * d).sum(2)
            sums = self.subtree(torch.cat([f, cross(pc, f), n, n * pc, n * (pc * pc).sum(-1, keepdim=True)], -1))
            b = sums[..., 3:6] - cross(pv, sums[..., 0:3])
            dd = (sums[..., 10:11] - 2 * (pv * sums[..., 7:10]).sum(-1, keepdim=True) + (pv * pv).sum(-1, keepdim=True) * sums[..., 6:7]).clamp_min(0)
            minv = 1.0 / ((2.0 / 3.0) * dd + self.damping2)
            x, r = torch.zeros_like(b), b
            z = minv * r
            p = z
            rz = (r * z).sum((1, 2), keepdim=True)
            for k in range(cg_steps):
                WC = self.prefix(torch.cat([p, cross(p, pv)], -1))
                u = (N @ (cross(WC[..., 0:3], pc) - WC[..., 3:6])[..., None])[..., 0]
                FM = self.subtree(torch.cat([u, cross(pc, u)], -1))
                Ap = FM[..., 3:6] - cross(pv, FM[..., 0:3]) + self.damping2 * p
                pAp = (p * Ap).sum((1, 2), keepdim=True)
                alpha = torch.where(pAp > 0, rz / pAp.clamp_min(1e-38), torch.zeros_like(rz))
                x = x + alpha * p
                if k + 1 == cg_steps:
                    break
                r = r - alpha * Ap
                z = minv * r
                rzn = (r * z).sum((1, 2), keepdim=True)
                p = z + (rzn / rz.clamp_min(1e-38)) * p
                rz = rzn
            q = self.turn(q, GR, x)
        return q, self.fk(q, gt)[1]


def cameras(joints, K, seed):
    """K camera centres at 4 extents from the middle of the rig's box, on random axes."""
    rng = np.random.default_rng(seed)
    ax = rng.normal(0, 1, (K, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ext = float((joints.max(0) - joints.min(0)).max())
    return (0.5 * (joints.max(0) + joints.min(0)) + 4.0 * ext * ax).astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rays_times.json"))
    ap.add_argument("--reps", type=int, default=100, help="timed calls of fit_rays and fit_pose (the torch-op form takes a twentieth)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "rays_time.py measures on the GPU"
    dev = torch.device("cuda")
    iterations, cg_steps = 32, 8
    rows = []
    for J, K in ((24, 2), (24, 8), (256, 8)):
        for B in (1, 60):
            joints, parents, depth, q0, q1 = make_problem(J, B, 100 + J)
            ref = TorchRays(joints, parents, depth, dev)
            q0, gt = torch.tensor(q0, device=dev), torch.zeros(B, 3, device=dev)
            targets = ref.fk(torch.tensor(q1, device=dev), gt)[1].contiguous()
            cams = torch.tensor(cameras(joints, K, 7 + J), device=dev)
            origins = cams.expand(B, J, K, 3).contiguous()
            directions = (targets[:, :, None] - origins).contiguous()
            unit = directions / directions.norm(dim=-1, keepdim=True)
            rig = (ref.x, torch.tensor(parents, dtype=torch.int32, device=dev))
            pose = {"local_rotation": q0, "global_trans": gt}
            call = lambda: PE.fit_rays(rig, pose, origins, directions, iterations=iterations, cg_steps=cg_steps)  # noqa: E731
            out = call()
            tq, tn = ref.solve(q0, gt, origins, unit, iterations, cg_steps)
            row = {"J": J, "K": K, "iterations": iterations, "cg_steps": cg_steps, "B": B, "levels": len(ref.levels),
                   "max_abs_diff_d_nodes": float((out["d_nodes"] - tn).abs().max()),
                   "residual_over_extent": float(out["residual"].max() / PE.rig_extent(ref.x)),
                   "fit_rays_ms": timed(call, args.reps)}
            L.set_option("rays_reread", 1)
            try:
                row["same_bits_reread"] = all(bool(torch.equal(v, out[k])) for k, v in call().items())
                row["fit_rays_reread_ms"] = timed(call, args.reps)
            finally:
                L.set_option("rays_reread", 0)
            row["fit_pose_ms"] = timed(lambda: PE.fit_pose(rig, pose, targets, iterations=iterations, cg_steps=cg_steps), args.reps)
            row["torch_ops_ms"] = timed(lambda: ref.solve(q0, gt, origins, unit, iterations, cg_steps), max(2, args.reps // 20), warmup=1)
            row["over_fit_pose"] = row["fit_rays_ms"] / row["fit_pose_ms"]
            row["speedup"] = row["torch_ops_ms"] / row["fit_rays_ms"]
            print(json.dumps(row), flush=True)
            rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "what": "ms per call, device events; fit_rays = one launch of csrc/rays.hip "
                   "(plus torch's allocations, the default weights and the extent) with the rays in registers, fit_rays_reread = with "
                   "riggs_set_option('rays_reread', 1), fit_pose = csrc/fit.hip on the points the rays run through, torch_ops = the "
                   "same iteration in torch ops on the device", "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
