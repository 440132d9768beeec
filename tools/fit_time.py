"""Time riggs_amd.pose_edit.fit_pose (one launch of csrc/fit.hip for all iterations) against the SAME iteration written in torch ops
on the device: the level-by-level chain, the two tree sweeps per conjugate-gradient step, the preconditioner and the quaternion
update, with the topology (levels, parents) prepared once on the host.  The torch form has no early stop of the CG (that would be
a read-back); where p.Ap <= 0 its step is zero.
Sizes: J = 24 and J = 256, 32 iterations of 8 CG steps, batches B = 1 and B = 60.  The two forms' results are compared first.
Device events around repeated calls, after a warm-up; milliseconds per call.  Needs the GPU.
Writes profiles/fit_times.json (or the path after --out)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from riggs_amd import pose_edit as PE  # noqa: E402
from pose_solve_common import TorchChain, make_problem, timed  # noqa: E402  (tools/ is the script's directory)


class TorchFit(TorchChain):
    """The iteration of include/riggs_hip.h (riggs_fit_pose) in torch ops, all weights 1, no locked joint, no translation."""

    def prefix(self, v):
        v = v.clone()
        for idx, p in zip(self.levels, self.level_parents):
            v[:, idx] = v[:, p] + v[:, idx]
        return v

    def subtree(self, v):
        v = v.clone()
        for idx, p in zip(reversed(self.levels), reversed(self.level_parents)):
            v.index_add_(1, p, v[:, idx])
        return v

    def solve(self, q, gt, targets, iterations, cg_steps):
        cross = torch.linalg.cross
        for _ in range(iterations):
            GR, posed = self.fk(q, gt)
            pc = posed - posed[:, :1]
            pv = pc[:, self.vp]
            rr = self.clamped(targets - posed)
            sums = self.subtree(torch.cat([rr, cross(pc, rr), torch.ones_like(pc[..., :1]), pc, (pc * pc).sum(-1, keepdim=True)], -1))
            b = sums[..., 3:6] - cross(pv, sums[..., 0:3])
            dd = (sums[..., 10:11] - 2 * (pv * sums[..., 7:10]).sum(-1, keepdim=True) + (pv * pv).sum(-1, keepdim=True) * sums[..., 6:7]).clamp_min(0)
            minv = 1.0 / ((2.0 / 3.0) * dd + self.damping2)
            x, r = torch.zeros_like(b), b
            z = minv * r
            p = z
            rz = (r * z).sum((1, 2), keepdim=True)
            for k in range(cg_steps):
                WC = self.prefix(torch.cat([p, cross(p, pv)], -1))
                u = cross(WC[..., 0:3], pc) - WC[..., 3:6]
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_times.json"))
    ap.add_argument("--reps", type=int, default=100, help="timed calls of fit_pose (the torch-op form takes a twentieth)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "fit_time.py measures on the GPU"
    dev = torch.device("cuda")
    iterations, cg_steps = 32, 8
    rows = []
    for J in (24, 256):
        for B in (1, 60):
            joints, parents, depth, q0, q1 = make_problem(J, B, 100 + J)
            ref = TorchFit(joints, parents, depth, dev)
            q0, gt = torch.tensor(q0, device=dev), torch.zeros(B, 3, device=dev)
            targets = ref.fk(torch.tensor(q1, device=dev), gt)[1].contiguous()
            rig = (ref.x, torch.tensor(parents, dtype=torch.int32, device=dev))
            pose = {"local_rotation": q0, "global_trans": gt}
            call = lambda: PE.fit_pose(rig, pose, targets, iterations=iterations, cg_steps=cg_steps)  # noqa: E731
            out = call()
            tq, tn = ref.solve(q0, gt, targets, iterations, cg_steps)
            row = {"J": J, "iterations": iterations, "cg_steps": cg_steps, "B": B, "levels": len(ref.levels),
                   "max_abs_diff_d_nodes": float((out["d_nodes"] - tn).abs().max()),
                   "residual_over_extent": float(out["residual"].max() / PE.rig_extent(ref.x)),
                   "fit_pose_ms": timed(call, args.reps),
                   "torch_ops_ms": timed(lambda: ref.solve(q0, gt, targets, iterations, cg_steps), max(2, args.reps // 20), warmup=1)}
            row["speedup"] = row["torch_ops_ms"] / row["fit_pose_ms"]
            print(json.dumps(row), flush=True)
            rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "what": "ms per call, device events; fit_pose = one launch of csrc/fit.hip "
                   "(plus torch's allocations and the extent), torch_ops = the same iteration in torch ops on the device", "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
