"""Time riggs_amd.pose_edit.fit_bones (one launch of csrc/bones.hip for all iterations) against the SAME iteration written in torch
ops on the device: the level-by-level chain, the two tree sweeps of 3 values per conjugate-gradient step, the preconditioner and
the quaternion update, with the topology (levels, parents) prepared once on the host.  The torch form has no early stop of the CG
(that would be a read-back); where p.Ap <= 0 its step is zero.  fit_pose runs on the same rigs and poses for scale: its sweeps
carry 6 values where fit_bones's carry 3.
Sizes: J = 24 and J = 256, 32 iterations of 8 CG steps, batches B = 1 and B = 60.  The targets are the bones of a second pose on a
copy of the rig with other bone lengths.  The two forms' results are compared first.
Device events around repeated calls, after a warm-up; milliseconds per call.  Needs the GPU.
Writes profiles/bones_times.json (or the path after --out)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from riggs_amd import pose_edit as PE  # noqa: E402
from pose_solve_common import TorchChain, make_problem, timed  # noqa: E402  (tools/ is the script's directory)

DAMPING, MAX_STEP = 0.05, 0.5


class TorchBones(TorchChain):
    """The iteration of include/riggs_hip.h (riggs_fit_bones) in torch ops, all weights 1, no locked joint."""

    def __init__(self, joints, parents, depth, dev):
        super().__init__(joints, parents, depth, dev)
        self.damping2 = torch.tensor(DAMPING * DAMPING, device=dev)
        self.max_step = torch.tensor(MAX_STEP, device=dev)
        self.s = torch.ones(1, self.J, 1, device=dev)
        self.s[:, 0] = 0
        self.minv = 1.0 / ((2.0 / 3.0) * self.subtree(self.s * self.s) + self.damping2)

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

    def bones(self, posed):
        beta = posed - posed[:, self.vp]
        return self.s * beta / beta.norm(dim=-1, keepdim=True).clamp_min(1e-30)

    def solve(self, q, gt, t, iterations, cg_steps):
        cross = torch.linalg.cross
        for _ in range(iterations):
            GR, posed = self.fk(q, gt)
            d = self.bones(posed)
            b = self.subtree(cross(d, self.s * self.clamped(t - d)))
            x, r = torch.zeros_like(b), b
            z = self.minv * r
            p = z
            rz = (r * z).sum((1, 2), keepdim=True)
            for k in range(cg_steps):
                Ap = self.subtree(cross(d, cross(self.prefix(p), d))) + self.damping2 * p
                pAp = (p * Ap).sum((1, 2), keepdim=True)
                alpha = torch.where(pAp > 0, rz / pAp.clamp_min(1e-38), torch.zeros_like(rz))
                x = x + alpha * p
                if k + 1 == cg_steps:
                    break
                r = r - alpha * Ap
                z = self.minv * r
                rzn = (r * z).sum((1, 2), keepdim=True)
                p = z + (rzn / rz.clamp_min(1e-38)) * p
                rz = rzn
            q = self.turn(q, GR, x)
        posed = self.fk(q, gt)[1]
        return q, posed, (t - self.bones(posed)).norm(dim=-1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bones_times.json"))
    ap.add_argument("--reps", type=int, default=100, help="timed calls of fit_bones and fit_pose (the torch-op form takes a twentieth)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bones_time.py measures on the GPU"
    dev = torch.device("cuda")
    iterations, cg_steps = 32, 8
    rows = []
    for J in (24, 256):
        for B in (1, 60):
            joints, parents, depth, q0, q1 = make_problem(J, B, 100 + J)
            ref = TorchBones(joints, parents, depth, dev)
            factors = np.random.default_rng(200 + J).uniform(0.5, 2.0, (J, 1)).astype(np.float32)
            other = joints.copy()
            for i in range(1, J):
                other[i] = other[parents[i]] + factors[i] * (joints[i] - joints[parents[i]])
            q0, gt = torch.tensor(q0, device=dev), torch.zeros(B, 3, device=dev)
            src = TorchChain(other, parents, depth, dev).fk(torch.tensor(q1, device=dev), gt)[1]
            directions = (src - src[:, ref.vp]).contiguous()
            t = directions / directions.norm(dim=-1, keepdim=True).clamp_min(1e-30)
            targets = ref.fk(torch.tensor(q1, device=dev), gt)[1].contiguous()  # (fit_pose: the same pose on the rig itself)
            rig = (ref.x, torch.tensor(parents, dtype=torch.int32, device=dev))
            pose = {"local_rotation": q0, "global_trans": gt}
            call = lambda: PE.fit_bones(rig, pose, directions, iterations=iterations, cg_steps=cg_steps, damping=DAMPING, max_step=MAX_STEP)  # noqa: E731
            fit = lambda: PE.fit_pose(rig, pose, targets, iterations=iterations, cg_steps=cg_steps)  # noqa: E731
            out = call()
            tq, tn, tres = ref.solve(q0, gt, t, iterations, cg_steps)
            row = {"J": J, "iterations": iterations, "cg_steps": cg_steps, "B": B, "levels": len(ref.levels),
                   "max_abs_diff_d_nodes": float((out["d_nodes"] - tn).abs().max()),
                   "largest_chord": float(out["residual"].max()), "largest_chord_torch_ops": float(tres.max()),
                   "fit_bones_ms": timed(call, args.reps), "fit_pose_ms": timed(fit, args.reps),
                   "torch_ops_ms": timed(lambda: ref.solve(q0, gt, t, iterations, cg_steps), max(2, args.reps // 20), warmup=1)}
            row["speedup"] = row["torch_ops_ms"] / row["fit_bones_ms"]
            row["fit_pose_over_fit_bones"] = row["fit_pose_ms"] / row["fit_bones_ms"]
            print(json.dumps(row), flush=True)
            rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "what": "ms per call, device events; fit_bones = one launch of csrc/bones.hip "
                   "(plus torch's allocations), torch_ops = the same iteration in torch ops on the device, fit_pose = one launch of "
                   "csrc/fit.hip on the same rig, poses and counts (position targets of the same second pose)", "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
