"""Time riggs_amd.pose_edit.solve_ik (one launch of csrc/ik.hip for all iterations) against the SAME iteration written in torch ops
on the device: the level-by-level chain, the Jacobian, J J^T, a Cholesky solve and the quaternion update per iteration.
Sizes: J = 24 / E = 2 / 16 iterations and J = 256 / E = 8 / 32 iterations, batches B = 1 and B = 60.  The two forms' results are
compared first.  Device events around repeated calls, after a warm-up; milliseconds per call.  Needs the GPU.
Writes profiles/ik_times.json (or the path after --out)."""
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


class TorchIK(TorchChain):
    """The iteration of include/riggs_hip.h (riggs_ik_solve) in torch ops on the E deepest joints of the tree as handles."""

    def __init__(self, joints, parents, depth, E, dev):
        super().__init__(joints, parents, depth, dev)
        handles = np.array(sorted(range(self.J), key=lambda i: (-depth[i], -i))[:E])
        self.E = E
        on = np.zeros((E, self.J), np.float32)
        for e, h in enumerate(handles):
            a = int(h)
            while True:
                on[e, a] = 1
                if a == 0:
                    break
                a = int(parents[a])
        self.on = torch.tensor(on, device=dev)
        self.handles = torch.tensor(handles, device=dev)
        self.eye = torch.eye(3 * E, device=dev)

    def solve(self, q, gt, targets, iterations):
        B, J, E = q.shape[0], self.J, self.E
        for _ in range(iterations):
            GR, posed = self.fk(q, gt)
            ph = posed[:, self.handles]                                        # (B, E, 3)
            d = self.clamped(targets - ph)
            P = (ph[:, :, None] - posed[:, self.vp][:, None]) * self.on[None, :, :, None]  # (B, E, J, 3)
            z = torch.zeros_like(P[..., 0])
            Jm = torch.stack([z, P[..., 2], -P[..., 1], -P[..., 2], z, P[..., 0], P[..., 1], -P[..., 0], z], -1)  # -[P]x
            Jm = Jm.reshape(B, E, J, 3, 3).permute(0, 1, 3, 2, 4).reshape(B, 3 * E, 3 * J)
            A = Jm @ Jm.transpose(1, 2) + self.damping2 * self.eye
            y = torch.cholesky_solve(d.reshape(B, 3 * E, 1), torch.linalg.cholesky(A))
            q = self.turn(q, GR, (Jm.transpose(1, 2) @ y).reshape(B, J, 3))
        return q, self.fk(q, gt)[1]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ik_times.json"))
    ap.add_argument("--reps", type=int, default=200, help="timed calls of solve_ik (the torch-op form takes a tenth)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ik_time.py measures on the GPU"
    dev = torch.device("cuda")
    rows = []
    for J, E, iterations in ((24, 2, 16), (256, 8, 32)):
        for B in (1, 60):
            joints, parents, depth, q0, q1 = make_problem(J, B, 100 + J)
            ref = TorchIK(joints, parents, depth, E, dev)
            q0, gt = torch.tensor(q0, device=dev), torch.zeros(B, 3, device=dev)
            targets = ref.fk(torch.tensor(q1, device=dev), gt)[1][:, ref.handles].contiguous()
            rig = (ref.x, torch.tensor(parents, dtype=torch.int32, device=dev))
            pose = {"local_rotation": q0, "global_trans": gt}
            h32 = ref.handles.to(torch.int32)
            out = PE.solve_ik(rig, pose, h32, targets, iterations=iterations)
            tq, tn = ref.solve(q0, gt, targets, iterations)
            row = {"J": J, "E": E, "iterations": iterations, "B": B, "levels": len(ref.levels),
                   "max_abs_diff_d_nodes": float((out["d_nodes"] - tn).abs().max()),
                   "residual_over_extent": float(out["residual"].max() / PE.rig_extent(ref.x)),
                   "solve_ik_ms": timed(lambda: PE.solve_ik(rig, pose, h32, targets, iterations=iterations), args.reps),
                   "torch_ops_ms": timed(lambda: ref.solve(q0, gt, targets, iterations), max(3, args.reps // 10))}
            row["speedup"] = row["torch_ops_ms"] / row["solve_ik_ms"]
            print(json.dumps(row), flush=True)
            rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "what": "ms per call, device events; solve_ik = one launch of csrc/ik.hip "
                   "(plus torch's allocations and the extent), torch_ops = the same iteration in torch ops on the device", "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
