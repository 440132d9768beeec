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
from riggs_amd.dual_quaternion import quaternion_raw_multiply, quaternion_to_matrix  # noqa: E402


def make_problem(J, E, B, seed):
    """A random tree (parents[i] = randint(0, i), bone offsets N(0, 0.25^2)), its E deepest joints as handles, a starting pose
    identity + N(0, 0.1^2) and the handles' positions under a second pose identity + N(0, 0.25^2) as targets."""
    rng = np.random.default_rng(seed)
    parents = np.zeros(J, np.int64)
    joints = np.zeros((J, 3), np.float32)
    depth = np.zeros(J, np.int64)
    for i in range(1, J):
        parents[i] = rng.integers(0, i)
        joints[i] = joints[parents[i]] + rng.normal(0, 0.25, 3)
        depth[i] = depth[parents[i]] + 1
    handles = np.array(sorted(range(J), key=lambda i: (-depth[i], -i))[:E])
    ident = np.array([1, 0, 0, 0], np.float32)
    q0 = (ident + rng.normal(0, 0.1, (B, J, 4))).astype(np.float32)
    q1 = (ident + rng.normal(0, 0.25, (B, J, 4))).astype(np.float32)
    return joints, parents, depth, handles, q0, q1


class TorchIK:
    """The iteration of include/riggs_hip.h (riggs_ik_solve) in torch ops; the topology is prepared once on the host."""

    def __init__(self, joints, parents, depth, handles, dev):
        J = len(parents)
        self.J, self.E = J, len(handles)
        self.x = torch.tensor(joints, device=dev)
        self.vp = torch.tensor(parents, device=dev)
        self.c = self.x[self.vp]
        self.levels = [torch.tensor(np.flatnonzero(depth == l), device=dev) for l in range(1, int(depth.max()) + 1)]
        on = np.zeros((self.E, J), np.float32)
        for e, h in enumerate(handles):
            a = int(h)
            while True:
                on[e, a] = 1
                if a == 0:
                    break
                a = int(parents[a])
        self.on = torch.tensor(on, device=dev)
        self.handles = torch.tensor(handles, device=dev)
        ext = PE.rig_extent(self.x)
        self.damping2, self.max_step = (0.05 * ext) ** 2, 0.5 * ext
        self.eye = torch.eye(3 * self.E, device=dev)

    def fk(self, q, gt):
        R = quaternion_to_matrix(q)                                            # (B, J, 3, 3)
        t = self.c - (R @ self.c[None, :, :, None])[..., 0]
        GR, Gt = R.clone(), t.clone()
        for idx in self.levels:
            p = self.vp[idx]
            Gt[:, idx] = (GR[:, p] @ t[:, idx, :, None])[..., 0] + Gt[:, p]
            GR[:, idx] = GR[:, p] @ R[:, idx]
        return GR, (GR @ self.x[None, :, :, None])[..., 0] + Gt + gt[:, None]

    def solve(self, q, gt, targets, iterations):
        B, J, E = q.shape[0], self.J, self.E
        for _ in range(iterations):
            GR, posed = self.fk(q, gt)
            ph = posed[:, self.handles]                                        # (B, E, 3)
            d = targets - ph
            n = d.norm(dim=-1, keepdim=True)
            d = torch.where(n > self.max_step, d * (self.max_step / n.clamp_min(1e-30)), d)
            P = (ph[:, :, None] - posed[:, self.vp][:, None]) * self.on[None, :, :, None]  # (B, E, J, 3)
            z = torch.zeros_like(P[..., 0])
            Jm = torch.stack([z, P[..., 2], -P[..., 1], -P[..., 2], z, P[..., 0], P[..., 1], -P[..., 0], z], -1)  # -[P]x
            Jm = Jm.reshape(B, E, J, 3, 3).permute(0, 1, 3, 2, 4).reshape(B, 3 * E, 3 * J)
            A = Jm @ Jm.transpose(1, 2) + self.damping2 * self.eye
            y = torch.cholesky_solve(d.reshape(B, 3 * E, 1), torch.linalg.cholesky(A))
            om = (Jm.transpose(1, 2) @ y).reshape(B, J, 3)
            delta = (GR[:, self.vp].transpose(2, 3) @ om[..., None])[..., 0]
            delta = torch.cat([om[:, :1], delta[:, 1:]], 1)
            th = delta.norm(dim=-1, keepdim=True)
            k = torch.sin(0.5 * th) / th.clamp_min(1e-30)
            dq = torch.cat([torch.cos(0.5 * th), k * delta], -1)
            q = torch.where(th > 0, quaternion_raw_multiply(dq, q), q)
        return q, self.fk(q, gt)[1]


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


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
            joints, parents, depth, handles, q0, q1 = make_problem(J, E, B, 100 + J)
            ref = TorchIK(joints, parents, depth, handles, dev)
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
