"""The bits of riggs_amd.pose_edit.solve_ik and fit_pose on a fixed grid: per case and output tensor the SHA-256 of its bytes.  Both
kernels are deterministic and built without contraction, so a change that keeps every expression's tree keeps every digest: run
this on the tree before and after, each in a process of its own, and compare (--merge).
The grid: trees and poses of tests/ik_ref.py at J = 1, 2, 24, 64, 65, 256 and B = 1, 3; the default solve at 0, 1 and 8 iterations,
and at 8 iterations each of: solve_translation; absolute damping and / or max_step (relative = 0, 1, 2; for solve_ik relative = 0
means extent NULL); locked joints; weights given, and with a zero; solve_ik: one handle, a handle index outside [0, J) on the
device; fit_pose: cg_steps = 1 and cg_steps = J + 3.  Needs the GPU; takes seconds; reads nothing outside the repository.
  python tools/pose_solve_bits.py --out A.json
  python tools/pose_solve_bits.py --merge parent=A.json new=B.json --out profiles/pose_solve_bits.json"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES, BATCHES, ITERATIONS = (1, 2, 24, 64, 65, 256), (1, 3), (0, 1, 8)


def problem(J, B):
    from tests import ik_ref as R
    joints, parents = R.tree(J, 700 + J)
    rng = np.random.default_rng(1700 + J)
    q0 = np.stack([R.pose(J, 0.1, rng) for _ in range(B)])
    gt0 = rng.normal(0, 0.05, (B, 3)).astype(np.float32)
    posed = np.stack([R.fk(joints.astype(np.float64), parents, R.pose(J, 0.25, rng).astype(np.float64), gt0[b].astype(np.float64))[2]
                      for b in range(B)]).astype(np.float32)
    return joints, parents, q0, gt0, posed, R.deepest(parents, min(8, J))


def grid():
    """(id, solver, J, B, iterations, keywords) of every case; 'locked' / 'weights' / 'handles' name what is built per problem."""
    for J in SIZES:
        for B in BATCHES:
            for solver in ("ik", "fit"):
                for n in ITERATIONS:
                    yield "%s-J%d-B%d-it%d" % (solver, J, B, n), solver, J, B, n, {}
                features = {"translation": dict(solve_translation=True), "relative0": dict(damping=0.07, max_step=0.6),
                            "relative1": dict(max_step=0.6), "relative2": dict(damping=0.07), "locked": dict(locked="every third"),
                            "weights": dict(weights="given"), "weight0": dict(weights="with a zero")}
                if solver == "ik":
                    features.update(one_handle=dict(handles="one"), handle_outside=dict(handles="one outside"))
                else:
                    features.update(cg1=dict(cg_steps=1), cg_over_J=dict(cg_steps=J + 3))
                for name, kw in features.items():
                    yield "%s-J%d-B%d-it8-%s" % (solver, J, B, name), solver, J, B, 8, kw


def run(out):
    import torch
    from riggs_amd import pose_edit as PE
    assert torch.cuda.is_available(), "pose_solve_bits.py runs the kernels: it needs the GPU"
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    problems, cases = {}, {}
    for cid, solver, J, B, n, kw in grid():
        if (J, B) not in problems:
            problems[(J, B)] = problem(J, B)
        joints, parents, q0, gt0, posed, deepest = problems[(J, B)]
        kw = dict(kw)
        handles = deepest[:1] if kw.get("handles") == "one" else deepest
        E = len(handles) if solver == "ik" else J
        if kw.get("locked"):
            kw["locked"] = T(np.arange(J) % 3 == 1)
        if kw.get("weights"):
            w = np.linspace(0.5, 2.0, B * E).astype(np.float32).reshape(B, E)
            if kw["weights"] == "with a zero":
                w[:, E // 2] = 0
            kw["weights"] = T(w)
        pose = {"local_rotation": T(q0), "global_trans": T(gt0)}
        rig = (T(joints), T(parents))
        if solver == "ik":
            h = np.array(handles, np.int32)
            if kw.pop("handles", None) == "one outside":
                h[0] = J + 5
            res = PE.solve_ik(rig, pose, T(h), T(posed[:, handles]), iterations=n, **kw)
        else:
            res = PE.fit_pose(rig, pose, T(posed), iterations=n, **kw)
        cases[cid] = {k: hashlib.sha256(v.contiguous().cpu().numpy().tobytes()).hexdigest() for k, v in sorted(res.items())}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "what": "SHA-256 of each output tensor's bytes per case of "
                   "tools/pose_solve_bits.py", "cases": cases}, f, indent=1, sort_keys=True)
    print(json.dumps({"cases": len(cases), "out": out}))


def merge(columns, out):
    names, runs = zip(*[(c.split("=", 1)[0], json.load(open(c.split("=", 1)[1]))) for c in columns])
    ids = sorted(set().union(*[r["cases"] for r in runs]))
    cases = {i: {k: [r["cases"].get(i, {}).get(k) for r in runs] for k in sorted(set().union(*[r["cases"].get(i, {}) for r in runs]))}
             for i in ids}
    differ = sorted(i for i in ids if any(len(set(d)) != 1 for d in cases[i].values()))
    with open(out, "w") as f:
        json.dump({"device": runs[0]["device"], "what": runs[0]["what"], "columns": list(names), "all_equal": not differ,
                   "differ": differ, "cases": cases}, f, indent=1, sort_keys=True)
    print(json.dumps({"cases": len(ids), "all_equal": not differ, "differ": differ[:8]}))
    return 1 if differ else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_solve_bits.json"))
    ap.add_argument("--merge", nargs="+", metavar="NAME=PATH", help="compare earlier runs instead of running: one column per run")
    args = ap.parse_args()
    return merge(args.merge, args.out) if args.merge else run(args.out)


if __name__ == "__main__":
    sys.exit(main())
