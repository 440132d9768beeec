"""Times skeleton thinning on the HIP path (riggs_amd.thinning: csrc/thin.hip) at the size the datasets have, 800 x 800:
``thin`` + ``thinned_elements`` of 1 mask and of 100 masks in one batch (device time: events around the two calls, the median
of ``--repeats`` runs; the host's issue time next to it), the NumPy / SciPy restatement the tests use as their oracle
(tests/thin_ref.py) on the same masks on the host (one mask timed, and at most ``--oracle-masks`` of the hundred), and the two
device paths against each other on the same batch (the LDS path, which the size takes, and the global-memory path forced).
The masks are silhouette-like unions of ellipses, seeded and generated here.  Writes profiles/thin_times.json (or the path
after --out)."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from riggs_amd import thinning as T  # noqa: E402
from tests import thin_ref as R  # noqa: E402

H = W = 800


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    issue = time.perf_counter() - t0
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), 1e3 * issue, out


def timed(fn, repeats):
    once(fn)  # warm-up: code objects, the allocator
    runs = [once(fn) for _ in range(repeats)]
    ms = [r[0] for r in runs]
    return {"device_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "host_issue_ms": statistics.median(r[1] for r in runs)}, runs[-1][2]


def main():
    repeats, n_oracle = arg("--repeats", 7), arg("--oracle-masks", 3)
    masks = np.stack([R.ellipses(H, W, 8, seed=100 + k, rmin=0.04, rmax=0.2) for k in range(100)])
    dev = torch.from_numpy(masks).cuda()
    out = {"what": "thin + thinned_elements of 800 x 800 union-of-ellipses masks; device ms = median of %d runs" % repeats,
           "device": torch.cuda.get_device_name(0), "path_800x800": int(T.L.lib().riggs_thin_path(H, W)),
           "set_fraction_mean": float(masks.mean())}
    cap = int(masks.reshape(100, -1).sum(-1).max())  # (an upper bound given up front: no host read between the two calls)
    for name, x in (("masks_1", dev[:1]), ("masks_100", dev)):
        row, (skel, points, counts) = timed(lambda: (lambda s: (s,) + T.thinned_elements(s, 1, capacity=cap))(T.thin(x)), repeats)
        row["ms_per_mask"] = row["device_ms"] / x.shape[0]
        row["skeleton_pixels_mean"] = float(counts.float().mean())
        out[name] = row
        print(name, json.dumps(row))
    # the oracle on the host, and that the device agrees with it on the masks it was run on
    t_oracle, iters = [], []
    for k in range(max(1, n_oracle)):
        t0 = time.perf_counter()
        want, iterations, _, _ = R.thin_details(masks[k])
        t_oracle.append(time.perf_counter() - t0)
        iters.append(iterations)
        assert torch.equal(skel[k].cpu(), torch.from_numpy(want)), "the device and the oracle differ on mask %d" % k
    out["oracle_host"] = {"masks": len(t_oracle), "s_per_mask": statistics.median(t_oracle), "s_first_mask": t_oracle[0],
                          "iterations": iters, "s_per_100_masks_extrapolated": 100 * statistics.median(t_oracle)}
    print("oracle", json.dumps(out["oracle_host"]))
    # the two device paths on the same batch: thin alone
    for name, path in (("lds", T.PATH_LDS), ("global", T.PATH_GLOBAL)):
        row, got = timed(lambda: T.thin(dev, _path=path), repeats)
        assert torch.equal(got, skel)
        out["paths_100_masks_thin_only_" + name] = row
        print(name, json.dumps(row))
    out["global_over_lds"] = out["paths_100_masks_thin_only_global"]["device_ms"] / out["paths_100_masks_thin_only_lds"]["device_ms"]
    path = arg("--out", os.path.join(ROOT, "profiles", "thin_times.json"))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
