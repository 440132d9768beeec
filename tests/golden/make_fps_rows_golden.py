"""Golden vectors of farthest-point sampling over rows of D floats from the REAL RigGS reference (CPU) — run in the build
container only:   python tests/golden/make_fps_rows_golden.py

fpsrows_*.npz hold ``rows`` (fp32), ``start`` and ``indices``: the indices of the reference's ``farthest_point_sample``
(utils/time_utils.py:461-482) with the torch RNG seeded and the start read back from ``indices[0]``.  Only data is written.

The reference's ``torch.sum`` over D columns has no defined order, so a cloud is a fixture only if no pick hangs on it
(tests/fps_rows_ref.py): in a float64 run of the loop the maximum of ``nearest`` exceeds the largest value strictly below it by a
relative gap of at least 4 (D + 2) 2^-24 at every step, and the reference's fp32 indices equal the float64 ones.  A seed that
fails either is replaced (the next one is tried), never tolerated.  The 48-wide rows are trajectories — a point and its
positions at 16 times of a smooth motion — on a grid of 1 / 256, which deflates to under half the bytes."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _ref_shim as S  # noqa: E402

S.install()
with S.quiet():
    import utils.time_utils as TU  # noqa: E402
from tests import fps_rows_ref as R  # noqa: E402


def trajectories(rng, N, times=16):
    """(N, 3 times) fp32 on a grid of 1 / 256: a point cloud swinging about two axes with a phase per point."""
    x = rng.standard_normal((N, 3))
    t = np.linspace(0.0, 1.0, times)[None, :, None]
    amp, phase = 0.3 * rng.standard_normal((N, 1, 3)), 2 * np.pi * rng.random((N, 1, 1))
    traj = x[:, None] + amp * np.sin(2 * np.pi * t + phase) + 0.2 * t * rng.standard_normal((1, 1, 3))
    return (np.round(traj.reshape(N, -1) * 256.0) / 256.0 + 0.0).astype(np.float32)


def record(name, make, npoint, seed, stored=None):
    """Try seeds from ``seed`` on until the cloud ``make(rng)`` passes both checks; write it (``stored``: the part of the rows
    the file keeps, which the reader expands)."""
    for s in range(seed, seed + 20):
        rows = make(np.random.default_rng(s))
        torch.manual_seed(s)
        idx = TU.farthest_point_sample(torch.from_numpy(rows).unsqueeze(0), npoint)[0].numpy().astype(np.int64)
        start = int(idx[0])
        idx64, gap = R.fps_rows_f64(rows, start, npoint)
        D = rows.shape[1]
        if gap < R.margin_bound(D) or not np.array_equal(idx, idx64):
            print(name, "seed", s, "rejected: gap %.3g (bound %.3g), reference == float64: %s" % (gap, R.margin_bound(D), np.array_equal(idx, idx64)))
            continue
        assert np.array_equal(R.fps_rows(rows, start, npoint), idx)  # (the sequential order is one of the orders the margin covers)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, rows=rows if stored is None else rows[:stored], start=start, indices=idx)
        print("wrote", name, rows.shape, "picks", npoint, "seed", s, "gap %.3g" % gap, "bound %.3g" % R.margin_bound(D), "bytes", os.path.getsize(path))
        assert os.path.getsize(path) < 400 * 1000
        return idx
    raise SystemExit(name + ": no usable seed")


if __name__ == "__main__":
    record("fpsrows_n2050_d48_p40", lambda g: trajectories(g, 2050), 40, 1)
    record("fpsrows_n1025_d5_p64", lambda g: g.standard_normal((1025, 5)).astype(np.float32), 64, 2)
    record("fpsrows_n4097_d1_p33", lambda g: g.standard_normal((4097, 1)).astype(np.float32), 33, 3)
    record("fpsrows_n300_d64_p40", lambda g: g.standard_normal((300, 64)).astype(np.float32), 40, 4)
    record("fpsrows_n1_d48_p1", lambda g: trajectories(g, 1), 1, 5)
    idx = record("fpsrows_n2050x2_d48_p20", lambda g: np.tile(trajectories(g, 2050), (2, 1)), 20, 6, stored=2050)
    assert int(idx[1:].max()) < 2050  # equal distances at n and n + 2050: the lower index
    idx = record("fpsrows_same300_d48_p5", lambda g: np.tile(trajectories(g, 1), (300, 1)), 5, 7, stored=1)
    assert idx[1:].tolist() == [0, 0, 0, 0]
