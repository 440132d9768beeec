"""Farthest-point sampling over rows of D floats, restated in numpy with the arithmetic csrc/fps.hip is held to bit for bit: the
squared distance is the sequential fp32 sum ((t_0^2 + t_1^2) + t_2^2) + ... over ascending columns, t_k = fl(p_k - c_k), every
product and sum rounded; ``nearest`` starts at 1e10 and updates on ``d < nearest``; ties on the maximum go to the lowest index.
Also the float64 run that says how far a cloud is from a tie, and the reader of tests/golden/fpsrows_*.npz
(tests/golden/make_fps_rows_golden.py wrote them from the reference)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("fpsrows_n2050_d48_p40", "fpsrows_n1025_d5_p64", "fpsrows_n4097_d1_p33", "fpsrows_n300_d64_p40", "fpsrows_n1_d48_p1",
            "fpsrows_n2050x2_d48_p20", "fpsrows_same300_d48_p5")
_CACHE = {}


def fixture(name):
    """(rows (N, D) fp32, start, reference indices (npoint,) int64).  Read once; do not modify."""
    if name not in _CACHE:
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        rows = z["rows"]
        if name == "fpsrows_n2050x2_d48_p20":  # the cloud twice: every distance occurs at n and at n + 2050
            rows = np.tile(rows, (2, 1))
        if name == "fpsrows_same300_d48_p5":
            rows = np.tile(rows, (300, 1))
        _CACHE[name] = (np.ascontiguousarray(rows, dtype=np.float32), int(z["start"]), z["indices"].astype(np.int64))
    return _CACHE[name]


def fps_rows(rows, start, npoint):
    """(npoint,) int64 indices of the sweep over ``rows`` (N, D) fp32 from ``start``, in the kernel's arithmetic."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    N, D = rows.shape
    cols = np.ascontiguousarray(rows.T)
    nearest = np.full(N, 1e10, dtype=np.float32)
    out = np.empty(npoint, dtype=np.int64)
    cur = min(max(int(start), 0), N - 1)
    for i in range(npoint):
        out[i] = cur
        if i == npoint - 1:
            break
        acc = np.zeros(N, dtype=np.float32)
        for k in range(D):
            t = cols[k] - cols[k, cur]
            acc = acc + t * t  # (fp32 arrays: the product is rounded, then the sum)
        assert acc.dtype == np.float32
        nearest = np.where(acc < nearest, acc, nearest)
        cur = int(np.argmax(nearest))  # (the first maximum: the lowest index)
    return out


def margin_bound(D):
    """Two fp32 evaluations of a D-term squared distance are each within (D + 2) 2^-24 of the exact value (relative): at a
    relative gap of four times that between the maximum and the next value below it they cannot order the two differently."""
    return 4.0 * (D + 2) * 2.0 ** -24


def fps_rows_f64(rows, start, npoint):
    """The same sweep in float64 (any summation order is exact enough there): ``(indices, gap)`` with ``gap`` the smallest
    relative distance, over the steps that decide a pick, between the maximum of ``nearest`` and the largest value strictly
    below it (inf if no step has two distinct values)."""
    r = np.asarray(rows, dtype=np.float64)
    N = r.shape[0]
    nearest = np.full(N, 1e10)
    out = np.empty(npoint, dtype=np.int64)
    cur, gap = int(start), np.inf
    for i in range(npoint):
        out[i] = cur
        if i == npoint - 1:
            break
        nearest = np.minimum(nearest, ((r - r[cur]) ** 2).sum(-1))
        m = nearest.max()
        below = nearest[nearest < m]
        if below.size and m > 0:
            gap = min(gap, (m - below.max()) / m)
        cur = int(np.argmax(nearest))
    return out, gap
