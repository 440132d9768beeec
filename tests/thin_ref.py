"""Guo and Hall's two-subiteration parallel thinning — the algorithm of ``skimage.morphology.thin`` — restated in NumPy +
``scipy.ndimage.correlate`` from its published definition; csrc/thin.hip is held to it bit for bit.  scikit-image itself is not
available to this suite: the restatement reproduces the one published example (the ``thin`` docstring's 7 x 7 case, see
tests/test_thin_cpu.py); agreement with an installed skimage beyond that example is not verified.

Neighbours of (r, c): x0 E (r, c+1), x1 NE, x2 N, x3 NW, x4 W, x5 SW, x6 S, x7 SE (r+1, c+1); the neighbourhood code is
sum x_i 2^i, pixels outside the image are 0.  A pixel is deleted by a sub-iteration when
  G1  exactly one i in {0, 2, 4, 6} has x_i = 0 and (x_{i+1} or x_{(i+2) mod 8}),
  G2  min(n1, n2) in {2, 3} with n1 = sum_{k in 1,3,5,7} (x_k or x_{k-1}), n2 = sum_k (x_k or x_{(k+1) mod 8}),
  G3  not ((x1 or x2 or not x7) and x0)        (first sub-iteration)
  G3' not ((x5 or x6 or not x3) and x4)        (second sub-iteration)
all hold on the state before the sub-iteration; all such pixels are cleared at once.  The two 256-entry tables below are
generated from this text."""
import numpy as np
from scipy import ndimage

KERNEL = np.array([[8, 4, 2], [16, 0, 1], [32, 64, 128]], dtype=np.int32)  # correlate(s, KERNEL, mode="constant") = the code


def deletes(code, sub):
    """Does sub-iteration ``sub`` (0: G3, 1: G3') delete a set pixel whose neighbourhood code is ``code``?"""
    x = [(code >> i) & 1 for i in range(8)]
    g1 = sum(1 for i in (0, 2, 4, 6) if not x[i] and (x[i + 1] or x[(i + 2) % 8])) == 1
    n1 = sum(1 for k in (1, 3, 5, 7) if x[k] or x[k - 1])
    n2 = sum(1 for k in (1, 3, 5, 7) if x[k] or x[(k + 1) % 8])
    g2 = min(n1, n2) in (2, 3)
    if sub == 0:
        g3 = not ((x[1] or x[2] or not x[7]) and x[0])
    else:
        g3 = not ((x[5] or x[6] or not x[3]) and x[4])
    return bool(g1 and g2 and g3)


TABLES = tuple(np.array([deletes(code, sub) for code in range(256)], dtype=bool) for sub in (0, 1))


def codes(s):
    """The neighbourhood code of every pixel of the binary image ``s`` (H, W)."""
    return ndimage.correlate(s.astype(np.int32), KERNEL, mode="constant", cval=0)


def thin_details(image, max_num_iter=None, first_subiter=0, max_subiters=None, histograms=False):
    """``(skeleton (H, W) bool, iterations, sub_iterations, histograms)``.  Sub-iteration number n (from 0) uses table
    ``(first_subiter + n) % 2``; after every second one the run stops if the pair deleted nothing.  ``iterations`` counts the
    pairs that ran, the one that only finds the fixed point included (the 7 x 7 example: 2); ``sub_iterations`` all that ran.
    ``max_subiters`` (or ``2 * max_num_iter``) bounds the sub-iterations exactly.  ``histograms``: per sub-iteration run, the
    (256,) counts of the neighbourhood codes at the pixels set in its input."""
    s = np.asarray(image) > 0
    if s.ndim != 2:
        raise ValueError("thin takes one (H, W) image")
    s = s.copy()
    limit = max_subiters if max_subiters is not None else (2 * max_num_iter if max_num_iter else None)
    hists, n, before = [], 0, int(s.sum())
    while limit is None or n < limit:
        c = codes(s)
        if histograms:
            hists.append(np.bincount(c[s], minlength=256))
        s &= ~TABLES[(first_subiter + n) % 2][c]
        n += 1
        if n % 2 == 0:
            after = int(s.sum())
            if after == before:
                break
            before = after
    return s, (n + 1) // 2, n, hists


def thin(image, max_num_iter=None, first_subiter=0, max_subiters=None):
    return thin_details(image, max_num_iter, first_subiter, max_subiters)[0]


# ---- the inputs the CPU and the GPU tests share (seeded; built once, do not modify) ------------------------------------------
_CACHE = {}


def ellipses(H, W, n, seed, rmin=0.05, rmax=0.22):
    """A silhouette-like union of ``n`` seeded, rotated ellipses, (H, W) bool."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((H, W), dtype=bool)
    for _ in range(n):
        cy, cx = rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W
        a, b = rng.uniform(rmin, rmax) * min(H, W), rng.uniform(rmin, rmax) * min(H, W)
        th = rng.uniform(0, np.pi)
        u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th)
        v = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
        out |= (u / a) ** 2 + (v / b) ** 2 <= 1.0
    return out


def discs(H, W, n, seed, rmax=6):
    """``n`` seeded discs of radius 1 .. rmax, (H, W) bool: thin in under ten iterations whatever the image size."""
    rng = np.random.default_rng(seed)
    out = np.zeros((H, W), dtype=bool)
    for _ in range(n):
        r = int(rng.integers(1, rmax + 1))
        cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
        y0, y1, x0, x1 = max(cy - r, 0), min(cy + r + 1, H), max(cx - r, 0), min(cx + r + 1, W)
        yy, xx = np.mgrid[y0:y1, x0:x1]
        out[y0:y1, x0:x1] |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return out


def blob():
    """The 97 x 131 union of six ellipses of the blob tests, with its thinned form: ``(mask, skeleton, iterations)``."""
    if "blob" not in _CACHE:
        m = ellipses(97, 131, 6, seed=28)
        s, it, _, _ = thin_details(m)
        m.setflags(write=False), s.setflags(write=False)
        _CACHE["blob"] = (m, s, it)
    return _CACHE["blob"]


def all_patches():
    """(80, 80) bool: the 256 possible 3 x 3 patches with the centre set on a 5-pixel pitch (two zero pixels between patches:
    they cannot interact within one sub-iteration).  Patch ``code`` has its centre at (5 (code // 16) + 1, 5 (code % 16) + 1)."""
    if "patches" not in _CACHE:
        off = ((0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1))  # x0 .. x7 as (dr, dc)
        img = np.zeros((80, 80), dtype=bool)
        for code in range(256):
            r, c = 5 * (code // 16) + 1, 5 * (code % 16) + 1
            img[r, c] = True
            for i, (dr, dc) in enumerate(off):
                img[r + dr, c + dc] = bool((code >> i) & 1)
        img.setflags(write=False)
        _CACHE["patches"] = img
    return _CACHE["patches"]
