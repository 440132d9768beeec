"""NumPy restatement of the multiresolution hash-grid encoding (Mueller et al., Instant Neural Graphics Primitives, 2022) that
csrc/hashgrid.hip is held to: written from the published algorithm as include/riggs_hip.h spells it out, not from tinycudann.

Indices are uint32 with wrap-around; the position is ``(x.double * scale.double + 0.5).float`` — the product of two float32 is
exact in double and so is the sum's single rounding to float32, which makes it ``fmaf(scale, x, 0.5f)`` exactly; weights and sums
are float64.  Besides the output the oracle returns the table gradient of a cotangent and, per table entry, sum |w mask g|: the
scale of the rounding error a float32 sum of those terms can have.

``table_values`` is the closed-form integer table the goldens use instead of storing 2^19-entry tables."""
import math

import numpy as np

PRIMES = np.array([1, 2654435761, 805459861, 3674653429], dtype=np.uint32)
REFERENCE_CONFIG = dict(n_levels=12, n_features_per_level=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=2.0)


def level_table(n_input_dims, n_levels=12, n_features_per_level=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=2.0, **_):
    """Per level: scale (float32), resolution, size, offset, hashed; and the number of entries of the whole table."""
    levels, at = [], 0
    for l in range(n_levels):
        scale = np.float32(float(base_resolution) * float(per_level_scale) ** l - 1.0)
        res = int(math.ceil(float(scale))) + 1
        cells = res ** n_input_dims                                   # a Python integer: exact
        size = min((cells + 7) // 8 * 8, 2 ** log2_hashmap_size)
        levels.append(dict(scale=scale, resolution=res, size=size, offset=at, hashed=cells > size))
        at += size
    return levels, at


def corners(x, level, n_input_dims):
    """x (R, D) float32 -> (idx (R, 2^D) int64 within the level, w (R, 2^D) float64)."""
    D = n_input_dims
    x = np.ascontiguousarray(x, dtype=np.float32)
    pos = (x.astype(np.float64) * np.float64(level["scale"]) + 0.5).astype(np.float32)
    fl = np.floor(pos)
    cell = fl.astype(np.int64).astype(np.int32).astype(np.uint32)     # (uint32)(int32)floorf(pos)
    frac = (pos - fl).astype(np.float64)                              # float32 subtraction (exact), then widened
    R = x.shape[0]
    idx = np.empty((R, 1 << D), dtype=np.int64)
    w = np.empty((R, 1 << D), dtype=np.float64)
    res = np.uint32(level["resolution"])
    with np.errstate(over="ignore"):
        for k in range(1 << D):
            i = np.zeros(R, dtype=np.uint32)
            wk = np.ones(R, dtype=np.float64)
            stride = np.uint32(1)
            for d in range(D):
                bit = (k >> d) & 1
                c = cell[:, d] + np.uint32(bit)
                wk = wk * (frac[:, d] if bit else 1.0 - frac[:, d])
                if level["hashed"]:
                    i = i ^ (c * PRIMES[d])
                else:
                    i = i + c * stride
                    stride = np.uint32((int(stride) * int(res)) & 0xFFFFFFFF)
            idx[:, k] = (i % np.uint32(level["size"])).astype(np.int64)
            w[:, k] = wk
    return idx, w


def encode(x, table, n_input_dims, config, mask=None, g_out=None):
    """table (entries, F) -> out (R, L F) float64; with ``g_out`` (R, L F) also (g_table (entries, F) float64,
    g_abs (entries, F) float64 = sum |w mask g| per entry)."""
    levels, total = level_table(n_input_dims, **config)
    F = config.get("n_features_per_level", 2)
    L = len(levels)
    table = np.asarray(table, dtype=np.float64).reshape(total, F)
    m = np.ones(L * F) if mask is None else np.asarray(mask, dtype=np.float64).reshape(L * F)
    R = np.asarray(x).shape[0]
    out = np.zeros((R, L * F))
    if g_out is not None:
        g_out = np.asarray(g_out, dtype=np.float64).reshape(R, L * F)
        g_table, g_abs = np.zeros((total, F)), np.zeros((total, F))
    for l, lv in enumerate(levels):
        idx, w = corners(x, lv, n_input_dims)
        sl = slice(l * F, (l + 1) * F)
        out[:, sl] = (w[:, :, None] * table[lv["offset"] + idx]).sum(1) * m[sl]
        if g_out is not None:
            contrib = w[:, :, None] * (m[sl] * g_out[:, sl])[:, None, :]          # (R, 2^D, F)
            flat = (lv["offset"] + idx).reshape(-1)
            np.add.at(g_table, flat, contrib.reshape(-1, F))
            np.add.at(g_abs, flat, np.abs(contrib).reshape(-1, F))
    return (out, g_table, g_abs) if g_out is not None else out


def table_values(n, a, b, m):
    """The closed-form table of the goldens: value i of the flat table = (((a i + b) mod 2^32) mod m) / m * 2 - 1, as float32
    (n = entries x F values in [-1, 1); the goldens store a, b, m only)."""
    i = np.arange(n, dtype=np.uint64)
    v = ((np.uint64(a) * i + np.uint64(b)) & np.uint64(0xFFFFFFFF)) % np.uint64(m)
    return (v.astype(np.float64) / float(m) * 2.0 - 1.0).astype(np.float32)


def cosine_mask(step, n_output_dims=24, start_level=6, n_levels=12, update_steps=1000, n_features_per_level=2):
    """The band mask of ProgressiveBandHashGridCosine after update_step(step), in float64 from the rule's text: ones below the
    start level, then (1 - cos(pi clamp(ratio band - i, 0, 1))) / 2 over the band."""
    start = start_level * n_features_per_level
    band = n_output_dims - start
    ratio = step / ((n_levels - start_level) * update_steps)
    m = np.ones(n_output_dims)
    m[start:] = (1.0 - np.cos(np.pi * np.clip(ratio * band - np.arange(band), 0.0, 1.0))) / 2.0
    return m
