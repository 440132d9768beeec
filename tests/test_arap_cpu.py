"""ARAP handle editing without a GPU: the float64 restatement (tests/arap_ref.py) against the reference's own recorded drags
(tests/golden/arap_*.npz, made by tests/golden/make_arap_golden.py), the graph and the operator of riggs_amd.arap on host tensors,
and what ``ARAPDeformer`` refuses before any launch.

THE BAR of the restatement against the goldens is 4 times the largest distance measured between them on the machine that recorded
the goldens — positions 4 x 7.3e-7 = 2.9e-6 of the cloud's extent, rotations 4 x 3.6e-6 = 1.4e-5 rad (the angle between the two
rotations; q and -q are one rotation).  That distance is the reference's own float32 error (its lstsq and its batched SVD run in
float32; the restatement in float64); the 4 is for LAPACK builds that differ between machines.  With RIGGS_ARAP_PARITY_JSON set
to a path the measured distances go there under "cpu" (profiles/arap_parity.json is such a record)."""
import glob
import os

import numpy as np
import pytest
import torch

from riggs_amd import _lib as L
from riggs_amd import arap as AR
from tests import arap_ref as R

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "arap_*.npz")))
BAR_POS = 4 * 7.3e-7   # of the cloud's extent
BAR_ROT = 4 * 3.6e-6   # rad
_REPORT = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    R.merge_report("RIGGS_ARAP_PARITY_JSON", "cpu", dict(_REPORT, bar_pos=BAR_POS, bar_rot=BAR_ROT))


def load(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def test_the_header_declares_the_entry_point():
    assert "riggs_arap_edit" in L.exported_symbols()
    assert AR.MAX_NODES == 1024 and AR.MAX_K == 16


def test_there_are_goldens():
    assert len(GOLDEN) >= 3, GOLDEN


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_graph_is_the_references_where_it_drops_no_edge(path):
    g = load(path)
    assert (g["nn"] >= 0).all() and np.isfinite(g["weight"]).all()  # (the maker's condition)
    traj = g.get("trajectory")
    nn_idx, _, weight = R.graph(g["verts"], g["radius"], int(g["K"]), trajectory=traj)
    assert np.array_equal(nn_idx, g["nn"])
    assert np.abs(weight - g["weight"]).max() <= 1e-6 * g["weight"].max()
    t_idx, _, t_w = AR.arap_graph(torch.from_numpy(g["verts"]), float(g["radius"]), int(g["K"]),
                                  trajectory=None if traj is None else torch.from_numpy(traj))
    assert t_idx.dtype == torch.int32 and np.array_equal(t_idx.numpy(), g["nn"])
    assert np.abs(t_w.numpy() - g["weight"]).max() <= 1e-6 * g["weight"].max()


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_float64_restatement_against_the_reference(path):
    """Every recorded call: the first from the initial solve, each further one from the reference's own previous positions
    (``init_verts``), so that no deviation is carried from call to call.  Bars: the module's docstring."""
    g = load(path)
    name = os.path.basename(path)[:-4]
    ext = R.extent_of(g["verts"])
    handles = tuple(int(h) for h in g["handle_idx"])
    G, null_dims = R.operator(R.laplacian(g["nn"], g["weight"]), handles)
    assert null_dims == 0
    worst_p = worst_r = 0.0
    for c in range(len(g["pos"])):
        init = None if c == 0 else g["pos"][c - 1]
        pos, quat, _ = R.deform(g["verts"], g["nn"], g["weight"], G, handles, g["handle_pos"], init, 3, np.float64)
        worst_p = max(worst_p, float(np.abs(pos - g["pos"][c]).max() / ext))
        worst_r = max(worst_r, float(R.rotation_angle(quat, g["quat"][c]).max()))
        assert np.array_equal(pos[list(handles)], g["handle_pos"].astype(np.float64))
    _REPORT[name] = {"pos_over_extent": worst_p, "rot_rad": worst_r}
    print(name, "positions %.3g of the extent, rotations %.3g rad" % (worst_p, worst_r))
    assert worst_p <= BAR_POS, (name, worst_p)
    assert worst_r <= BAR_ROT, (name, worst_r)


def test_the_float32_restatement_stays_next_to_the_oracle():
    """The yardstick itself: float32 within 2e-5 of the extent and 2e-4 rad of float64 on the small GPU cases (float32's epsilon
    times the condition of A_u, below 1e2 there, times a few dozen roundings)."""
    for case in R.CASES:
        if case["N"] > 130:
            continue
        inp = R.case_inputs(case)
        nn_idx, _, weight = R.graph(inp["verts"], inp["radius"], case["K"])
        o64, o32 = R.reference(case, nn_idx, weight)
        assert np.abs(o32["pos"] - o64["pos"]).max() / inp["extent"] <= 2e-5, case["name"]
        assert R.rotation_angle(o32["quat"], o64["quat"]).max() <= 2e-4, case["name"]


def test_handles_land_exactly_on_their_targets():
    case = next(c for c in R.CASES if c["name"] == "n65_m3_b3_k16")
    inp = R.case_inputs(case)
    nn_idx, _, weight = R.graph(inp["verts"], inp["radius"], case["K"])
    o64, o32 = R.reference(case, nn_idx, weight)
    h = list(inp["handles"])
    assert np.array_equal(o64["pos"][:, h], inp["handle_pos"].astype(np.float64))
    assert np.array_equal(o32["pos"][:, h].view(np.uint32), inp["handle_pos"].view(np.uint32))
    # the module's operator: zero rows for the handles, zero padding columns, the restatement's pseudo-inverse elsewhere
    d = AR.ARAPDeformer(torch.from_numpy(inp["verts"]), K=case["K"], radius=float(inp["radius"]))
    G, null_dims = d.operator(h)
    assert null_dims == 0 and G.dtype == torch.float32 and G.shape == (65, 68)
    assert not G[h].any() and not G[:, 65:].any()
    ref, _ = R.operator(R.laplacian(d.nn_idx.numpy(), d.weight.numpy()), inp["handles"])
    assert np.abs(G[:, :65].numpy() - ref).max() <= 1e-6 * np.abs(ref).max()
    assert d.operator(list(reversed(h)))[0] is G  # cached by the SET


def test_a_cluster_without_handles_stays_at_rest():
    """Two far-apart clusters, handles in one only: A_u's block of the other cluster is singular (its rows sum to zero), the
    dropped singular values are counted, and the displacement form leaves that cluster on its rest positions."""
    rng = np.random.default_rng(5)
    a = rng.uniform(-0.5, 0.5, (24, 3))
    b = rng.uniform(-0.5, 0.5, (20, 3)) + np.array([50.0, 0.0, 0.0])
    verts = np.concatenate([a, b]).astype(np.float32)
    d = AR.ARAPDeformer(torch.from_numpy(verts), K=6, radius=2.0)
    assert (d.nn_idx.numpy()[:24] < 24).all() and (d.nn_idx.numpy()[24:] >= 24).all()
    handles = (3, 17)
    G, null_dims = d.operator(handles)
    assert null_dims >= 1
    assert np.abs(G.numpy()[24:, :24]).max() <= 1e-6 and np.abs(G.numpy()[:24, 24:44]).max() <= 1e-6
    Gr, nd = R.operator(R.laplacian(d.nn_idx.numpy(), d.weight.numpy()), handles)
    assert nd == null_dims
    target = verts[list(handles)] + np.array([[0.3, 0.1, -0.2], [0.25, 0.15, -0.1]], np.float32)
    pos, quat, _ = R.deform(verts, d.nn_idx.numpy(), d.weight.numpy(), Gr, handles, target, None, 3, np.float64)
    # "at rest" to the weights' own rounding: they are float32, a row sums to 1 within (K + 1) 2^-24 = 4e-7, so the block times the
    # cluster's coordinates (up to the extent in size) is zero to that, and the kept part of the pseudo-inverse is O(1): 1e-6 of
    # the extent, and for the rotations twice that over the shortest edge
    bar = 1e-6 * R.extent_of(verts)
    moved = float(np.abs(pos[24:] - verts[24:]).max())
    print("the cluster without handles moved by %.3g (bar %.3g), the other by %.3g" % (moved, bar, np.abs(pos[:24] - verts[:24]).max()))
    assert moved <= bar
    assert np.abs(pos[:24] - verts[:24]).max() > 0.05
    shortest = float(np.sqrt(d.nn_dist.numpy()[24:].min()))
    assert R.rotation_angle(quat[24:], np.broadcast_to([1.0, 0, 0, 0], (20, 4))).max() <= 2 * bar / shortest


def test_weights_with_a_dropped_edge_are_the_references_formula_over_the_kept_edges():
    rng = np.random.default_rng(7)
    verts = R.cloud("blob", 300, rng)
    radius = R.extent_of(verts) / 8
    nn_idx, nn_dist, weight = (t.numpy() for t in AR.arap_graph(torch.from_numpy(verts), radius, 16))
    kept = nn_idx >= 0
    assert 0 < (~kept).sum() < kept.size and kept[:, :3].all()
    assert np.isfinite(weight).all() and (weight[~kept] == 0).all() and np.isinf(nn_dist[~kept]).all()
    assert (nn_dist[:, 3:][kept[:, 3:]] < np.float32(radius) ** 2).all()
    d64 = nn_dist.astype(np.float64)
    w = np.where(kept, np.exp(-np.where(kept, d64, 0) / d64[kept].mean()), 0.0)
    w /= w.sum(1, keepdims=True)
    assert np.abs(weight - w).max() <= 1e-6
    assert np.abs(weight.sum(1) - 1).max() <= 1e-6
    r_idx, _, r_w = R.graph(verts, radius, 16)
    assert np.array_equal(r_idx, nn_idx) and np.abs(r_w - weight).max() <= 1e-6


def test_argument_checks():
    v = torch.zeros(30, 3)
    with pytest.raises(NotImplementedError):
        AR.ARAPDeformer(v, point_mask=torch.ones(30, dtype=torch.bool))
    with pytest.raises(ValueError):
        AR.ARAPDeformer(torch.zeros(1025, 3))
    with pytest.raises(ValueError):
        AR.ARAPDeformer(v, K=17)
    d = AR.ARAPDeformer(torch.rand(30, 3, generator=torch.Generator().manual_seed(0)), K=4, radius=10.0)
    for bad in ([], [30], [-1], [2, 2]):
        with pytest.raises(ValueError):
            d.deform(bad, np.zeros((len(bad), 3), np.float32))
