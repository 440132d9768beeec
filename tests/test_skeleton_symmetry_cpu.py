"""CPU: the symmetry pass of the skeleton extraction (riggs_amd/skeleton_init.py: apply_symmetry through simplify_tree,
tree_from_samples and obtain_skeleton_tree) against what the reference returned for the same inputs and labels
(tests/golden/skelsym_*.npz, written by tests/golden/make_skeleton_symmetry_golden.py) — integer arrays equal, joint positions
bit for bit."""
import copy
import os

import numpy as np
import pytest
import torch

from riggs_amd import skeleton_init as SI
from tests import skeleton_init_ref as R

FIXTURES = ("skelsym_per40_twigs", "skelsym_per60", "skelsym_per12", "skelsym_uneven")
LABELS = ("zero", "limbs", "unique")
_CACHE = {}


def fixture(name):
    """The fixture as a dict of numpy arrays with the inputs put back to fp32.  Read once; do not modify."""
    if name not in _CACHE:
        z = dict(np.load(os.path.join(R.GOLDEN, name + ".npz")))
        grid = np.float32(z["grid"])
        z["nodes"] = z.pop("nodes_q").astype(np.float32) / grid
        z["all_deformed"] = z.pop("all_deformed_q").astype(np.float32) / grid
        _CACHE[name] = z
    return _CACHE[name]


def extract(z, labels):
    nodes, alld = torch.from_numpy(z["nodes"]), torch.from_numpy(z["all_deformed"])
    start = int(z["start"]) if nodes.shape[0] > 200 else None
    if labels is None:
        return SI.obtain_skeleton_tree(nodes, alld, None, start=start)
    return SI.obtain_skeleton_tree(nodes, alld, torch.from_numpy(labels), start=start, symmetry=True)


@pytest.mark.parametrize("kind", LABELS)
@pytest.mark.parametrize("name", FIXTURES)
def test_simplify_tree_with_labels_equals_the_reference(name, kind):
    z = fixture(name)
    points, labels = z["all_deformed"][:, z["indices1"]], z["labels_" + kind][z["indices1"]]
    if bool(z["index_error_" + kind]):
        with pytest.raises(IndexError, match="symmetry"):
            SI.simplify_tree(points, z["pruned"], labels)
        return
    assert np.array_equal(SI.simplify_tree(points, z["pruned"], labels), z["simplified_" + kind])
    assert np.array_equal(SI.simplify_tree(points, z["pruned"]), z["none_simplified"])
    assert np.array_equal(SI.simplify_tree(points, z["pruned"], None), z["none_simplified"])


@pytest.mark.parametrize("kind", LABELS)
@pytest.mark.parametrize("name", FIXTURES)
def test_whole_extraction_with_labels_equals_the_reference(name, kind):
    z = fixture(name)
    if bool(z["index_error_" + kind]):
        with pytest.raises(IndexError, match="symmetry"):
            extract(z, z["labels_" + kind])
        return
    joints, parents, indices = extract(z, z["labels_" + kind])
    assert joints.dtype == torch.float32 and parents.dtype == torch.int64 and indices.dtype == torch.int32
    assert np.array_equal(parents.numpy(), z["parents_" + kind]) and int(parents[0]) == -1
    assert np.array_equal(indices.numpy(), z["indices_" + kind])
    assert np.array_equal(joints.numpy().view(np.uint32), z["joints_" + kind].view(np.uint32))


@pytest.mark.parametrize("name", FIXTURES)
def test_tree_from_samples_takes_the_labels_by_node_index(name):
    """The labels are per NODE (M,): tree_from_samples reads them through the re-rooted tree's node indices."""
    z = fixture(name)
    sample = z["sample"]
    alld = torch.from_numpy(z["all_deformed"])
    md = SI.mean_pairwise_distances(alld[:, torch.from_numpy(sample)]).numpy()
    for kind in LABELS:
        if bool(z["index_error_" + kind]):
            continue
        out = SI.tree_from_samples(z["nodes"][sample], sample, md, z["all_deformed"], z["labels_" + kind])
        assert np.array_equal(out["indices1"], z["indices1"]) and np.array_equal(out["pruned"], z["pruned"])
        assert np.array_equal(out["simplified"], z["simplified_" + kind])
        assert np.array_equal(out["parents"], z["parents_" + kind]) and np.array_equal(out["indices"], z["indices_" + kind])
    out = SI.tree_from_samples(z["nodes"][sample], sample, md, z["all_deformed"])
    assert np.array_equal(out["simplified"], z["none_simplified"]) and np.array_equal(out["parents"], z["none_parents"])


def test_the_fixtures_cover_what_the_labels_change():
    """Zero labels are not None: at least two recorded trees differ from the tree without labels, one in its joint count, and
    the figure with uneven limbs is among them; labels that match nowhere leave every tree as it is."""
    changed = [(n, k) for n in FIXTURES for k in LABELS if not bool(fixture(n)["index_error_" + k])
               and not (np.array_equal(fixture(n)["parents_" + k], fixture(n)["none_parents"])
                        and np.array_equal(fixture(n)["indices_" + k], fixture(n)["none_indices"]))]
    assert len(changed) >= 2 and ("skelsym_uneven", "zero") in changed
    z = fixture("skelsym_per40_twigs")
    assert len(z["parents_zero"]) == 12 and len(z["none_parents"]) == 14
    assert int(fixture("skelsym_per60")["indices_zero"][4]) != int(fixture("skelsym_per60")["none_indices"][4])
    for n in FIXTURES:
        assert (n, "unique") not in changed
    for k in LABELS:
        assert ("skelsym_per12", k) not in changed


@pytest.mark.parametrize("name", R.SKELETON_FIXTURES)
def test_no_labels_still_match_the_fixtures_without_labels(name):
    z = R.skeleton_fixture(name)
    nodes, alld = torch.from_numpy(z["nodes"]), torch.from_numpy(z["all_deformed"])
    start = int(z["start"]) if nodes.shape[0] > 200 else None
    joints, parents, indices = SI.obtain_skeleton_tree(nodes, alld, seg_labels=None, start=start)
    assert np.array_equal(parents.numpy(), z["parents"]) and np.array_equal(indices.numpy(), z["indices"])
    assert np.array_equal(joints.numpy().view(np.uint32), z["joints"].view(np.uint32))
    out = SI.tree_from_samples(z["nodes"][z["sample"]], z["sample"], z["mean_distances"], z["all_deformed"], None)
    assert np.array_equal(out["simplified"], z["simplified"])


def test_apply_symmetry_leaves_the_pieces_alone_when_no_pair_qualifies():
    pts = fixture("skelsym_per12")["all_deformed"].astype(np.float64)
    paths = [[5, 4, 3, 2, 1, 0], [11, 10, 9, 8, 7, 0], [20, 19, 0]]
    pieces = [[(0, 2), (2, 5)], [(0, 5)], [(0, 2)]]
    # labels that differ between the chains: no semantic score above the threshold
    label = np.arange(pts.shape[1])
    before = copy.deepcopy(pieces)
    assert SI.apply_symmetry(paths, pieces, pts, label) == before
    # equal labels, but the only candidates left are too different in length (6 against 3 entries) or both one piece
    assert SI.apply_symmetry([paths[0], paths[2]], [pieces[0], pieces[2]], pts, np.zeros_like(label)) == [before[0], before[2]]
    assert SI.apply_symmetry([paths[1], [17, 16, 15, 14, 13, 0]], [[(0, 5)], [(0, 5)]], pts, np.zeros_like(label)) == [[(0, 5)], [(0, 5)]]
    # ... and with equal labels and like lengths the chain of two pieces gives its cut to the other one
    out = SI.apply_symmetry(paths[:2], copy.deepcopy(pieces[:2]), pts, np.zeros_like(label))
    assert out[0] == before[0] and len(out[1]) == 2 and out[1][0][0] == 0 and out[1][0][1] == out[1][1][0] and out[1][1][1] == 5


def test_path_distance_is_the_arc_length_of_the_mean_edges():
    pts = np.zeros((2, 4, 3))
    pts[:, 1, 0], pts[:, 2, 0], pts[0, 3, 0], pts[1, 3, 0] = 1.0, 3.0, 4.0, 6.0
    assert np.allclose(SI.compute_single_source_path_distance(pts, [0, 1, 2, 3]), [0.0, 1.0, 3.0, 5.0])
    assert np.allclose(SI.compute_single_source_path_distance(pts, [1, 0, -1]), [0.0, 1.0, 6.0])  # (-1: the last vertex)


def test_labels_are_validated():
    z = fixture("skelsym_per12")
    nodes, alld = torch.from_numpy(z["nodes"]), torch.from_numpy(z["all_deformed"])
    with pytest.raises(ValueError, match="seg_labels"):
        SI.obtain_skeleton_tree(nodes, alld, torch.zeros(nodes.shape[0] - 1, dtype=torch.int32), symmetry=True)
    with pytest.raises(ValueError, match="seg_labels"):
        SI.obtain_skeleton_tree(nodes, alld, torch.zeros(nodes.shape[0]), symmetry=True)
    a = SI.obtain_skeleton_tree(nodes, alld, torch.zeros(nodes.shape[0], dtype=torch.int64), symmetry=True)
    b = SI.obtain_skeleton_tree(nodes, alld, torch.zeros(nodes.shape[0], 1, dtype=torch.int32), symmetry=True)
    # the pass is opt-in: labels alone raise as they did before it existed, and symmetry=True alone has nothing to run on
    with pytest.raises(NotImplementedError, match="symmetry=True"):
        SI.obtain_skeleton_tree(nodes, alld, torch.zeros(nodes.shape[0], dtype=torch.int32))
    with pytest.raises(ValueError, match="seg_labels"):
        SI.obtain_skeleton_tree(nodes, alld, None, symmetry=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_library_exports_the_label_entry_and_sizes_the_node_tile_from_the_frames():
    """The node tile keeps F x T floats within 64 KiB of LDS; bad sizes and NULL buffers are refused before any HIP call."""
    from riggs_amd import _lib as L
    lib = L.lib()
    for name in ("riggs_node_semantic_tile", "riggs_node_semantic_labels"):
        assert name in L.exported_symbols() and hasattr(lib, name)
    assert [lib.riggs_node_semantic_tile(F) for F in (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024)] == [256, 256, 128, 128, 64, 64, 32, 32, 16, 16]
    assert all(4 * F * lib.riggs_node_semantic_tile(F) <= 64 * 1024 for F in range(1, 1025))
    assert lib.riggs_node_semantic_tile(0) == 0 and lib.riggs_node_semantic_tile(1025) == 0
    assert L.CONSTANTS["RIGGS_SEMANTIC_MAX_FRAMES"] == 1024 and L.CONSTANTS["RIGGS_SEMANTIC_MAX_NODES"] == 65536
    assert L.CONSTANTS["RIGGS_SEMANTIC_CAMERA_WORDS"] == 24 and L.ABI_VERSION == 102
    for F, M in ((0, 4), (1025, 4), (4, 0), (4, 65537)):
        assert lib.riggs_node_semantic_labels(F, M, None, None, None, None, None) != 0 and b"1 <= F <= 1024" in lib.riggs_last_error()
    assert lib.riggs_node_semantic_labels(4, 4, None, None, None, None, None) != 0 and b"NULL" in lib.riggs_last_error()
