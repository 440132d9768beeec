"""CPU: the host stages of the stage-2 skeleton extraction (riggs_amd/skeleton_init.py) against what the reference's stage
functions returned for the same inputs (tests/golden/skelinit_*.npz) — integer arrays equal, joint positions bit for bit —, the
key-frame choice, the skeleton_tree.npz round trip and the library's new entries."""
import os

import numpy as np
import pytest
import torch

from riggs_amd import skeleton_init as SI
from tests import skeleton_init_ref as R


@pytest.mark.parametrize("name", R.SKELETON_FIXTURES)
def test_every_host_stage_equals_the_reference(name):
    z = R.skeleton_fixture(name)
    sample = z["sample"]
    prim = SI.prim_tree(z["mean_distances"], 2)
    assert np.array_equal(prim, z["prim"])
    order1, parents1 = SI.reroot(z["prim"])
    assert np.array_equal(parents1, z["parents1"])
    assert np.array_equal(sample[order1], z["indices1"])
    pruned, nodes1 = SI.prune_tree(z["nodes"][z["indices1"]], z["parents1"])
    assert np.array_equal(pruned, z["pruned"])
    assert nodes1.dtype == np.float32 and np.array_equal(nodes1.view(np.uint32), z["nodes1"].view(np.uint32))
    simplified = SI.simplify_tree(z["all_deformed"][:, z["indices1"]], z["pruned"])
    assert np.array_equal(simplified, z["simplified"])
    order2, parents2 = SI.reroot(z["simplified"])
    assert np.array_equal(parents2, z["parents"])
    assert np.array_equal(z["indices1"][order2], z["indices"])
    assert np.array_equal(z["nodes1"][order2].view(np.uint32), z["joints"].view(np.uint32))
    # ... and chained, from the recorded distances and sample
    out = SI.tree_from_samples(z["nodes"][sample], sample, z["mean_distances"], z["all_deformed"])
    for k in ("prim", "parents1", "indices1", "pruned", "simplified", "parents", "indices"):
        assert np.array_equal(out[k], z[k]), k
    assert np.array_equal(out["joints"].view(np.uint32), z["joints"].view(np.uint32))
    assert len(z["parents"]) >= 11 and (z["simplified"] == -2).any()


def test_the_fixtures_reach_both_passes_of_the_pruning():
    """One fixture has side branches for the first pass to remove; three have a junction merged into another by the second."""
    z = R.skeleton_fixture("skelinit_per30_twigs")
    assert int((z["pruned"] == -2).sum()) > 10
    merged = [n for n in R.SKELETON_FIXTURES if (R.skeleton_fixture(n)["nodes1"] != R.skeleton_fixture(n)["nodes"][R.skeleton_fixture(n)["indices1"]]).any()]
    assert len(merged) >= 3


@pytest.mark.parametrize("name", R.SKELETON_FIXTURES)
def test_whole_extraction_on_cpu_tensors(name):
    z = R.skeleton_fixture(name)
    nodes, alld = torch.from_numpy(z["nodes"]), torch.from_numpy(z["all_deformed"])
    start = int(z["start"]) if nodes.shape[0] > 200 else None
    joints, parents, indices = SI.obtain_skeleton_tree(nodes, alld, None, start=start)
    assert joints.dtype == torch.float32 and parents.dtype == torch.int64 and indices.dtype == torch.int32
    assert torch.equal(parents, torch.from_numpy(z["parents"])) and int(parents[0]) == -1
    assert torch.equal(indices, torch.from_numpy(z["indices"]))
    assert np.array_equal(joints.numpy().view(np.uint32), z["joints"].view(np.uint32))
    assert torch.equal(nodes, torch.from_numpy(z["nodes"]))  # (merged junctions are written into a copy)


def test_select_key_frame_matches_the_recorded_choice():
    for name in R.SKELETON_FIXTURES:
        z = R.skeleton_fixture(name)
        alld = torch.from_numpy(z["all_deformed"])
        assert SI.select_key_frame(alld, torch.from_numpy(z["coverage"])) == int(z["key_frame"])
        assert SI.select_key_frame(alld) == int(z["key_frame_nearest"][0])  # no coverage: the frame nearest the mean
        assert SI.select_key_frame(alld, torch.from_numpy(z["coverage"]), manually_key_frame=3) == 3
    # (in at least one fixture the coverage overrules the nearest frame)
    assert any(int(R.skeleton_fixture(n)["key_frame"]) != int(R.skeleton_fixture(n)["key_frame_nearest"][0]) for n in R.SKELETON_FIXTURES)


def test_skeleton_tree_file_round_trip(tmp_path):
    z = R.skeleton_fixture("skelinit_per30")
    path = os.path.join(tmp_path, "skeleton_tree.npz")
    SI.save_skeleton_tree(path, torch.from_numpy(z["joints"]), torch.from_numpy(z["parents"]), torch.from_numpy(z["indices"]), 7)
    f = np.load(path)
    assert sorted(f.files) == ["indices", "nodes", "parents", "template_idx"]  # train_rig.py:233
    assert f["nodes"].dtype == np.float32 and f["parents"].dtype == np.int64 and f["indices"].dtype == np.int32
    assert f["template_idx"].dtype == np.int64 and f["template_idx"].shape == ()
    assert np.array_equal(f["nodes"], z["joints"]) and np.array_equal(f["parents"], z["parents"]) and np.array_equal(f["indices"], z["indices"])
    info = SI.load_skeleton_tree(path)
    assert torch.equal(info["joints"], torch.from_numpy(z["joints"])) and info["joints"].dtype == torch.float32
    assert torch.equal(info["parent_indices"], torch.from_numpy(z["parents"])) and info["parent_indices"].dtype == torch.int64
    assert torch.equal(info["joint_node_indices"], torch.from_numpy(z["indices"]).long()) and info["template_idx"] == 7
    with pytest.raises(FileNotFoundError):
        SI.load_skeleton_tree(os.path.join(tmp_path, "nothing.npz"))


def test_seg_labels_raise():
    z = R.skeleton_fixture("skelinit_per12")
    nodes, alld = torch.from_numpy(z["nodes"]), torch.from_numpy(z["all_deformed"])
    with pytest.raises(NotImplementedError, match="symmetry"):
        SI.obtain_skeleton_tree(nodes, alld, torch.zeros(nodes.shape[0], dtype=torch.int32))


def test_prim_needs_three_nodes_and_a_connected_graph():
    with pytest.raises(ValueError):
        SI.prim_tree(np.ones((2, 2), np.float32))
    with pytest.raises(ValueError):
        SI.prim_tree(np.zeros((4, 4), np.float32))  # no edge of positive weight


def test_library_exports_the_sampling_entries_and_sizes_the_grid_from_n():
    from riggs_amd import _lib as L
    lib = L.lib()
    for name in ("riggs_fps_blocks", "riggs_fps_workspace_bytes", "riggs_fps_sample"):
        assert name in L.exported_symbols() and hasattr(lib, name)
    assert lib.riggs_fps_blocks(200) == 1 and lib.riggs_fps_blocks(1024) == 1 and lib.riggs_fps_blocks(1025) == 2
    assert lib.riggs_fps_blocks(70001) == 69 and lib.riggs_fps_blocks(4100) == 5
    assert 256 <= lib.riggs_fps_blocks(300000) <= 1024 and lib.riggs_fps_blocks(2 ** 31 - 1) <= 1024
    for n in (1, 200, 70001, 300000):
        assert lib.riggs_fps_workspace_bytes(n) >= 4 * n + 16 * lib.riggs_fps_blocks(n)
    # bad sizes and NULL buffers are refused before any HIP call
    assert lib.riggs_fps_sample(0, 4, None, 3, None, None, None, None) != 0 and lib.riggs_last_error()
    assert lib.riggs_fps_sample(10, 4, None, 3, None, None, None, None) != 0 and b"NULL" in lib.riggs_last_error()
    assert lib.riggs_fps_sample(10, 4, None, 2, None, None, None, None) != 0


def test_cpu_and_other_shapes_keep_the_torch_loop():
    """gaussian_model.farthest_point_sample on what the kernel does not take: CPU tensors, batches, C != 3."""
    from riggs_amd.gaussian_model import farthest_point_sample
    pts, start, ref = R.fps_fixture("fps_n200_p200")
    got = farthest_point_sample(torch.from_numpy(pts)[None], 200, start=[start])
    assert torch.equal(got[0], torch.from_numpy(ref))
    two = farthest_point_sample(torch.from_numpy(pts)[None].repeat(2, 1, 1), 7, start=[start, start])
    assert torch.equal(two[0], two[1]) and torch.equal(two[0], torch.from_numpy(ref[:7]))
    assert farthest_point_sample(torch.randn(1, 50, 5), 9).shape == (1, 9)
