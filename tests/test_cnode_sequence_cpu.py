"""CPU: the control-node sequence blend's declarations, its oracle (tests/cnode_sequence_ref.py) and the reference's goldens
(tests/golden/cnodeseq_*.npz, written by tests/golden/make_cnode_sequence_golden.py)."""
import os
import re

import numpy as np
import pytest

from tests import cnode_sequence_ref as SR

SYMBOLS = ("riggs_cnode_sequence_forward", "riggs_cnode_sequence_pass_frames")


def test_header_declares_both_symbols_and_the_binding_exposes_them():
    import ctypes as C
    from riggs_amd import _abi, _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "riggs_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert set(SYMBOLS) <= set(_lib.exported_symbols())
    res, args = _abi.FUNCTIONS["riggs_cnode_sequence_forward"]
    fwd = _abi.FUNCTIONS["riggs_cnode_forward"][1]
    # riggs_cnode_forward's arguments with T after M
    assert res is C.c_int and len(args) == len(fwd) + 1 == 25 and list(args[:2]) + list(args[3:]) == list(fwd)
    res, args = _abi.FUNCTIONS["riggs_cnode_sequence_pass_frames"]
    assert res is C.c_int32 and list(args) == [C.c_int32, C.c_int32]
    from riggs_amd.control_nodes import ControlNodeWarp
    from riggs_amd import playback, skeleton_init
    import inspect
    assert callable(ControlNodeWarp.deform_sequence) and callable(playback.render_time_sequence)
    assert inspect.signature(skeleton_init.precompute_deformations).parameters["sequence_chunk"].default is None
    assert inspect.signature(playback.render_time_sequence).parameters["chunk"].default == 32


def test_oracle_equals_a_hand_written_two_frame_case():
    """Two Gaussians, two nodes, K = 1, no hyper coordinates, mask (1, 0.5): Gaussian 0 sits on node 0, Gaussian 1 next to node
    1, so every weight is 1 and each output is its node's record (times the mask), written out by hand."""
    x = np.array([[0.0, 0.0, 0.0], [1.0, 0.25, 0.0]])
    nodes = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    mask = np.array([[1.0], [0.5]])
    attrs = {"d_xyz": np.array([[[0.1, 0.2, 0.3], [1.0, 0.0, -1.0]], [[0.0, -0.5, 0.0], [0.0, 2.0, 0.0]]]),
             "d_rotation": np.array([[[0.1, 0.0, 0.0, 0.2], [0.0, 0.4, 0.0, 0.0]], [[0.0, 0.0, 0.0, 0.0], [0.2, 0.2, 0.2, 0.2]]]),
             "d_scaling": np.array([[[0.01, 0.02, 0.03], [0.2, 0.4, 0.6]], [[0.0, 0.0, 0.1], [-0.2, 0.0, 0.2]]]),
             # node 1 turns by 90 degrees about z in frame 0 (q = (1, 0, 0, 1) after the bias, un-normalised), not in frame 1
             "local_rotation": np.array([[[0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]], [[0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]]])}
    kw = dict(K=1, hyper_dim=0)
    out = SR.forward_sequence(x, None, mask, nodes, np.zeros(2), None, attrs, local_frame=False, d_rot_as_res=True, **kw)
    assert np.array_equal(out["nn_idx"], [[0], [1]]) and np.allclose(out["nn_weight"], 1.0) and np.allclose(out["nn_dist"], [[0.0], [0.0625]])
    assert out["d_xyz"].shape == (2, 2, 3) and out["d_rotation"].shape == (2, 2, 4) and out["d_nodes"].shape == (2, 2, 3)
    np.testing.assert_allclose(out["d_xyz"], [[[0.1, 0.2, 0.3], [0.5, 0.0, -0.5]], [[0.0, -0.5, 0.0], [0.0, 1.0, 0.0]]], atol=1e-15)
    np.testing.assert_allclose(out["d_rotation"], [[[0.1, 0.0, 0.0, 0.2], [0.0, 0.2, 0.0, 0.0]], [[0.0] * 4, [0.1] * 4]], atol=1e-15)
    np.testing.assert_allclose(out["d_scaling"], [[[0.01, 0.02, 0.03], [0.1, 0.2, 0.3]], [[0.0, 0.0, 0.1], [-0.1, 0.0, 0.1]]], atol=1e-15)
    np.testing.assert_allclose(out["d_nodes"], nodes[None] + attrs["d_xyz"], atol=1e-15)
    # local frame + absolute rotation: Gaussian 1's offset (0, 0.25, 0) to node 1 turns into (-0.25, 0, 0) in frame 0
    out = SR.forward_sequence(x, None, mask, nodes, np.zeros(2), None, attrs, local_frame=True, d_rot_as_res=False, **kw)
    np.testing.assert_allclose(out["d_xyz"][0, 1], 0.5 * (np.array([-0.25, 0.0, 0.0]) + nodes[1] + attrs["d_xyz"][0, 1] - x[1]), atol=1e-15)
    np.testing.assert_allclose(out["d_xyz"][1, 1], 0.5 * attrs["d_xyz"][1, 1], atol=1e-15)
    np.testing.assert_allclose(out["d_xyz"][:, 0], attrs["d_xyz"][:, 0], atol=1e-15)
    # (sum w (rot + e) - e) m + e
    np.testing.assert_allclose(out["d_rotation"][0, 1], 0.5 * attrs["d_rotation"][0, 1] + [1.0, 0.0, 0.0, 0.0], atol=1e-15)
    # the lists can be handed in, and T = 0 keeps the shapes
    swapped = SR.forward_sequence(x, None, mask, nodes, np.zeros(2), None, attrs, local_frame=False, d_rot_as_res=True,
                                  nn_idx=np.array([[1], [0]]), **kw)
    np.testing.assert_allclose(swapped["d_scaling"][0], [[0.2, 0.4, 0.6], [0.005, 0.01, 0.015]], atol=1e-15)
    empty = SR.forward_sequence(x, None, mask, nodes, np.zeros(2), None, {k: v[:0] for k, v in attrs.items()}, local_frame=False,
                                d_rot_as_res=True, **kw)
    assert empty["d_xyz"].shape == (0, 2, 3) and empty["nn_idx"].shape == (2, 1)


@pytest.mark.parametrize("name", SR.GOLDENS)
def test_golden_loads_with_its_keys_shapes_and_tie_gap(name):
    z = SR.golden(name)
    N, M, T, K, h = 300, 48, 4, int(z["K"]), int(z["hyper_dim"])
    pred = bool(z["pred"])
    assert K == 3 and z["x"].shape == (N, 3) and z["nodes"].shape == (M, 3 + h) and z["times"].shape == (T,)
    assert z["_node_radius"].shape == (M,) and z["_node_weight"].shape == (M, 1) and z["motion_mask"].shape == (N, 1)
    assert z["feature"].shape == ((N, h + 1) if h else (0, 0))
    for k, c in (("d_xyz", 3), ("d_rotation", 4), ("d_scaling", 3), ("local_rotation", 4), ("d_opacity", 1), ("d_color", 3)):
        assert z["attr_" + k].shape == (T, M, c) and z["attr_" + k].dtype == np.float32, k
    widths = {"d_xyz": (N, 3), "d_rotation": (N, 4), "d_scaling": (N, 3), "d_nodes": (M, 3)}
    if pred:
        widths.update(d_opacity=(N, 1), d_color=(N, 3))
    assert {k for k in z.files if k.startswith("out_")} == {"out_" + k for k in widths}
    for k, s in widths.items():
        assert z["out_" + k].shape == (T,) + s and np.isfinite(z["out_" + k]).all(), k
    assert z["nn_idx"].shape == (N, K) and z["nn_idx"].dtype == np.int32 and z["nn_weight"].shape == (N, K) and z["nn_dist"].shape == (N, K)
    # no row is at a near-tie of its K-th and (K+1)-th node, so float32 and float64 select alike and nn_idx is compared exactly
    assert SR.tie_gap(z) > SR.TIE_GAP and abs(SR.tie_gap(z) - float(z["tie_gap"])) < 1e-12
    # and the oracle reproduces the reference's frames from the file's inputs, lists included
    attrs = {k: z["attr_" + k] for k in ("d_xyz", "d_rotation", "d_scaling", "local_rotation")}
    out = SR.forward_sequence(z["x"], z["feature"] if h else None, z["motion_mask"], z["nodes"], z["_node_radius"], z["_node_weight"],
                              attrs, K=K, hyper_dim=h, local_frame=bool(z["local_frame"]), d_rot_as_res=bool(z["d_rot_as_res"]))
    assert np.array_equal(out["nn_idx"], z["nn_idx"])
    assert np.abs(out["nn_weight"] - z["nn_weight"]).max() < 2e-6
    for k in SR.OUTS:
        assert np.abs(out[k] - z["out_" + k]).max() <= 1e-5 * max(1.0, np.abs(z["out_" + k]).max()), k
