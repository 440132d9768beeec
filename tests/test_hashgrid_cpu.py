"""CPU: the hash-grid encoding's level table (the library's host function against the oracle tests/hashgrid_ref.py and against
hand-computed values), the oracle's own known answers, the cosine band mask against the masks recorded from the reference, and the
rejections that need no device."""
import json
import os

import numpy as np
import pytest
import torch

from tests import hashgrid_ref as HR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMALL = dict(n_levels=5, n_features_per_level=2, log2_hashmap_size=10, base_resolution=3, per_level_scale=1.5)


def c_table(D, cfg):
    from riggs_amd import hash_network as HN
    lv = HN.hashgrid_levels(D, cfg)
    L = lv.n_levels
    return [dict(scale=np.float32(lv.scale[l]), resolution=int(lv.resolution[l]), size=int(lv.size[l]), offset=int(lv.offset[l]),
                 hashed=bool(lv.hashed[l])) for l in range(L)], int(lv.offset[L])


def test_reference_configuration_level_table():
    for D in (3, 4):
        levels, total = HR.level_table(D, **HR.REFERENCE_CONFIG)
        assert [lv["resolution"] for lv in levels] == [16 * 2 ** l for l in range(12)]
        assert [float(lv["scale"]) for lv in levels] == [16.0 * 2 ** l - 1 for l in range(12)]
        if D == 3:
            assert [lv["size"] for lv in levels] == [4096, 32768, 262144] + [2 ** 19] * 9
            assert [lv["hashed"] for lv in levels] == [False] * 3 + [True] * 9
            assert total == 4096 + 32768 + 262144 + 9 * 2 ** 19 == 5017600
        else:
            assert [lv["size"] for lv in levels] == [65536] + [2 ** 19] * 11      # 16^4 = 65 536 is dense, 32^4 = 2^20 is hashed
            assert [lv["hashed"] for lv in levels] == [False] + [True] * 11
        assert [lv["offset"] for lv in levels] == list(np.cumsum([0] + [lv["size"] for lv in levels[:-1]]))


def test_small_configuration_where_the_cell_count_is_no_multiple_of_8():
    """base 3, scale 1.5, 2^10: scales 2, 3.5, 5.75, 9.125, 14.1875 -> resolutions 3, 5, 7, 11, 16 (ceil + 1)."""
    levels, total = HR.level_table(3, **SMALL)
    assert [float(lv["scale"]) for lv in levels] == [2.0, 3.5, 5.75, 9.125, 14.1875]
    assert [lv["resolution"] for lv in levels] == [3, 5, 7, 11, 16]
    assert [lv["size"] for lv in levels] == [32, 128, 344, 1024, 1024]              # 27 -> 32, 125 -> 128, 343 -> 344, 1331 and 4096 -> 2^10
    assert [lv["hashed"] for lv in levels] == [False, False, False, True, True]
    assert total == 2552
    levels4, _ = HR.level_table(4, **SMALL)
    assert [lv["size"] for lv in levels4] == [88, 632, 1024, 1024, 1024]            # 81 -> 88, 625 -> 632, then 2401, 14641, 65536 -> 2^10
    assert [lv["hashed"] for lv in levels4] == [False, False, True, True, True]


@pytest.mark.parametrize("D", [3, 4])
@pytest.mark.parametrize("cfg", [HR.REFERENCE_CONFIG, SMALL, dict(SMALL, n_levels=12, base_resolution=2, per_level_scale=2.0),
                                 dict(HR.REFERENCE_CONFIG, n_levels=16, log2_hashmap_size=24, per_level_scale=1.38),
                                 dict(HR.REFERENCE_CONFIG, n_levels=16, log2_hashmap_size=3, base_resolution=1)])
def test_c_level_table_equals_the_oracle(D, cfg):
    got, total = c_table(D, cfg)
    want, wtotal = HR.level_table(D, **cfg)
    assert total == wtotal and len(got) == len(want)
    for g, w in zip(got, want):
        assert g["scale"] == w["scale"] and g["scale"].dtype == np.float32
        assert (g["resolution"], g["size"], g["offset"], g["hashed"]) == (w["resolution"], w["size"], w["offset"], w["hashed"])


def test_new_symbols_are_exported_and_the_abi_version_is_unchanged():
    from riggs_amd import _lib as L
    lib = L.lib()
    for name in ("riggs_hashgrid_levels_fill", "riggs_hashgrid_forward", "riggs_hashgrid_backward"):
        assert name in L.exported_symbols() and hasattr(lib, name)
    assert L.ABI_VERSION == 102 and lib.riggs_version() == 102  # (unchanged by the hash grid; 102 since the fused heads' entries were folded)
    K = L.CONSTANTS
    assert K["RIGGS_HASHGRID_MAX_LEVELS"] == 16
    assert K["RIGGS_HASHGRID_TABLE_WORDS"] == K["RIGGS_HASHGRID_HEADER_WORDS"] + 16 * K["RIGGS_HASHGRID_LEVEL_WORDS"]


def test_c_entries_reject_bad_arguments_before_any_hip_call():
    import ctypes as C
    from riggs_amd import _lib as L
    from riggs_amd import hash_network as HN
    lib = L.lib()
    words = (C.c_uint32 * L.CONSTANTS["RIGGS_HASHGRID_TABLE_WORDS"])()
    for args in ((2, 12, 2, 19, 16.0, 2.0), (5, 12, 2, 19, 16.0, 2.0), (3, 0, 2, 19, 16.0, 2.0), (3, 17, 2, 19, 16.0, 2.0),
                 (3, 12, 4, 19, 16.0, 2.0), (3, 12, 1, 19, 16.0, 2.0), (3, 12, 2, 25, 16.0, 2.0), (3, 12, 2, 19, 0.5, 2.0),
                 (3, 16, 2, 19, 16.0, 8.0)):
        assert lib.riggs_hashgrid_levels_fill(*args, words) != 0 and lib.riggs_last_error()
    assert lib.riggs_hashgrid_levels_fill(3, 12, 2, 19, 16.0, 2.0, None) != 0
    empty = (C.c_uint32 * L.CONSTANTS["RIGGS_HASHGRID_TABLE_WORDS"])()
    assert lib.riggs_hashgrid_forward(empty, 4, 8, 8, None, 8, None) != 0 and b"riggs_hashgrid_levels_fill" in lib.riggs_last_error()
    good = HN.hashgrid_levels(3).words
    assert lib.riggs_hashgrid_forward(good, -1, 8, 8, None, 8, None) != 0
    assert lib.riggs_hashgrid_forward(good, 2 ** 27, 8, 8, None, 8, None) != 0      # R L F >= 2^31
    assert lib.riggs_hashgrid_forward(good, 4, None, 8, None, 8, None) != 0 and b"NULL" in lib.riggs_last_error()
    assert lib.riggs_hashgrid_forward(good, 4, 8, 4, None, 8, None) != 0 and b"aligned" in lib.riggs_last_error()
    assert lib.riggs_hashgrid_backward(good, 4, 8, None, None, 8, None) != 0 and b"NULL" in lib.riggs_last_error()
    assert lib.riggs_hashgrid_backward(good, 4, 8, None, 8, 12, None) != 0 and b"aligned" in lib.riggs_last_error()
    broken = HN.hashgrid_levels(3).words
    broken[L.CONSTANTS["RIGGS_HASHGRID_HEADER_WORDS"] + 3 * L.CONSTANTS["RIGGS_HASHGRID_LEVEL_WORDS"] + 3] += 8    # level 3's window off the running sum
    assert lib.riggs_hashgrid_forward(broken, 4, 8, 8, None, 8, None) != 0
    assert lib.riggs_hashgrid_forward(good, 0, None, None, None, None, None) == 0    # no rows: nothing to do


def test_python_rejections_without_a_device():
    from riggs_amd import _lib as L
    from riggs_amd import hash_network as HN
    with pytest.raises(L.RiggsHipError, match="n_features_per_level"):
        HN.hashgrid_levels(3, {"n_features_per_level": 4})
    with pytest.raises(L.RiggsHipError, match="n_input_dims"):
        HN.hashgrid_levels(2)
    with pytest.raises(NotImplementedError, match="interpolation"):
        HN.hashgrid_levels(3, {"interpolation": "Smoothstep"})
    with pytest.raises(NotImplementedError, match="tcnn_mlp"):
        HN.HashDeformNetwork(tcnn_mlp=True, device="cpu")
    enc = HN.HashGridEncoding(3, SMALL, device="cpu")
    assert enc.n_output_dims == 10 and enc.params.shape == (2 * 2552,) and float(enc.params.detach().abs().max()) <= 1e-4
    with pytest.raises(L.RiggsHipError, match="CUDA"):
        enc(torch.rand(5, 3))
    with pytest.raises(L.RiggsHipError, match="detached"):
        enc(torch.rand(5, 3, requires_grad=True))
    with pytest.raises(L.RiggsHipError, match=r"\(R, 3\)"):
        enc(torch.rand(5, 4))


def test_oracle_dense_level_reproduces_trilinear_interpolation():
    """One dense level of resolution 5 (scale 3.5) holding value(i) = (i, 2 i): the index of corner (cx, cy, cz) is
    cx + 5 cy + 25 cz, linear in the corner, so interpolation returns it at the continuous position pos = 3.5 x + 0.5:
    feature 0 = px + 5 py + 25 pz.  Hand-computed: x = (0, 0, 0) -> pos 0.5 each -> 15.5; x = (1, 1, 1) -> pos 4 -> 124;
    x = (0.5, 0.25, 0.75) -> pos (2.25, 1.375, 3.125) -> 2.25 + 6.875 + 78.125 = 87.25."""
    cfg = dict(n_levels=1, n_features_per_level=2, log2_hashmap_size=10, base_resolution=4.5, per_level_scale=1.0)
    levels, total = HR.level_table(3, **cfg)
    assert levels[0]["resolution"] == 5 and total == 128 and not levels[0]["hashed"]
    table = np.stack([np.arange(total), 2.0 * np.arange(total)], 1)
    x = np.array([[0, 0, 0], [1, 1, 1], [0.5, 0.25, 0.75]], dtype=np.float32)
    out = HR.encode(x, table, 3, cfg)
    assert np.array_equal(out[:, 0], [15.5, 124.0, 87.25]) and np.array_equal(out[:, 1], 2 * out[:, 0])
    # x = 1 lies on the last grid plane: cell 4 with frac 0, so the corner beyond the grid (5, .., ..) carries weight 0
    idx, w = HR.corners(x[1:2], levels[0], 3)
    assert idx[0, 0] == 124 and w[0, 0] == 1.0 and np.count_nonzero(w) == 1


def test_oracle_weights_sum_to_one_and_indices_stay_in_range():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.random((200, 4)) * 1.6 - 0.3, [[0, 0, 0, 0], [1, 1, 1, 1], [-0.2, 1.3, 0.5, -7.0]]]).astype(np.float32)
    for D in (3, 4):
        for cfg in (HR.REFERENCE_CONFIG, SMALL):
            for lv in HR.level_table(D, **cfg)[0]:
                idx, w = HR.corners(x[:, :D], lv, D)
                assert np.allclose(w.sum(1), 1.0, rtol=0, atol=1e-12) and (w >= 0).all()
                assert idx.min() >= 0 and idx.max() < lv["size"]


def test_oracle_gradient_is_the_transpose_of_the_forward():
    """<encode(table), g> is linear in the table: its gradient is what the oracle returns, checked on unit tables; a zero mask
    column gets no gradient, and g_abs bounds |g_table|."""
    rng = np.random.default_rng(6)
    x = (rng.random((9, 3)) * 1.4 - 0.2).astype(np.float32)
    total = HR.level_table(3, **SMALL)[1]
    g = rng.standard_normal((9, 10))
    mask = np.array([1, 1, 0.5, 0, 0, 0, 1, 0.25, 1, 1.0])
    _, gt, ga = HR.encode(x, np.zeros((total, 2)), 3, SMALL, mask=mask, g_out=g)
    assert (np.abs(gt) <= ga + 1e-15).all()
    for e in list(np.argwhere(ga > 0)[::7]) + [np.array([40, 1])]:
        unit = np.zeros((total, 2))
        unit[e[0], e[1]] = 1.0
        assert abs((HR.encode(x, unit, 3, SMALL, mask=mask) * g).sum() - gt[e[0], e[1]]) < 1e-12
    lv = HR.level_table(3, **SMALL)[0]
    assert not gt[lv[2]["offset"]:lv[2]["offset"] + lv[2]["size"]].any()       # level 2: both mask columns are 0
    assert not gt[lv[1]["offset"]:lv[2]["offset"], 1].any() and gt[lv[1]["offset"]:lv[2]["offset"], 0].any()


def test_cosine_mask_against_the_recorded_masks():
    """ProgressiveBandHashGridCosine.update_step on the CPU against what the reference's class left in ``mask`` (same torch
    operations: equal bits), and both against the rule's text in float64."""
    from riggs_amd import hash_network as HN
    for name, D in (("xyz", 3), ("xyzt", 4)):
        z = np.load(os.path.join(GOLDEN, "hashgrid_net_%s.npz" % name))
        grid = HN.ProgressiveBandHashGridCosine(D, device="cpu")
        assert grid.n_masking_step == 6000 and grid.n_output_dims == 24 and int(grid.current_step) == 0
        assert np.array_equal(grid.mask.numpy(), z["mask_0"]) and not z["mask_0"][12:].any() and z["mask_0"][:12].all()
        for step in (3000, 3250, 7000):
            grid.update_step(step)
            assert np.array_equal(grid.mask.numpy(), z["mask_%d" % step]), step
            assert np.abs(z["mask_%d" % step] - HR.cosine_mask(step)).max() < 1e-6
            assert int(grid.current_step) == step and grid.current_step.dtype == torch.int32
        grid.update_step(100)                      # an older step changes nothing
        assert np.array_equal(grid.mask.numpy(), z["mask_7000"]) and int(grid.current_step) == 7000
        grid.update_step(-1)
        assert int(grid.current_step) == 7000
        assert abs(z["mask_3250"][18] - 0.5) < 1e-6 and z["mask_3250"][17] == 1.0 and z["mask_3250"][19] == 0.0   # half-way up column 18


def test_state_dict_names_and_shapes_are_the_reference_s():
    from riggs_amd import hash_network as HN
    layout = json.load(open(os.path.join(GOLDEN, "hashgrid_state_dict_layout.json")))
    assert len(layout["no_hash_time"]) == 33 and len(layout["hash_time"]) == 29
    assert layout["no_hash_time"]["mlp.layers.0.weight"] == [256, 37] and layout["hash_time"]["mlp.layers.0.weight"] == [256, 24]
    for key, hash_time in (("no_hash_time", False), ("hash_time", True)):
        net = HN.HashDeformNetwork(hash_time=hash_time, local_frame=True, pred_opacity=True, device="cpu")
        sd = net.state_dict()
        assert list(sd.keys()) == list(layout[key].keys())
        assert {k: list(v.shape) for k, v in sd.items()} == layout[key]
        assert sd["hashgrid.current_step"].dtype == torch.int32 and sd["bbox"].tolist() == [-2.0, 2.0]
        if not hash_time:
            assert float(net.mlp.layers[-1].weight.detach().std()) < 2e-5 and not net.mlp.layers[-1].bias.any()
