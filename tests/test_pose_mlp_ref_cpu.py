"""The PoseMLP references of tests/pose_mlp_ref.py on the host: the per-element bounds accept a numpy float32 restatement of both
kernel paths (one launch / one launch per layer) on every case of the GPU grid — in the kernels' lane order, reversed and permuted —
and reject each planted fault on the arrays it spoils and on no others; the stage references and the float64 autograd network agree;
the inputs of every case meet the vacuity condition; PoseMLP(depth <= 2) is not taken by the kernels."""
import types

import numpy as np
import pytest
import torch

from tests import pose_mlp_ref as P

GRID = P.grid()
DRAWS = [P.random_case(i) for i in range(16)]
CASES = GRID + DRAWS
_BY_NAME = {c["name"]: c for c in CASES}


def _paths(c):
    return [False, True] if P.one_launch(c) else [True]


def _bad(res):
    return sorted(k for k, v in res.items() if v["bad"])


def test_reseed_table_is_small_and_names_are_unique():
    assert len(_BY_NAME) == len(CASES)
    assert set(P.RESEED) <= set(_BY_NAME)
    assert len(P.RESEED) <= 0.05 * len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_is_accepted_and_the_inputs_are_not_vacuous(case):
    c, p = P.make(case)
    for layered in _paths(c):
        P.assert_case_is_safe(c, p, layered)
        out = P.restate(c, p, layered)
        res = P.check_stages(c, p, out, layered)
        P.check_end_to_end(c, p, out, layered, res)
        assert not _bad(res), (layered, {k: res[k] for k in _bad(res)})
        # the vacuity condition (on the inputs): per array at most 1 % of the non-zero-reference elements have bound >= |reference|
        vac = {k: v["vac"] for k, v in res.items() if v["vac"] > 0.01}
        assert not vac, (layered, vac)
        for order in ("reversed", 3):
            res = P.check_stages(c, p, P.restate(c, p, layered, order=order), layered)
            assert not _bad(res), (layered, order, {k: res[k] for k in _bad(res)})


@pytest.mark.parametrize("name,t", [(n, t) for n in P.STATE_CASES for t in P.STATE_TS] + [(P.EMBED_CASE, t) for t in P.EMBED_TS])
def test_the_other_times_of_the_gpu_tests_are_safe_too(name, t):
    c, p = P.make(_BY_NAME[name])
    p["t"] = np.float32(t)
    P.assert_case_is_safe(c, p, False)
    assert not _bad(P.check_stages(c, p, P.restate(c, p, False), False))


# fault -> (grid case it is planted in, the stage arrays it spoils)
FAULTS = {
    "emb_behind": ("inside 256x24", {"acts", "dW"}),
    "skip_late": ("inside 256x24", {"acts", "dW"}),
    "chunk5": ("inside 256x24", {"acts"}),
    "head_bias": ("extra 128x64", {"rotation", "translation"}),
    "rot_bias_idx": ("inside 256x24", {"rotation"}),
    "sincos": ("inside 256x24", {"emb"}),
    "freq": ("inside 256x24", {"emb"}),
    "mask_next": ("inside 256x24", {"v"}),
    "head256": ("extra 256x64", {"v"}),
    "no_tr_rows": ("inside 256x24", {"v"}),
    "dw_emb_from_h": ("inside 256x24", {"dW"}),
    "late_row": ("inside 256x24", {"v", "dW", "db_heads"}),
    "stale": ("inside 256x24", {"acts", "v"}),
    "no_gn_sum": ("fk J=24", {"dgt"}),
    "no_g_rot": ("fk J=24", {"dq"}),
    "unit1": ("fk J=24", {"dq", "fixed_loss"}),
}
_ONE_LAUNCH_ONLY = {"late_row", "stale"}  # (hand-offs and late rows exist in the one-launch kernels only)


def _faulty(name, fault, layered, pick="max"):
    c, p = P.make(_BY_NAME[name])
    prev = None
    if fault == "stale":
        p2 = dict(p)
        p2["t"] = np.float32(0.81)  # (the previous launch: another time, other cotangents)
        p2["g_rot"], p2["g_tr"] = p["g_rot"][::-1].copy(), -p["g_tr"]
        prev = P.restate(c, p2, layered)
    return c, p, P.restate(c, p, layered, fault=fault, prev=prev, pick=pick)


def test_every_listed_fault_is_planted():
    assert set(FAULTS) == set(P.FAULTS) and len(FAULTS) == 16


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_fault_is_rejected_on_the_arrays_it_spoils_and_on_no_others(fault):
    name, spoiled = FAULTS[fault]
    for layered in ([False] if fault in _ONE_LAUNCH_ONLY else [False, True]):
        c, p, out = _faulty(name, fault, layered)
        res = P.check_stages(c, p, out, layered)
        assert set(_bad(res)) == spoiled, (fault, layered, _bad(res))
        e2e = P.check_end_to_end(c, p, out, layered, {}, strict=False)
        assert _bad(e2e), (fault, layered, "the end-to-end reference lets it through")
    if fault == "stale":  # (not only the unit that changed most between the launches: the median one as well)
        c, p, out = _faulty(name, fault, False, pick="median")
        assert set(_bad(P.check_stages(c, p, out, False))) == spoiled


def old_bars(c, p, out):
    """The bars of test_fused_pose_mlp_matches_torch_and_reference_fixture: 1e-5 of the largest entry on the outputs, 1e-4 of a
    parameter gradient's largest entry.  True: the fault passes them."""
    ref = P.end_to_end(c, p)
    for k in ("rotation", "translation"):
        if np.abs(out[k] - ref[k]).max() > 1e-5 * np.abs(ref[k]).max() or not np.isfinite(out[k]).all():
            return False
    lay, _ = P.layout(c)
    for w_off, b_off, rows, n in lay:
        for lo, hi in ((w_off, w_off + rows * n), (b_off, b_off + rows)):
            g, r = out["flat"][lo:hi].astype(np.float64), ref["flat"][lo:hi]
            if not np.isfinite(g).all() or np.abs(g - r).max() > 1e-4 * max(np.abs(r).max(), 1e-12):
                return False
    return True


def test_what_the_old_bars_let_through(capsys):
    """Not an assertion on the old bars (they stay where they are): the figures of NOTES.md, printed.  Faults of the _fk entry and of
    head rows beyond the width are out of the old test's reach (it runs neither); the others are planted in its (256, 24) shape."""
    passed = []
    for fault in sorted(FAULTS):
        name = FAULTS[fault][0]
        c, p, out = _faulty(name, fault, False)
        if old_bars(c, p, out):
            passed.append(fault)
    if old_bars(*_faulty("inside 256x24", "stale", False, pick="median")):
        passed.append("stale (the median unit)")
    with capsys.disabled():
        print("\nplanted faults that pass the old max-norm bars:", passed)
    c, p = P.make(_BY_NAME["inside 256x24"])
    assert old_bars(c, p, P.restate(c, p, False))  # (the bars themselves accept the restatement)


@pytest.mark.parametrize("name", ["inside 256x24", "extra 128x64", "depth 3 skip 2", "multires 0", "depth 1 skip 0"])
def test_the_two_references_agree_on_given_masks(name):
    c, p = P.make(_BY_NAME[name])
    g = np.random.default_rng(5)
    masks = [(g.random(c["width"]) < 0.5).astype(np.float64) for _ in range(c["depth"])]
    a, b = P.compose_stages(c, p, masks), P.end_to_end(c, p, masks=masks)
    for k in ("rotation", "translation", "flat"):
        assert np.abs(a[k] - b[k]).max() <= 1e-10 * max(1.0, np.abs(b[k]).max()), k


def test_exact_zeros_are_compared_exactly():
    c, p = P.make(_BY_NAME["dead layer"])
    out = P.restate(c, p, False)
    lay, _ = P.layout(c)
    assert not out["flat"][: lay[5][1] + c["width"]].any()  # everything below the dead layer
    out["flat"][3] = np.float32(1e-30)
    assert "dW" in _bad(P.check_stages(c, p, out, False))


@pytest.mark.parametrize("depth,fusable", [(1, False), (2, False), (3, True), (8, True)])
def test_depth_two_and_less_is_not_taken_by_the_kernels(depth, fusable):
    """skips[0] == depth - 1 there: the module's heads are Linear(hidden, ...) while h has become [emb, h] — the reference raises a
    shape error, and the kernels would stride the head rows by width + emb past the end of W_rot / W_tr."""
    from riggs_amd.skeleton import PoseMLP
    net = PoseMLP(1, 16, depth=depth, hidden_dimensions=32)
    t = types.SimpleNamespace(is_cuda=True, dtype=torch.float32, numel=lambda: 1)
    assert net._fusable(t) is fusable
    if not fusable:
        with pytest.raises(RuntimeError):
            net(torch.tensor([0.37]))
