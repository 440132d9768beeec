"""tests/cnode_f64_ref.py on the host: the autograd reference agrees with the hand-derived oracle/cnode_ref.py on given lists;
its per-element bounds accept an fp32 restatement of the kernel's formulas whose node rows are summed in three orders, reject the
faults the GPU test (tests/test_gpu_cnode_f64.py) is there to catch — each planted fault is its own case — and are not vacuous
on any case of that test's grid."""
import numpy as np
import pytest
import torch

from oracle import cnode_ref as O
from tests import cnode_f64_ref as R
from tests import test_gpu_cnode_f64 as G

F = torch.float32
NODE_CAP, GAUSS_CAP = 0.01, 0.10


# ------------------------------------------------------------------------------------------------ the fp32 restatement
def node_sum32(rows, flat, M, perm):
    """Per-node sums of the entries' rows (N K, W) in fp32 with the reduce kernel's structure: the node's rows in the order
    ``perm`` leaves them, row p to lane p % 32 and partial (p // 32) % 4, the four partials as a tree, the 32 lanes in sequence."""
    rows, flat = rows[perm], flat[perm]
    order = torch.argsort(flat, stable=True)
    off = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(torch.bincount(flat, minlength=M), 0)]).tolist()
    W = rows.shape[1]
    out = torch.zeros(M, W, dtype=F)
    for n in range(M):
        seg = rows[order[off[n]:off[n + 1]]]
        if seg.shape[0] == 0:
            continue
        seg = torch.cat([seg, torch.zeros((-seg.shape[0]) % 128, W, dtype=F)]).reshape(-1, 4, 32, W)
        acc = seg[0].clone()
        for j in range(1, seg.shape[0]):
            acc = acc + seg[j]
        lane = (acc[0] + acc[1]) + (acc[2] + acc[3])
        v = torch.zeros(W, dtype=F)
        for r in range(32):
            v = v + lane[r]
        out[n] = v
    return out


def kernel32(c, t, idx, order="stored", fault=None):
    """cnode.hip's forward and backward formulas in fp32 torch on the lists ``idx``; ``fault`` plants one error."""
    N, M, K, H = c["N"], c["M"], c["K"], c["hyper"]
    x, nodes, cot = t["x"], t["nodes"], t["cot"]
    E = torch.tensor([1.0, 0, 0, 0])
    n3 = nodes[:, :3]
    rel = x[:, None] - n3[idx]
    d = torch.zeros(N, K)
    for j in range(3):
        d = d + rel[..., j] * rel[..., j]
    if H:
        diff = t["feature"][:, None, :H] - nodes[idx, 3:3 + H]
        for j in range(H):
            d = d + diff[..., j] * diff[..., j]
    r = torch.exp(t["radius"])
    r2 = (r * r)[idx]
    e = torch.exp(-d / (2.0 * r2))
    sg = None if t["weight"] is None else 1.0 / (1.0 + torch.exp(-t["weight"]))
    u = e if sg is None else e * sg[idx]
    v = u + 1e-7
    S = torch.zeros(N)
    for k in range(K):
        S = S + v[:, k]
    w = v / S[:, None]
    m = torch.ones(N) if t["mask"] is None else t["mask"]
    tr, ro, sc = t["attrs"]["d_xyz"], t["attrs"]["d_rotation"], t["attrs"]["d_scaling"]
    lq = t["attrs"]["local_rotation"].clone().requires_grad_(True)
    if c["local"]:
        Rm = R.quat_to_R(lq + E)
        y = ((Rm.detach()[idx] @ rel[..., None])[..., 0] + n3[idx]) + tr[idx]
    else:
        y = tr[idx]
    bias = 0.0 if c["res"] else 1.0
    roe = (ro + bias * E)[idx]
    sci = sc[idx]
    wsum = lambda a: sum(w[:, k, None] * a[:, k] for k in range(K))  # noqa: E731
    ts, rs, ss = wsum(y), wsum(roe), wsum(sci)
    if c["local"]:
        ts = ts - x
    out = {"d_xyz": ts * m[:, None], "d_rotation": (rs - bias * E) * m[:, None] + bias * E, "d_scaling": ss * m[:, None],
           "nn_weight": w, "nn_dist": d}
    z = lambda wd: torch.zeros(N, wd)  # noqa: E731
    g, h, s = (z(wd) if cot[k] is None else cot[k] for k, wd in (("g_xyz", 3), ("g_rot", 4), ("g_scale", 3)))
    a = m[:, None] * ((g[:, None] * y).sum(-1) + (h[:, None] * roe).sum(-1) + (s[:, None] * sci).sum(-1))
    wa = (w * a).sum(1, keepdim=True)
    Sb = u.sum(1) if fault == "no_eps" else S
    dv = (a if fault == "drop_wdw" else a - wa) / Sb[:, None]
    if t["mask"] is not None:
        rsm = rs.clone()
        if fault != "mask_bias":
            rsm[:, 0] = rsm[:, 0] - bias
        out["g_mask"] = (g * ts).sum(1) + (h * rsm).sum(1) + (s * ss).sum(1)
    c1 = w if fault == "no_mask_rows" else w * m[:, None]
    TR = c1[..., None, None] * (g[:, None, None, :] * rel[:, :, :, None] if fault == "transpose_dR" else g[:, None, :, None] * rel[:, :, None, :])
    cols = [c1[..., None] * g[:, None], c1[..., None] * h[:, None], c1[..., None] * s[:, None], TR.reshape(N, K, 9),
            (dv * u * d / (r[idx] if fault == "radius_r" else r2))[..., None], (dv * e)[..., None]]
    if H:
        vh = (dv * u * (-1.0 / (2.0 * r2)))[..., None] * 2.0 * diff
        out["g_feature"] = vh.sum(1)
        rowh = vh if fault == "hyper_sign" else -vh
        if fault == "swap_hyper":
            rowh = torch.cat([rowh[..., 1:2], rowh[..., 0:1], rowh[..., 2:]], -1)
        cols.append(rowh)
    rows = torch.cat(cols, -1).reshape(N * K, -1).to(F)
    flat = idx.reshape(-1).clone()
    perm = {"stored": torch.arange(N * K), "reversed": torch.arange(N * K - 1, -1, -1),
            "permuted": torch.randperm(N * K, generator=torch.Generator().manual_seed(5))}[order]
    big = int(torch.bincount(flat, minlength=M).argmax())
    if fault == "drop_last":  # the last row of the fullest node's segment
        rows = rows.clone()
        rows[torch.nonzero(flat == big)[-1]] = 0
    if fault == "offset":  # that node's rows credited to the next node
        flat[flat == big] = (big + 1) % M
    Sn = node_sum32(rows, flat, M, perm)
    out.update(g_trans=Sn[:, 0:3], g_rot=Sn[:, 3:7], g_scale=Sn[:, 7:10], g_radius=Sn[:, 19])
    if c["local"]:
        out["g_local_rot"] = torch.autograd.grad((Rm * Sn[:, 10:19].reshape(M, 3, 3)).sum(), lq)[0]
    if sg is not None:
        out["g_weight"] = Sn[:, 20] if fault == "no_sigmoid_deriv" else Sn[:, 20] * sg * (1.0 - sg)
    if H:
        out["g_nodes_hyper"] = Sn[:, 21:21 + H]
    return out


def failing(got, ref):
    return sorted(k for k, (r, b) in ref.items() if k in got and R.violations(got[k].reshape(r.shape), r, b)[0])


# ------------------------------------------------------------------------------------------- the two references agree
AGREE = [(K, (0, 1, 5, 9, 11)[K % 5], K % 8) for K in range(1, 9)] + [(3, h, f) for h, f in zip((0, 1, 5, 9, 11, 5, 9, 11), range(8))]


@pytest.mark.parametrize("K,hyper,f", AGREE)
def test_autograd_reference_agrees_with_the_oracle_on_given_lists(K, hyper, f):
    c = G.case(300, 24, K, hyper, f, mask=("rand" if f & 1 else "none"), seed=40 + K + 10 * f + hyper)
    t = G.build(c)
    idx = R.true_lists(t["x"], t["feature"], t["nodes"], hyper, K)
    if K < c["M"]:  # given lists, not the nearest: every fifth Gaussian's last neighbour becomes one outside its list
        other = R.true_lists(t["x"], t["feature"], t["nodes"], hyper, K + 1)[:, K]
        idx[::5, K - 1] = other[::5]
    ref = G.reference(c, t, idx)
    npy = lambda v: None if v is None else v.numpy()  # noqa: E731
    mask = np.ones((c["N"], 1), np.float32) if t["mask"] is None else t["mask"].numpy()[:, None]
    args = (t["x"].numpy(), None if hyper == 0 else t["feature"].numpy()[:, :hyper], mask, t["nodes"][:, :3 + hyper].numpy(),
            t["radius"].numpy(), None if t["weight"] is None else t["weight"].numpy()[:, None], {k: v.numpy() for k, v in t["attrs"].items()})
    cfg = dict(K=K, hyper_dim=hyper, local_frame=c["local"], d_rot_as_res=c["res"], nn_idx=idx.numpy())
    fw = O.forward(*args, **cfg)
    assert np.array_equal(fw["nn_idx"], idx.numpy())
    gout = {k: npy(t["cot"][kk]) for k, kk in (("d_xyz", "g_xyz"), ("d_rotation", "g_rot"), ("d_scaling", "g_scale"))}
    gout["d_nodes"] = np.zeros((c["M"], 3))
    bw = O.backward(*args, gout=gout, **cfg)
    pairs = [(k, fw[k]) for k in R.FWD_KEYS] + [("g_trans", bw["d_xyz"]), ("g_rot", bw["d_rotation"]), ("g_scale", bw["d_scaling"]),
                                                ("g_radius", bw["_node_radius"])]
    if c["local"]:
        pairs.append(("g_local_rot", bw["local_rotation"]))
    if c["nw"]:
        pairs.append(("g_weight", bw["_node_weight"][:, 0]))
    if hyper:
        pairs += [("g_nodes_hyper", bw["nodes"][:, 3:]), ("g_feature", bw["feature"])]
        assert np.abs(bw["nodes"][:, :3]).max() == 0
    if t["mask"] is not None:
        pairs.append(("g_mask", bw["motion_mask"][:, 0]))
    assert {k for k, _ in pairs} == set(ref)
    top = max(np.abs(o).max() for k, o in pairs if k not in R.FWD_KEYS)
    for k, o in pairs:  # (an array that is identically 0 in the oracle - the weight path at K = 1 - against the largest gradient)
        a = ref[k][0].numpy()
        assert np.abs(a - o.reshape(a.shape)).max() <= 1e-10 * (np.abs(o).max() if np.abs(o).max() > 0 else top), k


# ---------------------------------------------------------------------------------------------- acceptance, rejection
BASE = G.case(1500, 40, 3, 5, 5, local=True, res=False, nw=True, mask="rand", seed=77)
ACCEPT = [BASE, G.GRID[0], G.GRID[1], G.case(1025, 40, 8, 11, 3, seed=78), G.case(257, 5, 5, 2, 6, seed=79),
          G.case(600, 64, 2, 9, 0, mask="rand", cot="consistent", seed=80)]
_cache = {}


def prepared(c):
    key = G.case_id(c) + str(c["seed"])
    if key not in _cache:
        t = G.build(c)
        idx = R.true_lists(t["x"], t["feature"], t["nodes"], c["hyper"], c["K"])
        _cache[key] = (t, idx, G.reference(c, t, idx))
    return _cache[key]


@pytest.mark.parametrize("order", ["stored", "reversed", "permuted"])
@pytest.mark.parametrize("c", ACCEPT, ids=[G.case_id(c) for c in ACCEPT])
def test_fp32_restatement_is_within_every_bound(c, order):
    t, idx, ref = prepared(c)
    got = kernel32(c, t, idx, order)
    assert set(got) == set(ref)
    for k, (r, b) in ref.items():
        R.assert_within(k, got[k].reshape(r.shape), r, b)
    assert R.selection_violations(t["x"], t["feature"], t["nodes"], c["hyper"], idx, got["nn_dist"]) == 0


FAULTS = {"drop_last": "g_trans", "offset": "g_trans", "drop_wdw": "g_radius", "no_eps": "g_feature", "radius_r": "g_radius",
          "no_sigmoid_deriv": "g_weight", "no_mask_rows": "g_trans", "transpose_dR": "g_local_rot", "mask_bias": "g_mask",
          "swap_hyper": "g_nodes_hyper", "hyper_sign": "g_nodes_hyper"}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_fault_is_rejected(fault):
    t, idx, ref = prepared(BASE)
    bad = failing(kernel32(BASE, t, idx, "stored", fault), ref)
    assert FAULTS[fault] in bad, (fault, bad)


def test_a_replaced_far_neighbour_breaks_the_selection_rule():
    t, idx, _ = prepared(BASE)
    assert R.selection_violations(t["x"], t["feature"], t["nodes"], BASE["hyper"], idx) == 0
    row = 700
    nxt = int(idx[row, -1])
    while nxt in idx[row].tolist():
        nxt = (nxt + 1) % BASE["M"]
    wrong = idx.clone()
    wrong[row, -1] = nxt  # the smallest weight of one Gaussian: the next node instead
    assert R.selection_violations(t["x"], t["feature"], t["nodes"], BASE["hyper"], wrong) == 1


def test_selection_rule_rejects_swapped_twins_and_repeated_entries():
    c = G.case(513, 64, 3, 5, 1, ties=True, seed=81)
    t, idx, _ = prepared(c)
    assert R.selection_violations(t["x"], t["feature"], t["nodes"], 5, idx) == 0
    rows = torch.nonzero((idx[:, 0] == 0) & (idx[:, 1] == 1))[:, 0]
    assert len(rows) > 0
    sw = idx.clone()
    sw[rows[0], 0], sw[rows[0], 1] = 1, 0  # bit-identical nodes: the higher index first
    assert R.selection_violations(t["x"], t["feature"], t["nodes"], 5, sw) == 1
    rep = idx.clone()
    rep[5, 2] = rep[5, 0]
    assert R.selection_violations(t["x"], t["feature"], t["nodes"], 5, rep) == 1


# ------------------------------------------------------------- the gap that was open: test_against_oracle's hyper_dim = 11 case
def test_zeroed_small_gradients_pass_the_old_tolerance_and_fail_the_bounds():
    N, M, K, hyper = 1, 64, 3, 11  # tests/test_gpu_cnode.py::test_against_oracle's last case, by its own recipe
    g = torch.Generator().manual_seed(N + M)
    x = torch.randn(N, 3, generator=g) * 0.5
    nodes = torch.cat([x[torch.randint(0, N, (M,), generator=g)] + 0.05 * torch.randn(M, 3, generator=g),
                       1e-2 + 0.02 * torch.randn(M, hyper, generator=g)], -1)
    feature = 0.02 * torch.randn(N, hyper + 1, generator=g)
    mask = torch.rand(N, 1, generator=g)
    radius = np.log(0.15) + 0.3 * torch.randn(M, generator=g)
    attrs = {"d_xyz": 0.1 * torch.randn(M, 3, generator=g), "d_rotation": 0.2 * torch.randn(M, 4, generator=g),
             "d_scaling": 0.05 * torch.randn(M, 3, generator=g), "local_rotation": 0.3 * torch.randn(M, 4, generator=g)}
    cot = {k: torch.randn(N, w, generator=g) for k, w in (("g_xyz", 3), ("g_rot", 4), ("g_scale", 3))}
    c = dict(N=N, M=M, K=K, hyper=hyper, local=True, res=True)
    t = dict(x=x, feature=feature, mask=mask[:, 0], nodes=nodes, radius=radius, weight=None, attrs=attrs, cot=cot)
    idx = R.true_lists(x, feature, nodes, hyper, K)
    ref = G.reference(c, t, idx)
    good = kernel32(c, t, idx)
    assert failing(good, ref) == []
    old = lambda got, r: float((got.double() - r).abs().max()) <= 2e-4 * max(float(r.abs().max()), 1.0)  # noqa: E731
    # hyper columns 8..10 (accumulator columns 29..31): max |ref| 7.2e-4, 2.1e-4, 4.6e-4, so the old tolerance takes them a quarter
    # off (and column 9 nearly zeroed: 2.1e-4 against 2e-4), though not all three zeroed; the bounds reject both
    full = lambda hy: torch.cat([torch.zeros(M, 3, dtype=hy.dtype), hy], 1)  # noqa: E731  (dL/dnodes as the old test compares it)
    z, q = good["g_nodes_hyper"].clone(), good["g_nodes_hyper"].clone()
    z[:, 8:11] = 0
    q[:, 8:11] *= 0.75
    assert old(full(q), full(ref["g_nodes_hyper"][0])) and not old(full(z), full(ref["g_nodes_hyper"][0]))
    assert failing(dict(good, g_nodes_hyper=q), ref) == ["g_nodes_hyper"]
    assert failing(dict(good, g_nodes_hyper=z), ref) == ["g_nodes_hyper"]
    zl = torch.zeros_like(good["g_local_rot"])
    assert old(zl, ref["g_local_rot"][0])
    assert failing(dict(good, g_local_rot=zl), ref) == ["g_local_rot"]


# ------------------------------------------------------------------------------------------------------- non-vacuity
ALL = G.GRID + G.RANDOM + [G.SHIPPED]
WEIGHT_PATH = ("g_radius", "g_weight", "g_nodes_hyper", "g_feature")
SHARES = {}


def vacuity(c):
    """Per array: (elements counted, share of them with bound >= |ref|).  Not counted: elements whose bound is 0 (compared
    exactly), the weight-path gradients at K = 1 (zero by construction) and the deliberately degenerate rows."""
    t, idx, ref = prepared(c)
    out = {}
    for k, (r, b) in ref.items():
        if c["K"] == 1 and k in WEIGHT_PATH:
            continue
        counted = b > 0
        if k not in R.NODE_KEYS:
            counted = counted & ~t["degen"].reshape((-1,) + (1,) * (r.dim() - 1))
        n = int(counted.sum())
        out[k] = (n, float(((b >= r.abs()) & counted).sum()) / max(n, 1))
    _cache.pop(G.case_id(c) + str(c["seed"]), None)
    return out


@pytest.mark.parametrize("c", ALL, ids=["%d-%s" % (i, G.case_id(c)) for i, c in enumerate(ALL)])
def test_bounds_are_not_vacuous_on_the_gpu_grid(c):
    sh = vacuity(c)
    SHARES[G.case_id(c)] = sh
    print({k: "%d: %.4f" % v for k, v in sh.items()})
    for k, (n, share) in sh.items():
        assert share <= (NODE_CAP if k in R.NODE_KEYS else GAUSS_CAP), (k, n, share)
