"""tests/skin_ref.py on the host: the per-element bounds accept fp32 arithmetic of the same formulas summed in other orders, and
reject the faults the GPU tests (tests/test_gpu_wideskel_f64.py) are there to catch — each planted fault is its own case."""
import numpy as np
import pytest
import torch

from tests import skin_ref as R

F = torch.float32


def star(J):
    return torch.tensor([-1] + [0] * (J - 1))


def scene(N, J, seed, topo="tree"):
    g = torch.Generator().manual_seed(seed)
    if topo == "chain":
        parents = torch.arange(-1, J - 1)
        joints = torch.stack([torch.zeros(J), torch.linspace(-0.8, 0.8, J), torch.zeros(J)], -1) + 0.01 * torch.randn(J, 3, generator=g)
    elif topo == "star":
        parents = star(J)
        joints = 0.5 * torch.randn(J, 3, generator=g)
        joints[0] = 0
    else:
        parents = torch.full((J,), -1, dtype=torch.long)
        joints = torch.zeros(J, 3)
        for i in range(1, J):
            parents[i] = int(torch.randint(0, i, (1,), generator=g))
            joints[i] = joints[parents[i]] + 0.25 * torch.randn(3, generator=g)
    bone = torch.randint(1, J, (N,), generator=g)
    t = torch.rand(N, 1, generator=g) * 1.4 - 0.2
    x = joints[parents[bone]] + t * (joints[bone] - joints[parents[bone]]) + 0.05 * torch.randn(N, 3, generator=g)
    q = torch.tensor([1.0, 0, 0, 0]) + 0.1 * torch.randn(J, 4, generator=g)
    rho = torch.log(0.1 + 0.1 * torch.rand(J, generator=g))
    gt = 0.02 * torch.randn(3, generator=g)
    mask = torch.rand(N, 1, generator=g)
    return dict(x=x.contiguous(), joints=joints.contiguous(), parents=parents, q=q, rho=rho, gt=gt, mask=mask, g=g)


def chain32(q, joints, parents, alt=False):
    """The chain in fp32 (autograd-able); alt: the 3x4 products summed in the other order."""
    T, _ = R.local_T(q, joints, parents)
    vp = R._parents(parents)
    Ta = R._aug(T)
    G = [T[0]]
    for j in range(1, T.shape[0]):
        G.append((Ta[j].t() @ G[vp[j]].t()).t() if alt else G[vp[j]] @ Ta[j])
    G = torch.stack(G)
    posed = (G[:, :, :3] @ joints[..., None])[..., 0] + G[:, :, 3]
    return G, posed


def kernel_inputs(s):
    G, _ = R.chain(s["q"].double(), s["joints"].double(), s["parents"])
    from oracle.deform_ref import matrix_to_quaternion
    return G.reshape(-1, 12).float(), matrix_to_quaternion(G[:, :, :3]).float()


def skin32(s, tr, nr, wm=None, sel=None, rev=False, cot=None):
    """The skinning kernel's formulas in fp32 (bone_d2_fast form), bones summed in index order or in reverse (rev: and the
    Gaussians of the backward's sums reversed too).  Returns d_xyz, d_rotation (and the fp32 autograd gradients)."""
    x, joints, parents = s["x"], s["joints"], s["parents"]
    N, J = x.shape[0], joints.shape[0]
    B = J - 1
    par = parents.long()
    a = joints[par[1:]]
    ba = joints[1:] - a
    l2 = (ba * ba).sum(-1)
    rl2 = 1.0 / l2.clamp_min(1e-6)
    G = tr[1:].clone().requires_grad_(cot is not None)
    rho = s["rho"][1:].clone().requires_grad_(cot is not None)
    m = s["mask"].reshape(-1).clone().requires_grad_(cot is not None)
    w_ = None if wm is None else wm.clone().requires_grad_(cot is not None)
    e = x[:, None] - a[None]
    t = ((e * ba[None]).sum(-1) * rl2[None]).clamp(0, 1)
    sv = t[..., None] * ba[None] - e
    d2 = (sv * sv).sum(-1)
    rad = torch.exp(rho)
    inv2r2 = 1.0 / (2.0 * rad * rad)
    u = torch.exp(-d2 * inv2r2[None])
    if w_ is not None:
        u = u * w_
    v = u + 1e-7
    if sel is not None:
        selm = torch.zeros(N, B)
        selm.scatter_(1, sel, 1.0)
        v = v * selm
    if rev:
        S, M, Q = 0, 0, 0
        for k in range(B - 1, -1, -1):
            S = S + v[:, k]
            M = M + v[:, k, None] * G[k][None]
            Q = Q + v[:, k, None] * nr[1 + k][None]
    else:
        S, M, Q = v.sum(1), v @ G, v @ nr[1:]
    inv = 1.0 / S
    xt = torch.cat([x, torch.ones(N, 1)], 1)
    ax = (M.reshape(N, 3, 4) @ xt[..., None])[..., 0] * inv[:, None] + s["gt"][None]
    dxyz = (ax - x) * m[:, None]
    drot = Q * inv[:, None] * m[:, None]
    nw = (v / S[:, None]).detach()
    res = {"d_xyz": dxyz.detach(), "d_rotation": drot.detach(), "nn_weight": nw if sel is None else torch.gather(nw, 1, sel)}
    if cot is None:
        return res
    gx, gr = cot
    ins = [G, rho, m] + ([w_] if w_ is not None else [])
    if rev:  # the gradients' sums over the Gaussians in another order: per chunk of 97 Gaussians, chunks added last first
        gs = None
        for s0 in reversed(range(0, N, 97)):
            sl = slice(s0, s0 + 97)
            part = torch.autograd.grad((dxyz[sl] * gx[sl]).sum() + (drot[sl] * gr[sl]).sum(), ins, retain_graph=True)
            gs = list(part) if gs is None else [a + b for a, b in zip(gs, part)]
    else:
        gs = torch.autograd.grad((dxyz * gx).sum() + (drot * gr).sum(), ins)
    res["dL/dtransforms"] = torch.cat([torch.zeros(1, 12), gs[0]])
    res["dL/dnode_radius_log"] = torch.cat([torch.zeros(1), gs[1]])
    res["dL/dmotion_mask"] = gs[2]
    res["dL/dglobal_trans"] = (gx * m.detach()[:, None]).sum(0)
    if w_ is not None:
        res["dL/dweight_mod"] = gs[3]
    return res


def cotangents(N, g, kind):
    gx, gr = torch.randn(N, 3, generator=g), torch.randn(N, 4, generator=g)
    if kind == "consistent":
        gx, gr = 1 + 0.3 * gx, 1 + 0.3 * gr
    return gx, gr


def n_bad(got, ref_bnd):
    return R.violations(torch.as_tensor(got).double(), ref_bnd[0], ref_bnd[1])[0]


# --------------------------------------------------------------------------------------------------------------- accepts
@pytest.mark.parametrize("topo", ["chain", "tree", "star"])
def test_chain_bounds_accept_fp32_in_two_orders(topo):
    J = 130
    s = scene(10, J, 1, topo)
    g = s["g"]
    dG, gn = torch.randn(J, 12, generator=g), torch.randn(J, 3, generator=g)
    fw = R.chain_forward(s["q"], s["joints"], s["parents"], s["gt"])
    bw = R.chain_backward(s["q"], s["joints"], s["parents"], dG, gn)
    for alt in (False, True):
        q = s["q"].clone().requires_grad_(True)
        G, posed = chain32(q, s["joints"], s["parents"], alt)
        assert n_bad(G.detach().reshape(J, 12), fw["transforms"]) == 0
        assert n_bad((posed + s["gt"]).detach(), fw["d_nodes"]) == 0
        ((G.reshape(J, 12) * dG).sum() + (posed * gn).sum()).backward()
        assert n_bad(q.grad, bw["dL/dlocal_rot"]) == 0
    assert n_bad(gn.sum(0), bw["dL/dglobal_trans"]) == 0
    tr, _ = kernel_inputs(s)
    ref, bnd = R.node_rot(tr)
    from oracle.deform_ref import matrix_to_quaternion
    assert n_bad(matrix_to_quaternion(tr.reshape(J, 3, 4)[:, :, :3]), (ref, bnd)) == 0


@pytest.mark.parametrize("wm,K", [(False, -1), (True, -1), (False, 3)])
@pytest.mark.parametrize("kind", ["random", "consistent"])
def test_skin_bounds_accept_fp32_in_two_orders(wm, K, kind):
    N, J = 3001, 70
    s = scene(N, J, 2)
    tr, nr = kernel_inputs(s)
    g = s["g"]
    w = torch.sigmoid(torch.randn(N, J - 1, generator=g)) if wm else None
    sel = torch.from_numpy(R.topk_select(s["x"].numpy(), s["joints"].numpy(), s["parents"].numpy(), K)) if K > 0 else None
    cot = cotangents(N, g, kind)
    L = R.depth_topk(N) if K > 0 else R.depth_bonelane(N, J)
    ref = R.skin(s["x"], s["joints"], s["parents"], s["rho"], tr, nr, s["gt"], s["mask"], w, sel, cot, L, chunk=1000)
    for rev in (False, True):
        got = skin32(s, tr, nr, w, sel, rev, cot)
        for k in ref:
            assert n_bad(got[k], ref[k]) == 0, (k, rev, R.violations(got[k].double(), *ref[k]))


def test_selection_is_the_stable_float32_order():
    s = scene(2000, 70, 3, "star")  # every bone shares the root: ties everywhere at the root
    x = s["x"].clone()
    x[:50] = s["joints"][0]         # Gaussians exactly on the shared joint: all d2 equal
    d2 = R.bone_d2_f32(x.numpy(), s["joints"].numpy(), s["parents"].numpy())
    sel = R.topk_select(x.numpy(), s["joints"].numpy(), s["parents"].numpy(), 5)
    assert (sel[:50] == np.arange(5)).all()
    ds = np.take_along_axis(d2, sel, 1)
    assert (np.diff(ds, axis=1) >= 0).all()


# --------------------------------------------------------------------------------------------------------- planted faults
@pytest.fixture(scope="module")
def wide():
    N, J = 3001, 130
    s = scene(N, J, 4)
    tr, nr = kernel_inputs(s)
    g = s["g"]
    cot = cotangents(N, g, "random")
    dG, gn = torch.randn(J, 12, generator=g), torch.randn(J, 3, generator=g)
    ref = R.skin(s["x"], s["joints"], s["parents"], s["rho"], tr, nr, s["gt"], s["mask"], None, None, cot, R.depth_bonelane(N, J))
    got = skin32(s, tr, nr, None, None, False, cot)
    bw = R.chain_backward(s["q"], s["joints"], s["parents"], dG, gn)
    q = s["q"].clone().requires_grad_(True)
    G, posed = chain32(q, s["joints"], s["parents"])
    ((G.reshape(J, 12) * dG).sum() + (posed * gn).sum()).backward()
    return dict(s=s, tr=tr, nr=nr, ref=ref, got=got, bw=bw, dq=q.grad.detach(), cot=cot)


def _plant_rel(got, rb, rel=1e-4):
    """Move one element by ``rel`` of its own magnitude, at an element whose bound is below that."""
    ref, bnd = rb
    ok = (bnd < 0.5 * rel * ref.abs()) & (ref.abs() > 0)
    assert ok.any(), "no element with a bound below %g of itself" % rel
    i = int(torch.nonzero(ok.reshape(-1))[0])
    bad = got.clone().double().reshape(-1)
    bad[i] = ref.reshape(-1)[i] * (1 + rel)
    return bad.reshape(got.shape)


def test_rejects_d_xyz_off_by_1e4(wide):
    assert n_bad(wide["got"]["d_xyz"], wide["ref"]["d_xyz"]) == 0
    assert n_bad(_plant_rel(wide["got"]["d_xyz"], wide["ref"]["d_xyz"]), wide["ref"]["d_xyz"]) == 1


def test_rejects_dlocal_rot_off_by_1e4(wide):
    assert n_bad(wide["dq"], wide["bw"]["dL/dlocal_rot"]) == 0
    assert n_bad(_plant_rel(wide["dq"], wide["bw"]["dL/dlocal_rot"]), wide["bw"]["dL/dlocal_rot"]) == 1


@pytest.mark.parametrize("what", ["transforms", "d_nodes"])
def test_rejects_chain_forward_off_by_1e4(wide, what):
    s = wide["s"]
    J = s["joints"].shape[0]
    fw = R.chain_forward(s["q"], s["joints"], s["parents"], s["gt"])
    G, posed = chain32(s["q"], s["joints"], s["parents"])
    got = G.reshape(J, 12) if what == "transforms" else posed + s["gt"]
    assert n_bad(got, fw[what]) == 0
    assert n_bad(_plant_rel(got, fw[what]), fw[what]) == 1


def test_rejects_dglobal_trans_off_by_1e4():
    # (consistent-sign cotangents: under random signs sum_n g_n cancels to ~1/sqrt(N) of sum_n |g_n|, and the depth-L bound is
    # then 2e-4 of the value at N = 3001)
    N, J = 3001, 70
    s = scene(N, J, 9)
    tr, nr = kernel_inputs(s)
    cot = cotangents(N, s["g"], "consistent")
    ref = R.skin(s["x"], s["joints"], s["parents"], s["rho"], tr, nr, s["gt"], s["mask"], None, None, cot, R.depth_bonelane(N, J))
    got = skin32(s, tr, nr, None, None, False, cot)
    k = "dL/dglobal_trans"
    assert n_bad(got[k], ref[k]) == 0
    assert n_bad(_plant_rel(got[k], ref[k]), ref[k]) == 1


def test_rejects_dtransforms_off_by_1e4(wide):
    k = "dL/dtransforms"
    assert n_bad(wide["got"][k], wide["ref"][k]) == 0
    assert n_bad(_plant_rel(wide["got"][k], wide["ref"][k]), wide["ref"][k]) == 1


@pytest.mark.parametrize("kind", ["random", "consistent"])
def test_rejects_a_dropped_bone_pass(kind):
    N, J = 65_537, 130  # (the GPU grid's N; bones 64..127 are the second pass of 64)
    s = scene(N, J, 5)
    tr, nr = kernel_inputs(s)
    cot = cotangents(N, s["g"], kind)
    ref = R.skin(s["x"], s["joints"], s["parents"], s["rho"], tr, nr, s["gt"], s["mask"], None, None, cot, R.depth_bonelane(N, J))
    for k in ("dL/dtransforms", "dL/dnode_radius_log"):
        bad = ref[k][0].clone()
        bad[1 + 64:1 + 128] = 0
        nb = n_bad(bad, ref[k])
        assert nb >= 0.9 * bad[1 + 64:1 + 128].numel(), (k, nb)


def test_rejects_a_single_small_bone_zeroed():
    N, J = 3001, 130
    s = scene(N, J, 4)
    s["rho"][40:50] = torch.linspace(np.log(0.01), np.log(0.05), 10)  # narrow bones: gradients ~1e-3 of the largest
    tr, nr = kernel_inputs(s)
    cot = cotangents(N, s["g"], "consistent")
    ref = R.skin(s["x"], s["joints"], s["parents"], s["rho"], tr, nr, s["gt"], s["mask"], None, None, cot, R.depth_bonelane(N, J))
    got = skin32(s, tr, nr, None, None, False, cot)
    for k in ("dL/dtransforms", "dL/dnode_radius_log"):
        ref_, bnd = ref[k]
        assert n_bad(got[k], ref[k]) == 0, k
        per = ref_.reshape(J, -1).abs().amax(1)
        ratio = per / per.max()
        b = 1 + int(torch.argmin((ratio[1:].log10() + 3).abs()))
        assert 3e-4 < float(ratio[b]) < 3e-3, float(ratio[b])
        bad = got[k].clone()
        bad[b] = 0
        assert n_bad(bad, ref[k]) >= 1, k


@pytest.mark.parametrize("a,b", [(63, 64), (31, 32)])
def test_rejects_swapped_bones(wide, a, b):
    for k in ("dL/dtransforms", "dL/dnode_radius_log"):
        bad = wide["got"][k].clone()
        bad[[1 + a, 1 + b]] = bad[[1 + b, 1 + a]]
        assert n_bad(bad, wide["ref"][k]) >= 1, k
    bad = wide["got"]["nn_weight"].clone()
    bad[:, [a, b]] = bad[:, [b, a]]
    assert n_bad(bad, wide["ref"]["nn_weight"]) >= 1


def test_rejects_weight_mod_read_with_stride_b_plus_1():
    N, J = 2000, 70
    s = scene(N, J, 6)
    tr, nr = kernel_inputs(s)
    B = J - 1
    flat = torch.sigmoid(torch.randn(N * (B + 1), generator=s["g"]))
    wm = flat[:N * B].reshape(N, B)
    ref = R.skin(s["x"], s["joints"], s["parents"], s["rho"], tr, nr, s["gt"], s["mask"], wm)
    assert n_bad(skin32(s, tr, nr, wm)["d_xyz"], ref["d_xyz"]) == 0
    wrong = flat.reshape(N, B + 1)[:, :B]
    assert n_bad(skin32(s, tr, nr, wrong)["d_xyz"], ref["d_xyz"]) > 0


def test_rejects_the_last_ragged_row_zeroed(wide):
    for k in ("d_xyz", "d_rotation", "nn_weight"):
        bad = wide["got"][k].clone()
        bad[-1] = 0
        assert n_bad(bad, wide["ref"][k]) >= 1, k


def test_rejects_a_topk_selection_with_the_kth_and_next_swapped():
    s = scene(500, 70, 7)
    K = 3
    x, jn, pn = s["x"].numpy(), s["joints"].numpy(), s["parents"].numpy()
    sel = R.topk_select(x, jn, pn, K)
    nxt = np.argsort(R.bone_d2_f32(x, jn, pn), axis=1, kind="stable")[:, K]
    d2 = R.bone_d2_f32(x, jn, pn)
    rows = np.arange(x.shape[0])
    gap = (d2[rows, nxt] - d2[rows, sel[:, K - 1]]) / d2[rows, nxt]
    r = int(np.argmax(gap))  # a row whose K-th and (K+1)-th distances are far apart
    assert gap[r] > 0.1
    bad = sel.copy()
    bad[r, K - 1] = nxt[r]
    assert np.array_equal(sel, R.topk_select(x, jn, pn, K))
    assert not np.array_equal(bad, R.topk_select(x, jn, pn, K))
    assert R.selection_violations(x, jn, pn, sel) == 0
    assert R.selection_violations(x, jn, pn, bad) == 1
    # and the blend over the wrong bones leaves the bound on its row
    tr, nr = kernel_inputs(s)
    ref = R.skin(s["x"], s["joints"], s["parents"], s["rho"], tr, nr, s["gt"], s["mask"], None, torch.from_numpy(sel))
    got = skin32(s, tr, nr, None, torch.from_numpy(bad))
    assert R.violations(got["d_xyz"][r:r + 1].double(), ref["d_xyz"][0][r:r + 1], ref["d_xyz"][1][r:r + 1])[0] >= 1


def test_rejects_a_reverse_sweep_that_drops_a_child_of_the_root():
    J = 256
    s = scene(1, J, 8, "star")  # 255 children of the root, one mask of 256 bits
    g = s["g"]
    dG, gn = torch.randn(J, 12, generator=g), torch.randn(J, 3, generator=g)
    bw = R.chain_backward(s["q"], s["joints"], s["parents"], dG, gn)
    ref, bnd = bw["dL/dlocal_rot"]
    for c in (1, 31, 32, 200, 255):
        only = torch.zeros_like(dG), torch.zeros_like(gn)
        only[0][c], only[1][c] = dG[c], gn[c]
        part = R.chain_backward(s["q"], s["joints"], s["parents"], only[0], only[1])["dL/dlocal_rot"][0]
        bad = ref.clone()
        bad[0] -= part[0]
        assert R.violations(bad, ref, bnd)[0] >= 1, c
