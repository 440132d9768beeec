"""-m gpu: the deformation kernels of 63..256-joint skeletons pinned per element to float64 (tests/skin_ref.py), through the C ABI
so that every output and workspace is under the test's control.  Each kernel is checked from the fp32 inputs it read (the
skinning from the chain kernel's own transforms), across the dispatch boundaries the 65-256-joint kernels introduced: 64 / 65 joints,
bone passes of 64 and mask words of 32 bones, the bone-lane backward's 1024-Gaussian workgroups, K from 1 to J - 1.  Every
output is a view into a larger buffer whose sentinel tail must survive bit for bit, and every per-Gaussian input carries a NaN
tail past row N, so that a read past N poisons a result."""
import numpy as np
import pytest
import torch

from riggs_amd import _lib as L
from tests import gpu_util as GU
from tests import skin_ref as R

pytestmark = pytest.mark.gpu

from tests.gpu_util import SENT, TAIL, in_buf, out_buf, tail_intact  # noqa: F401


def skeleton(J, topo, g):
    if topo == "chain":
        parents = torch.arange(-1, J - 1)
        joints = torch.stack([torch.zeros(J), torch.linspace(-0.8, 0.8, J), torch.zeros(J)], -1) + 0.01 * torch.randn(J, 3, generator=g)
    elif topo == "star":  # every joint's parent is the root: 255 children in one mask, every bone shares a joint
        parents = torch.tensor([-1] + [0] * (J - 1))
        joints = 0.5 * torch.randn(J, 3, generator=g)
        joints[0] = 0
    elif topo == "broom":  # a long chain that fans out
        h = J // 2
        parents = torch.tensor([-1] + list(range(0, h - 1)) + [h - 1] * (J - h))
        joints = torch.zeros(J, 3)
        joints[:h, 1] = torch.linspace(-0.8, 0.2, h)
        joints[h:] = joints[h - 1] + 0.3 * torch.randn(J - h, 3, generator=g)
    else:  # random tree; "zerobone": one bone of zero length (the len2c clamp)
        parents = torch.full((J,), -1, dtype=torch.long)
        joints = torch.zeros(J, 3)
        for i in range(1, J):
            parents[i] = int(torch.randint(0, i, (1,), generator=g))
            joints[i] = joints[parents[i]] + 0.25 * torch.randn(3, generator=g)
        if topo == "zerobone":
            joints[J // 2] = joints[parents[J // 2]]
    q = torch.tensor([1.0, 0, 0, 0]) + 0.1 * torch.randn(J, 4, generator=g)
    q[:: 7] *= 0.6  # un-normalised local rotations
    rho = torch.log(0.06 + 0.1 * torch.rand(J, generator=g))
    return joints.contiguous(), parents, q.contiguous(), rho, 0.02 * torch.randn(3, generator=g)


def gaussians(N, joints, parents, rho, g):
    J = joints.shape[0]
    bone = torch.randint(1, J, (N,), generator=g)
    t = torch.rand(N, 1, generator=g) * 1.6 - 0.3  # past both ends of the bone too
    a, b = joints[parents[bone]], joints[bone]
    x = a + t * (b - a) + 0.05 * torch.randn(N, 3, generator=g)
    if N >= 8:
        k = max(1, N // 20)
        x[:k] = joints[torch.randint(0, J, (k,), generator=g)]  # exactly on a joint: d2 = 0
        x[k:2 * k] = 1000.0 + torch.rand(k, 3, generator=g)    # every u underflows: uniform 1e-7 weights
        # u ~ 1e-7: d2 inv2r2 ~ 16.1 from the child joint of a bone, off its axis
        bj = torch.randint(1, J, (k,), generator=g)
        r = torch.exp(rho[bj])[:, None] * (2 * 16.1) ** 0.5
        d = torch.nn.functional.normalize(torch.randn(k, 3, generator=g), dim=1)
        x[2 * k:3 * k] = joints[bj] + r * d
    return x.contiguous()


def cotangent(N, kind, g):
    gx, gr = torch.randn(N, 3, generator=g), torch.randn(N, 4, generator=g)
    if kind == "consistent":
        gx, gr = 1 + 0.3 * gx, 1 + 0.3 * gr
    elif kind == "sparse":
        keep = (torch.rand(N, 1, generator=g) < 0.05).float()
        gx, gr = gx * keep, gr * keep
    elif kind == "zero":
        gx, gr = gx * 0, gr * 0
    elif kind == "last":
        gx[:-1], gr[:-1] = 0, 0
    return gx.contiguous(), gr.contiguous()


def motion(N, kind, g):
    if kind == "none":
        return None
    if kind == "ones":
        return torch.ones(N, 1)
    m = torch.rand(N, 1, generator=g)
    if kind == "zeros":
        m = m * (torch.rand(N, 1, generator=g) > 0.3).float()
    return m


def check(what, got, rb, stats=GU.STATS):
    ref, bnd = rb
    R.assert_within(what, got.double().reshape(ref.shape), ref, bnd, stats=stats)


def run_chain(J, q, joints, parents, gt):
    p32 = parents.to(torch.int32).cuda()
    qc, jc, gtc = q.cuda(), joints.cuda(), gt.cuda()
    tr, trb = out_buf((J, 12))
    nr, nrb = out_buf((J, 4))
    dn, dnb = out_buf((J, 3))
    L.check(L.lib().riggs_fk_forward(J, qc.data_ptr(), jc.data_ptr(), p32.data_ptr(), gtc.data_ptr(), tr.data_ptr(), nr.data_ptr(),
                                     dn.data_ptr(), L.stream_ptr()), "riggs_fk_forward")
    torch.cuda.synchronize()
    assert tail_intact(trb, J) and tail_intact(nrb, J) and tail_intact(dnb, J)
    return tr, nr, dn


def check_chain_outputs(tag, q, joints, parents, gt, tr, nr, dn):
    fw = R.chain_forward(q, joints, parents, gt)
    check("transforms " + tag, tr.cpu(), fw["transforms"])
    check("d_nodes " + tag, dn.cpu(), fw["d_nodes"])
    check("node_rot " + tag, nr.cpu(), R.node_rot(tr.cpu()))


CHAIN = [(J, topo) for J in (63, 64, 65, 66, 72, 96, 128, 129, 160, 192, 193, 255, 256)
         for topo in ("chain", "tree", "star", "broom", "zerobone")]


@pytest.mark.parametrize("J,topo", CHAIN)
def test_chain_against_float64(J, topo):
    g = torch.Generator().manual_seed(J * 10 + len(topo))
    joints, parents, q, rho, gt = skeleton(J, topo, g)
    tag = "J=%d %s" % (J, topo)
    tr, nr, dn = run_chain(J, q, joints, parents, gt)
    check_chain_outputs(tag, q, joints, parents, gt, tr, nr, dn)
    dG, gn = torch.randn(J, 12, generator=g), torch.randn(J, 3, generator=g)
    p32 = parents.to(torch.int32).cuda()
    qc, jc, dGc, gnc = q.cuda(), joints.cuda(), dG.cuda(), gn.cuda()
    dq, dqb = out_buf((J, 4))
    dgt, dgtb = out_buf((3,))
    dgt.zero_()  # (accumulated into: zeros in front of the sentinel tail)
    L.check(L.lib().riggs_fk_backward(J, qc.data_ptr(), jc.data_ptr(), p32.data_ptr(), dGc.data_ptr(), gnc.data_ptr(), dq.data_ptr(),
                                      dgt.data_ptr(), L.stream_ptr()), "riggs_fk_backward")
    torch.cuda.synchronize()
    assert tail_intact(dqb, J) and tail_intact(dgtb, 3)
    bw = R.chain_backward(q, joints, parents, dG, gn)
    check("dL/dlocal_rot " + tag, dq.cpu(), bw["dL/dlocal_rot"])
    check("dL/dglobal_trans " + tag, dgt.cpu(), bw["dL/dglobal_trans"])


def run_skin(c):
    """One skinning case through riggs_lbs_forward(_fk) and riggs_lbs_backward, every output per element against float64."""
    J, N, K, topo = c["J"], c["N"], c["K"], c["topo"]
    g = torch.Generator().manual_seed(c["seed"])
    joints, parents, q, rho, gt = skeleton(J, topo, g)
    x = gaussians(N, joints, parents, rho, g)
    mask = motion(N, c["mask"], g)
    wm = None
    if c["wm"]:
        wm = torch.sigmoid(2 * torch.randn(N, J - 1, generator=g))
        if N:
            wm.view(-1)[:: 13] = 0.0
            wm.view(-1)[5:: 17] = 1.0
    gx, gr = cotangent(N, c["cot"], g)
    tag = str(c)
    B = J - 1
    p32 = parents.to(torch.int32).cuda()
    jc, rc, gtc, qc = joints.cuda(), rho.cuda(), gt.cuda(), q.cuda()
    xc, _ = in_buf(x)
    mc = None if mask is None else in_buf(mask)[0]
    wc = None if wm is None else in_buf(wm)[0]
    dx, dxb = out_buf((N, 3))
    dr, drb = out_buf((N, 4))
    lib = L.lib()
    if c["fk"]:
        tr, trb = out_buf((J, 12))
        nr, nrb = out_buf((J, 4))
        dn, dnb = out_buf((J, 3))
        L.check(lib.riggs_lbs_forward_fk(N, J, K, xc.data_ptr(), jc.data_ptr(), p32.data_ptr(), rc.data_ptr(), qc.data_ptr(),
                                         gtc.data_ptr(), L.ptr(mc), L.ptr(wc), tr.data_ptr(), nr.data_ptr(), dn.data_ptr(),
                                         dx.data_ptr(), dr.data_ptr(), None, L.stream_ptr()), "riggs_lbs_forward_fk")
        torch.cuda.synchronize()
        assert tail_intact(trb, J) and tail_intact(nrb, J) and tail_intact(dnb, J)
        if J > 64:  # the same wide chain kernel as riggs_fk_forward: bit for bit
            tr2, nr2, dn2 = run_chain(J, q, joints, parents, gt)
            assert torch.equal(tr, tr2) and torch.equal(nr, nr2) and torch.equal(dn, dn2), tag
        else:  # the chain ran inside the skinning workgroup
            check_chain_outputs(tag, q, joints, parents, gt, tr, nr, dn)
        nw = nidx = None
    else:
        tr, nr, dn = run_chain(J, q, joints, parents, gt)
        Kp = B if K <= 0 else K
        nw, nwb = out_buf((N, Kp))
        nidx, nib = out_buf((N, Kp), torch.int64, -77)
        L.check(lib.riggs_lbs_forward(N, J, K, xc.data_ptr(), jc.data_ptr(), p32.data_ptr(), rc.data_ptr(), tr.data_ptr(), nr.data_ptr(),
                                      gtc.data_ptr(), L.ptr(mc), L.ptr(wc), dx.data_ptr(), dr.data_ptr(), nw.data_ptr(), nidx.data_ptr(),
                                      None, L.stream_ptr()), "riggs_lbs_forward")
        torch.cuda.synchronize()
        assert tail_intact(nwb, N) and tail_intact(nib, N, -77)
    assert tail_intact(dxb, N) and tail_intact(drb, N)
    sel = None
    if K > 0:
        if nidx is None:  # (riggs_lbs_forward_fk has no nn outputs: the same selection code through riggs_lbs_forward, own outputs)
            nw_, _ = out_buf((N, K))
            nidx, nib = out_buf((N, K), torch.int64, -77)
            dx2, dr2 = torch.empty(N, 3, device="cuda"), torch.empty(N, 4, device="cuda")
            L.check(lib.riggs_lbs_forward(N, J, K, xc.data_ptr(), jc.data_ptr(), p32.data_ptr(), rc.data_ptr(), tr.data_ptr(),
                                          nr.data_ptr(), gtc.data_ptr(), L.ptr(mc), None, dx2.data_ptr(), dr2.data_ptr(), nw_.data_ptr(),
                                          nidx.data_ptr(), None, L.stream_ptr()), "riggs_lbs_forward")
            torch.cuda.synchronize()
            assert tail_intact(nib, N, -77)
            if J > 64:  # the _fk form launches the same 256-joint lbs_forward_kernel after its chain: bit for bit
                assert torch.equal(dx, dx2) and torch.equal(dr, dr2), "riggs_lbs_forward_fk != riggs_lbs_forward " + tag
        sel = nidx.cpu() - 1
        # The kernel's bone_d2 is contracted into FMAs (see tests/skin_ref.py), so the numpy float32 restatement does not pick
        # the same bones on every row: the count is reported, and the float64 (d2, bound) rule is asserted.
        emu = torch.from_numpy(R.topk_select(x.numpy(), joints.numpy(), parents.numpy(), K))
        differ = int((emu != sel).any(1).sum())
        print("top-K rows differing from the non-contracted fp32 restatement: %d of %d %s" % (differ, N, tag))
        nbad = R.selection_violations(x, joints, parents, sel)
        assert nbad == 0, "%d rows of the top-K selection break the float64 (d2, bound) order %s" % (nbad, tag)
    # backward
    gxc, _ = in_buf(gx)
    grc, _ = in_buf(gr)
    dG, dGb = out_buf((J, 12), fill=float("nan"))
    drho, drhob = out_buf((J,), fill=float("nan"))
    dgt, dgtb = out_buf((3,), fill=float("nan"))
    dm, dmb = out_buf((N,), fill=float("nan"))
    dw, dwb = (None, None) if wm is None else out_buf((N, B), fill=float("nan"))
    ws = torch.empty(int(lib.riggs_lbs_backward_workspace_bytes(N, J)), dtype=torch.uint8, device="cuda")
    L.check(lib.riggs_lbs_backward(N, J, K, xc.data_ptr(), jc.data_ptr(), p32.data_ptr(), rc.data_ptr(), tr.data_ptr(), nr.data_ptr(),
                                   gtc.data_ptr(), L.ptr(mc), L.ptr(wc), gxc.data_ptr(), grc.data_ptr(), dG.data_ptr(), drho.data_ptr(),
                                   dgt.data_ptr(), dm.data_ptr(), L.ptr(dw), ws.data_ptr(), L.stream_ptr()), "riggs_lbs_backward")
    torch.cuda.synchronize()
    for buf, rows in ((dGb, J), (drhob, J), (dgtb, 3), (dmb, N)) + (((dwb, N),) if dw is not None else ()):
        assert torch.isnan(buf[rows:]).all(), "write past the end " + tag
    # (the <= 64-joint bone-lane backward gives a workgroup 4096 / 8192 Gaussians from 4 / 8 x 240 x 1024 on: deform.hip)
    gpb = 1024 if J > 64 or N < 4 * 240 * 1024 else (4096 if N < 8 * 240 * 1024 else 8192)
    depth = R.depth_topk(N) if K > 0 else R.depth_bonelane(N, J, gpb)
    dev = "cuda"
    ref = R.skin(x.to(dev), joints.to(dev), parents.to(dev), rho.to(dev), tr, nr, gt.to(dev),
                 None if mask is None else mask.to(dev), None if wm is None else wm.to(dev),
                 None if sel is None else sel.to(dev), (gx.to(dev), gr.to(dev)), depth)
    check("d_xyz " + tag, dx, ref["d_xyz"])
    check("d_rotation " + tag, dr, ref["d_rotation"])
    if nw is not None:
        check("nn_weight " + tag, nw, ref["nn_weight"])
    for k, got in (("dL/dtransforms", dG), ("dL/dnode_radius_log", drho), ("dL/dglobal_trans", dgt), ("dL/dmotion_mask", dm)):
        check(k + " " + tag, got, ref[k])
    if dw is not None:
        check("dL/dweight_mod " + tag, dw, ref["dL/dweight_mod"])


def _grid():
    Js = [63, 64, 65, 66, 72, 96, 128, 129, 160, 192, 193, 255, 256]
    topos = ["chain", "tree", "star", "broom", "zerobone"]
    Ks = [-1, 1, 3, 8, 32, 33, 0]  # 0: J - 1
    Ns = [0, 1, 255, 256, 257, 1023, 1024, 1025, 4097, 65537]
    masks = ["none", "ones", "rand", "zeros"]
    cots = ["random", "consistent", "sparse", "zero", "last"]
    cases = []
    i = 0
    for J in Js:
        for rep in range(3):
            K = Ks[i % 7]
            K = J - 1 if K == 0 else K
            cases.append(dict(J=J, N=Ns[(3 * i + rep) % 10], K=K, topo=topos[i % 5], mask=masks[i % 4], cot=cots[(i + rep) % 5],
                              wm=(K < 0 and rep == 2), fk=(rep == 1), seed=100 + i))
            i += 1
    # the bone-lane backward (K = -1) on its pass and block edges, with dense cotangents: B = 64 (one full pass), 65 (a pass
    # holding one real bone), 73 (a block of 8 holding one), 128 / 129, 192 / 193; N on both sides of its 1024-Gaussian workgroup
    lane = [(65, 1024), (66, 1025), (74, 1023), (129, 4097), (130, 1025), (193, 2049), (194, 1024)]
    for j, (J, N) in enumerate(lane):
        for cot in ("random", "consistent"):
            cases.append(dict(J=J, N=N, K=-1, topo=topos[j % 5], mask=masks[j % 4], cot=cot, wm=(cot == "consistent" and j % 2 == 0),
                              fk=(cot == "random"), seed=700 + 2 * j + (cot == "random")))
    # the bone-lane backward and the top-K backward at 300 000 Gaussians, two cases each
    cases += [dict(J=200, N=300_000, K=-1, topo="tree", mask="rand", cot="random", wm=False, fk=False, seed=1),
              dict(J=256, N=300_000, K=-1, topo="broom", mask="zeros", cot="consistent", wm=True, fk=True, seed=2),
              dict(J=129, N=300_000, K=3, topo="tree", mask="ones", cot="consistent", wm=False, fk=False, seed=3),
              dict(J=193, N=300_000, K=33, topo="star", mask="none", cot="random", wm=False, fk=True, seed=4)]
    # the top-K forward's nn_weight / nn_idx (ascending d2) on both sides of 64 joints — the register mask and the LDS column
    # of the one selection code — at K = 3 and K = J - 1
    for j, (J, K) in enumerate([(64, 3), (64, 63), (65, 3), (65, 64)]):
        cases.append(dict(J=J, N=257, K=K, topo=topos[j % 5], mask=masks[j % 4], cot="random", wm=False, fk=False, seed=800 + j))
    # the <= 64-joint bone-lane backward's large-scene workgroups (4096 and 8192 Gaussians: N >= 4 x 240 x 1024 and
    # N >= 8 x 240 x 1024) with one block of bones, a sparse cotangent, with and without weight_mod
    for j, N in enumerate([4 * 240 * 1024 + 1, 8 * 240 * 1024 + 1]):
        for wm in (False, True):
            cases.append(dict(J=9, N=N, K=-1, topo="tree", mask="rand", cot="sparse", wm=wm, fk=False, seed=900 + 2 * j + wm))
    # ... and its 2 to 7 blocks of bones (J - 1 = 9, 17, 25, 33, 41, 49), each with weight_mod (41 bones and fewer: the
    # forward stages weight_mod through its LDS tile) and without it (then with the chain inside the forward)
    for j, J in enumerate([10, 18, 26, 34, 42, 50]):
        for wm in (j % 2 == 0, j % 2 == 1):
            cases.append(dict(J=J, N=1025, K=-1, topo=topos[j % 5], mask=masks[j % 4], cot=cots[j % 5], wm=wm, fk=not wm,
                              seed=950 + j + (0 if wm == (j % 2 == 0) else 10)))
    return cases


GRID = _grid()


@pytest.mark.parametrize("c", GRID, ids=["J%d-N%d-K%d-%s-%s-%s%s%s" % (c["J"], c["N"], c["K"], c["topo"], c["mask"], c["cot"],
                                                                        "-wm" if c["wm"] else "", "-fk" if c["fk"] else "") for c in GRID])
def test_skinning_against_float64(c):
    run_skin(c)


@pytest.mark.parametrize("seed", range(16))
def test_random_wide_skinning_against_float64(seed):
    r = np.random.RandomState(4200 + seed)
    J = int(r.randint(65, 257))
    K = int(r.choice([-1, -1, 1, 3, 8, 32, 33, J - 1]))
    c = dict(J=J, N=int(r.choice([1, 255, 257, 1023, 1025, 4097, 20011])), K=K,
             topo=str(r.choice(["chain", "tree", "star", "broom", "zerobone"])), mask=str(r.choice(["none", "ones", "rand", "zeros"])),
             cot=str(r.choice(["random", "consistent", "sparse", "zero", "last"])), wm=bool(K < 0 and r.randint(2)), fk=bool(r.randint(2)),
             seed=5000 + seed)
    run_skin(c)


@pytest.mark.parametrize("J", [64, 65, 200])
def test_weight_mod_with_topk_is_refused(J):
    N = 10
    g = torch.Generator().manual_seed(J)
    joints, parents, q, rho, gt = skeleton(J, "tree", g)
    x = gaussians(N, joints, parents, rho, g).cuda()
    wm = torch.rand(N, J - 1, device="cuda")
    p32 = parents.to(torch.int32).cuda()
    jc, rc, gtc = joints.cuda(), rho.cuda(), gt.cuda()
    tr, nr, _ = run_chain(J, q, joints, parents, gt)
    dx, dr = torch.empty(N, 3, device="cuda"), torch.empty(N, 4, device="cuda")
    rc_ = L.lib().riggs_lbs_forward(N, J, 3, x.data_ptr(), jc.data_ptr(), p32.data_ptr(), rc.data_ptr(), tr.data_ptr(), nr.data_ptr(),
                                    gtc.data_ptr(), None, wm.data_ptr(), dx.data_ptr(), dr.data_ptr(), None, None, None, L.stream_ptr())
    assert rc_ != 0
