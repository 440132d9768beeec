"""-m gpu: the control-node blend (csrc/cnode.hip) pinned per element to float64 (tests/cnode_f64_ref.py), through the C ABI so
that every output and the workspace are under the test's control.  The reference runs on the forward kernel's OWN neighbour
lists, which are checked first by the float64 selection rule, so every gradient is compared in every case.  Every output is a
view in front of a sentinel tail that must survive bit for bit, every per-Gaussian input carries a NaN tail past row N, the
spare node columns hold NaN, and the workspace is exactly riggs_cnode_backward_workspace_floats of NaN in front of a sentinel
tail: the backward may depend on nothing it did not write.

GRID is a plain list of dicts and ``build`` makes every tensor from a seeded CPU generator: tests/test_cnode_ref_cpu.py imports
both and shows on the host that the bounds are not vacuous on these very cases."""
import numpy as np
import pytest
import torch

from riggs_amd import _lib as L
from tests import cnode_f64_ref as R
from tests import gpu_util as GU
from tests.gpu_util import SENT, TAIL, in_buf, out_buf, tail_intact

pytestmark = pytest.mark.gpu

LOCAL_FRAME, ROT_AS_RES = 1, 2
# entry counts of the reduce-edge layout: the 32 row lanes (31 / 32 / 33), the four-loads-in-flight loop (p + 96 < hi: 95 / 96 /
# 97, steps of 128: 127 / 128 / 129, 255 / 256 / 257), 1024, one hub, and nodes without entries first, in the middle and last
COUNTS = [0, 1, 31, 32, 33, 95, 96, 97, 0, 127, 128, 129, 255, 256, 257, 1024, 5000, 0]
COT_KINDS = ["random", "consistent", "sparse", "zero", "last"]


def _cot(N, w, kind, g):
    t = torch.randn(N, w, generator=g)
    if kind == "consistent":
        t = 1 + 0.3 * t
    elif kind == "sparse":
        t = t * (torch.rand(N, 1, generator=g) < 0.05).float()
    elif kind == "zero":
        t = t * 0
    elif kind == "last":
        t[:-1] = 0
    return t.contiguous()


def build(c):
    """Every tensor of case ``c`` on the CPU.  ``degen``: the deliberately degenerate rows (on a node, far away, u ~ 1e-7)."""
    g = torch.Generator().manual_seed(c["seed"])
    N, M, K, H = c["N"], c["M"], c["K"], c["hyper"]
    degen = torch.zeros(N, dtype=torch.bool)
    if c.get("layout") == "cluster":
        cnt = torch.tensor(COUNTS)
        assert M == len(COUNTS) and N == int(cnt.sum())
        nxyz = torch.zeros(M, 3)
        full = cnt > 0
        nxyz[full, 0] = 0.3 * torch.arange(int(full.sum())).float()
        nxyz[~full] = torch.tensor([[0.0, 30.0, 0.0], [0.0, 0.0, 40.0], [50.0, 0.0, 0.0]])  # never among the 3 nearest
        own = torch.repeat_interleave(torch.arange(M), cnt)[torch.randperm(N, generator=g)]
        x = nxyz[own] + 0.02 * torch.randn(N, 3, generator=g)
    else:
        x = 0.5 * torch.randn(N, 3, generator=g)
        pick = x[torch.randint(0, N, (M,), generator=g)] if N >= 4 else 0.5 * torch.randn(M, 3, generator=g)
        nxyz = pick + 0.05 * torch.randn(M, 3, generator=g)
    nodes = torch.full((M, 3 + H + 2), float("nan"))
    nodes[:, :3] = nxyz
    nodes[:, 3:3 + H] = 1e-2 + 0.02 * torch.randn(M, H, generator=g)
    feature = 0.02 * torch.randn(N, H + 3, generator=g) if H else None
    # radii against the node spacing (M nodes in a cloud of deviation 0.5): with one neighbour dominating, the weight-path
    # gradients are differences of nearly equal terms and no fp32 kernel could be held to them
    radius = np.log(min(max(0.75 * M ** (-1.0 / 3.0), 0.1), 0.5)) + 0.3 * torch.randn(M, generator=g)
    dup = []
    if c.get("ties") and M >= 16:  # four nodes duplicated bit for bit: adjacent and far apart in index
        dup = [(0, 1), (2, M - 1), (M // 2 - 1, M // 2), (3, M - 2)]
        for lo, hi in dup:
            nodes[hi] = nodes[lo]
        k = min(N // 8, 64)
        for j, (lo, hi) in enumerate(dup):
            x[j * k:(j + 1) * k] = nodes[lo, :3] + 0.03 * torch.randn(k, 3, generator=g)
    if c.get("degen") and N >= 20:
        k = N // 20
        a, b = N - 3 * k, N - 2 * k
        n0 = torch.randint(0, M, (k,), generator=g)
        x[a:a + k] = nodes[n0, :3]  # exactly on a node: distance 0
        x[b:b + k] = 1000.0 + torch.rand(k, 3, generator=g)  # every kernel weight underflows: w = 1 / K
        n2 = torch.randint(0, M, (k,), generator=g)
        dirs = torch.nn.functional.normalize(torch.randn(k, 3, generator=g), dim=1)
        x[b + k:] = nodes[n2, :3] + torch.exp(radius[n2])[:, None] * (2 * 16.1) ** 0.5 * dirs  # u ~ 1e-7 from that node
        if H:
            feature[a:a + k, :H] = nodes[n0, 3:3 + H]
            feature[b + k:, :H] = nodes[n2, 3:3 + H]
        degen[a:] = True
    mask = None
    if c["mask"] != "none":
        mask = torch.rand(N, generator=g)
        mask[::13] = 0.0
        mask[5::17] = 1.0
    weight = 0.5 * torch.randn(M, generator=g) if c["nw"] else None
    attrs = {"d_xyz": 0.1 * torch.randn(M, 3, generator=g), "d_rotation": 0.2 * torch.randn(M, 4, generator=g),
             "d_scaling": 0.05 * torch.randn(M, 3, generator=g)}
    e = torch.tensor([1.0, 0, 0, 0])
    q = e + 0.3 * torch.randn(M, 4, generator=g)
    q[::7] *= 0.6  # un-normalised local rotations
    attrs["local_rotation"] = (q - e).contiguous()
    cot = {k: (None if k in c.get("null", ()) else _cot(N, w, c["cot"], g)) for k, w in (("g_xyz", 3), ("g_rot", 4), ("g_scale", 3))}
    return dict(x=x.contiguous(), feature=feature, mask=mask, nodes=nodes, radius=radius, weight=weight, attrs=attrs, cot=cot,
                degen=degen, dup=dup)


def reference(c, t, idx, dev="cpu"):
    """tests/cnode_f64_ref.blend of case ``c`` with tensors ``t`` (from ``build``) on the lists ``idx``."""
    d = lambda v: None if v is None else v.to(dev)  # noqa: E731
    return R.blend(d(t["x"]), d(t["feature"]), d(t["mask"]), d(t["nodes"]), d(t["radius"]), d(t["weight"]),
                   {k: d(v) for k, v in t["attrs"].items()}, idx.to(dev), c["hyper"], c["local"], c["res"],
                   {k: d(v) for k, v in t["cot"].items()})


def case(N, M, K, hyper, i, **kw):
    c = dict(N=N, M=M, K=K, hyper=hyper, local=bool(i & 1), res=bool(i & 2), nw=bool(i & 4), mask=("rand" if i % 3 else "none"),
             cot=COT_KINDS[0], null=(), gf=True, gm=True, layout="random", degen=True, ties=False, seed=1000 + i)
    c.update(kw)
    return c


def _grid():
    cases = []
    n = [0]

    def add(N, M, K, hyper, **kw):
        cases.append(case(N, M, K, hyper, n[0], **kw))
        n[0] += 1

    # reduce edges: dictated entry counts at K = 1; the same layout at K = 3 (the weight path, zero-count nodes remain)
    NC = sum(COUNTS)
    add(NC, len(COUNTS), 1, 2, layout="cluster", degen=False, local=True, res=True, nw=True, mask="rand")
    add(NC, len(COUNTS), 3, 2, layout="cluster", degen=False, local=True, res=False, nw=True, mask="rand")
    # list edges: N K = 4095 / 4096 / 4097 (one list chunk), 7 / 8 / 9 / 17 list blocks (the scan's unroll by eight)
    add(1365, 48, 3, 5)       # 4095
    add(1024, 33, 4, 0)       # 4096
    add(4097, 64, 1, 9)       # 4097
    add(4000, 100, 7, 6)      # 28 000: 7 blocks
    add(4096, 64, 8, 1)       # 32 768: 8 blocks
    add(10923, 200, 3, 8)     # 32 769: 9 blocks
    add(8193, 300, 8, 10)     # 65 544: 17 blocks
    # N on both sides of the 1024-thread backward workgroup, and tiny
    for N, K, hyper in ((1, 3, 11), (1023, 2, 2), (1024, 5, 11), (1025, 6, 9), (2049, 3, 10)):
        add(N, 40, K, hyper)
    # every K (K = M among them), every boundary width, all flag combinations, ties
    for K, M, hyper in ((1, 16, 5), (2, 2, 1), (3, 64, 11), (4, 4, 6), (5, 5, 2), (6, 37, 9), (7, 7, 10), (8, 8, 0), (8, 129, 11)):
        add(513, M, K, hyper, ties=True)
    for f in range(4):
        add(777, 96, 3, (0, 1, 6, 11)[f], local=bool(f & 1), res=bool(f & 2), nw=bool(f & 1) ^ bool(f & 2), mask=("rand", "none")[f // 2],
            ties=True)
    # cotangents: kinds, NULLs singly and in pairs, NULL g_feature / g_motion_mask
    for j, kind in enumerate(COT_KINDS[1:]):
        add(1500, 64, 3, (8, 5, 2, 11)[j], cot=kind, local=True, mask="rand", nw=True)
    for null in (("g_xyz",), ("g_rot",), ("g_scale",), ("g_xyz", "g_rot"), ("g_xyz", "g_scale"), ("g_rot", "g_scale")):
        add(1400, 128, 3, 8, null=null, local=True, mask="rand", nw=True)  # (M > 100: one node whose random-sign sum happens to
    add(1400, 128, 3, 8, gf=False, local=True, mask="rand")                 # cancel is within the host test's 1 % cap)
    add(1400, 128, 3, 8, gm=False, local=True, mask="rand")
    # limits: M = 4096 (the backward's LDS bins), M = 2048 with hyper 11 (the forward's 128 KB table exactly)
    add(4097, 4096, 3, 1, local=True, res=True, nw=True, mask="rand")
    add(3000, 2048, 3, 11, local=True, res=True, nw=True, mask="rand")
    return cases


GRID = _grid()
SHIPPED = case(20011, 512, 3, 8, 77, local=True, res=True, nw=True, mask="rand", seed=4077)


def random_case(seed):
    r = np.random.RandomState(4300 + seed)
    M = int(r.choice([8, 40, 64, 512, 1024]))
    return dict(N=int(r.choice([1, 255, 1023, 1025, 4097, 20011])), M=M, K=int(r.randint(1, 9)), hyper=int(r.choice([0, 1, 2, 5, 6, 8, 9, 10, 11])),
                local=bool(r.randint(2)), res=bool(r.randint(2)), nw=bool(r.randint(2)), mask=str(r.choice(["none", "rand"])),
                cot=str(r.choice(COT_KINDS)), null=tuple(k for k in ("g_xyz", "g_rot", "g_scale") if r.rand() < 0.2), gf=bool(r.rand() < 0.8),
                gm=bool(r.rand() < 0.8), layout="random", degen=True, ties=bool(r.randint(2)), seed=5300 + seed)


RANDOM = [random_case(s) for s in range(16)]


def case_id(c):
    return "N%d-M%d-K%d-h%d-%s%s%s-%s-%s%s%s%s%s" % (
        c["N"], c["M"], c["K"], c["hyper"], "L" if c["local"] else "g", "r" if c["res"] else "a", "w" if c["nw"] else "", c["mask"], c["cot"],
        "".join("-no_" + k for k in c["null"]), "" if c["gf"] else "-nogf", "" if c["gm"] else "-nogm",
        "-cluster" if c["layout"] == "cluster" else ("-ties" if c["ties"] else ""))


def check(what, got, rb, must_zero=None):
    ref, bnd = rb
    R.assert_within(what, got.double().reshape(ref.shape), ref, bnd, must_zero=must_zero, stats=GU.STATS)


def flags_of(c):
    return (LOCAL_FRAME if c["local"] else 0) | (ROT_AS_RES if c["res"] else 0)


class Buffers:
    """Device inputs of a case (per-Gaussian ones in front of a NaN tail) and its outputs in front of sentinel tails."""

    def __init__(self, c, t):
        N, M, K, H = c["N"], c["M"], c["K"], c["hyper"]
        self.x = in_buf(t["x"])[0]
        self.feature = None if t["feature"] is None else in_buf(t["feature"])[0]
        self.mask = None if t["mask"] is None else in_buf(t["mask"])[0]
        self.cot = {k: (None if v is None else in_buf(v)[0]) for k, v in t["cot"].items()}
        cu = lambda v: None if v is None else v.cuda().contiguous()  # noqa: E731
        self.nodes, self.radius, self.weight = cu(t["nodes"]), cu(t["radius"]), cu(t["weight"])
        self.attrs = {k: cu(v) for k, v in t["attrs"].items()}
        self.fs = 0 if t["feature"] is None else t["feature"].shape[1]
        self.out = {"d_xyz": out_buf((N, 3)), "d_rotation": out_buf((N, 4)), "d_scaling": out_buf((N, 3)),
                    "nn_idx": out_buf((N, K), torch.int32, -77), "nn_weight": out_buf((N, K)), "nn_dist": out_buf((N, K))}
        nan = float("nan")
        self.grad = {"g_trans": out_buf((M, 3), fill=nan), "g_rot": out_buf((M, 4), fill=nan), "g_scale": out_buf((M, 3), fill=nan),
                     "g_local_rot": out_buf((M, 4), fill=nan), "g_radius": out_buf((M,), fill=nan)}
        if c["nw"]:
            self.grad["g_weight"] = out_buf((M,), fill=nan)
        if H:
            self.grad["g_nodes_hyper"] = out_buf((M, H), fill=nan)
            if c["gf"]:
                self.grad["g_feature"] = out_buf((N, self.fs), fill=nan)
        if self.mask is not None and c["gm"]:
            self.grad["g_mask"] = out_buf((N,), fill=nan)

    def front(self, c):
        H = c["hyper"]
        return (c["N"], c["M"], c["K"], H, self.fs, self.nodes.shape[1], flags_of(c), L.ptr(self.x), L.ptr(self.feature), L.ptr(self.mask),
                self.nodes.data_ptr(), self.radius.data_ptr(), L.ptr(self.weight), self.attrs["d_xyz"].data_ptr(),
                self.attrs["d_rotation"].data_ptr(), self.attrs["d_scaling"].data_ptr(),
                self.attrs["local_rotation"].data_ptr() if c["local"] else None)

    def forward(self, c):
        o = self.out
        return L.lib().riggs_cnode_forward(*self.front(c), o["d_xyz"][0].data_ptr(), o["d_rotation"][0].data_ptr(), o["d_scaling"][0].data_ptr(),
                                           o["nn_idx"][0].data_ptr(), o["nn_weight"][0].data_ptr(), o["nn_dist"][0].data_ptr(), L.stream_ptr())

    def workspace(self, c):
        n = int(L.lib().riggs_cnode_backward_workspace_floats(c["N"], c["M"], c["K"], c["hyper"]))
        ws = torch.full((n + TAIL,), float("nan"), dtype=torch.float32, device="cuda")
        ws[n:] = SENT
        return ws, n

    def backward(self, c, ws):
        gp = lambda k: self.grad[k][0].data_ptr() if k in self.grad else None  # noqa: E731
        return L.lib().riggs_cnode_backward(*self.front(c), self.out["nn_idx"][0].data_ptr(), self.out["nn_dist"][0].data_ptr(),
                                            L.ptr(self.cot["g_xyz"]), L.ptr(self.cot["g_rot"]), L.ptr(self.cot["g_scale"]), gp("g_feature"),
                                            gp("g_mask"), gp("g_trans"), gp("g_rot"), gp("g_scale"), gp("g_local_rot"), gp("g_radius"),
                                            gp("g_weight"), gp("g_nodes_hyper"), ws.data_ptr(), L.stream_ptr())

    def tails_intact(self, c):
        N, M = c["N"], c["M"]
        for k, (_, buf) in self.out.items():
            assert tail_intact(buf, N, -77 if k == "nn_idx" else SENT), "write past the end of " + k
        for k, (_, buf) in self.grad.items():
            assert torch.isnan(buf[(N if k in R.GAUSS_KEYS else M):]).all(), "write past the end of " + k


def check_backward(c, b, ref, tag):
    H = c["hyper"]
    for k, (view, _) in b.grad.items():
        if k == "g_feature":
            assert bool((view[:, H:] == 0).all()), "g_feature's columns past hyper_dim are not exactly 0 " + tag
            check(k + " " + tag, view[:, :H], ref[k])
        elif k == "g_local_rot" and not c["local"]:
            assert bool((view == 0).all()), "g_local_rot without local_frame is not exactly 0 " + tag
        else:
            check(k + " " + tag, view, ref[k])


def run_case(c, twice=False):
    tag = case_id(c)
    t = build(c)
    b = Buffers(c, t)
    N, M, K, H = c["N"], c["M"], c["K"], c["hyper"]
    L.check(b.forward(c), "riggs_cnode_forward")
    torch.cuda.synchronize()
    b.tails_intact(c)
    idx = b.out["nn_idx"][0]
    dev = lambda v: None if v is None else v.cuda()  # noqa: E731
    nbad = R.selection_violations(dev(t["x"]), dev(t["feature"]), dev(t["nodes"]), H, idx, b.out["nn_dist"][0])
    assert nbad == 0, "%d neighbour lists break the float64 selection rule %s" % (nbad, tag)
    if c["layout"] == "cluster" and K == 1:
        assert torch.bincount(idx.long().reshape(-1), minlength=M).tolist() == COUNTS, tag
    if t["dup"]:
        twins = torch.tensor(sorted({j for p in t["dup"] for j in p}), device="cuda")
        around = 4 * min(N // 8, 64)  # (the Gaussians build() put around the duplicated nodes)
        rows = torch.isin(idx.long(), twins).any(1) & (torch.arange(N, device="cuda") < around)
        true = R.true_lists(dev(t["x"]), dev(t["feature"]), dev(t["nodes"]), H, K)
        assert int(rows.sum()) > 0 or around == 0, tag
        assert torch.equal(idx.long()[rows], true[rows]), "ties: not the stable float64 order " + tag
    ref = reference(c, t, idx, "cuda")
    for k in R.FWD_KEYS:
        check(k + " " + tag, b.out[k][0], ref[k])
    ws, n = b.workspace(c)
    runs = []
    for _ in range(2 if twice else 1):  # (the second run: on the first run's leftovers)
        L.check(b.backward(c, ws), "riggs_cnode_backward")
        torch.cuda.synchronize()
        assert bool((ws[n:] == SENT).all()), "write past the end of the workspace " + tag
        b.tails_intact(c)
        check_backward(c, b, ref, tag)
        runs.append({k: v[0].clone() for k, v in b.grad.items()})
    if twice:
        same = all(torch.equal(runs[0][k].view(torch.int32), runs[1][k].view(torch.int32)) for k in runs[0])
        print("two backward runs on one workspace bit-identical: %s %s" % (same, tag))


@pytest.mark.parametrize("c", GRID, ids=[case_id(c) for c in GRID])
def test_blend_against_float64(c):
    run_case(c)


@pytest.mark.parametrize("c", RANDOM, ids=["%d-%s" % (i, case_id(c)) for i, c in enumerate(RANDOM)])
def test_random_blend_against_float64(c):
    run_case(c)


def test_shipped_shape_twice_on_one_workspace():
    run_case(SHIPPED, twice=True)


@pytest.mark.parametrize("which,M,hyper,msg", [("forward", 2049, 11, "128 KB"), ("backward", 4097, 1, "4096")])
def test_sizes_past_the_limits_are_refused_without_a_launch(which, M, hyper, msg):
    c = case(64, M, 3, hyper, 5, seed=9)
    b = Buffers(c, build(c))
    if which == "forward":
        rc = b.forward(c)
    else:
        b.out["nn_idx"][0].zero_()
        b.out["nn_dist"][0].zero_()
        ws, n = b.workspace(c)
        rc = b.backward(c, ws)
    torch.cuda.synchronize()
    assert rc != 0 and msg in L.lib().riggs_last_error().decode(errors="replace")
    for k, (view, _) in (b.out if which == "forward" else b.grad).items():  # nothing was launched: every output as it was filled
        fill = -77 if k == "nn_idx" else SENT
        assert bool((view == fill).all()) if which == "forward" else bool(torch.isnan(view).all()), k
    if which == "backward":
        assert bool(torch.isnan(ws[:n]).all())


def test_no_gaussians_through_the_c_abi():
    """N = 0 with every per-Gaussian pointer NULL: the forward returns, the backward writes zero node gradients."""
    c = case(0, 24, 3, 5, 7, seed=11)
    b = Buffers(c, build(c))
    b.x = b.feature = b.mask = None
    b.cot = {k: None for k in b.cot}
    lib = L.lib()
    f = b.front(c)
    L.check(lib.riggs_cnode_forward(*f, None, None, None, None, None, None, L.stream_ptr()), "riggs_cnode_forward")
    ws, n = b.workspace(c)
    gp = lambda k: b.grad[k][0].data_ptr() if k in b.grad else None  # noqa: E731
    L.check(lib.riggs_cnode_backward(*f, None, None, None, None, None, None, None, gp("g_trans"), gp("g_rot"), gp("g_scale"),
                                     gp("g_local_rot"), gp("g_radius"), gp("g_weight"), gp("g_nodes_hyper"), ws.data_ptr(), L.stream_ptr()),
            "riggs_cnode_backward")
    torch.cuda.synchronize()
    assert bool((ws[n:] == SENT).all())
    for k, (view, buf) in b.grad.items():
        if k in R.NODE_KEYS:
            assert bool((view == 0).all()) and torch.isnan(buf[c["M"]:]).all(), k


def test_no_gaussians_through_autograd():
    """An empty selection through control_node_blend and .sum().backward(): empty tensors' data_ptr() is 0."""
    from riggs_amd.control_nodes import control_node_blend
    c = case(0, 24, 3, 5, 7, seed=11)
    t = build(c)
    rg = lambda v: v.cuda().requires_grad_(True)  # noqa: E731
    nodes = rg(t["nodes"][:, :3 + c["hyper"]].contiguous())
    feature, radius, weight = rg(t["feature"]), rg(t["radius"]), rg(t["weight"].reshape(-1, 1))
    mask = rg(torch.zeros(0, 1))
    attrs = {k: rg(v) for k, v in t["attrs"].items()}
    out = control_node_blend(t["x"].cuda(), feature, mask, nodes, radius, weight, attrs, K=3, hyper_dim=c["hyper"], local_frame=True,
                             d_rot_as_res=True)
    assert out["d_xyz"].shape == (0, 3) and out["nn_idx"].shape == (0, 3)
    (out["d_xyz"].sum() + out["d_rotation"].sum() + out["d_scaling"].sum()).backward()
    for k, v in list(attrs.items()) + [("nodes", nodes), ("_node_radius", radius), ("_node_weight", weight)]:
        assert v.grad is not None and v.grad.shape == v.shape and bool((v.grad == 0).all()), k
