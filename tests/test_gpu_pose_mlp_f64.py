"""-m gpu: the PoseMLP kernels (csrc/pose_mlp.hip) pinned per element to float64 (tests/pose_mlp_ref.py), stage by stage, through
the C ABI so that every output and workspace is under the test's control.  Each stage is checked from the fp32 values the kernel
itself read (acts, the bias gradients, dL/dlocal_rot / dL/dglobal_trans), and the whole against a float64 autograd network, across
the dispatch rules (one launch with the heads inside the width / with head workgroups of their own / one launch per layer by size
or by option / the two chain placements), the 64-lane and 8-row granule edges, depth, skip, multires, t, the cotangents and the
options of the _fk entry.  Every output is a view into a larger buffer whose sentinel tail must survive, weights and cotangents
sit in front of NaN tails, flat_grads and the workspace are NaN-filled at exactly the size the library states."""
import ctypes as C

import numpy as np
import pytest
import torch

from riggs_amd import _lib as L
from tests import gpu_util as GU
from tests import pose_mlp_ref as P
from tests.gpu_util import SENT, TAIL, in_buf, out_buf, tail_intact

pytestmark = pytest.mark.gpu

GRID = P.grid()
DRAWS = [P.random_case(i) for i in range(16)]
_BY_NAME = {c["name"]: c for c in GRID}
WORST, VAC = {}, {}          # case [path] -> {array: worst err / bound}, {array: vacuity share}  (tools/pose_mlp_parity.py)
MEASURED = {"sincos_ulp": 0.0}
_SYNC = {}                   # (depth, width) -> the persistent hand-off state, zeroed once


def _nan_front(n):
    """n NaN floats in front of a sentinel tail."""
    buf = torch.full((n + TAIL,), SENT, dtype=torch.float32, device="cuda")
    buf[:n] = float("nan")
    return buf[:n], buf


def _sync_state(c):
    key = (c["depth"], c["width"])
    if key not in _SYNC:
        words = int(L.lib().riggs_pose_mlp_sync_bytes(c["depth"], c["width"])) // 4
        _SYNC[key] = torch.zeros(words, dtype=torch.int32, device="cuda")
    return _SYNC[key]


class Net:
    """The device copies of one case's parameters (each in front of a NaN tail) and the C entries' pointer arguments."""

    def __init__(self, c, p):
        self.c, self.p = c, p
        self.keep = []
        dev = lambda a: self._in(torch.from_numpy(np.ascontiguousarray(a)))  # noqa: E731
        self.W = [dev(x) for x in p["W"]]
        self.b = [dev(x) for x in p["b"]]
        self.heads = [dev(p[k]) for k in ("W_rot", "b_rot", "W_tr", "b_tr")]
        d = c["depth"]
        self.Wp = (C.c_void_p * d)(*[x.data_ptr() for x in self.W])
        self.bp = (C.c_void_p * d)(*[x.data_ptr() for x in self.b])
        self.rot_bias = None if p["rot_bias"] is None else dev(p["rot_bias"])
        self.g_rot, self.g_tr = dev(p["g_rot"]), dev(p["g_tr"])

    def _in(self, t):
        v, buf = in_buf(t)
        self.keep.append(buf)
        return v

    def shape_args(self):
        c = self.c
        return (c["depth"], c["width"], c["multires"], c["skip"], c["n_rot"], self.Wp, self.bp) + tuple(x.data_ptr() for x in self.heads)

    def forward(self, t, sync):
        c, lib = self.c, L.lib()
        n_acts = int(lib.riggs_pose_mlp_acts_floats(c["depth"], c["width"], c["multires"]))
        acts, actsb = out_buf((n_acts,))
        rot, rotb = out_buf((c["n_rot"],))
        tr, trb = out_buf((3,))
        tt = torch.tensor([float(t)], dtype=torch.float32, device="cuda")
        L.check(lib.riggs_pose_mlp_forward(*self.shape_args(), tt.data_ptr(), L.ptr(self.rot_bias), L.ptr(sync), acts.data_ptr(),
                                           rot.data_ptr(), tr.data_ptr(), L.stream_ptr()), "riggs_pose_mlp_forward")
        torch.cuda.synchronize()
        assert tail_intact(actsb, n_acts) and tail_intact(rotb, c["n_rot"]) and tail_intact(trb, 3), "a forward output's tail was written"
        return {"acts_dev": acts, "acts": acts[:c["emb"] + c["depth"] * c["width"]].cpu().numpy(), "rotation": rot.cpu().numpy(),
                "translation": tr.cpu().numpy()}

    def backward(self, fw, sync, transforms=None, force_outs=False):
        c, p, lib = self.c, self.p, L.lib()
        _, total = P.layout(c)
        flat, flatb = _nan_front(total)
        n_ws = int(lib.riggs_pose_mlp_backward_workspace_floats(c["depth"], c["width"], c["multires"]))
        ws, wsb = _nan_front(n_ws)
        out = {}
        fk = p.get("fk")
        if fk is None:
            L.check(lib.riggs_pose_mlp_backward(*self.shape_args(), fw["acts_dev"].data_ptr(), self.g_rot.data_ptr(), self.g_tr.data_ptr(),
                                                ws.data_ptr(), flat.data_ptr(), L.ptr(sync), L.stream_ptr()), "riggs_pose_mlp_backward")
            torch.cuda.synchronize()
        else:
            J = c["J"]
            dev = lambda a: self._in(torch.from_numpy(np.ascontiguousarray(a)))  # noqa: E731
            q, joints, dG = dev(fk["local_rot"]), dev(fk["joints"]), dev(fk["dG"])
            par = torch.from_numpy(fk["parents"]).to(torch.int32).cuda()
            gn = dev(fk["gn"]) if fk["gn"] is not None else None
            coef = None if fk["coef"] is None else torch.tensor([fk["coef"]], dtype=torch.float32, device="cuda")
            outs = fk["outs"] or force_outs
            dq, dqb = out_buf((J, 4))
            dgt, dgtb = out_buf((3,))
            loss, lossb = out_buf((1,))
            L.check(lib.riggs_pose_mlp_backward_fk(*self.shape_args(), fw["acts_dev"].data_ptr(), J, q.data_ptr(), joints.data_ptr(),
                                                   par.data_ptr(), L.ptr(transforms), dG.data_ptr(), L.ptr(gn),
                                                   self.g_rot.data_ptr() if fk["g_rot"] else None,
                                                   self.g_tr.data_ptr() if fk["g_tr"] else None,
                                                   dq.data_ptr() if outs else None, dgt.data_ptr() if outs else None, L.ptr(coef),
                                                   loss.data_ptr() if fk["loss"] else None, ws.data_ptr(), flat.data_ptr(), L.ptr(sync),
                                                   L.stream_ptr()), "riggs_pose_mlp_backward_fk")
            torch.cuda.synchronize()
            assert tail_intact(dqb, J) and tail_intact(dgtb, 3) and tail_intact(lossb, 1), "an _fk output's tail was written"
            if outs:
                out["dq"], out["dgt"] = dq.cpu().numpy(), dgt.cpu().numpy()
            else:
                assert bool((dq == SENT).all()) and bool((dgt == SENT).all()), "an output that was not asked for was written"
            if fk["loss"]:
                out["loss"] = loss.cpu().numpy()
            else:
                assert float(loss[0]) == np.float32(SENT)
        assert tail_intact(flatb, total) and tail_intact(wsb, n_ws), "the tail of flat_grads / the workspace was written"
        out["flat"] = flat.cpu().numpy()
        return out


def _transforms(p, J):
    """The chain's forward result as riggs_fk_forward leaves it (what the frame hands to the _fk entry)."""
    fk = p["fk"]
    q, joints = torch.from_numpy(fk["local_rot"]).cuda(), torch.from_numpy(fk["joints"]).cuda()
    par = torch.from_numpy(fk["parents"]).to(torch.int32).cuda()
    gt = torch.zeros(3, device="cuda")
    tr, nr, dn = (torch.empty(J, n, device="cuda") for n in (12, 4, 3))
    L.check(L.lib().riggs_fk_forward(J, q.data_ptr(), joints.data_ptr(), par.data_ptr(), gt.data_ptr(), tr.data_ptr(), nr.data_ptr(),
                                     dn.data_ptr(), L.stream_ptr()), "riggs_fk_forward")
    return tr


def _handoff_clean(c, sync, out, what):
    """A one-launch kernel can time out on a shared GPU: that is reported as such, not as an arithmetic failure."""
    word = int(L.lib().riggs_pose_mlp_status_word(c["depth"], c["width"]))
    hit = sync is not None and int(sync[word].item()) != 0
    nan = any(not np.isfinite(out[k]).all() for k in ("acts", "rotation", "translation", "flat", "dq", "dgt") if out.get(k) is not None)
    if hit:
        sync[word] = 0
    assert not hit and not nan, "%s: hand-off time-out (status word %s, NaN in the outputs %s)" % (what, hit, nan)


def run(case, layered_option, sync="case", placement=None, t=None, net=None):
    """One forward + backward of a case; returns (c, p, out, layered)."""
    c, p = P.make(case)
    if t is not None:
        p["t"] = np.float32(t)
    layered = not P.one_launch(c, layered_option)
    net = Net(c, p) if net is None else net
    use_sync = case["kw"].get("sync", True) if sync == "case" else sync
    st = _sync_state(c) if use_sync else None
    old = L.get_option("pose_mlp_layered")
    try:
        if layered_option:
            L.set_option("pose_mlp_layered", 1)
        if placement is not None:
            L.lib().riggs_pose_mlp_set_placement(placement)
        fw = net.forward(p["t"], st)
        fk = p.get("fk")
        tr = _transforms(p, c["J"]) if fk is not None and fk["transforms"] else None
        out = net.backward(fw, st, tr, force_outs=layered)
    finally:
        L.set_option("pose_mlp_layered", old)
        L.lib().riggs_pose_mlp_set_placement(1)
    out.update(fw)
    _handoff_clean(c, st, out, case["name"])
    return c, p, out, layered


def check(case, layered_option, **kw):
    c, p, out, layered = run(case, layered_option, **kw)
    tag = "%s [%s]" % (case["name"], "layered" if layered else "one launch")
    MEASURED["sincos_ulp"] = max(MEASURED["sincos_ulp"], P.sincos_ulp_error(c, p["t"], out["acts"]))
    res = P.check_stages(c, p, out, layered)
    P.check_end_to_end(c, p, out, layered, res)
    WORST[tag] = {k: v["worst"] for k, v in res.items()}
    VAC[tag] = {k: v["vac"] for k, v in res.items()}
    for k, v in res.items():
        GU.STATS.append(("pose_mlp %s %s [err/bound]" % (k, tag), v["n"], v["bad"] / max(1, v["n"]), v["worst"], v["bad"] / max(1, v["n"])))
    bad = {k: (v["bad"], v["worst"], v["first"]) for k, v in res.items() if v["bad"]}
    assert not bad, "%s: elements outside the bound (count, worst err/bound, first index): %r" % (tag, bad)
    return out


def _ids(cases):
    return [c["name"] for c in cases]


@pytest.mark.parametrize("case", GRID, ids=_ids(GRID))
def test_grid_against_float64(case):
    check(case, False)


ONE_LAUNCH = [c for c in GRID if P.one_launch(P.make(c)[0])]


@pytest.mark.parametrize("case", ONE_LAUNCH, ids=_ids(ONE_LAUNCH))
def test_one_launch_cases_again_one_launch_per_layer(case):
    check(case, True)


@pytest.mark.parametrize("seed", range(16))
def test_random_draws_against_float64(seed):
    case = DRAWS[seed]
    check(case, False)
    if P.one_launch(P.make(case)[0]):
        check(case, True)


def _same_bits(a, b, keys=("acts", "rotation", "translation", "flat")):
    for k in keys:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


@pytest.mark.parametrize("name", ["inside 256x24", "extra 128x64", "inside 20x4"])
def test_the_two_placements_give_the_same_bits(name):
    case = _BY_NAME[name]
    a = check(case, False, placement=1)
    b = check(case, False, placement=0)
    _same_bits(a, b)


@pytest.mark.parametrize("name", P.STATE_CASES)
def test_three_launches_on_one_sync_state(name):
    """Each launch held to its own reference; the first t again gives the first bits (no granule of another launch is taken)."""
    case = _BY_NAME[name]
    outs = [check(case, False, sync=True, t=t) for t in P.STATE_TS + P.STATE_TS[:1]]
    _same_bits(outs[0], outs[3])
    assert not np.array_equal(outs[0]["rotation"], outs[1]["rotation"])


@pytest.mark.parametrize("name,sync", [("inside 256x24", True), ("extra 128x64", False), ("fk J=24", True)])
def test_two_backwards_over_one_acts_give_equal_bits(name, sync):
    case = _BY_NAME[name]
    c, p = P.make(case)
    net = Net(c, p)
    st = _sync_state(c) if sync else None
    fw = net.forward(p["t"], st)
    tr = _transforms(p, c["J"]) if p.get("fk") is not None and p["fk"]["transforms"] else None
    a = net.backward(fw, st, tr)
    b = net.backward(fw, st, tr)
    a.update(fw)
    _handoff_clean(c, st, a, name)
    _same_bits(a, b, [k for k in ("flat", "dq", "dgt", "loss") if k in a])
    res = P.check_stages(c, p, a, False)
    assert not [k for k, v in res.items() if v["bad"]]


def test_measured_sincos_error_is_within_the_allowance():
    """SINCOS_ULP is twice the worst error measured over the grid, rounded up to a whole ulp; more than 4 ulp would be a finding."""
    for t in P.EMBED_TS:
        check(_BY_NAME[P.EMBED_CASE], False, t=t)
    assert 2.0 * MEASURED["sincos_ulp"] <= P.SINCOS_ULP <= 4.0, MEASURED


def test_depth_two_takes_the_torch_path_and_raises_its_shape_error():
    """PoseMLP(depth <= 2): the skip sits on the last layer, the heads are Linear(hidden, ...) and h is [emb, h].  The reference
    raises a shape error; so does this module, on the torch-op path — no kernel is launched."""
    from riggs_amd.skeleton import PoseMLP
    net = PoseMLP(1, 16, depth=2, hidden_dimensions=32).cuda()
    t = torch.tensor([0.37], device="cuda")
    assert not net._fusable(t)
    with pytest.raises(RuntimeError):
        net(t)
