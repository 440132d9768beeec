"""GPU: the node network (riggs_amd/node_network.py over csrc/node_mlp.hip) against the reference's float64 fixtures and the
float64 restatement of tests/node_mlp_ref.py, through the module and through the C ABI.

Bounds (none of them from what the kernels give):
  outputs, hidden     1e-5 of the tensor's maximum against float64 (the project's bar for values; the reference's own float32
                      run sits at 0.6-1.1e-6 on the fixtures).
  parameter gradients 1e-4 of the tensor's maximum against the float64 restatement WITH THE RELU MASKS PINNED to the activations
                      the kernel stored; one flipped unit alone moves a weight gradient by ~1/R of its maximum.
  the masks           a kernel mask may differ from the float64 mask only where |pre| <= 32 eps32 sum_k |w_k a_k| (float64, per
                      unit), and at most 2e-6 of the units differ — counted per fixture, and over all cases of the sweep
                      together (a single case of R = 1 has 2 304 units: a share of one case means nothing).
  fixtures without a differing mask are also compared directly, unpinned.
"""
import ctypes as C
import itertools
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import gpu_util as GU
from tests import node_mlp_ref as NR
from tests.test_node_mlp_cpu import FIXTURES, SUBROWS, compare_grads, fixture_cot, load_fixture

pytestmark = pytest.mark.gpu
EPS32 = 2.0 ** -24 * 2   # float32 machine epsilon (2^-23)
OUT_TOL, GRAD_TOL, MASK_SHARE = 1e-5, 1e-4, 2e-6
WIDTH = dict(d_xyz=3, d_scaling=3, d_rotation=4, local_rotation=4, d_opacity=1)


def _module(cfg, params=None):
    from riggs_amd.node_network import DeformNetwork
    net = DeformNetwork(D=8, W=cfg["W"], is_blender=cfg["is_blender"], local_frame=cfg["local_frame"],
                        pred_opacity=cfg["pred_opacity"], max_d_scale=cfg["max_d_scale"])
    if params is not None:
        net.load_state_dict({k: v.float() for k, v in params.items()})
    net = net.cuda()
    net.keep_stored_activations = True
    return net


def _heads(cfg):
    return [k for k in NR.OUT_KEYS if not (k == "local_rotation" and not cfg["local_frame"])
            and not (k == "d_opacity" and not cfg["pred_opacity"])]


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _run_module(net, x, t, cot):
    for p in net.parameters():
        p.grad = None
    out = net(x, t)
    loss = sum((out[k] * cot[k]).sum() for k in cot)
    loss.backward()
    st = net.stored_activations
    return out, OrderedDict((k, p.grad.clone()) for k, p in net.named_parameters()), st


def _masks(st, cfg):
    return {"act": (st["act"] > 0), "timenet": (st["timenet_hidden"] > 0) if cfg["is_blender"] else None}


def _mask_check(params64, x, t, cfg, masks, free=None):
    """(units, differing units); every differing unit obeys the |pre| bound (asserted here)."""
    out = free if free is not None else NR.forward(params64, x.double(), t.double(), cfg)
    ap = {k: v.abs() for k, v in params64.items()}
    units = diff = 0

    def one(pre, inp, name, km):
        nonlocal units, diff
        d = (pre > 0) != km
        units += pre.numel()
        n = int(d.sum())
        if n:
            s = inp.abs() @ ap[name + ".weight"].t() + ap[name + ".bias"]
            assert bool((pre.abs()[d] <= 32 * EPS32 * s[d]).all()), "%s: a ReLU mask differs away from zero" % name
            diff += n
    if cfg["is_blender"]:
        tt = t.double().reshape(-1, 1).expand(x.shape[0], 1)
        one(out["timenet_pre"], NR.embed(tt, 6), "timenet.0", masks["timenet"])
    h = out["inp"]
    for l in range(8):
        one(out["pre"][l], h, "linear.%d" % l, masks["act"][l])
        h = torch.cat([out["inp"], out["act"][l]], -1) if l == 4 else out["act"][l]
    return units, diff


def _check_case(cfg, params64, x, t, cot, out, grads, st, what, record=True):
    """outputs / hidden against the free float64 run, gradients against the pinned one; returns (units, differing)."""
    free = NR.forward(params64, x.double(), t.double(), cfg)
    for k in _heads(cfg) + ["hidden"]:
        e = _rel(out[k], free[k])
        if record:
            GU.STATS.append(("node_mlp %s %s" % (what, k), int(out[k].numel()), 0.0, e, 0.0))
        assert e <= OUT_TOL, "%s %s: %.3g" % (what, k, e)
    masks = _masks(st, cfg)
    _, g64 = NR.grads(params64, x.double(), t.double(), cfg, {k: v.double() for k, v in cot.items()}, masks=masks)
    for k, g in grads.items():
        e = _rel(g, g64[k])
        if record:
            GU.STATS.append(("node_mlp %s grad %s" % (what, k), int(g.numel()), 0.0, e, 0.0))
        assert e <= GRAD_TOL, "%s grad %s: %.3g" % (what, k, e)
    return _mask_check(params64, x, t, cfg, masks, free)


# ------------------------------------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("key", FIXTURES)
def test_fixtures_through_the_module(golden_dir, key):
    cfg, params, z = load_fixture(golden_dir, key)
    net = _module(cfg, params)
    x, t = torch.from_numpy(z["x"]).cuda(), torch.from_numpy(z["t"]).cuda()
    cot = {k: v.cuda() for k, v in fixture_cot(z).items()}
    out, grads, st = _run_module(net, x, t, cot)
    assert set(out.keys()) == {"d_xyz", "d_rotation", "d_scaling", "hidden", "d_opacity", "d_color"} | ({"local_rotation"} if cfg["local_frame"] else set())
    assert out["d_color"] is None and (out["d_opacity"] is None) == (not cfg["pred_opacity"])
    assert not out["hidden"].requires_grad and out["d_xyz"].requires_grad
    for k in z.files:
        if k.startswith("out/"):
            mine = out[k[4:]].detach().cpu().numpy()
            mine = mine[:50] if k == "out/hidden" else mine
            e = float(np.abs(mine - z[k]).max() / np.abs(z[k]).max())
            GU.STATS.append(("node_mlp fixture %s %s" % (key, k), int(z[k].size), 0.0, e, 0.0))
            print("fixture", key, k, e)
            assert e <= OUT_TOL, (k, e)
    p64 = OrderedDict((k, v.double().cuda()) for k, v in params.items())
    units, diff = _check_case(cfg, p64, x, t, cot, out, grads, st, "fixture " + key)
    print("fixture", key, "mask units", units, "differing", diff)
    assert diff <= MASK_SHARE * units
    if diff == 0:
        compare_grads(grads, z, GRAD_TOL, record=lambda k, e: print("fixture", key, k, e))


# --------------------------------------------------------------------------------------------------- C ABI, the sweep
def _capi(cfg, params32, x, t, t_stride, cot, pad=64):
    """One forward + backward through the C ABI with NaN tails behind the inputs and sentinel tails behind every output."""
    from riggs_amd import _lib as L
    from riggs_amd import node_network as NN
    lib = L.lib()
    R, W, dev = x.shape[0], cfg["W"], "cuda"
    heads = _heads(cfg)
    present = (True, True, True, cfg["local_frame"], cfg["pred_opacity"])
    c = NN._Cfg(W, cfg["is_blender"], float(cfg["max_d_scale"]), present)
    plist = [params32[k] for k in NR.param_shapes(cfg)]

    def padded(n, fill):
        b = torch.full((n + pad,), fill, dtype=torch.float32, device=dev)
        return b
    xb = padded(R * 3, float("nan")); xb[:R * 3] = x.reshape(-1)
    nt = R if t_stride else 1
    tb = padded(nt, float("nan")); tb[:nt] = t.reshape(-1)[:nt]
    SENT = 12345.5
    n_acts = int(lib.riggs_node_mlp_acts_floats(R, W, 8))
    acts = padded(n_acts, SENT)
    outs = {k: padded(R * WIDTH[k], SENT) for k in heads}
    net = NN._net_struct(c, plist)
    optr = [outs[k].data_ptr() if k in outs else None for k in NR.OUT_KEYS]
    L.check(lib.riggs_node_mlp_forward(C.byref(net), R, xb.data_ptr(), tb.data_ptr(), t_stride, acts.data_ptr(), *optr,
                                       L.stream_ptr()), "forward")
    cb = {k: padded(R * WIDTH[k], float("nan")) for k in heads}
    for k in heads:
        cb[k][:R * WIDTH[k]] = cot[k].reshape(-1)
    ws = padded(int(lib.riggs_node_mlp_backward_workspace_floats(R, W, 8)), SENT)
    gb = [padded(p.numel(), SENT) for p in plist]
    gst = NN._fill(L.NodeMlpGrads(), c, gb)
    cptr = [cb[k].data_ptr() if k in cb else None for k in NR.OUT_KEYS]
    L.check(lib.riggs_node_mlp_backward(C.byref(net), R, acts.data_ptr(), *cptr, ws.data_ptr(), C.byref(gst), L.stream_ptr()),
            "backward")
    for b in [acts, ws] + list(outs.values()) + gb:
        assert bool((b[-pad:] == SENT).all()), "a sentinel tail was overwritten"
    out = {k: outs[k][:R * WIDTH[k]].view(R, WIDTH[k]) for k in heads}
    off = int(lib.riggs_node_mlp_hidden_offset(R, W, 8))
    out["hidden"] = acts[off:off + R * W].view(R, W)
    o_t = R * (96 + 16)
    o_a = o_t + R * 256 + R * 4
    st = {"timenet_hidden": acts[o_t:o_t + R * 256].view(R, 256), "act": acts[o_a:o_a + 8 * R * W].view(8, R, W)}
    grads = OrderedDict((k, g[:p.numel()].view(p.shape)) for k, g, p in zip(NR.param_shapes(cfg), gb, plist))
    return out, grads, st


SWEEP_R = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 511, 512, 1536, 4095, 4096, 4097, 4129, 65535, 65536]
FLAGS = list(itertools.product([True, False], [True, False], [False, True], [-1, 2]))  # is_blender, local_frame, pred_opacity, max_d_scale


@pytest.mark.parametrize("W", [64, 256])
def test_float64_sweep_through_the_c_abi(W):
    """Every R (the edges of the 16- and 32-row tiles and of the switch between them at 4 096 rows included) with every flag
    combination while R <= 65, then two combinations per R (rotating through all sixteen); shared and per-row times alternate."""
    g = torch.Generator().manual_seed(1234 + W)
    units = diff = case = 0
    worst = 0.0
    for R in SWEEP_R:
        combos = FLAGS if R <= 65 else [FLAGS[(case + i * 7) % 16] for i in range(2)]
        for (bl, lf, po, mds) in combos:
            case += 1
            cfg = dict(W=W, is_blender=bl, local_frame=lf, pred_opacity=po, max_d_scale=mds)
            p64 = OrderedDict((k, v.cuda()) for k, v in NR.integer_params(cfg).items())
            p32 = OrderedDict((k, v.float().contiguous()) for k, v in p64.items())
            x = (torch.rand(R, 3, generator=g) * 2 - 1).cuda()
            shared = case % 2 == 0
            t = torch.rand(1 if shared else R, 1, generator=g).cuda()
            cot = {k: torch.randn(R, WIDTH[k], generator=g).cuda() for k in _heads(cfg)}
            out, grads, st = _capi(cfg, p32, x, t, 0 if shared else 1, cot)
            u, d = _check_case(cfg, p64, x, t.expand(R, 1), cot, out, grads, st, "W%d R%d %s" % (W, R, (bl, lf, po, mds)),
                               record=False)
            units, diff = units + u, diff + d
            del out, grads, st
    print("sweep W", W, "cases", case, "units", units, "differing masks", diff)
    GU.STATS.append(("node_mlp sweep W%d differing mask share" % W, units, 0.0, diff / units, 0.0))
    assert diff <= MASK_SHARE * units


# ------------------------------------------------------------------------------------------------- module behaviour
def _shipped(W=256, seed=0):
    cfg = dict(NR.CONFIGS["a"], W=W)
    params = NR.integer_params(cfg)
    return cfg, params, _module(cfg, params)


def test_four_calls_of_a_node_rendering_iteration_accumulate():
    cfg, params, net = _shipped()
    p64 = OrderedDict((k, v.cuda()) for k, v in params.items())
    g = torch.Generator().manual_seed(5)
    want = None
    for p in net.parameters():
        p.grad = None
    total = 0
    for R in (2000, 8 * 512, 3 * 512, 2 * 512):
        x = (torch.rand(R, 3, generator=g) * 2 - 1).cuda()
        t = torch.rand(R, 1, generator=g).cuda()
        cot = {k: torch.randn(R, WIDTH[k], generator=g).cuda() for k in _heads(cfg)}
        out = net(x, t)
        sum((out[k] * cot[k]).sum() for k in cot).backward()
        masks = _masks(net.stored_activations, cfg)
        _, g64 = NR.grads(p64, x.double(), t.double(), cfg, {k: v.double() for k, v in cot.items()}, masks=masks)
        want = g64 if want is None else OrderedDict((k, want[k] + g64[k]) for k in g64)
    for k, p in net.named_parameters():
        assert _rel(p.grad, want[k]) <= GRAD_TOL, k


def _fwd_bwd(net, x, t, cot):
    out = net(x, t)
    loss = sum((out[k] * cot[k]).sum() for k in cot)
    gs = torch.autograd.grad(loss, list(net.parameters()))
    return [out[k].detach() for k in cot] + [out["hidden"]] + list(gs)


@pytest.mark.parametrize("R", [512, 5000])
def test_no_host_sync_and_bitwise_repeatable(R):
    cfg, params, net = _shipped()
    net.keep_stored_activations = False
    g = torch.Generator().manual_seed(R)
    x, t = (torch.rand(R, 3, generator=g) * 2 - 1).cuda(), torch.rand(1, generator=g).cuda()
    cot = {k: torch.randn(R, WIDTH[k], generator=g).cuda() for k in _heads(cfg)}
    _fwd_bwd(net, x, t, cot)  # warm-up: library load, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):  # positive control: the mode is honoured by this build
            torch.zeros(1, device="cuda").item()
        a = _fwd_bwd(net, x, t, cot)
        b = _fwd_bwd(net, x, t, cot)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(a) == len(b) >= 30
    for u, v in zip(a, b):
        assert torch.equal(u, v) and bool(torch.isfinite(u).all())


def test_graph_capture_replays_the_eager_bits():
    cfg, params, net = _shipped()
    net.keep_stored_activations = False
    g = torch.Generator().manual_seed(3)
    R = 1024
    x, t = (torch.rand(R, 3, generator=g) * 2 - 1).cuda(), torch.rand(R, 1, generator=g).cuda()
    cot = {k: torch.randn(R, WIDTH[k], generator=g).cuda() for k in _heads(cfg)}
    eager = [v.clone() for v in _fwd_bwd(net, x, t, cot)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            _fwd_bwd(net, x, t, cot)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = _fwd_bwd(net, x, t, cot)
    for _ in range(2):
        for v in static:
            v.fill_(7.0) if v.is_floating_point() else None
        graph.replay()
        torch.cuda.synchronize()
        for u, v in zip(eager, static):
            assert torch.equal(u, v)


def test_chunked_rows_match_unchunked_halves():
    from riggs_amd import node_network as NN
    cfg, params, net = _shipped(W=64)
    net.keep_stored_activations = False
    g = torch.Generator().manual_seed(8)
    R = NN.MAX_ROWS + 4000
    x, t = (torch.rand(R, 3, generator=g) * 2 - 1).cuda(), torch.rand(R, 1, generator=g).cuda()
    cot = {k: torch.randn(R, WIDTH[k], generator=g).cuda() for k in _heads(cfg)}
    whole = _fwd_bwd(net, x, t, cot)
    h = NN.MAX_ROWS
    a = _fwd_bwd(net, x[:h], t[:h], {k: v[:h] for k, v in cot.items()})
    b = _fwd_bwd(net, x[h:], t[h:], {k: v[h:] for k, v in cot.items()})
    n_out = len(cot) + 1
    for i in range(n_out):  # the rows of a chunk do not depend on the other chunk: the same bits
        assert torch.equal(whole[i], torch.cat([a[i], b[i]], 0))
    for i in range(n_out, len(whole)):  # one float32 addition of the two chunks' gradients
        assert torch.equal(whole[i], a[i] + b[i]) or _rel(whole[i], a[i] + b[i]) <= 1e-6
    shared = net(x, torch.tensor(0.25, device="cuda"))
    assert shared["d_xyz"].shape == (R, 3) and shared["hidden"].shape == (R, 64)


def test_rejections():
    from riggs_amd import _lib as L
    from riggs_amd.node_network import DeformNetwork
    cfg, params, net = _shipped(W=64)
    x, t = torch.rand(10, 3, device="cuda"), torch.rand(10, 1, device="cuda")
    with pytest.raises(L.RiggsHipError):
        net(x.clone().requires_grad_(True), t)
    with pytest.raises(L.RiggsHipError):
        net(x, t.clone().requires_grad_(True))
    with pytest.raises(L.RiggsHipError):
        net(x.cpu(), t.cpu())
    with pytest.raises(L.RiggsHipError):
        net(torch.rand(10, 4, device="cuda"), t)
    with pytest.raises(L.RiggsHipError):
        net(x, torch.rand(7, 1, device="cuda"))
    with pytest.raises(L.RiggsHipError):
        net(x.double(), t)
    with pytest.raises(L.RiggsHipError):
        DeformNetwork(W=64)(x, t)  # parameters on the CPU: no eager path
    with pytest.raises(NotImplementedError):
        DeformNetwork(W=512)
    lib = L.lib()
    bad = L.NodeMlp()
    bad.width, bad.depth = 512, 8
    assert lib.riggs_node_mlp_forward(C.byref(bad), 10, x.data_ptr(), t.data_ptr(), 1, *([None] * 7)) != 0
    assert b"width" in lib.riggs_last_error()


def test_parameters_changed_in_place_between_calls():
    cfg, params, net = _shipped(W=64)
    g = torch.Generator().manual_seed(21)
    R = 700
    x, t = (torch.rand(R, 3, generator=g) * 2 - 1).cuda(), torch.rand(R, 1, generator=g).cuda()
    cot = {k: torch.randn(R, WIDTH[k], generator=g).cuda() for k in _heads(cfg)}
    opt = torch.optim.Adam(net.trainable_parameters()[0]["params"], lr=1e-2)

    def check(what):
        out, grads, st = _run_module(net, x, t, cot)
        p64 = OrderedDict((k, v.detach().double().clone()) for k, v in net.named_parameters())
        return _check_case(cfg, p64, x, t, cot, out, grads, st, what, record=False), out
    _, o1 = check("before the step")
    opt.step()  # .grad of the call above: every master changes in place
    _, o2 = check("after an optimizer step")
    assert _rel(o2["d_xyz"], o1["d_xyz"]) > 1e-3
    cfg2 = dict(cfg)
    new = NR.integer_params(cfg2)
    net.load_state_dict({k: (0.5 * v).float() for k, v in new.items()})
    _, o3 = check("after load_state_dict")
    assert _rel(o3["d_xyz"], o2["d_xyz"]) > 1e-3


# ----------------------------------------------------------------------------------------- one whole stage-1 iteration
class _Rec(torch.nn.Module):
    """Wraps a node network: records the time input, the inputs and the ReLU masks of every call; with ``replay`` (the calls of
    another run) the times are substituted in order and, for the torch restatement, the ReLU masks are pinned to the recorded
    ones."""

    def __init__(self, net, replay=None):
        super().__init__()
        self.net, self.replay, self.calls = net, replay, []

    def update(self, *a, **k):
        return

    def forward(self, x, t, **kwargs):
        if self.replay is not None:
            t = self.replay[len(self.calls)]["t"].reshape(t.shape)
            if isinstance(self.net, NR.RefNetwork):
                self.net.pin = self.replay[len(self.calls)]["masks"]
        out = self.net(x, t, **kwargs)
        if isinstance(self.net, NR.RefNetwork):
            last = self.net.last
            masks = {"act": torch.stack([z.detach() > 0 for z in last["pre"]]), "timenet": last["timenet_pre"].detach() > 0}
        else:
            st = self.net.stored_activations
            masks = {"act": st["act"] > 0, "timenet": st["timenet_hidden"] > 0}
        self.calls.append({"x": x.detach().clone(), "t": t.detach().clone(), "masks": masks})
        return out


def _stage1(M=512, N=6000, H=8):
    from riggs_amd import synth
    from riggs_amd.gaussian_model import GaussianModel
    sc = synth.make_scene(N, 8, 7)
    cam = synth.look_at_camera(96, 96, fid=0.4).to("cuda")
    gm = GaussianModel.from_tensors(sc["xyz"], sc["features_dc"], sc["features_rest"], sc["scaling"], sc["rotation"],
                                    sc["opacity"], device="cuda")
    gm.fea_dim, gm.with_motion_mask = H + 1, True
    g = torch.Generator().manual_seed(5)
    gm.feature = torch.nn.Parameter(torch.cat([0.02 * torch.randn(N, H, generator=g), 2.0 + torch.randn(N, 1, generator=g)], -1).cuda())
    sel = torch.randperm(N, generator=g)[:M].cuda()
    nodes = torch.cat([gm.get_xyz.detach()[sel], (1e-2 + 0.02 * torch.randn(M, H, generator=g)).cuda()], -1)
    weight = (0.3 * torch.randn(M, 1, generator=g)).cuda()
    cfg = NR.CONFIGS["a"]
    params = NR.integer_params(cfg)
    for k in params:  # heads at 1/32: deformations of a few percent of the scene
        if k.split(".")[0] in dict(NR.HEADS):
            params[k] = params[k] / 32
    return cfg, params, gm, cam, nodes, weight


def _stage1_warp(network, nodes, weight, M=512, H=8):
    from riggs_amd.control_nodes import ControlNodeWarp
    cn = ControlNodeWarp(node_num=M, K=3, local_frame=True, d_rot_as_res=True, hyper_dim=H, network=network, is_blender=True,
                         with_arap_loss=True).cuda()
    with torch.no_grad():
        cn.nodes.copy_(nodes)
        cn._node_radius.fill_(float(np.log(0.2)))
        cn._node_weight.copy_(weight)
    return cn


def _stage1_loss(cn, gm, cam, target, it, tt):
    """ControlNodeWarp.forward at an iteration where the ARAP schedule is on (node_deform + arap_loss), elastic_loss, acc_loss,
    render, L1 + SSIM: four calls of the node network."""
    from riggs_amd.graph import _Pipe
    from riggs_amd.loss import image_loss
    from riggs_amd.render import render
    dv = cn(gm.get_xyz.detach(), tt, gm.feature, gm.motion_mask, iteration=it)
    pkg = render(cam, gm, _Pipe, torch.zeros(3, device="cuda"), dv["d_xyz"], dv["d_rotation"], dv["d_scaling"], d_rot_as_res=True)
    loss, _ = image_loss(pkg["render"], target, 0.2)
    return loss + cn.reg_loss + 1e-3 * cn.elastic_loss(t=tt, delta_t=0.01) + 1e-5 * cn.acc_loss(t=tt, delta_t=0.03)


def test_whole_stage1_iteration_against_the_torch_restatement_and_thirty_steps():
    cfg, params, gm, cam, nodes, weight = _stage1()
    target = torch.rand(3, 96, 96, generator=torch.Generator().manual_seed(9)).cuda()
    tt = torch.tensor(0.4, device="cuda")
    native = _Rec(_module(cfg, params))
    cn = _stage1_warp(native, nodes, weight)
    torch.manual_seed(77)
    loss = _stage1_loss(cn, gm, cam, target, 3000, tt)
    assert torch.is_tensor(cn.reg_loss) and len(native.calls) == 4
    loss.backward()
    mine = OrderedDict((k, p.grad.clone()) for k, p in native.net.named_parameters())
    mine_nodes = {k: getattr(cn, k).grad.clone() for k in ("nodes", "_node_radius", "_node_weight")}

    ref = _Rec(NR.RefNetwork(cfg, OrderedDict((k, v.float().cuda()) for k, v in params.items())), replay=native.calls)
    cn2 = _stage1_warp(ref, nodes, weight)
    gm.feature.grad = None
    torch.manual_seed(77)
    loss2 = _stage1_loss(cn2, gm, cam, target, 3000, tt)
    loss2.backward()
    assert len(ref.calls) == 4
    assert abs(float(loss.detach()) - float(loss2.detach())) <= 1e-5 * abs(float(loss2.detach()))
    # the native run's ReLU masks against float64, call by call (the comparator ran with the masks pinned to the native run's, so
    # the two runs' masks agree everywhere and every gradient is compared)
    p64 = OrderedDict((k, v.double().cuda()) for k, v in params.items())
    units = differing = free_differing = 0
    for a, b in zip(native.calls, ref.calls):
        assert torch.equal(a["x"], b["x"]) and torch.equal(a["t"].reshape(-1), b["t"].reshape(-1))
        free_differing += int((a["masks"]["act"] != b["masks"]["act"]).sum()) + int((a["masks"]["timenet"] != b["masks"]["timenet"]).sum())
        u, d = _mask_check(p64, a["x"], a["t"].reshape(-1, 1).expand(a["x"].shape[0], 1), cfg, a["masks"])
        units, differing = units + u, differing + d
    print("stage-1 iteration: units", units, "native masks differing from float64", differing,
          "and from the fp32 restatement's own signs", free_differing)
    assert differing <= MASK_SHARE * units
    theirs = ref.net.named()
    for k, g in mine.items():
        e = _rel(g, theirs[k].grad)
        GU.STATS.append(("node_mlp stage-1 iteration grad %s" % k, int(g.numel()), 0.0, e, 0.0))
        assert e <= GRAD_TOL, (k, e)
    for k, g in mine_nodes.items():
        e = _rel(g, getattr(cn2, k).grad)
        assert e <= GRAD_TOL, (k, e)

    # thirty optimizer steps with the native network: finite, and the loss falls
    opt = torch.optim.Adam(cn.trainable_parameters(), lr=2e-4, eps=1e-15)
    losses = []
    for it in range(30):
        native.calls.clear()
        torch.manual_seed(1000)  # the same time samples every step: the sequence measures the optimisation alone
        opt.zero_grad()
        loss = _stage1_loss(cn, gm, cam, target, 3000 + it, tt)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = torch.stack(losses).cpu()
    print("stage-1 losses", losses[0].item(), losses[-1].item())
    assert bool(torch.isfinite(losses).all()) and float(losses[-1]) < float(losses[0])
    for p in cn.parameters():
        assert bool(torch.isfinite(p).all())
