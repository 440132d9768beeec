"""-m gpu: the image loss (csrc/loss.hip) and the evaluation report (csrc/metrics.hip) — the two users of csrc/ssim_window.h — pinned
per pixel / per workgroup to float64 (tests/ssim_window_ref.py), stage by stage, through the C ABI so that ``state`` and the
workspace are the test's own buffers.  Loss: the three derivative maps, the per-workgroup partials, ``out3`` from the kernel's own
partials and end to end, ``dL/dimage`` from the kernel's own maps and end to end, the backward's options one by one.  Metrics: the
pools bit for bit, every level's per-workgroup partials, ``levels`` / ``out`` from the kernel's own partials.  Inputs sit in front
of NaN tails, outputs in front of sentinel tails; ``state`` and the workspace are NaN-filled at exactly the size the library
states."""
import numpy as np
import pytest
import torch

from riggs_amd import _lib as L
from tests import gpu_util as GU
from tests import ssim_window_ref as S
from tests.gpu_util import SENT, TAIL, in_buf, out_buf, tail_intact

pytestmark = pytest.mark.gpu

GRID = S.grid()
OPTION_SHAPES = (((3, 65, 33), "noisy"), ((1, 11, 38), "dark"))
WORST, VAC, STRUCT = {}, {}, {}     # case -> {array: worst err / bound}, {array: vacuity share}, worst bound / (k magnitude)


def _nan_front(n):
    buf = torch.full((n + TAIL,), SENT, dtype=torch.float32, device="cuda")
    buf[:n] = float("nan")
    return buf[:n], buf


def _dev(a):
    """A flat device copy in front of a NaN tail (the buffer is returned to keep it alive)."""
    return in_buf(torch.from_numpy(np.ascontiguousarray(a, np.float32).ravel()))


def _scalar(v):
    return None if v is None else torch.tensor([float(np.float32(v))], dtype=torch.float32, device="cuda")


class Loss:
    def __init__(self, x, y):
        self.x, self.y = x, y
        self.shape = x.shape
        (self.xd, self._xb), (self.yd, self._yb) = _dev(x), _dev(y)

    def forward(self, lam):
        C, H, W = self.shape
        lib = L.lib()
        n = int(lib.riggs_l1_ssim_state_floats(C, H, W))
        assert n == S.state_floats(C, H, W)
        state, stateb = _nan_front(n)
        out3, out3b = out_buf((3,))
        L.check(lib.riggs_l1_ssim_forward(C, H, W, self.xd.data_ptr(), self.yd.data_ptr(), float(lam), state.data_ptr(), out3.data_ptr(),
                                          L.stream_ptr()), "riggs_l1_ssim_forward")
        torch.cuda.synchronize()
        assert tail_intact(stateb, n) and tail_intact(out3b, 3), "the tail of state / out3 was written"
        return state, out3.cpu().numpy()

    def backward(self, state, lam, g):
        C, H, W = self.shape
        n = C * H * W
        dx, dxb = out_buf((n,))
        gs = [_scalar(v) for v in g]
        L.check(L.lib().riggs_l1_ssim_backward(C, H, W, self.xd.data_ptr(), self.yd.data_ptr(), state.data_ptr(), float(lam), L.ptr(gs[0]),
                                               L.ptr(gs[1]), L.ptr(gs[2]), dx.data_ptr(), L.stream_ptr()), "riggs_l1_ssim_backward")
        torch.cuda.synchronize()
        assert tail_intact(dxb, n), "the tail of dL/dimage was written"
        return dx.cpu().numpy().reshape(C, H, W)


def _record(tag, res, what):
    WORST[tag] = {k: v["worst"] for k, v in res.items() if isinstance(v, dict)}
    VAC[tag] = {k: v["vac"] for k, v in res.items() if isinstance(v, dict)}
    if "structural" in res:
        STRUCT[tag] = res["structural"]
    for k, v in res.items():
        if isinstance(v, dict):
            GU.STATS.append(("%s %s %s [err/bound]" % (what, k, tag), v["n"], v["bad"] / max(1, v["n"]), v["worst"], v["bad"] / max(1, v["n"])))
    print(tag, {k: (round(v["worst"], 4), round(v["vac"], 5)) for k, v in res.items() if isinstance(v, dict)})
    bad = {k: (res[k]["bad"], res[k]["worst"], res[k]["first"]) if k != "nan_free" else "NaN left in state" for k in S.bad_arrays(res)}
    assert not bad, "%s: elements outside the bound (count, worst err/bound, first index): %r" % (tag, bad)


@pytest.mark.parametrize("case", GRID, ids=[c["name"] for c in GRID])
def test_loss_grid_against_float64(case):
    x, y = S.make_images(case["shape"], case["family"])
    k = Loss(x, y)
    state, out3 = k.forward(case["lam"])
    dx = k.backward(state, case["lam"], case["g"])
    res = S.check_loss(case, x, y, state.cpu().numpy(), out3, dx)
    _record(case["name"], res, "loss")
    assert res["nan_free"]
    if case["family"] == "identical":
        assert res["dx_zero"]["bad"] == 0


@pytest.mark.parametrize("shape,family", OPTION_SHAPES)
def test_backward_options_one_by_one(shape, family):
    x, y = S.make_images(shape, family)
    k = Loss(x, y)
    ref = S.loss_reference(x, y)
    for lam in S.LAMBDAS:
        state, out3 = k.forward(lam)
        st = state.cpu().numpy()
        for i, g in enumerate(S.G_OPTIONS):
            dx = k.backward(state, lam, g)
            case = {"name": "%dx%dx%d %s option %d lambda %g" % (shape + (family, i, lam)), "shape": shape, "family": family, "lam": lam, "g": g}
            _record(case["name"], S.check_loss(case, x, y, st, out3, dx, ref=ref), "loss")
            if i == 0:
                assert not dx.any(), "every upstream gradient NULL: dx is exactly 0"
        a, b = k.backward(state, lam, (None, None, 1.3)), k.backward(state, lam, S.split_route(lam, 1.3))
        assert S.routes_agree(x, y, st, lam, 1.3, a, b), "the g_loss route against the g_l1 / g_ssim route, lambda %g" % lam
    same = Loss(x, x.copy())
    state, out3 = same.forward(0.2)
    assert not same.backward(state, 0.2, (0.7, None, None)).any(), "x == y and g_l1 alone: sign(0) = 0"
    assert out3[0] == 0.0


@pytest.mark.parametrize("shape,family", [((2, 130, 70), "noisy"), ((3, 65, 33), "flat")])
def test_equal_bits_and_an_untouched_state(shape, family):
    x, y = S.make_images(shape, family)
    k = Loss(x, y)
    s1, o1 = k.forward(0.2)
    s2, o2 = k.forward(0.2)
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32)) and np.array_equal(o1.view(np.uint32), o2.view(np.uint32))
    keep = s1.clone()
    a = k.backward(s1, 0.2, S.G_OPTIONS[7])
    b = k.backward(s1, 0.2, S.G_OPTIONS[7])
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert torch.equal(s1.view(torch.int32), keep.view(torch.int32)), "the backward wrote into state"


# ---- the evaluation report -------------------------------------------------------------------------------------------------------
def run_metrics(x, y, clamp, want_ms):
    B, C, H, W = x.shape
    lib = L.lib()
    n = int(lib.riggs_image_metrics_workspace_floats(B, C, H, W))
    p = S.plan(B, C, H, W)
    assert n == p["total_floats"]
    (xd, _xb), (yd, _yb) = _dev(x), _dev(y)
    ws, wsb = _nan_front(n)
    out, outb = out_buf((B, 4))
    levels, levelsb = out_buf((B * 6 * C * 2,))
    L.check(lib.riggs_image_metrics(B, C, H, W, xd.data_ptr(), yd.data_ptr(), int(clamp), int(want_ms), out.data_ptr(), levels.data_ptr(),
                                    ws.data_ptr(), n, L.stream_ptr()), "riggs_image_metrics")
    torch.cuda.synchronize()
    assert tail_intact(wsb, n) and tail_intact(outb, B) and tail_intact(levelsb, B * 6 * C * 2), "a tail was written"
    w = ws.cpu().numpy()
    if bool(want_ms) == bool(p["ms"]):   # (the pyramid is planned whenever the image admits it, wanted or not)
        assert not np.isnan(w[2 * p["doubles"]:]).any(), "a part of the stated workspace was not written"   # (the images; the partials below)
    got = S.split_workspace(w, B, C, H, W, want_ms)
    assert not np.isnan(got["partial"]).any()
    got["out"], got["levels"] = out.cpu().numpy(), levels.cpu().numpy().reshape(B, 6, C, 2)
    return got


@pytest.mark.parametrize("name,shape,family,ms", S.METRICS_CASES, ids=[c[0] for c in S.METRICS_CASES])
def test_metrics_pools_partials_and_means(name, shape, family, ms):
    x, y = S.metrics_inputs(shape, family)
    got = run_metrics(x, y, 0, ms)
    _record("metrics " + name, S.check_metrics(x, y, False, ms, got), "metrics")


@pytest.mark.parametrize("shape,ms", [((1, 75, 43), False), ((3, 161, 161), True), ((1, 385, 385), True)])
def test_metrics_clamp_on_load_equals_clamped_inputs_in_every_partial(shape, ms):
    x, y = S.metrics_inputs(shape, "noisy")
    x, y = np.float32(x * 1.4 - 0.2), np.float32(y * 1.4 - 0.2)
    assert x.min() < 0 and x.max() > 1
    a = run_metrics(x, y, 1, ms)
    b = run_metrics(np.clip(x, 0, 1), np.clip(y, 0, 1), 0, ms)
    assert np.array_equal(a["partial"].view(np.uint64), b["partial"].view(np.uint64))
    for l in a["img"]:
        assert np.array_equal(a["img"][l].view(np.uint32), b["img"][l].view(np.uint32)), l
    _record("metrics clamp %dx%dx%d" % shape, S.check_metrics(x, y, True, ms, a), "metrics")
