"""A torch restatement of the stage-1 node network, written from its description (not from the reference's source), and the
exact integer weight formula of the W = 256 fixtures.

  x_emb = [x, sin(2^k x), cos(2^k x)]_{k=0..9}                       (63 columns)
  t_emb = timenet([t, sin(2^k t), cos(2^k t)]_{k=0..5})              (13 -> 256 -> ReLU -> 30)   with is_blender
        = [t, sin(2^k t), cos(2^k t)]_{k=0..9}                       (21 columns)                otherwise
  h = [x_emb, t_emb]; for l in 0..7: h = relu(linear[l](h)); after l = 4: h = [x_emb, t_emb, h]
  heads on h: gaussian_warp 3, gaussian_scaling 3 (max_d_scale > 0: tanh(.) * log(max_d_scale)), gaussian_rotation 4,
              local_rotation 4 (local_frame), gaussian_opacity 1 (pred_opacity)

dtype-generic (it runs in the dtype of its parameters); ``masks`` replaces every ReLU by a multiplication with the given 0/1 mask
(``{"timenet": (R, 256), "act": (8, R, W)}``), which pins the ReLU decisions of another evaluation.
"""
import math
from collections import OrderedDict

import torch

HEADS = (("gaussian_warp", 3), ("gaussian_scaling", 3), ("gaussian_rotation", 4), ("local_rotation", 4), ("gaussian_opacity", 1))
CONFIGS = {
    "a": dict(W=256, is_blender=True, local_frame=True, pred_opacity=False, max_d_scale=-1),
    "b": dict(W=256, is_blender=False, local_frame=True, pred_opacity=False, max_d_scale=-1),
    "c": dict(W=256, is_blender=True, local_frame=False, pred_opacity=True, max_d_scale=2),
    "w64": dict(W=64, is_blender=False, local_frame=True, pred_opacity=True, max_d_scale=-1),
}


def in_ch(cfg):
    return 63 + (30 if cfg["is_blender"] else 21)


def param_shapes(cfg):
    """name -> shape, the reference's names in the reference's order."""
    W, n_in = cfg["W"], in_ch(cfg)
    s = OrderedDict()
    if cfg["is_blender"]:
        s["timenet.0.weight"], s["timenet.0.bias"] = (256, 13), (256,)
        s["timenet.2.weight"], s["timenet.2.bias"] = (30, 256), (30,)
    for l in range(8):
        k = n_in if l == 0 else (W + n_in if l == 5 else W)
        s["linear.%d.weight" % l], s["linear.%d.bias" % l] = (W, k), (W,)
    for name, n in HEADS:
        if (name == "local_rotation" and not cfg["local_frame"]) or (name == "gaussian_opacity" and not cfg["pred_opacity"]):
            continue
        s[name + ".weight"], s[name + ".bias"] = (n, W), (n,)
    return s


def integer_params(cfg, dtype=torch.float64):
    """Parameters from an exact integer formula of (tensor index, row, column): n / 1024 * 2^-e with |n| <= 1023, the same bits in
    every float format and on every machine.  e follows the fan-in (roughly the kaiming bound)."""
    out = OrderedDict()
    for idx, (name, shape) in enumerate(param_shapes(cfg).items()):
        rows = torch.arange(shape[0], dtype=torch.int64)[:, None]
        cols = torch.arange(shape[1] if len(shape) == 2 else 1, dtype=torch.int64)[None, :]
        n = ((idx + 1) * 1000003 + rows * 7919 + cols * 104729 + ((rows + 3) * (cols + 5)) % 8191 * 31) % 2047 - 1023
        if len(shape) == 2:
            e = 1 if shape[1] <= 16 else (2 if shape[1] <= 128 else 3)
            if name.split(".")[0] in dict(HEADS):
                e += 1
        else:
            e = 4
        v = n.to(torch.float64) / 1024.0 * 2.0 ** -e
        out[name] = v.reshape(shape).to(dtype)
    return out


def embed(v, n_freq):
    cols = [v]
    for k in range(n_freq):
        cols += [torch.sin(v * 2.0 ** k), torch.cos(v * 2.0 ** k)]
    return torch.cat(cols, -1)


def forward(params, x, t, cfg, masks=None):
    """params: name -> tensor.  x (R, 3), t (R, 1) or broadcastable.  Returns the network's dict plus ``pre`` (the eight
    pre-activations, a list), ``act`` (the eight post-ReLU activations) and ``timenet_pre`` (or None)."""
    dt = params["linear.0.weight"].dtype
    x = x.to(dt)
    t = t.to(dt).reshape(-1, 1).expand(x.shape[0], 1)
    lin = lambda name, h: h @ params[name + ".weight"].t() + params[name + ".bias"]  # noqa: E731
    x_emb = embed(x, 10)
    tn_pre = None
    if cfg["is_blender"]:
        tn_pre = lin("timenet.0", embed(t, 6))
        hid = tn_pre * masks["timenet"].to(dt) if masks is not None else torch.relu(tn_pre)
        t_emb = lin("timenet.2", hid)
    else:
        t_emb = embed(t, 10)
    inp = torch.cat([x_emb, t_emb], -1)
    h, pre, act = inp, [], []
    for l in range(8):
        z = lin("linear.%d" % l, h)
        pre.append(z)
        a = z * masks["act"][l].to(dt) if masks is not None else torch.relu(z)
        act.append(a)
        h = torch.cat([inp, a], -1) if l == 4 else a
    d_scaling = lin("gaussian_scaling", h)
    if cfg["max_d_scale"] > 0:
        d_scaling = torch.tanh(d_scaling) * math.log(cfg["max_d_scale"])
    out = {"d_xyz": lin("gaussian_warp", h), "d_rotation": lin("gaussian_rotation", h), "d_scaling": d_scaling, "hidden": h,
           "d_opacity": lin("gaussian_opacity", h) if cfg["pred_opacity"] else None, "d_color": None}
    if cfg["local_frame"]:
        out["local_rotation"] = lin("local_rotation", h)
    out.update(pre=pre, act=act, timenet_pre=tn_pre, inp=inp)
    return out


OUT_KEYS = ("d_xyz", "d_scaling", "d_rotation", "local_rotation", "d_opacity")


def loss_of(out, cot):
    """sum over the outputs of <output, cotangent>: its gradient is the vector-Jacobian product the fixtures store."""
    s = 0
    for k in OUT_KEYS:
        if out.get(k) is not None and k in cot:
            s = s + (out[k] * cot[k].to(out[k].dtype)).sum()
    return s


def grads(params, x, t, cfg, cot, masks=None):
    ps = OrderedDict((k, v.detach().clone().requires_grad_(True)) for k, v in params.items())
    out = forward(ps, x, t, cfg, masks)
    g = torch.autograd.grad(loss_of(out, cot), list(ps.values()), allow_unused=True)
    return out, OrderedDict((k, (gi if gi is not None else torch.zeros_like(p))) for (k, p), gi in zip(ps.items(), g))


class RefNetwork(torch.nn.Module):
    """The restatement as a module (fp32 comparator of the timing tool and the stage-1 iteration test): same parameter names."""

    def __init__(self, cfg, params):
        super().__init__()
        self.cfg = dict(cfg)
        self.name, self.reg_loss = "mlp", 0.
        self.keys = list(params.keys())
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(v.detach().clone()) for v in params.values()])
        self.last = None
        self.pin = None   # ReLU masks for the next calls (see forward(masks=)), or None

    def named(self):
        return OrderedDict(zip(self.keys, self.ps))

    def update(self, *a, **k):
        return

    def forward(self, x, t, **kwargs):
        out = forward(self.named(), x, t, self.cfg, masks=self.pin)
        self.last = out
        return {k: v for k, v in out.items() if k not in ("pre", "act", "timenet_pre", "inp")}
