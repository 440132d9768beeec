"""Fixtures of the hash-grid node network from the reference's HashDeformNetwork (imported through _ref_shim, never copied; CPU
only).  The reference's encoding is tinycudann.Encoding, which is not available: a ``tinycudann`` stub is registered whose
``Encoding`` is the NumPy oracle tests/hashgrid_ref.py (the published algorithm), and ``torch.cuda.device`` is replaced by a null
context in this process.  What is recorded is therefore the REFERENCE's module code (contraction, time embedding, band mask, trunk,
heads, state-dict names) around the oracle's encoding.

  hashgrid_net_{xyz,xyzt}.npz   hidden_dim = 64, hash_time off / on, local_frame and pred_opacity on, bbox (-1.3, 1.7):
                                inputs x, t; every trunk and head parameter; the constants (a, b, m, scale) of the closed-form
                                table (tests/hashgrid_ref.table_values — the 2^19-entry levels are not stored); the masks after
                                update(0), update(3000), update(3250) and update(7000); at step 3250 the float32 outputs, the
                                cotangents, the gradients of mlp.layers.0 and of the touched table entries (flat indices + values);
                                ``ref_fp32_out_dev`` / ``ref_fp32_grad_dev``: the float32 run against a float64 rerun on the same
                                encoding input (largest deviation over the tensor's largest magnitude)
  hashgrid_state_dict_layout.json   names and shapes of HashDeformNetwork(local_frame=True, pred_opacity=True).state_dict() with
                                hash_time off / on (default hidden_dim = 256)
"""
import contextlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_shim as S  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import hashgrid_ref as HR  # noqa: E402

OUT_KEYS = ["d_xyz", "d_rotation", "d_scaling", "d_opacity", "local_rotation"]
WIDTH = dict(d_xyz=3, d_rotation=4, d_scaling=3, d_opacity=1, local_rotation=4)
TABLE = dict(a=2654435761, b=12345, m=65521, scale=0.25)
BBOX = [-1.3, 1.7]
R = 64
CONFIG_KEYS = ("n_levels", "n_features_per_level", "log2_hashmap_size", "base_resolution", "per_level_scale")


class _OracleEncode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, params, enc):
        xs = x.detach().float().numpy() if enc.fixed_input is None else enc.fixed_input
        enc.last_input = xs
        ctx.enc, ctx.xs, ctx.dtype = enc, xs, params.dtype
        out = HR.encode(xs, params.detach().numpy(), enc.n_input_dims, enc.config)
        return torch.from_numpy(out).to(params.dtype)

    @staticmethod
    def backward(ctx, g):
        enc = ctx.enc
        _, g_table, _ = HR.encode(ctx.xs, np.zeros(enc.params.numel()), enc.n_input_dims, enc.config, g_out=g.double().numpy())
        return None, torch.from_numpy(g_table.reshape(-1)).to(ctx.dtype), None


class OracleEncoding(torch.nn.Module):
    """tinycudann.Encoding's surface as the reference uses it: ``params``, ``n_output_dims``, ``forward``."""

    def __init__(self, n_input_dims, encoding_config, dtype=torch.float32):
        super().__init__()
        self.n_input_dims = n_input_dims
        self.config = {k: encoding_config[k] for k in CONFIG_KEYS}
        levels, total = HR.level_table(n_input_dims, **self.config)
        self.n_output_dims = len(levels) * self.config["n_features_per_level"]
        self.params = torch.nn.Parameter(torch.zeros(total * self.config["n_features_per_level"], dtype=dtype))
        self.fixed_input, self.last_input = None, None      # (the float64 rerun encodes the float32 run's input: same bits)

    def forward(self, x):
        return _OracleEncode.apply(x, self.params, self)


def run(net, x, t, cot, dtype):
    net = net.to(dtype)
    net.zero_grad()
    to_float = torch.Tensor.float
    if dtype is torch.float64:        # (the reference casts the trunk's output with .float(): the float64 rerun stays float64)
        torch.Tensor.float = lambda self: self
    try:
        out = net(x.to(dtype), t.to(dtype))
    finally:
        torch.Tensor.float = to_float
    sum((out[k] * cot[k].to(dtype)).sum() for k in OUT_KEYS).backward()
    grads = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    return {k: out[k].detach().clone() for k in OUT_KEYS}, grads


def fixture(name, net, hash_time, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in net.named_parameters():
            if k == "hashgrid.encoding.params":
                p.copy_(torch.from_numpy(HR.table_values(p.numel(), TABLE["a"], TABLE["b"], TABLE["m"]) * np.float32(TABLE["scale"])))
            elif k.endswith(".bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
            elif k == "mlp.layers.%d.weight" % (len(net.mlp.layers) - 1):
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)     # (the reference draws it at 1e-5: every output would be its bias)
    x = (torch.rand(R, 3, generator=g) * 2.6 - 1.1).float()          # inside the box but for a few rows below and above it
    x[:4] = torch.tensor([[-1.3, -1.3, -1.3], [1.7, 1.7, 1.7], [-1.5, 0.2, 1.9], [0.2, 0.2, 0.2]])
    t = torch.rand(R, 1, generator=g).float()
    t[:8] = t[0]
    cot = {k: torch.randn(R, WIDTH[k], generator=g).float() for k in OUT_KEYS}
    z = dict(x=x.numpy(), t=t.numpy(), bbox=np.asarray(BBOX, dtype=np.float32),
             **{"table_" + k: np.float64(v) for k, v in TABLE.items()})
    for step in (0, 3000, 3250):
        net.update(step)
        z["mask_%d" % step] = net.hashgrid.mask.numpy().copy()
    sd32 = {k: v.detach().clone() for k, v in net.state_dict().items()}
    enc = net.hashgrid.encoding
    o32, g32 = run(net, x, t, cot, torch.float32)
    z["enc_input"] = enc.last_input.copy()
    enc.fixed_input = enc.last_input
    mask32 = net.hashgrid.mask
    net.hashgrid.mask = mask32.double()
    o64, g64 = run(net, x, t, cot, torch.float64)
    net.hashgrid.mask = mask32
    enc.fixed_input = None
    net.float()
    net.load_state_dict(sd32)
    dev = max(float((o32[k].double() - o64[k]).abs().max() / o64[k].abs().max()) for k in OUT_KEYS)
    gkeys = ["mlp.layers.0.weight", "mlp.layers.0.bias", "hashgrid.encoding.params"]
    gdev = max(float((g32[k].double() - g64[k]).abs().max() / g64[k].abs().max()) for k in gkeys)
    z["ref_fp32_out_dev"], z["ref_fp32_grad_dev"] = np.float64(dev), np.float64(gdev)
    for k in OUT_KEYS:
        z["cot/" + k] = cot[k].numpy()
        z["out/" + k] = o32[k].numpy()
    for k in gkeys[:2]:
        z["grad/" + k] = g32[k].numpy()
    gt = g32["hashgrid.encoding.params"].numpy()
    touched = np.flatnonzero(gt)
    z["grad_table_index"], z["grad_table_value"] = touched.astype(np.int32), gt[touched]
    z["grad_table_max"] = np.float64(np.abs(g64["hashgrid.encoding.params"].numpy()).max())
    for k, v in sd32.items():
        if k != "hashgrid.encoding.params":
            z["param/" + k] = v.numpy()
    net.update(7000)
    z["mask_7000"] = net.hashgrid.mask.numpy().copy()
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **z)
    print(name, "fp32 ref: out dev %.2e grad dev %.2e, %d table values touched" % (dev, gdev, touched.size))


def main():
    S.install()
    mod = types.ModuleType("tinycudann")
    mod.Encoding = OracleEncoding
    sys.modules["tinycudann"] = mod
    torch.cuda.device = lambda *a, **k: contextlib.nullcontext()
    with S.quiet():
        from utils.time_utils import HashDeformNetwork
    layout = {}
    for name, hash_time in (("xyz", False), ("xyzt", True)):
        torch.manual_seed(100)
        full = HashDeformNetwork(hash_time=hash_time, local_frame=True, pred_opacity=True)
        layout["hash_time" if hash_time else "no_hash_time"] = {k: list(v.shape) for k, v in full.state_dict().items()}
        del full
        torch.manual_seed(101)
        net = HashDeformNetwork(hidden_dim=64, hash_time=hash_time, local_frame=True, pred_opacity=True, bbox=BBOX)
        fixture("hashgrid_net_" + name, net, hash_time, 17 if hash_time else 16)
    with open(os.path.join(HERE, "hashgrid_state_dict_layout.json"), "w") as f:
        json.dump(layout, f, indent=1)


if __name__ == "__main__":
    main()
