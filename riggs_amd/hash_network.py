"""The stage-1 hash-grid node network with the reference's names (``HashDeformNetwork`` over ``ProgressiveBandHashGridCosine``,
utils/time_utils.py:517-571, 712-767; the flags ``use_hash`` / ``hash_time``) on the grid encoding of csrc/hashgrid.hip.

The reference takes its encoding from ``tinycudann.Encoding``, a CUDA-only extension.  ``HashGridEncoding`` is that encoding
("Grid" / "Hash" / linear interpolation, two features per level) restated from the published algorithm (Mueller et al., Instant
Neural Graphics Primitives, 2022; spelled out in include/riggs_hip.h, restated in NumPy in tests/hashgrid_ref.py).  tinycudann
was not available where this was written: agreement with its binary is NOT verified, and exchanging checkpoints with a reference
run rests on the parameter layout (names, shapes, level-major / entry-major / feature-minor table) and on the published algorithm.

One encoding call is one autograd node and one launch per direction.  The only gradient is the table's, a scatter of float atomic
adds: it can differ in its last bits from run to run.  Coordinates are not differentiated (every caller of the reference passes
detached positions; a coordinate tensor that requires a gradient raises, as in ``riggs_amd.node_network``).  The trunk and the
heads are ``nn.Linear`` in torch: they see the 512 node rows.  There is no CPU path: tensors that are not on the GPU are rejected.
Not supported: ``tcnn_mlp=True`` (tinycudann's fused MLP) raises ``NotImplementedError``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
from torch import nn

from . import _lib as L

_HEAD, _LW, _WORDS = (L.CONSTANTS["RIGGS_HASHGRID_" + k] for k in ("HEADER_WORDS", "LEVEL_WORDS", "TABLE_WORDS"))


class HashGridLevels:
    """The per-level table of a configuration as the C ABI takes it (include/riggs_hip.h: RIGGS_HASHGRID_TABLE_WORDS host words in
    ``words``, filled by ``riggs_hashgrid_levels_fill``) and, read back from those words, as Python lists: ``scale`` (the float32
    values), ``resolution``, ``size``, ``offset`` (n_levels + 1 entries, the last one the whole table's) and ``hashed``."""

    def __init__(self, n_input_dims, n_levels, n_features_per_level, log2_hashmap_size, base_resolution, per_level_scale):
        self.words = (C.c_uint32 * _WORDS)()
        L.check(L.lib().riggs_hashgrid_levels_fill(int(n_input_dims), int(n_levels), int(n_features_per_level), int(log2_hashmap_size),
                                                   float(base_resolution), float(per_level_scale), self.words), "riggs_hashgrid_levels_fill")
        w = self.words
        self.n_input_dims, self.n_levels, self.n_features_per_level, self.log2_hashmap_size = int(w[0]), int(w[1]), int(w[2]), int(w[3])
        at = [_HEAD + _LW * l for l in range(self.n_levels)]
        self.scale = [C.c_float.from_buffer_copy(C.c_uint32(w[a])).value for a in at]
        self.resolution, self.size = [int(w[a + 1]) for a in at], [int(w[a + 2]) for a in at]
        self.offset, self.hashed = [int(w[a + 3]) for a in at] + [int(w[4])], [bool(w[a + 4]) for a in at]
DEFAULT_CONFIG = {"otype": "Grid", "type": "Hash", "n_levels": 12, "n_features_per_level": 2, "log2_hashmap_size": 19,
                  "base_resolution": 16, "per_level_scale": 2.0, "interpolation": "Linear"}


def hashgrid_levels(n_input_dims, config=None):
    """The per-level table (``HashGridLevels``: scale, resolution, size, offset, hashed) of a configuration, filled by the
    library's host function.  Keys of ``config`` default to the reference's (DEFAULT_CONFIG)."""
    cfg = dict(DEFAULT_CONFIG)
    cfg.update(config or {})
    if cfg.get("otype", "Grid") not in ("Grid", "HashGrid") or cfg.get("type", "Hash") != "Hash":
        raise NotImplementedError("the grid encoding supports otype 'Grid' with type 'Hash' only")
    if cfg.get("interpolation", "Linear") != "Linear":
        raise NotImplementedError("the grid encoding supports linear interpolation only")
    return HashGridLevels(n_input_dims, cfg["n_levels"], cfg["n_features_per_level"], cfg["log2_hashmap_size"], cfg["base_resolution"],
                          cfg["per_level_scale"])


class _HashGrid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, levels, x, params, mask):
        R = x.shape[0]
        out = torch.empty(R, 2 * levels.n_levels, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            L.check(L.lib().riggs_hashgrid_forward(levels.words, R, x.data_ptr(), params.data_ptr(), L.ptr(mask), out.data_ptr(),
                                                   L.stream_ptr()), "riggs_hashgrid_forward")
        ctx.levels, ctx.R = levels, R
        ctx.save_for_backward(x, mask)
        ctx.shape = params.shape
        return out

    @staticmethod
    def backward(ctx, g):
        x, mask = ctx.saved_tensors
        g = L.require_cuda_f32("cotangent", g, (ctx.R, 2 * ctx.levels.n_levels))
        g_table = torch.zeros(ctx.shape, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            L.check(L.lib().riggs_hashgrid_backward(ctx.levels.words, ctx.R, x.data_ptr(), L.ptr(mask), g.data_ptr(),
                                                    g_table.data_ptr(), L.stream_ptr()), "riggs_hashgrid_backward")
        return None, None, g_table, None


class HashGridEncoding(nn.Module):
    """``tinycudann.Encoding(n_input_dims, config)`` for the grid encoding: ``.params`` is the flat float32 table
    (``F * sum size_l`` values: level-major, entry-major, feature-minor; uniform in [-1e-4, 1e-4]), ``.n_output_dims = L F``.
    ``forward(x, mask=None)``: x (R, D) float32 on the device, taken as it comes (no clamp) -> (R, L F); ``mask`` (L F floats)
    multiplies the output, and the cotangent in the backward, inside the kernels."""

    def __init__(self, n_input_dims, config=None, device="cuda"):
        super().__init__()
        self.levels = hashgrid_levels(n_input_dims, config)
        self.n_input_dims, self.n_levels = int(n_input_dims), int(self.levels.n_levels)
        self.n_features_per_level = 2
        self.n_output_dims = self.n_levels * self.n_features_per_level
        self.n_entries = int(self.levels.offset[self.n_levels])
        self.params = nn.Parameter(torch.empty(self.n_entries * self.n_features_per_level, dtype=torch.float32,
                                               device=device).uniform_(-1e-4, 1e-4))

    def level_table(self):
        """[(scale, resolution, size, offset, hashed)] per level, as Python numbers."""
        lv = self.levels
        return [(lv.scale[l], lv.resolution[l], lv.size[l], lv.offset[l], lv.hashed[l]) for l in range(self.n_levels)]

    def forward(self, x, mask=None):
        if not torch.is_tensor(x):
            raise L.RiggsHipError("the grid encoding takes a tensor")
        if x.requires_grad:
            raise L.RiggsHipError("the grid encoding does not differentiate its coordinates: pass x detached")
        if x.dim() != 2 or x.shape[1] != self.n_input_dims:
            raise L.RiggsHipError("x must be (R, %d), got %s" % (self.n_input_dims, tuple(x.shape)))
        x = L.require_cuda_f32("x", x)
        p = self.params
        if not (p.is_cuda and p.dtype is torch.float32 and p.is_contiguous() and p.numel() == 2 * self.n_entries):
            raise L.RiggsHipError("the grid encoding's table must be a contiguous float32 CUDA(HIP) tensor of %d values" % (2 * self.n_entries))
        if x.shape[0] * self.n_output_dims >= 2 ** 31:
            raise L.RiggsHipError("the grid encoding takes fewer than 2^31 / %d rows per call" % self.n_output_dims)
        if mask is not None:
            mask = L.require_cuda_f32("mask", mask.detach(), (self.n_output_dims,))
        return _HashGrid.apply(self.levels, x, p, mask)


class ProgressiveBandHashGridCosine(nn.Module):
    """time_utils.py:517-571: the grid encoding under a band mask that opens the levels from ``start_level`` upward, one cosine
    ramp per output column, over ``(n_levels - start_level) * update_steps`` steps.  ``update_step`` is the reference's rule
    evaluated on the device: a step older than ``current_step`` changes nothing, and nothing is read back to decide that."""

    def __init__(self, in_channels, start_level=6, n_levels=12, start_step=1000, update_steps=1000, dtype=torch.float32, device="cuda"):
        super().__init__()
        if dtype is not torch.float32:
            raise NotImplementedError("the grid encoding is float32")
        config = dict(DEFAULT_CONFIG, n_levels=n_levels)
        self.n_input_dims = in_channels
        self.encoding = HashGridEncoding(in_channels, config, device=device)
        self.n_output_dims = self.encoding.n_output_dims
        self.n_level, self.n_features_per_level = n_levels, config["n_features_per_level"]
        self.start_level, self.start_step, self.update_steps = start_level, start_step, update_steps
        self.register_buffer("current_step", torch.tensor(0, dtype=torch.int32, device=device))
        self.n_masking_step = (n_levels - start_level) * update_steps
        self.mask = torch.ones(self.n_output_dims, dtype=torch.float32, device=device)
        self.update_step(0)

    def forward(self, x):
        if self.mask.device != self.encoding.params.device:
            self.mask = self.mask.to(self.encoding.params.device)
        return self.encoding(x, self.mask)

    def update_step(self, global_step):
        if global_step is None or global_step < 0 or self.n_masking_step <= 0:
            return      # (n_masking_step <= 0: the mask is all ones and stays so)
        dev = self.current_step.device
        if self.mask.device != dev:
            self.mask = self.mask.to(dev)
        stale = self.current_step > global_step                       # the reference's early return, as a device flag
        ratio = global_step / self.n_masking_step
        start_idx = self.start_level * self.n_features_per_level
        band_len = self.n_output_dims - start_idx
        band = (1.0 - torch.cos(torch.pi * (ratio * band_len - torch.arange(0, band_len, device=dev)).clamp(0, 1))) / 2.0
        mask = self.mask.clone()
        mask[start_idx:] = torch.where(stale, mask[start_idx:], band)
        self.mask = mask
        self.current_step.data = torch.clamp(self.current_step, min=int(global_step))


class _MLP(nn.Module):
    """The reference's ``MLP`` (time_utils.py:648-684) as far as its state dict and arithmetic go: ``layers`` alternates Linear and
    ReLU, ``n_hidden_layers`` hidden Linear layers of ``n_neurons`` and an output Linear; the hidden layer behind a listed skip
    takes ``cat([h, x])``.  He-uniform weights (fan in, ReLU gain), zero biases."""

    def __init__(self, dim_in, dim_out, n_neurons, n_hidden_layers=1, skip=()):
        super().__init__()
        self.n_neurons, self.n_hidden_layers, self.skip = n_neurons, n_hidden_layers, list(skip)
        widths = [dim_in] + [n_neurons + dim_in if i in self.skip else n_neurons for i in range(n_hidden_layers - 1)]
        self.skip_idx = [2 * (i + 1) for i in range(n_hidden_layers - 1) if i in self.skip]
        mods = []
        for w in widths:
            mods += [self._linear(w, n_neurons), nn.ReLU(inplace=True)]
        mods.append(self._linear(n_neurons, dim_out))
        self.layers = nn.ModuleList(mods)

    @staticmethod
    def _linear(dim_in, dim_out):
        layer = nn.Linear(dim_in, dim_out)
        nn.init.kaiming_uniform_(layer.weight, mode="fan_in", nonlinearity="relu")
        nn.init.zeros_(layer.bias)
        return layer

    def forward(self, x):
        h = x
        for i, layer in enumerate(self.layers):
            if i in self.skip_idx:
                h = torch.cat([h, x], dim=-1)
            h = layer(h)
        return h


def _embed_time(t, multires):
    """get_embedder(multires, 1) of the reference: [t, sin(t), cos(t), sin(2 t), cos(2 t), ..., sin(2^(m-1) t), cos(2^(m-1) t)]."""
    parts = [t]
    for k in range(multires):
        tf = t * float(2 ** k)
        parts += [torch.sin(tf), torch.cos(tf)]
    return torch.cat(parts, -1)


class HashDeformNetwork(nn.Module):
    """The reference's ``HashDeformNetwork``: constructor keywords, parameter and buffer names, initialisers and the returned
    dict.  x (R, 3), t (R, 1), both detached, on the device."""

    def __init__(self, num_layers=2, hidden_dim=256, hash_time=False, tcnn_mlp=False, t_multires=6, bbox=None, scale_range=2.,
                 local_frame=False, pred_opacity=False, pred_color=False, device="cuda"):
        super().__init__()
        if tcnn_mlp:
            raise NotImplementedError("tcnn_mlp: tinycudann's fused MLP is not part of this library; the trunk is nn.Linear")
        self.hash_time, self.tcnn_mlp = hash_time, False
        self.register_buffer("bbox", torch.tensor([-2, 2] if bbox is None else bbox).float().to(device))
        self.hashgrid = ProgressiveBandHashGridCosine(in_channels=4 if hash_time else 3, start_level=6, n_levels=12, start_step=1000,
                                                      update_steps=1000, device=device)
        n_enc = self.hashgrid.n_output_dims
        if not hash_time:
            self.t_multires, self.time_embed_dim = t_multires, 1 + 2 * t_multires
        self.mlp = _MLP(dim_in=n_enc if hash_time else n_enc + self.time_embed_dim, dim_out=hidden_dim, n_neurons=hidden_dim,
                        n_hidden_layers=num_layers if hash_time else num_layers + 2, skip=[] if hash_time else [2])
        self.translate_layer = _MLP(hidden_dim, 3, 64)
        self.rotation_layer = _MLP(hidden_dim, 4, 64)
        self.scaling_layer = _MLP(hidden_dim, 3, 64)
        self.log_scale_range = np.log(scale_range)
        self.register_buffer("_identity_rotation", torch.tensor([1., 0, 0, 0]), persistent=False)    # (not in the state dict)
        if not hash_time:
            nn.init.normal_(self.mlp.layers[-1].weight, mean=0., std=1e-5)
        self.local_frame, self.pred_opacity, self.pred_color = local_frame, pred_opacity, pred_color
        if local_frame:
            self.local_rotation_layer = _MLP(hidden_dim, 4, 64)
        if pred_opacity:
            self.opacity_layer = _MLP(hidden_dim, 1, 64)
        if pred_color:
            self.color_layer = _MLP(hidden_dim, 3, 64)
        self.to(device)

    def contract(self, x):
        """contract_to_unisphere(x, bbox, unbounded=False): ``(x - b0) / (b1 - b0)``, the reference's torch operations in its
        order (its trailing ``* 1 + 0`` changes no value the encoding can tell apart), so the encoding's input has the same bits
        wherever torch evaluates it."""
        return (x - self.bbox[0]) / (self.bbox[1] - self.bbox[0])

    def forward(self, x, t, **kwargs):
        if not (torch.is_tensor(x) and torch.is_tensor(t)):
            raise L.RiggsHipError("x and t must be tensors")
        if x.requires_grad or t.requires_grad:
            raise L.RiggsHipError("the node network does not differentiate its inputs: pass x and t detached")
        if not (x.is_cuda and t.is_cuda):
            raise L.RiggsHipError("x and t must be CUDA(HIP) tensors — the product path is GPU-only")
        x = self.contract(x)
        if self.hash_time:
            embed = self.hashgrid(torch.cat([x, t], dim=-1))
        else:
            x_embed = self.hashgrid(x)
            t_embed = _embed_time(t, self.t_multires)
            t_embed = t_embed / self.time_embed_dim * self.hashgrid.n_output_dims      # "align the scale"
            embed = torch.cat([x_embed, t_embed], dim=-1)
        hidden = self.mlp(embed).float()
        translate = self.translate_layer(hidden)
        rotation = self.rotation_layer(hidden) + self._identity_rotation
        scaling = torch.tanh(self.scaling_layer(hidden)) * self.log_scale_range
        ret = {"d_xyz": translate, "d_rotation": rotation, "d_scaling": scaling,
               "d_opacity": self.opacity_layer(hidden) if self.pred_opacity else None,
               "d_color": self.color_layer(hidden) if self.pred_color else None}
        if self.local_frame:
            ret["local_rotation"] = self.local_rotation_layer(hidden)
        return ret

    def update(self, global_step, *args, **kwargs):
        self.hashgrid.update_step(global_step=global_step)
