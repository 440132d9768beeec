"""The stage-1 node network with the reference's names (``DeformNetwork``, utils/time_utils.py:310-458) over the fp32 MFMA kernels
of csrc/node_mlp.hip: positional embedding, time net, 8-layer trunk with one skip, output heads.

One call is ONE autograd node and three launches (forward; backward data chain; backward parameters).  The parameters keep the
reference's names, shapes and initialisers, so ``state_dict()`` / ``load_state_dict()`` exchange checkpoints with the reference in
both directions, alone (the ``'mlp'`` deform type) and as ``ControlNodeWarp.network`` (keys ``network.*``).  The kernels read the
fp32 masters in place on every call: an optimizer step or a ``load_state_dict`` between two calls cannot leave a stale copy.

Not differentiated: ``x`` and ``t`` (every caller of the reference passes detached positions and a time without a graph; an input
that requires a gradient raises).  ``hidden`` is returned non-differentiable: no caller in the reference reads it.
Not supported (``NotImplementedError`` at construction): ``pred_color`` in any form and ``progressive_brand_time`` — pass the
reference's module as ``network=`` for those.  There is no CPU / eager path: tensors that are not on the GPU are rejected.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn

from . import _lib as L

MAX_ROWS = 65536            # rows per C call; longer inputs are split into chunks of rows in ascending order
_HEADS = ("gaussian_warp", "gaussian_scaling", "gaussian_rotation", "local_rotation", "gaussian_opacity")
_HEAD_WIDTH = (3, 3, 4, 4, 1)
_EMB, _TEMB, _TNH = 96, 16, 256


def _ordered_params(net):
    """The parameters in the order the autograd node takes them (and returns their gradients)."""
    ps = []
    if net.is_blender:
        ps += [net.timenet[0].weight, net.timenet[0].bias, net.timenet[2].weight, net.timenet[2].bias]
    for lin in net.linear:
        ps += [lin.weight, lin.bias]
    for name in _HEADS:
        head = getattr(net, name, None)
        if head is not None:
            ps += [head.weight, head.bias]
    return ps


class _Cfg:
    __slots__ = ("W", "is_blender", "max_d_scale", "heads")

    def __init__(self, W, is_blender, max_d_scale, heads):
        self.W, self.is_blender, self.max_d_scale, self.heads = W, is_blender, max_d_scale, heads


def _fill(struct, cfg, tensors):
    """Pointers of ``tensors`` (ordered as _ordered_params) into a riggs_node_mlp / riggs_node_mlp_grads struct."""
    it = iter(tensors)
    if cfg.is_blender:
        struct.tn_w0, struct.tn_b0, struct.tn_w1, struct.tn_b1 = (next(it).data_ptr() for _ in range(4))
    for l in range(8):
        struct.w[l] = next(it).data_ptr()
        struct.b[l] = next(it).data_ptr()
    for h in range(5):
        if cfg.heads[h]:
            struct.head_w[h] = next(it).data_ptr()
            struct.head_b[h] = next(it).data_ptr()
    return struct


def _net_struct(cfg, params):
    s = L.NodeMlp()
    s.width, s.depth, s.is_blender, s.max_d_scale = cfg.W, 8, int(cfg.is_blender), float(cfg.max_d_scale)
    return _fill(s, cfg, params)


class _NodeMlp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cfg, x, t, t_stride, keep, *params):
        lib = L.lib()
        R, W, dev = x.shape[0], cfg.W, x.device
        acts = torch.empty(int(lib.riggs_node_mlp_acts_floats(R, W, 8)), dtype=torch.float32, device=dev)
        outs = [torch.empty(R, _HEAD_WIDTH[h], dtype=torch.float32, device=dev) if cfg.heads[h] else None for h in range(5)]
        net = _net_struct(cfg, params)
        L.check(lib.riggs_node_mlp_forward(C.byref(net), R, x.data_ptr(), t.data_ptr(), t_stride, acts.data_ptr(),
                                           *[L.ptr(o) for o in outs], L.stream_ptr()), "riggs_node_mlp_forward")
        off = int(lib.riggs_node_mlp_hidden_offset(R, W, 8))
        hidden = acts[off:off + R * W].view(R, W)
        ctx.cfg, ctx.R = cfg, R
        ctx.save_for_backward(acts, *params)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(hidden)
        if keep is not None:
            keep["acts"] = acts
        present = tuple(o for o in outs if o is not None)
        return present + (hidden,)

    @staticmethod
    def backward(ctx, *gs):
        cfg, R = ctx.cfg, ctx.R
        acts, params = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        lib = L.lib()
        cot, it = [], iter(gs)
        for h in range(5):
            g = next(it) if cfg.heads[h] else None
            cot.append(None if g is None else L.require_cuda_f32("cotangent", g, (R, _HEAD_WIDTH[h])))
        ws = torch.empty(int(lib.riggs_node_mlp_backward_workspace_floats(R, cfg.W, 8)), dtype=torch.float32, device=acts.device)
        grads = [torch.empty_like(p, memory_format=torch.contiguous_format) for p in params]
        net = _net_struct(cfg, params)
        gst = _fill(L.NodeMlpGrads(), cfg, grads)
        L.check(lib.riggs_node_mlp_backward(C.byref(net), R, acts.data_ptr(), *[L.ptr(g) for g in cot], ws.data_ptr(),
                                            C.byref(gst), L.stream_ptr()), "riggs_node_mlp_backward")
        return (None, None, None, None, None) + tuple(grads)


class DeformNetwork(nn.Module):
    """The reference's ``DeformNetwork`` (constructor keywords, parameter names, initialisers and the returned dict) on the HIP
    kernels.  ``t_multires`` is ignored as in the reference (6 with ``is_blender``, else 10).  D = 8, W in {64, 128, 256}."""

    def __init__(self, D=8, W=256, input_ch=3, output_ch=59, t_multires=6, multires=10, is_blender=False, local_frame=False,
                 pred_opacity=False, pred_color=False, resnet_color=True, hash_color=False, color_wrt_dir=False,
                 progressive_brand_time=False, max_d_scale=-1, **kwargs):
        super().__init__()
        if pred_color:
            raise NotImplementedError("pred_color: the colour heads are not part of the HIP node network; pass the reference's "
                                      "module as network=")
        if progressive_brand_time:
            raise NotImplementedError("progressive_brand_time is not part of the HIP node network; pass the reference's module "
                                      "as network=")
        if D != 8 or W not in (64, 128, 256) or multires != 10 or input_ch != 3:
            raise NotImplementedError("the HIP node network supports D = 8, W in {64, 128, 256}, multires = 10, input_ch = 3")
        self.name = "mlp"
        self.D, self.W, self.output_ch = D, W, output_ch
        self.t_multires = 6 if is_blender else 10
        self.skips = [D // 2]
        self.progressive_brand_time = False
        time_input_ch = 2 * self.t_multires + 1
        xyz_input_ch = 3 + 3 * 2 * multires
        self.input_ch = xyz_input_ch + time_input_ch
        self.pred_opacity, self.pred_color, self.resnet_color = pred_opacity, False, resnet_color
        self.hash_color, self.color_wrt_dir, self.max_d_scale = (not resnet_color and hash_color), color_wrt_dir, max_d_scale
        self.reg_loss = 0.
        if is_blender:
            self.time_out = 30
            self.timenet = nn.Sequential(nn.Linear(time_input_ch, 256), nn.ReLU(inplace=True), nn.Linear(256, self.time_out))
            in0 = xyz_input_ch + self.time_out
        else:
            in0 = self.input_ch
        self.linear = nn.ModuleList([nn.Linear(in0, W)] + [nn.Linear(W, W) if i not in self.skips else nn.Linear(W + in0, W)
                                                            for i in range(D - 1)])
        self.is_blender = is_blender
        self.gaussian_warp = nn.Linear(W, 3)
        self.gaussian_scaling = nn.Linear(W, 3)
        self.gaussian_rotation = nn.Linear(W, 4)
        self.local_frame = local_frame
        if local_frame:
            self.local_rotation = nn.Linear(W, 4)
            nn.init.normal_(self.local_rotation.weight, mean=0, std=1e-4)
            nn.init.zeros_(self.local_rotation.bias)
        for layer in self.linear:
            nn.init.kaiming_uniform_(layer.weight, mode="fan_in", nonlinearity="relu")
            nn.init.zeros_(layer.bias)
        nn.init.normal_(self.gaussian_warp.weight, mean=0, std=1e-5)
        nn.init.normal_(self.gaussian_scaling.weight, mean=0, std=1e-8)
        nn.init.normal_(self.gaussian_rotation.weight, mean=0, std=1e-5)
        nn.init.zeros_(self.gaussian_warp.bias)
        nn.init.zeros_(self.gaussian_scaling.bias)
        nn.init.zeros_(self.gaussian_rotation.bias)
        if pred_opacity:
            self.gaussian_opacity = nn.Linear(W, 1)
            nn.init.normal_(self.gaussian_opacity.weight, mean=0, std=1e-5)
            nn.init.zeros_(self.gaussian_opacity.bias)
        # tests: set to True to keep the last call's stored activations (``stored_activations``)
        self.keep_stored_activations = False
        self._kept = None

    def trainable_parameters(self):
        return [{"params": list(self.parameters()), "name": "mlp"}]

    def update(self, iteration, *args, **kwargs):
        return

    def _cfg(self):
        return _Cfg(self.W, self.is_blender, self.max_d_scale if self.max_d_scale > 0 else -1.0,
                    (True, True, True, self.local_frame, self.pred_opacity))

    @property
    def stored_activations(self):
        """What the last forward (one chunk) stored for its backward, as views: ``emb`` (R, 96; the embedded input, zero padded),
        ``timenet_hidden`` (R, 256; is_blender) and ``act`` (8, R, W), the post-ReLU activations whose signs are the ReLU masks.
        Kept only while ``keep_stored_activations`` is set."""
        if not self._kept:
            return None
        acts, R, W = self._kept["acts"], self._kept["R"], self.W
        o_t = R * (_EMB + _TEMB)
        o_a = o_t + R * _TNH + R * 4
        return {"emb": acts[:R * _EMB].view(R, _EMB), "timenet_hidden": acts[o_t:o_t + R * _TNH].view(R, _TNH),
                "act": acts[o_a:o_a + 8 * R * W].view(8, R, W)}

    def forward(self, x, t, **kwargs):
        if not (torch.is_tensor(x) and torch.is_tensor(t)):
            raise L.RiggsHipError("x and t must be tensors")
        if x.requires_grad or t.requires_grad:
            raise L.RiggsHipError("the node network does not differentiate its inputs: pass x and t detached")
        if x.dim() != 2 or x.shape[1] != 3 or x.shape[0] < 1:
            raise L.RiggsHipError("x must be (R, 3) with R >= 1, got %s" % (tuple(x.shape),))
        x = L.require_cuda_f32("x", x)
        R = x.shape[0]
        t = L.require_cuda_f32("t", t)
        if t.numel() == 1:
            t, t_stride = t.reshape(1), 0
        else:
            try:
                te = t.expand(R, 1) if t.dim() == 2 else t.reshape(-1, 1).expand(R, 1)
            except RuntimeError:
                raise L.RiggsHipError("t must be (R, 1) or broadcastable to it, got %s for R = %d" % (tuple(t.shape), R))
            if te.stride(0) == 0:
                t, t_stride = te[0].reshape(1), 0
            else:
                t, t_stride = te.contiguous().reshape(R), 1
        params = _ordered_params(self)
        for p in params:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise L.RiggsHipError("the node network's parameters must be contiguous float32 CUDA(HIP) tensors")
        cfg = self._cfg()
        keep = {} if self.keep_stored_activations else None
        chunks = []
        for r0 in range(0, R, MAX_ROWS):
            r1 = min(R, r0 + MAX_ROWS)
            tc = t if t_stride == 0 else t[r0:r1]
            chunks.append(_NodeMlp.apply(cfg, x[r0:r1], tc, t_stride, keep, *params))
            if keep is not None:
                keep["R"] = r1 - r0
        self._kept = keep
        outs = chunks[0] if len(chunks) == 1 else tuple(torch.cat(c, 0) for c in zip(*chunks))
        it = iter(outs)
        d_xyz, scaling, rotation = next(it), next(it), next(it)
        local = next(it) if self.local_frame else None
        opac = next(it) if self.pred_opacity else None
        hidden = next(it)
        ret = {"d_xyz": d_xyz, "d_rotation": rotation, "d_scaling": scaling, "hidden": hidden, "d_opacity": opac, "d_color": None}
        if self.local_frame:
            ret["local_rotation"] = local
        return ret
