"""Float64 restatement of the stage-1 node regularisers (csrc/node_reg.hip; utils/deform_utils.py:51-198 and
utils/time_utils.py:1091-1120 of the reference) in plain torch ops, device-agnostic: the tests' yardstick for the HIP path.

Neighbour lists are the KNN contract in fp32 (squared distances summed coordinate by coordinate, ascending, ties to the lowest
index; what the kernel computes bit for bit), everything after them is float64 with autograd.  The ARAP rotation is the SVD
Kabsch solution of estimate_rotation (R = V U^T, the column of U of the smallest singular value flipped when det R <= 0; S = 0
when some coordinate of every edge is unchanged), solved on the host in float64 and held constant."""
import torch


def knn_ref(points, Kq, drop_first=False, least_edge_num=0, radius=None):
    """(M, D) fp32 -> int64 indices and fp32 squared distances (M, Kq - drop_first), -1 / inf where dropped or missing."""
    p = points.detach().float()
    M, D = p.shape
    d = torch.zeros(M, M, dtype=torch.float32, device=p.device)
    for c in range(D):
        t = p[:, None, c] - p[None, :, c]
        d = d + t * t
    dist, idx = torch.sort(d, dim=1, stable=True)
    k = min(Kq, M)
    dist, idx = dist[:, :k], idx[:, :k]
    if k < Kq:
        dist = torch.cat([dist, torch.full((M, Kq - k), float("inf"), device=p.device)], 1)
        idx = torch.cat([idx, torch.full((M, Kq - k), -1, dtype=idx.dtype, device=p.device)], 1)
    if drop_first:
        dist, idx = dist[:, 1:], idx[:, 1:]
    if radius is not None:
        r2 = torch.tensor(float(radius) ** 2, dtype=torch.float32).item()
        far = ~(dist < r2)
        far[:, :least_edge_num] = False
        idx = torch.where(far, torch.full_like(idx, -1), idx)
        dist = torch.where(far, torch.full_like(dist, float("inf")), dist)
    return idx, dist


def _edges(p, idx):
    """p (M, 3), idx (M, K) with -1 -> (M, K, 3) edges p_i - p_j, zero where dropped"""
    ic = idx.clamp_min(0)
    e = p[:, None, :] - p[ic]
    return torch.where((idx >= 0)[..., None], e, torch.zeros_like(e))


def arap_rotations(seq32, idx, rows):
    """(Ns, T, 3, 3) float64 rotations of estimate_rotation for every sample row and time (t = 0: identity)."""
    T = seq32.shape[0]
    out = [torch.eye(3, dtype=torch.float64).expand(rows.shape[0], 3, 3)]
    src32 = _edges(seq32[0], idx)[rows]
    for t in range(1, T):
        tgt32 = _edges(seq32[t], idx)[rows]
        src, tgt = src32.double().cpu(), tgt32.double().cpu()
        S = src.transpose(1, 2) @ tgt
        same = (src32 == tgt32).all(dim=1).any(dim=1).cpu()
        S[same] = 0
        U, sig, Vh = torch.linalg.svd(S)
        V = Vh.transpose(1, 2)
        R = V @ U.transpose(1, 2)
        flip = torch.det(R) <= 0
        if flip.any():
            U2 = U.clone()
            col = sig.argmin(dim=1)
            U2[torch.arange(U.shape[0])[flip], :, col[flip]] *= -1
            R = torch.where(flip[:, None, None], V @ U2.transpose(1, 2), R)
        zero = (S == 0).all(dim=2).all(dim=1)
        R[zero] = torch.eye(3, dtype=torch.float64)  # torch.svd of a zero 3x3: U = V = I
        out.append(R)
    return torch.stack(out, 1).to(seq32.device)


def arap_ref(seq, idx, rows, R=None):
    """cal_arap_error (weight = None): seq (T, M, 3) float64 with grad; idx (M, K) int64 (-1 dropped); rows (Ns) int64."""
    if R is None:
        R = arap_rotations(seq.detach().float(), idx, rows)
    src = _edges(seq[0], idx)[rows]
    w = (idx >= 0)[rows].double()
    e = seq.new_zeros(())
    for t in range(1, seq.shape[0]):
        tgt = _edges(seq[t], idx)[rows]
        r = tgt - torch.einsum("sab,snb->sna", R[:, t], src)
        e = e + (w * (r * r).sum(-1)).sum()
    return e


def elastic_ref(nodes_t, idx, w):
    """nodes_t (M, T, 3) float64, idx (M, K) int64 (-1: none), w (M, K) float64."""
    ic = idx.clamp_min(0)
    d = nodes_t[ic] - nodes_t[:, None]  # M, K, T, 3
    # the norm's gradient at 0 is 0 (torch's convention)
    n2 = (d * d).sum(-1)
    safe = torch.where(n2 > 0, n2, torch.ones_like(n2))
    ln = torch.where(n2 > 0, safe.sqrt(), torch.zeros_like(n2))
    var = ln.var(dim=2)
    v = var / (var.detach() + 1e-5)
    v = torch.where(idx >= 0, v, torch.zeros_like(v))
    return (v * w).sum(1).mean()


def acc_ref(nodes_t):
    d = nodes_t[:, 0] + nodes_t[:, 2] - 2 * nodes_t[:, 1]
    n2 = (d * d).sum(-1)
    safe = torch.where(n2 > 0, n2, torch.ones_like(n2))
    a = torch.where(n2 > 0, safe.sqrt(), torch.zeros_like(n2))
    return (a / (a.detach() + 1e-5)).mean()


def graph_weight_ref(nodes, radius_log, weight_logit, hyper, idx):
    """cal_nn_weight(x=nodes[:, :3], feature=nodes[:, 3:], K) on given (M, K + 1) lists, float64, before column 0 is dropped."""
    q = nodes[:, :3].detach()
    if hyper > 0:
        q = torch.cat([q, nodes[:, 3:3 + hyper]], -1)
    ic = idx.clamp_min(0)
    d2 = ((q[:, None] - q[ic]) ** 2).sum(-1)
    w = torch.exp(-d2 / (2 * torch.exp(radius_log)[ic] ** 2))
    if weight_logit is not None:
        w = w * torch.sigmoid(weight_logit)[ic][..., 0]
    w = torch.where(idx >= 0, w + 1e-7, torch.zeros_like(w))
    return w / w.sum(-1, keepdim=True)


class ClosedFormNodeNet(torch.nn.Module):
    """A node network with parameters and a closed form, for the stage-1 fixtures: d_xyz = A sin(2 pi f t + 20 x U) + t (x B),
    a phase per component (so no node's second time difference vanishes in all three at once); the other attributes follow
    d_xyz (dtype follows the parameters)."""

    def __init__(self):
        super().__init__()
        self.A = torch.nn.Parameter(torch.tensor([0.05, -0.03, 0.02]))
        self.B = torch.nn.Parameter(torch.tensor([[0.10, 0.02, -0.01], [0.00, 0.08, 0.03], [-0.02, 0.01, 0.12]]))
        self.f = torch.nn.Parameter(torch.tensor(1.3))
        self.register_buffer("U", torch.tensor([[1.0, -2.0, 0.5], [2.0, 1.0, -1.0], [-1.0, 0.5, 2.0]]))

    def forward(self, x, t, **kwargs):
        x = x.to(self.A.dtype)
        t = t.to(self.A.dtype)
        d = self.A * torch.sin(2 * torch.pi * self.f * t + 20.0 * (x @ self.U.to(x.dtype))) + t * (x @ self.B)
        z4 = torch.zeros(x.shape[0], 4, dtype=d.dtype, device=d.device)
        return {"d_xyz": d, "d_rotation": z4 + 0.01 * d[:, :1], "d_scaling": 0.1 * d, "local_rotation": z4.clone(), "hidden": None,
                "d_opacity": None, "d_color": None}


class TimeReplay(torch.nn.Module):
    """Wraps a node network: records the time input of every call (``replay=None``) or substitutes recorded ones, in order."""

    def __init__(self, net, replay=None):
        super().__init__()
        self.net, self.replay, self.seen = net, replay, []

    def forward(self, x, t, **kwargs):
        if self.replay is not None:
            t = self.replay[len(self.seen)].to(device=x.device, dtype=t.dtype).reshape(t.shape)
        self.seen.append(t.detach().clone())
        return self.net(x=x, t=t, **kwargs)


class DensifyOpt:
    """training arguments of the node Gaussians in the densify fixture"""
    percent_dense = 0.01
    position_lr_init = position_lr_final = 1e-4
    position_lr_delay_mult = 0.01
    position_lr_max_steps = 1000
    feature_lr, opacity_lr, scaling_lr, rotation_lr = 2.5e-3, 0.05, 1e-3, 1e-3
    skeleton_gs_position_lr = 1e-4


def densify_inputs(seed):
    """The Gaussians, the initial point cloud (three far outliers: nodes no Gaussian uses) and the densification inputs."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(1500, 3, generator=g) * 0.5
    pcl = torch.cat([x[:800], torch.tensor([[3.0, 3.0, 3.0], [-3.0, 2.5, 0.0], [2.0, -3.0, 1.0]])])
    feature = 0.02 * torch.randn(1500, 9, generator=g)
    x_grad = torch.rand(1500, 3, generator=g) * 1e-4
    x_grad[:300] += 0.05
    return x, pcl, feature, x_grad


def densify_step_loss(cn):
    """the one optimizer step before densify: non-zero moments in every 'nodes' parameter"""
    return (cn.nodes ** 2).sum() + (cn._node_radius ** 2).sum() + (cn._node_weight ** 2).sum() + sum(p.sum() for p in cn.network.parameters())
