"""Float64 references of the PoseMLP kernels (csrc/pose_mlp.hip) with per-element bounds, stage by stage.

Every stage boundary of the network is in memory: ``acts[0 : emb + depth * width]`` holds the embedding and every layer's stored
activation, ``rotation`` / ``translation`` the heads, every bias gradient in ``flat_grads`` is that stage's v_l (dz_l, or the heads'
cotangents) stored unchanged, and the ``_fk`` entry leaves dL/dlocal_rot and dL/dglobal_trans.  Each stage is therefore checked
on its own from the fp32 values the kernel itself read (``check_stages``): a float64 evaluation of those inputs is exact to
~1e-15, so what is left between kernel and reference is the kernel's fp32 arithmetic of that one stage.  u = 2^-24.

Embedding.  acts[0] = t bit for bit.  t * 2^k is exact in fp32, so acts[1 + 2k], acts[2 + 2k] are compared with float64 sin / cos
of that product; the allowance for OCML's sinf / cosf (-fno-fast-math) is SINCOS_ULP ulp of the result — no figure is documented
in the ROCm tree, so it is twice the worst error measured on the grid, rounded up to a whole ulp (NOTES.md has the measurement).

Forward unit r of layer l, and the head rows (pm_forward_fused_kernel and pm_layer_kernel alike: one wave per row, lane i takes
inputs i, i + 64, ...).  Per lane ceil(in_dim / 64) <= 5 serial FMAs (one rounding each under -ffp-contract=fast), the six DPP
steps of wave_sum, the bias add, and for the rotation rows one more add of rot_bias4[r & 3]:
    L_fwd = ceil(in_dim / 64) + 6 + 1 (+ 1),     |got - ref| <= L_fwd u (sum_i |w_i||x_i| + |b| (+ |rot_bias|)).
ReLU is exact and 1-Lipschitz, so the same bound holds for the stored max(z, 0): a unit whose float64 pre-activation lies within
its bound of 0 may be stored as 0 or as the (small) value, nothing else.

Backward chain D_{l-1}[c] = sum_r M_l[r][off + c] v_l[r], then v_{l-1}[c] = D_{l-1}[c] where the kernel's own stored h_{l-1}[c] > 0
and exactly 0 elsewhere (the reference takes the mask from the kernel's ``acts``: h is the forward's stored value, bit for bit).
  one launch (pm_backward_fused_kernel): lane i takes rows i, i + 64, i + 128, i + 192 — 4 serial FMAs whatever the row count —,
      one more for head rows 256.., then the six steps of the tree:              L_bwd1 = 4 (+ 1 if heads and n_rows > 256) + 6
  layered (pm_backward_step_kernel): thread (grid.y, wave) takes rows r0, r0 + 32, ...: ceil(n_rows / 32) serial FMAs, the 4-wave
      LDS sum (3 adds), and eight atomicAdds onto a zeroed word in free order, an any-order sum of 8 (8 roundings at most):
                                                                                 L_bwdL = ceil(n_rows / 32) + 3 + 8
Both with |got - ref| <= L u sum_r |M||v|.

Weight gradients dW[r][c] = fl(v_r * in_c): one rounding, u |ref| (+ 2^-149 for a product below the normal range); in_c through the
skip layout with the embedding in front.  Bias gradients: bit for bit the stage's v; with no chain in front the heads' are bit
for bit g_rotation / g_translation.

``_fk`` entry.  dL/dlocal_rot = skin_ref.chain_backward's value and bound (the reverse sweep, float64 autograd) + g_rotation
+ coef (q - unit): two more adds, one product and one subtraction -> + 4 u (|chain| + |g_rot| + |coef||q - unit|) + the chain's
bound.  dL/dglobal_trans = g_tr + sum_j dL/dd_nodes_j: the one-launch kernel starts from g_tr and adds the J terms serially (J
roundings); the layered path copies g_tr, and riggs_fk_backward adds a serial sum s = sum_j gn_j (J - 1 roundings from 0) with one
more add: J roundings as well, in the other association.  Both: J u (|g_tr| + sum |gn|).  template_fixed_loss = mean((q - unit)^2):
the one-launch kernel sums ceil(4J / 64) <= 4 elements per lane and a 6-step butterfly; pm_fixed_add_kernel ceil(4J / 256) <= 4 per
thread, a 6-step butterfly and 3 adds over the waves; each element carries the subtraction and the square (2 u), the division 1:
    (4 + 6 + 3 + 2 + 1) u loss  covers both.

An element whose bound is 0 is compared exactly: dead units, zero cotangents, weight-gradient rows of dead units.

End to end, as the second opinion (``end_to_end``): the same network as float64 torch ops from the fp32 parameters, gradients by
float64 autograd (no formula shared with the stage references), held at the stage bounds accumulated through |W|:
    with the ReLU decisions fixed both chains are linear in the stages' rounding errors rho_k (|rho_k| <= the stage bound b_k,
    the embedding's allowance included), delta_out = sum_k P_k rho_k with P_k the product of the masked matrices from stage k to
    the output, so |delta_out| <= sum_k |P_k| b_k; b_k is evaluated on the reference input widened by its own accumulated error.
    The absolute value is taken of the PRODUCT: factor by factor (|W_d| ... |W_k|) a width-256 row sums to ~20, eight layers put
    the bound ten orders above the values and nothing would be held (see ``accumulated``).
    dW_l      (1 + u) (|v_l| + ev_l) (|in| + e_in) - |v_l||in|.
This needs the ReLU decisions of kernel and reference to agree: ``assert_case_is_safe`` asserts, on the float32 restatement
(``restate``), that no unit is within its accumulated error of 0 (a case that fails gets another seed through RESEED), and the GPU
test asserts the same on the kernel's acts (``check_end_to_end``).

Weight scales.  nn.Linear's default initialisation (U(+-1/sqrt(in))) shrinks a ReLU network's activations by ~sqrt(6) per layer:
over 12 layers the outputs would sit at 1e-5 of the biases and every bound would be vacuous.  The cases draw He-uniform inner
layers, U(+-sqrt(6 / in)), which keep the activations' scale, and heads U(+-sqrt(3 / in)); biases U(+-0.1).  The vacuity condition
(tests/test_pose_mlp_ref_cpu.py): per array and case at most 1 % of the non-zero-reference elements have bound >= |reference|.

numpy / torch on the host; tests/test_pose_mlp_ref_cpu.py shows that these bounds reject the faults the GPU grid
(tests/test_gpu_pose_mlp_f64.py) is there to catch, and accept fp32 arithmetic summed in other lane orders.
"""
import math
import zlib

import numpy as np
import torch

from tests.mlp_ref import assert_within, violations  # noqa: F401  (the same checker)
from tests.skin_ref import U, chain_backward

SINCOS_ULP = 3.0   # allowance for OCML sinf / cosf in ulp of the result: 2 x the measured worst (1.41 ulp), rounded up (NOTES.md)
TINY = 2.0 ** -149
PM_MAX_HEAD = 320
MAX_J = 64


# ------------------------------------------------------------------------------------------------------------- configuration
def cfg(width, J, depth=8, skip=None, multires=8):
    return {"width": width, "J": J, "n_rot": 4 * J, "depth": depth, "skip": depth // 2 if skip is None else skip,
            "multires": multires, "emb": 1 + 2 * multires}


def one_launch(c, layered_option=False):
    """pm_one_launch: the dispatch rule of csrc/pose_mlp.hip."""
    if layered_option or c["n_rot"] > 4 * MAX_J:
        return False
    return c["n_rot"] + 3 <= c["width"] or (c["width"] >= 128 and c["n_rot"] + 3 <= PM_MAX_HEAD)


def in_dim(c, l):
    """Input width of consumer l (l == depth: the heads)."""
    if l == 0:
        return c["emb"]
    return c["width"] + c["emb"] if l - 1 == c["skip"] else c["width"]


def layout(c):
    """Offsets of [W_0, b_0, ..., W_rot, b_rot, W_tr, b_tr] in flat_grads: list of (w_off, b_off, rows, in_dim), total."""
    o, out = 0, []
    for l in range(c["depth"]):
        out.append((o, o + c["width"] * in_dim(c, l), c["width"], in_dim(c, l)))
        o += c["width"] * in_dim(c, l) + c["width"]
    ih = in_dim(c, c["depth"])
    for rows in (c["n_rot"], 3):
        out.append((o, o + rows * ih, rows, ih))
        o += rows * ih + rows
    return out, o


def layer_input(c, acts, l):
    """Input vector of consumer l from the stored activations (embedding IN FRONT of h after the skip layer)."""
    emb, w = c["emb"], c["width"]
    if l == 0:
        return acts[:emb]
    h = acts[emb + (l - 1) * w: emb + l * w]
    return np.concatenate([acts[:emb], h]) if l - 1 == c["skip"] else h


def matrices(c, p):
    """Consumer matrices M_0 .. M_depth (the heads stacked: rotation rows, then translation) and biases, as given."""
    Ms = [p["W"][l] for l in range(c["depth"])] + [np.concatenate([p["W_rot"], p["W_tr"]], 0)]
    bs = [p["b"][l] for l in range(c["depth"])] + [np.concatenate([p["b_rot"], p["b_tr"]])]
    return Ms, bs


# case name -> seed offset, for the cases whose first seed put a unit within its accumulated error of 0 (or, "width 191", one of the
# 96 rotation outputs below its end-to-end bound: the vacuity condition); tests/test_pose_mlp_ref_cpu.py holds the table to 5 % of the cases
RESEED = {"inside 256x63": 1, "extra 256x64": 1, "size 256x65": 1, "width+emb 319": 1, "draw 1": 1}


def build(c, seed, t=0.37, rot_bias=True, cot="random", dead_layer=None, fk=None, name=None):
    """The fp32 parameters, inputs and cotangents of one case (numpy float32).  ``fk``: None or a dict of options of the _fk
    entry (see tests/test_gpu_pose_mlp_f64.py)."""
    g = np.random.default_rng(seed + 1000 * RESEED.get(name, 0))
    f32 = np.float32
    p = {"W": [], "b": []}
    for l in range(c["depth"]):
        n = in_dim(c, l)
        a = math.sqrt(6.0 / n)
        p["W"].append(g.uniform(-a, a, (c["width"], n)).astype(f32))
        p["b"].append(g.uniform(-0.1, 0.1, c["width"]).astype(f32))
    if dead_layer is not None:
        p["b"][dead_layer][:] = -1.0
        p["W"][dead_layer][:] = -np.abs(p["W"][dead_layer]) if dead_layer > 0 else 0.0
        if dead_layer > 0 and dead_layer - 1 == c["skip"]:
            p["W"][dead_layer][:, :c["emb"]] = 0.0  # (the embedding in front of h has both signs)
    ih = in_dim(c, c["depth"])
    a = math.sqrt(3.0 / ih)
    p["W_rot"] = g.uniform(-a, a, (c["n_rot"], ih)).astype(f32)
    p["b_rot"] = g.uniform(-0.1, 0.1, c["n_rot"]).astype(f32)
    p["W_tr"] = g.uniform(-a, a, (3, ih)).astype(f32)
    p["b_tr"] = g.uniform(-0.1, 0.1, 3).astype(f32)
    p["t"] = f32(t)
    p["rot_bias"] = np.array([1, 0, 0, 0], f32) + (0.01 * g.standard_normal(4)).astype(f32) if rot_bias else None
    gr, gt = g.standard_normal(c["n_rot"]).astype(f32), g.standard_normal(3).astype(f32)
    if cot == "zero":
        gr[:], gt[:] = 0, 0
    elif cot == "row":
        k = int(g.integers(0, c["n_rot"]))
        v = gr[k]
        gr[:], gt[:] = 0, 0
        gr[k] = v
    elif cot == "rot":
        gt[:] = 0
    elif cot == "tr":
        gr[:] = 0
    p["g_rot"], p["g_tr"] = gr, gt
    p["fk"] = fk
    return p


# ------------------------------------------------------------------------------------------------------- the checker's plumbing
def _check(res, name, got, ref, bnd, must_zero=None):
    got_t = torch.from_numpy(np.ascontiguousarray(np.asarray(got, np.float32).reshape(-1)))
    ref_t = torch.from_numpy(np.ascontiguousarray(np.asarray(ref, np.float64).reshape(-1)))
    bnd_t = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(np.asarray(bnd, np.float64), np.shape(ref)).reshape(-1).copy()))
    mz = None if must_zero is None else torch.from_numpy(np.ascontiguousarray(np.asarray(must_zero).reshape(-1)))
    n_bad, worst, first = violations(got_t, ref_t, bnd_t, must_zero=mz)
    nz = ref_t != 0
    vac = float(((bnd_t >= ref_t.abs()) & nz).sum()) / max(1, int(nz.sum()))
    old = res.get(name)
    if old is None:
        res[name] = {"n": got_t.numel(), "bad": n_bad, "worst": worst, "first": first, "vac": vac, "nz": int(nz.sum())}
    else:  # (an array checked piecewise: per layer)
        tot = old["nz"] + int(nz.sum())
        res[name] = {"n": old["n"] + got_t.numel(), "bad": old["bad"] + n_bad, "worst": max(old["worst"], worst),
                     "first": old["first"] if old["first"] is not None else first,
                     "vac": (old["vac"] * old["nz"] + vac * int(nz.sum())) / max(1, tot), "nz": tot}


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def embedding(c, t):
    """float64 reference and bound of acts[:emb]."""
    t64 = float(np.float32(t))
    ref, bnd = [t64], [0.0]
    for k in range(c["multires"]):
        x = t64 * float(2 ** k)
        for v in (math.sin(x), math.cos(x)):
            ref.append(v)
            bnd.append(0.0 if (v == 0.0 or abs(v) == 1.0 and x == 0.0) else SINCOS_ULP * float(ulp32(v)))
    return np.array(ref), np.array(bnd)


def sincos_ulp_error(c, t, acts):
    """The worst error of the stored embedding in ulp of the result (the measurement behind SINCOS_ULP)."""
    ref, _ = embedding(c, t)
    err = np.abs(np.asarray(acts[:c["emb"]], np.float64) - ref)[1:]
    return float((err / ulp32(ref[1:])).max()) if err.size else 0.0


def fwd_depth(n_in, rot_bias=False):
    return -(-n_in // 64) + 6 + 1 + (1 if rot_bias else 0)


def bwd_depth(n_rows, heads, layered):
    if layered:
        return -(-n_rows // 32) + 3 + 8
    return 4 + (1 if heads and n_rows > 256 else 0) + 6


# ------------------------------------------------------------------------------------------------------------ stage references
def check_stages(c, p, out, layered, res=None):
    """Every stage of forward and backward from the values the kernel read.  ``out``: acts, rotation, translation, flat (and dq,
    dgt, loss for the _fk entry) as numpy float32.  Returns {array: {bad, worst, vac, ...}}."""
    res = {} if res is None else res
    d, w, emb, nr = c["depth"], c["width"], c["emb"], c["n_rot"]
    acts = np.asarray(out["acts"], np.float32)[:emb + d * w]
    a64 = acts.astype(np.float64)
    Ms, bs = matrices(c, p)
    ref, bnd = embedding(c, p["t"])
    _check(res, "emb", acts[:emb], ref, bnd)
    # ---- forward
    for l in range(d + 1):
        x = layer_input(c, a64, l)
        M, b = Ms[l].astype(np.float64), bs[l].astype(np.float64)
        z = M @ x + b
        s = np.abs(M) @ np.abs(x) + np.abs(b)
        if l < d:
            _check(res, "acts", acts[emb + l * w: emb + (l + 1) * w], np.maximum(z, 0), fwd_depth(x.size) * U * s)
        else:
            rb = p["rot_bias"]
            zr, sr = z[:nr], s[:nr]
            if rb is not None:
                rb64 = np.tile(rb.astype(np.float64), nr // 4)
                zr, sr = zr + rb64, sr + np.abs(rb64)
            _check(res, "rotation", out["rotation"], zr, fwd_depth(x.size, rb is not None) * U * sr)
            _check(res, "translation", out["translation"], z[nr:], fwd_depth(x.size) * U * s[nr:])
    if out.get("flat") is None:
        return res
    # ---- backward: v_l observed in the bias gradients
    lay, total = layout(c)
    flat = np.asarray(out["flat"], np.float32)
    assert flat.size == total
    v = [flat[lay[l][1]: lay[l][1] + w] for l in range(d)]
    v.append(np.concatenate([flat[lay[d][1]: lay[d][1] + nr], flat[lay[d + 1][1]: lay[d + 1][1] + 3]]))
    fk = p.get("fk")
    if fk is None:
        heads_cot = np.concatenate([p["g_rot"], p["g_tr"]])
        _check(res, "db_heads", v[d], heads_cot.astype(np.float64), 0.0)
    elif out.get("dq") is not None:
        check_fk(c, p, out, layered, res)
        heads_cot = np.concatenate([np.asarray(out["dq"], np.float32).reshape(-1), np.asarray(out["dgt"], np.float32)])
        _check(res, "db_heads", v[d], heads_cot.astype(np.float64), 0.0)
    else:  # (the two totals not asked for: the heads' bias gradients are the only copy)
        check_fk(c, p, dict(out, dq=v[d][:nr], dgt=v[d][nr:]), layered, res)
    for l in range(d, 0, -1):
        off = emb if l - 1 == c["skip"] else 0
        M = Ms[l].astype(np.float64)[:, off: off + w]
        vl = v[l].astype(np.float64)
        D = M.T @ vl
        S = np.abs(M).T @ np.abs(vl)
        alive = acts[emb + (l - 1) * w: emb + l * w] > 0
        _check(res, "v", v[l - 1], np.where(alive, D, 0.0), np.where(alive, bwd_depth(M.shape[0], l == d, layered) * U * S, 0.0),
               must_zero=~alive)
    # ---- weight gradients: one rounding of v_r * in_c
    for m in range(d + 2):
        l = min(m, d)
        x = layer_input(c, a64, l)
        vm = v[l].astype(np.float64) if m < d else (v[d][:nr] if m == d else v[d][nr:]).astype(np.float64)
        w_off, _, rows, n = lay[m]
        refW = vm[:, None] * x[None, :]
        _check(res, "dW", flat[w_off: w_off + rows * n].reshape(rows, n), refW, U * np.abs(refW) + np.where(refW != 0, TINY, 0.0))
    return res


def fk_reference(c, p):
    """float64 reference and bound of the _fk entry's dL/dlocal_rot (J, 4), dL/dglobal_trans (3) and the fixed-pose loss."""
    fk = p["fk"]
    J = c["J"]
    tt = lambda a: torch.from_numpy(np.asarray(a))  # noqa: E731
    q = fk["local_rot"]
    bw = chain_backward(tt(q), tt(fk["joints"]), tt(fk["parents"]), tt(fk["dG"]), None if fk["gn"] is None else tt(fk["gn"]))
    dq, bq = bw["dL/dlocal_rot"][0].numpy().copy(), bw["dL/dlocal_rot"][1].numpy().copy()
    mag = np.abs(dq)
    if fk["g_rot"]:
        gr = p["g_rot"].astype(np.float64).reshape(J, 4)
        dq, mag = dq + gr, mag + np.abs(gr)
    dev = q.astype(np.float64) - np.array([1.0, 0, 0, 0])
    if fk["coef"] is not None:
        dq = dq + float(fk["coef"]) * dev
        mag = mag + abs(float(fk["coef"])) * np.abs(dev)
    bq = bq + 4 * U * mag
    gt = p["g_tr"].astype(np.float64) if fk["g_tr"] else np.zeros(3)
    gn = np.zeros((J, 3)) if fk["gn"] is None else fk["gn"].astype(np.float64)
    dgt = gt + gn.sum(0)
    bgt = J * U * (np.abs(gt) + np.abs(gn).sum(0))
    loss = float((dev ** 2).mean())
    return (dq, bq), (dgt, bgt), (loss, 16 * U * loss)


def check_fk(c, p, out, layered, res):
    (dq, bq), (dgt, bgt), (loss, bl) = fk_reference(c, p)
    if out.get("dq") is not None:
        _check(res, "dq", out["dq"], dq, bq)
        _check(res, "dgt", out["dgt"], dgt, bgt)
    if out.get("loss") is not None:
        _check(res, "fixed_loss", out["loss"], np.array([loss]), np.array([bl]))
    return res


# ------------------------------------------------------------------------------------------------------------------ end to end
def end_to_end(c, p, masks=None):
    """The network as float64 torch ops with float64 autograd: outputs, the flat gradient, the pre-activations.  ``masks``
    (list of bool arrays per layer) replaces the ReLU decisions (the agreement test of the two references)."""
    T = lambda a: torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(True)  # noqa: E731
    Ws, bsl = [T(x) for x in p["W"]], [T(x) for x in p["b"]]
    heads = [T(p["W_rot"]), T(p["b_rot"]), T(p["W_tr"]), T(p["b_tr"])]
    t = torch.tensor([float(np.float32(p["t"]))], dtype=torch.float64)
    e = [t]
    for k in range(c["multires"]):
        e += [torch.sin(t * float(2 ** k)), torch.cos(t * float(2 ** k))]
    e = torch.cat(e)
    h, zs = e, []
    for l in range(c["depth"]):
        z = Ws[l] @ h + bsl[l]
        zs.append(z.detach().numpy())
        h = torch.relu(z) if masks is None else z * torch.from_numpy(np.asarray(masks[l], np.float64))
        if l == c["skip"]:
            h = torch.cat([e, h])
    rot = heads[0] @ h + heads[1]
    if p["rot_bias"] is not None:
        rot = rot + torch.from_numpy(np.tile(p["rot_bias"].astype(np.float64), c["n_rot"] // 4))
    tr = heads[2] @ h + heads[3]
    if p.get("fk") is None:
        gr, gt = p["g_rot"].astype(np.float64), p["g_tr"].astype(np.float64)
    else:
        (dq, _), (dgt, _), _ = fk_reference(c, p)
        gr, gt = dq.reshape(-1), dgt
    ((rot * torch.from_numpy(gr)).sum() + (tr * torch.from_numpy(gt)).sum()).backward()
    params = []
    for l in range(c["depth"]):
        params += [Ws[l], bsl[l]]
    params += heads
    flat = np.concatenate([(x.grad if x.grad is not None else torch.zeros_like(x)).numpy().reshape(-1) for x in params])
    return {"rotation": rot.detach().numpy(), "translation": tr.detach().numpy(), "flat": flat, "z": zs}


def _spread(srcs):
    """sum_k |A_k| b_k: the error of a vector that is sum_k A_k rho_k with |rho_k| <= b_k."""
    return sum(np.abs(A) @ b for A, b in srcs)


def accumulated(c, p, layered):
    """The stage bounds accumulated along both chains around the float64 network: (e2e values, bounds per output array,
    per-layer accumulated pre-activation error).  With the ReLU decisions fixed, both chains are LINEAR in the stages' rounding
    errors rho_k: delta = sum_k P_k rho_k with P_k the product of the (masked) matrices between stage k and the output, so
    |delta| <= sum_k |P_k| b_k.  (The absolute value is taken of the product, not factor by factor: a row of |W_l| sums to
    ~20 at width 256, and eight such factors would put every bound 10 orders above the values.)  Each b_k is evaluated on
    |x| + e_x, the reference input widened by its own accumulated error."""
    ref = end_to_end(c, p)
    d, w, emb, nr = c["depth"], c["width"], c["emb"], c["n_rot"]
    Ms, bs = matrices(c, p)
    eref, ebnd = embedding(c, p["t"])
    Ie = np.eye(emb)
    xs, exs, zerr = [], [], []
    srcs = [(Ie, ebnd)]            # sources of the current input vector; source 0 is the embedding's allowance
    x = eref
    for l in range(d + 1):
        ex = _spread(srcs)
        xs.append(x)
        exs.append(ex)
        M = Ms[l].astype(np.float64)
        s = np.abs(M) @ (np.abs(x) + ex) + np.abs(bs[l].astype(np.float64))
        L = np.full(M.shape[0], float(fwd_depth(x.size)))
        if p["rot_bias"] is not None and l == d:
            L[:nr] += 1
            s[:nr] += np.abs(np.tile(p["rot_bias"].astype(np.float64), nr // 4))
        srcs = [(M @ A, b) for A, b in srcs] + [(np.eye(M.shape[0]), L * U * s)]
        zerr.append(_spread(srcs))
        if l < d:
            alive = (ref["z"][l] > 0).astype(np.float64)
            srcs = [(alive[:, None] * A, b) for A, b in srcs]
            x = np.maximum(ref["z"][l], 0)
            if l == c["skip"]:  # [emb, h]: the embedding's rows carry the embedding's sources only
                srcs = [(np.concatenate([Ie if i == 0 else np.zeros((emb, A.shape[1])), A]), b) for i, (A, b) in enumerate(srcs)]
                x = np.concatenate([eref, x])
    bounds = {"rotation": zerr[d][:nr], "translation": zerr[d][nr:]}
    # ---- backward
    lay, total = layout(c)
    fb = np.zeros(total)
    if p.get("fk") is None:
        v, vsrc = np.concatenate([p["g_rot"], p["g_tr"]]).astype(np.float64), []
    else:
        (dq, bq), (dgt, bgt), _ = fk_reference(c, p)
        v = np.concatenate([dq.reshape(-1), dgt])
        vsrc = [(np.eye(nr + 3), np.concatenate([bq.reshape(-1), bgt]))]
    for l in range(d, -1, -1):
        ev = _spread(vsrc) if vsrc else np.zeros(v.size)
        x, ex = xs[l], exs[l]
        mats = [(l, v, ev)] if l < d else [(d, v[:nr], ev[:nr]), (d + 1, v[nr:], ev[nr:])]
        for m, vm, evm in mats:
            w_off, b_off, rows, n = lay[m]
            refW = np.abs(vm)[:, None] * np.abs(x)[None, :]
            full = (np.abs(vm) + evm)[:, None] * (np.abs(x) + ex)[None, :]
            bW = U * full + (full - refW)
            fb[w_off: w_off + rows * n] = (bW + np.where(bW != 0, TINY, 0.0)).reshape(-1)
            fb[b_off: b_off + rows] = evm
        if l == 0:
            break
        off = emb if l - 1 == c["skip"] else 0
        M = Ms[l].astype(np.float64)[:, off: off + w]
        alive = (ref["z"][l - 1] > 0).astype(np.float64)
        S = np.abs(M).T @ (np.abs(v) + ev)
        bD = alive * bwd_depth(M.shape[0], l == d, layered) * U * S
        vsrc = [(alive[:, None] * (M.T @ A), b) for A, b in vsrc] + [(np.eye(w), bD)]
        lo = lay[l - 1][1]
        v = ref["flat"][lo: lo + w]
    bounds["flat"] = fb
    return ref, bounds, zerr[:d]


def relu_decisions_safe(ref, zerr, acts=None, c=None):
    """No unit's float64 pre-activation within its accumulated error of 0 (and, given the kernel's acts, the same decisions)."""
    for l, (z, e) in enumerate(zip(ref["z"], zerr)):
        if bool((np.abs(z) <= e).any()):
            return False
        if acts is not None:
            h = np.asarray(acts)[c["emb"] + l * c["width"]: c["emb"] + (l + 1) * c["width"]]
            if not np.array_equal(h > 0, z > 0):
                return False
    return True


def check_end_to_end(c, p, out, layered, res=None, strict=True):
    """The kernel's outputs and every gradient against the float64 network at the accumulated bounds.  The ReLU decisions of the
    kernel's acts must be the reference's (``strict``: asserted; else recorded as a failed array "e2e relu decisions")."""
    res = {} if res is None else res
    ref, bounds, zerr = accumulated(c, p, layered)
    safe = relu_decisions_safe(ref, zerr, out["acts"], c)
    if strict:
        assert safe, "a ReLU decision of the case is within its accumulated error of 0, or the kernel decided otherwise: reseed (RESEED)"
    elif not safe:
        res["e2e relu decisions"] = {"n": 1, "bad": 1, "worst": float("inf"), "first": None, "vac": 0.0, "nz": 0}
    _check(res, "e2e rotation", out["rotation"], ref["rotation"], bounds["rotation"])
    _check(res, "e2e translation", out["translation"], ref["translation"], bounds["translation"])
    if out.get("flat") is not None:
        _check(res, "e2e flat_grads", out["flat"], ref["flat"], bounds["flat"])
    return res


def compose_stages(c, p, masks):
    """The stage formulas composed end to end in float64 on given ReLU masks (no rounding in between): outputs and the flat gradient,
    for the agreement test with ``end_to_end`` (autograd)."""
    d, w, emb, nr = c["depth"], c["width"], c["emb"], c["n_rot"]
    Ms, bs = matrices(c, p)
    eref, _ = embedding(c, p["t"])
    acts = np.zeros(emb + d * w)
    acts[:emb] = eref
    for l in range(d):
        z = Ms[l].astype(np.float64) @ layer_input(c, acts, l) + bs[l]
        acts[emb + l * w: emb + (l + 1) * w] = z * masks[l]
    z = Ms[d].astype(np.float64) @ layer_input(c, acts, d) + bs[d]
    rot = z[:nr] + (0 if p["rot_bias"] is None else np.tile(p["rot_bias"].astype(np.float64), nr // 4))
    lay, total = layout(c)
    flat = np.zeros(total)
    v = np.concatenate([p["g_rot"], p["g_tr"]]).astype(np.float64)
    for l in range(d, -1, -1):
        x = layer_input(c, acts, l)
        for m, vm in ([(l, v)] if l < d else [(d, v[:nr]), (d + 1, v[nr:])]):
            w_off, b_off, rows, n = lay[m]
            flat[w_off: w_off + rows * n] = (vm[:, None] * x[None, :]).reshape(-1)
            flat[b_off: b_off + rows] = vm
        if l:
            off = emb if l - 1 == c["skip"] else 0
            v = (Ms[l].astype(np.float64)[:, off: off + w].T @ v) * masks[l - 1]
    return {"rotation": rot, "translation": z[nr:], "flat": flat}


# ----------------------------------------------------------------------------- the float32 restatement of both kernel paths
def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def _fma_chain(Wc, xc):
    """acc = fma(w_k, x_k, acc) over axis 1 of (rows, K, lanes): product exact in float64, one rounding to fp32 per step."""
    acc = np.zeros((Wc.shape[0], Wc.shape[2]), np.float32)
    for k in range(Wc.shape[1]):
        acc = _f32(acc.astype(np.float64) + Wc[:, k].astype(np.float64) * xc[:, k].astype(np.float64))
    return acc


def _tree(v):
    """Pairwise fp32 sum over the last axis (64 lanes -> 1): the DPP tree's association."""
    while v.shape[-1] > 1:
        v = (v[..., 0::2] + v[..., 1::2]).astype(np.float32)
    return v[..., 0]


def wave_gemv(M, x, chunks, perm=None, drop_chunk=None):
    """y[r] = wave_sum over lanes of the lane's serial FMAs over inputs lane + 64 k (k < chunks).  ``perm``: a permutation of the 64
    lanes (another summation order within the same tree depth)."""
    rows, n = M.shape
    Mp = np.zeros((rows, chunks * 64), np.float32)
    xp = np.zeros(chunks * 64, np.float32)
    Mp[:, :n], xp[:n] = M, x
    Wc = Mp.reshape(rows, chunks, 64)
    xc = np.broadcast_to(xp.reshape(1, chunks, 64), Wc.shape)
    if drop_chunk is not None:
        Wc = Wc.copy()
        Wc[:, drop_chunk] = 0
    acc = _fma_chain(Wc, xc)
    if perm is not None:
        acc = acc[:, perm]
    return _tree(acc)


def _pick(diff, pick):
    nz = np.nonzero(diff)[0]
    order = nz[np.argsort(diff[nz])]
    return int(order[-1] if pick == "max" else order[len(order) // 2])


def restate(c, p, layered, fault=None, order=None, prev=None, pick="max"):
    """Both kernel paths in numpy float32, in the kernels' order of operations.  ``order``: None, "reversed" or an int seed for a
    random lane permutation.  ``fault``: one of FAULTS.  ``prev``: a previous launch's outputs (for the stale hand-off)."""
    d, w, emb, nr = c["depth"], c["width"], c["emb"], c["n_rot"]
    perm = None
    if order == "reversed":
        perm = np.arange(64)[::-1]
    elif order is not None:
        perm = np.random.default_rng(order).permutation(64)
    Ms, bs = matrices(c, p)
    t = np.float32(p["t"])
    acts = np.zeros(emb + d * w, np.float32)
    acts[0] = t
    for k in range(c["multires"]):
        kk = k + 1 if fault == "freq" else k
        x = float(t) * float(2 ** kk)
        sc = (math.sin(x), math.cos(x))
        if fault == "sincos" and k == min(2, c["multires"] - 1):
            sc = sc[::-1]
        acts[1 + 2 * k], acts[2 + 2 * k] = np.float32(sc[0]), np.float32(sc[1])
    fc = dict(c)
    if fault == "skip_late":
        fc["skip"] = c["skip"] + 1

    def inp(l, a=None):
        a = acts if a is None else a
        if fault == "emb_behind" and l - 1 == c["skip"] and l >= 1:
            return np.concatenate([a[emb + (l - 1) * w: emb + l * w], a[:emb]])
        if fault == "skip_late" and l >= 1:
            x = layer_input(fc, a, l)
            n = in_dim(c, l)
            return np.concatenate([x, np.zeros(max(0, n - x.size), np.float32)])[:n]
        return layer_input(c, a, l)

    rot = tr = None
    for l in range(d + 1):
        x = inp(l)
        n = x.size
        z = wave_gemv(Ms[l], x, 5, perm, drop_chunk=4 if (fault == "chunk5" and n > 256) else None)
        b = bs[l].copy()
        if fault == "head_bias" and l == d:
            b[w:] = 0
        z = (z + b).astype(np.float32)
        if l < d:
            h = np.maximum(z, np.float32(0))
            if fault == "stale" and l == d // 2 and prev is not None:
                ph = prev["acts"][emb + l * w: emb + (l + 1) * w]
                k = _pick(np.abs(h - ph), pick)  # (one granule not re-written: the unit whose previous value differs most / as the median does)
                h[k] = ph[k]
            acts[emb + l * w: emb + (l + 1) * w] = h
        else:
            rot, tr = z[:nr].copy(), z[nr:].copy()
            if p["rot_bias"] is not None:
                idx = np.arange(nr) & 3 if fault != "rot_bias_idx" else np.minimum(np.arange(nr), 3)
                rot = (rot + p["rot_bias"][idx]).astype(np.float32)
    out = {"acts": acts, "rotation": rot, "translation": tr}
    # ---- backward
    lay, total = layout(c)
    flat = np.full(total, np.nan, np.float32)
    fk = p.get("fk")
    if fk is None:
        v = np.concatenate([p["g_rot"], p["g_tr"]]).astype(np.float32)
    else:
        J = c["J"]
        base = chain_backward(torch.from_numpy(fk["local_rot"]), torch.from_numpy(fk["joints"]), torch.from_numpy(fk["parents"]),
                              torch.from_numpy(fk["dG"]), None if fk["gn"] is None else torch.from_numpy(fk["gn"]))
        dq = _f32(base["dL/dlocal_rot"][0].numpy())
        if fk["g_rot"] and fault != "no_g_rot":
            dq = (dq + p["g_rot"].reshape(J, 4)).astype(np.float32)
        unit = np.array([0, 1, 0, 0], np.float32) if fault == "unit1" else np.array([1, 0, 0, 0], np.float32)
        dev = (fk["local_rot"] - unit).astype(np.float32)
        if fk["coef"] is not None:
            dq = _f32(dq.astype(np.float64) + float(np.float32(fk["coef"])) * dev.astype(np.float64))
        gt = p["g_tr"].copy() if fk["g_tr"] else np.zeros(3, np.float32)
        if fk["gn"] is not None and fault != "no_gn_sum":
            if layered:
                s = np.zeros(3, np.float32)
                for j in range(J):
                    s = (s + fk["gn"][j]).astype(np.float32)
                gt = (gt + s).astype(np.float32)
            else:
                for j in range(J):
                    gt = (gt + fk["gn"][j]).astype(np.float32)
        out["dq"], out["dgt"] = dq, gt
        ss = np.float32(0)
        for x in (dev.reshape(-1) ** 2).astype(np.float32):
            ss = np.float32(ss + x)
        out["loss"] = np.array([ss / np.float32(4 * J)], np.float32)
        v = np.concatenate([dq.reshape(-1), gt]).astype(np.float32)
    vs = [None] * (d + 1)
    vs[d] = v
    for l in range(d, 0, -1):
        off = emb if l - 1 == c["skip"] else 0
        M = Ms[l][:, off: off + w]
        vl = vs[l].copy()
        if l == d and fault == "head256":
            vl[256:] = 0
        if l == d and fault == "no_tr_rows":
            vl[nr:] = 0
        n_rows = M.shape[0]
        if not layered:
            D = wave_gemv(np.ascontiguousarray(M.T), vl, 5, perm)
        else:
            D = np.zeros(w, np.float32)
            bys = list(range(8))
            if order == "reversed":
                bys = bys[::-1]
            elif order is not None:
                bys = list(np.random.default_rng(order).permutation(8))
            for by in bys:
                parts = []
                for wave in range(4):
                    acc = np.zeros(w, np.float32)
                    for r in range(by * 4 + wave, n_rows, 32):
                        acc = _f32(acc.astype(np.float64) + M[r].astype(np.float64) * float(vl[r]))
                    parts.append(acc)
                D = (D + (((parts[0] + parts[1]).astype(np.float32) + parts[2]).astype(np.float32) + parts[3]).astype(np.float32)).astype(np.float32)
        ml = l - 1
        if fault == "mask_next" and l - 1 == d // 2 and l < d:
            ml = l
        alive = acts[emb + ml * w: emb + (ml + 1) * w] > 0
        vs[l - 1] = np.where(alive, D, np.float32(0)).astype(np.float32)
        if fault == "stale" and prev is not None and l - 1 == d // 2:
            pv = prev["flat"][lay[l - 1][1]: lay[l - 1][1] + w]
            k = _pick(np.abs(vs[l - 1] - pv), pick)
            vs[l - 1][k] = pv[k]
    for m in range(d + 2):
        l = min(m, d)
        x = inp(l) if fault in ("emb_behind", "skip_late") else layer_input(c, acts, l)
        vm = vs[l] if m < d else (vs[d][:nr] if m == d else vs[d][nr:])
        w_off, b_off, rows, n = lay[m]
        xx = x.copy()
        if fault == "dw_emb_from_h" and m == c["skip"] + 1 and m < d:
            xx[:emb] = xx[emb: 2 * emb]
        flat[w_off: w_off + rows * n] = (vm[:, None] * xx[None, :]).astype(np.float32).reshape(-1)
        flat[b_off: b_off + rows] = vm
        if fault == "late_row":
            first = np.arange(0, rows, 8) if m != d + 1 else np.arange((-nr) % 8, rows, 8)
            for r in first:
                flat[w_off + r * n: w_off + (r + 1) * n] = np.nan
                flat[b_off + r] = np.nan
    out["flat"] = flat
    return out


FAULTS = ("emb_behind", "skip_late", "chunk5", "head_bias", "rot_bias_idx", "sincos", "freq", "mask_next", "head256", "no_tr_rows",
          "dw_emb_from_h", "late_row", "stale", "no_gn_sum", "no_g_rot", "unit1")


# ------------------------------------------------------------------------------------------------------------------ the grid
def _c(name, width, J, depth=8, skip=None, multires=8, seed=None, **kw):
    return dict(name=name, width=width, J=J, depth=depth, skip=skip, multires=multires, seed=seed, kw=kw)


def _fk(topo="tree", transforms=True, g_rot=True, g_tr=True, gn=True, coef=0.003, loss=True, outs=True):
    return dict(topo=topo, transforms=transforms, g_rot=g_rot, g_tr=g_tr, gn=gn, coef=coef, loss=loss, outs=outs)


def grid():
    """The cases of tests/test_gpu_pose_mlp_f64.py (and, on the restatement, of tests/test_pose_mlp_ref_cpu.py).  ``sync``: a
    persistent sync_state (default) or NULL."""
    G = []
    # dispatch: heads inside the width | head workgroups of their own | both sides of each rule | layered by size
    for w, J in ((256, 24), (256, 63), (64, 15), (64, 8), (32, 7), (20, 4), (9, 1), (8, 1), (7, 1)):
        G.append(_c("inside %dx%d" % (w, J), w, J, sync=(w, J) != (64, 8)))
    for w, J in ((256, 64), (248, 64), (200, 64), (128, 64), (128, 32)):
        G.append(_c("extra %dx%d" % (w, J), w, J, sync=(w, J) != (128, 32)))
    for w, J in ((128, 31), (127, 32), (32, 8)):
        G.append(_c("rule %dx%d" % (w, J), w, J))
    for w, J in ((256, 65), (256, 128), (256, 256), (32, 128)):
        G.append(_c("size %dx%d" % (w, J), w, J))
    # lane and granule edges
    for w in (63, 64, 65, 127, 129, 191, 192, 193, 255):
        G.append(_c("width %d" % w, w, min(24, (w - 3) // 4)))
    for w in (129, 193, 255):
        G.append(_c("width %d extra" % w, w, 64))
    for w in (47, 48, 111, 112, 239, 240):
        G.append(_c("width+emb %d" % (w + 17), w, min(24, (w - 3) // 4)))
    G.append(_c("width+emb 319", 256, 24, multires=31))
    G.append(_c("width+emb 319 extra", 256, 64, multires=31, skip=7))
    # structure
    for d in (1, 2, 3, 12):
        for s in sorted({-1, 0, max(d - 2, 0), d - 1}):
            G.append(_c("depth %d skip %d" % (d, s), 40, 6, depth=d, skip=s))
    G.append(_c("depth 12 wide", 256, 64, depth=12, skip=11))
    G.append(_c("depth 1 wide", 256, 64, depth=1, skip=0))
    for m in (0, 1, 31):
        G.append(_c("multires %d" % m, 64, 8, multires=m))
        G.append(_c("multires %d skip last" % m, 136, 33, multires=m, skip=7))
    # inputs
    for i, t in enumerate((0.0, 1e-3, 0.37, 1.0, -0.5)):
        G.append(_c("t=%g" % t, (72, 256, 24, 136, 64)[i], (8, 24, 4, 64, 15)[i], t=t, rot_bias=i % 2 == 0))
    for i, cot in enumerate(("zero", "row", "rot", "tr")):
        G.append(_c("cot %s" % cot, (64, 256, 136, 64)[i], (8, 64, 33, 15)[i], cot=cot, rot_bias=i % 2 == 1, sync=i != 1))
    G.append(_c("dead layer", 64, 8, dead_layer=5))
    G.append(_c("dead layer wide", 256, 64, dead_layer=3, rot_bias=False))
    # the _fk entry: each option on both paths (J <= 64 one launch — and again layered by option —, J = 65, 256 layered)
    G.append(_c("fk J=1", 16, 1, fk=_fk("chain", transforms=False, coef=None)))
    G.append(_c("fk J=2", 16, 2, fk=_fk("chain", g_rot=False, loss=False)))
    G.append(_c("fk J=24", 256, 24, fk=_fk("tree")))
    G.append(_c("fk J=24 bare", 256, 24, fk=_fk("tree", transforms=False, g_rot=False, g_tr=False, gn=False, coef=None, loss=False)))
    G.append(_c("fk J=63", 256, 63, fk=_fk("star", coef=0.0, outs=False)))
    G.append(_c("fk J=64", 256, 64, fk=_fk("tree", g_tr=False), sync=False))
    G.append(_c("fk J=64 narrow", 128, 64, fk=_fk("tree", gn=False, coef=None, loss=True)))
    G.append(_c("fk J=65", 256, 65, fk=_fk("tree", transforms=False)))
    G.append(_c("fk J=65 bare", 64, 65, fk=_fk("star", g_rot=False, g_tr=False, gn=False, coef=None, loss=False)))
    G.append(_c("fk J=256", 256, 256, fk=_fk("tree", coef=0.0)))
    G.append(_c("fk J=256 loss only", 32, 256, fk=_fk("star", g_rot=False, coef=None, loss=True)))
    for case in G:
        if case["seed"] is None:
            case["seed"] = zlib.crc32(case["name"].encode()) % 100000  # (a case keeps its inputs when the grid grows)
    return G


# further (case, t) pairs of the GPU tests (three launches on one sync_state; the embedding measurement): held to the same host
# assertion as the grid (tests/test_pose_mlp_ref_cpu.py)
STATE_TS = (0.37, -0.5, 1e-3)
STATE_CASES = ("inside 256x24", "extra 200x64", "inside 9x1")
EMBED_TS = (0.0, 1e-3, 0.37, 1.0, -0.5)
EMBED_CASE = "multires 31"


def random_case(seed):
    """One seeded draw over all of the above."""
    g = np.random.default_rng(7000 + seed)
    depth = int(g.choice([1, 2, 3, 5, 8, 12]))
    width = int(g.choice([8, 20, 33, 64, 100, 128, 129, 200, 255, 256]))
    J = int(g.choice([1, 2, 5, 17, 24, 32, 63, 64, 65, 100]))
    multires = int(g.choice([0, 1, 4, 8, 15, 31]))
    skip = int(g.integers(-1, depth))
    fk = None
    if g.random() < 0.5:
        fk = _fk(str(g.choice(["chain", "tree", "star", "broom"] if J <= 8 else ["tree", "star"])), bool(g.integers(2)), bool(g.integers(2)), bool(g.integers(2)),
                 bool(g.integers(2)), [None, 0.0, 0.01][int(g.integers(3))], bool(g.integers(2)), True)
    return _c("draw %d" % seed, width, J, depth=depth, skip=skip, multires=multires, seed=9000 + seed,
              t=float(g.choice([0.0, 1e-3, 0.37, 1.0, -0.5])), rot_bias=bool(g.integers(2)),
              cot=str(g.choice(["random", "random", "row", "rot", "tr"])), fk=fk, sync=bool(g.integers(4)))


def make(case):
    """(c, p) of a grid case.  The _fk inputs come from tests.test_gpu_wideskel_f64.skeleton."""
    c = cfg(case["width"], case["J"], case["depth"], case["skip"], case["multires"])
    kw = dict(case["kw"])
    kw.pop("sync", None)
    fk = kw.pop("fk", None)
    p = build(c, case["seed"], name=case["name"], **kw)
    if fk is not None:
        from tests.test_gpu_wideskel_f64 import skeleton
        g = torch.Generator().manual_seed(case["seed"])
        J = c["J"]
        joints, parents, q, _, _ = skeleton(J, fk["topo"], g)
        f = dict(fk)
        f.update(local_rot=q.numpy().astype(np.float32), joints=joints.numpy().astype(np.float32), parents=parents.numpy().astype(np.int64),
                 dG=torch.randn(J, 12, generator=g).numpy(), gn=torch.randn(J, 3, generator=g).numpy() if fk["gn"] else None)
        p["fk"] = f
    return c, p


def assert_case_is_safe(c, p, layered):
    """The host assertion on the float32 restatement: no ReLU decision within its accumulated error of 0."""
    ref, _, zerr = accumulated(c, p, layered)
    r = restate(c, p, layered)
    assert relu_decisions_safe(ref, zerr, r["acts"], c), "a unit is within its accumulated error of 0: add the case to RESEED"
