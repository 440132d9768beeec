"""Float64 references of the fused MLP heads' products (riggs_amd/mlp.py, csrc/mlp.hip) with a rigorous per-element bound.

Every reference is built from the SAME 16-bit operands the kernel reads (the fp32 masters rounded with ``.to(dtype)``: the
round-to-nearest-even of f2h) and from the kernel's own stored input of the layer.  A product of two 16-bit numbers is exact in
float64 and a float64 sum of a few hundred of them is exact to ~1e-14, so what is left between kernel and reference is the
kernel's fp32 accumulation and the final rounding of the result to 16 bits.  For y = A @ B^T over K terms (a bias add counts as
one more term):

    S     = |A| @ |B|^T (+ |bias|)                       (float64)
    gam   = K * 2^-24                                     (fp32 accumulation, any order)
    |got - ref| <= gam * S + u16 * (|ref| + gam * S) + sub16

with u16 = 2^-11 (fp16) / 2^-8 (bf16) for a result stored in 16 bits and 0 for an fp32 result; sub16 = 2^-25 (half of fp16's
subnormal spacing) for fp16 results, 0 for bf16 (fp32's range).  ReLU is 1-Lipschitz and commutes with the rounding, so the same
bound holds for relu(y) with |relu(ref)| in place of |ref|.

The ReLU mask of the data gradient: the kernel keeps a unit where its fp32 pre-activation rounds to a non-zero 16-bit value, so
``act > 0`` means the unit passed; where ``act == 0`` a bf16 unit was masked (exact 0), and an fp16 unit may have a positive
pre-activation below the smallest subnormal: there exact 0 or the unmasked value within its bound is accepted, nothing else.

Pure torch on whatever device the tensors live on: the GPU tests run it on the device, tests/test_mlp_ref_cpu.py shows on the
host that it rejects the errors the GPU tests are there to catch.
"""
import torch

EPS32 = 2.0 ** -24
U16 = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
SUB16 = {torch.float16: 2.0 ** -25, torch.bfloat16: 0.0}


def product(a, b, bias=None):
    """``a @ b^T (+ bias)`` and ``|a| @ |b|^T (+ |bias|)`` in float64 (a: (N, K), b: (M, K), bias: (M) or None)."""
    a64, b64 = a.double(), b.double()
    ref = a64 @ b64.t()
    s = a64.abs() @ b64.abs().t()
    if bias is not None:
        ref = ref + bias.double()
        s = s + bias.double().abs()
    return ref, s


def bound(ref, s, k, dtype=None, extra=0.0):
    """The per-element bound of a K-term fp32 sum ``ref`` (float64) with absolute sum ``s``, rounded to ``dtype`` (float16 /
    bfloat16; None: an fp32 result); ``extra`` (broadcast) is added to the accumulation error (an fp32 input of its own)."""
    gs = (k * EPS32) * s + extra
    if dtype is None:
        return gs
    return gs + U16[dtype] * (ref.abs() + gs) + SUB16[dtype]


def relu_mask_rule(act, dtype):
    """(must_be_zero, may_be_zero) for the data gradient of a layer whose stored activations are ``act``."""
    dead = act == 0
    if dtype == torch.bfloat16:
        return dead, torch.zeros_like(dead)
    return torch.zeros_like(dead), dead


def violations(got, ref, bnd, must_zero=None, may_zero=None):
    """(elements outside the bound, worst err / bound, first violating index or None).  ``must_zero``: the element is exactly 0;
    ``may_zero``: exact 0 is accepted besides ``ref`` within the bound.  NaN anywhere is a violation."""
    g = got.double()
    err = (g - ref).abs()
    bnd = torch.broadcast_to(torch.as_tensor(bnd, dtype=torch.float64, device=g.device), g.shape)
    ok = err <= bnd
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err))
    if may_zero is not None:
        z = may_zero & (g == 0)
        ok = ok | z
        ratio = torch.where(z, torch.zeros_like(ratio), ratio)
    if must_zero is not None:
        ok = torch.where(must_zero, g == 0, ok)
        ratio = torch.where(must_zero, torch.where(g == 0, torch.zeros_like(ratio), torch.full_like(ratio, float("inf"))), ratio)
    ratio = torch.where(torch.isnan(g), torch.full_like(ratio, float("inf")), ratio)
    bad = ~ok
    n_bad = int(bad.sum())
    worst = float(ratio.max()) if ratio.numel() else 0.0
    first = None
    if n_bad:
        first = tuple(int(i) for i in torch.nonzero(bad)[0])
    return n_bad, worst, first


def assert_within(what, got, ref, bnd, must_zero=None, may_zero=None, stats=None):
    """``violations`` == 0, or an AssertionError naming the first element outside; returns the worst err / bound and appends
    ``(what, elements, fraction outside, worst err / bound, fraction outside)`` to ``stats`` (tests.gpu_util.STATS)."""
    n_bad, worst, first = violations(got, ref, bnd, must_zero, may_zero)
    if stats is not None:
        stats.append((what + " [err/bound]", int(got.numel()), n_bad / max(1, got.numel()), worst, n_bad / max(1, got.numel())))
    if n_bad:
        b = torch.broadcast_to(torch.as_tensor(bnd, dtype=torch.float64, device=got.device), got.shape)
        raise AssertionError("%s: %d of %d elements outside the bound (worst err/bound %.3g); first at %s: got %r, ref %r, bound %.3g"
                             % (what, n_bad, got.numel(), worst, first, float(got[first]), float(ref[first]), float(b[first])))
    return worst


def decode_masks(masks, n):
    """The forward's ReLU-mask record (depth, workgroups, 256 threads, 4 words) int32 -> (depth, n, 256) bool.  Thread t = 64 w + lane
    holds, in word gt, bit 31 - (16 nt + 4 q + j) for row 32 gt + (lane & 31) of its workgroup's 128 and unit
    64 w + 32 nt + 8 q + 4 (lane >> 5) + j (the accumulator layout the bits were pushed in)."""
    depth, wgs = masks.shape[0], masks.shape[1]
    dev = masks.device
    t = torch.arange(256, device=dev)[:, None, None]
    gt = torch.arange(4, device=dev)[None, :, None]
    i = torch.arange(32, device=dev)[None, None, :]
    lane, w = t % 64, t // 64
    row = 32 * gt + lane % 32
    unit = 64 * w + 32 * (i // 16) + 8 * ((i // 4) % 4) + 4 * (lane // 32) + i % 4
    flat = (row * 256 + unit).reshape(-1)
    bits = (masks.to(torch.int64)[..., None] >> (31 - torch.arange(32, device=dev))) & 1
    out = torch.empty(depth, wgs, 128 * 256, dtype=torch.bool, device=dev)
    out[:, :, flat] = bits.reshape(depth, wgs, -1).bool()
    return out.reshape(depth, wgs * 128, 256)[:, :n]


# ---- the parameter gradients through the library (torch.bmm = hipBLASLt): what ``riggs_amd.mlp.param_grads`` replaced; the
# comparison tests/test_gpu_mlp.py and tools/mlp_kernel_time.py run beside it
def _wgrad(d: torch.Tensor, a: torch.Tensor, splits: int = 128) -> torch.Tensor:
    """d^T · a for d (N, M), a (N, K) in bf16 with fp32 output.  The reduction runs over N = 3e5 rows: one GEMM with
    K_gemm = N leaves the library without parallelism (0.63 ms at 256 x 256 outputs); a batched GEMM over `splits` row
    blocks plus a sum is 8x faster (0.08 ms)."""
    N = d.shape[0]
    n = N // splits
    if n < 64:
        return torch.mm(d.t(), a, out_dtype=torch.float32)
    main = n * splits
    out = torch.bmm(d[:main].view(splits, n, -1).transpose(1, 2), a[:main].view(splits, n, -1), out_dtype=torch.float32).sum(0)
    if main < N:
        out = out + torch.mm(d[main:].t(), a[main:], out_dtype=torch.float32)
    return out


def _wgrad_multi(d: torch.Tensor, a: torch.Tensor, splits: int = 128) -> torch.Tensor:
    """``_wgrad`` for a stack of layers: d (L, N, M), a (L, N, K) -> (L, M, K), one batched GEMM over L x splits blocks.

    The (layer, split) axes only merge into one batch axis without a copy when the split count divides N, so the
    divisor of N nearest ``splits`` is used; without one in [splits/2, 2*splits] the layers go one at a time."""
    Lr, N = d.shape[0], d.shape[1]
    best = 0
    for c in range(splits // 2, 2 * splits + 1):
        if N % c == 0 and abs(c - splits) < abs(best - splits):
            best = c
    if best == 0 or N // best < 64:
        return torch.stack([_wgrad(d[i], a[i], splits) for i in range(Lr)])
    n = N // best
    dm = d.view(Lr * best, n, d.shape[2])
    am = a.view(Lr * best, n, a.shape[2])
    return torch.bmm(dm.transpose(1, 2), am, out_dtype=torch.float32).view(Lr, best, d.shape[2], a.shape[2]).sum(1)


_ONES = {}


def _colsum(d: torch.Tensor) -> torch.Tensor:
    """Column sums of a tall bf16 matrix in fp32, as a (split-K) GEMM with a block of ones: torch's column reduction of a
    (3e5, 256) bf16 tensor takes 0.09 ms and of a (3e5, 23) fp32 one 0.6 ms; this is ~0.03 ms."""
    key = (d.device, d.shape[0], d.dtype)
    ones = _ONES.get(key)
    if ones is None:
        ones = _ONES[key] = torch.ones(d.shape[0], 8, dtype=d.dtype, device=d.device)
    return _wgrad(d, ones)[:, 0].contiguous()


def library_param_grads(p, xb: torch.Tensor, acts: torch.Tensor, dpre: torch.Tensor, db: torch.Tensor, g_out: torch.Tensor,
                        scale: torch.Tensor = None):
    """``riggs_amd.mlp.param_grads`` through library GEMMs (``p``: its ``Packed``; ``db`` from ``backward_data(..., bias_sums=True)``)."""
    # every layer's product with the previous layer's activations has the same shape — the skip layer's hidden block
    # included — so layers 1 .. depth - 1 are ONE batched split-K GEMM; the two products with the embedding stay single calls
    if p.tail_ch:
        raise ValueError("library_param_grads: the comparison path knows no constant tail")
    gws = [None] * p.depth
    ls = p.skip + 1
    xb = xb[:g_out.shape[0]]
    g_run = _wgrad_multi(dpre[1:p.depth], acts[0:p.depth - 1])
    for l in range(1, p.depth):
        gws[l] = g_run[l - 1]
    gws[0] = _wgrad(dpre[0], xb)[:, :p.in_ch]
    gws[ls] = torch.cat([_wgrad(dpre[ls], xb)[:, :p.in_ch], gws[ls]], 1)
    grads = []
    for l in range(p.depth):
        grads += [gws[l], db[l]]
    gob = torch.nn.functional.pad(g_out if scale is None else g_out * scale, (0, 32 - p.out_ch)).to(p.dtype)
    grads += [_wgrad(gob, acts[p.depth - 1])[:p.out_ch], _colsum(gob)[:p.out_ch]]
    if scale is not None:  # every product above carries the factor once: take it out again (a power of two: exact)
        grads = [g.contiguous() for g in grads]
        torch._foreach_mul_(grads, torch.reciprocal(scale).reshape(()))
    return grads
