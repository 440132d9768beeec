"""The float64 reference of the fused MLP heads' GPU tests (tests/mlp_ref.py) on the host: it accepts a torch emulation of the
kernels' arithmetic (fp32 products of the same 16-bit operands, then rounded) and rejects each of the errors those tests are there
to catch — one element 2 ulps off, the ragged last rows zeroed, two 8-column groups swapped inside one 32-row tile, a ReLU mask bit
flipped, an fp32 output 1e-5 off — so a passing GPU test means the kernel is right to within its own rounding."""
import pytest
import torch

from tests import mlp_ref as R

N, H, OUT = 161, 64, 8  # 161 rows: one whole 128-row workgroup and a ragged one of 33


def _operands(dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    d_above = (torch.randn(N, H, generator=g) * 3.0).to(dtype)           # the layer above's data gradient (16-bit, as stored)
    w = (torch.randn(H, H, generator=g) / H ** 0.5).to(dtype)            # W_{l+1}[:, hidden part]: (units above, units here)
    act = torch.relu(torch.randn(N, H, generator=g)).to(dtype)          # this layer's stored activations: about half are 0
    return d_above, w, act


def _dgrad(dtype, seed=0):
    """(kernel stand-in, reference, bound, must_zero, may_zero, act) of one layer's data gradient."""
    d_above, w, act = _operands(dtype, seed)
    got = ((d_above.float() @ w.float()) * (act > 0)).to(dtype)
    ref, s = R.product(d_above, w.t())
    bnd = R.bound(ref, s, H, dtype)
    must, may = R.relu_mask_rule(act, dtype)
    return got, ref, bnd, must, may, act


def _rejects(got, ref, bnd, must=None, may=None):
    n_bad, _worst, _first = R.violations(got, ref, bnd, must, may)
    with pytest.raises(AssertionError):
        R.assert_within("mutated", got, ref, bnd, must, may)
    return n_bad > 0


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_reference_accepts_the_emulated_kernel(dtype):
    got, ref, bnd, must, may, _act = _dgrad(dtype)
    worst = R.assert_within("dpre", got, ref, bnd, must, may)
    assert 0.0 < worst <= 1.0


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_reference_rejects_an_element_two_ulps_off(dtype):
    got, ref, bnd, must, may, act = _dgrad(dtype)
    i = int(torch.argmax((ref.abs() * (act > 0)).flatten()))
    bad = got.clone()
    bad.view(torch.int16).view(-1)[i] += 2
    assert _rejects(bad, ref, bnd, must, may)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_reference_rejects_zeroed_ragged_rows(dtype):
    got, ref, bnd, must, may, _act = _dgrad(dtype)
    bad = got.clone()
    bad[128:] = 0
    assert _rejects(bad, ref, bnd, must, may)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_reference_rejects_swapped_column_groups_in_one_tile(dtype):
    got, ref, bnd, must, may, _act = _dgrad(dtype)
    bad = got.clone()
    bad[32:64, 8:16], bad[32:64, 16:24] = got[32:64, 16:24], got[32:64, 8:16]
    assert _rejects(bad, ref, bnd, must, may)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_reference_rejects_a_flipped_mask_bit(dtype):
    got, ref, bnd, must, may, act = _dgrad(dtype)
    i = int(torch.argmax((ref.abs() * (act > 0)).flatten()))
    bad = got.clone()
    bad.view(-1)[i] = 0  # the unit passed (act > 0), the kernel dropped it
    assert _rejects(bad, ref, bnd, must, may)
    if dtype == torch.bfloat16:  # and the other way: a unit masked in the forward (act == 0) that lets its gradient through
        j = int(torch.argmax((ref.abs() * (act == 0)).flatten()))
        bad = got.clone()
        bad.view(-1)[j] = ref.view(-1)[j].to(dtype)
        assert _rejects(bad, ref, bnd, must, may)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_reference_rejects_an_output_off_by_1e5_relative(dtype):
    """The head's fp32 output ``act @ W_out^T + b_out`` (K = 64 + 1 terms: the accumulation term of the bound is 3.9e-6 S)."""
    _d, _w, act = _operands(dtype)
    g = torch.Generator().manual_seed(1)
    w_out = (torch.randn(OUT, H, generator=g) / H ** 0.5).to(dtype)
    b_out = torch.randn(OUT, generator=g) * 0.1
    got = act.float() @ w_out.float().t() + b_out
    ref, s = R.product(act, w_out, b_out)
    bnd = R.bound(ref, s, H + 1)
    worst = R.assert_within("out", got, ref, bnd)
    assert worst < 1.0
    i = int(torch.argmax((ref.abs() / s).flatten()))
    bad = got.clone()
    bad.view(-1)[i] *= 1.0 + 1e-5
    assert _rejects(bad, ref, bnd)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_reference_of_the_forward_activations(dtype):
    """relu(a @ W^T + b) rounded: accepted; one element 2 ulps off: rejected."""
    d_above, w, act = _operands(dtype, seed=2)
    b = torch.randn(H) * 0.1
    got = torch.relu(act.float() @ w.float().t() + b).to(dtype)
    pre, s = R.product(act, w, b)
    ref = torch.relu(pre)
    bnd = R.bound(ref, s, H + 1, dtype)
    R.assert_within("act", got, ref, bnd)
    i = int(torch.argmax(ref.flatten()))
    bad = got.clone()
    bad.view(torch.int16).view(-1)[i] += 2
    assert _rejects(bad, ref, bnd)


def _encode_masks(m):
    """The forward kernel's push loop (csrc/mlp.hip, mlp_forward_kernel) written out: (n, 256) bool -> (workgroups, 256, 4) int32."""
    wgs = (m.shape[0] + 127) // 128
    full = torch.zeros(wgs * 128, 256, dtype=torch.bool)
    full[:m.shape[0]] = m
    out = torch.zeros(wgs, 256, 4, dtype=torch.int64)
    for wg in range(wgs):
        blk = full[128 * wg:128 * (wg + 1)].tolist()
        for tid in range(256):
            lane, wave = tid % 64, tid // 64
            for gt in range(4):
                word = 0
                for nt in range(2):
                    for q in range(4):
                        for j in range(4):
                            unit = 64 * wave + 32 * nt + 8 * q + 4 * (lane // 32) + j
                            word = (word << 1) | int(blk[32 * gt + lane % 32][unit])
                out[wg, tid, gt] = word
    return torch.where(out >= 2 ** 31, out - 2 ** 32, out).to(torch.int32)


def test_mask_record_decodes_to_the_units_it_was_pushed_from():
    g = torch.Generator().manual_seed(4)
    m = torch.rand(N, 256, generator=g) < 0.5
    rec = _encode_masks(m)[None]
    assert torch.equal(R.decode_masks(rec, N)[0], m)
