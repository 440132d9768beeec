"""CPU: the marshalling the pose -> kinematic chain -> skinning nodes share (riggs_amd/skeleton.py): the two small-block
layouts handed to the kernels, the PoseMLP's parameter list in the C entries' order, the scalar motion mask, the split of the
flat PoseMLP gradient.  No GPU, no library call."""
import pytest
import torch

from riggs_amd import skeleton as SK

JOINTS = (2, 24, 64, 65, 256)


def _check_block(views, flat, n_floats, shapes, aligned):
    """``views`` carved out of ``flat``: the stated shapes, pairwise disjoint, inside the first ``n_floats`` floats, and the
    first ``aligned`` of them on 16-byte boundaries relative to the block's base."""
    assert [tuple(v.shape) for v in views] == list(shapes)
    spans = []
    for v in views:
        assert v.dtype == torch.float32 and v.is_contiguous()
        assert v.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr()
        start = v.storage_offset() - flat.storage_offset()
        spans.append((start, start + v.numel()))
    for i, (a0, a1) in enumerate(spans):
        assert 0 <= a0 < a1 <= n_floats
        for b0, b1 in spans[i + 1:]:
            assert a1 <= b0 or b1 <= a0
    for a0, _ in spans[:aligned]:
        assert (4 * a0) % 16 == 0


@pytest.mark.parametrize("J", JOINTS)
def test_forward_block_layout(J):
    n = SK._pose_block_floats(J)
    assert n == 23 * J + 4
    # (a slice of a larger buffer at an offset, as _FrameFn and _PoseDeform hand it over)
    flat = torch.zeros(64 + n)[64:]
    views = SK._pose_block(flat, J)
    _check_block(views, flat, n, [(J, 4), (J, 12), (J, 4), (J, 3), (3,)], aligned=3)
    assert [v.storage_offset() - 64 for v in views] == [0, 4 * J, 16 * J, 20 * J, 23 * J]


@pytest.mark.parametrize("J", JOINTS)
def test_backward_block_layout(J):
    n = SK._pose_grad_block_floats(J)
    assert n == 16 * J + 8
    flat = torch.zeros(n)
    views = SK._pose_grad_block(flat, J)
    _check_block(views, flat, n, [(J, 12), (J, 4), (3,), (3,)], aligned=4)
    assert [v.storage_offset() for v in views] == [0, 12 * J, 16 * J, 16 * J + 4]


def _net():
    return SK.PoseMLP(1, 24 * 4, depth=3, hidden_dimensions=32)


def test_parameter_list_is_the_modules_own_in_c_order():
    net = _net()
    expect = []
    for layer in net.net:
        expect += [layer.weight, layer.bias]
    expect += [net.rotation_predictor.weight, net.rotation_predictor.bias, net.translation_predictor.weight,
               net.translation_predictor.bias]
    got = net.c_params()
    assert len(got) == len(expect) == 2 * 3 + 4
    assert all(g is e for g, e in zip(got, expect))


def test_handoff_buffer_is_not_handed_to_another_device():
    net = _net()  # (its buffer is on the CPU: a launch on a GPU must get None, and no library call is made to find that out)
    assert net.handoff(torch.device("cuda", 0)) is None


def test_scalar_motion_mask():
    N, dev = 7, torch.device("cpu")
    assert SK._mask_tensor(None, N, dev) is None
    assert SK._mask_tensor(1.0, N, dev) is None
    m = SK._mask_tensor(0.5, N, dev)
    assert tuple(m.shape) == (N, 1) and m.dtype == torch.float32 and bool((m == 0.5).all())
    t = torch.rand(N, 1)
    assert SK._mask_tensor(t, N, dev) is t


def test_zero_scaling_is_cached_per_size():
    net = _net()
    z = SK._zero_scaling(net, 5, torch.device("cpu"))
    assert tuple(z.shape) == (5, 3) and not bool(z.any())
    assert SK._zero_scaling(net, 5, torch.device("cpu")) is z
    assert tuple(SK._zero_scaling(net, 6, torch.device("cpu")).shape) == (6, 3)


def test_split_returns_views_of_the_flat_gradient():
    params = _net().c_params()
    flat = torch.arange(sum(p.numel() for p in params), dtype=torch.float32)
    grads = SK._split_grads(flat, params)
    assert len(grads) == len(params)
    o = 0
    for g, p in zip(grads, params):
        assert g.shape == p.shape
        assert g.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr() and g.storage_offset() == o
        assert torch.equal(g.reshape(-1), flat[o:o + p.numel()])
        o += p.numel()
    assert o == flat.numel()
