"""GPU: farthest-point sampling over rows of D floats (csrc/fps.hip riggs_fps_sample_rows, riggs_amd/fps.py
farthest_point_sample_rows) — the indices are EXACTLY the reference's for every fixture (tests/golden/fpsrows_*.npz, each with its
margin to a tie: tests/test_fps_rows_cpu.py), exactly the 3-column kernel's at D = 3, and exactly those of the sequential fp32
restatement (tests/fps_rows_ref.py) on a cloud of many workgroups; strides, batches, starts and refusals as the 3-column sampler."""
import numpy as np
import pytest
import torch

from tests import fps_rows_ref as R
from tests import skeleton_init_ref as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", R.FIXTURES)
def test_indices_equal_the_reference_and_repeat(name):
    from riggs_amd.fps import farthest_point_sample_rows
    rows, start, ref = R.fixture(name)
    x = torch.from_numpy(rows).cuda()[None]
    got = farthest_point_sample_rows(x, len(ref), start=[start])
    assert got.dtype == torch.int64 and got.shape == (1, len(ref)) and got.is_cuda
    again = farthest_point_sample_rows(x, len(ref), start=torch.tensor([start], device="cuda"))
    got, again = got.cpu().numpy()[0], again.cpu().numpy()[0]
    wrong = np.flatnonzero(got != ref)
    print(name, "rows", rows.shape, "picks", len(ref), "mismatches", len(wrong))
    assert len(wrong) == 0, (name, wrong[:5], got[wrong[:5]], ref[wrong[:5]])
    assert np.array_equal(got, again)
    if name == "fpsrows_n2050x2_d48_p20":
        assert int(got[1:].max()) < 2050  # equal distances in different workgroups: the lower index
    if name == "fpsrows_same300_d48_p5":
        assert got.tolist() == [start, 0, 0, 0, 0]


@pytest.mark.parametrize("name", ("fps_n70001_p64", "fps_n200_p200", "fps_n2050x2_p40", "ragged3001"))
def test_three_columns_give_the_three_column_kernels_indices(name):
    from riggs_amd.fps import farthest_point_sample, farthest_point_sample_rows
    if name == "ragged3001":  # three workgroups of the 3-column kernel, the last one ragged; twelve of the wide one
        x, start, npoint = torch.randn(1, 3001, 3, generator=torch.Generator().manual_seed(21)).cuda(), 1234, 48
    else:
        pts, start, ref = S.fps_fixture(name)
        x, npoint = torch.from_numpy(pts).cuda()[None], len(ref)
    assert torch.equal(farthest_point_sample_rows(x, npoint, start=[start]), farthest_point_sample(x, npoint, start=[start]))


def test_many_workgroups_equal_the_restatement():
    from riggs_amd.fps import farthest_point_sample_rows
    g = torch.Generator(device="cuda").manual_seed(31)
    x = torch.randn(1, 70001, 48, generator=g, device="cuda")
    got = farthest_point_sample_rows(x, 64, start=[45678])[0].cpu().numpy()
    ref = R.fps_rows(x[0].cpu().numpy(), 45678, 64)  # the same summation order: no margin needed
    assert np.array_equal(got, ref), np.flatnonzero(got != ref)[:5]
    assert len(set(got.tolist())) == 64


def test_strides_batches_starts_and_refusals():
    from riggs_amd import _lib as L
    from riggs_amd import gaussian_model as GM
    from riggs_amd.fps import farthest_point_sample, farthest_point_sample_rows
    g = torch.Generator().manual_seed(32)
    x = torch.randn(1, 2500, 48, generator=g).cuda()
    direct = farthest_point_sample_rows(x, 33, start=[7])
    assert np.array_equal(direct[0].cpu().numpy(), R.fps_rows(x[0].cpu().numpy(), 7, 33))
    # one cloud of wide rows on the device is routed to the wide sampler
    assert torch.equal(GM.farthest_point_sample(x, 33, start=[7]), direct)
    # rows 50 floats apart (a view into a wider tensor) are read in place
    wide = torch.full((1, 2500, 50), 1e6, device="cuda")
    wide[..., :48] = x
    view = wide[..., :48]
    assert view.stride(1) == 50 and torch.equal(farthest_point_sample_rows(view, 33, start=[7]), direct)
    # batches run one after the other
    y = torch.randn(1, 2500, 48, generator=g).cuda()
    both = farthest_point_sample_rows(torch.cat([x, y]), 33, start=[7, 11])
    assert torch.equal(both[0], direct[0]) and torch.equal(both[1], farthest_point_sample_rows(y, 33, start=[11])[0])
    # a random start: in range, first in the output, and the RNG draw the torch loop would make
    torch.manual_seed(5)
    a = GM.farthest_point_sample(x, 9)
    torch.manual_seed(5)
    s = torch.randint(0, 2500, (1,), dtype=torch.long, device="cuda")
    assert int(a[0, 0]) == int(s) and torch.equal(a, farthest_point_sample_rows(x, 9, start=s))
    # more picks than rows repeats indices, as the reference's loop does; nothing is read past the cloud
    few = farthest_point_sample_rows(x[:, :5], 8, start=[2])
    assert few.shape == (1, 8) and int(few.max()) < 5 and sorted(set(few[0, :5].tolist())) == [0, 1, 2, 3, 4]
    assert farthest_point_sample_rows(x, 0).shape == (1, 0)
    with pytest.raises(L.RiggsHipError):
        farthest_point_sample_rows(torch.zeros(1, 10, 65, device="cuda"), 4)
    with pytest.raises(L.RiggsHipError):
        farthest_point_sample_rows(x.cpu(), 4)
    with pytest.raises(L.RiggsHipError):
        farthest_point_sample_rows(x.double(), 4)
    with pytest.raises(L.RiggsHipError):
        farthest_point_sample_rows(torch.zeros(1, 10, 0, device="cuda"), 4)
    with pytest.raises(L.RiggsHipError):  # the 3-column sampler keeps refusing other widths
        farthest_point_sample(torch.zeros(1, 10, 5, device="cuda"), 4)
