"""GPU: farthest-point sampling (csrc/fps.hip, riggs_amd/fps.py) — the indices are EXACTLY the reference's
(utils/time_utils.py:461-482 on the CPU, tests/golden/fps_*.npz) for every fixture, ties included; runs repeat; a case without
ties equals the torch loop on the device; gaussian_model.farthest_point_sample routes to the kernel."""
import numpy as np
import pytest
import torch

from tests import skeleton_init_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", R.FPS_FIXTURES)
def test_indices_equal_the_reference_and_repeat(name):
    from riggs_amd.fps import farthest_point_sample
    pts, start, ref = R.fps_fixture(name)
    x = torch.from_numpy(pts).cuda()[None]
    got = farthest_point_sample(x, len(ref), start=[start])
    assert got.dtype == torch.int64 and got.shape == (1, len(ref)) and got.is_cuda
    again = farthest_point_sample(x, len(ref), start=torch.tensor([start], device="cuda"))
    got, again = got.cpu().numpy()[0], again.cpu().numpy()[0]
    wrong = np.flatnonzero(got != ref)
    print(name, "points", pts.shape[0], "picks", len(ref), "mismatches", len(wrong))
    assert len(wrong) == 0, (name, wrong[:5], got[wrong[:5]], ref[wrong[:5]])
    assert np.array_equal(got, again)
    if name == "fps_n200_p200":
        assert sorted(got.tolist()) == list(range(200))
    if name == "fps_n2050x2_p40":
        assert int(got[1:].max()) < 2050  # equal distances in two workgroups: the lower index
    if name == "fps_same300_p5":
        assert got.tolist() == [start, 0, 0, 0, 0]


def test_a_case_without_ties_equals_the_torch_loop_on_the_device():
    from riggs_amd.fps import farthest_point_sample
    from riggs_amd.gaussian_model import farthest_point_sample_torch
    g = torch.Generator().manual_seed(21)
    x = torch.randn(1, 3001, 3, generator=g).cuda()  # three workgroups, the last one ragged
    got = farthest_point_sample(x, 48, start=[1234])
    ref = farthest_point_sample_torch(x, 48, start=[1234])
    assert torch.equal(got, ref)
    assert len(set(got[0].tolist())) == 48


def test_routed_sampler_strides_batches_and_random_start():
    from riggs_amd import _lib as L
    from riggs_amd import gaussian_model as GM
    from riggs_amd.fps import farthest_point_sample
    g = torch.Generator().manual_seed(22)
    x = torch.randn(1, 2500, 3, generator=g).cuda()
    direct = farthest_point_sample(x, 33, start=[7])
    assert torch.equal(GM.farthest_point_sample(x, 33, start=[7]), direct)
    # rows 4 floats apart (a view into a wider tensor) are read in place
    wide = torch.zeros(1, 2500, 4, device="cuda")
    wide[..., :3] = x
    assert torch.equal(farthest_point_sample(wide[..., :3], 33, start=[7]), direct)
    # batches run one after the other
    y = torch.randn(1, 2500, 3, generator=g).cuda()
    both = farthest_point_sample(torch.cat([x, y]), 33, start=[7, 11])
    assert torch.equal(both[0], direct[0]) and torch.equal(both[1], farthest_point_sample(y, 33, start=[11])[0])
    # a random start: in range, first in the output, and the RNG draw the torch loop made
    torch.manual_seed(5)
    a = GM.farthest_point_sample(x, 9)
    torch.manual_seed(5)
    s = torch.randint(0, 2500, (1,), dtype=torch.long, device="cuda")
    assert int(a[0, 0]) == int(s) and torch.equal(a, farthest_point_sample(x, 9, start=s))
    # more picks than points repeats indices, as the reference's loop does; nothing is read past the cloud
    few = farthest_point_sample(x[:, :5], 8, start=[2])
    assert few.shape == (1, 8) and int(few.max()) < 5 and sorted(set(few[0, :5].tolist())) == [0, 1, 2, 3, 4]
    assert farthest_point_sample(x, 0).shape == (1, 0)
    with pytest.raises(L.RiggsHipError):
        farthest_point_sample(x.cpu(), 4)
    with pytest.raises(L.RiggsHipError):
        farthest_point_sample(torch.zeros(1, 10, 5, device="cuda"), 4)
