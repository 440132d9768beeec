"""GPU: riggs_amd.thinning (csrc/thin.hip) against the NumPy restatement of the algorithm (tests/thin_ref.py), bit for bit —
everything is integer.  Every case runs on the LDS path and on the global-memory path (forced with ``_path`` at these small
sizes) with the device counters read back every iteration and every fourth."""
import numpy as np
import pytest
import torch

from tests import thin_ref as R

pytestmark = pytest.mark.gpu

# (name, _path, _check_every): PATH_LDS = 0, PATH_GLOBAL = 1
CONFIGS = [("lds", 0, 8), ("global-every-1", 1, 1), ("global-every-4", 1, 4)]
_config = pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
_ORACLE = {}


def _want(key, image, **kw):
    """The oracle's result for ``image``, computed once per key."""
    if key not in _ORACLE:
        s = R.thin_details(image, **kw)
        s[0].setflags(write=False)
        _ORACLE[key] = s
    return _ORACLE[key]


def _thin(image, cfg, **kw):
    from riggs_amd.thinning import thin
    x = torch.from_numpy(np.array(image)).cuda()  # (a copy: the shared inputs are read-only)
    return thin(x, _path=cfg[1], _check_every=cfg[2], **kw)


def _same(got, want):
    return got.dtype is torch.bool and torch.equal(got.cpu(), torch.from_numpy(np.array(want)))


def _noise(H, W, seed):
    return np.random.default_rng(seed).random((H, W)) < 0.5


@_config
@pytest.mark.parametrize("first", [0, 1])
def test_every_neighbourhood_with_either_table(cfg, first):
    """One sub-iteration over the 256 possible 3 x 3 patches with the centre set (5-pixel pitch: no patch sees another), with the
    first table and with the second: either of the two 256-entry decisions, whole."""
    patches = R.all_patches()
    want, _, subiters, hists = _want(("patches", first), patches, first_subiter=first, max_subiters=1, histograms=True)
    centres = R.codes(patches)[1::5, 1::5].ravel()
    assert subiters == 1 and np.array_equal(centres, np.arange(256)) and patches[1::5, 1::5].all()
    assert (hists[0] > 0).all()  # all 256 codes occur at a set pixel of this sub-iteration's input
    # ... and the oracle deletes exactly the table's 37 centres
    assert int((~want[1::5, 1::5]).sum()) == 37 and np.array_equal(~want[1::5, 1::5].ravel(), R.TABLES[first])
    assert _same(_thin(patches, cfg, _first_subiter=first, _max_subiters=1), want)


WIDTHS, HEIGHTS = (1, 31, 32, 33, 63, 64, 65, 97), (1, 2, 3, 40)


@_config
def test_word_and_border_edges(cfg):
    """Widths around the 32-pixel word (1, 31, 32, 33, 63, 64, 65, 97) x heights 1, 2, 3, 40: all ones and seeded noise, to
    convergence and after one sub-iteration of either table."""
    for H in HEIGHTS:
        for W in WIDTHS:
            for name, image in (("ones", np.ones((H, W), dtype=bool)), ("noise", _noise(H, W, 1000 * H + W))):
                want = _want((name, H, W), image)[0]
                assert _same(_thin(image, cfg), want), (name, H, W)
            for first in (0, 1):
                want = _want(("noise1", H, W, first), image, first_subiter=first, max_subiters=1)[0]
                assert _same(_thin(image, cfg, _first_subiter=first, _max_subiters=1), want), ("noise1", H, W, first)


@_config
@pytest.mark.parametrize("shape", [(33, 70), (70, 33)])
def test_all_ones_takes_17_iterations_to_38_pixels(cfg, shape):
    want, iterations, _, _ = _want(("ones",) + shape, np.ones(shape, dtype=bool))
    assert iterations == 17 and int(want.sum()) == 38
    got = _thin(np.ones(shape, dtype=np.float32), cfg)
    assert _same(got, want) and int(got.sum()) == 38


@_config
def test_blob(cfg):
    mask, skel, iterations = R.blob()
    assert iterations == 16
    assert _same(_thin(mask, cfg), skel)
    # set means > 0, whatever the dtype; a view that is not contiguous
    as_float = np.where(mask, 0.25, -1.0).astype(np.float32)
    assert _same(_thin(as_float, cfg), skel)
    from riggs_amd.thinning import thin
    wide = torch.zeros(97, 262, dtype=torch.int16, device="cuda")
    wide[:, ::2] = torch.from_numpy(mask.astype(np.int16) * 255).cuda()
    assert _same(thin(wide[:, ::2], _path=cfg[1], _check_every=cfg[2]), skel)


def _batch():
    """B = 6 images of 64 x 96 that converge at different times: zeros, one pixel, a one-pixel line along two borders, noise, a
    blob."""
    if "batch" not in _ORACLE:
        b = np.zeros((6, 64, 96), dtype=bool)
        b[1, 17, 40] = True
        b[2, 0, :] = True
        b[3, :, 95] = True
        b[4] = _noise(64, 96, 5)
        b[5] = R.ellipses(64, 96, 4, seed=11)
        details = [R.thin_details(x) for x in b]
        _ORACLE["batch"] = (b, np.stack([d[0] for d in details]), [d[1] for d in details])
    return _ORACLE["batch"]


@_config
def test_batch_whose_images_converge_at_different_times(cfg):
    b, want, iterations = _batch()
    assert len(set(iterations)) >= 3 and max(iterations) >= 8 and min(iterations) == 1
    got = _thin(b, cfg)
    assert got.shape == (6, 64, 96)
    for k in range(6):
        assert _same(got[k], want[k]), k
    assert _same(_thin(b[5], cfg), want[5])  # ... and an image's result does not depend on its batch


@_config
@pytest.mark.parametrize("max_num_iter", [1, 2, 5])
def test_max_num_iter_is_honoured_exactly(cfg, max_num_iter):
    mask, skel, _ = R.blob()
    want = _want(("blob-max", max_num_iter), mask, max_num_iter=max_num_iter)[0]
    assert want.sum() > skel.sum()  # (not converged yet: one iteration more would show)
    assert _same(_thin(mask, cfg, max_num_iter=max_num_iter), want)
    odd = _want(("blob-sub", max_num_iter), mask, max_subiters=2 * max_num_iter + 1)[0]
    assert _same(_thin(mask, cfg, _max_subiters=2 * max_num_iter + 1), odd)


def test_path_boundary():
    """The largest H x 1280 image of the LDS path and the first of the global path (riggs_thin_path decides), filled with
    small discs so that the oracle is done in under ten iterations."""
    from riggs_amd import _lib as L
    from riggs_amd.thinning import PATH_GLOBAL, PATH_LDS, thin
    lib = L.lib()
    H = max(h for h in range(1, 2000) if lib.riggs_thin_path(h, 1280) == PATH_LDS)
    assert 900 < H < 1100 and lib.riggs_thin_path(H + 1, 1280) == PATH_GLOBAL
    assert lib.riggs_thin_workspace_bytes(1, H, 1280, -1) == 0 < lib.riggs_thin_workspace_bytes(1, H + 1, 1280, -1)
    for h in (H, H + 1):
        image = R.discs(h, 1280, 1500, seed=3)
        want, iterations, _, _ = R.thin_details(image)
        assert 3 <= iterations < 10
        x = torch.from_numpy(image).cuda()
        assert _same(thin(x), want), h                                                    # the path the size takes
        assert _same(thin(x, _path=PATH_GLOBAL, _check_every=4), want), h
    with pytest.raises(L.RiggsHipError, match="does not fit"):
        thin(x, _path=PATH_LDS)


def _np_elements(t, resolution):
    """scene/dataset_readers.py + utils/camera_utils.py:60 of the reference."""
    return (np.concatenate(np.where(t > 0)).reshape(2, -1).T / resolution).astype(np.float32)


@pytest.mark.parametrize("resolution", [1, 2, 3])
def test_thinned_elements(resolution):
    from riggs_amd.thinning import elements_into, thinned_elements
    _, want, _ = _batch()
    skel = torch.from_numpy(want.copy()).cuda()
    n = want.reshape(6, -1).sum(-1)
    assert n[0] == 0 and n[1] == 1 and n.max() > 64
    points, counts = thinned_elements(skel, resolution)
    assert points.shape == (6, n.max(), 2) and points.dtype is torch.float32 and counts.dtype is torch.int32
    assert counts.tolist() == n.tolist()
    for b in range(6):
        assert torch.equal(points[b, :n[b]].cpu(), torch.from_numpy(_np_elements(want[b], resolution))), b
    # an explicit capacity beyond the counts; rows at and beyond count keep what was there
    cap = int(n.max()) + 37
    buf = torch.full((6, cap, 2), -7.0, device="cuda")
    cnt = torch.full((6,), -1, dtype=torch.int32, device="cuda")
    elements_into(skel, resolution, buf, cnt)
    assert cnt.tolist() == n.tolist()
    for b in range(6):
        assert torch.equal(buf[b, :n[b]], points[b, :n[b]]) and (buf[b, n[b]:] == -7.0).all(), b
    p2, c2 = thinned_elements(skel, resolution, capacity=cap)
    assert p2.shape == (6, cap, 2) and torch.equal(c2, counts) and torch.equal(p2[:, :n.max()], points)
    # a capacity below the count caps it: nothing is written past the buffer
    p3, c3 = thinned_elements(skel[5], resolution, capacity=10)
    assert c3.tolist() == [10] and torch.equal(p3[0], points[5, :10])
    # more than one round of 1024 words, a width that is no multiple of 4, dense: 97 x 131 noise
    noise = _noise(97, 131, 9)
    p4, c4 = thinned_elements(torch.from_numpy(noise).cuda(), resolution)
    assert c4.tolist() == [int(noise.sum())] and torch.equal(p4[0].cpu(), torch.from_numpy(_np_elements(noise, resolution)))


class _Cam:
    def __init__(self, H, W, thinned):
        view = np.eye(4, dtype=np.float32)
        view[3, :3] = [0.05, -0.02, 3.0]  # row-vector convention: the translation in the last row
        self.world_view_transform = torch.from_numpy(view).cuda()
        self.FoVx, self.FoVy = 0.7, 0.55
        self.image_height, self.image_width = H, W
        self.K = None
        self.thinned = thinned


@pytest.mark.parametrize("resolution", [1, 2])
def test_into_the_skeleton_loss(resolution):
    """cal_skeleton_loss on ``points[b]`` with ``pixel_count=counts[b]`` is, bit for bit, the loss on the NumPy-built ``thinned`` of
    the same image: value and gradient."""
    from riggs_amd.loss import cal_skeleton_loss
    from riggs_amd.thinning import camera_thinned, thin, thinned_elements
    b, want, _ = _batch()
    mask = torch.from_numpy(b[5].copy()).cuda()
    ref = _np_elements(want[5], resolution)
    points, counts = thinned_elements(thin(mask), resolution, capacity=len(ref) + 29)
    assert int(counts[0]) == len(ref)
    assert torch.equal(camera_thinned(mask[None].float(), resolution).cpu(), torch.from_numpy(ref))
    rng = np.random.default_rng(4)
    parents = torch.tensor([-1, 0, 1, 1, 3, 0], dtype=torch.int32).cuda()
    joints = (0.4 * rng.standard_normal((6, 3))).astype(np.float32)
    H, W = 64 // resolution, 96 // resolution
    out = []
    for cam, kw in ((_Cam(H, W, torch.from_numpy(ref).cuda()), {}), (_Cam(H, W, points[0]), {"pixel_count": counts[0]})):
        x = torch.from_numpy(joints).cuda().requires_grad_(True)
        loss = cal_skeleton_loss(x, parents, cam, num_sample=64, **kw)
        loss.backward()
        out.append((loss.detach(), x.grad))
    assert torch.isfinite(out[0][0]) and float(out[0][1].abs().sum()) > 0
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_mirrors_of_the_reference_script():
    from riggs_amd.thinning import extract_skeleton, get_2d_skeleton
    b, want, _ = _batch()
    one = get_2d_skeleton(torch.from_numpy(b[5].astype(np.float64)).cuda())
    assert one.dtype is torch.int32 and one.shape == (64, 96) and one.is_cuda
    assert torch.equal(one.cpu(), torch.from_numpy(want[5].astype(np.int32) * 255))
    many = extract_skeleton(torch.from_numpy(b[:, None]).cuda())
    assert isinstance(many, list) and len(many) == 6
    for k, img in enumerate(many):
        assert img.dtype is torch.int32 and img.shape == (64, 96)
        assert set(img.unique().tolist()) <= {0, 255} and torch.equal(img.cpu() > 0, torch.from_numpy(want[k])), k
