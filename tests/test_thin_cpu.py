"""CPU: the thinning oracle (tests/thin_ref.py, the NumPy restatement csrc/thin.hip is compared with on the GPU) against what is
published about the algorithm and against its own invariants; the public entries of riggs_amd.thinning refuse CPU tensors and
bad shapes."""
import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import thin_ref as R


def test_published_7x7_example():
    """The example of skimage.morphology.thin's documentation: rows 1-5 x columns 2-4 set plus pixel (0, 1) thin to five
    pixels; the second iteration finds the fixed point."""
    x = np.zeros((7, 7), dtype=np.uint8)
    x[1:6, 2:5] = 1
    x[0, 1] = 1
    s, iterations, subiters, _ = R.thin_details(x)
    assert np.argwhere(s).tolist() == [[0, 1], [1, 2], [2, 3], [3, 3], [4, 3]]
    assert iterations == 2 and subiters == 4
    assert np.array_equal(R.thin(x, max_num_iter=1), s) and np.array_equal(R.thin(x, max_num_iter=2), s)
    assert R.thin(x, max_subiters=1).sum() > s.sum()


def test_tables_have_37_deleting_codes_and_the_second_is_the_first_turned_by_180_degrees():
    assert [int(t.sum()) for t in R.TABLES] == [37, 37]
    turned = np.array([((c << 4) | (c >> 4)) & 0xFF for c in range(256)])  # x_i -> x_{(i + 4) % 8}
    assert np.array_equal(R.TABLES[1], R.TABLES[0][turned])
    assert not np.array_equal(R.TABLES[0], R.TABLES[1])
    assert not R.TABLES[0][0] and not R.TABLES[0][255]  # an isolated pixel and an interior pixel stay


def test_codes_are_the_neighbourhood_sums_with_zeros_outside():
    p = R.all_patches()
    c = R.codes(p)
    assert np.array_equal(c[1::5, 1::5].ravel(), np.arange(256)) and p[1::5, 1::5].all()
    ones = np.ones((3, 4), dtype=bool)
    assert R.codes(ones)[0, 0] == 1 + 64 + 128 and R.codes(ones)[2, 3] == 4 + 8 + 16


def test_all_ones_33_by_70():
    for shape in ((33, 70), (70, 33)):
        s, iterations, _, _ = R.thin_details(np.ones(shape, dtype=bool))
        assert iterations == 17 and int(s.sum()) == 38


def test_blob_invariants():
    """Subset of the input, idempotent, and the separately connected blobs stay separately connected (8-connectivity)."""
    mask, skel, iterations = R.blob()
    assert mask.shape == (97, 131) and iterations == 16
    assert not (skel & ~mask).any() and 0 < skel.sum() < mask.sum()
    again, it2, _, _ = R.thin_details(skel)
    assert np.array_equal(again, skel) and it2 == 1
    eight = np.ones((3, 3), dtype=int)
    lab_m, n_m = ndimage.label(mask, structure=eight)
    lab_s, n_s = ndimage.label(skel, structure=eight)
    assert n_m == n_s and n_m >= 2
    # every component of the skeleton lies in its own component of the mask
    owners = [np.unique(lab_m[lab_s == k]) for k in range(1, n_s + 1)]
    assert all(len(o) == 1 for o in owners) and len({int(o[0]) for o in owners}) == n_m


def test_max_num_iter_and_either_table_first():
    mask, skel, _ = R.blob()
    a = R.thin(mask, max_num_iter=2)
    assert np.array_equal(a, R.thin(mask, max_subiters=4)) and a.sum() > skel.sum()
    one = R.thin(mask, max_subiters=1)
    other = R.thin(mask, first_subiter=1, max_subiters=1)
    assert not np.array_equal(one, other)
    _, _, _, hists = R.thin_details(mask, max_subiters=3, histograms=True)
    assert len(hists) == 3 and hists[0].shape == (256,) and hists[0].sum() == mask.sum()


def test_public_entries_refuse_cpu_tensors_and_bad_shapes():
    from riggs_amd import _lib as L
    from riggs_amd import thinning as T
    cpu = torch.ones(8, 8)
    for fn in (T.thin, T.thinned_elements, T.get_2d_skeleton, T.camera_thinned):
        with pytest.raises(L.RiggsHipError, match="CUDA"):
            fn(cpu)
    with pytest.raises(L.RiggsHipError, match="CUDA"):
        T.extract_skeleton(torch.ones(2, 1, 8, 8))
    with pytest.raises(L.RiggsHipError, match="B, 1, H, W"):
        T.extract_skeleton(torch.ones(2, 8, 8))
    with pytest.raises(L.RiggsHipError, match="CUDA"):
        T.thin(np.ones((8, 8)))
    with pytest.raises(L.RiggsHipError):
        T.camera_thinned(torch.ones(2, 8, 8))
    assert (T.PATH_AUTO, T.PATH_LDS, T.PATH_GLOBAL) == (-1, 0, 1)


def test_c_entries_reject_bad_arguments_before_any_hip_call():
    """NULL pointers, non-positive sizes, an unknown path, the LDS path for an image that does not fit it: a status and a message."""
    from riggs_amd import _lib as L
    lib = L.lib()
    N = None
    assert lib.riggs_thin_path(800, 800) == 0 and lib.riggs_thin_path(2000, 2000) == 1
    assert lib.riggs_thin_path(0, 5) == -1 and lib.riggs_thin_path(5, 40000) == -1
    assert lib.riggs_thin_workspace_bytes(3, 64, 96, 0) == 0 and lib.riggs_thin_workspace_bytes(3, 64, 96, -1) == 0
    # two padded planes per image ((H + 2) (ceil(W / 32) + 1) + 1 words, rounded up to 4) and one counter per image
    assert lib.riggs_thin_workspace_bytes(3, 64, 96, 1) == 2 * 3 * 4 * 268 + 256
    for args in ((0, 8, 8, N, N, 0, -1, -1, 8, N, N), (1, 0, 8, N, N, 0, -1, -1, 8, N, N), (1, 8, 8, N, N, 0, -1, -1, 8, N, N)):
        assert lib.riggs_thin(*args) != 0 and lib.riggs_last_error()
    assert lib.riggs_thin(1, 8, 8, 1, 1, 2, -1, -1, 8, N, N) != 0 and b"first_subiter" in lib.riggs_last_error()
    assert lib.riggs_thin(1, 8, 8, 1, 1, 0, -1, 7, 8, N, N) != 0 and b"path" in lib.riggs_last_error()
    assert lib.riggs_thin(1, 2000, 2000, 1, 1, 0, -1, 0, 8, N, N) != 0 and b"does not fit" in lib.riggs_last_error()
    assert lib.riggs_thin(1, 8, 8, 1, 1, 0, -1, 1, 8, N, N) != 0 and b"workspace" in lib.riggs_last_error()
    assert lib.riggs_thin(1, 8, 8, 1, 1, 0, -1, 1, 0, 1, N) != 0 and b"check_every" in lib.riggs_last_error()
    for args in ((0, 8, 8, 1, 1.0, 4, 1, 1, N), (1, 8, 8, N, 1.0, 4, 1, 1, N), (1, 8, 8, 1, 0.0, 4, 1, 1, N), (1, 8, 8, 1, 1.0, -1, 1, 1, N),
                 (1, 8, 8, 1, 1.0, 4, N, 1, N), (1, 8, 8, 1, 1.0, 4, 1, N, N)):
        assert lib.riggs_thin_elements(*args) != 0 and lib.riggs_last_error()
