"""CPU: the restatement of farthest-point sampling over rows of D floats (tests/fps_rows_ref.py, the arithmetic csrc/fps.hip is
held to) returns the reference's indices for every fixture; every fixture keeps its margin to a tie; at D = 3 the restatement
returns the 3-column fixtures' indices; include/riggs_hip.h declares the wide entries."""
import os
import re

import numpy as np
import pytest

from tests import fps_rows_ref as R
from tests import skeleton_init_ref as S


@pytest.mark.parametrize("name", R.FIXTURES)
def test_restatement_returns_the_fixture_indices(name):
    rows, start, ref = R.fixture(name)
    assert rows.dtype == np.float32 and 1 <= rows.shape[1] <= 64 and ref[0] == start
    got = R.fps_rows(rows, start, len(ref))
    assert np.array_equal(got, ref), (name, np.flatnonzero(got != ref)[:5])
    if name == "fpsrows_n2050x2_d48_p20":
        assert rows.shape == (4100, 48) and int(ref[1:].max()) < 2050
    if name == "fpsrows_same300_d48_p5":
        assert rows.shape == (300, 48) and ref.tolist() == [start, 0, 0, 0, 0]


@pytest.mark.parametrize("name", R.FIXTURES)
def test_fixture_margins_in_float64(name):
    rows, start, ref = R.fixture(name)
    idx64, gap = R.fps_rows_f64(rows, start, len(ref))
    print(name, "gap", gap, "bound", R.margin_bound(rows.shape[1]))
    assert np.array_equal(idx64, ref)
    assert gap >= R.margin_bound(rows.shape[1])
    assert os.path.getsize(os.path.join(R.GOLDEN, name + ".npz")) < 400 * 1000


@pytest.mark.parametrize("name", S.FPS_FIXTURES)
def test_three_columns_give_the_three_column_fixtures(name):
    pts, start, ref = S.fps_fixture(name)
    assert np.array_equal(R.fps_rows(pts, start, len(ref)), ref)


def test_header_declares_the_wide_entries():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "riggs_hip.h")).read(), flags=re.S)
    txt = " ".join(txt.split())
    assert "size_t riggs_fps_rows_workspace_bytes(int32_t N, int32_t D);" in txt
    assert re.search(r"int riggs_fps_sample_rows\(int32_t N, int32_t D, int32_t npoint, const float\* rows, int64_t row_stride, "
                     r"const int64_t\* start, void\* workspace, int64_t\* out_indices, riggs_stream stream\);", txt)
    from riggs_amd import _lib
    assert {"riggs_fps_rows_workspace_bytes", "riggs_fps_sample_rows"} <= set(_lib.exported_symbols())
    L = _lib.lib()
    assert L.riggs_fps_rows_workspace_bytes(1000, 48) >= 4 * 1000 * 49
    # widths outside 1..64 and a stride below the width are refused before any HIP call
    for (n, d, stride) in ((10, 65, 65), (10, 0, 3), (10, 48, 47), (0, 48, 48)):
        assert L.riggs_fps_sample_rows(n, d, 4, None, stride, None, None, None, None) != 0 and L.riggs_last_error()
