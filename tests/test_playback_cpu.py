"""Pose-track playback without a GPU: the CPU restatement (tests/playback_ref.py) against goldens captured from the reference
(tests/golden/make_playback_golden.py: playback_*.npz), the entry points in the header and in riggs_amd._lib, and the host
logic of riggs_amd.playback.run_interpolation that needs no device.

Bounds: node colours and point colours bit for bit (a neighbouring 1/255 step is another colour); everything else 1e-6 relative
to the largest reference value — the restatement runs the same torch operations as the reference."""
import glob
import os

import numpy as np
import pytest
import torch

from riggs_amd import _lib as L
from riggs_amd import playback as PB
from tests import playback_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SYMBOLS = ("riggs_pose_slerp", "riggs_lbs_sequence_forward", "riggs_skinning_colors", "riggs_lbs_sequence_pass_frames")


def T(a):
    return torch.from_numpy(np.asarray(a))


def close(a, b, what, rel=1e-6):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, what
    err = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))
    assert err <= rel, "%s: max error %.3g of the largest value (bound %.1e)" % (what, err, rel)


def files(pat):
    out = sorted(glob.glob(os.path.join(GOLD, pat)))
    assert out, pat
    return out


@pytest.mark.parametrize("path", files("playback_slerp_*.npz"), ids=lambda p: os.path.basename(p)[:-4])
def test_slerp_restatement_reproduces_the_reference(path):
    g = np.load(path)
    q0, q1 = T(g["q0"]), T(g["q1"])
    assert float((q0[0] * q1[0]).sum()) < 0 and torch.equal(q1[1], 2.0 * q0[1]) and torch.equal(q1[2], -q0[2])  # the special rows
    out = R.slerp_batch(q0, q1, T(g["t"]))
    assert bool(torch.isfinite(out).all())
    close(out, g["out"], "slerp_batch")


def test_interpolation_restatement_reproduces_the_reference():
    g = np.load(os.path.join(GOLD, "playback_interp_p3_j24_f7.npz"))
    keys = [{"local_rotation2": T(g["key_rot"][i]), "global_trans": T(g["key_trans"][i])} for i in range(3)]
    out = R.run_interpolation(keys, int(g["num_frames"]))
    assert out["num"] == int(g["num"]) == 14 and out["local_rotation2"].shape == (14, 24, 4)
    close(out["local_rotation2"], g["local_rotation"], "interpolated rotations")
    close(out["global_trans"], g["global_trans"], "interpolated translations")
    # a segment starts ON its first key pose (t = 0) and stops short of its second
    close(out["local_rotation2"][7], torch.nn.functional.normalize(keys[1]["local_rotation2"], dim=1), "frame 7 = key pose 1")


@pytest.mark.parametrize("path", files("playback_colors_*.npz"), ids=lambda p: os.path.basename(p)[:-4])
def test_colour_restatement_reproduces_the_reference(path):
    g = np.load(path)
    x, joints = T(g["x"]), T(g["joints"])
    assert np.array_equal(R.get_geometric_color(joints).numpy().view(np.uint32), g["node_colors"].view(np.uint32)), "node colours: bits"
    assert np.array_equal(R.get_geometric_color(x).numpy().view(np.uint32), g["point_colors"].view(np.uint32)), "point colours: bits"
    nc = g["node_colors"]
    assert nc.min() >= 0 and nc.max() == np.float32(0.99) and not (nc >= 1).any()  # the >= 1 -> 0.99 rule is exercised
    close(R.get_color_for_skinning_weights(x, T(g["nn_idx"]), T(g["nn_weight"]), joints), g["colors"], "skinning colours")
    # the library's torch mirror runs the same operations on the CPU too
    assert np.array_equal(PB.get_geometric_color(joints).numpy().view(np.uint32), g["node_colors"].view(np.uint32))
    close(PB.get_color_for_skinning_weights(x, T(g["nn_idx"]), T(g["nn_weight"]), joints), g["colors"], "mirror: skinning colours")


@pytest.mark.parametrize("path", files("playback_seq_*.npz"), ids=lambda p: os.path.basename(p)[:-4])
def test_sequence_restatement_reproduces_the_reference(path):
    g = np.load(path)
    keys = [{"local_rotation2": T(g["key_rot"][i]), "global_trans": T(g["key_trans"][i])} for i in range(2)]
    track = R.run_interpolation(keys, int(g["num_frames"]))
    close(track["local_rotation2"], g["local_rotation"], "track rotations")
    close(track["global_trans"], g["global_trans"], "track translations")
    out = R.deform_sequence(T(g["x"]), T(g["joints"]), T(g["parents"]), T(g["node_radius_log"]), T(g["local_rotation"]),
                            T(g["global_trans"]), T(g["motion_mask"]), int(g["K"]))
    for k in ("d_xyz", "d_rotation", "d_nodes"):
        close(out[k], g[k], k)


def test_header_declares_the_entry_points_and_the_binding_has_their_signatures():
    assert set(SYMBOLS) <= set(L.exported_symbols())  # (read from the header; tests/test_capi_cpu.py has the compiler check each one)


def test_fewer_than_two_key_poses_give_none():
    assert PB.run_interpolation([], "cpu") is None
    assert PB.run_interpolation([{"local_rotation": torch.zeros(4, 4), "global_trans": torch.zeros(1, 3)}], "cpu") is None
    assert R.run_interpolation([]) is None


def test_key_poses_are_read_under_either_name(monkeypatch):
    """'local_rotation2' where a key pose has it, else 'local_rotation'; the track comes back under both names, one tensor.  The
    launch is replaced by the restatement: what is checked is which tensors reach it and what is returned."""
    seen = {}

    def launch(S, m, n, q0, q1, q_stride, t, tr0, tr1, strides, out_rot, out_trans):
        seen.update(S=S, m=m, n=n, q_stride=q_stride, strides=strides)
        for s in range(S):
            out_rot[s * m:(s + 1) * m] = R.slerp_batch(q0[s], q1[s], t).transpose(0, 1)
            out_trans[s * m:(s + 1) * m] = (1 - t[:, None]) * tr0[s] + t[:, None] * tr1[s]
    monkeypatch.setattr(PB, "_slerp_launch", launch)
    monkeypatch.setattr(L, "require_cuda_f32", lambda name, t, shape=None: t)
    g = torch.Generator().manual_seed(5)
    a, b, c, decoy = (torch.randn(6, 4, generator=g) for _ in range(4))
    tr = [torch.randn(1, 3, generator=g) for _ in range(3)]
    keys = [{"local_rotation": a, "global_trans": tr[0]},                                  # the editor's name
            {"local_rotation2": b, "local_rotation": decoy, "global_trans": tr[1]},        # both: '2' wins
            {"local_rotation2": c, "global_trans": tr[2]}]                                 # the reference's name
    out = PB.run_interpolation(keys, "cpu", num_frames=4)
    assert seen == dict(S=2, m=4, n=6, q_stride=24, strides=(4 * 6 * 4, 6 * 4, 4))
    assert out["local_rotation"] is out["local_rotation2"] and out["num"] == 8 and out["global_trans"].shape == (8, 3)
    want = R.run_interpolation([{"local_rotation2": q, "global_trans": t_} for q, t_ in zip((a, b, c), tr)], 4)
    close(out["local_rotation2"], want["local_rotation2"], "track")
    close(out["global_trans"], want["global_trans"], "translations")
