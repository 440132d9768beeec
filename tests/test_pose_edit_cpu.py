"""riggs_amd/pose_edit.py without a GPU: the mirrors of the reference editor's edit step (interactive_GUI.py) on CPU tensors
against NumPy / scipy restatements carrying the reference's line numbers, and the IK oracle (tests/ik_ref.py) on its own bar."""
import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

from riggs_amd import pose_edit as PE
from riggs_amd import synth
from tests import ik_ref as R


def hamilton(a, b):
    aw, ax, ay, az = np.moveaxis(a, -1, 0)
    bw, bx, by, bz = np.moveaxis(b, -1, 0)
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


# --------------------------------------------------------------------------- rotate_joint, apply_edit
@pytest.mark.parametrize("angle", [0.0, 1e-5, 5e-4, 0.3, -1.2, 3.0, 4.0])
def test_rotate_joint_is_scipys_rotation_vector(angle):
    axis = np.array([0.36, -0.48, 0.8])
    edit = PE.rotate_joint(None, 3, torch.tensor(axis, dtype=torch.float32), angle, num_joints=6)
    q = Rotation.from_rotvec(np.float32(axis).astype(np.float64) * angle).as_quat()  # :298-300 (xyzw)
    want = np.tile(np.array([1.0, 0, 0, 0]), (6, 1))
    want[3] = [q[3], q[0], q[1], q[2]]  # :320
    assert np.abs(edit["local_rotation"].numpy() - want).max() <= 4 * 2.0 ** -24
    assert tuple(edit["global_trans"].shape) == (1, 3) and float(edit["global_trans"].abs().max()) == 0.0


def test_rotate_joint_overwrites_the_row_and_the_translation():
    axis = torch.tensor([0.0, 0.0, 1.0])
    edit = PE.rotate_joint(None, 2, axis, 0.5, translation=torch.tensor([1.0, 2.0, 3.0]), num_joints=4)
    same = PE.rotate_joint(edit, torch.tensor(2), axis, torch.tensor(-0.25))  # (a joint and an angle that are tensors; no translation)
    assert same is edit
    q = Rotation.from_rotvec([0, 0, -0.25]).as_quat()
    assert np.abs(edit["local_rotation"][2].numpy() - [q[3], q[0], q[1], q[2]]).max() <= 2.0 ** -23  # not composed with the 0.5 before
    assert float(edit["global_trans"].abs().max()) == 0.0  # :321: overwritten by the default
    PE.rotate_joint(edit, 1, axis, 0.1, translation=torch.tensor([[0.5, 0.0, -0.5]]))
    assert edit["global_trans"].tolist() == [[0.5, 0.0, -0.5]]
    assert edit["local_rotation"][0].tolist() == [1, 0, 0, 0] and edit["local_rotation"][3].tolist() == [1, 0, 0, 0]
    with pytest.raises(ValueError):
        PE.rotate_joint(None, 0, axis, 0.1)


def test_apply_edit_is_the_hamilton_product():
    rng = np.random.default_rng(3)
    e, p = rng.normal(size=(7, 4)), rng.normal(size=(7, 4))
    te, tp = rng.normal(size=(1, 3)), rng.normal(size=(1, 3))
    attrs = {"local_rotation": torch.tensor(p, dtype=torch.float32), "global_trans": torch.tensor(tp, dtype=torch.float32), "t": 0.25}
    out = PE.apply_edit(attrs, {"local_rotation": torch.tensor(e, dtype=torch.float32), "global_trans": torch.tensor(te, dtype=torch.float32)})
    want = hamilton(np.float32(e).astype(np.float64), np.float32(p).astype(np.float64))  # :398
    want = np.where(want[:, :1] < 0, -want, want)  # (quaternion_multiply standardises: real part >= 0)
    assert np.abs(out["local_rotation"].numpy() - want).max() <= 1e-6 * np.abs(want).max()
    assert np.abs(out["global_trans"].numpy() - (np.float32(tp).astype(np.float64) + np.float32(te))).max() <= 1e-6  # :399
    assert out["t"] == 0.25 and attrs["local_rotation"] is not out["local_rotation"]
    assert PE.apply_edit(attrs, None)["local_rotation"] is attrs["local_rotation"]  # :397: no edit yet


# --------------------------------------------------------------------------- view_axis, joint_drag
def camera():
    return synth.look_at_camera(120, 160, azimuth_deg=30.0, elevation_deg=15.0, radius=3.0)


def view_axis_ref(cam):
    m = cam.full_proj_transform.numpy().astype(np.float64)
    d = (np.array([[0.0, 0, 1, 1]]) @ np.linalg.inv(m))[0, :3]  # :337-338
    return d / np.linalg.norm(d)  # :339


def project_ref(cam, pts):
    m = cam.full_proj_transform.numpy().astype(np.float64)
    hom = np.concatenate([pts, np.ones((len(pts), 1))], 1) @ m  # :1314
    uv = hom[:, :2] / hom[:, 3:]  # :1315
    return (uv + 1) / 2 * np.array([cam.image_height, cam.image_width])  # :1316


def joint_drag_ref(cam, nodes, parents, idx, mouse_loc, app_data=None, cam_rot=None):
    parent_idx = parents[idx]  # :1297
    translation, angle = np.zeros(3), 0.0  # :1298-1299
    moving_point_uv = np.array([int(mouse_loc[0]), int(mouse_loc[1])])  # :1300
    if parent_idx < 0:  # :1301
        dx, dy = app_data  # :1302-1303
        translation = 0.001 * cam_rot @ np.array([dx, -dy, 0])  # :1304
    else:
        point_uv = project_ref(cam, nodes[[parent_idx, idx]])  # :1307-1317
        vec_a = point_uv[1] - point_uv[0]  # :1318
        vec_b = moving_point_uv - point_uv[0]  # :1319
        cos_angle = np.dot(vec_a, vec_b) / (np.linalg.norm(vec_a) * np.linalg.norm(vec_b) + 1e-16)  # :1320
        angle = np.arccos(np.clip(cos_angle, -1, 1))  # :1321 (clamped: the stated deviation)
        if vec_a[0] * vec_b[1] - vec_a[1] * vec_b[0] < 0:  # :1323-1325 (np.cross of two 2-D vectors)
            angle = -angle
    return angle, translation


def rig():
    rng = np.random.default_rng(8)
    parents = np.array([-1, 0, 1, 1, 3], np.int64)
    nodes = np.float32(rng.normal(0, 0.3, (5, 3)))
    return nodes, parents


def test_view_axis():
    cam = camera()
    got = PE.view_axis(cam)
    assert np.abs(got.numpy() - view_axis_ref(cam)).max() <= 1e-5
    assert abs(float(got.norm()) - 1) <= 1e-6


def test_joint_drag_of_the_root_translates():
    cam, (nodes, parents) = camera(), rig()
    rot = Rotation.from_euler("xyz", [0.2, -0.4, 0.1]).as_matrix()
    angle, trans = PE.joint_drag(cam, torch.from_numpy(nodes), torch.from_numpy(parents), 0, (50.7, 60.2), mouse_delta=(12.0, -7.0),
                                 cam_rot=torch.tensor(rot))
    a_ref, t_ref = joint_drag_ref(cam, nodes.astype(np.float64), parents, 0, (50.7, 60.2), (12.0, -7.0), rot)
    assert float(angle) == 0.0 and a_ref == 0.0
    assert np.abs(trans.numpy() - t_ref).max() <= 1e-8
    assert angle.dim() == 0 and tuple(trans.shape) == (3,)


@pytest.mark.parametrize("joint", [1, 2, 3, 4])
def test_joint_drag_of_a_joint_is_the_signed_angle_in_the_image(joint):
    cam, (nodes, parents) = camera(), rig()
    uv = project_ref(cam, nodes.astype(np.float64))
    a, p = uv[joint], uv[parents[joint]]
    turn = lambda v, t: np.array([np.cos(t) * v[0] - np.sin(t) * v[1], np.sin(t) * v[0] + np.cos(t) * v[1]])  # noqa: E731
    signs = []
    for t in (0.7, -0.7, 2.5, -2.5):
        mouse = p + 40.0 * turn((a - p) / np.linalg.norm(a - p), t) + 0.5  # (+ 0.5: the truncation :1300 keeps it near)
        got, trans = PE.joint_drag(cam, torch.from_numpy(nodes), torch.from_numpy(parents), torch.tensor(joint), mouse, mouse_delta=(3.0, 4.0))
        want, _ = joint_drag_ref(cam, nodes.astype(np.float64), parents, joint, mouse)
        assert abs(float(got) - want) <= 1e-4 and abs(want - t) < 0.05, (t, float(got), want)
        assert float(trans.abs().max()) == 0.0
        signs.append(np.sign(float(got)))
    assert signs == [1, -1, 1, -1]


def test_joint_drag_with_the_mouse_on_the_bone_is_no_turn():
    """The parent projects onto an integer pixel and the joint lies on the pixel row through it, so an integer mouse further
    along that row is on the bone.  acos near 1 is ill-conditioned — acos(1 - e) = sqrt(2 e) — so one float32 rounding of the
    cosine (6e-8) shows as 3.5e-4 rad: the bar is 1e-3, against 1e-6 for the float64 restatement."""
    cam = camera()
    m = cam.full_proj_transform.numpy().astype(np.float64)

    def unproject(u, v, depth_w):  # the point whose editor projection is (u, v), at clip w = depth_w
        ndc = np.array([2 * u / cam.image_height - 1, 2 * v / cam.image_width - 1])
        # solve [x y z 1] m = w [ndc_x, ndc_y, *, 1]: two ratios and w fix the three unknowns
        A = np.stack([m[:3, 0] - ndc[0] * m[:3, 3], m[:3, 1] - ndc[1] * m[:3, 3], m[:3, 3]], 0)
        rhs = np.array([ndc[0] * m[3, 3] - m[3, 0], ndc[1] * m[3, 3] - m[3, 1], depth_w - m[3, 3]])
        return np.linalg.solve(A, rhs)
    nodes = np.float32(np.stack([unproject(70.0, 55.0, 3.0), unproject(88.5, 55.0, 3.2)]))
    parents = np.array([-1, 0], np.int64)
    uv = project_ref(cam, nodes.astype(np.float64))
    assert np.abs(uv - [[70.0, 55.0], [88.5, 55.0]]).max() < 1e-3
    want, _ = joint_drag_ref(cam, nodes.astype(np.float64), parents, 1, (120, 55))
    got, _ = PE.joint_drag(cam, torch.from_numpy(nodes), torch.from_numpy(parents), 1, (120, 55))
    assert abs(want) <= 1e-4 and abs(float(got)) <= 1e-3 and np.isfinite(float(got))


# --------------------------------------------------------------------------- the oracle on its own bar
@pytest.mark.parametrize("name", list(R.CASES))
def test_the_float64_oracle_reaches_the_targets(name):
    for B in (1, 3):
        case = R.make_case(name, B)
        out = R.solve_case(case, 32, np.float64)
        assert (out["residual"] <= 1e-6 * case["extent"]).all(), (B, out["residual"].max() / case["extent"])


def test_the_oracle_keeps_what_it_must():
    case = R.make_case("tree24", 1)
    on = R.paths(case["parents"], case["handles"]).any(0)
    locked = np.zeros(24, bool)
    locked[np.flatnonzero(on)[::2]] = True
    out = R.solve_case(case, 8, np.float32, locked=locked)
    still = locked | ~on
    assert np.array_equal(out["local_rotation"][0][still], case["q0"][0][still]) and (out["local_rotation"][0][~still] != case["q0"][0][~still]).any()
    start = R.solve_case(case, 0, np.float32)
    same = R.solve_case(case, 8, np.float32, targets=start["d_nodes"][:, case["handles"]])
    assert np.array_equal(same["local_rotation"], start["local_rotation"]) and (same["residual"] == 0).all()
    # the Cholesky solve against LAPACK
    rng = np.random.default_rng(1)
    M = rng.normal(size=(24, 30))
    A, r = M @ M.T + 0.01 * np.eye(24), rng.normal(size=24)
    assert np.abs(R.cholesky_solve(A, r) - np.linalg.solve(A, r)).max() <= 1e-9 * np.abs(np.linalg.solve(A, r)).max()
