"""CPU: the host side of the recolour pass — the ABI's two new entry points and the checks ``render(lists=...)`` makes before
any device work."""
import inspect
import os
import re
from types import SimpleNamespace

import pytest
import torch

from riggs_amd import _lib
from riggs_amd.render import render


def _declaration(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "riggs_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, "%s is not declared in include/riggs_hip.h" % name
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", ["riggs_raster_recolor_forward", "riggs_raster_recolor_backward"])
def test_recolor_entry_points_are_bound_with_the_headers_argument_count(name):
    args = _declaration(name)
    assert name in _lib._SIGS
    res, argtypes = _lib._SIGS[name]
    assert len(argtypes) == len(args), (args, argtypes)
    assert args[0].startswith("const riggs_raster_cfg*") and args[-1].startswith("riggs_stream")
    assert hasattr(_lib.lib(), name)  # exported (the library loads without a GPU)


def test_recolor_entry_points_reject_bad_arguments_without_a_gpu():
    L = _lib.lib()
    cfg = _lib.RasterCfg()
    cfg.num_points, cfg.image_height, cfg.image_width = 10, 0, 16
    assert L.riggs_raster_recolor_forward(cfg, None, None, 0, None, None, None, None, None, None) != 0 and L.riggs_last_error()
    cfg.image_height = 16
    assert L.riggs_raster_recolor_forward(cfg, None, None, 0, None, None, None, None, None, None) != 0
    assert b"NULL" in L.riggs_last_error()
    assert L.riggs_raster_recolor_backward(cfg, None, None, 0, None, None, None, None, None) != 0
    assert L.riggs_raster_recolor_forward(None, None, None, 0, None, None, None, None, None, None) != 0


class _Pipe:
    convert_SHs_python = compute_cov3D_python = debug = False


def _call(lists, N=12, H=32, W=48, **kw):
    cam = SimpleNamespace(image_height=H, image_width=W, FoVx=0.7, FoVy=0.6, world_view_transform=torch.eye(4),
                          full_proj_transform=torch.eye(4), camera_center=torch.zeros(3))
    pc = SimpleNamespace(get_xyz=torch.zeros(N, 3), motion_mask=torch.full((N, 1), 0.5), active_sh_degree=0)
    return render(cam, pc, _Pipe, torch.zeros(3), 0.0, 0.0, 0.0, lists=lists, **kw)


def test_render_over_lists_raises_before_any_device_work():
    """Host tensors throughout: a call that got as far as the library would raise RiggsHipError ("must be a CUDA(HIP) tensor"),
    not ValueError."""
    stub = SimpleNamespace(N=12, H=32, W=48)
    with pytest.raises(ValueError, match="render_motion"):
        _call(stub)  # neither render_motion nor override_color
    with pytest.raises(ValueError, match="render_motion"):
        _call(stub, d_color=torch.zeros(12, 3))
    for bad in (SimpleNamespace(N=13, H=32, W=48), SimpleNamespace(N=12, H=33, W=48), SimpleNamespace(N=12, H=32, W=47)):
        with pytest.raises(ValueError):
            _call(bad, render_motion=True)
        with pytest.raises(ValueError):
            _call(bad, override_color=torch.zeros(12, 3))
    with pytest.raises(ValueError, match="scale_const"):
        _call(stub, render_motion=True, scale_const=0.01)
    # a consistent call gets past the checks and is stopped by the library's own guard: the product path is GPU-only
    with pytest.raises(_lib.RiggsHipError, match="CUDA"):
        _call(stub, render_motion=True)
    with pytest.raises(ValueError, match="keep_lists"):
        _call(stub, render_motion=True, keep_lists=True)


def test_render_signature_still_begins_with_the_references_parameters():
    want = ["viewpoint_camera", "pc", "pipe", "bg_color", "d_xyz", "d_rotation", "d_scaling", "d_opacity", "d_color",
            "scaling_modifier", "override_color", "random_bg_color", "render_motion", "detach_xyz", "detach_scale", "detach_rot",
            "detach_opacity", "d_rot_as_res", "scale_const", "d_rotation_bias", "force_visible"]
    p = inspect.signature(render).parameters
    assert list(p)[:len(want)] == want
    assert list(p)[len(want):] == ["fused", "arena", "keep_lists", "lists"]
    assert p["keep_lists"].default is False and p["lists"].default is None
