"""What tests/test_gpu_ik.py and tests/test_gpu_fit.py share: the two solvers run on one frame (csrc/pose_solve.h), and their tests on
one set of helpers."""
import json
import os

import numpy as np
import pytest
import torch


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def deviation(a, b, key, extent):
    """max |a - b|; positions, the translation and the residual relative to the rig's extent."""
    d = float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())
    return d if key == "local_rotation" else d / extent


def parity_bars(o64, o32, keys, extent):
    """The parity bar of every tensor, max(8 * e32, 1e-6), and e32 (the float32 restatement's deviation from float64) behind it."""
    e32 = {k: deviation(o32[k], o64[k], k, extent) for k in keys}
    return {k: max(8 * e32[k], 1e-6) for k in keys}, e32


def parity_report(env, records):
    """A module's autouse fixture: behind its tests, ``records`` goes as JSON to the path the environment variable ``env`` names."""
    @pytest.fixture(scope="module", autouse=True)
    def report():
        yield
        path = os.environ.get(env)
        if records and path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                json.dump(records, f, indent=1, sort_keys=True)
    return report


def make_rig(case):
    from riggs_amd.skeleton import SkeletonWarp
    sw = SkeletonWarp(is_blender=True, joints=torch.from_numpy(case["joints"]), parent_indices=torch.from_numpy(case["parents"]).long(),
                      K=-1, hyper_dim=8, use_skinning_weight_mlp=False, use_template_offsets=False).cuda()
    g = torch.Generator().manual_seed(5)
    x = (torch.from_numpy(case["joints"])[torch.randint(0, case["J"], (500,), generator=g)] + 0.05 * torch.randn(500, 3, generator=g)).cuda()
    return sw, x
