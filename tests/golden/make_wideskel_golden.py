"""Golden vectors for skeletons of more than 64 joints, captured from the REAL RigGS reference (CPU) — run in the build
container only:   python tests/golden/make_wideskel_golden.py

The reference's own skeleton extraction samples up to 200 nodes (extract_skeleton_utils.py:426-471), so skeletons of 65..256
joints are reachable.  The file names carry a `wideskel_` prefix: the `deform_*.npz` glob of the older tests stays as it is.
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import S, SkeletonWarp, fixture_deform, fixture_posemlp, random_tree  # noqa: E402


def fixture_state_dict_layouts(Js):
    """Names and shapes of the reference SkeletonWarp's state dict (static scene, hyper_dim = 8, WeightMLP on) per joint count."""
    out = {}
    for J in Js:
        joints, parents = random_tree(torch.Generator().manual_seed(J), J)
        with S.quiet():
            sw = SkeletonWarp(is_blender=True, joints=joints, parent_indices=parents, K=-1, is_scene_static=True, hyper_dim=8)
        out[str(J)] = {k: list(v.shape) for k, v in sw.state_dict().items()}
    json.dump(out, open(os.path.join(HERE, "wideskel_state_dict_layout.json"), "w"), indent=0)
    print("wrote wideskel_state_dict_layout", Js)


if __name__ == "__main__":
    fixture_deform("wideskel_tree200_n200_mask", 201, 200, 200, -1, mask_random=True)
    fixture_deform("wideskel_tree128_n300_k3", 202, 128, 300, 3)
    fixture_deform("wideskel_tree65_n257", 203, 65, 257, -1)
    fixture_deform("wideskel_chain256_n200", 204, 256, 200, -1, chain=True)
    fixture_posemlp("wideskel_posemlp_j128", 205, 128)
    fixture_state_dict_layouts([65, 128, 200, 256])
