"""The nodes of a deformation module as a small Gaussian model (utils/time_utils.py:867-872, 1238-1260): shared by
``SkeletonWarp`` and ``ControlNodeWarp``, which both keep their node positions in ``self.nodes`` (first three columns)."""
from __future__ import annotations

import torch


class NodeGaussians:
    @staticmethod
    def _gaussian_classes():
        try:  # the trainer's own classes when this module runs inside a RigGS checkout
            from scene.gaussian_model import BasicPointCloud, StandardGaussianModel
        except Exception:
            from .gaussian_model import BasicPointCloud, StandardGaussianModel
        return BasicPointCloud, StandardGaussianModel

    @property
    def as_gaussians(self):
        if getattr(self, "gs", None) is None:
            print("Building Learnable Gaussians for Nodes!")
            BasicPointCloud, StandardGaussianModel = self._gaussian_classes()
            joints = self.nodes[..., :3].detach()
            pcd = BasicPointCloud(points=joints, colors=torch.zeros_like(joints), normals=joints)
            self.gs = StandardGaussianModel(sh_degree=0, all_the_same=True, with_motion_mask=False)
            self.gs.create_from_pcd(pcd=pcd, spatial_lr_scale=0.0, print_info=False)  # distCUDA2 on the nodes
            self.gs._scaling.data = torch.log(1e-2 * torch.ones_like(self.gs._scaling))
            self.gs._xyz.data = self.nodes[..., :3]
        return self.gs

    def init_gaussians(self, init_pcl, with_motion_mask):
        if getattr(self, "gs", None) is None:
            print("Initialize Learnable Gaussians for Nodes with Point Clouds!")
            BasicPointCloud, StandardGaussianModel = self._gaussian_classes()
            pcd = BasicPointCloud(points=init_pcl.detach(), colors=torch.zeros_like(init_pcl), normals=torch.zeros_like(init_pcl))
            self.gs = StandardGaussianModel(sh_degree=0, all_the_same=True, with_motion_mask=with_motion_mask)
            self.gs.create_from_pcd(pcd=pcd, spatial_lr_scale=0.0, print_info=False)
        return self.gs

    def state_dict(self, *args, **kwargs):
        """The module's entries plus, once the node Gaussians exist, theirs as ``gs_<name>`` (utils/time_utils.py:867-872)."""
        sd = super().state_dict(*args, **kwargs)
        if getattr(self, "gs", None) is not None:
            prefix = kwargs.get("prefix", args[1] if len(args) > 1 else "")
            for name in self.gs.param_names():
                sd[prefix + "gs_" + name] = getattr(self.gs, name)
        return sd
