"""Single-hypothesis 3-D key-point detector (reference: modules/keypoint_detector_integral.py:7-65):
softmax over D*H*W and the plain three-axis expectation, fused into one HIP reduction."""
import torch
import torch.nn as nn

from modules.integral_base_modules.network import get_default_network_config, get_pose_net
from xas_amd import ops_head, ops_nn


class KPDetector3D(nn.Module):
    def __init__(self, name, num_kp, depth_dim, num_layers=50):
        super().__init__()
        cfg = get_default_network_config()
        cfg.depth_dim = depth_dim
        cfg.num_layers = num_layers
        self.num_kp = num_kp
        self.depth_dim = depth_dim
        self.net = get_pose_net(cfg, num_joints=num_kp)
        self.name = name

    def forward(self, x):
        ops_head.check_patch_size(x, self.depth_dim, 'KPDetector3D')
        kps, depth_prob_map = ops_head.softargmax_single(self.net(x), self.num_kp)
        return kps, depth_prob_map          # kps [B, 1, num_kp, 3], aligned with the multi-hypothesis layout

    @torch.no_grad()
    def forward_logits(self, x):
        """forward plus the logits the head ran on, [B, K*D, D, D] in its NHWC storage: see KPDetector3DMulti.forward_logits.
        -> (kps, depth_prob_map, heatmap)."""
        ops_head.check_patch_size(x, self.depth_dim, 'KPDetector3D')
        heatmap = self.net(x)
        kps, depth_prob_map = ops_head.softargmax_single(heatmap, self.num_kp)
        return kps, depth_prob_map, ops_head._nhwc_storage(heatmap)

    def forward_flip(self, x, flip_pairs):
        """Flip test (eval() only, no autograd): see KPDetector3DMulti.forward_flip.  -> what forward returns."""
        x2, perm = ops_head.detector_flip_input(self, x, flip_pairs, 'KPDetector3D')
        kps, depth_prob_map, _ = ops_head.softargmax_flip(self.net(x2), self.num_kp, 1, 0, perm)
        return kps, depth_prob_map

    @torch.no_grad()
    def forward_spread(self, x, flip_pairs=None):
        """forward (forward_flip when flip_pairs is given) plus the spatial spread [B, K, 5] of the heat-map the head ran on:
        see KPDetector3DMulti.forward_spread.  -> (kps, depth_prob_map, spread)."""
        if flip_pairs is None:
            ops_head.check_patch_size(x, self.depth_dim, 'KPDetector3D')
            heatmap = self.net(x)
            kps, depth_prob_map = ops_head.softargmax_single(heatmap, self.num_kp)
        else:
            x2, perm = ops_head.detector_flip_input(self, x, flip_pairs, 'KPDetector3D')
            heatmap = self.net(x2)
            kps, depth_prob_map, _ = ops_head.softargmax_flip(heatmap, self.num_kp, 1, 0, perm)
        return kps, depth_prob_map, ops_head.detector_spread(self, heatmap, flip_pairs)

    def forward_groups(self, x, groups):
        """`groups` consecutive reference calls as one camera-batched pass (see KPDetector3DMulti.forward_groups)."""
        ops_head.check_patch_size(x, self.depth_dim, 'KPDetector3D')
        with ops_nn.bn_groups(groups):
            heatmap = self.net(x)
        return ops_head.softargmax_single(heatmap, self.num_kp, groups=groups)
