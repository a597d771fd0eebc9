"""Multi-hypothesis 3-D key-point detector (reference: modules/keypoint_detector_integral_multi.py:7-88).

`net` (ResNet-50 + deconv head) produces logits [B, K*D, D, D] with NHWC storage, D = depth_dim = input side / 4 (64 for
the 256^2 patches of the shipped configurations; any multiple of 4 up to 128 is taken); the softmax over
D*H*W, the three marginals, the depth-peak top-k and the windowed expectations run as ONE fused HIP
reduction that reads the logits once (xas_head_softargmax_fwd) instead of ~15 ATen kernels and five
passes over a 604 MB tensor.  Ties between equal peak scores resolve to the lower depth bin.
"""
import torch
import torch.nn as nn

from modules.integral_base_modules.network import get_default_network_config, get_pose_net
from xas_amd import ops_head, ops_nn


class KPDetector3DMulti(nn.Module):
    def __init__(self, name, num_kp, depth_dim, num_hypo, neighbor_size, num_layers=50):
        super().__init__()
        cfg = get_default_network_config()
        cfg.depth_dim = depth_dim
        cfg.num_layers = num_layers
        self.num_hypo = num_hypo
        self.neighbor_size = neighbor_size
        self.num_kp = num_kp
        self.depth_dim = depth_dim
        self.net = get_pose_net(cfg, num_joints=num_kp)
        self.name = name
        # the final 1x1 convolution writes the head's first-pass records from its epilogue (forward half)
        last = self.net.head.features[-1]
        if hasattr(last, 'head_kd') and depth_dim == 64:
            last.head_kd = (num_kp, depth_dim)
        self.last_peak_indices = None      # int64 [B, K, num_hypo] of the latest forward (diagnostics / tests)

    def forward(self, x):
        ops_head.check_patch_size(x, self.depth_dim, 'KPDetector3DMulti')
        heatmap = self.net(x)
        kps, depth_prob_map, idx = ops_head.softargmax_multi(heatmap, self.num_kp, self.num_hypo, self.neighbor_size)
        self.last_peak_indices = idx
        return kps, depth_prob_map

    @torch.no_grad()
    def forward_logits(self, x):
        """forward plus the logits the head ran on: -> (kps, depth_prob_map, heatmap [B, K*D, D, D] in the head's NHWC
        storage), for ops_eval.triangulate_volume.  The caller keeps the 604 MB (B = 32) alive.  For eval(): records no graph."""
        ops_head.check_patch_size(x, self.depth_dim, 'KPDetector3DMulti')
        heatmap = self.net(x)
        kps, depth_prob_map, idx = ops_head.softargmax_multi(heatmap, self.num_kp, self.num_hypo, self.neighbor_size)
        self.last_peak_indices = idx
        return kps, depth_prob_map, ops_head._nhwc_storage(heatmap)

    def forward_flip(self, x, flip_pairs):
        """Flip test (eval() only, no autograd): x and its horizontal mirrors go through the network as ONE batch of 2B
        images - batch norm uses running statistics, so the mirrors change nothing for the originals - and the head runs on
        the average of each heat-map and the mirrored, left/right-swapped heat-map of its mirror, formed from the first-pass
        records alone (ops_head.softargmax_flip).  flip_pairs: model_params.flip_pairs.  -> what forward returns."""
        x2, perm = ops_head.detector_flip_input(self, x, flip_pairs, 'KPDetector3DMulti')
        heatmap = self.net(x2)
        kps, depth_prob_map, idx = ops_head.softargmax_flip(heatmap, self.num_kp, self.num_hypo, self.neighbor_size, perm)
        self.last_peak_indices = idx
        return kps, depth_prob_map

    @torch.no_grad()
    def forward_spread(self, x, flip_pairs=None):
        """forward (forward_flip when flip_pairs is given) plus the spatial spread of the heat-map the head ran on:
        -> (kps, depth_prob_map, spread [B, K, 5] = (E w, E h, Var w, Var h, Cov) in heat-map cells, ops_head.heatmap_spread;
        with flip_pairs the spread of the averaged heat-map, ops_head.spread_flip).  One more pass over the logits.  For
        eval(): records no graph."""
        if flip_pairs is None:
            ops_head.check_patch_size(x, self.depth_dim, 'KPDetector3DMulti')
            heatmap = self.net(x)
            kps, depth_prob_map, idx = ops_head.softargmax_multi(heatmap, self.num_kp, self.num_hypo, self.neighbor_size)
        else:
            x2, perm = ops_head.detector_flip_input(self, x, flip_pairs, 'KPDetector3DMulti')
            heatmap = self.net(x2)
            kps, depth_prob_map, idx = ops_head.softargmax_flip(heatmap, self.num_kp, self.num_hypo, self.neighbor_size, perm)
        self.last_peak_indices = idx
        return kps, depth_prob_map, ops_head.detector_spread(self, heatmap, flip_pairs)

    def forward_groups(self, x, groups, prefix_groups=0):
        """The reference's `groups` consecutive calls forward(x[0:B]), forward(x[B:2B]), ... as ONE pass over the
        concatenated batch: convolutions see G*B images, every batch-norm layer keeps per-call statistics and applies
        its running-statistic updates in call order (ops_nn.bn_groups).  -> kps [G*B, Hy, K, 3], depth maps [G, K, D].
        prefix_groups = P > 0 (ops_nn: prefix pass): the first P calls record no graph (the discriminator step's
        detector pass, model.py:231).  `x` is then the TAIL view [(G-P)*B, ...] of one image buffer [G*B, ...] whose
        first P*B images are those calls' inputs; -> (kps of the G-P graph calls, depth maps [G, K, D], kps of the prefix
        calls [P*B, Hy, K, 3], no graph)."""
        ops_head.check_patch_size(x, self.depth_dim, 'KPDetector3DMulti')
        if not prefix_groups:
            with ops_nn.bn_groups(groups):
                heatmap = self.net(x)
            kps, depth_prob_map, idx = ops_head.softargmax_multi(heatmap, self.num_kp, self.num_hypo, self.neighbor_size,
                                                                groups=groups)
            self.last_peak_indices = idx
            return kps, depth_prob_map
        per_group = x.shape[0] // (groups - prefix_groups)
        with ops_nn.bn_groups(groups, prefix_groups, per_group):
            heatmap = self.net(x)
            kps, depth_prob_map, idx = ops_head.softargmax_multi(heatmap, self.num_kp, self.num_hypo, self.neighbor_size,
                                                                groups=groups)
        self.last_peak_indices = idx
        return kps, depth_prob_map, ops_head._last_prefix[0]
