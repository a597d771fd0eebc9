#!/usr/bin/env python3
"""torchrun entry of the MI355X-native evaluation (reference: eval.py:1-408, same CLI and result file).

    torchrun --nproc-per-node=N eval.py --config config/HM36_Multi_SurS1.yaml --checkpoint ckpt.pth.tar
             [--batch_size B --worker W --multi_hypo best|confident] [--synthetic STEPS] [--ema] [--flip]
             [--tri dlt|robust --tri_thresh PX] [--resolve gt|views] [--tri-weight depth|spread]
             [--tri-refine none|lm --tri-huber PX] [--tri-skeleton --tri-sym W]
             [--tri-volume --tri-vol-side MM --tri-vol-grid G --tri-vol-levels N]
             [--fit-smpl OUT.npz --smpl-model ROOT|.npz --fit-iters N --fit-pose-prior W --fit-shape-prior W]
             [--calibrate OUT.npz --calib-iters N --calib-prior-rot W --calib-prior-trans W --calib-free MASK]
             [--calibration IN.npz]
             [--smooth OUT.npz --smooth-acc W --smooth-gap FRAMES --smooth-iters N]
             [--resolve-track OUT.npz --rt-vel W --rt-hyp W --rt-swap W --rt-gap FRAMES]
             [--smooth-data reproj|anchor --smooth-depth W --smooth-anchor-huber D]
             [--fit-shape frame|track --fit-gap FRAMES --fit-smooth [W_ROT] --fit-smooth-trans W]

One evaluation batch = the detector in eval mode on every camera, then ON THE DEVICE: left/right switch +
hypothesis selection + 2-D error (one launch per camera), patch->world of every view, DLT triangulation of all
joints (one launch), MPJPE / N-MPJPE / P-MPJPE / PCK / AUC of every prediction set (one launch each), and ONE
host transfer of the per-sample numbers that the per-action tables (host dictionaries, as in the reference)
accumulate.  The reference does the same work with per-hypothesis tensor chains, a batched fp32 SVD and numpy
SVDs on the host (eval.py:111-204, metrics.py).  TensorBoard pose images (eval.py:150-156,172-202) are
visualisation and are not rebuilt.

--resolve views (opt-in; the default, gt, is the reference's evaluation unchanged) decides the left/right exchange of every
view and the depth hypothesis of every view and joint from the agreement of the cameras in one launch
(ops_eval.multiview_resolve) instead of from the labels; the labels then only name each left/right pair, once per sample for
all views.  --multi_hypo is ignored in that mode.  No accuracy or time figure of that mode has been measured, neither on real
data nor on the device.

--tri-weight spread (opt-in; the default, depth, is the reference's weight unchanged: the joint's depth in mm) weighs every view
of a joint in the triangulation (both --tri modes) and in --resolve views by 1 / sigma of its heat-map in full-image pixels
(ops_head.heatmap_spread -> modules.util.spread_weight): one more streaming pass over each camera's logits.  No accuracy or
time figure of that mode has been measured either.

--tri-refine lm (opt-in; the default, none, runs exactly the calls above) moves every triangulated joint from the DLT's point,
which minimises an algebraic error, to the minimum of the reprojection error in pixels over the cameras the triangulation used
(ops_eval.triangulate_refine: Levenberg-Marquardt in one launch; --tri-huber PX makes the loss Huber's).  With --tri-weight
spread every residual counts in sigmas of its heat-map.  No accuracy figure has been measured: its effect on MPJPE is unknown.

--tri-skeleton (opt-in; model_params.tri_refine = 'skeleton'; it takes the place of --tri-refine, whose two choices stay as
they were) refines the joints of a sample TOGETHER instead: the same reprojection error over the same
cameras, plus --tri-sym W (px^2 per mm^2, default 0.1) times the squared difference in length of every left/right limb pair,
upper and lower arm and leg (ops_eval.triangulate_skeleton: one wave per sample, one launch).  A limb seen well on one side
then says how long its mirror is, where a wrist or elbow is ill determined along the rays.  A joint that lm would pass through
stays where it was and switches its limb pairs off.  Unknown: its effect on MPJPE, and the right --tri-sym; the default only
puts a 1 mm mismatch on the scale of a 1 px residual at roughly 0.3 px per mm.

--tri-volume (opt-in; model_params.tri_volume) runs after whatever the options above produced and starts from that point: a
voxel grid round it (--tri-vol-side MM, --tri-vol-grid G voxels per side, --tri-vol-levels N, each level half the side of the
one before, round its result) is looked up in every camera's heat-map cube, the log-probabilities are added (a product of
experts) and the soft-argmax of the fused volume, in world space, replaces the point (ops_eval.triangulate_volume: one
launch).  Every stage above sees ONE point per camera and joint, the soft-argmax of its heat-map, which lies between the
modes of a two-mode heat-map; here the whole distributions meet and the other cameras choose the mode.  The cameras are those
the triangulation used (--tri robust: its inliers), each reading the heat-map channel that the left/right decisions above
assigned to the joint.  The detector's logits of all cameras stay alive until then: V x 604 MB at B = 32, D = 64, K = 18.
Not with --flip.  Unknown: its effect on MPJPE (no checkpoint or dataset here), and the right grid: the defaults are read off
the cell size (31 mm), not tuned.

--fit-smpl OUT.npz (opt-in; model_params.fit_smpl) runs after everything else, on the final world joints (the triangulated
ones with several cameras, the selected hypothesis with one): SMPL parameters per sample by a double-precision
Levenberg-Marquardt on the device (xas_amd.ops_smplfit.fit_smpl, one launch per batch).  A joint that is not finite or that a
solver above passed through counts 0; with a covariance (--tri-volume, or --tri-refine lm with --tri-weight spread) a joint
counts 1 / trace(cov), normalised to mean 1 per sample.  OUT.npz (`pose` [N,72], `betas`, `trans`, `cost`, `status`,
`joint_rms_mm`) is a bank that train.py --pseudo-online reads as it is; eval_result.txt gains one last line.  Unknown: how good
the fits are on real detections (no checkpoint or dataset here), and the prior weights, which are untuned guesses.

--fit-shape track (opt-in with --fit-smpl; model_params.fit_shape; one rank; without it exactly the calls above) keeps every
batch's fit targets, weights and first-camera paths on the device and, after the loop, runs one fit_smpl_tracks over the whole
set: tracks from tracks_of(paths, --fit-gap), ONE beta vector per track, pose and translation per frame, warm-started from the
per-sample fits.  In OUT.npz `pose`, `betas` (each row its track's), `trans`, `cost`, `status` and `joint_rms_mm` then come from
the track fit, and `betas_per_frame`, `track`, `frame`, `track_betas`, `track_status`, `track_trials` join; the FIT line gains
the number of tracks and their mean length, joint RMS per frame -> per track and the mean within-track standard deviation of
the per-frame betas.  There is no temporal prior on the pose unless --fit-smooth asks for one.

--fit-smooth [W_ROT] and --fit-smooth-trans W (opt-in with --fit-shape track; model_params.fit_smooth, fit_smooth_trans; without
them exactly the calls above) make that one call fit_smpl_tracks_smooth: the same problem plus an acceleration prior on the 72
angles (W_ROT, mm^2 per rad^2) and the translation (W) over the frames of a track, the root vectors unwrapped along it.
OUT.npz gains `fit_smooth` [2] (the weights) and `joint_accel_mm` [N,3] (the norm of the second difference of the fitted joints
over the frames, mean over the joints: of the per-frame fits, NaN (no unsmoothed track fit is run), of the result; NaN at a
track's ends and at frames passed through); the FIT line ends with its mean before and after and the joint RMS before and after.
Both weights are untuned guesses.

--fit-data reproj (opt-in with --fit-smpl; model_params.fit_data; default joints = exactly the calls above, nothing new
imported; not with --fit-shape track, not with --flip) fits the body to the DETECTIONS: per batch the joint fit runs as before
and is the warm start, then xas_amd.ops_smplfit.fit_smpl_views holds every model joint to the pixels of the cameras that see it
(the batch's triangulation inputs; --tri-weight spread scales the residuals, --tri-huber is Huber's delta, the robust inliers
are the views) and to a 3-D anchor: with one camera the selected world point with information --smooth-depth along its ray,
with more none unless --tri-volume ran (the fused point with the inverse of its covariance).  --fit-pose-prior and
--fit-shape-prior, when given, apply to both fits; otherwise each has its own defaults.  OUT.npz stays a bank: `pose`, `betas`,
`trans`, `cost` (px^2), `status` and `joint_rms_mm` come from the pixel fit; `fit_data`, `reproj_rms_px` [N,2] (at the warm
start and at the result, over the observations used) and the warm start `pose_joints`, `betas_joints`, `trans_joints` join; the
FIT line names the mode and the reprojection RMS before -> after.  Unknown: whether it helps on real detections, and every weight.

--calibrate OUT.npz (opt-in; model_params.calibrate; 2+ cameras, one rank) keeps every batch's triangulation inputs, final
points and the views they used on the device and, after the loop, runs one bundle adjustment of the camera extrinsics per rig
(xas_amd.ops_calib.calibrate_bundle).  OUT.npz holds the rigs' projection matrices (`keys`) and their corrections (`delta`:
rotation vector in rad, translation in mm) with `cost`, `rms`, `status` and `cam_cov`; eval_result.txt gains one line per rig.
--calibration IN.npz (model_params.calibration; not with --calibrate) applies such a file: the cameras of every batch are
corrected before anything is predicted from them (modules.util.apply_calibration), while the ground truth keeps reading the
cameras as given.  Unknown: what either does to MPJPE on real rigs, and the prior weights.

--smooth OUT.npz (opt-in; model_params.smooth; 2+ cameras, one rank) keeps the same rows plus the ground truth and the image
paths, which name the sequence and frame of every sample, and after the loop smooths every joint's triangulated track over the
frames of its sequence: reprojection cost plus --smooth-acc times the squared acceleration, frames without data filled
(xas_amd.ops_track.track_smooth).  OUT.npz holds `joints`, `status`, `track`, `frame`, `track_status`, `cost` and `trials`;
eval_result.txt gains two lines.  Unknown: its effect on MPJPE on real sequences, and the right --smooth-acc.

--resolve-track OUT.npz (opt-in; model_params.resolve_track; one rank, any number of cameras) keeps every camera's raw
detections and, after the loop and without labels, chooses per camera every joint's depth hypothesis and every limb pair's
left/right exchange over the frames of its sequence: motion cost plus priors, exact by dynamic programming
(xas_amd.ops_track.track_resolve).  OUT.npz holds per camera `joints`, `sel`, `hyp`, `swap`, `status`, `cost`, `named`,
`track` and `frame`; eval_result.txt gains one line per camera, which also states the MPJPE of the choice made with labels.
Unknown: its accuracy on real detections, and the weights, untuned guesses all four.

--smooth-data anchor (opt-in with --smooth; model_params.smooth_data; the default, reproj, makes exactly the calls above) holds
the tracks by a 3-D anchor per frame and joint (xas_amd.ops_track.track_anchor_smooth), which lets --smooth run with ONE camera:
that camera's pixels, known across the ray, plus its selected world point (--resolve-track's choice, `cam_<c>_joints`, when that
flag is given too), known --smooth-depth W along it, under Huber's loss (--smooth-anchor-huber D) so that a wrongly chosen
hypothesis is an outlier.  With 2+ cameras it needs --tri-volume and smooths the fused points with the inverse of their
covariance, no pixels: the cost is then in sigma^2, and --smooth-acc weighs against it, not against pixels.  OUT.npz gains
`anchored`; the two SMOOTH lines name the mode.  Unknown: its accuracy on real detections; both new constants are untuned.

--smooth-bones [W] (opt-in with --smooth and either --smooth-data; model_params.smooth_bones; without it exactly the calls above)
makes the one call after the loop xas_amd.ops_track.track_skeleton_smooth on the same kept tensors: all joints of a track at
once, coupled in every frame, gap frames included, by the lengths of the bones of model_params.parent_ids (the per-track
medians of the points the smoother starts from, track_bone_lengths).  OUT.npz gains `bones`, `bone_length` and `bone_err`, its
`track_status`, `cost` and `trials` are per track, and the two SMOOTH lines end with the bone-length RMS before and after (over
all active bones; over the bones at a filled joint).
Unknown: its accuracy on real detections; W is an untuned guess; the workspace is 74 KB per frame at K = 18.

The post-loop options keep their rows in the plain lists fit_rows, calib_rows, smooth_rows and rt_rows and write their files
(atomically) from record().
"""
import copy
import os
from argparse import ArgumentParser
from collections import namedtuple

import numpy as np

os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')   # dmabuf IPC (RCCL between processes) on this driver
import torch
import yaml
from torch.distributed import destroy_process_group, init_process_group

from metrics import pose_errors
from modules.keypoint_detector_integral import KPDetector3D as KPDetector3D_integral
from modules.keypoint_detector_integral_multi import KPDetector3DMulti as KPDetector3DMulti_integral
from modules.util import (apply_calibration, convert_patch_to_world, resolve_views_weighted, spread_weight, triangulation_inputs,
                          triangulation_refined, triangulation_skeleton, triangulation_volume, triangulation_weighted)
from eval_utils import cal_per_class_error
from xas_amd import ops_eval, ops_head
from xas_amd.synthetic import synthetic_eval_batch

ACTIONS = ('Directions', 'Discussion', 'Eating', 'Greeting', 'Phoning', 'Posing', 'Purchases', 'Sitting',
           'SittingDown', 'Smoking', 'TakingPhoto', 'Waiting', 'Walking', 'WalkDog', 'WalkTogether')
act = {name: 0.0 for name in ACTIONS}
act_idx_2_name = {i + 2: name for i, name in enumerate(ACTIONS)}              # eval.py:31-36
METRICS_3D = (('mpjpe', 0), ('n-mpjpe', 1), ('p-mpjpe', 2))                   # alignment none / scale / procrustes


def update_dict(record_table, count_table, error, act_names):
    """Per-action accumulation (eval.py:38-42): the action id sits in characters 4-5 of the sample's `act`."""
    for i, item in enumerate(act_names):
        name = act_idx_2_name[int(item[4:6])]
        record_table[name] += error[i]
        count_table[name] += 1


def ddp_setup():
    init_process_group(backend='nccl')            # RCCL on ROCm
    torch.cuda.set_device(int(os.environ['LOCAL_RANK']))


# What the stages of Eval.eval_batch hand on.  A field is None where the options that ran produce none.
#   sel {cam: [B,K,3]} the selected joints in the patch; trans [B,K,1] the views that exchanged each joint; chan, per camera,
#   [B,K] int32 the heat-map channel each joint was read from (tri_volume); raw {cam: [B,Hy,K,3]} the detections as they came;
#   weights {cam: [B,K]} (tri_weight='spread'); cubes {cam: logits} (tri_volume); out: the stage's entries of the result
Selection = namedtuple('Selection', 'sel trans chan raw weights cubes out')
#   point [B,K,3] world mm; used [B,K] uint8 the views behind it (tri='robust'); bad [B,K] joints a solver passed through and
#   cov [B,K,6] mm^2 (both fit_smpl only); inputs (points [B,V,K,3], projection matrices [B,V,3,4]), formed once per batch
Triangulated = namedtuple('Triangulated', 'point used bad cov inputs out')

# the per-batch figures of eval_batch's result that eval() sums and the lines of eval_result.txt report as means over the batches
MEANS = ('tri_inlier_views', 'resolve_exchanged', 'resolve_hyp0', 'tri_sigma', 'tri_refine_px', 'tri_refine_gain_px', 'tri_sym_mm',
         'tri_vol_move_mm', 'tri_vol_sigma_mm', 'tri_vol_status')


def check_cameras(cam_id_list, message, least=0):
    """An option's bound on the cameras, `least` to ops_eval.TRI_MAX_VIEWS of them: outside it a ValueError of `message`, formatted
    with that maximum and the number of cameras."""
    if not least <= len(cam_id_list) <= ops_eval.TRI_MAX_VIEWS:
        raise ValueError(message.format(ops_eval.TRI_MAX_VIEWS, len(cam_id_list)))


def check_single_rank(message):
    """An option that needs the whole set on one rank: a ValueError of `message` unless WORLD_SIZE is 1 or unset."""
    if int(os.environ.get('WORLD_SIZE', 1)) != 1:
        raise ValueError(message)


def save_npz(path, cols):
    """np.savez of `cols` at `path`, atomically: a temporary file beside it, then a rename."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = path + '.tmp.npz'
    np.savez(tmp, **cols)
    os.replace(tmp, path)


def cat_rows(rows, key):
    """Column `key` of the rows that the batches kept, as one: tensors concatenated, lists (the image paths) chained, and None
    where the rows hold None (no views, no paths)."""
    first = rows[0][key]
    if first is None:
        return None
    return [p for r in rows for p in r[key]] if isinstance(first, list) else torch.cat([r[key] for r in rows])


def joint_errors(joints, gt):
    """[N,K] mm between `joints` and `gt` without alignment (the MPJPE's terms); a joint that is not finite counts as the origin
    and is for the caller to mask out."""
    return pose_errors(torch.where(torch.isfinite(joints), joints, torch.zeros_like(joints)), gt, want=('err',))['err'][0]


def masked_mean(errors, mask):
    """Mean of errors[mask] as a float, NaN where the mask is empty."""
    return float(errors[mask].mean()) if bool(mask.any()) else float('nan')


def full_covariance(c):
    """[...,6] (xx xy xz yy yz zz, as the solvers write a covariance) -> [...,3,3]."""
    return torch.stack([c[..., 0], c[..., 1], c[..., 2], c[..., 1], c[..., 3], c[..., 4], c[..., 2], c[..., 4], c[..., 5]],
                       dim=-1).reshape(c.shape[:-1] + (3, 3))


def homogeneous(point):
    """[...,3+] -> [...,4]: the first three coordinates and a one, the form the solvers take their start in."""
    return torch.cat([point[..., :3], torch.ones_like(point[..., :1])], dim=-1).contiguous()


class Eval:
    """Same constructor and method signatures as the reference Eval (eval.py:63-107)."""

    def __init__(self, config, detector, eval_data, log_dir, img_size=256.0, flip_test=False, tri='dlt',
                 tri_thresh=ops_eval.TRI_ROBUST_PX, resolve='gt'):
        mp = config['model_params']                # the options after --resolve are no keys of the shipped configs: eval.py's flags
        cam_id_list = mp['cam_id_list']
        if tri not in ('dlt', 'robust'):
            raise ValueError('Unknown triangulation: {}'.format(tri))
        if resolve not in ('gt', 'views'):
            raise ValueError('Unknown resolve mode: {}'.format(resolve))
        tri_weight = mp.get('tri_weight', 'depth')
        if tri_weight not in ('depth', 'spread'):
            raise ValueError('Unknown triangulation weight: {}'.format(tri_weight))
        tri_refine = mp.get('tri_refine', 'none')
        if tri_refine not in ('none', 'lm', 'skeleton'):
            raise ValueError('Unknown triangulation refinement: {}'.format(tri_refine))
        if tri_refine != 'none':
            check_cameras(cam_id_list, "tri_refine='" + tri_refine + "' refines over at most {} cameras; cam_id_list has {}")
        if tri_refine == 'skeleton':
            num_kp = getattr(detector, 'num_kp', mp.get('detector_params', {}).get('num_kp'))
            if num_kp is not None and num_kp > ops_eval.SKEL_MAX_JOINTS:
                raise ValueError("tri_refine='skeleton' couples at most {} joints; the detector has {}".format(
                    ops_eval.SKEL_MAX_JOINTS, num_kp))
        tri_volume = bool(mp.get('tri_volume', False))
        if tri_volume and flip_test:
            raise ValueError('tri_volume fuses the heat-map cubes of the cameras; the flip test\'s head works on an average of two '
                             'cubes that is never formed in memory: --tri-volume does not go with --flip')
        if tri_volume:
            check_cameras(cam_id_list, 'tri_volume fuses at most {} cameras; cam_id_list has {}')
        self.gpu_id = int(os.environ.get('LOCAL_RANK', 0))
        self.config = config
        self.cam_id_list = cam_id_list
        self.cal_per_act = config['dataset_params']['dataset']['name'] != 'mpi_inf_3dhp'
        self.detector = detector.to(self.gpu_id)
        self.detector.eval()                       # BN uses running statistics; no DDP wrapper is needed to evaluate
        self.eval_data = eval_data
        self.log_dir = log_dir
        self.img_size = img_size
        self.flip_test = bool(flip_test)           # --flip: every image is evaluated together with its horizontal mirror
        self.tri, self.tri_thresh = tri, float(tri_thresh)   # --tri robust: DLT over the views that agree within tri_thresh px
        self.resolve = resolve                     # --resolve views: exchange and hypothesis by the cameras' agreement
        if resolve == 'views':
            check_cameras(cam_id_list, "resolve='views' decides by the agreement of the cameras and needs 2 to {} of them; "
                                       'cam_id_list has {}', least=2)
        self.sums = {}                             # key of MEANS -> [sum over the batches, batches]: see add() and mean()
        self.tri_weight = tri_weight               # --tri-weight spread: a view counts by its heat-map's 1 / sigma, not its depth
        self.spread = None                         # spread only: heat-map spread [B,K,5] of the latest detect()
        self.tri_refine = tri_refine               # --tri-refine lm: the triangulated point minimises the reprojection error in pixels
        self.tri_huber = float(mp.get('tri_huber', 0.0))   # lm and skeleton: Huber's delta, 0 = plain least squares
        self.tri_sym = float(mp.get('tri_sym', ops_eval.TRI_SYM_W))    # skeleton only: --tri-sym, px^2 per mm^2
        self.tri_volume = tri_volume               # --tri-volume: the cameras' heat-map cubes fused round the triangulated point
        self.vol_side = float(mp.get('tri_vol_side', ops_eval.TRI_VOL_SIDE_MM))
        self.vol_grid, self.vol_levels = int(mp.get('tri_vol_grid', ops_eval.TRI_VOL_G)), int(mp.get('tri_vol_levels', ops_eval.TRI_VOL_LEVELS))
        self.logits = None                         # volume only: the logits [B,K*D,D,D] of the latest detect()
        self.fit_smpl = mp.get('fit_smpl') or None     # --fit-smpl OUT.npz: SMPL parameters of the final world joints, a --pseudo-online bank
        if self.fit_smpl:
            # --fit-data reproj: after the joint fit, the pixel fit from it (joints = today's calls, nothing new imported)
            self.fit_data = mp.get('fit_data') or 'joints'
            if self.fit_data not in ('joints', 'reproj'):
                raise ValueError('fit_data is joints or reproj, got {!r}'.format(self.fit_data))
            if self.fit_data == 'reproj':
                if (mp.get('fit_shape') or 'frame') == 'track':
                    raise ValueError('fit_data reproj fits every sample to its own detections; the track fits have no pixel term yet: '
                                     '--fit-data reproj does not go with --fit-shape track')
                if flip_test:
                    raise ValueError('fit_data reproj reads the detections of the views as they were selected; with the flip test '
                                     'that pairing is not wired up yet: --fit-data reproj does not go with --flip')
                check_cameras(cam_id_list, 'fit_data reproj fits 1 to {} cameras; cam_id_list has {}', least=1)
            smpl = prepare_smpl(mp)                  # (Eval's signature is pinned: the model comes through model_params.smpl_model)
            if smpl[0] is None or smpl[1] is None:
                raise ValueError('fit_smpl needs an SMPL layer and the H36M joint regressor (eval.py --smpl-model)')
            from xas_amd import ops_smplfit          # only with the flag
            self.smpl_layer, self.h36m_regressor = smpl[0].to(self.gpu_id), smpl[1].to(self.gpu_id)
            self.fit_iters = int(mp.get('fit_iters', 30))
            self.fit_pose_prior = float(mp.get('fit_pose_prior', ops_smplfit.POSE_PRIOR))      # untuned guesses, both
            self.fit_shape_prior = float(mp.get('fit_shape_prior', ops_smplfit.SHAPE_PRIOR))
            self.fit_rows = []                         # per batch: the host arrays of the file
            if self.fit_data == 'reproj':
                from xas_amd import ops_track          # only with the flag
                self.fit_views_priors = (float(mp.get('fit_pose_prior', ops_smplfit.VIEWS_POSE_PRIOR)),      # untuned guesses, both
                                         float(mp.get('fit_shape_prior', ops_smplfit.VIEWS_SHAPE_PRIOR)))
                self.fit_depth = float(mp.get('smooth_depth', ops_track.TRACK_DEPTH_W))
            self.fit_shape = mp.get('fit_shape') or 'frame'    # --fit-shape track: one beta vector per track, after the loop
            if self.fit_shape not in ('frame', 'track'):
                raise ValueError('fit_shape is frame or track, got {!r}'.format(self.fit_shape))
            if self.fit_shape == 'track':
                check_single_rank('fit_shape track solves over whole tracks: run it on one rank')
                from xas_amd import ops_track
                self.fit_gap = int(mp.get('fit_gap', ops_track.TRACK_MAX_GAP))
                self.fit_track_rows = []               # per batch, on the device: targets, weights, usable joints, first-camera paths
            # --fit-smooth: an acceleration prior on pose and translation over the frames of a track (None = off: today's calls)
            self.fit_smooth = None
            if mp.get('fit_smooth') is not None or mp.get('fit_smooth_trans') is not None:
                if self.fit_shape != 'track':
                    raise ValueError('fit_smooth is a mode of --fit-shape track: it needs fit_shape track (model_params.fit_shape)')
                rot = ops_smplfit.FIT_SMOOTH_ROT if mp.get('fit_smooth') is None else float(mp['fit_smooth'])
                trans = ops_smplfit.FIT_SMOOTH_TRANS if mp.get('fit_smooth_trans') is None else float(mp['fit_smooth_trans'])
                self.fit_smooth = (rot, trans)
        elif (mp.get('fit_data') or 'joints') != 'joints':
            raise ValueError('fit_data reproj is a mode of --fit-smpl: it needs fit_smpl (model_params.fit_smpl)')
        elif (mp.get('fit_shape') or 'frame') != 'frame':
            raise ValueError('fit_shape track is a mode of --fit-smpl: it needs fit_smpl (model_params.fit_smpl)')
        elif mp.get('fit_smooth') is not None or mp.get('fit_smooth_trans') is not None:
            raise ValueError('fit_smooth is a mode of --fit-shape track: it needs fit_smpl (model_params.fit_smpl)')
        self.calibrate = mp.get('calibrate') or None   # --calibrate OUT.npz: bundle adjustment of the extrinsics over the whole set
        self.calibration = mp.get('calibration') or None   # --calibration IN.npz: every batch's cameras corrected by such a file
        if self.calibrate and self.calibration:
            raise ValueError('calibrate estimates corrections of the given cameras and calibration applies earlier ones: '
                             '--calibrate and --calibration do not go together')
        if self.calibrate:
            check_cameras(cam_id_list, 'calibrate needs 2 to {} cameras; cam_id_list has {}', least=2)
            check_single_rank('calibrate needs WORLD_SIZE == 1: a rank sees only its shard of the set, and a bundle over '
                              'several ranks is not built')
            from xas_amd import ops_calib              # only with the flag
            self.calib_iters = int(mp.get('calib_iters', 30))
            self.calib_prior_rot = float(mp.get('calib_prior_rot', ops_calib.CALIB_PRIOR_ROT))        # untuned guesses, both
            self.calib_prior_trans = float(mp.get('calib_prior_trans', ops_calib.CALIB_PRIOR_TRANS))
            self.calib_free = mp.get('calib_free')     # mask of the cameras that may move; None = all but camera 0
            self.calib_rows = []                       # per batch, on the device: points, pmat, init, views
        self.smooth = mp.get('smooth') or None         # --smooth OUT.npz: the joint tracks smoothed over time, over the whole set
        self.smooth_data = mp.get('smooth_data') or 'reproj'   # --smooth-data anchor: the tracks are held by 3-D anchors
        if self.smooth:
            if self.smooth_data not in ('reproj', 'anchor'):
                raise ValueError('Unknown smoothing data: {}'.format(self.smooth_data))
            if self.smooth_data == 'reproj':
                check_cameras(cam_id_list, 'smooth needs 2 to {} cameras; cam_id_list has {}', least=2)
            else:
                check_cameras(cam_id_list, "smooth_data='anchor' smooths 1 to {} cameras; cam_id_list has {}", least=1)
                if len(cam_id_list) > 1 and not tri_volume:
                    raise ValueError("smooth_data='anchor' with two or more cameras smooths the fused points of the volume with "
                                     'their covariance: it needs --tri-volume (model_params.tri_volume)')
            check_single_rank('smooth needs WORLD_SIZE == 1: a DistributedSampler deals the frames of a sequence out over '
                              'the ranks, and no rank sees a track')
            from xas_amd import ops_track              # only with the flag
            self.smooth_acc = float(mp.get('smooth_acc', ops_track.TRACK_ACC_W))                     # untuned guesses, both
            self.smooth_gap = int(mp.get('smooth_gap', ops_track.TRACK_MAX_GAP))
            self.smooth_iters = int(mp.get('smooth_iters', 30))
            self.smooth_depth = float(mp.get('smooth_depth', ops_track.TRACK_DEPTH_W))               # anchor only; untuned too
            self.smooth_anchor_huber = float(mp.get('smooth_anchor_huber', ops_track.TRACK_ANCHOR_HUBER))
            self.smooth_rows = []                      # per batch, on the device: points, pmat, init, views, gt (anchor, info); and the paths
            self.smooth_bones = mp.get('smooth_bones')         # --smooth-bones [W]: all joints of a track at once, coupled by bone lengths
            if self.smooth_bones is False:             # `smooth_bones: false` in a config is off, like no key
                self.smooth_bones = None
            if self.smooth_bones is not None:
                self.smooth_bones = ops_track.TRACK_BONE_W if self.smooth_bones is True else float(self.smooth_bones)   # an untuned guess
                self.bones = ops_track.bones_of(mp['parent_ids'])
        elif mp.get('smooth_bones') is not None and mp.get('smooth_bones') is not False:
            raise ValueError('smooth_bones couples the joints of --smooth: it needs smooth (model_params.smooth)')
        self.resolve_track = mp.get('resolve_track') or None   # --resolve-track OUT.npz: hypothesis and exchange chosen over time, per camera
        if self.resolve_track:
            check_single_rank('resolve_track needs WORLD_SIZE == 1: a DistributedSampler deals the frames of a sequence out '
                              'over the ranks, and no rank sees a track')
            from xas_amd import ops_track              # only with the flag
            self.rt_vel = float(mp.get('rt_vel', ops_track.TRACK_VEL_W))                             # untuned guesses, all four
            self.rt_hyp = float(mp.get('rt_hyp', ops_track.TRACK_HYP_W))
            self.rt_swap = float(mp.get('rt_swap', ops_track.TRACK_SWAP_W))
            self.rt_gap = int(mp.get('rt_gap', ops_track.TRACK_MAX_GAP))
            self.rt_rows = []                          # per batch, on the device: per camera kps, world, labels, view; gt; and the paths
            self.rt_joints = {}                        # after the loop: camera -> the chosen world joints of the whole set
        if self.calibration:
            with np.load(self.calibration) as f:
                self.calib_keys = torch.from_numpy(f['keys']).to(self.gpu_id)
                self.calib_delta = torch.from_numpy(f['delta']).to(self.gpu_id)

    def add(self, key, value):
        """One batch's figure (a scalar, or a vector such as tri_sym_mm [2] and tri_vol_status [4]) into the sum of `key`, in double."""
        value = float(value) if np.ndim(value) == 0 else np.asarray(value, dtype=np.float64)
        entry = self.sums.setdefault(key, [0.0, 0])
        entry[0], entry[1] = entry[0] + value, entry[1] + 1

    def mean(self, key, size=None):
        """Mean of `key` over the batches that produced it; without any, 0.0 (np.zeros(size) for a vector of that size)."""
        total, n = self.sums.get(key, (0.0 if size is None else np.zeros(size), 0))
        return total / max(n, 1)

    def option_lines(self):
        """The lines that the options add to eval_result.txt after the reference's, in their fixed order.  An option that is off
        adds none, so the file is then as it was; the post-loop options also write their files here."""
        lines, cams = [], len(self.cam_id_list)
        if self.tri == 'robust':
            lines.append('TRI inlier views ({} px): {} of {}'.format(self.tri_thresh, self.mean('tri_inlier_views'), cams))
        if self.resolve == 'views':
            lines.append('RESOLVE views: exchanged {} , hypothesis 0 kept {}'.format(self.mean('resolve_exchanged'), self.mean('resolve_hyp0')))
        if self.tri_weight == 'spread':
            lines.append('TRI weight spread: mean sigma {} px'.format(self.mean('tri_sigma')))
        if self.tri_refine == 'lm':
            lines.append('TRI refine lm (huber {}): reprojection RMS {} px, gained {} px'.format(
                self.tri_huber, self.mean('tri_refine_px'), self.mean('tri_refine_gain_px')))
        if self.tri_refine == 'skeleton':
            lines.append('TRI refine skeleton (huber {}, sym {}): reprojection RMS {} px, gained {} px, limb asymmetry {} -> {} mm'.format(
                self.tri_huber, self.tri_sym, self.mean('tri_refine_px'), self.mean('tri_refine_gain_px'), *self.mean('tri_sym_mm', 2)))
        if self.tri_volume:
            lines.append('TRI volume (side {} mm, grid {}, levels {}): moved {} mm, sigma {} mm'.format(
                self.vol_side, self.vol_grid, self.vol_levels, self.mean('tri_vol_move_mm'), self.mean('tri_vol_sigma_mm')))
            lines.append('TRI volume status: fused {} , passed through {} , mode on a face {} , logits not finite {}'.format(
                *self.mean('tri_vol_status', 4)))
        if self.fit_smpl:
            lines.append(self.write_fit())
        if self.calibrate:
            lines.extend(self.write_calibration())
        # --resolve-track's step runs before --smooth's, which with --smooth-data anchor and one camera takes its choice as the
        # anchors; its lines stay the last ones
        track_lines = self.write_resolve_track() if self.resolve_track else []
        if self.smooth:
            lines.extend(self.write_smooth())
        return lines + track_lines

    def write_calibration(self):
        """--calibrate: one bundle adjustment over everything the batches kept, the file and -> the lines of eval_result.txt,
        one per rig."""
        from xas_amd import ops_calib
        points, pmat, init, views = (cat_rows(self.calib_rows, k) for k in ('points', 'pmat', 'init', 'views'))
        rig, keys = ops_calib.rigs_of(pmat)
        r = ops_calib.calibrate_bundle(points, pmat, init, rig, views=views, free=self.calib_free,
                                       weighted=self.tri_weight == 'spread', huber_px=self.tri_huber,
                                       prior_rot=self.calib_prior_rot, prior_trans=self.calib_prior_trans,
                                       max_iter=self.calib_iters, num_rigs=keys.shape[0])
        cols = {k: r[k].cpu().numpy() for k in ('delta', 'cost', 'rms', 'status', 'cam_cov')}
        made = r['trials'].cpu().numpy()
        cols['keys'] = keys.cpu().numpy()
        save_npz(self.calibrate, cols)
        d = cols['delta']
        return ['CALIBRATE rig {} ({} of {} trials, prior rot {}, prior trans {}): reprojection RMS {} -> {} px, largest |omega| {} deg, '
                'largest |tau| {} mm, {}'.format(i, int(made[i, 0]), self.calib_iters, self.calib_prior_rot, self.calib_prior_trans,
                                                 cols['rms'][i, 0], cols['rms'][i, 1],
                                                 float(np.degrees(np.linalg.norm(d[i, :, :3], axis=-1).max())),
                                                 float(np.linalg.norm(d[i, :, 3:], axis=-1).max()),
                                                 ops_calib.STATUS_NAMES[int(cols['status'][i])]) for i in range(len(d))]

    def write_smooth(self):
        """--smooth: one track_smooth over everything the batches kept, the file and -> the two lines of eval_result.txt."""
        from xas_amd import ops_track
        points, pmat, init, gt, views, paths = (cat_rows(self.smooth_rows, k) for k in ('points', 'pmat', 'init', 'gt', 'views', 'paths'))
        track, frame = ops_track.tracks_of(paths, self.smooth_gap, count=len(points))
        if self.smooth_data == 'anchor':
            return self.write_smooth_anchor(points, pmat, init, gt, views, track, frame)
        if self.smooth_bones is not None:
            r = self.smooth_skeleton(points, pmat, init, track, frame, views)
        else:
            r = ops_track.track_smooth(points, pmat, init, track, frame, views=views, weighted=self.tri_weight == 'spread',
                                       huber_px=self.tri_huber, acc_w=self.smooth_acc, max_iter=self.smooth_iters)
        joints, status = r['xyzw'][..., :3].contiguous(), r['status']
        both = torch.isfinite(joints).all(-1) & torch.isfinite(init[..., :3]).all(-1)                  # [N,K]
        e_before, e_after = joint_errors(init[..., :3].contiguous(), gt), joint_errors(joints, gt)
        filled = (status == ops_track.STATUS_FILLED) & torch.isfinite(joints).all(-1)
        rms = lambda c: float(torch.sqrt((r['resid'][..., c] ** 2).nanmean()))
        cols = {'joints': joints, 'status': status, 'track_status': r['track_status'], 'cost': r['cost'], 'trials': r['trials']}
        cols = {k: v.cpu().numpy() for k, v in cols.items()}
        cols['track'], cols['frame'] = track, frame
        cols.update(self.bone_columns(r))
        save_npz(self.smooth, cols)
        S = len(r['tracks'])
        return [line + words for line, words in zip(['SMOOTH {} tracks of mean length {} (acc {}, gap {}, {} trials): TRI MPJPE {} -> {} mm, reprojection RMS {} -> {} px, '
                'gaps filled {} , passed through {}'.format(S, len(points) / S, self.smooth_acc, self.smooth_gap, self.smooth_iters,
                                                            masked_mean(e_before, both), masked_mean(e_after, both), rms(0), rms(1),
                                                            float((status == ops_track.STATUS_FILLED).float().mean()),
                                                            float((status == ops_track.STATUS_PASSED).float().mean())),
                'SMOOTH filled gap joints: MPJPE {} mm over {} joints'.format(masked_mean(e_after, filled), int(filled.sum()))],
            self.bone_words(r, filled))]

    def write_smooth_anchor(self, points, pmat, init, gt, views, track, frame):
        """--smooth --smooth-data anchor: one track_anchor_smooth over everything the batches kept, the file (write_smooth's
        columns and `anchored` [N,K]: the joint had a usable anchor) and -> the two lines.  One camera: the anchors are
        --resolve-track's choice where that ran, else the evaluation's own selected points, with information along the ray."""
        from xas_amd import ops_track
        anchor, one = cat_rows(self.smooth_rows, 'anchor'), len(self.cam_id_list) == 1
        if one:
            if self.resolve_track:
                anchor = self.rt_joints['cam_{}'.format(self.cam_id_list[0])]
                init = homogeneous(anchor)
            info = ops_track.ray_information(pmat[:, 0], anchor, self.smooth_depth)
        else:
            info = cat_rows(self.smooth_rows, 'info')
        if self.smooth_bones is not None:
            r = self.smooth_skeleton(points, pmat, init, track, frame, views, anchor=anchor, info=info,
                                     anchor_huber=self.smooth_anchor_huber)
        else:
            r = ops_track.track_anchor_smooth(points, pmat, init, track, frame, anchor=anchor, info=info, views=views,
                                              weighted=self.tri_weight == 'spread', huber_px=self.tri_huber,
                                              anchor_huber=self.smooth_anchor_huber, acc_w=self.smooth_acc, max_iter=self.smooth_iters)
        joints, status = r['xyzw'][..., :3].contiguous(), r['status']
        anchored = torch.isfinite(anchor).all(-1) & torch.isfinite(info).all(-1) & (info[..., 0] + info[..., 3] + info[..., 5] > 0)
        both = torch.isfinite(joints).all(-1) & torch.isfinite(init[..., :3]).all(-1)
        e_before, e_after = joint_errors(init[..., :3].contiguous(), gt), joint_errors(joints, gt)
        filled = (status == ops_track.STATUS_FILLED) & torch.isfinite(joints).all(-1)
        rms = lambda c: float(torch.sqrt((r['resid'][..., c] ** 2).nanmean()))
        cols = {'joints': joints, 'status': status, 'track_status': r['track_status'], 'cost': r['cost'], 'trials': r['trials'],
                'anchored': anchored.to(torch.uint8)}
        cols = {k: v.cpu().numpy() for k, v in cols.items()}
        cols['track'], cols['frame'] = track, frame
        cols.update(self.bone_columns(r))
        save_npz(self.smooth, cols)
        S = len(r['tracks'])
        what = 'one camera, depth {}'.format(self.smooth_depth) if one else 'fused points'
        return [line + words for line, words in zip(['SMOOTH anchor ({}, huber {}) {} tracks of mean length {} (acc {}, gap {}, {} trials): {} MPJPE {} -> {} mm, '
                'reprojection RMS {} -> {} px, anchored {} , gaps filled {} , passed through {}'.format(
                    what, self.smooth_anchor_huber, S, len(points) / S, self.smooth_acc, self.smooth_gap, self.smooth_iters,
                    'VIEW' if one else 'TRI', masked_mean(e_before, both), masked_mean(e_after, both), rms(0), rms(1),
                    float(anchored.float().mean()), float((status == ops_track.STATUS_FILLED).float().mean()),
                    float((status == ops_track.STATUS_PASSED).float().mean())),
                'SMOOTH filled gap joints (anchor): MPJPE {} mm over {} joints'.format(masked_mean(e_after, filled), int(filled.sum()))],
            self.bone_words(r, filled))]

    SKELETON_WORKSPACE_WARN = 1 << 30        # bytes: above this smooth_skeleton says what it is about to allocate

    def smooth_skeleton(self, points, pmat, init, track, frame, views, **anchors):
        """--smooth-bones: the one call of --smooth as track_skeleton_smooth, the lengths the per-track medians of the points it
        starts from.  Its track_status, cost and trials are per track, not per (track, joint)."""
        from xas_amd import _lib, ops_track
        nbytes = _lib.query('xas_track_skeleton_workspace_bytes', points.shape[0], points.shape[2])
        if nbytes > self.SKELETON_WORKSPACE_WARN:
            print('SMOOTH bones: the solver keeps its factor per frame, a workspace of {:.1f} GB for {} frames'.format(
                nbytes / 1e9, points.shape[0]), flush=True)
        length = ops_track.track_bone_lengths(init, track, frame, self.bones)
        return ops_track.track_skeleton_smooth(points, pmat, init, track, frame, self.bones, length=length, views=views,
                                               weighted=self.tri_weight == 'spread', huber_px=self.tri_huber, acc_w=self.smooth_acc,
                                               bone_w=self.smooth_bones, max_iter=self.smooth_iters, **anchors)

    def bone_columns(self, r):
        """What --smooth-bones adds to the file: bones [Bn,2], bone_length [S,Bn], bone_err [N,Bn,2].  Nothing without it."""
        if self.smooth_bones is None:
            return {}
        return {'bones': self.bones, 'bone_length': r['length'].cpu().numpy(), 'bone_err': r['bone'].cpu().numpy()}

    def bone_words(self, r, filled):
        """What --smooth-bones appends to the two SMOOTH lines: the RMS over active bones and frames of (length in the frame -
        length of the track) before and after, and the same over the bones with a filled joint (filled [N,K]) in that frame.
        Nothing without it."""
        if self.smooth_bones is None:
            return '', ''
        bones = torch.as_tensor(self.bones, dtype=torch.long, device=filled.device)
        at_gap = (filled[:, bones[:, 0]] | filled[:, bones[:, 1]]).unsqueeze(-1)                          # [N,Bn,1]
        rms = lambda e: [float(torch.sqrt((e[..., c] ** 2).nanmean())) for c in (0, 1)]
        return (', bones ({} of weight {}): length RMS {} -> {} mm'.format(len(self.bones), self.smooth_bones, *rms(r['bone'])),
                ', bone length RMS at them {} -> {} mm'.format(*rms(torch.where(at_gap, r['bone'], torch.full_like(r['bone'], float('nan'))))))

    def write_resolve_track(self):
        """--resolve-track: one track_resolve per camera over everything the batches kept, the file and -> the lines of
        eval_result.txt, one per camera."""
        from xas_amd import ops_track
        rows = self.rt_rows
        gt = cat_rows(rows, 'gt')
        cols, lines = {}, []
        for c in self.cam_id_list:
            m = 'cam_{}'.format(c)
            kps, world, view, labels, paths = (cat_rows([r[m] for r in rows], k) for k in ('kps', 'world', 'view', 'labels', 'paths'))
            track, frame = ops_track.tracks_of(paths, self.rt_gap, count=len(kps))
            r = ops_track.track_resolve(kps, world, track, frame, vel_w=self.rt_vel, hyp_w=self.rt_hyp, swap_w=self.rt_swap,
                                        gt=labels, image_size=self.img_size)
            perm = ops_eval.switch_perm(kps.shape[2], ops_eval.SWITCH_PAIRS, kps.device)
            joints = ops_track.resolved_gather(world, r['hyp'], r['swap'], perm)[..., :3].contiguous()
            self.rt_joints[m] = joints                 # cam_<c>_joints, on the device: what write_smooth anchors one camera's tracks on
            first = world[:, 0, :, :3].contiguous()
            ok = torch.isfinite(joints).all(-1) & torch.isfinite(first).all(-1) & torch.isfinite(view).all(-1)
            for k, v in (('joints', joints), ('sel', r['sel']), ('hyp', r['hyp']), ('swap', r['swap']), ('status', r['status']),
                         ('cost', r['cost']), ('named', r['named'])):
                cols['{}_{}'.format(m, k)] = v.cpu().numpy()
            cols[m + '_track'], cols[m + '_frame'] = track, frame
            S = len(r['tracks'])
            paired = perm.long() != torch.arange(len(perm), device=perm.device)
            lines.append('RESOLVE track {}: {} tracks of mean length {} (vel {}, hyp {}, swap {}, gap {}): MPJPE hypothesis 0 as given {} '
                         '-> {} mm ({} with labels: {} mm), exchanged {} , hypothesis 0 kept {} , passed through {}'.format(
                             m, S, len(kps) / S, self.rt_vel, self.rt_hyp, self.rt_swap, self.rt_gap, masked_mean(joint_errors(first, gt), ok),
                             masked_mean(joint_errors(joints, gt), ok), rows[0]['mode'], masked_mean(joint_errors(view, gt), ok),
                             float(r['swap'][:, paired].float().mean()), float((r['hyp'] == 0).float().mean()),
                             float((r['status'] == ops_track.RESOLVE_PASSED).float().mean())))
        save_npz(self.resolve_track, cols)
        return lines

    def fit_batch(self, joints, bad, cov, paths=None, views=None):
        """--fit-smpl on the final world joints [B,18,3] of a batch.  A joint's weight is 0 where it is not finite or `bad`
        [B,18] marks it (a triangulation that passed it through), else 1, or with `cov` [B,18,6] (xx xy xz yy yz zz, mm^2)
        1 / trace(cov) normalised to mean 1 over the usable joints of the sample.  -> the file's rows, on the device.
        With fit_shape track the batch's targets, weights and `paths` (the first camera's image paths, or None) are kept too.
        With fit_data reproj that fit is the warm start of fit_batch_views on `views` (see there)."""
        from xas_amd import ops_smplfit
        ok = torch.isfinite(joints).all(dim=-1)
        if bad is not None:
            ok = ok & ~bad
        w = ok.float()
        if cov is not None:
            tr = cov[..., 0] + cov[..., 3] + cov[..., 5]
            ok = ok & torch.isfinite(tr) & (tr > 0)
            inv = torch.where(ok, 1.0 / tr.clamp(min=1e-30), torch.zeros_like(tr))
            w = inv / (inv.sum(dim=1, keepdim=True) / ok.float().sum(dim=1, keepdim=True).clamp(min=1.0)).clamp(min=1e-30)
        r = ops_smplfit.fit_smpl(joints, w, self.smpl_layer, self.h36m_regressor, iters=self.fit_iters,
                                 pose_prior=self.fit_pose_prior, shape_prior=self.fit_shape_prior)
        d2 = ((r['joints'] - torch.where(ok.unsqueeze(-1), joints.double(), r['joints'])) ** 2).sum(dim=-1)
        rms = (d2.sum(dim=1) / ok.double().sum(dim=1).clamp(min=1.0)).sqrt()
        if self.fit_shape == 'track':                  # the per-sample fit is the warm start of write_fit_tracks
            self.fit_track_rows.append({'targets': joints, 'weights': w, 'ok': ok, 'paths': None if paths is None else [str(p) for p in paths]})
            if self.fit_smooth:                        # the per-frame fits' joints: the `before` column of joint_accel_mm
                self.fit_track_rows[-1]['joints'] = r['joints']
        rows = {'fit_pose': r['pose'].float(), 'fit_betas': r['betas'].float(), 'fit_trans': r['trans'].float(),
                'fit_cost': r['cost'].float(), 'fit_status': r['status'], 'fit_joint_rms_mm': rms.float()}
        if self.fit_data == 'reproj':
            rows = self.fit_batch_views(rows, r, joints, ok, views)
        return rows

    def fit_batch_views(self, rows, warm, joints, ok, views):
        """--fit-data reproj: fit_smpl_views on the batch's detections `views` = (points [B,V,K,3], P [B,V,3,4], inlier bytes
        or None, anchor, info or None), warm-started from the joint fit `warm`.  -> the file's rows: the pixel fit's, the warm
        start as *_joints, and reproj_rms_px [B,2] at the warm start and at the result over the observations used."""
        from xas_amd import ops_smplfit
        points, pmat, used, anchor, info = views
        r = ops_smplfit.fit_smpl_views(points, pmat, self.smpl_layer, self.h36m_regressor, warm, views=used, anchor=anchor, info=info,
                                       weighted=self.tri_weight == 'spread', huber=self.tri_huber, iters=self.fit_iters,
                                       pose_prior=self.fit_views_priors[0], shape_prior=self.fit_views_priors[1])
        bits = ((r['used'].unsqueeze(1).int() >> torch.arange(points.shape[1], device=points.device, dtype=torch.int32).view(1, -1, 1)) & 1).bool()

        def rms_px(Y):                                 # [B,18,3] float64 -> [B] over the (view, joint) pairs used
            h = torch.einsum('bvij,bkj->bvki', pmat.double()[..., :3], Y) + pmat.double()[..., 3].unsqueeze(2)
            d2 = ((h[..., :2] / h[..., 2:] - points[..., :2].double()) ** 2).sum(-1)
            return (torch.where(bits, d2, torch.zeros_like(d2)).sum(dim=(1, 2)) / bits.double().sum(dim=(1, 2)).clamp(min=1.0)).sqrt()
        d2 = ((r['joints'] - torch.where(ok.unsqueeze(-1), joints.double(), r['joints'])) ** 2).sum(dim=-1)
        rms = (d2.sum(dim=1) / ok.double().sum(dim=1).clamp(min=1.0)).sqrt()
        return {'fit_pose': r['pose'].float(), 'fit_betas': r['betas'].float(), 'fit_trans': r['trans'].float(),
                'fit_cost': r['cost'].float(), 'fit_status': r['status'], 'fit_joint_rms_mm': rms.float(),
                'fit_pose_joints': rows['fit_pose'], 'fit_betas_joints': rows['fit_betas'], 'fit_trans_joints': rows['fit_trans'],
                'fit_reproj_rms_px': torch.stack([rms_px(warm['joints']), rms_px(r['joints'])], dim=1).float()}

    def keep_fit_rows(self, host):
        """--fit-smpl: the fit_* entries of a batch's host arrays as one row of the file (none without the flag: no row)."""
        row = {k[4:]: v for k, v in host.items() if k.startswith('fit_')}
        if row:
            self.fit_rows.append(row)

    FIT_TRACKS_WORKSPACE_WARN = 1 << 30      # bytes: above this fit_tracks says what it is about to allocate

    def fit_tracks(self, cols):
        """--fit-shape track: one fit_smpl_tracks over the whole set, warm-started from the per-sample rows `cols`; the file's
        columns of the track fit replace theirs and the new ones join.  -> the words the FIT line gains."""
        from xas_amd import ops_smplfit, ops_track
        targets, weights, ok, paths = (cat_rows(self.fit_track_rows, k) for k in ('targets', 'weights', 'ok', 'paths'))
        dev, N = targets.device, targets.shape[0]
        track, frame = ops_track.tracks_of(paths, self.fit_gap, count=N)
        S = len(np.unique(track))
        sizer = ops_smplfit.tracks_smooth_workspace_bytes if self.fit_smooth else ops_smplfit.tracks_workspace_bytes
        nbytes = sizer(N, self.smpl_layer.th_v_template.shape[-2], S)
        if nbytes > self.FIT_TRACKS_WORKSPACE_WARN:
            print('FIT tracks: the solver keeps its factor per frame, a workspace of {:.1f} GiB for {} frames'.format(nbytes / 2.0 ** 30, N), flush=True)
        init = {k: torch.as_tensor(cols[k], device=dev) for k in ('pose', 'betas', 'trans')}
        if self.fit_smooth:
            r = ops_smplfit.fit_smpl_tracks_smooth(targets, weights, track, frame, self.smpl_layer, self.h36m_regressor, init=init,
                                                   iters=self.fit_iters, rot_w=self.fit_smooth[0], trans_w=self.fit_smooth[1],
                                                   pose_prior=self.fit_pose_prior, shape_prior=self.fit_shape_prior)
        else:
            r = ops_smplfit.fit_smpl_tracks(targets, weights, track, frame, self.smpl_layer, self.h36m_regressor, init=init,
                                            iters=self.fit_iters, pose_prior=self.fit_pose_prior, shape_prior=self.fit_shape_prior)
        d2 = ((r['joints'] - torch.where(ok.unsqueeze(-1), targets.double(), r['joints'])) ** 2).sum(dim=-1)
        rms = (d2.sum(dim=1) / ok.double().sum(dim=1).clamp(min=1.0)).sqrt()
        per_frame, rms_frame = cols['betas'], cols['joint_rms_mm']
        fitted = (r['status'] != ops_smplfit.STATUS_PASSED).cpu().numpy()
        cols.update(pose=r['pose'].float().cpu().numpy(), betas=r['betas'].float().cpu().numpy(), trans=r['trans'].float().cpu().numpy(),
                    cost=r['cost'].float().cpu().numpy(), status=r['status'].cpu().numpy(), joint_rms_mm=rms.float().cpu().numpy(),
                    betas_per_frame=per_frame, track=r['track'].cpu().numpy(), frame=np.asarray(frame, np.int32),
                    track_betas=r['track_betas'].float().cpu().numpy(), track_status=r['track_status'].cpu().numpy(),
                    track_trials=r['track_trials'].cpu().numpy())
        spread = [per_frame[(cols['track'] == s) & fitted].std(axis=0).mean() for s in range(S) if ((cols['track'] == s) & fitted).any()]
        mean = lambda v: float(np.mean(v)) if len(v) else float('nan')
        if self.fit_smooth:
            before = cat_rows(self.fit_track_rows, 'joints').cpu().numpy()
            accel = np.stack([joint_accel_mm(before, cols['track'], cols['frame'], fitted), np.full(N, np.nan),
                              joint_accel_mm(r['joints'].cpu().numpy(), cols['track'], cols['frame'], fitted)], axis=1)
            cols.update(fit_smooth=np.asarray(self.fit_smooth, np.float64), joint_accel_mm=accel.astype(np.float32))
            nanmean = lambda v: float(np.nanmean(v)) if np.isfinite(v).any() else float('nan')
            smooth = ', smoothed over frames (weights {} {}): joint acceleration {} -> {} mm / frame^2, joint RMS {} -> {} mm'.format(
                self.fit_smooth[0], self.fit_smooth[1], nanmean(accel[:, 0]), nanmean(accel[:, 2]), mean(rms_frame[fitted]),
                mean(cols['joint_rms_mm'][fitted]))
        else:
            smooth = ''
        return ', shape per track: {} tracks of mean length {} (gap {}), joint RMS per frame {} -> per track {} mm, within-track std of the per-frame betas {}'.format(
            S, N / max(S, 1), self.fit_gap, mean(rms_frame[fitted]), mean(cols['joint_rms_mm'][fitted]), mean(spread)) + smooth

    def write_fit(self):
        """Writes the --fit-smpl file; passed-through samples are kept with their status.  -> the line of eval_result.txt."""
        from xas_amd import ops_smplfit
        shapes = {'pose': (0, 72), 'betas': (0, 10), 'trans': (0, 3), 'cost': (0, 2), 'status': (0,), 'joint_rms_mm': (0,)}
        cols = {k: (np.concatenate([r[k] for r in self.fit_rows]) if self.fit_rows else np.zeros(sh, np.uint8 if k == 'status' else np.float32))
                for k, sh in shapes.items()}
        words = self.fit_tracks(cols) if self.fit_shape == 'track' and self.fit_rows else ''
        if self.fit_data == 'reproj':
            return self.write_fit_views(cols)
        save_npz(self.fit_smpl, cols)
        n = max(len(cols['status']), 1)
        fitted = cols['status'] != ops_smplfit.STATUS_PASSED
        rms = float(cols['joint_rms_mm'][fitted].mean()) if fitted.any() else float('nan')
        share = ' , '.join('{} {}'.format(name, float((cols['status'] == c).sum()) / n) for c, name in enumerate(ops_smplfit.STATUS_NAMES))
        return 'FIT smpl ({} trials, pose prior {}, shape prior {}): joint RMS {} mm; {}'.format(
            self.fit_iters, self.fit_pose_prior, self.fit_shape_prior, rms, share) + words

    def write_fit_views(self, cols):
        """--fit-data reproj: the file with the pixel fit's columns, `fit_data`, `reproj_rms_px` [N,2] and the warm start
        (pose_joints, betas_joints, trans_joints).  -> the FIT line with the mode and the reprojection RMS."""
        from xas_amd import ops_smplfit
        more = {'pose_joints': (0, 72), 'betas_joints': (0, 10), 'trans_joints': (0, 3), 'reproj_rms_px': (0, 2)}
        cols.update({k: (np.concatenate([r[k] for r in self.fit_rows]) if self.fit_rows else np.zeros(sh, np.float32)) for k, sh in more.items()})
        cols['fit_data'] = np.asarray(self.fit_data)
        save_npz(self.fit_smpl, cols)
        n = max(len(cols['status']), 1)
        fitted = cols['status'] != ops_smplfit.STATUS_PASSED
        mean = lambda v: float(v[fitted].mean()) if fitted.any() else float('nan')
        share = ' , '.join('{} {}'.format(name, float((cols['status'] == c).sum()) / n) for c, name in enumerate(ops_smplfit.STATUS_NAMES))
        return ('FIT smpl reproj ({} trials, pose prior {}, shape prior {}; joint fit: {}, {}): reprojection RMS {} -> {} px, '
                'joint RMS {} mm; {}').format(self.fit_iters, self.fit_views_priors[0], self.fit_views_priors[1], self.fit_pose_prior,
                                              self.fit_shape_prior, mean(cols['reproj_rms_px'][:, 0]), mean(cols['reproj_rms_px'][:, 1]),
                                              mean(cols['joint_rms_mm']), share)

    def detect(self, img):
        """Joints [B,Hy,K,3] of one camera's images: the detector's forward, or with flip_test its forward_flip (the head on
        the average of each heat-map and the mirrored, left/right-swapped heat-map of the mirrored image).  With
        tri_weight='spread' through forward_spread, which also leaves that heat-map's spread in self.spread.  With tri_volume
        through forward_logits, which leaves the logits in self.logits (never with flip_test)."""
        if self.tri_volume:
            kps, _, self.logits = self.detector.forward_logits(img)
            if self.tri_weight == 'spread':
                self.spread = ops_head.detector_spread(self.detector, self.logits, None)
            return kps
        if self.tri_weight == 'spread':
            pairs = self.config['model_params']['flip_pairs'] if self.flip_test else None
            kps, _, self.spread = self.detector.forward_spread(img, pairs)
            return kps
        if self.flip_test:
            return self.detector.forward_flip(img, self.config['model_params']['flip_pairs'])[0]
        return self.detector(img)[0]

    def convert_data_to_device(self, x):
        for key, v in x.items():
            if isinstance(v, torch.Tensor):
                x[key] = v.to(self.gpu_id, non_blocking=True)
            elif isinstance(v, dict):
                x[key] = self.convert_data_to_device(v)
            elif isinstance(v, np.ndarray):
                x[key] = torch.from_numpy(v).to(self.gpu_id)
        return x

    # ---- the stages of one batch, in the order eval_batch calls them ----

    def calibrated(self, x):
        """-> the batch the predictions read: `x` itself, or with --calibration a shallow copy whose cameras are corrected."""
        return apply_calibration(x, self.cam_id_list, self.calib_keys, self.calib_delta) if self.calibration else x

    def detect_camera(self, x, m, kps_by_cam, weights, cubes):
        """-> the detections [B,Hy,K,3] of camera `m`: the planted kps_by_cam[m] where given, else the detector's.  Under planted
        detections the detector still runs when the spread or the logits are needed, and only then: `weights` and `cubes`
        (None where the options want none) gain the camera's entry."""
        kps = self.detect(x[m + '_img']) if kps_by_cam is None or weights is not None or cubes is not None else None
        if weights is not None:
            weights[m] = spread_weight(self.spread, x[m + '_trans_image'])
        if cubes is not None:
            cubes[m] = self.logits                 # every camera's logits stay alive until the fusion
        return kps if kps_by_cam is None else kps_by_cam[m]

    def select_by_labels(self, x, cams, mode, kps_by_cam):
        """The reference's selection: left/right exchange and hypothesis of every view by its labels (ops_eval.eval_select, one
        launch per camera).  -> Selection; out: err2d_<cam> [B]."""
        weights, cubes = {} if self.tri_weight == 'spread' else None, {} if self.tri_volume else None
        sel, raw, out, trans, chan = {}, {}, {}, None, [] if self.tri_volume else None
        for m in cams:
            raw[m] = kps = self.detect_camera(x, m, kps_by_cam, weights, cubes)
            s = ops_eval.eval_select(kps, x[m + '_joints'], image_size=self.img_size, mode=mode)
            sel[m] = s['sel3d']
            out['err2d_' + m] = s['err2d']
            t = s['swapped'].float()
            trans = t if trans is None else trans + t
            if chan is not None:                   # the joint was taken from its partner's channel where eval_select exchanged
                K = s['swapped'].shape[1]
                perm = ops_eval.switch_perm(K, ops_eval.SWITCH_PAIRS, kps.device)
                chan.append(torch.where(s['swapped'].squeeze(-1), perm, torch.arange(K, device=kps.device, dtype=torch.int32)))
        return Selection(sel, trans, chan, raw, weights, cubes, out)

    def select_by_views(self, x, cams, kps_by_cam):
        """--resolve views: exchange and hypothesis of all views by the cameras' agreement in one launch; the labels only name
        each pair and then measure.  -> Selection; out: err2d_<cam> [B], resolve_exchanged and resolve_hyp0 (scalars)."""
        weights, cubes = {} if self.tri_weight == 'spread' else None, {} if self.tri_volume else None
        raw = {m: self.detect_camera(x, m, kps_by_cam, weights, cubes) for m in cams}
        sel, r = resolve_views_weighted(raw, x, self.cam_id_list, ops_eval.SWITCH_PAIRS, weights, gt=True)   # None: the depth
        out = {}
        for m in cams:                             # the labels' part from here on: measuring, no longer choosing
            out['err2d_' + m] = ops_eval.eval_select(sel[m].unsqueeze(1), x[m + '_joints'], image_size=self.img_size,
                                                     mode='confident', no_switch=True, want=('err2d',))['err2d']
        shifts = torch.arange(len(cams), device=r['swap'].device, dtype=torch.int32)
        count = lambda mask: ((mask.unsqueeze(-1).int() >> shifts) & 1).sum(dim=-1).float()     # [B,K] bits set
        trans = count(r['swap']).unsqueeze(-1)
        B, K = r['swap'].shape
        own = torch.arange(K, device=shifts.device, dtype=torch.int32)
        perm = ops_eval.switch_perm(K, ops_eval.SWITCH_PAIRS, shifts.device)
        paired = (perm != own).float()                                                            # [K], both of a pair
        before = torch.where(r['named'].bool(), count(r['valid']) - count(r['swap']), count(r['swap']))   # naming undone
        out['resolve_exchanged'] = (before * paired).sum() / (paired.sum().clamp(min=1.0) * B * len(cams))
        out['resolve_hyp0'] = (r['hyp'] == 0).float().mean()
        chan = None
        if self.tri_volume:                        # view v read joint k from perm[k] where bit v of swap is set
            chan = [torch.where(((r['swap'].int() >> v) & 1).bool(), perm, own) for v in range(len(cams))]
        return Selection(sel, trans, chan, raw, weights, cubes, out)

    def triangulate(self, s, x, cams):
        """The world joints of the selected views: the DLT or the robust DLT over inputs formed once, then --tri-refine lm or
        skeleton from its point.  One camera without robust or refinement: that view's own point, and no inputs.
        -> Triangulated; out: tri_refine_px, tri_refine_gain_px, tri_sym_mm [2], tri_inlier_views, tri_sigma, each with its option."""
        robust_px = self.tri_thresh if self.tri == 'robust' else None
        out, inputs, used, bad, cov = {}, None, None, None, None
        if len(cams) == 1 and self.tri == 'dlt' and self.tri_refine == 'none':      # nothing to triangulate (the DLT refuses one view)
            tri = convert_patch_to_world(s.sel[cams[0]], x, cams[0], is_norm=True)[..., :3]
        elif self.tri_refine == 'none':
            inputs = triangulation_inputs(s.sel, x, self.cam_id_list, s.weights)
            tri, used = triangulation_weighted(s.sel, x, self.cam_id_list, s.weights, robust_px=robust_px, return_inliers=True, inputs=inputs)
        else:                                      # the same start, then the pixel error minimised over the views it used
            inputs = triangulation_inputs(s.sel, x, self.cam_id_list, s.weights)
            want = ('resid',)
            if self.fit_smpl:                      # the joints passed through, and a covariance where the solver has a meaningful one
                want += ('status', 'cov') if self.tri_refine == 'lm' and s.weights is not None else ('status',)
            if self.tri_refine == 'lm':
                tri, r = triangulation_refined(s.sel, x, self.cam_id_list, s.weights, huber_px=self.tri_huber, want=want,
                                               robust_px=robust_px, inputs=inputs)
            else:                                  # the joints of a sample refined together
                tri, r = triangulation_skeleton(s.sel, x, self.cam_id_list, s.weights, huber_px=self.tri_huber, sym_w=self.tri_sym,
                                                want=want + ('sym',), robust_px=robust_px, inputs=inputs)
            used = r.get('inliers')
            out['tri_refine_px'] = r['resid'][..., 1].nanmean()            # a joint passed through or fixed has no residual (NaN)
            out['tri_refine_gain_px'] = (r['resid'][..., 0] - r['resid'][..., 1]).nanmean()
            if self.tri_refine == 'skeleton':
                out['tri_sym_mm'] = r['sym'].abs().reshape(-1, 2).nanmean(dim=0)   # [2]: before, after; a pair switched off is NaN
            if self.fit_smpl:
                bad, cov = r['status'] == 2, r.get('cov')
        if self.tri == 'robust':
            bits = (used.unsqueeze(-1).int() >> torch.arange(len(cams), device=used.device, dtype=torch.int32)) & 1
            # a zero mask is the fallback: no two views agreed, the DLT ran over all of them
            out['tri_inlier_views'] = torch.where(used == 0, len(cams), bits.sum(dim=-1)).float().mean()
        if s.weights is not None:
            out['tri_sigma'] = torch.stack([1.0 / s.weights[m] for m in cams]).mean()
        return Triangulated(tri, used, bad, cov, inputs, out)

    def fuse(self, t, s, x, cams):
        """--tri-volume: the cameras' heat-map cubes fused round the triangulated point, over the views that produced it.
        -> Triangulated with the fused point (and for fit_smpl its pass-through marks and covariance) in place of t's, `t` itself
        without the option; out gains tri_vol_move_mm, tri_vol_sigma_mm, tri_vol_status [4]."""
        if not self.tri_volume:
            return t
        views = None
        if self.tri == 'robust':                   # a zero mask is the fallback: the DLT ran over all views, and so does the fusion
            views = torch.where(t.used == 0, torch.full_like(t.used, (1 << len(cams)) - 1), t.used)
        tri, r = triangulation_volume(t.point, s.cubes, x, self.cam_id_list, torch.stack(s.chan, dim=0).contiguous(), views=views,
                                      G=self.vol_grid, levels=self.vol_levels, side_mm=self.vol_side, want=('cov', 'status'))
        out = dict(t.out)
        out['tri_vol_move_mm'] = (tri - r['init']).norm(dim=-1).nanmean()
        out['tri_vol_sigma_mm'] = (r['cov'][..., 0] + r['cov'][..., 3] + r['cov'][..., 5]).sqrt().nanmean()   # passed through: NaN
        out['tri_vol_status'] = torch.stack([(r['status'] == c).float().mean() for c in range(4)])
        # passed through (1, 3): the start came back and there is no covariance.  --smooth-data anchor reads both as --fit-smpl does
        if self.fit_smpl or (self.smooth and self.smooth_data == 'anchor'):
            return t._replace(point=tri, bad=(r['status'] == 1) | (r['status'] == 3), cov=r['cov'], out=out)
        return t._replace(point=tri, out=out)

    def keep_solver_rows(self, t, s, x, gt, cams):
        """--calibrate and --smooth: one row each of what their solver reads after the loop, kept on the device: the batch's
        triangulation inputs, the final point as the start (formed once, shared by the two) and the views it used.
        --smooth-data anchor adds the anchors.  One camera: its pixel points and matrix (formed here where nothing was
        triangulated) and its selected world point, whose information along the ray write_smooth forms.  More: the fused point
        with the inverse of its covariance, NaN where the volume passed the joint through, and weights of 0, which switch the
        reprojection term off."""
        if not (self.calibrate or self.smooth):
            return
        inputs = t.inputs if t.inputs is not None else triangulation_inputs(s.sel, x, self.cam_id_list, s.weights)
        row = {'points': inputs[0], 'pmat': inputs[1], 'views': t.used if self.tri == 'robust' else None, 'init': homogeneous(t.point)}
        if self.calibrate:
            self.calib_rows.append(dict(row))
        if self.smooth:
            paths = x.get(cams[0] + '_img_path')
            row = dict(row, gt=gt[..., :3].contiguous(), paths=None if paths is None else [str(p) for p in paths])
            if self.smooth_data == 'anchor':
                row['anchor'] = t.point[..., :3].contiguous()
                if len(cams) > 1:
                    from xas_amd import ops_track
                    row['info'] = ops_track.covariance_information(full_covariance(t.cov))
                    row['anchor'] = torch.where(t.bad.unsqueeze(-1), torch.full_like(row['anchor'], float('nan')), row['anchor'])
                    row['points'] = torch.cat([inputs[0][..., :2], torch.zeros_like(inputs[0][..., 2:])], dim=-1)
                    row['views'] = torch.zeros(t.bad.shape, dtype=torch.uint8, device=t.bad.device)
            self.smooth_rows.append(row)

    def measure(self, s, t, x, gt, cams):
        """The triangulated joints and every view's own against the ground truth (one pose_errors launch per set and kind).
        -> (preds {'tri', 'view_<cam>': world joints}, out: mpjpe_ / n-mpjpe_ / p-mpjpe_<set> [B], without per-action tables
        pck_ / auc_<set> (scalars), world_gt and world_tri)."""
        preds, out = {'tri': t.point}, {}
        for m in cams:
            preds['view_' + m] = convert_patch_to_world(s.sel[m], x, m, is_norm=True)
        for name, p in preds.items():
            e = pose_errors(p, gt, want=('err',))['err'].mean(dim=2)                       # [3,B]
            for metric, a in METRICS_3D:
                out['{}_{}'.format(metric, name)] = e[a]
            if not self.cal_per_act:                                                       # eval.py:51-55
                q = pose_errors(p, gt, in_div=1000.0, want=('pck', 'auc_hits'))
                out['pck_' + name] = q['pck'].mean()
                out['auc_' + name] = (q['auc_hits'].sum(dim=0).float() / q['pck'].numel()).mean() * 100
        out['world_gt'], out['world_tri'] = gt, preds['tri']
        return preds, out

    def keep_track_rows(self, s, x, gt, preds, cams, mode):
        """--resolve-track: one row of what track_resolve reads per camera after the loop, kept on the device: the detections as
        they came, in the patch and in the world, the labels, the view as selected with them, the paths; and the ground truth."""
        if not self.resolve_track:
            return
        row = {'gt': gt[..., :3].contiguous(), 'mode': 'views' if self.resolve == 'views' else mode}
        for m in cams:
            paths = x.get(m + '_img_path')
            if paths is None:                      # the cameras of a sample show the same frame
                paths = x.get(cams[0] + '_img_path')
            row[m] = {'kps': s.raw[m].detach().float().contiguous(), 'labels': x[m + '_joints'],
                      'world': convert_patch_to_world(s.raw[m], x, m, is_norm=True)[..., :3].contiguous(),
                      'view': preds['view_' + m][..., :3].contiguous(), 'paths': None if paths is None else [str(p) for p in paths]}
        self.rt_rows.append(row)

    def fit(self, t, s, preds, cams, x):
        """--fit-smpl, after everything else, on the final world joints: the triangulated ones with their pass-through marks and
        covariance, or with one camera that view's selected hypothesis.  -> out: the fit_* rows of fit_batch, {} without the option."""
        if not self.fit_smpl:
            return {}
        paths = x.get(cams[0] + '_img_path')       # read by fit_shape track alone
        views = self.fit_views(t, s, preds, cams, x) if self.fit_data == 'reproj' else None
        if len(cams) > 1:
            return self.fit_batch(preds['tri'][..., :3].contiguous(), t.bad, t.cov, paths, views)
        return self.fit_batch(preds['view_' + cams[0]][..., :3].contiguous(), None, None, paths, views)

    def fit_views(self, t, s, preds, cams, x):
        """--fit-data reproj: what fit_smpl_views reads of a batch: the triangulation inputs (formed here where nothing was
        triangulated), the robust inliers, and the anchors.  One camera: the selected world point with information along its
        ray.  More: none, unless --tri-volume ran: then the fused point with the inverse of its covariance, NaN where the volume
        passed the joint through."""
        from xas_amd import ops_track
        points, pmat = t.inputs if t.inputs is not None else triangulation_inputs(s.sel, x, self.cam_id_list, s.weights)
        used = t.used if self.tri == 'robust' else None
        anchor, info = None, None
        if len(cams) == 1:
            anchor = preds['view_' + cams[0]][..., :3].contiguous()
            info = ops_track.ray_information(pmat[:, 0], anchor, self.fit_depth)
        elif self.tri_volume:
            info = ops_track.covariance_information(full_covariance(t.cov))
            anchor = t.point[..., :3].contiguous()
            anchor = torch.where(t.bad.unsqueeze(-1), torch.full_like(anchor, float('nan')), anchor)
        return points, pmat, used, anchor, info

    @torch.no_grad()
    def eval_batch(self, x, mode='best', kps_by_cam=None):
        """Device part of one iteration of eval.py:111-204.  Returns ({name: tensor on the device}, layout) where
        every tensor is per sample [B] (errors), or a scalar (ambiguity, pck, auc).  With resolve='views' `mode` is ignored:
        the cameras' agreement picks the hypotheses."""
        cams = ['cam_{}'.format(c) for c in self.cam_id_list]
        given, x = x, self.calibrated(x)           # the ground truth reads the cameras as given; --calibration corrects the predictions'
        s = self.select_by_views(x, cams, kps_by_cam) if self.resolve == 'views' else self.select_by_labels(x, cams, mode, kps_by_cam)
        out = dict(s.out, ambiguity=torch.minimum(s.trans, len(cams) - s.trans).mean())    # eval.py:164-167
        gt = convert_patch_to_world(given['cam_0_joints'], given, 'cam_0', is_norm=False)  # eval.py:170
        t = self.fuse(self.triangulate(s, x, cams), s, x, cams)
        out.update(t.out)
        self.keep_solver_rows(t, s, x, gt, cams)
        preds, errors = self.measure(s, t, x, gt, cams)
        out.update(errors)
        self.keep_track_rows(s, x, gt, preds, cams, mode)
        out.update(self.fit(t, s, preds, cams, x))
        return out

    def eval(self, tb_log, record_table, count_table, record_3d_table, count_3d_table, record_3d_tri_table,
             count_3d_tri_table, ambiguity_ratio, mode='best'):
        cams = ['cam_{}'.format(c) for c in self.cam_id_list]
        for x in self.eval_data:
            x = self.convert_data_to_device(x)
            out = self.eval_batch(x, mode)
            host = {k: v.detach().cpu().numpy() for k, v in out.items() if not k.startswith('world')}   # the one sync
            for m in cams:
                if self.cal_per_act:
                    update_dict(record_table, count_table, host['err2d_' + m], x['act'])
                else:
                    record_table = record_table + host['err2d_' + m]
                    count_table += 1
            ambiguity_ratio = ambiguity_ratio + float(host['ambiguity'])
            for key in MEANS:                      # whatever the options of this run produce
                if key in host:
                    self.add(key, host[key])
            self.keep_fit_rows(host)
            for table, count, names in ((record_3d_tri_table, count_3d_tri_table, ['tri']),
                                        (record_3d_table, count_3d_table, ['view_' + m for m in cams])):
                for name in names:
                    for metric, _ in METRICS_3D:
                        err = host['{}_{}'.format(metric, name)]
                        if self.cal_per_act:
                            update_dict(table[metric], count[metric], err, x['act'])
                        else:
                            table[metric] = table[metric] + err
                            count[metric] += 1
                    if not self.cal_per_act:
                        for key in ('pck', 'auc'):
                            table[key] += float(host['{}_{}'.format(key, name)])
                            count[key] += 1
        return [record_table, count_table, record_3d_table, count_3d_table, record_3d_tri_table, count_3d_tri_table,
                ambiguity_ratio]

    def record(self, record_table, count_table, record_3d_table, count_3d_table, record_3d_tri_table,
               count_3d_tri_table, ambiguity_ratio):
        """Prints and writes <log_dir>/eval/eval_result.txt with the reference's lines (eval.py:206-296), then the options'."""
        lines = []
        if self.cal_per_act:
            full2d, sel2d = cal_per_class_error(record_table, count_table)
            full3d, sel3d = cal_per_class_error(record_3d_table, count_3d_table, multi=True)
            fulltri, seltri = cal_per_class_error(record_3d_tri_table, count_3d_tri_table, multi=True)
            for title, e2, e3, et in (('', full2d, full3d, fulltri), ('--------select---------', sel2d, sel3d, seltri)):
                if title:
                    lines.append(title)
                lines.append('2D MSE: {} %'.format(float(e2)))
                for tag, tbl in (('', e3), ('TRI ', et)):
                    for label, key in (('MPJPE', 'mpjpe'), ('N-MPJPE', 'n-mpjpe'), ('P-MPJPE', 'p-mpjpe')):
                        lines.append('{}{}: {} %'.format(tag, label, float(tbl[key])))
        else:
            lines.append('2D MSE: {} %'.format(float(np.mean(record_table) / count_table)))
            for title, tbl, cnt in (('---3D-----', record_3d_table, count_3d_table),
                                    ('---Tri3D-----', record_3d_tri_table, count_3d_tri_table)):
                lines.append(title)
                for key in tbl.keys():
                    if key in ('pck', 'auc'):
                        lines.append('{}: {} %'.format(key, float(tbl[key] / cnt[key])))
                    else:
                        lines.append('{}: {}'.format(key, float(np.mean(tbl[key]) / cnt[key])))
        lines.extend(self.option_lines())
        print('\n'.join(lines))
        os.makedirs(os.path.join(self.log_dir, 'eval'), exist_ok=True)
        path = os.path.join(self.log_dir, 'eval', 'eval_result.txt')
        with open(path, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        print('Results saved in {}'.format(path))
        print('Ambiguity Ratio:{}'.format(ambiguity_ratio / len(self.eval_data) / len(self.cam_id_list)))
        return lines


def prepare_smpl(mp):
    """--fit-smpl: the SMPL layer and the H36M regressor, loaded the way train.py loads them (model_params.smpl_model, the
    --smpl-model flag: a directory of the model files, or an .npz of exported arrays; None = smpl_layer_params.model_path)."""
    from xas_amd.engine import _load_smpl
    from xas_amd.pseudo import load_smpl_arrays
    path, arrays = mp.get('smpl_model'), None
    if path is not None and str(path).endswith('.npz'):
        arrays = load_smpl_arrays(path)
    elif path is not None:
        mp.setdefault('smpl_layer_params', {})['model_path'] = path
    elif not mp.get('smpl_layer_params', {}).get('model_path'):
        return None, None
    return _load_smpl(mp, arrays)


def prepare_model(config, opt):
    """Detector from the `unsup_model` entry of a training checkpoint (eval.py:298-314); with --ema from `unsup_model_ema`,
    the averaged weights a run with train_params.ema_decay saves beside it."""
    dp = config['model_params']['detector_params']
    detector = (KPDetector3DMulti_integral if dp['name'] == 'resnet_multi' else KPDetector3D_integral)(**dp)
    if opt.checkpoint is not None:
        checkpoint = torch.load(opt.checkpoint, map_location='cpu')
        key = 'unsup_model_ema' if getattr(opt, 'ema', False) else 'unsup_model'
        if key not in checkpoint:
            hint = ' (--ema needs a run with train_params.ema_decay set)' if key.endswith('_ema') else ''
            raise KeyError("checkpoint %s has no '%s' entry%s" % (opt.checkpoint, key, hint))
        detector.load_state_dict({k.replace('regressor.', ''): v for k, v in checkpoint[key].items()
                                  if 'regressor.' in k})
    return detector


class _SyntheticEvalLoader:
    def __init__(self, steps, batch, cams, device, seed=0):
        self.steps, self.batch, self.cams, self.device, self.seed = steps, batch, cams, device, seed

    def __len__(self):
        return self.steps

    def __iter__(self):
        for i in range(self.steps):
            yield synthetic_eval_batch(self.batch, self.cams, self.device, seed=self.seed + i)


def prepare_data(config, world_size, worker, synthetic_steps=0, device='cuda'):
    bs = config['train_params']['batch_size'] // world_size
    if synthetic_steps:
        return _SyntheticEvalLoader(synthetic_steps, bs, config['dataset_params']['cam_id_list'], device)
    from torch.utils.data import DataLoader
    from torch.utils.data.distributed import DistributedSampler
    from train_util import basic_data              # the reference's CPU dataset code (cv2, scikit-fmm)
    ds = basic_data(config, eval_only=True)
    return DataLoader(ds, batch_size=bs, shuffle=False, num_workers=worker, drop_last=False, pin_memory=True,
                      sampler=DistributedSampler(ds, shuffle=False))


def init_tables(cal_per_act):
    """The seven accumulators of eval.py:344-376."""
    if cal_per_act:
        three = lambda: {m: copy.deepcopy(act) for m, _ in METRICS_3D}
        return [copy.deepcopy(act), copy.deepcopy(act), three(), three(), three(), three(), 0.0]
    flat = lambda: {'mpjpe': 0.0, 'n-mpjpe': 0.0, 'p-mpjpe': 0.0, 'pck': 0.0, 'auc': 0.0}
    return [0.0, 0.0, flat(), flat(), flat(), flat(), 0.0]


CLI = (  # same flags as the reference entry (eval.py:326-334) + --synthetic
    ('--config', dict(required=True, help='path to config')),
    ('--log_dir', dict(default='log', help='path to log into')),
    ('--checkpoint', dict(default=None, help='path to checkpoint to restore')),
    ('--batch_size', dict(default=None, type=int)),
    ('--worker', dict(default=10, type=int)),
    ('--extra_tag', dict(default=' ')),
    ('--multi_hypo', dict(default='best', choices=['best', 'confident'],
                          help='multi-hypothesis eval mode (ignored with --resolve views)')),
    ('--synthetic', dict(default=0, type=int, help='evaluate N synthetic batches (no dataset on this machine)')),
    ('--ema', dict(default=False, action='store_true', help="evaluate the averaged weights ('unsup_model_ema')")),
    ('--flip', dict(default=False, action='store_true',
                    help='flip test: average every heat-map with the one of the mirrored image (model_params.flip_pairs)')),
    ('--tri', dict(default='dlt', choices=['dlt', 'robust'],
                   help='triangulation: the DLT over all cameras, or over the largest set of cameras that agree within --tri_thresh')),
    ('--tri_thresh', dict(default=ops_eval.TRI_ROBUST_PX, type=float, metavar='PX',
                          help='--tri robust: inlier threshold in pixels of the full-resolution image')),
    ('--resolve', dict(default='gt', choices=['gt', 'views'],
                       help='left/right exchange and depth hypothesis of every view: by the labels as the reference does, or by '
                            'the agreement of the cameras (labels only name each pair; --multi_hypo is ignored)')),
    ('--tri-weight', dict(default='depth', choices=['depth', 'spread'], dest='tri_weight',
                          help="weight of every view in the triangulation and in --resolve views: the joint's depth in mm as "
                               'the reference has it, or 1 / sigma of its heat-map in image pixels')),
    ('--tri-refine', dict(default='none', choices=['none', 'lm'], dest='tri_refine',
                          help='after the triangulation: nothing, or Levenberg-Marquardt on the reprojection error in pixels '
                               'over the cameras the triangulation used (scaled by the weights with --tri-weight spread)')),
    ('--tri-huber', dict(default=0.0, type=float, metavar='PX', dest='tri_huber',
                         help="--tri-refine lm: Huber's delta in the unit of the residual (pixels; sigmas with --tri-weight "
                              'spread); 0 = plain least squares')),
    ('--tri-skeleton', dict(default=False, action='store_true', dest='tri_skeleton',
                            help='after the triangulation, in place of --tri-refine: the same Levenberg-Marquardt over all joints '
                                 'of a sample together, with left/right limb symmetry (--tri-huber applies; weight: --tri-sym)')),
    ('--tri-sym', dict(default=ops_eval.TRI_SYM_W, type=float, metavar='W', dest='tri_sym',
                       help='--tri-skeleton: weight of the squared length difference of a left/right limb pair, in px^2 '
                            'per mm^2 (sigma^2 per mm^2 with --tri-weight spread)')),
)
CLI_VOLUME = (  # --tri-volume and its grid, parsed after CLI (a table per option: each names what one option adds, a test per
    # option pins its table, and --help lists the tables in this order)
    ('--tri-volume', dict(default=False, action='store_true', dest='tri_volume',
                          help="after everything above: fuse the cameras' heat-map cubes over a voxel grid round the triangulated "
                               'point and take the soft-argmax of the fused volume in world space (not with --flip)')),
    ('--tri-vol-side', dict(default=ops_eval.TRI_VOL_SIDE_MM, type=float, metavar='MM', dest='tri_vol_side',
                            help='--tri-volume: side of the first grid in mm (untuned default)')),
    ('--tri-vol-grid', dict(default=ops_eval.TRI_VOL_G, type=int, metavar='G', dest='tri_vol_grid',
                            help='--tri-volume: voxels per side of every grid, 2..32 (untuned default)')),
    ('--tri-vol-levels', dict(default=ops_eval.TRI_VOL_LEVELS, type=int, metavar='N', dest='tri_vol_levels',
                              help='--tri-volume: grids, each half the side of the one before round its result, 1..4')),
)


CLI_FIT = (  # --fit-smpl and its settings, parsed after CLI_VOLUME (a table per option, as above)
    ('--fit-smpl', dict(default=None, metavar='OUT.npz', dest='fit_smpl',
                        help='after everything above: fit SMPL parameters to the final world joints of every sample and write '
                             'them as a bank that train.py --pseudo-online reads (needs --smpl-model)')),
    ('--smpl-model', dict(default=None, metavar='ROOT', dest='smpl_model',
                          help='--fit-smpl: directory of the SMPL model files, or an .npz of exported arrays with `h36m_regressor`')),
    ('--fit-iters', dict(default=30, type=int, metavar='N', dest='fit_iters', help='--fit-smpl: Levenberg-Marquardt trials per sample')),
    ('--fit-pose-prior', dict(default=None, type=float, metavar='W', dest='fit_pose_prior',
                              help='--fit-smpl: weight of the squared body-pose angles against mm^2 (untuned default)')),
    ('--fit-shape-prior', dict(default=None, type=float, metavar='W', dest='fit_shape_prior',
                               help='--fit-smpl: weight of the squared betas against mm^2 (untuned default)')),
)


def mirror_options(config, opt, always=(), given=()):
    """Parsed flags as model_params keys, which is where Eval reads its options: the keys of `always` as they are, those of
    `given` only where the flag was given (not None), so that their defaults stay where the option's module has them."""
    mp = config['model_params']
    for key in always:
        mp[key] = getattr(opt, key)
    for key in given:
        if getattr(opt, key) is not None:
            mp[key] = getattr(opt, key)


def mirror_tri_options(config, opt):
    """The --tri-* flags of CLI and CLI_VOLUME as model_params keys; --tri-skeleton is the third choice of tri_refine."""
    mirror_options(config, opt, always=('tri_weight', 'tri_refine', 'tri_huber', 'tri_sym', 'tri_volume', 'tri_vol_side', 'tri_vol_grid',
                                        'tri_vol_levels'))
    if opt.tri_skeleton:
        config['model_params']['tri_refine'] = 'skeleton'


def mirror_fit_options(config, opt):
    """The --fit-smpl flags as model_params keys (only the ones given: the defaults live in xas_amd.ops_smplfit)."""
    mirror_options(config, opt, always=('fit_smpl', 'smpl_model', 'fit_iters'), given=('fit_pose_prior', 'fit_shape_prior'))


CLI_FIT_SHAPE = (  # --fit-shape and its gap, parsed after CLI_SMOOTH_BONES (a table per option, as above)
    ('--fit-shape', dict(default=None, choices=('frame', 'track'), dest='fit_shape',
                         help='--fit-smpl: frame = betas per sample (the default); track = after the loop, one beta vector per '
                              'track with pose and translation per frame, warm-started from the per-sample fits (needs one rank)')),
    ('--fit-gap', dict(default=None, type=int, metavar='FRAMES', dest='fit_gap',
                       help='--fit-shape track: consecutive frames of a sequence further apart start a new track')),
)


def mirror_fit_shape_options(config, opt):
    """--fit-shape and --fit-gap as model_params keys (only if given: the gap's default is xas_amd.ops_track's)."""
    if opt.fit_shape == 'track' and not opt.fit_smpl:
        raise ValueError('--fit-shape track is a mode of --fit-smpl: it needs --fit-smpl')
    mirror_options(config, opt, given=('fit_shape', 'fit_gap'))


CLI_FIT_DATA = (  # --fit-data, parsed after CLI_FIT_SMOOTH (a table per option, as above)
    ('--fit-data', dict(default=None, choices=('joints', 'reproj'), dest='fit_data',
                        help='--fit-smpl: joints = fit the final world joints in mm (the default); reproj = then, from that fit, fit '
                             'the detections of every camera in pixels, with 3-D anchors where there is one (one camera: the '
                             'selected point along its ray; --tri-volume: the fused point with its covariance)')),
)


def mirror_fit_data_options(config, opt):
    """--fit-data as a model_params key (only if given)."""
    if opt.fit_data == 'reproj':
        if not opt.fit_smpl:
            raise ValueError('--fit-data reproj is a mode of --fit-smpl: it needs --fit-smpl')
        if opt.fit_shape == 'track':
            raise ValueError('--fit-data reproj does not go with --fit-shape track: the track fits have no pixel term yet')
        if opt.flip:
            raise ValueError('--fit-data reproj does not go with --flip')
    mirror_options(config, opt, given=('fit_data',))


CLI_FIT_SMOOTH = (  # --fit-smooth and its translation weight, parsed after CLI_FIT_SHAPE (a table per option, as above)
    ('--fit-smooth', dict(default=None, nargs='?', const=True, type=float, metavar='W_ROT', dest='fit_smooth',
                          help='--fit-shape track: an acceleration prior on pose and translation over the frames of a track; W_ROT '
                               'weighs the 72 angles (mm^2 per rad^2; default xas_amd.ops_smplfit.FIT_SMOOTH_ROT)')),
    ('--fit-smooth-trans', dict(default=None, type=float, metavar='W', dest='fit_smooth_trans',
                                help='--fit-smooth: the weight of the translation (default xas_amd.ops_smplfit.FIT_SMOOTH_TRANS)')),
)


def mirror_fit_smooth_options(config, opt):
    """--fit-smooth and --fit-smooth-trans as model_params keys (only if given; the bare flag takes the default weight)."""
    if (opt.fit_smooth is not None or opt.fit_smooth_trans is not None) and opt.fit_shape != 'track':
        raise ValueError('--fit-smooth is a mode of --fit-shape track: it needs --fit-shape track')
    if opt.fit_smooth is True:
        from xas_amd import ops_smplfit              # only with the flag
        opt.fit_smooth = ops_smplfit.FIT_SMOOTH_ROT
    mirror_options(config, opt, given=('fit_smooth', 'fit_smooth_trans'))


def joint_accel_mm(joints, track, frame, fitted):
    """--fit-smooth: per sample the norm of the acceleration stencil's second difference of joints [N,18,3] over the fitted
    frames of its track in frame order, mean over the 18 joints; NaN at a track's ends and at frames passed through."""
    out = np.full(len(track), np.nan)
    for s in np.unique(track):
        rows = np.nonzero((track == s) & fitted)[0]
        rows = rows[np.argsort(frame[rows], kind='stable')]
        f = frame[rows].astype(np.float64)
        for k in range(1, len(rows) - 1):
            h0, h1 = f[k] - f[k - 1], f[k + 1] - f[k]
            q = joints[rows[k - 1]] / h0 - joints[rows[k]] * (1.0 / h0 + 1.0 / h1) + joints[rows[k + 1]] / h1
            out[rows[k]] = np.linalg.norm(q, axis=-1).mean()
    return out


CLI_CALIB = (  # --calibrate / --calibration and their settings, parsed after CLI_FIT (a table per option, as above)
    ('--calibrate', dict(default=None, metavar='OUT.npz', dest='calibrate',
                         help='after everything above: bundle adjustment of the camera extrinsics over the whole set, per rig, '
                              'written as corrections that --calibration applies (needs 2+ cameras and one rank)')),
    ('--calibration', dict(default=None, metavar='IN.npz', dest='calibration',
                           help='correct every batch\'s cameras by a --calibrate file before triangulation (not with --calibrate)')),
    ('--calib-iters', dict(default=30, type=int, metavar='N', dest='calib_iters', help='--calibrate: Levenberg-Marquardt trials per rig')),
    ('--calib-prior-rot', dict(default=None, type=float, metavar='W', dest='calib_prior_rot',
                               help='--calibrate: weight of the squared rotation corrections, cost per rad^2 (untuned default)')),
    ('--calib-prior-trans', dict(default=None, type=float, metavar='W', dest='calib_prior_trans',
                                 help='--calibrate: weight of the squared translation corrections, cost per mm^2 (untuned default)')),
    ('--calib-free', dict(default=None, type=int, metavar='MASK', dest='calib_free',
                          help='--calibrate: bit v set = camera v may move (default: every camera but the first)')),
)


def mirror_calib_options(config, opt):
    """The --calibrate / --calibration flags as model_params keys (only the ones given: the defaults live in xas_amd.ops_calib)."""
    if opt.calibrate and opt.calibration:
        raise ValueError('--calibrate and --calibration do not go together')
    mirror_options(config, opt, always=('calibrate', 'calibration', 'calib_iters'), given=('calib_prior_rot', 'calib_prior_trans', 'calib_free'))


CLI_SMOOTH = (  # --smooth and its settings, parsed after CLI_CALIB (a table per option, as above)
    ('--smooth', dict(default=None, metavar='OUT.npz', dest='smooth',
                      help='after everything above: smooth every joint\'s triangulated track over the frames of its sequence '
                           '(reprojection cost + acceleration penalty) and fill frames without data (needs 2+ cameras and one rank)')),
    ('--smooth-acc', dict(default=None, type=float, metavar='W', dest='smooth_acc',
                          help='--smooth: weight of the squared acceleration, px^2 per (mm^2 / frame^3) (untuned default)')),
    ('--smooth-gap', dict(default=None, type=int, metavar='FRAMES', dest='smooth_gap',
                          help='--smooth: frames of a sequence further apart than this start a new track (untuned default)')),
    ('--smooth-iters', dict(default=30, type=int, metavar='N', dest='smooth_iters', help='--smooth: Levenberg-Marquardt trials per track')),
)


def mirror_smooth_options(config, opt):
    """The --smooth flags as model_params keys (only the ones given: the defaults live in xas_amd.ops_track)."""
    mirror_options(config, opt, always=('smooth', 'smooth_iters'), given=('smooth_acc', 'smooth_gap'))


CLI_RESOLVE_TRACK = (  # --resolve-track and its settings, parsed after CLI_SMOOTH (a table per option, as above)
    ('--resolve-track', dict(default=None, metavar='OUT.npz', dest='resolve_track',
                             help='after everything above, per camera and without labels: choose every joint\'s depth hypothesis '
                                  'and every limb pair\'s left/right exchange over the frames of its sequence (motion cost + priors, '
                                  'exact by dynamic programming; works with one camera; needs one rank)')),
    ('--rt-vel', dict(default=None, type=float, metavar='W', dest='rt_vel',
                      help='--resolve-track: weight of the squared jump between frames, cost per (mm^2 / frame) (untuned default)')),
    ('--rt-hyp', dict(default=None, type=float, metavar='W', dest='rt_hyp',
                      help='--resolve-track: cost of one rank step away from hypothesis 0 (untuned default)')),
    ('--rt-swap', dict(default=None, type=float, metavar='W', dest='rt_swap',
                       help='--resolve-track: cost of an exchanged pair in a frame (untuned default)')),
    ('--rt-gap', dict(default=None, type=int, metavar='FRAMES', dest='rt_gap',
                      help='--resolve-track: frames of a sequence further apart than this start a new track (untuned default)')),
)


def mirror_resolve_track_options(config, opt):
    """The --resolve-track flags as model_params keys (only the ones given: the defaults live in xas_amd.ops_track)."""
    mirror_options(config, opt, given=('resolve_track', 'rt_vel', 'rt_hyp', 'rt_swap', 'rt_gap'))


CLI_SMOOTH_ANCHOR = (  # --smooth-data and its settings, parsed after CLI_RESOLVE_TRACK (a table per option, as above)
    ('--smooth-data', dict(default=None, choices=('reproj', 'anchor'), dest='smooth_data',
                           help='--smooth: what holds the tracks.  reproj (the default): the pixels of 2+ cameras.  anchor: a 3-D '
                                'point per frame and joint with an information matrix.  With one camera its pixels plus its '
                                'selected world point (--resolve-track\'s choice if that is given too), known --smooth-depth '
                                'along the ray.  With 2+ cameras it needs --tri-volume and smooths the fused points with the '
                                'inverse of their covariance alone, no pixels: the cost is then in sigma^2, so --smooth-acc is '
                                'in sigma^2 per (mm^2 / frame^3) and weighs against mm-scale covariances, not pixels')),
    ('--smooth-depth', dict(default=None, type=float, metavar='W', dest='smooth_depth',
                            help='--smooth-data anchor, one camera: information along the ray, px^2 per mm^2 (untuned default)')),
    ('--smooth-anchor-huber', dict(default=None, type=float, metavar='D', dest='smooth_anchor_huber',
                                   help='--smooth-data anchor: Huber delta of the anchor term, in sqrt(e^T W e); 0 = squared '
                                        '(untuned default)')),
)


def mirror_smooth_anchor_options(config, opt):
    """The --smooth-data flags as model_params keys (only the ones given: the defaults live in Eval and xas_amd.ops_track)."""
    mirror_options(config, opt, given=('smooth_data', 'smooth_depth', 'smooth_anchor_huber'))


CLI_SMOOTH_BONES = (  # --smooth-bones, parsed after CLI_SMOOTH_ANCHOR (a table per option, as above)
    ('--smooth-bones', dict(default=None, nargs='?', const=True, type=float, metavar='W', dest='smooth_bones',
                            help='--smooth (with either --smooth-data): smooth all joints of a track at once, coupled in every '
                                 'frame by the lengths of the bones of model_params.parent_ids (the per-track medians of the start); '
                                 'W = weight of a squared length error, px^2 per mm^2 (untuned default)')),
)


def mirror_smooth_bones_options(config, opt):
    """--smooth-bones as a model_params key (only if given: True stands for the default weight of xas_amd.ops_track)."""
    if opt.smooth_bones is not None and not opt.smooth:
        raise ValueError('--smooth-bones couples the joints of --smooth: it needs --smooth')
    mirror_options(config, opt, given=('smooth_bones',))


def main():
    parser = ArgumentParser()
    for flag, kw in CLI + CLI_VOLUME + CLI_FIT + CLI_CALIB + CLI_SMOOTH + CLI_RESOLVE_TRACK + CLI_SMOOTH_ANCHOR + CLI_SMOOTH_BONES + CLI_FIT_SHAPE + CLI_FIT_SMOOTH + CLI_FIT_DATA:
        parser.add_argument(flag, **kw)
    opt = parser.parse_args()
    with open(opt.config) as f:
        config = yaml.load(f, Loader=yaml.FullLoader)
    config['model_params']['cam_id_list'] = config['dataset_params']['cam_id_list']
    mirror_tri_options(config, opt)
    mirror_fit_options(config, opt)
    mirror_calib_options(config, opt)
    mirror_smooth_options(config, opt)
    mirror_resolve_track_options(config, opt)
    mirror_smooth_anchor_options(config, opt)
    mirror_smooth_bones_options(config, opt)
    mirror_fit_shape_options(config, opt)
    mirror_fit_smooth_options(config, opt)
    mirror_fit_data_options(config, opt)
    if opt.batch_size:
        config['train_params']['batch_size'] = opt.batch_size
    if opt.checkpoint is None and not opt.synthetic:
        raise Exception('Must specify checkpoint path')
    ddp_setup()
    rank_local, world = int(os.environ['LOCAL_RANK']), int(os.environ['WORLD_SIZE'])
    log_dir = os.path.dirname(opt.checkpoint) if opt.checkpoint else opt.log_dir
    detector = prepare_model(config, opt)
    loader = prepare_data(config, world, opt.worker, opt.synthetic, torch.device('cuda', rank_local))
    ev = Eval(config, detector, loader, log_dir, flip_test=opt.flip, tri=opt.tri, tri_thresh=opt.tri_thresh,
              resolve=opt.resolve)
    tables = init_tables(ev.cal_per_act)
    record = ev.eval(None, *tables, mode=opt.multi_hypo)
    destroy_process_group()
    if rank_local == 0:
        ev.record(*record)


if __name__ == '__main__':
    main()
