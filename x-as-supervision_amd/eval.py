#!/usr/bin/env python3
"""torchrun entry of the MI355X-native evaluation (reference: eval.py:1-408, same CLI and result file).

    torchrun --nproc-per-node=N eval.py --config config/HM36_Multi_SurS1.yaml --checkpoint ckpt.pth.tar
             [--batch_size B --worker W --multi_hypo best|confident] [--synthetic STEPS] [--ema] [--flip]
             [--tri dlt|robust --tri_thresh PX] [--resolve gt|views] [--tri-weight depth|spread]
             [--tri-refine none|lm --tri-huber PX] [--tri-skeleton --tri-sym W]
             [--tri-volume --tri-vol-side MM --tri-vol-grid G --tri-vol-levels N]
             [--fit-smpl OUT.npz --smpl-model ROOT|.npz --fit-iters N --fit-pose-prior W --fit-shape-prior W]

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
"""
import copy
import os
from argparse import ArgumentParser

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


class Eval:
    """Same constructor and method signatures as the reference Eval (eval.py:63-107)."""

    def __init__(self, config, detector, eval_data, log_dir, img_size=256.0, flip_test=False, tri='dlt',
                 tri_thresh=ops_eval.TRI_ROBUST_PX, resolve='gt'):
        if tri not in ('dlt', 'robust'):
            raise ValueError('Unknown triangulation: {}'.format(tri))
        if resolve not in ('gt', 'views'):
            raise ValueError('Unknown resolve mode: {}'.format(resolve))
        tri_weight = config['model_params'].get('tri_weight', 'depth')         # --tri-weight; not a key of the shipped configs
        if tri_weight not in ('depth', 'spread'):
            raise ValueError('Unknown triangulation weight: {}'.format(tri_weight))
        tri_refine = config['model_params'].get('tri_refine', 'none')          # --tri-refine / --tri-huber; not keys of the shipped configs either
        if tri_refine not in ('none', 'lm', 'skeleton'):
            raise ValueError('Unknown triangulation refinement: {}'.format(tri_refine))
        if tri_refine == 'lm' and len(config['model_params']['cam_id_list']) > ops_eval.TRI_MAX_VIEWS:
            raise ValueError("tri_refine='lm' refines over at most {} cameras; cam_id_list has {}".format(
                ops_eval.TRI_MAX_VIEWS, len(config['model_params']['cam_id_list'])))
        if tri_refine == 'skeleton':
            if len(config['model_params']['cam_id_list']) > ops_eval.TRI_MAX_VIEWS:
                raise ValueError("tri_refine='skeleton' refines over at most {} cameras; cam_id_list has {}".format(
                    ops_eval.TRI_MAX_VIEWS, len(config['model_params']['cam_id_list'])))
            num_kp = getattr(detector, 'num_kp', config['model_params'].get('detector_params', {}).get('num_kp'))
            if num_kp is not None and num_kp > ops_eval.SKEL_MAX_JOINTS:
                raise ValueError("tri_refine='skeleton' couples at most {} joints; the detector has {}".format(
                    ops_eval.SKEL_MAX_JOINTS, num_kp))
        tri_volume = bool(config['model_params'].get('tri_volume', False))     # --tri-volume; not a key of the shipped configs either
        if tri_volume and flip_test:
            raise ValueError('tri_volume fuses the heat-map cubes of the cameras; the flip test\'s head works on an average of two '
                             'cubes that is never formed in memory: --tri-volume does not go with --flip')
        if tri_volume and len(config['model_params']['cam_id_list']) > ops_eval.TRI_MAX_VIEWS:
            raise ValueError('tri_volume fuses at most {} cameras; cam_id_list has {}'.format(
                ops_eval.TRI_MAX_VIEWS, len(config['model_params']['cam_id_list'])))
        self.gpu_id = int(os.environ.get('LOCAL_RANK', 0))
        self.config = config
        self.cam_id_list = config['model_params']['cam_id_list']
        self.cal_per_act = config['dataset_params']['dataset']['name'] != 'mpi_inf_3dhp'
        self.detector = detector.to(self.gpu_id)
        self.detector.eval()                       # BN uses running statistics; no DDP wrapper is needed to evaluate
        self.eval_data = eval_data
        self.log_dir = log_dir
        self.img_size = img_size
        self.flip_test = bool(flip_test)           # --flip: every image is evaluated together with its horizontal mirror
        self.tri, self.tri_thresh = tri, float(tri_thresh)   # --tri robust: DLT over the views that agree within tri_thresh px
        self.tri_views, self.tri_batches = 0.0, 0  # robust only: mean views used per joint, summed over the batches
        self.resolve = resolve                     # --resolve views: exchange and hypothesis by the cameras' agreement
        if resolve == 'views' and not 2 <= len(self.cam_id_list) <= ops_eval.TRI_MAX_VIEWS:
            raise ValueError("resolve='views' decides by the agreement of the cameras and needs 2 to {} of them; cam_id_list "
                             'has {}'.format(ops_eval.TRI_MAX_VIEWS, len(self.cam_id_list)))
        self.res_exchanged, self.res_hyp0, self.res_batches = 0.0, 0.0, 0      # views only, summed over the batches
        self.tri_weight = tri_weight               # --tri-weight spread: a view counts by its heat-map's 1 / sigma, not its depth
        self.spread = None                         # spread only: heat-map spread [B,K,5] of the latest detect()
        self.tri_sigma, self.sigma_batches = 0.0, 0    # spread only: mean sigma in pixels, summed over the batches
        self.tri_refine = tri_refine               # --tri-refine lm: the triangulated point minimises the reprojection error in pixels
        self.tri_huber = float(config['model_params'].get('tri_huber', 0.0))   # lm only: Huber's delta, 0 = plain least squares
        self.refine_px, self.refine_gain, self.refine_batches = 0.0, 0.0, 0    # lm and skeleton, summed over the batches
        self.tri_sym = float(config['model_params'].get('tri_sym', ops_eval.TRI_SYM_W))    # skeleton only: --tri-sym, px^2 per mm^2
        self.sym_mm = np.zeros(2)                  # skeleton only: mean |limb a| - |limb b| in mm before and after, summed
        self.tri_volume = tri_volume               # --tri-volume: the cameras' heat-map cubes fused round the triangulated point
        mp = config['model_params']
        self.vol_side = float(mp.get('tri_vol_side', ops_eval.TRI_VOL_SIDE_MM))
        self.vol_grid, self.vol_levels = int(mp.get('tri_vol_grid', ops_eval.TRI_VOL_G)), int(mp.get('tri_vol_levels', ops_eval.TRI_VOL_LEVELS))
        self.logits = None                         # volume only: the logits [B,K*D,D,D] of the latest detect()
        self.vol_move, self.vol_sigma, self.vol_status, self.vol_batches = 0.0, 0.0, np.zeros(4), 0   # volume only, summed
        self.fit_smpl = mp.get('fit_smpl') or None     # --fit-smpl OUT.npz: SMPL parameters of the final world joints, a --pseudo-online bank
        if self.fit_smpl:
            smpl = prepare_smpl(mp)                  # (Eval's signature is pinned: the model comes through model_params.smpl_model)
            if smpl[0] is None or smpl[1] is None:
                raise ValueError('fit_smpl needs an SMPL layer and the H36M joint regressor (eval.py --smpl-model)')
            from xas_amd import ops_smplfit          # only with the flag
            self.smpl_layer, self.h36m_regressor = smpl[0].to(self.gpu_id), smpl[1].to(self.gpu_id)
            self.fit_iters = int(mp.get('fit_iters', 30))
            self.fit_pose_prior = float(mp.get('fit_pose_prior', ops_smplfit.POSE_PRIOR))      # untuned guesses, both
            self.fit_shape_prior = float(mp.get('fit_shape_prior', ops_smplfit.SHAPE_PRIOR))
            self.fit_rows = []                         # per batch: the host arrays of the file
        self.calibrate = mp.get('calibrate') or None   # --calibrate OUT.npz: bundle adjustment of the extrinsics over the whole set
        self.calibration = mp.get('calibration') or None   # --calibration IN.npz: every batch's cameras corrected by such a file
        if self.calibrate and self.calibration:
            raise ValueError('calibrate estimates corrections of the given cameras and calibration applies earlier ones: '
                             '--calibrate and --calibration do not go together')
        if self.calibrate:
            if not 2 <= len(self.cam_id_list) <= ops_eval.TRI_MAX_VIEWS:
                raise ValueError('calibrate needs 2 to {} cameras; cam_id_list has {}'.format(ops_eval.TRI_MAX_VIEWS, len(self.cam_id_list)))
            if int(os.environ.get('WORLD_SIZE', 1)) != 1:
                raise ValueError('calibrate needs WORLD_SIZE == 1: a rank sees only its shard of the set, and a bundle over '
                                 'several ranks is not built')
            from xas_amd import ops_calib              # only with the flag
            self.calib_iters = int(mp.get('calib_iters', 30))
            self.calib_prior_rot = float(mp.get('calib_prior_rot', ops_calib.CALIB_PRIOR_ROT))        # untuned guesses, both
            self.calib_prior_trans = float(mp.get('calib_prior_trans', ops_calib.CALIB_PRIOR_TRANS))
            self.calib_free = mp.get('calib_free')     # mask of the cameras that may move; None = all but camera 0
            self.calib_rows = []                       # per batch, on the device: points, pmat, init, views
        self.smooth = mp.get('smooth') or None         # --smooth OUT.npz: the joint tracks smoothed over time, over the whole set
        if self.smooth:
            if not 2 <= len(self.cam_id_list) <= ops_eval.TRI_MAX_VIEWS:
                raise ValueError('smooth needs 2 to {} cameras; cam_id_list has {}'.format(ops_eval.TRI_MAX_VIEWS, len(self.cam_id_list)))
            if int(os.environ.get('WORLD_SIZE', 1)) != 1:
                raise ValueError('smooth needs WORLD_SIZE == 1: a DistributedSampler deals the frames of a sequence out over '
                                 'the ranks, and no rank sees a track')
            from xas_amd import ops_track              # only with the flag
            self.smooth_acc = float(mp.get('smooth_acc', ops_track.TRACK_ACC_W))                     # untuned guesses, both
            self.smooth_gap = int(mp.get('smooth_gap', ops_track.TRACK_MAX_GAP))
            self.smooth_iters = int(mp.get('smooth_iters', 30))
            self.smooth_rows = []                      # per batch, on the device: points, pmat, init, views, gt; and the paths
        self.resolve_track = mp.get('resolve_track') or None   # --resolve-track OUT.npz: hypothesis and exchange chosen over time, per camera
        if self.resolve_track:
            if int(os.environ.get('WORLD_SIZE', 1)) != 1:
                raise ValueError('resolve_track needs WORLD_SIZE == 1: a DistributedSampler deals the frames of a sequence out '
                                 'over the ranks, and no rank sees a track')
            from xas_amd import ops_track              # only with the flag
            self.rt_vel = float(mp.get('rt_vel', ops_track.TRACK_VEL_W))                             # untuned guesses, all four
            self.rt_hyp = float(mp.get('rt_hyp', ops_track.TRACK_HYP_W))
            self.rt_swap = float(mp.get('rt_swap', ops_track.TRACK_SWAP_W))
            self.rt_gap = int(mp.get('rt_gap', ops_track.TRACK_MAX_GAP))
            self.rt_rows = []                          # per batch, on the device: per camera kps, world, labels, view; gt; and the paths
        if self.calibration:
            with np.load(self.calibration) as f:
                self.calib_keys = torch.from_numpy(f['keys']).to(self.gpu_id)
                self.calib_delta = torch.from_numpy(f['delta']).to(self.gpu_id)

    def write_calibration(self):
        """--calibrate: one bundle adjustment over everything the batches kept, the file (atomically: a temporary file beside
        it, then a rename) and -> the lines of eval_result.txt, one per rig."""
        from xas_amd import ops_calib
        cat = lambda k: torch.cat([r[k] for r in self.calib_rows])
        points, pmat, init = cat('points'), cat('pmat'), cat('init')
        views = cat('views') if self.calib_rows[0]['views'] is not None else None
        rig, keys = ops_calib.rigs_of(pmat)
        r = ops_calib.calibrate_bundle(points, pmat, init, rig, views=views, free=self.calib_free,
                                       weighted=self.tri_weight == 'spread', huber_px=self.tri_huber,
                                       prior_rot=self.calib_prior_rot, prior_trans=self.calib_prior_trans,
                                       max_iter=self.calib_iters, num_rigs=keys.shape[0])
        cols = {k: r[k].cpu().numpy() for k in ('delta', 'cost', 'rms', 'status', 'cam_cov')}
        made = r['trials'].cpu().numpy()
        cols['keys'] = keys.cpu().numpy()
        os.makedirs(os.path.dirname(os.path.abspath(self.calibrate)), exist_ok=True)
        tmp = self.calibrate + '.tmp.npz'
        np.savez(tmp, **cols)
        os.replace(tmp, self.calibrate)
        d = cols['delta']
        return ['CALIBRATE rig {} ({} of {} trials, prior rot {}, prior trans {}): reprojection RMS {} -> {} px, largest |omega| {} deg, '
                'largest |tau| {} mm, {}'.format(i, int(made[i, 0]), self.calib_iters, self.calib_prior_rot, self.calib_prior_trans,
                                                 cols['rms'][i, 0], cols['rms'][i, 1],
                                                 float(np.degrees(np.linalg.norm(d[i, :, :3], axis=-1).max())),
                                                 float(np.linalg.norm(d[i, :, 3:], axis=-1).max()),
                                                 ops_calib.STATUS_NAMES[int(cols['status'][i])]) for i in range(len(d))]

    def write_smooth(self):
        """--smooth: one track_smooth over everything the batches kept, the file (atomically: a temporary file beside it, then
        a rename) and -> the two lines of eval_result.txt."""
        from xas_amd import ops_track
        rows = self.smooth_rows
        cat = lambda k: torch.cat([r[k] for r in rows])
        points, pmat, init, gt = cat('points'), cat('pmat'), cat('init'), cat('gt')
        views = cat('views') if rows[0]['views'] is not None else None
        paths = [p for r in rows for p in r['paths']] if rows[0]['paths'] is not None else None
        track, frame = ops_track.tracks_of(paths, self.smooth_gap, count=len(points))
        r = ops_track.track_smooth(points, pmat, init, track, frame, views=views, weighted=self.tri_weight == 'spread',
                                   huber_px=self.tri_huber, acc_w=self.smooth_acc, max_iter=self.smooth_iters)
        joints, status = r['xyzw'][..., :3].contiguous(), r['status']
        both = torch.isfinite(joints).all(-1) & torch.isfinite(init[..., :3]).all(-1)                  # [N,K]
        err = lambda p: pose_errors(torch.where(torch.isfinite(p), p, torch.zeros_like(p)), gt, want=('err',))['err'][0]   # [N,K] mm, no alignment
        e_before, e_after = err(init[..., :3].contiguous()), err(joints)
        mean = lambda e, m: float(e[m].mean()) if bool(m.any()) else float('nan')
        filled = (status == ops_track.STATUS_FILLED) & torch.isfinite(joints).all(-1)
        rms = lambda c: float(torch.sqrt((r['resid'][..., c] ** 2).nanmean()))
        cols = {'joints': joints, 'status': status, 'track_status': r['track_status'], 'cost': r['cost'], 'trials': r['trials']}
        cols = {k: v.cpu().numpy() for k, v in cols.items()}
        cols['track'], cols['frame'] = track, frame
        os.makedirs(os.path.dirname(os.path.abspath(self.smooth)), exist_ok=True)
        tmp = self.smooth + '.tmp.npz'
        np.savez(tmp, **cols)
        os.replace(tmp, self.smooth)
        S = len(r['tracks'])
        return ['SMOOTH {} tracks of mean length {} (acc {}, gap {}, {} trials): TRI MPJPE {} -> {} mm, reprojection RMS {} -> {} px, '
                'gaps filled {} , passed through {}'.format(S, len(points) / S, self.smooth_acc, self.smooth_gap, self.smooth_iters,
                                                            mean(e_before, both), mean(e_after, both), rms(0), rms(1),
                                                            float((status == ops_track.STATUS_FILLED).float().mean()),
                                                            float((status == ops_track.STATUS_PASSED).float().mean())),
                'SMOOTH filled gap joints: MPJPE {} mm over {} joints'.format(mean(e_after, filled), int(filled.sum()))]

    def write_resolve_track(self):
        """--resolve-track: one track_resolve per camera over everything the batches kept, the file (atomically: a temporary
        file beside it, then a rename) and -> the lines of eval_result.txt, one per camera."""
        from xas_amd import ops_track
        rows = self.rt_rows
        gt = torch.cat([r['gt'] for r in rows])
        err = lambda p: pose_errors(torch.where(torch.isfinite(p), p, torch.zeros_like(p)), gt, want=('err',))['err'][0]   # [N,K] mm, no alignment
        mean = lambda e, m: float(e[m].mean()) if bool(m.any()) else float('nan')
        cols, lines = {}, []
        for c in self.cam_id_list:
            m = 'cam_{}'.format(c)
            cat = lambda k: torch.cat([r[m][k] for r in rows])
            kps, world, view = cat('kps'), cat('world'), cat('view')
            paths = [p for r in rows for p in r[m]['paths']] if rows[0][m]['paths'] is not None else None
            track, frame = ops_track.tracks_of(paths, self.rt_gap, count=len(kps))
            r = ops_track.track_resolve(kps, world, track, frame, vel_w=self.rt_vel, hyp_w=self.rt_hyp, swap_w=self.rt_swap,
                                        gt=cat('labels'), image_size=self.img_size)
            perm = ops_eval.switch_perm(kps.shape[2], ops_eval.SWITCH_PAIRS, kps.device)
            joints = ops_track.resolved_gather(world, r['hyp'], r['swap'], perm)[..., :3].contiguous()
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
                             m, S, len(kps) / S, self.rt_vel, self.rt_hyp, self.rt_swap, self.rt_gap, mean(err(first), ok),
                             mean(err(joints), ok), rows[0]['mode'], mean(err(view), ok), float(r['swap'][:, paired].float().mean()),
                             float((r['hyp'] == 0).float().mean()), float((r['status'] == ops_track.RESOLVE_PASSED).float().mean())))
        os.makedirs(os.path.dirname(os.path.abspath(self.resolve_track)), exist_ok=True)
        tmp = self.resolve_track + '.tmp.npz'
        np.savez(tmp, **cols)
        os.replace(tmp, self.resolve_track)
        return lines

    def fit_batch(self, joints, bad, cov):
        """--fit-smpl on the final world joints [B,18,3] of a batch.  A joint's weight is 0 where it is not finite or `bad`
        [B,18] marks it (a triangulation that passed it through), else 1, or with `cov` [B,18,6] (xx xy xz yy yz zz, mm^2)
        1 / trace(cov) normalised to mean 1 over the usable joints of the sample.  -> the file's rows, on the device."""
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
        return {'fit_pose': r['pose'].float(), 'fit_betas': r['betas'].float(), 'fit_trans': r['trans'].float(),
                'fit_cost': r['cost'].float(), 'fit_status': r['status'], 'fit_joint_rms_mm': rms.float()}

    def write_fit(self):
        """Writes the --fit-smpl file (atomically: a temporary file beside it, then a rename); passed-through samples are kept
        with their status.  -> the line of eval_result.txt."""
        from xas_amd import ops_smplfit
        shapes = {'pose': (0, 72), 'betas': (0, 10), 'trans': (0, 3), 'cost': (0, 2), 'status': (0,), 'joint_rms_mm': (0,)}
        cols = {k: (np.concatenate([r[k] for r in self.fit_rows]) if self.fit_rows else np.zeros(sh, np.uint8 if k == 'status' else np.float32))
                for k, sh in shapes.items()}
        os.makedirs(os.path.dirname(os.path.abspath(self.fit_smpl)), exist_ok=True)
        tmp = self.fit_smpl + '.tmp.npz'
        np.savez(tmp, **cols)
        os.replace(tmp, self.fit_smpl)
        n = max(len(cols['status']), 1)
        fitted = cols['status'] != ops_smplfit.STATUS_PASSED
        rms = float(cols['joint_rms_mm'][fitted].mean()) if fitted.any() else float('nan')
        share = ' , '.join('{} {}'.format(name, float((cols['status'] == c).sum()) / n) for c, name in enumerate(ops_smplfit.STATUS_NAMES))
        return 'FIT smpl ({} trials, pose prior {}, shape prior {}): joint RMS {} mm; {}'.format(
            self.fit_iters, self.fit_pose_prior, self.fit_shape_prior, rms, share)

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

    @torch.no_grad()
    def eval_batch(self, x, mode='best', kps_by_cam=None):
        """Device part of one iteration of eval.py:111-204.  Returns ({name: tensor on the device}, layout) where
        every tensor is per sample [B] (errors), or a scalar (ambiguity, pck, auc).  With resolve='views' `mode` is ignored:
        the cameras' agreement picks the hypotheses."""
        cams = ['cam_{}'.format(c) for c in self.cam_id_list]
        sel, out, trans = {}, {}, None
        given = x                                  # the ground truth reads the cameras as given; --calibration corrects the predictions'
        if self.calibration:
            x = apply_calibration(x, self.cam_id_list, self.calib_keys, self.calib_delta)
        weights = {} if self.tri_weight == 'spread' else None
        cubes, chan = ({}, []) if self.tri_volume else (None, None)
        raw_kps = {} if self.resolve_track else None   # --resolve-track: every camera's detections as they came

        def detect(m):                             # one camera's joints; spread: also its weights, which need the detector
            kps = self.detect(x[m + '_img']) if kps_by_cam is None or weights is not None or cubes is not None else None
            if weights is not None:
                weights[m] = spread_weight(self.spread, x[m + '_trans_image'])
            if cubes is not None:
                cubes[m] = self.logits             # every camera's logits stay alive until the fusion
            return kps if kps_by_cam is None else kps_by_cam[m]

        if self.resolve == 'views':
            raw = {m: detect(m) for m in cams}
            if raw_kps is not None:
                raw_kps.update(raw)
            sel, r = resolve_views_weighted(raw, x, self.cam_id_list, ops_eval.SWITCH_PAIRS, weights, gt=True)   # None: the depth
            for m in cams:                         # the labels' part from here on: measuring, no longer choosing
                out['err2d_' + m] = ops_eval.eval_select(sel[m].unsqueeze(1), x[m + '_joints'], image_size=self.img_size,
                                                         mode='confident', no_switch=True, want=('err2d',))['err2d']
            shifts = torch.arange(len(cams), device=r['swap'].device, dtype=torch.int32)
            count = lambda mask: ((mask.unsqueeze(-1).int() >> shifts) & 1).sum(dim=-1).float()     # [B,K] bits set
            trans = count(r['swap']).unsqueeze(-1)
            B, K = r['swap'].shape
            perm = ops_eval.switch_perm(K, ops_eval.SWITCH_PAIRS, shifts.device)
            paired = (perm != torch.arange(K, device=shifts.device, dtype=torch.int32)).float()       # [K], both of a pair
            before = torch.where(r['named'].bool(), count(r['valid']) - count(r['swap']), count(r['swap']))   # naming undone
            out['resolve_exchanged'] = (before * paired).sum() / (paired.sum().clamp(min=1.0) * B * len(cams))
            out['resolve_hyp0'] = (r['hyp'] == 0).float().mean()
            if chan is not None:                   # view v read joint k from perm[k] where bit v of swap is set
                own = torch.arange(K, device=shifts.device, dtype=torch.int32)
                chan = [torch.where(((r['swap'].int() >> v) & 1).bool(), perm, own) for v in range(len(cams))]
        for m in ([] if self.resolve == 'views' else cams):
            kps = detect(m)
            if raw_kps is not None:
                raw_kps[m] = kps
            s = ops_eval.eval_select(kps, x[m + '_joints'], image_size=self.img_size, mode=mode)
            sel[m] = s['sel3d']
            out['err2d_' + m] = s['err2d']
            t = s['swapped'].float()
            trans = t if trans is None else trans + t
            if chan is not None:                   # the joint was taken from its partner's channel where eval_select exchanged
                K = s['swapped'].shape[1]
                perm = ops_eval.switch_perm(K, ops_eval.SWITCH_PAIRS, kps.device)
                chan.append(torch.where(s['swapped'].squeeze(-1), perm, torch.arange(K, device=kps.device, dtype=torch.int32)))
        out['ambiguity'] = torch.minimum(trans, len(cams) - trans).mean()                  # eval.py:164-167
        gt = convert_patch_to_world(given['cam_0_joints'], given, 'cam_0', is_norm=False)  # eval.py:170
        fit_bad = fit_cov = None                   # --fit-smpl only: joints a solver passed through, and a covariance if one came
        fit_want = (('status',) + (('cov',) if weights is not None and self.tri_refine == 'lm' else ())) if self.fit_smpl else ()
        if len(cams) == 1 and self.tri == 'dlt' and self.tri_refine == 'none':     # one camera: nothing to triangulate, its own point
            tri = convert_patch_to_world(sel[cams[0]], x, cams[0], is_norm=True)[..., :3]            # (the DLT refuses one view)
        elif self.tri_refine == 'lm':              # the same solver, then the pixel error minimised over the views it used
            tri, r = triangulation_refined(sel, x, self.cam_id_list, weights, huber_px=self.tri_huber, want=('resid',) + fit_want,
                                           robust_px=self.tri_thresh if self.tri == 'robust' else None)
            used = r.get('inliers')
            out['tri_refine_px'] = r['resid'][..., 1].nanmean()            # a joint passed through has no residual (NaN)
            out['tri_refine_gain_px'] = (r['resid'][..., 0] - r['resid'][..., 1]).nanmean()
            if self.fit_smpl:
                fit_bad, fit_cov = r['status'] == 2, r.get('cov')
        elif self.tri_refine == 'skeleton':        # the same start and views, the joints of a sample refined together
            tri, r = triangulation_skeleton(sel, x, self.cam_id_list, weights, huber_px=self.tri_huber, sym_w=self.tri_sym,
                                            want=('resid', 'sym') + fit_want, robust_px=self.tri_thresh if self.tri == 'robust' else None)
            used = r.get('inliers')
            out['tri_refine_px'] = r['resid'][..., 1].nanmean()            # a fixed joint has no residual (NaN)
            out['tri_refine_gain_px'] = (r['resid'][..., 0] - r['resid'][..., 1]).nanmean()
            out['tri_sym_mm'] = r['sym'].abs().reshape(-1, 2).nanmean(dim=0)   # [2]: before, after; a pair switched off is NaN
            if self.fit_smpl:
                fit_bad = r['status'] == 2
        elif self.tri == 'robust':
            tri, used = triangulation_weighted(sel, x, self.cam_id_list, weights, robust_px=self.tri_thresh, return_inliers=True)
        else:
            tri = triangulation_weighted(sel, x, self.cam_id_list, weights)
        if self.tri == 'robust':
            bits = (used.unsqueeze(-1).int() >> torch.arange(len(cams), device=used.device, dtype=torch.int32)) & 1
            # a zero mask is the fallback: no two views agreed, the DLT ran over all of them
            out['tri_inlier_views'] = torch.where(used == 0, len(cams), bits.sum(dim=-1)).float().mean()
        if weights is not None:
            out['tri_sigma'] = torch.stack([1.0 / weights[m] for m in cams]).mean()
        if self.tri_volume:                        # from whatever point the options above produced, over the views they used
            views = None
            if self.tri == 'robust':               # a zero mask is the fallback: the DLT ran over all views, and so does the fusion
                views = torch.where(used == 0, torch.full_like(used, (1 << len(cams)) - 1), used)
            tri, r = triangulation_volume(tri, cubes, x, self.cam_id_list, torch.stack(chan, dim=0).contiguous(), views=views,
                                          G=self.vol_grid, levels=self.vol_levels, side_mm=self.vol_side, want=('cov', 'status'))
            out['tri_vol_move_mm'] = (tri - r['init']).norm(dim=-1).nanmean()
            out['tri_vol_sigma_mm'] = (r['cov'][..., 0] + r['cov'][..., 3] + r['cov'][..., 5]).sqrt().nanmean()   # passed through: NaN
            out['tri_vol_status'] = torch.stack([(r['status'] == c).float().mean() for c in range(4)])
            if self.fit_smpl:                      # passed through (1, 3): the start came back and there is no covariance
                fit_bad, fit_cov = (r['status'] == 1) | (r['status'] == 3), r['cov']
        if self.calibrate:                         # kept on the device for the one bundle after the loop: the final point, the views it used
            pts, pm = triangulation_inputs(sel, x, self.cam_id_list, weights)
            self.calib_rows.append({'points': pts, 'pmat': pm, 'views': used if self.tri == 'robust' else None,
                                    'init': torch.cat([tri[..., :3], torch.ones_like(tri[..., :1])], dim=-1).contiguous()})
        if self.smooth:                            # kept on the device for the one smoothing after the loop, as --calibrate keeps its rows
            pts, pm = triangulation_inputs(sel, x, self.cam_id_list, weights)
            paths = x.get(cams[0] + '_img_path')
            self.smooth_rows.append({'points': pts, 'pmat': pm, 'views': used if self.tri == 'robust' else None, 'gt': gt[..., :3].contiguous(),
                                     'init': torch.cat([tri[..., :3], torch.ones_like(tri[..., :1])], dim=-1).contiguous(),
                                     'paths': None if paths is None else [str(p) for p in paths]})
        preds = {'tri': tri}
        for m in cams:
            preds['view_' + m] = convert_patch_to_world(sel[m], x, m, is_norm=True)
        for name, p in preds.items():
            e = pose_errors(p, gt, want=('err',))['err'].mean(dim=2)                       # [3,B]
            for metric, a in METRICS_3D:
                out['{}_{}'.format(metric, name)] = e[a]
            if not self.cal_per_act:                                                       # eval.py:51-55
                q = pose_errors(p, gt, in_div=1000.0, want=('pck', 'auc_hits'))
                out['pck_' + name] = q['pck'].mean()
                out['auc_' + name] = (q['auc_hits'].sum(dim=0).float() / q['pck'].numel()).mean() * 100
        out['world_gt'], out['world_tri'] = gt, preds['tri']
        if self.resolve_track:                     # kept on the device for the one pass per camera after the loop, as --smooth keeps its rows
            row = {'gt': gt[..., :3].contiguous(), 'mode': 'views' if self.resolve == 'views' else mode}
            for m in cams:
                paths = x.get(m + '_img_path')
                if paths is None:                  # the cameras of a sample show the same frame
                    paths = x.get(cams[0] + '_img_path')
                row[m] = {'kps': raw_kps[m].detach().float().contiguous(), 'labels': x[m + '_joints'],
                          'world': convert_patch_to_world(raw_kps[m], x, m, is_norm=True)[..., :3].contiguous(),
                          'view': preds['view_' + m][..., :3].contiguous(), 'paths': None if paths is None else [str(p) for p in paths]}
            self.rt_rows.append(row)
        if self.fit_smpl:                          # after everything else, on the final world joints
            if len(cams) > 1:
                out.update(self.fit_batch(preds['tri'][..., :3].contiguous(), fit_bad, fit_cov))
            else:                                  # one camera: its selected hypothesis
                out.update(self.fit_batch(preds['view_' + cams[0]][..., :3].contiguous(), None, None))
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
            if 'tri_inlier_views' in host:
                self.tri_views += float(host['tri_inlier_views'])
                self.tri_batches += 1
            if 'tri_sigma' in host:
                self.tri_sigma += float(host['tri_sigma'])
                self.sigma_batches += 1
            if 'tri_refine_px' in host:
                self.refine_px += float(host['tri_refine_px'])
                self.refine_gain += float(host['tri_refine_gain_px'])
                self.refine_batches += 1
            if 'tri_sym_mm' in host:
                self.sym_mm += host['tri_sym_mm']
            if 'tri_vol_status' in host:
                self.vol_move += float(host['tri_vol_move_mm'])
                self.vol_sigma += float(host['tri_vol_sigma_mm'])
                self.vol_status += host['tri_vol_status']
                self.vol_batches += 1
            if 'fit_status' in host:
                self.fit_rows.append({k[4:]: v for k, v in host.items() if k.startswith('fit_')})
            if 'resolve_hyp0' in host:
                self.res_exchanged += float(host['resolve_exchanged'])
                self.res_hyp0 += float(host['resolve_hyp0'])
                self.res_batches += 1
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
        """Prints and writes <log_dir>/eval/eval_result.txt with the reference's lines (eval.py:206-296)."""
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
        if self.tri == 'robust':                   # after the reference's lines; --tri dlt leaves the file as it was
            lines.append('TRI inlier views ({} px): {} of {}'.format(self.tri_thresh, self.tri_views / max(self.tri_batches, 1),
                                                                     len(self.cam_id_list)))
        if self.resolve == 'views':                # after everything else; --resolve gt leaves the file as it was
            n = max(self.res_batches, 1)
            lines.append('RESOLVE views: exchanged {} , hypothesis 0 kept {}'.format(self.res_exchanged / n, self.res_hyp0 / n))
        if self.tri_weight == 'spread':            # after everything else; --tri-weight depth leaves the file as it was
            lines.append('TRI weight spread: mean sigma {} px'.format(self.tri_sigma / max(self.sigma_batches, 1)))
        if self.tri_refine == 'lm':                # after everything else; --tri-refine none leaves the file as it was
            n = max(self.refine_batches, 1)
            lines.append('TRI refine lm (huber {}): reprojection RMS {} px, gained {} px'.format(
                self.tri_huber, self.refine_px / n, self.refine_gain / n))
        if self.tri_refine == 'skeleton':          # after everything else; none and lm leave the file as it was
            n = max(self.refine_batches, 1)
            lines.append('TRI refine skeleton (huber {}, sym {}): reprojection RMS {} px, gained {} px, limb asymmetry {} -> {} mm'.format(
                self.tri_huber, self.tri_sym, self.refine_px / n, self.refine_gain / n, self.sym_mm[0] / n, self.sym_mm[1] / n))
        if self.tri_volume:                        # after everything else; without --tri-volume the file is as it was
            n = max(self.vol_batches, 1)
            lines.append('TRI volume (side {} mm, grid {}, levels {}): moved {} mm, sigma {} mm'.format(
                self.vol_side, self.vol_grid, self.vol_levels, self.vol_move / n, self.vol_sigma / n))
            lines.append('TRI volume status: fused {} , passed through {} , mode on a face {} , logits not finite {}'.format(
                *(self.vol_status / n)))
        if self.fit_smpl:                          # after everything else; without --fit-smpl the file is as it was
            lines.append(self.write_fit())
        if self.calibrate:                         # after everything else; without --calibrate the file is as it was
            lines.extend(self.write_calibration())
        if self.smooth:                            # after everything else; without --smooth the file is as it was
            lines.extend(self.write_smooth())
        if self.resolve_track:                     # after everything else; without --resolve-track the file is as it was
            lines.extend(self.write_resolve_track())
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
CLI_VOLUME = (  # --tri-volume and its grid, parsed after CLI (a table of their own: CLI's last entries are pinned by older tests)
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


CLI_FIT = (  # --fit-smpl and its settings, parsed after CLI_VOLUME (a table of their own: older tests pin the tables above)
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


def mirror_fit_options(config, opt):
    """The --fit-smpl flags as model_params keys (only the ones given: the defaults live in xas_amd.ops_smplfit)."""
    mp = config['model_params']
    mp['fit_smpl'], mp['smpl_model'], mp['fit_iters'] = opt.fit_smpl, opt.smpl_model, opt.fit_iters
    for key in ('fit_pose_prior', 'fit_shape_prior'):
        if getattr(opt, key) is not None:
            mp[key] = getattr(opt, key)


CLI_CALIB = (  # --calibrate / --calibration and their settings, parsed after CLI_FIT (a table of their own, as above)
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
    mp = config['model_params']
    mp['calibrate'], mp['calibration'], mp['calib_iters'] = opt.calibrate, opt.calibration, opt.calib_iters
    for key in ('calib_prior_rot', 'calib_prior_trans', 'calib_free'):
        if getattr(opt, key) is not None:
            mp[key] = getattr(opt, key)


CLI_SMOOTH = (  # --smooth and its settings, parsed after CLI_CALIB (a table of their own, as above)
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
    mp = config['model_params']
    mp['smooth'], mp['smooth_iters'] = opt.smooth, opt.smooth_iters
    for key in ('smooth_acc', 'smooth_gap'):
        if getattr(opt, key) is not None:
            mp[key] = getattr(opt, key)


CLI_RESOLVE_TRACK = (  # --resolve-track and its settings, parsed after CLI_SMOOTH (a table of their own, as above)
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
    for key in ('resolve_track', 'rt_vel', 'rt_hyp', 'rt_swap', 'rt_gap'):
        if getattr(opt, key) is not None:
            config['model_params'][key] = getattr(opt, key)


def main():
    parser = ArgumentParser()
    for flag, kw in CLI + CLI_VOLUME + CLI_FIT + CLI_CALIB + CLI_SMOOTH + CLI_RESOLVE_TRACK:
        parser.add_argument(flag, **kw)
    opt = parser.parse_args()
    with open(opt.config) as f:
        config = yaml.load(f, Loader=yaml.FullLoader)
    config['model_params']['cam_id_list'] = config['dataset_params']['cam_id_list']
    config['model_params']['tri_weight'] = opt.tri_weight
    config['model_params']['tri_refine'] = 'skeleton' if opt.tri_skeleton else opt.tri_refine
    config['model_params']['tri_huber'] = opt.tri_huber
    config['model_params']['tri_sym'] = opt.tri_sym
    config['model_params']['tri_volume'] = opt.tri_volume
    config['model_params']['tri_vol_side'] = opt.tri_vol_side
    config['model_params']['tri_vol_grid'] = opt.tri_vol_grid
    config['model_params']['tri_vol_levels'] = opt.tri_vol_levels
    mirror_fit_options(config, opt)
    mirror_calib_options(config, opt)
    mirror_smooth_options(config, opt)
    mirror_resolve_track_options(config, opt)
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
