#!/usr/bin/env python3
"""torchrun entry of the MI355X-native trainer (reference: train.py:1-344, same CLI and checkpoint format).

    torchrun --nproc-per-node=N train.py --config config/HM36_Multi_SurS1.yaml [--checkpoint ... --finetune]
             [--batch_size B --epoch E --worker W --seed S --extra_tag T --log_dir D] [--synthetic STEPS]
             [--mv-2d W --mv-3d W --mv-huber PX --mv-detach]
             [--pseudo-online BANK.npz --pseudo-look shade|parts --smpl-model ROOT]

Differences from the reference, all outside the hot step: the two DistributedDataParallel wrappers are
replaced by xas_amd.engine.TrainStep (flat gradient arenas + bucketed RCCL all-reduce on a side stream);
TensorBoard logging is optional (skipped when tensorboard is not installed); `--synthetic STEPS` trains on
synthetic batches with the dataloader's key contract when the licensed datasets / cv2 / scikit-fmm loader
(`train_util.basic_data`, taken from the reference checkout on PYTHONPATH) are unavailable.
"""
import os
import random
from argparse import ArgumentParser
from time import gmtime, strftime

import numpy as np

os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')   # dmabuf IPC (RCCL between processes) on this driver
import torch
import yaml
from torch.distributed import destroy_process_group, init_process_group
from torch.optim.lr_scheduler import MultiStepLR

from train_util import tb_vis
from xas_amd import engine
from xas_amd.synthetic import synthetic_batch


def setup_seed(seed):
    if seed != -1:
        torch.manual_seed(seed)
        torch.cuda.manual_seed_all(seed)
        np.random.seed(seed)
        random.seed(seed)


def ddp_setup():
    init_process_group(backend='nccl')            # RCCL on ROCm
    torch.cuda.set_device(int(os.environ['LOCAL_RANK']))


class Trainer:
    """Same constructor arguments as the reference Trainer (train.py:47-59)."""

    def __init__(self, config, unsup_model, unsup_disc, train_data, optimizer_detector, save_dir,
                 checkpoint_path=None, optimizer_discriminator=None, mode='train', pseudo=None):
        self.pseudo = pseudo               # xas_amd.pseudo.PseudoSynth (--pseudo-online) or None: the batch's own pseudo samples
        self.gpu_id = int(os.environ['LOCAL_RANK'])
        self.unsup_model = unsup_model.to(self.gpu_id)
        self.unsup_disc = unsup_disc.to(self.gpu_id)
        self.train_data = train_data
        self.optimizer_detector = optimizer_detector
        self.optimizer_discriminator = optimizer_discriminator
        self.epochs_run = 0
        self.config = config
        self.tb_parent_ids = np.array(config['model_params']['parent_ids'])      # train.py:91-92
        self.tb_pair_ids = np.array(config['model_params']['flip_pairs'])
        self.save_dir = save_dir
        if checkpoint_path is not None:
            self._load_checkpoint(checkpoint_path, mode)
        tp = config['train_params']
        self.scheduler_detector = MultiStepLR(optimizer_detector, tp['epoch_milestones'], gamma=0.1,
                                              last_epoch=-1 + self.epochs_run * (tp['lr_kp_detector'] != 0))
        self.scheduler_discriminator = None
        if optimizer_discriminator is not None:
            self.scheduler_discriminator = MultiStepLR(optimizer_discriminator, tp['epoch_milestones'], gamma=0.1,
                                                       last_epoch=-1 + self.epochs_run * (tp['lr_discriminator'] != 0))
        self.step = engine.TrainStep(config, self.unsup_model, self.unsup_disc, optimizer_detector,
                                     optimizer_discriminator)

    def _load_checkpoint(self, checkpoint_path, mode):
        ckpt = torch.load(checkpoint_path, map_location=f'cuda:{self.gpu_id}')
        self.unsup_model.load_state_dict(ckpt['unsup_model'], strict=False)
        self.optimizer_detector.load_state_dict(ckpt['optimizer_detector'])
        if self.optimizer_detector.ema_arena is not None:       # averaged weights (train_params.ema_decay)
            ema, names = ckpt.get('unsup_model_ema'), self._ema_param_names()
            if ema is None:
                print("Checkpoint has no 'unsup_model_ema': the averaged weights start from the loaded parameters")
                self.optimizer_detector.load_ema([p.data for p in self.optimizer_detector.arena_params()])
            else:                                                # all of them or none: never a mix of averaged and raw weights
                missing = [n for n in names if n not in ema]
                if missing:
                    raise KeyError("checkpoint %s: 'unsup_model_ema' lacks %d of %d parameters (%s%s)" % (
                        checkpoint_path, len(missing), len(names), ', '.join(missing[:4]), ', ...' if len(missing) > 4 else ''))
                self.optimizer_detector.load_ema([ema[n] for n in names])
        try:
            self.unsup_disc.load_state_dict(ckpt['unsup_disc'], strict=False)
            if self.optimizer_discriminator is not None:
                self.optimizer_discriminator.load_state_dict(ckpt['optimizer_discriminator'])
        except Exception:
            print('Load new discriminator for ablation')
        if mode == 'train':
            self.epochs_run = ckpt['epochs']
            print(f'Resuming training from checkpoint at Epoch {self.epochs_run}')
        elif mode == 'finetune':
            print(f'Finetuning from checkpoint at Epoch {self.epochs_run}')
        else:
            raise NotImplementedError

    def _ema_param_names(self):
        """Names in unsup_model.state_dict() of the detector optimizer's parameters, in the optimizer's order."""
        by_id = {id(p): n for n, p in self.unsup_model.named_parameters()}
        return [by_id[id(p)] for p in self.optimizer_detector.arena_params()]

    def _save_checkpoint(self, epoch):
        ckpt = {'unsup_model': self.unsup_model.state_dict(), 'unsup_disc': self.unsup_disc.state_dict(),
                'epochs': epoch, 'optimizer_detector': self.optimizer_detector.state_dict(),
                'optimizer_discriminator': self.optimizer_discriminator.state_dict()}
        if self.optimizer_detector.ema_arena is not None:
            # the keys of 'unsup_model': parameters from the shadow arena, buffers (the batch-norm running statistics are
            # momentum averages already) from the live model
            ema = dict(ckpt['unsup_model'])
            ema.update((n, v.clone()) for n, v in zip(self._ema_param_names(), self.optimizer_detector.ema_views()))
            ckpt['unsup_model_ema'] = ema
        torch.save(ckpt, os.path.join(self.save_dir, '{:05d}_ckpt.pth.tar'.format(epoch)))

    def convert_data_to_device(self, x):
        for key in x:
            if isinstance(x[key], torch.Tensor):
                x[key] = x[key].to(self.gpu_id, non_blocking=True)
            elif isinstance(x[key], dict):
                x[key] = self.convert_data_to_device(x[key])
            elif isinstance(x[key], np.ndarray):
                x[key] = torch.tensor(x[key]).to(self.gpu_id)
        return x

    def train(self, tb_logger=None):
        tp = self.config['train_params']
        for epoch in range(self.epochs_run, tp['num_epochs']):
            if hasattr(self.train_data, 'sampler') and hasattr(self.train_data.sampler, 'set_epoch'):
                self.train_data.sampler.set_epoch(epoch)
            for it, x in enumerate(self.train_data):
                x = self.convert_data_to_device(x)
                if self.pseudo is not None:                          # rendered pseudo samples in place of the batch's
                    self.pseudo.fill(x, ['cam_{}'.format(c) for c in self.config['dataset_params']['cam_id_list']])
                loss_disc, loss_kp, total, output = self.step(x)
                if self.gpu_id == 0 and tb_logger is not None:      # train.py:192-199: every step, total = None on steps
                    cur = epoch * len(self.train_data) + it          # where only the discriminator was updated
                    tb_vis(tb_logger, cur, self.tb_pair_ids, self.tb_parent_ids,
                           total.detach().item() if total is not None else None, loss_kp, loss_disc, output, x, self.config,
                           self.scheduler_detector)
            if self.gpu_id == 0 and tb_logger is not None:           # guarded optimizer step (train_params.max_grad_norm /
                skipped = self.step.skipped_steps()                   # skip_nonfinite_grads): once per epoch, one sync
                for k, norm in self.step.last_grad_norm.items():
                    if norm is not None:
                        tb_logger.add_scalar('grad_guard/%s_grad_norm' % k, float(norm), epoch)
                        tb_logger.add_scalar('grad_guard/%s_skipped_steps' % k, skipped[k], epoch)
            self.scheduler_detector.step()
            if self.scheduler_discriminator is not None:
                self.scheduler_discriminator.step()
            if self.gpu_id == 0 and (epoch % tp['checkpoint_freq'] == 0 or epoch == tp['num_epochs'] - 1):
                self._save_checkpoint(epoch)


class _SyntheticLoader:
    def __init__(self, steps, batch, cams, device, seed):
        self.steps, self.batch, self.cams, self.device, self.seed = steps, batch, cams, device, seed

    def __len__(self):
        return self.steps

    def __iter__(self):
        for i in range(self.steps):
            yield synthetic_batch(self.batch, self.cams, self.device, seed=self.seed + i)


def prepare_data(config, world_size, worker, synthetic_steps, device, seed):
    bs = config['train_params']['batch_size'] // world_size            # batch_size is GLOBAL (train.py:274)
    if synthetic_steps:
        return _SyntheticLoader(synthetic_steps, bs, config['dataset_params']['cam_id_list'], device, max(seed, 0))
    from torch.utils.data import DataLoader
    from torch.utils.data.distributed import DistributedSampler
    from train_util import basic_data              # the reference's CPU dataset code (cv2, scikit-fmm)
    ds = basic_data(config)
    return DataLoader(ds, batch_size=bs, shuffle=False, pin_memory=True, num_workers=worker, sampler=DistributedSampler(ds))


def create_logger(opt):
    if opt.checkpoint is not None and not opt.finetune:
        log_dir = os.path.dirname(opt.checkpoint)
    else:
        seed = 'seed{}_'.format(opt.seed if opt.seed != -1 else '_rand')
        log_dir = os.path.join(opt.log_dir, os.path.basename(opt.config).split('.')[0])
        if opt.finetune:
            log_dir += '_FINETUNE'
        log_dir += '_' + seed + opt.extra_tag + strftime('%d_%m_%y_%H.%M.%S', gmtime())
    tb = None
    if os.environ['LOCAL_RANK'] == '0':
        os.makedirs(log_dir, exist_ok=True)
        try:
            from torch.utils.tensorboard import SummaryWriter
            tb = SummaryWriter(log_dir=os.path.join(log_dir, 'tensorboard'))
        except Exception:                      # TensorBoard not installed: same calls, plain files
            from train_util import JsonlWriter
            tb = JsonlWriter(os.path.join(log_dir, 'tensorboard'))
    return log_dir, tb


CLI = (  # same flags as the reference entry (train.py:305-315) + --synthetic
    ('--config', dict(required=True, help='path to config')),
    ('--log_dir', dict(default='log', help='path to log into')),
    ('--checkpoint', dict(default=None, help='path to checkpoint to restore')),
    ('--batch_size', dict(default=None, type=int)),
    ('--epoch', dict(default=None, type=int)),
    ('--worker', dict(default=10, type=int)),
    ('--extra_tag', dict(default='')),
    ('--finetune', dict(default=False, action='store_true', help='finetune the model')),
    ('--seed', dict(default=-1, type=int)),
    ('--synthetic', dict(default=0, type=int, help='train on N synthetic batches per epoch')),
    # (no reference counterpart) the multi-view consistency term, model_params.loss_config.multiview_loss; given neither weight,
    # nothing is inserted and the step runs the launches it ran before
    ('--mv-2d', dict(default=None, type=float, metavar='W', dest='mv_2d',
                     help='weight of the multi-view reprojection term (px^2 per joint) against the triangulated joint')),
    ('--mv-3d', dict(default=None, type=float, metavar='W', dest='mv_3d',
                     help="weight of the multi-view depth term (mm^2 per joint): every view's nearest hypothesis against the "
                          'triangulated joint')),
    ('--mv-huber', dict(default=0.0, type=float, metavar='PX', dest='mv_huber',
                        help="Huber's delta of the reprojection term in pixels, 0 = squared loss")),
    ('--mv-detach', dict(default=False, action='store_true', dest='mv_detach',
                         help='the triangulated joint is a constant target (a pseudo-label), not a function of the views')),
)


CLI_PSEUDO = (  # online pseudo samples, parsed after CLI (a table of their own: CLI's entries are pinned by older tests)
    ('--pseudo-online', dict(default=None, metavar='BANK.npz', dest='pseudo_online',
                             help='render the pseudo images and joints of every batch on the device from this bank of SMPL '
                                  'poses (`pose` [N,72], optional `betas` [N,10]) in place of the ones the batch brings')),
    ('--pseudo-look', dict(default='shade', choices=['shade', 'parts'], dest='pseudo_look',
                           help='--pseudo-online: shaded untextured body, or pure body-part colours')),
    ('--smpl-model', dict(default=None, metavar='ROOT', dest='smpl_model',
                          help='directory of the SMPL model files (replaces model_params.smpl_layer_params.model_path), or an '
                               '.npz of exported arrays with `h36m_regressor` and the faces `f`')),
)


def pseudo_source(opt, config, model):
    """The PseudoSynth of --pseudo-online on `model`'s SMPL layer, or None without the flag (nothing is imported then)."""
    if opt.pseudo_online is None:
        return None
    from xas_amd.pseudo import PseudoSynth
    di = config['dataset_params'].get('dataiter') or {}
    seed = max(opt.seed, 0) + int(os.environ.get('RANK', '0'))           # every rank draws bodies of its own
    return PseudoSynth(opt.pseudo_online, model.smpl_layer, model.h36m_regressor, look=opt.pseudo_look, seed=seed,
                       mean=di.get('mean'), std=di.get('std'))


def multiview_entry(opt):
    """loss_config's `multiview_loss` entry of --mv-2d / --mv-3d / --mv-huber / --mv-detach, or None if neither weight is given."""
    if opt.mv_2d is None and opt.mv_3d is None:
        return None
    return dict(weight_2d=opt.mv_2d or 0.0, weight_3d=opt.mv_3d or 0.0, huber_px=opt.mv_huber, detach_target=opt.mv_detach)


def main():
    parser = ArgumentParser()
    for flag, kw in CLI + CLI_PSEUDO:
        parser.add_argument(flag, **kw)
    opt = parser.parse_args()
    with open(opt.config) as f:
        config = yaml.load(f, Loader=yaml.FullLoader)
    config['model_params']['cam_id_list'] = config['dataset_params']['cam_id_list']
    if multiview_entry(opt) is not None:
        config['model_params']['loss_config']['multiview_loss'] = multiview_entry(opt)
    for key, val in (('batch_size', opt.batch_size), ('num_epochs', opt.epoch)):
        if val:
            config['train_params'][key] = val
    ddp_setup()
    setup_seed(opt.seed)
    rank_local, world = int(os.environ['LOCAL_RANK']), int(os.environ['WORLD_SIZE'])
    save_dir, tb_logger = create_logger(opt)
    smpl_arrays = None
    if opt.smpl_model is not None and opt.smpl_model.endswith('.npz'):
        from xas_amd.pseudo import load_smpl_arrays
        smpl_arrays = load_smpl_arrays(opt.smpl_model)
    elif opt.smpl_model is not None:
        config['model_params'].setdefault('smpl_layer_params', {})['model_path'] = opt.smpl_model
    nets = engine.prepare_model(config, smpl_arrays)
    loader = prepare_data(config, world, opt.worker, opt.synthetic, torch.device('cuda', rank_local), opt.seed)
    trainer = Trainer(config, nets[0], nets[1], loader, nets[2], save_dir, checkpoint_path=opt.checkpoint,
                      optimizer_discriminator=nets[3], mode='finetune' if opt.finetune else 'train',
                      pseudo=pseudo_source(opt, config, nets[0]))
    trainer.train(tb_logger)
    if tb_logger is not None:
        tb_logger.close()
    destroy_process_group()


if __name__ == '__main__':
    main()
