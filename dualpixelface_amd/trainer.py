"""A small native trainer behind the reference's entry point.

The reference drives its plugin with ``pytorch_lightning.Trainer`` 1.4.9 (main.py:43-58: fit / test, ``ModelCheckpoint`` every epoch
into the workspace, ``resume_from_checkpoint``, validation every epoch, ``max_epochs = option.epoch``, DDP + SyncBatchNorm under
``accelerator == 'ddp'``).  pytorch_lightning is not part of this image, and the MI355X step keeps its gradients and optimiser state in
flat arenas that a generic trainer would not know how to checkpoint, so this module provides those behaviours natively:

  * ``Trainer(option).fit(model)`` / ``.test(model)`` -- epochs over ``model.train_dataloader()`` (or loaders passed in) calling the
    fused ``model.train_step`` (forward + loss + backward + bucketed RCCL all-reduce + Adam / SGD / RMSprop), the scheduler of
    ``scheduler_selector`` (StepLR(35, 0.5) / ExponentialLR(0.5) / CosineAnnealingLR(500, 1e-6) stepped per epoch), validation
    with the metric hooks every epoch, one checkpoint per epoch ``checkpoint_epoch=XX.ckpt``.
  * the option keys ``accumulate_grad_batches`` (N micro-batches per optimiser step; the last group of an epoch may be short),
    ``gradient_clip_val`` (global 2-norm) and ``track_grad_norm`` (2), with PL's meaning and executed inside ``train_step``:
    ``global_step``, ``max_steps`` and ``log_every`` count optimiser steps, and the log records carry ``grad_norm``.
  * checkpoints hold ``state_dict`` under the reference's parameter names (a PL checkpoint of the reference loads into this
    model, and the other way round), the flat optimiser state (Adam moments, SGD momentum buffer or RMSprop square average), the step /
    epoch counters and the learning rate.
  * one process per GPU under torchrun: the training set is sharded by SAMPLE with torch's DistributedSampler (own generator
    seeded by (seed, epoch), padded so every rank runs the same number of equal-shape steps -- what PL does for the reference), gradient all-reduce through
    ``distributed.make_reducer``, SyncBatchNorm when ``option.sync_batch``; rank 0 writes checkpoints and logs.
"""
import json
import math
import os
import re
import time

import torch

from . import distributed as dd
from . import optim
from . import confidence, reconstruct, shading


def epoch_lr(option, epoch):
    """Learning rate of ``epoch`` (0-based) under the reference's schedulers (model_selector.py:45-58), stepped once per epoch."""
    lr0 = float(option.init_lr)
    name = getattr(option, 'scheduler', 'none')
    if name == 'steplr':
        return lr0 * 0.5 ** (epoch // 35)
    if name == 'explr':
        return lr0 * 0.5 ** epoch
    if name == 'cosanneal':
        return 1e-6 + (lr0 - 1e-6) * (1 + math.cos(math.pi * epoch / 500)) / 2
    if name == 'none':
        return lr0
    raise NotImplementedError('scheduler is not defined, please check your scheduler configuration !')


CKPT_VERSION = 2


class Trainer(object):
    def __init__(self, option, workspace_path=None, log_every=10, max_steps=None, rank=None, world_size=None):
        self.option = option
        self.workspace_path = str(workspace_path or getattr(option, 'workspace_path', '.'))
        self.log_every = log_every
        self.max_steps = max_steps              # optional cap on optimizer steps (smoke runs)
        if rank is None:
            rank, world_size, _ = dd.init_from_env()
        self.rank, self.world_size = rank, world_size
        self.epoch = 0
        self.global_step = 0
        self.history = []

    # ------------------------------------------------------------------ checkpoints
    def checkpoint_path(self, epoch):
        return os.path.join(self.workspace_path, 'checkpoint_epoch=%02d.ckpt' % epoch)

    def save_checkpoint(self, model, path=None):
        path = path or self.checkpoint_path(self.epoch)
        ckpt = {
            # PL 1.4.9 dump_checkpoint: the NEXT epoch to run and global_step + 1; 'dpf_ckpt_version' tells load_checkpoint which
            # convention a file follows (absent + no 'pytorch-lightning_version' = round-1 files: 'epoch' was the FINISHED epoch)
            'dpf_ckpt_version': CKPT_VERSION, 'epoch': self.epoch + 1, 'global_step': self.global_step + 1,
            'state_dict': {k: v.detach().cpu() for k, v in model.state_dict().items()},
            'optimizer_states': [optim.to_checkpoint(model, self.option)],
            'lr': epoch_lr(self.option, self.epoch),
            'hyper_parameters': {'model_name': getattr(self.option, 'model_name', 'stereodpnet')},
        }
        if self.rank == 0:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            tmp = path + '.tmp'
            torch.save(ckpt, tmp)
            os.replace(tmp, path)
        return path

    def load_checkpoint(self, model, path, resume=True):
        """``resume``: restore optimizer moments and counters too (PL's resume_from_checkpoint); else weights only."""
        ckpt = torch.load(path, map_location='cpu', weights_only=False)
        weights = ckpt['state_dict'] if 'state_dict' in ckpt else ckpt['model']
        epoch, global_step = self.epoch, self.global_step
        if resume:
            # Resolve the counters BEFORE anything is restored: a checkpoint whose convention cannot be determined must leave the model
            # and the trainer untouched (the error used to fire after load_state_dict and the counter update).
            epoch = int(ckpt.get('epoch', 0))                                 # PL restores current_epoch = ckpt['epoch']
            global_step = int(ckpt.get('global_step', 0))
            if int(ckpt.get('dpf_ckpt_version', 0)) >= 2:
                global_step = max(global_step - 1, 0)                         # our own files: undo dump_checkpoint's + 1 exactly
            elif 'pytorch-lightning_version' not in ckpt and 'epoch' in ckpt:
                # Unversioned files of this trainer exist in two generations that no key tells apart: round 1 stored the FINISHED epoch,
                # later revisions the NEXT epoch to run (and the plain global_step).  save_checkpoint names the file after the finished
                # epoch (checkpoint_epoch=NN.ckpt), so the name decides; without it the caller has to say (option.legacy_ckpt_epoch =
                # 'finished' | 'next') -- never guess: a wrong guess silently skips or repeats an epoch and shifts the LR schedule.
                m = re.search(r'checkpoint_epoch=(\d+)\.ckpt$', os.path.basename(path))
                conv = getattr(self.option, 'legacy_ckpt_epoch', None)
                if conv is None and m is not None:
                    if epoch == int(m.group(1)):
                        conv = 'finished'
                    elif epoch == int(m.group(1)) + 1:
                        conv = 'next'
                if conv not in ('finished', 'next'):
                    raise ValueError("unversioned checkpoint %r: cannot tell whether its 'epoch' = %d is the finished epoch or the next one to "
                                     "run; set option.legacy_ckpt_epoch to 'finished' or 'next', or load the weights only "
                                     "(load_checkpoint(..., resume=False) / --load_model without resume).  Nothing was restored." % (path, epoch))
                if conv == 'finished':
                    epoch += 1
            # the same rule for the optimiser: state of another kind than option.optim selects cannot continue this run
            states = ckpt.get('optimizer_states') or []
            kind = states[0].get('kind') if states and isinstance(states[0], dict) else None
            want = optim.of(self.option).ckpt
            if kind in [r.ckpt for r in optim.TABLE.values()] and kind != want:
                raise ValueError("checkpoint %r holds %s optimiser state, option.optim = %r needs %s: resume with the optimiser the run was "
                                 "trained with, or load the weights only (load_checkpoint(..., resume=False) / --load_model without "
                                 "resume).  Nothing was restored." % (path, kind, getattr(self.option, 'optim', 'adam'), want))
        model.load_state_dict(weights, strict=bool(getattr(self.option, 'load_strict', True)))
        if resume:
            self.epoch, self.global_step = epoch, global_step
            if states:
                optim.from_checkpoint(model, states[0])
        return ckpt

    # ------------------------------------------------------------------ loops
    def _shard(self, loader, epoch):
        """This rank's batches of one epoch.  world_size 1: the loader as it is.  Otherwise the loader is rebuilt over the same
        dataset with a DistributedSampler (shuffled by its own generator seeded with (seed, epoch), padded to a multiple of the
        world size): every rank sees the same number of batches with the same shapes, so the per-step collectives always pair up."""
        if self.world_size == 1:
            if hasattr(loader, 'set_epoch'):
                loader.set_epoch(epoch)                              # FaceDPBatcher: its own generator seeded with (seed, epoch)
            return loader
        key = id(loader)
        if getattr(self, '_dist_key', None) != key:
            from torch.utils.data import DataLoader
            from torch.utils.data.distributed import DistributedSampler
            self._dist_sampler = DistributedSampler(loader.dataset, num_replicas=self.world_size, rank=self.rank, shuffle=True,
                                                    seed=int(getattr(self.option, 'seed', 1)), drop_last=False)
            if hasattr(loader, 'with_sampler'):
                self._dist_loader = loader.with_sampler(self._dist_sampler)
            else:
                self._dist_loader = DataLoader(loader.dataset, batch_size=loader.batch_size, sampler=self._dist_sampler,
                                               num_workers=loader.num_workers, collate_fn=loader.collate_fn,
                                               pin_memory=loader.pin_memory, drop_last=loader.drop_last)
            self._dist_key = key
        self._dist_sampler.set_epoch(epoch)
        return self._dist_loader

    def _to_device(self, batch, device):
        return {k: (v.to(device, non_blocking=True) if torch.is_tensor(v) else v) for k, v in batch.items()}

    def _log(self, record):
        self.history.append(record)
        if self.rank == 0:
            os.makedirs(self.workspace_path, exist_ok=True)
            with open(os.path.join(self.workspace_path, 'log.jsonl'), 'a') as fh:
                fh.write(json.dumps(record) + '\n')

    def validates_on_all_ranks(self):
        """Config key ``validate_on_all_ranks`` (default true): with more than one rank every rank validates its share of the batches;
        false keeps validation on rank 0 while the others wait."""
        return self.world_size > 1 and bool(getattr(self.option, 'validate_on_all_ranks', True))

    def validate(self, model, loader, test=False):
        """One pass over ``loader`` in deferred metric mode (selectors.metric_selector): no host read per batch, one flush before the
        epoch-end hook.  On all ranks: rank r takes the batches r, r + world, ... of the same loader order, then ONE all-reduce per
        benchmark of (sum of its rows, its batch count) -- issued by every rank whatever it counted, a rank without a batch adds zeros --
        and every rank returns the mean over all batches of the per-batch rows, the figure a single process logs.
        A test pass with option.reconstruct.write_ply on also writes the mesh of every sample it evaluates to
        <output_path or workspace_path/output>/recon/<loader position>_<sample>.ply (self.written_meshes lists them); validation during fit
        writes nothing."""
        device = model.flat_parameters().device
        write = test and reconstruct.settings(self.option).write_ply
        self.written_meshes = []
        sel = model.metric_model
        share = self.validates_on_all_ranks()
        model.eval()
        outputs = []
        self.validated_batches = []                          # loader positions this rank ran (tests)
        with torch.no_grad(), sel.deferred():
            for i, batch in enumerate(loader):
                if share and i % self.world_size != self.rank:
                    continue
                batch = self._to_device(batch, device)
                results = (model.test_step if test else model.validation_step)(batch, i)
                outputs.append(None if results is None else i)
                if write and results is not None:
                    guide = model._views(batch)[0] if hasattr(model, '_views') else None
                    self.written_meshes += reconstruct.write_batch(self.option, self.workspace_path, i, results,
                                                                   confidence.gated(self.option, results, batch, 'reconstruct'), guide)
                self.validated_batches.append(i)
        sel.flush()
        (model.test_epoch_end if test else model.validation_epoch_end)(outputs)
        if share:
            rows = self._all_rank_rows(sel, device)
        else:
            rows = {n: f.get_value() for n, f in zip(sel.metric_name, sel.metric_func) if f.index > 0}
        for f in sel.metric_func:
            f.clear()
        self._confidence_report(model, device, share)
        self._shading_report(model, device, share)
        model.train()
        return rows

    def _shading_report(self, model, device, share):
        """option.shading.report: the sums the validation steps added into model.shading_table, read ONCE here (summed over the ranks by one
        all-reduce that every rank issues, whatever it counted) -> self.shading_report, the dict of shading.report_rows, logged; None with
        the report off.  The model's table is cleared for the next pass."""
        s = shading.settings(self.option)
        self.shading_report = None
        if not (s.enabled and s.report):
            return
        table = getattr(model, 'shading_table', None)
        model.shading_table = None
        if table is None:
            table = shading.new_table(device)
        if share:
            import torch.distributed as dist
            dist.all_reduce(table, op=dist.ReduceOp.SUM)
        self.shading_report = shading.report_rows(table.tolist())
        self._log({'epoch': self.epoch, 'shading_report': self.shading_report})
        if self.rank == 0:
            print('shading: %s' % (self.shading_report,))

    def _confidence_report(self, model, device, share):
        """option.confidence.report: the sparsification table the validation steps added into model.confidence_table, read ONCE here (summed
        over the ranks by one all-reduce that every rank issues, whatever it counted) -> self.confidence_curve, the rows of
        confidence.curve_rows, logged per bin edge; None with the report off.  The model's table is cleared for the next pass."""
        s = confidence.settings(self.option)
        self.confidence_curve = None
        if not (s.enabled and s.report):
            return
        table = getattr(model, 'confidence_table', None)
        model.confidence_table = None
        if table is None:
            table = confidence.new_table(s, device)
        if share:
            import torch.distributed as dist
            dist.all_reduce(table, op=dist.ReduceOp.SUM)
        self.confidence_curve = confidence.curve_rows(table.tolist())
        self._log({'epoch': self.epoch, 'confidence_curve': self.confidence_curve})
        if self.rank == 0:
            print('confidence >= edge: coverage, mean |pred - label| (%s, %d bins)' % (s.measure, s.bins))
            for row in self.confidence_curve:
                err = 'none' if row['mean_error'] is None else '%.4f' % row['mean_error']
                print('%10.4f %10.4f %10s' % (row['edge'], row['coverage'], err))

    def _all_rank_rows(self, sel, device):
        import torch.distributed as dist
        rows = {}
        for name, f in zip(sel.metric_name, sel.metric_func):
            packed = torch.tensor([math.fsum(f.metric[k]) for k in f.keys] + [float(f.index)], dtype=torch.float64, device=device)
            dist.all_reduce(packed, op=dist.ReduceOp.SUM)
            packed = packed.tolist()
            if packed[-1] > 0:
                rows[name] = [v / packed[-1] for v in packed[:-1]]
        return rows

    def fit(self, model, train_loader=None, val_loader=None):
        opt = self.option
        train_loader = train_loader if train_loader is not None else model.train_dataloader()
        if val_loader is None and hasattr(model, 'val_dataloader'):
            try:
                val_loader = model.val_dataloader()
            except Exception:
                val_loader = None
        if getattr(opt, 'load_model', None) and getattr(opt, 'mode', 'train') == 'train':
            self.load_checkpoint(model, opt.load_model, resume=bool(getattr(opt, 'load_strict', True)))
        dd.make_wait_group()                                 # while the ranks are in lock-step (see distributed.make_wait_group)
        dd.broadcast_flat(model.flat_parameters(), 0)
        reducer = dd.make_reducer(model) if self.world_size > 1 else None
        if self.world_size > 1 and getattr(opt, 'sync_batch', False):
            model.enable_sync_batchnorm()
        device = model.flat_parameters().device
        model.train()
        done = False
        accum = optim.knobs(opt).accum                       # (validated here, before the first batch)
        while self.epoch < int(opt.epoch) and not done:
            lr = epoch_lr(opt, self.epoch)
            t0, n = time.time(), 0
            pending = 0                                      # micro-steps since the last optimiser step; 0 again at every epoch end
            for batch, last in _flag_last(self._shard(train_loader, self.epoch), accum > 1):
                batch = self._to_device(batch, device)
                # (the keyword only where it says something: a model without the knobs keeps its train_step(batch, reducer, lr))
                res = model.train_step(batch, reducer, lr=lr, **({'last_in_epoch': True} if last else {}))
                n += int(next(iter(batch.values())).shape[0])
                pending += 1
                if pending < accum and not last:
                    continue
                pending = 0
                self.global_step += 1
                if self.global_step % self.log_every == 0 or self.max_steps:
                    rec = {'epoch': self.epoch, 'step': self.global_step, 'lr': lr}
                    rec.update({k: float(v.detach()) for k, v in res.items() if ('loss' in k or k == 'grad_norm') and torch.is_tensor(v)})
                    self._log(rec)
                if self.max_steps and self.global_step >= self.max_steps:
                    done = True
                    break
            if device.type == 'cuda':
                torch.cuda.synchronize()
            self._log({'epoch': self.epoch, 'epoch_seconds': time.time() - t0, 'samples_per_s_rank': n / max(time.time() - t0, 1e-9)})
            share = self.validates_on_all_ranks()
            if val_loader is not None and (self.rank == 0 or share) and not done:
                rows = self.validate(model, val_loader)
                self._log({'epoch': self.epoch, 'metrics': rows})
            if self.world_size > 1 and not share:
                dd.wait_for_rank0()            # rank-0-only validation: the other ranks wait here (host-side, own long timeout), not inside the next epoch's first all-reduce
            self.save_checkpoint(model)
            self.epoch += 1
        if reducer is not None:
            reducer.remove()
        return self.history

    def test(self, model, loader=None):
        loader = loader if loader is not None else model.test_dataloader()
        return self.validate(model, loader, test=True)


def _flag_last(batches, on):
    """(batch, whether it is the last one) over `batches`, one batch ahead of the caller; with `on` false nothing is looked ahead and
    every flag is False."""
    if not on:
        for batch in batches:
            yield batch, False
        return
    it = iter(batches)
    try:
        held = next(it)
    except StopIteration:
        return
    for batch in it:
        yield held, False
        held = batch
    yield held, True
