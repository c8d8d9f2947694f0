"""One record per ``option.optim``: everything the train step (plugin.py) and the checkpoints (trainer.py) ask about the fused optimiser.

The state lives on the model: ``model._adam`` = {'m', 'v', 'step'} under 'adam'; ``model._optim`` = {'kind', 'buf' | 'sq'} (+ 'dead', 'live':
SGD's liveness mask) under 'sgd' / 'rmsprop', which share the attribute and therefore name their kind.  Both are None before the first step."""
import collections

import torch

from . import ops


class Knobs(collections.namedtuple('Knobs', 'accum clip track')):
    """The trainer's optimisation knobs as PyTorch-Lightning 1.4.9 names them: accum = accumulate_grad_batches (micro-steps per optimiser
    step), clip = gradient_clip_val (0: off; the global 2-norm otherwise), track = track_grad_norm == 2."""
    __slots__ = ()

    @property
    def on(self):
        return self.accum > 1 or self.clip > 0 or self.track

    @property
    def reports(self):
        """Whether an optimiser step returns results['grad_norm']."""
        return self.clip > 0 or self.track


def knobs(option):
    """The Knobs of the top-level option keys accumulate_grad_batches (1), gradient_clip_val (0), gradient_clip_algorithm ('norm') and
    track_grad_norm (-1), validated: ValueError for what is malformed, NotImplementedError for value clipping."""
    accum = getattr(option, 'accumulate_grad_batches', 1)
    if isinstance(accum, bool) or not isinstance(accum, int):
        if not (isinstance(accum, float) and accum.is_integer()):
            raise ValueError('accumulate_grad_batches = %r: an integer >= 1 is expected (per-epoch schedules -- a dict -- are not supported)'
                             % (_plain(accum),))
        accum = int(accum)
    if accum < 1:
        raise ValueError('accumulate_grad_batches = %r: an integer >= 1 is expected' % (accum,))
    clip = getattr(option, 'gradient_clip_val', 0)
    if isinstance(clip, bool) or not isinstance(clip, (int, float)) or not clip >= 0:
        raise ValueError('gradient_clip_val = %r: a number >= 0 is expected (0 = no clipping)' % (_plain(clip),))
    algorithm = getattr(option, 'gradient_clip_algorithm', 'norm')
    if algorithm == 'value':
        raise NotImplementedError("gradient_clip_algorithm = 'value' is not implemented: only 'norm' (the global 2-norm) is")
    if algorithm != 'norm':
        raise ValueError("gradient_clip_algorithm = %r: 'norm' is expected" % (_plain(algorithm),))
    track = getattr(option, 'track_grad_norm', -1)
    if isinstance(track, bool) or track not in (-1, 2):
        raise ValueError('track_grad_norm = %r: -1 (off) or 2 (the 2-norm) is expected' % (_plain(track),))
    return Knobs(accum, float(clip), track == 2)


def _plain(value):
    return vars(value) if hasattr(value, '__dict__') else value            # (config.Option wraps a JSON dict)


class Record(collections.namedtuple('Record', 'name attr names counter masked ckpt hyper launch launch_dev launch_ctl')):
    """attr: where the state lives; names: its checkpointed arenas; counter: Adam's bias-correction step count; masked: SGD's 'live' arena;
    ckpt: optimizer_states[0]['kind']; hyper: the fixed hyper-parameters as selectors.optimizer_selector gives torch's (model_selector.py:34-38);
    launch / launch_dev: the fused step with its changing scalars as kernel arguments / in device memory (the form a captured graph replays);
    launch_ctl: the step behind the gradient control record (ops.GRAD_CTL_FLOATS; group_step).  Under accumulation the state also holds
    'acc', the arena the micro-steps' gradients are summed in: created with the state, part of arenas() and key(), never checkpointed."""
    __slots__ = ()

    def state(self, model):
        """The state dict (None before the first step)."""
        return getattr(model, self.attr)

    def new_state(self, tensors, step):
        st = dict(zip(self.names, tensors))
        st.update({'step': step} if self.counter else {'kind': self.name})
        return st

    def arenas(self, model):
        """The device tensors of the state: what a captured step bakes in of the optimiser."""
        st = self.state(model) or {}
        return [st[k] for k in self.names + ('live',) * self.masked + ('acc',) if st.get(k) is not None]

    def key(self, model):
        """The capture-key component: the kind and the arenas' addresses (none before they exist)."""
        return (self.name,) + tuple(t.data_ptr() for t in self.arenas(model))

    def counter_of(self, model):
        """Adam's step count, else None.  A capture only RECORDS its step, so the count is put back afterwards (set_counter)."""
        return (self.state(model) or {}).get('step')

    def set_counter(self, model, value):
        if value is not None:
            self.state(model)['step'] = value

    def step(self, model, flat_g, dead, hyper, lr, gscale):
        """One fused step over the flat arenas.  hyper: the slot write_hyper fills (graph capture), else the scalars travel as kernel
        arguments.  dead: the arena ranges of the parameters backward() left without a gradient (gather scheme only; SGD needs them)."""
        st = self.ready(model, flat_g)
        if self.counter:
            st['step'] += 1
        # (without a mask -- RMSprop -- a parameter without a gradient has a zero one in the arena: no update, state stays 0)
        kw = {'live': _live_mask(st, flat_g, dead)} if self.masked else {}
        tensors = [model.flat_parameters(), flat_g] + [st[k] for k in self.names]
        if hyper is not None:
            self.launch_dev(*tensors, hyper, *self.hyper, gscale, **kw)
        else:
            self.launch(*tensors, *((st['step'], lr) if self.counter else (lr,)), *self.hyper, gscale, **kw)

    def ready(self, model, flat_g, accumulate=False):
        """The state dict, created zero-filled on the gradient arena's device if need be (with the accumulation arena when asked)."""
        st, first = self.state(model), self.names[0]
        if st is None or st.get('kind', self.name) != self.name or st.get(first) is None or st[first].device != flat_g.device:
            st = self.new_state([torch.zeros_like(flat_g) for _ in self.names], 0)
            setattr(model, self.attr, st)
        if accumulate and (st.get('acc') is None or st['acc'].device != flat_g.device):
            st['acc'] = torch.zeros_like(flat_g)
        return st

    def group_step(self, model, flat_g, dead, ctl, knobs, world, micro, reducer=None, capturing=False):
        """One micro-step behind the control record `ctl`, which write_hyper has filled (before a replay when `capturing`): fold the
        gradient into the accumulation arena (knobs.accum > 1), and where the micro-step ends its group -- micro = (first, apply) as the
        host knows them; a capture records everything and the kernels decide by ctl[apply] -- the all-reduce of the accumulated sum, the
        norm (in the fold's own pass on a single process), ops.grad_finish and the optimiser.  Returns the device scalar the norm is left
        in (None where nothing was launched for it)."""
        first, apply = micro
        st = self.ready(model, flat_g, knobs.accum > 1)
        src, fused = flat_g, False
        if knobs.accum > 1:
            src, fused = st['acc'], reducer is None
            ops.grad_fold(src, flat_g, ctl, partials=fused)
            # SGD: dead for the update = without a gradient in EVERY micro-step of the group
            st['group_dead'] = set(dead) if first or st.get('group_dead') is None else st['group_dead'] & set(dead)
            dead = st['group_dead']
        if not apply and not capturing:
            return None
        if reducer is not None and knobs.accum > 1:
            reducer.reduce_all(src)
        if not fused:
            ops.grad_sumsq(src)
        ops.grad_finish(src.numel(), ctl, 1.0 / (knobs.accum * world), knobs.clip)
        kw = {'live': _live_mask(st, flat_g, dead)} if self.masked else {}
        self.launch_ctl(model.flat_parameters(), src, *[st[k] for k in self.names], ctl, *self.hyper, **kw)
        return ctl[ops.GRAD_CTL_NORM]

    def write_hyper(self, model, slot, lr, micro=None):
        """Before a replay: what changes between steps goes into the slot.  Adam advances its counter and writes ops.adam_hyper's two
        floats; for the others the rate is the only such scalar.  micro = (first, apply): the slot is a gradient control record and gets
        the two flags as well; Adam's counter then advances only where the optimiser runs."""
        values = (lr,)
        if self.counter:
            st = self.state(model)
            if micro is None or micro[1]:
                st['step'] += 1
            values = ops.adam_hyper(max(st['step'], 1), lr, *self.hyper[:2])
        if micro is not None:
            values = (tuple(values) + (0.0,))[:2] + (float(bool(micro[0])), float(bool(micro[1])))
        for i, x in enumerate(values):
            slot[i:i + 1].fill_(float(x))                  # (scalars travel as kernel arguments: no host buffer the next step could overwrite)


TABLE = {r.name: r for r in (
    Record('adam', '_adam', ('m', 'v'), True, False, 'flat_adam', (0.9, 0.999, 1e-5), ops.adam_step, ops.adam_step_hyper, ops.adam_step_ctl),
    Record('sgd', '_optim', ('buf',), False, True, 'flat_sgd', (0.9, 2e-4), ops.sgd_step, ops.sgd_step_lr, ops.sgd_step_ctl),
    Record('rmsprop', '_optim', ('sq',), False, False, 'flat_rmsprop', (0.99, 1e-5), ops.rmsprop_step, ops.rmsprop_step_lr,
           ops.rmsprop_step_ctl))}


def _live_mask(st, flat_g, dead):
    # SGD: torch skips a parameter whose .grad is None, while weight decay over its zero-filled arena view would shrink it every step.
    # The kernel gets a byte mask of the live elements, rebuilt only when the set of such parameters changes -- it is a property of
    # the network, so the warm-up steps settle it and a capture bakes in its address (key, arenas).  None: every element is live.
    dead = tuple(sorted(set(dead)))                        # (never None here: train_step refuses SGD without the gather scheme)
    if st.get('dead') != dead or (dead and (st.get('live') is None or st['live'].device != flat_g.device)):
        live = None
        if dead:
            live = torch.ones(flat_g.numel(), dtype=torch.uint8, device=flat_g.device)
            for off, numel in dead:
                live[off:off + numel] = 0
        st['dead'], st['live'] = dead, live
    return st['live']


def of(option):
    """The record of option.optim; an unknown name, which train_step refuses, checkpoints as Adam."""
    return TABLE.get(getattr(option, 'optim', 'adam'), TABLE['adam'])


def to_checkpoint(model, option):
    """optimizer_states[0]: the kind, Adam's counter, the arenas on the CPU (None before the first step).  A model that only exposes
    `_adam` is written as 'flat_adam'."""
    rec = of(option) if hasattr(model, of(option).attr) else TABLE['adam']
    st = getattr(model, rec.attr, None) or {}
    if st.get('kind', rec.name) != rec.name:
        raise ValueError("the model holds %r optimiser state while option.optim is %r" % (st.get('kind'), rec.name))
    out = {'kind': rec.ckpt, 'step': int(st.get('step', 0))} if rec.counter else {'kind': rec.ckpt}
    out.update((k, st[k].detach().cpu() if st.get(k) is not None else None) for k in rec.names)
    return out


def from_checkpoint(model, saved):
    """Put optimizer_states[0] back on the model's device; a record from before the first step (None arenas) restores nothing."""
    rec = next((r for r in TABLE.values() if r.ckpt == saved.get('kind')), None)
    if rec is not None and saved.get(rec.names[0]) is not None:
        dev = model.flat_parameters().device
        setattr(model, rec.attr, rec.new_state([saved[k].to(dev) for k in rec.names], int(saved.get('step', 0))))
