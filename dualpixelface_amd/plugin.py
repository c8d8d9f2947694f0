"""``STEREODPNET``: the class the reference's ``model_selector`` instantiates
(src/model/model_selector.py:11-15 -> src/model/stereodpnet/mainmodel.py:21), with the same methods PL / main.py call
(mainmodel.py:67-177) plus an MI355X-native ``train_step`` (flat-arena gradients, fused Adam / SGD / RMSprop step as ``option.optim`` selects, optional RCCL
all-reduce).
"""
import contextlib
import os
import sys
import traceback
import warnings

import torch

from . import confidence, normal_refine, ops, optim, postprocess, reconstruct, refocus, shading
from .losses import loss_selector
from .selectors import metric_selector, optimizer_selector, scheduler_selector
from .dpnet import DPNetCore
from .nnet import NNetCore
from .psmnet import PSMNetCore
from .stereonet import StereoNetCore
from .stereodpnet import StereoDPNetCore, two_stream_grad_warning_off


class _PluginHooks(object):
    """The methods PL / main.py call on a model plugin (mainmodel.py:67-177), shared by every model family of the build."""

    def __init__(self, option):
        super(_PluginHooks, self).__init__(option)         # the model family's core (core.ArenaModule)
        self.loss_model = loss_selector(option)
        self.metric_model = metric_selector(option)
        confidence.check_model(option)                     # (block on: a model without disparity hypotheses is refused by name)
        self.confidence_table = None                       # the sparsification table of a validation pass (confidence.report), on the device
        shading.check_model(option)                        # (block on with normals "predicted": a model without a normal head is refused by name)
        self.shading_table = None                          # the sums of a validation pass (shading.report), on the device
        self._adam = None                                  # the fused optimiser's state, kept by optim.py: 'adam' here,
        self._optim = None                                 # 'sgd' / 'rmsprop' here

    # ---- reference surface -------------------------------------------------------------------------------
    def forward(self, batch):
        return self._behind_replays(lambda: self._forward(batch))

    def _forward(self, batch):
        results = self.network(batch)
        self.last_taps = results.pop('_taps')
        # (a batch without 'abvalue': the loss fits (a, b) and needs depth and inverse depth, not 'disp')
        fitted = self.loss_model.least_square(batch) and 'depth' in batch and 'idepth' in batch
        if not self.training and confidence.active(self.option):    # estimate -> filter -> fit -> refine -> surface: all see the estimator's map
            confidence.apply(self.option, results, batch)
        if not self.training and postprocess.active(self.option):   # the fit and the metric hooks below see the filtered map
            postprocess.apply(self.option, results, batch, guide=self._views(batch)[0])
        if self.training and ('disp' in batch or fitted or self.loss_model.label_free()):     # (label-free: the two views are enough)
            results.update(self.loss_model.forward(results, batch, target_type=self._target_type()))
        elif not self.training and 'idepth' in batch and 'abvalue' not in batch and results.get('pred_depth') is not None:
            results['abvalue'] = ops.affine_fit(results['pred_depth'], batch['idepth'])       # what metrics.absolute_dp converts with
        if not self.training and normal_refine.active(self.option):  # filter -> fit -> refine -> surface: metrics and mesh see the refined map
            normal_refine.apply(self.option, results, batch)
        if not self.training and reconstruct.active(self.option):   # the surface of the filtered map, placed with the fitted (a, b)
            reconstruct.apply(self.option, results, confidence.gated(self.option, results, batch, 'reconstruct'), guide=self._views(batch)[0])
        if not self.training and shading.active(self.option):       # ... -> surface -> shade: the lighting under the final normals
            shading.apply(self.option, results, batch, guide=self._views(batch)[0])
        if not self.training and refocus.active(self.option):       # ... -> shade -> refocus: the view (or the relit one) through a virtual aperture
            refocus.apply(self.option, results, batch, guide=self._views(batch)[0])
        results.pop('_heads', None)                         # (the heads' logits, for the loss hook only: losses.UNIMODALLoss)
        return results

    def _target_type(self):
        return getattr(self.option.model, 'target_type', 'disp')

    def _loaders(self, train, batch_size, shuffle):
        import torch.utils.data as torch_data
        from dataloader.loader_selector import loader_selector     # this repo's (or a user's) data package, CWD-relative
        dataset = loader_selector(self.option, train)
        if hasattr(dataset, 'produce'):                              # device-side FaceDP path: decode threads + preprocessing kernels
            from .facedp import FaceDPBatcher
            return FaceDPBatcher(dataset, batch_size, shuffle=shuffle, workers=self.option.workers, drop_last=False)
        return torch_data.DataLoader(dataset, batch_size=batch_size, shuffle=shuffle,
                                     num_workers=self.option.workers, drop_last=False, pin_memory=self.option.pin_memory)

    def train_dataloader(self):
        return self._loaders(True, self.option.batch_size, True)

    def val_dataloader(self):
        return self._loaders(False, 1, False)

    def test_dataloader(self):
        return self._loaders(False, self.option.batch_size, False)

    def training_step(self, batch, batch_idx):
        results = self.forward(batch)
        losses = {}
        for key, val in results.items():
            if key != 'final_loss' and 'loss' in key:
                losses[key] = val
                self.log(key, val, prog_bar=True)
        return {'loss': results['final_loss'], 'log': losses}

    def validation_step(self, batch, batch_idx):
        results = self.forward(batch)
        if 'depth' in batch:
            self.metric_model.forward(results, confidence.gated(self.option, results, batch, 'metrics'), target_type=self._target_type())
        self.confidence_table = confidence.accumulate(self.option, results, batch, self.confidence_table, target_type=self._target_type())
        self.shading_table = shading.accumulate(self.option, results, self.shading_table)
        return results

    def validation_epoch_end(self, outputs):
        self.metric_model.viewer()

    def test_step(self, batch, batch_idx):
        return self.validation_step(batch, batch_idx)

    def test_epoch_end(self, outputs):
        if self.option.mode == 'test':
            self.metric_model.viewer()

    def configure_optimizers(self):
        optimizer = optimizer_selector(self.parameters(), self.option)
        scheduler = scheduler_selector(optimizer, self.option)
        return [optimizer], ([scheduler] if scheduler is not None else [])

    # ---- MI355X-native step ------------------------------------------------------------------------------
    def _grad_pairs(self):
        """[(parameter, its view in the flat gradient arena)] in layout order (cached per arena)."""
        fg = self.flat_gradients(zero=False)
        cache = getattr(self, '_pairs_cache', None)
        if cache is None or cache[0] is not fg:
            pd = dict(self.named_parameters())
            cache = (fg, [(pd[name], fg[off:off + numel].view(shape)) for name, off, numel, shape in self._layout])
            self._pairs_cache = cache
        return cache[1]

    def train_step(self, batch, reducer=None, lr=None, last_in_epoch=False):
        """forward + loss + backward + (gradient all-reduce) + the fused step of option.optim (Adam, SGD with momentum, RMSprop, configured as
        selectors.optimizer_selector configures torch's); returns the results dict.

        With option.accumulate_grad_batches = N > 1 a call is a MICRO-step: its gradient is added to the group's, the model counts its
        position inside the group, and the optimiser runs on the N-th call with (sum of the group) / (N * world_size) -- or earlier on the
        call that passes last_in_epoch=True, which ends a short group (the divisor stays N).  Ranks exchange the accumulated sum once, on
        that call.  option.gradient_clip_val = c > 0 scales that gradient by min(1, c / (its global 2-norm + 1e-6)); then, or with
        option.track_grad_norm = 2, a call on which the optimiser ran returns the norm before clipping as results['grad_norm'] (a device
        scalar).  All of it stays on the device (optim.Record.group_step, csrc/grad_ctl.hip), so such steps are captured like any other.

        Single-process steps on a fixed batch shape are captured into ONE HIP graph after two eager warm-up steps and replayed from then on
        (option.step_graph / DPF_STEP_GRAPH, default on): the ~2 400 kernel launches of a step leave the host once, so the launch gaps between
        the many short kernels disappear.  The C ABI never allocates or synchronises, which is what makes the step capturable."""
        if self.option.optim not in optim.TABLE:
            raise NotImplementedError('optimizer is not defined, please check your optimizer configuration !')
        if self.option.optim == 'sgd' and not getattr(self, 'gather_grads', True):
            raise NotImplementedError("optim 'sgd' needs the gather scheme (model.gather_grads): gradients accumulated into arena views do "
                                      "not tell an unused parameter, which SGD must skip, from a zero gradient")
        knobs = optim.knobs(self.option)
        if not knobs.on:
            return self._one_step(batch, reducer, lr)
        if not getattr(self, 'gather_grads', True):
            raise NotImplementedError('accumulate_grad_batches, gradient_clip_val and track_grad_norm need the gather scheme '
                                      '(model.gather_grads): they work on the gathered gradient arena')
        pos = getattr(self, '_group_pos', 0)                               # micro-steps of the current group already taken
        first, apply = pos == 0, pos + 1 >= knobs.accum or bool(last_in_epoch)
        self._micro = (first, apply)
        try:
            results = self._one_step(batch, reducer, lr)
        finally:
            self._micro = None
        self._group_pos = 0 if apply else pos + 1
        if not (apply and knobs.reports):
            results.pop('grad_norm', None)
        return results

    def _one_step(self, batch, reducer, lr):
        # (eager when a per-launch profile is being recorded -- ops.PROFILE -- or gradients are exchanged between ranks)
        if reducer is None and ops.PROFILE is None and _graph_enabled(self) and all(v.is_cuda for v in batch.values() if torch.is_tensor(v)):
            return self._graph_step(batch, lr)
        return self._eager_step(batch, reducer, lr)

    def _lr(self, lr):
        return float(lr if lr is not None else self.option.init_lr)

    # ---- the step as one HIP graph ---------------------------------------------------------------------
    def _graph_step(self, batch, lr):
        self.train()                                       # (a replay runs no Python: the mode flag must not depend on it)
        tensors = {k: v for k, v in batch.items() if torch.is_tensor(v)}
        st = self._graph_lookup(self._graph_key(tensors))
        if st.get('failed'):
            return self._eager_step(batch, None, lr)
        st['calls'] += 1
        device = self.flat_gradients(zero=False).device
        # The step lives on its OWN stream, warm-up included: autograd's gradient-accumulation nodes remember the stream they were created
        # on, and a capture cannot make the default stream wait for the capturing one.
        ss = getattr(self, '_step_stream', None)
        if ss is None or ss.device != device:
            ss = self._step_stream = ops.shared_stream(device, 'step')             # one per process, not per model: ops.shared_stream
        if st['calls'] <= 2 or not optim.of(self.option).state(self):
            # warm-up: lazily created streams, scratch buffers, sampler tables, kernel attributes
            with _on_stream(ss) as cur:
                res = self._eager_step(batch, None, lr)
            for v in (res.values() if cur is not None else ()):
                if torch.is_tensor(v):
                    v.record_stream(cur)
            return _detached(res)
        if st['graph'] is None and not self._graph_capture(st, ss, tensors, batch, lr):
            return self._eager_step(batch, None, lr)
        return self._graph_replay(st, ss, tensors, lr)

    def _graph_key(self, tensors):
        """Everything a captured graph has baked in: shapes, the kernel-path switches, the arenas' addresses (a device move re-creates them)."""
        return tuple((k, tuple(v.shape), v.dtype) for k, v in sorted(tensors.items())) + (
            bool(ops.deterministic()), ops.CONV_OPERANDS_BF16, ops.f32_matrix_path(), ops.WGRAD_ASYNC) + self._capture_key() + (
            self.flat_parameters().data_ptr(), self.flat_gradients(zero=False).data_ptr(), optim.of(self.option).key(self),
            self.stat_exchange is None) + ((optim.knobs(self.option),) if getattr(self, '_micro', None) else ())

    def _graph_lookup(self, key):
        """The graph state of `key`, new if need be.  A few states are kept (most recently used last): the last, partial batch of an epoch
        has its own key and must not throw the main shape's graph away."""
        states = self.__dict__.setdefault('_graph_states', [])
        st = next((g for g in states if g['key'] == key), None)
        if st is None:
            st = {'key': key, 'calls': 0, 'graph': None}
        else:
            states.remove(st)
        states.append(st)
        del states[:-3]
        self._graph_state = st
        return st

    def _graph_capture(self, st, ss, tensors, batch, lr):
        """Record one step into st['graph']; returns whether the state now holds a graph.  After a refused capture (an unsupported call
        inside) the state is marked `failed`, everything the recording moved is put back, and the caller stays eager."""
        # static inputs (the caller's tensors are copied in before every replay), the hyper-parameter slot, then the capture itself
        st['inputs'] = {k: v.clone() for k, v in tensors.items()}
        st['extra'] = {k: v for k, v in batch.items() if not torch.is_tensor(v)}
        st['hyper'] = torch.zeros(ops.GRAD_CTL_FLOATS if getattr(self, '_micro', None) else 2, dtype=torch.float32, device=ss.device)
        rec = optim.of(self.option)
        counts_before = dict(self._pending_counts)
        step_before = rec.counter_of(self)                 # (Adam's bias-correction counter; the other optimisers have none)
        self._flush_counts()
        baked = self._baked_buffers()                      # (before AND after: a buffer replaced mid-capture was baked in as well)
        graph = torch.cuda.CUDAGraph()
        try:
            torch.cuda.synchronize()
            ops.reset_zero_arenas()
            # (thread-local error mode: the data path's worker threads -- facedp.FaceDPBatcher decodes and preprocesses the next batch on
            # the GPU meanwhile -- make allocator and copy calls of their own, which a global-mode capture takes for violations)
            with torch.cuda.graph(graph, stream=ss, capture_error_mode='thread_local'):
                st['results'] = self._captured_step(st, lr)
            st['counts'] = dict(self._pending_counts)                # BatchNorm call counters one step adds (host-side bookkeeping)
            self._pending_counts = {}
            rec.set_counter(self, step_before)                       # the capture only RECORDED the step: nothing ran
            st['owned'] = baked + self._baked_buffers()              # released when the LRU (_graph_lookup) drops the state
            st['graph'] = graph
            return True
        except Exception as e:                                       # capture refused: stay eager, say so once
            warnings.warn('train_step: HIP graph capture failed (%s: %s); continuing with eager launches' % (type(e).__name__, e))
            st['failed'] = True
            self._pending_counts = counts_before
            torch.cuda.synchronize()
            # the aborted capture only RECORDED its work: the clearing fill of the zero arenas never ran although their cursors moved
            # on (the warm-up steps' slots are still dirty), and the Adam step counter may have been advanced
            ops.reset_zero_arenas()
            rec.set_counter(self, step_before)
            return False

    def _captured_step(self, st, lr):
        try:
            cap_batch = dict(st['extra'])
            cap_batch.update(st['inputs'])
            return _detached(self._eager_step(cap_batch, None, lr, hyper=st['hyper']))
        except BaseException as e:                         # (ending an invalidated capture has crashed the process before the error could surface)
            sys.stderr.write('train_step: exception inside the graph capture: %r\n%s\n' % (e, traceback.format_exc()))
            sys.stderr.flush()
            raise

    def _graph_replay(self, st, ss, tensors, lr):
        # The replay runs on the dedicated stream, bracketed by explicit event waits in both directions.  Launched into the caller's stream
        # -- the legacy default stream in a plain script -- kernels the caller enqueued right after the replay were observed to start before
        # the graph had finished (bench.py --wgrad-inline: eager steps behind two replays read parameters the replay was still writing: GPU
        # memory faults and hangs in 2 of 5 runs; none in 12 runs with this ordering).
        with _on_stream(ss):
            for k, v in tensors.items():
                if v.data_ptr() != st['inputs'][k].data_ptr():
                    st['inputs'][k].copy_(v, non_blocking=True)
                    v.record_stream(ss)
            optim.of(self.option).write_hyper(self, st['hyper'], self._lr(lr), getattr(self, '_micro', None))
            st['graph'].replay()
        for name, n in st['counts'].items():
            self._pending_counts[name] = self._pending_counts.get(name, 0) + n
        return dict(st['results'])                         # (a fresh dict; the tensors are the graph's static buffers, valid until the next step)

    def _baked_buffers(self):
        """The device tensors whose addresses a capture of the step bakes in, besides the state's own inputs, hyper-parameter slot and
        results.  A graph state holds them for as long as it can replay, so none of them is ever freed and handed to another tensor that
        the next replay would then overwrite:
          * ops.workspace_buffers(): the scratch slabs and pre-zeroed arenas of every stream the step runs on (step, second feature pass,
            weight-gradient side stream).  A later call that needs more room replaces them -- an eager step or a validation at a larger
            shape, on the replays' own stream (_behind_replays);
          * the model's lazily built shape constants (_shape_constants): StereoDPNet's sampler tables (only added to, but re-created
            by a device move) and NNet's cost-level volume (replaced whenever the batch shape changes);
          * the parameter, gradient and optimiser arenas (SGD's liveness mask among them) and the BatchNorm buffers: updated in place, and
            the arenas' addresses are part of the key -- held, a key match can never mean a new tensor at a recycled address.
        Not buffers: `_pairs_cache` (views of the gradient arena), the shared streams (`ops._wgrad_side`, the feature stream); the
        normal head's lazily registered `grid` is read by no kernel and only ever written in place."""
        found = ops.workspace_buffers() + list(self.buffers()) + [self.flat_parameters(), self.flat_gradients(zero=False)]
        return found + optim.of(self.option).arenas(self) + self._shape_constants()

    def _behind_replays(self, fn):
        """Once a train step of this model replays as a HIP graph, everything the model launches one by one (an eager step, forward,
        validation) runs on the SAME stream as the replays, bracketed by event waits against the caller's stream.

        Why (tools/debug/graph_eager_alternation.py): with eager launches on another stream, ordered against the replay
        only through `caller.wait_stream(step stream)` -- an event recorded right behind hipGraphLaunch -- a headline-size replay followed by
        this model's eager forward ended in a GPU memory access fault in about one run of three (100 alternations each); with launch
        blocking, with a host wait, or with the eager work on the replay's own stream: none (0 of 80 / 12 / 14 runs).  4 000 trivial
        kernels behind each replay on the other stream never faulted either: what races is the model's own state (parameters, running
        statistics, cached tables) between the graph's tail and the eager kernels, i.e. the cross-stream event does not cover the whole
        graph on this runtime (ROCm 7.0.2 / PyTorch 2.10).  Same-stream order does not depend on it."""
        ss = getattr(self, '_step_stream', None)
        if ss is None or not any(g.get('graph') is not None for g in getattr(self, '_graph_states', ())):
            return fn()
        with _on_stream(ss) as cur:
            out = fn()
        if cur is None:                                    # (already on the step stream)
            return out
        for v in (out.values() if isinstance(out, dict) else ()):
            if torch.is_tensor(v) and v.is_cuda:
                v.record_stream(cur)
        return out

    def _eager_step(self, batch, reducer=None, lr=None, hyper=None):
        if hyper is None and torch.cuda.is_available() and not torch.cuda.is_current_stream_capturing():
            return self._behind_replays(lambda: self._eager_step_body(batch, reducer, lr, None))
        return self._eager_step_body(batch, reducer, lr, hyper)

    def _eager_step_body(self, batch, reducer=None, lr=None, hyper=None):
        self.train()
        micro = getattr(self, '_micro', None)
        if micro is not None:
            return self._micro_step_body(batch, reducer, lr, hyper, micro)
        if getattr(self, 'gather_grads', True):
            results, flat_g, dead = self._grads_gathered(batch, reducer)
        else:
            results, flat_g, dead = self._grads_into_views(batch, reducer)
        gscale = 1.0 / reducer.world_size if reducer is not None else 1.0
        optim.of(self.option).step(self, flat_g, dead, hyper, self._lr(lr), gscale)
        return results

    def _micro_step_body(self, batch, reducer, lr, hyper, micro):
        """The step with a gradient knob on (train_step).  Everything after the gather is launched on the current stream in one order:
        fold, (all-reduce), norm, finish, optimiser.  Under accumulation the ranks exchange the accumulated arena on the group's last
        micro-step only, unstaged; at N = 1 the staged bucket exchange during backward stays."""
        knobs, rec = optim.knobs(self.option), optim.of(self.option)
        results, flat_g, dead = self._grads_gathered(batch, reducer if knobs.accum == 1 else None)
        ctl = hyper
        if ctl is None:                                    # launched one by one: the model's own record, filled here
            ctl = getattr(self, '_grad_ctl', None)
            if ctl is None or ctl.device != flat_g.device:
                ctl = self._grad_ctl = torch.zeros(ops.GRAD_CTL_FLOATS, dtype=torch.float32, device=flat_g.device)
            rec.ready(self, flat_g, knobs.accum > 1)
            rec.write_hyper(self, ctl, self._lr(lr), micro)
        world = reducer.world_size if reducer is not None else 1
        norm = rec.group_step(self, flat_g, dead, ctl, knobs, world, micro, reducer, capturing=hyper is not None)
        if norm is not None:
            results['grad_norm'] = norm.clone()            # (the record is overwritten by the next optimiser step)
        return results

    def _grads_gathered(self, batch, reducer):
        """forward + backward under the gather scheme; returns (results, gradient arena, arena ranges of the parameters backward() left
        without a gradient).

        Gradients are produced as fresh tensors (autograd hands them over without an accumulate kernel when .grad is None) and gathered
        into the flat arena by one multi-tensor copy; the 14.7 MB all-reduce then runs once over the arena.  The alternative
        (_grads_into_views) accumulates into arena views (one add kernel per parameter, ~300 per step) and overlaps bucketed all-reduces
        with the backward pass through hooks -- an overlap worth < 0.1 % of a 400 ms step."""
        flat_g = self.flat_gradients(zero=False)
        pairs = self._grad_pairs()
        dead = []
        for p, _ in pairs:
            p.grad = None
        ops.wgrad_async_begin([p for p, _ in pairs])
        staged = reducer is not None and getattr(reducer, 'collectives', reducer.world_size > 1) and getattr(self, 'stage_grads', True)
        if staged:
            # Data-parallel: the network fires self._grad_stage(bucket) from tensor hooks at its bucket boundaries (normal head done;
            # aggregation + cost volume done); that bucket is gathered and its all-reduce enqueued while the backward pass continues.
            reducer.stage_begin()
            main = torch.cuda.current_stream() if flat_g.is_cuda else None

            def on_stage(name):
                # `name`: 'aggregation' | 'normal' (StereoDPNetCore._network).  A reducer cut differently has no bucket of that name:
                # nothing is staged then and stage_finish exchanges everything after backward().
                bi = reducer.stage_of.get(name) if hasattr(reducer, 'stage_of') else None
                if bi is None:
                    return
                # The hook may fire on another stream than the step's (the second feature pass has its own): the bucket's gradients
                # were produced on the main stream (and the weight-gradient side stream), and Adam will read the arena there -- so the
                # gather and the collective are enqueued on the main stream, after whatever the hook's stream has produced so far.
                cur = torch.cuda.current_stream() if main is not None else None
                if main is not None and cur != main:
                    main.wait_stream(cur)
                with (torch.cuda.stream(main) if main is not None else contextlib.nullcontext()):
                    _attach_deferred(ops.wgrad_async_take(lambda q: reducer.bucket_of(q) == bi))
                    _gather([(p, v) for p, v in pairs if reducer.bucket_of(p) == bi], dead)
                    reducer.stage_launch(bi)
            self._grad_stage = on_stage
        self._two_streams_ok = True                # see StereoDPNetCore._network
        try:
            with two_stream_grad_warning_off():
                results = self.forward(batch)
                results['final_loss'].backward()
        finally:
            self._grad_stage = None
            self._two_streams_ok = False
        _attach_deferred(ops.wgrad_async_finish())
        _gather(pairs, dead)
        if staged:
            reducer.stage_finish()
        elif reducer is not None:
            reducer.reduce_all()
        return results, flat_g, dead

    def _grads_into_views(self, batch, reducer):
        """forward + backward accumulating into arena views, bucketed all-reduces overlapping through the reducer's hooks; returns
        (results, gradient arena, None: a parameter without a gradient cannot be told from one with a zero gradient here)."""
        flat_g = self.flat_gradients(zero=True)
        if reducer is not None:
            reducer.begin()
        results = self.forward(batch)
        results['final_loss'].backward()
        if reducer is not None:
            reducer.finish()
        return results, flat_g, None


@contextlib.contextmanager
def _on_stream(ss):
    """Run the body on the stream `ss` between event waits: `ss` waits for the caller's current stream, and the caller's stream waits for
    `ss` afterwards.  Yields the caller's stream, for a `record_stream` of what the body hands back -- or None when the caller already is on
    `ss` and nothing is done."""
    cur = torch.cuda.current_stream(ss.device)
    if cur == ss:
        yield None
        return
    ss.wait_stream(cur)
    with torch.cuda.stream(ss):
        yield cur
    cur.wait_stream(ss)


def _detached(res):
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in res.items()}


def _graph_enabled(model):
    env = os.environ.get('DPF_STEP_GRAPH')
    if env is not None:
        return env != '0'
    return bool(getattr(model.option, 'step_graph', True))


def _gather(sel, dead):
    """Copy the gradients of the selected (parameter, arena view) pairs into the arena; afterwards .grad IS the view.  A parameter
    without a gradient gets a zero view, and its arena range is appended to `dead`."""
    views, grads = [], []
    for p, v in sel:
        if p.grad is v:
            continue
        if p.grad is None:
            v.zero_()
            dead.append((v.storage_offset(), v.numel()))
        else:
            views.append(v)
            grads.append(p.grad)
    if views:
        torch._foreach_copy_(views, grads)
    for p, v in sel:
        p.grad = v


def _attach_deferred(pairs):
    """Hand the side-stream weight gradients to their parameters.  A weight used twice per step (the shared feature extractor: left and
    right pass) gets two gradients: the second is added in place by ONE multi-tensor launch for all such weights instead of an add kernel
    (and a fresh tensor) per weight."""
    dst, src, busy = [], [], set()
    for p, g in pairs:
        if p.grad is None:
            p.grad = g
            continue
        if id(p) in busy:                                  # a third gradient for the same weight: finish the pending adds first
            torch._foreach_add_(dst, src)
            dst, src, busy = [], [], set()
        dst.append(p.grad)
        src.append(g)
        busy.add(id(p))
    if dst:
        torch._foreach_add_(dst, src)


class STEREODPNET(_PluginHooks, StereoDPNetCore):
    """src/model/stereodpnet/mainmodel.py::STEREODPNET (mainmodel.py:21-177)."""


class _NoValidation(object):
    """The validation hooks are no-ops in the reference (psmnet/mainmodel.py:143-149, dpnet/mainmodel.py:236-245)."""

    def validation_step(self, batch, batch_idx):
        return None

    def validation_epoch_end(self, outputs):
        return None


class PSMNET(_NoValidation, _PluginHooks, PSMNetCore):
    """src/model/psmnet/mainmodel.py::PSMNET."""


class NNET(_PluginHooks, NNetCore):
    """src/model/nnet/mainmodel.py::NNET (mainmodel.py:31-240)."""


class STEREONET(_PluginHooks, StereoNetCore):
    """src/model/stereonet/mainmodel.py::STEREONET (mainmodel.py:30-220)."""


class DPNET(_NoValidation, _PluginHooks, DPNetCore):
    """src/model/dpnet/mainmodel.py::DPNET (mainmodel.py:29-270); test_step runs the metric hooks (mainmodel.py:247-251)."""

    def test_step(self, batch, batch_idx):
        return _PluginHooks.validation_step(self, batch, batch_idx)
