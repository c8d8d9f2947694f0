"""What no model of the plugin owns: the flat parameter arena, the deferred BatchNorm call counters and the conv / BatchNorm primitives.

A model is not a module tree of torch layers: a ``Spec`` lists its parameters and buffers under the reference's state_dict names,
``ArenaModule`` lays the parameters out in ONE flat HBM arena (one fused optimiser launch, one RCCL all-reduce over the matching flat
gradient arena), and the forward pass is a straight-line program over the HIP operator layer (ops.py).  A model family subclasses
``ArenaModule``, names its spec in ``_spec`` and writes ``_network``; ``_views`` gives it the two images in reference order and
``_shape_constants`` tells a captured train step which lazily built device tensors the model bakes in.
"""
import math

import torch
import torch.nn as nn

from . import ops
from .ops import ACT_NONE

try:                                    # optional: neither is installed on the MI355X image
    import pytorch_lightning as pl
    _Base = pl.LightningModule
except Exception:                       # pragma: no cover - depends on the environment
    class _Base(nn.Module):
        """nn.Module with the LightningModule methods the reference's class touches."""

        def save_hyperparameters(self, *a, **k):
            pass

        def log(self, *a, **k):
            pass


class _Node(nn.Module):
    """Anonymous container used to reproduce the reference's dotted state_dict names."""


def _owner(root, dotted):
    """The (created on demand) sub-module that holds the last component of a dotted name, and that component."""
    parts = dotted.split('.')
    mod = root
    for p in parts[:-1]:
        if p not in mod._modules:
            mod.add_module(p, _Node())
        mod = mod._modules[p]
    return mod, parts[-1]


def _attach(root, dotted, tensor, is_param, requires_grad=True):
    mod, leaf = _owner(root, dotted)
    if is_param:
        mod.register_parameter(leaf, nn.Parameter(tensor, requires_grad))
    else:
        mod.register_buffer(leaf, tensor)


class Spec(object):
    """Ordered list of (name, shape, kind, init) for every parameter / buffer of a model.  kind: 'param' (in the arena; init
    ('normal', std) | ('uniform', bound) | ('const', value)), 'buffer' (('const', value)), 'counter' (num_batches_tracked),
    'frozen' (a parameter outside the arena that never trains; init = its values), 'alias' (init = the name it repeats)."""

    def __init__(self):
        self.items = []

    def add(self, name, shape, kind, init):
        self.items.append((name, tuple(shape), kind, init))

    # --- layer helpers (names follow the reference's module tree) ---
    def conv(self, p, cout, cin, ks, bias=None, transpose=False):
        taps = 1
        for k in ks:
            taps *= k
        shape = (cin, cout) + tuple(ks) if transpose else (cout, cin) + tuple(ks)
        self.add(p + '.weight', shape, 'param', ('normal', math.sqrt(2.0 / (taps * cout))))
        if bias is not None:
            self.add(p + '.bias', (cout,), 'param', bias)

    def bn(self, p, c):
        self.add(p + '.weight', (c,), 'param', ('const', 1.0))
        self.add(p + '.bias', (c,), 'param', ('const', 0.0))
        self.add(p + '.running_mean', (c,), 'buffer', ('const', 0.0))
        self.add(p + '.running_var', (c,), 'buffer', ('const', 1.0))
        self.add(p + '.num_batches_tracked', (), 'counter', None)

    def prelu(self, p):
        self.add(p + '.weight', (1,), 'param', ('const', 0.05))

    def convbn2(self, p, cin, cout):
        self.conv(p + '.0', cout, cin, (3, 3))
        self.bn(p + '.1', cout)

    def convbn3(self, p, cin, cout):
        self.conv(p + '.0', cout, cin, (3, 3, 3))
        self.bn(p + '.1', cout)


def geometry_abvalue(batch, what):
    """batch['abvalue'] for a coordinate volume.  A batch without it can still be trained against (losses.py fits (a, b) to the prediction),
    but the volume would have to be built from a fit of a prediction that is made after it: not built."""
    if 'abvalue' not in batch:
        raise NotImplementedError("%s builds its coordinate volume from batch['abvalue'], which this batch does not have (the 'least_square' "
                                  "conversion fits it to the prediction, after the volume)" % what)
    return batch['abvalue'].float()


def reference_key(option):
    """The batch key of the reference view, the one a prediction is aligned to: 'right' under dataset.flip_lr, else 'left'.  (An option
    without a dataset block reads as not flipped.)  ArenaModule._views adds its capture-group rule to this."""
    return 'right' if getattr(getattr(option, 'dataset', None), 'flip_lr', False) else 'left'


def cost_levels(mindisp, maxdisp, level):
    """The quarter-resolution disparity of every cost level (stereodpnet/modules.py:144-145)."""
    step = (maxdisp / 4.0 - mindisp / 4.0) / float(level)
    return [i * step + mindisp / 4.0 for i in range(int(level))]


def set_levels(model, mindisp, maxdisp, level, hypotheses):
    """The disparity geometry of a cost-volume model: `level` cost levels, `hypotheses` soft-argmin values (modules.py:345)."""
    model.mindisp, model.maxdisp, model.level = mindisp, maxdisp, level
    model.costrange = cost_levels(mindisp, maxdisp, level)
    model.disp_values = [i * ((maxdisp - mindisp) / float(hypotheses)) + mindisp for i in range(hypotheses)]


class ArenaModule(_Base):
    """Parameters (flat arena) + the primitives of the straight-line HIP forward; plugin._PluginHooks adds the plugin hooks."""

    _spec = None            # staticmethod(option) -> Spec: every family names its own
    grid_owner = None       # the sub-module whose lazily registered `grid` a checkpoint may carry (load_state_dict)

    def __init__(self, option):
        super(ArenaModule, self).__init__()
        self.save_hyperparameters()
        self.option = option
        self._pending_counts = {}
        self.stat_exchange = None          # distributed.StatExchange -> SyncBatchNorm (see enable_sync_batchnorm)
        # mixed precision: the reference's `precision: 16` is PL autocast (every nn.Conv2d / nn.Conv3d in half precision).  Here 16 / 'bf16'
        # make the dense conv kernels round their operands to bf16 (fp32 accumulation, fp32 tensors; ops.conv_operands); 'bf16-2d' is
        # BASELINE configs[4] read literally: only the 2-D convs, on the stand-alone bf16 kernel (conv_bf16.hip).
        prec = str(getattr(option, 'precision', 32))
        self.bf16_all = prec in ('16', 'bf16')
        self.bf16_2d = prec == 'bf16-2d'
        self._build_parameters(self._spec(option))

    def enable_sync_batchnorm(self, group=None):
        """Training BatchNorm statistics over the global batch, like torch.nn.SyncBatchNorm which the reference switches on for
        accelerator == 'ddp' (config_manager.py:57, main.py:55).  ``group=False`` turns it off again."""
        from .distributed import StatExchange
        self.stat_exchange = None if group is False else StatExchange(group)
        return self

    # ------------------------------------------------------------------ parameters
    def _build_parameters(self, spec):
        g = torch.Generator().manual_seed(torch.initial_seed() % (2 ** 31))
        total = sum(int(torch.Size(shape).numel()) for _, shape, kind, _ in spec.items if kind == 'param')
        flat = torch.zeros(total, dtype=torch.float32)
        self._layout = []            # (name, offset, numel, shape)
        off = 0
        for name, shape, kind, init in spec.items:
            if kind == 'param':
                numel = int(torch.Size(shape).numel())
                view = flat[off:off + numel].view(shape)
                if init[0] == 'normal':
                    view.normal_(0.0, init[1], generator=g)
                elif init[0] == 'uniform':
                    view.uniform_(-init[1], init[1], generator=g)
                else:
                    view.fill_(init[1])
                self._layout.append((name, off, numel, shape))
                _attach(self, name, view, True)
                off += numel
            elif kind == 'buffer':
                _attach(self, name, torch.full(shape, init[1], dtype=torch.float32), False)
            elif kind == 'counter':
                _attach(self, name, torch.zeros((), dtype=torch.long), False)
            elif kind == 'frozen':
                _attach(self, name, torch.tensor(init, dtype=torch.float32).view(shape), True, requires_grad=False)
        # alias keys: the same Parameter object registered under a second name
        pd = dict(self.named_parameters())
        for name, shape, kind, init in spec.items:
            if kind == 'alias':
                mod, leaf = _owner(self, name)
                mod._parameters[leaf] = pd[init]
        self._flat = flat
        self._flat_grad = None
        self._index()

    def _index(self):
        self._P = dict(self.named_parameters(remove_duplicate=False))
        self._B = dict(self.named_buffers())

    def _apply(self, fn, *a, **k):
        super(ArenaModule, self)._apply(fn, *a, **k)
        self._repack()
        return self

    def _repack(self):
        """Re-establish the flat arena after a device / dtype move (Parameter objects are kept)."""
        pd = dict(self.named_parameters())
        dev = pd[self._layout[0][0]].device
        flat = torch.empty(self._flat.numel(), dtype=torch.float32, device=dev)
        for name, off, numel, shape in self._layout:
            p = pd[name]
            flat[off:off + numel].copy_(p.data.reshape(-1))
            p.data = flat[off:off + numel].view(shape)
        self._flat = flat
        self._flat_grad = None
        self._index()

    def flat_parameters(self):
        return self._flat

    def flat_gradients(self, zero=True):
        """Flat gradient arena; every trainable parameter's .grad is a view into it."""
        if self._flat_grad is None or self._flat_grad.device != self._flat.device:
            self._flat_grad = torch.zeros_like(self._flat)
            pd = dict(self.named_parameters())
            for name, off, numel, shape in self._layout:
                pd[name].grad = self._flat_grad[off:off + numel].view(shape)
        elif zero:
            self._flat_grad.zero_()
        return self._flat_grad

    def state_dict(self, *a, **k):
        self._flush_counts()
        return super(ArenaModule, self).state_dict(*a, **k)

    def _register_grid(self, owner, h, w, device):
        """The reference's normal heads register a resolution-specific pixel grid [1, 3, h, w] as a frozen parameter on their first
        forward: same key, same values, here as well."""
        if 'grid' not in self._modules[owner]._parameters:
            ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
            grid = torch.stack([xs, ys, torch.ones_like(xs)], 0).unsqueeze(0).to(device)
            self._modules[owner].register_parameter('grid', nn.Parameter(grid, False))
            self._index()

    def load_state_dict(self, state_dict, strict=True, **kw):
        """As nn.Module.load_state_dict; a checkpoint written after the first forward also carries the lazily registered
        ``<grid_owner>.grid`` -- it is materialised here so that resuming into a fresh model works under strict=True (the reference's
        own strict load trips over that key)."""
        owner = self.grid_owner
        if owner is not None and owner + '.grid' in state_dict and 'grid' not in self._modules[owner]._parameters:
            grid = torch.as_tensor(state_dict[owner + '.grid']).detach().clone().to(device=self._flat.device, dtype=torch.float32)
            self._modules[owner].register_parameter('grid', nn.Parameter(grid, False))
            self._index()
        self._pending_counts = {}
        return super(ArenaModule, self).load_state_dict(state_dict, strict=strict, **kw)

    def _count(self, key, n=1):
        """A training BatchNorm call: `num_batches_tracked` is bumped on the host and written back by _flush_counts."""
        self._pending_counts[key] = self._pending_counts.get(key, 0) + n

    def _flush_counts(self):
        for name, n in self._pending_counts.items():
            self._B[name] += n
        self._pending_counts = {}

    # ------------------------------------------------------------------ hooks of a model family
    def _views(self, batch):
        """(reference image, target image): left / right, swapped for the one capture group recorded the other way round (evaluation)
        or by dataset.flip_lr (reference_key; mainmodel.py:69-77 of every family)."""
        a, b = batch['left'], batch['right']
        if 'groupname' in batch and not self.training:
            if batch['groupname'][0] == '2020-2-9_group20':
                a, b = b, a
        elif reference_key(self.option) == 'right':
            a, b = b, a
        return a, b

    def _shape_constants(self):
        """The lazily built device tensors a captured train step bakes in (plugin._baked_buffers keeps them alive)."""
        return []

    def _capture_key(self):
        """Model-specific switches a captured train step bakes in (part of the graph key)."""
        return ()

    # ------------------------------------------------------------------ primitives
    def _conv2d(self, *args):
        """nn.Conv2d; with option.precision 'bf16' / 16 on the bf16 MFMA kernel (BASELINE config 5), else exact fp32."""
        return ops.conv2d(*args, bf16=self.bf16_2d)

    def _bn(self, x, p, act=ACT_NONE, slope=None, res=None, res2=None, slope_const=0.0, stats=None):
        P, B = self._P, self._B
        if self.training:
            self._count(p + '.num_batches_tracked')
        return ops.norm_act(x, P[p + '.weight'], P[p + '.bias'], slope, res, res2, B[p + '.running_mean'], B[p + '.running_var'],
                            1 if self.training else 2, act, slope_const, self.stat_exchange if self.training else None, stats)

    def _stats_holder(self):
        """conv -> training BatchNorm pairs: the conv's epilogue leaves the channel sums, the BatchNorm skips its statistics pass
        (per-rank statistics only; SyncBatchNorm exchanges {mean, M2} and keeps its own pass)."""
        return {} if (self.training and self.stat_exchange is None) else None

    def _convbn2(self, x, p, stride=1, pad=1, dil=1, act=ACT_NONE, slope=None, res=None, slope_const=0.0, res2=None):
        st = self._stats_holder()
        y = ops.conv2d(x, self._P[p + '.0.weight'], None, stride, dil if dil > 1 else pad, dil, bf16=self.bf16_2d, stats=st)  # basics.py:17-22
        return self._bn(y, p + '.1', act, slope, res, res2, slope_const, stats=st)

    def _convbn3(self, x, p, stride=1, act=ACT_NONE, res=None):
        st = self._stats_holder()
        y = ops.conv3d(x, self._P[p + '.0.weight'], None, stride, 1, 1, stats=st)                  # basics.py:32-36
        return self._bn(y, p + '.1', act, None, res, stats=st)

    # ------------------------------------------------------------------ whole network
    def network(self, batch):
        with ops.conv_operands(self.bf16_all):
            return self._network(batch)
