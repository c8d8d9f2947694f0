"""StereoDPNet on MI355X: the reference's plugin surface over the libdpf_hip kernels.

Mirrors ``STEREODPNET`` of the reference (src/model/stereodpnet/mainmodel.py:21-177): same constructor
argument (the ``option`` object built from config_/*.json + src/model/stereodpnet/config.json +
dataloader/FaceDP/config.json), same ``forward(batch) -> dict`` keys, same ``state_dict`` key names and
shapes (511 entries, 512 with the PReLU gate of ``asm_activation = 'relu'``, + the lazily registered ``normal_estimator.grid``), same loss/metric hooks and
optimiser/scheduler selection.  This file is the network alone: its spec and its straight-line forward over the
HIP operator layer (ops.py); the flat parameter arena and the conv / BatchNorm primitives are core.ArenaModule's.
"""
import math
import os

import torch

from . import ops
from .core import ArenaModule, Spec, cost_levels, geometry_abvalue, set_levels
from .ops import ACT_NONE, ACT_RELU, ACT_PRELU, ACT_LEAKY, ACT_SIGMOID
from .sampler_tables import build_phase_tables, build_shift_tables, is_fractional


def _dpblock_spec(s, p, c, t):
    """DPBlock (modules.py:21-35)."""
    for n in ('conv1', 'conv2'):
        s.convbn2(p + '.%s.0' % n, c, c)
        s.prelu(p + '.%s.1' % n)
    for i in range(3):
        s.convbn2(p + '.conv_dilate.%d' % i, c, c)
    s.convbn2(p + '.conv3', 3 * c, c)
    s.convbn2(p + '.conv4.0', c, t * c)
    s.prelu(p + '.conv4.1')
    s.conv(p + '.conv5.depthwise', t * c, 1, (3, 3))
    s.conv(p + '.conv5.pointwise', t * c, t * c, (1, 1))
    s.bn(p + '.conv5.bn', t * c)
    s.prelu(p + '.conv5.prelu')
    s.conv(p + '.conv_skip', t * c, c, (1, 1), bias=('uniform', 1.0 / math.sqrt(c)))
    s.prelu(p + '.prelu')


class HourglassAggregation(object):
    """The stacked-hourglass 3-D aggregation (modules.py:204-337) of StereoDPNet and PSMNet: mix-in over core.ArenaModule."""

    @staticmethod
    def aggregation_spec(s, cin, c):
        """modules.py:264-296; cin: the channels of the cost volume."""
        def hourglass(p):                                   # PSMNetHourglass (modules.py:204-227)
            s.convbn3(p + '.conv1.0', c, 2 * c)
            s.convbn3(p + '.conv2', 2 * c, 2 * c)
            s.convbn3(p + '.conv3.0', 2 * c, 2 * c)
            s.convbn3(p + '.conv4.0', 2 * c, 2 * c)
            s.conv(p + '.conv5.0', 2 * c, 2 * c, (3, 3, 3), transpose=True)
            s.bn(p + '.conv5.1', 2 * c)
            s.conv(p + '.conv6.0', c, 2 * c, (3, 3, 3), transpose=True)
            s.bn(p + '.conv6.1', c)

        ag = 'aggregation'
        s.convbn3(ag + '.dres0.0', cin, c)
        s.convbn3(ag + '.dres0.2', c, c)
        s.convbn3(ag + '.dres1.0', c, c)
        s.convbn3(ag + '.dres1.2', c, c)
        for n in ('dres2', 'dres3', 'dres4'):
            hourglass(ag + '.' + n)
        for n in ('classif1', 'classif2', 'classif3'):
            s.convbn3(ag + '.%s.0' % n, c, c)
            s.conv(ag + '.%s.2' % n, 1, c, (3, 3, 3))

    def _hourglass(self, x, p, presqu, postsqu):
        P = self._P
        out = self._convbn3(x, p + '.conv1.0', 2, ACT_RELU)
        pre = self._convbn3(out, p + '.conv2', 1, ACT_RELU, postsqu)
        out = self._convbn3(pre, p + '.conv3.0', 2, ACT_RELU)
        out = self._convbn3(out, p + '.conv4.0', 1, ACT_RELU)
        up = ops.conv_transpose3d(out, P[p + '.conv5.0.weight'])
        post = self._bn(up, p + '.conv5.1', ACT_RELU, None, presqu if presqu is not None else pre)
        up = ops.conv_transpose3d(post, P[p + '.conv6.0.weight'])
        return up, pre, post

    def _aggregate(self, cost):
        P, p = self._P, 'aggregation'
        c0 = self._convbn3(cost, p + '.dres0.0', 1, ACT_RELU)
        c0 = self._convbn3(c0, p + '.dres0.2', 1, ACT_RELU)
        r = self._convbn3(c0, p + '.dres1.0', 1, ACT_RELU)
        c0 = self._convbn3(r, p + '.dres1.2', 1, ACT_NONE, c0)                        # dres1(cost0) + cost0
        u1, pre1, post1 = self._hourglass(c0, p + '.dres2', None, None)
        o1 = self._bn(u1, p + '.dres2.conv6.1', ACT_NONE, None, c0)                    # conv6 bn + cost0
        u2, _, post2 = self._hourglass(o1, p + '.dres3', pre1, post1)
        o2 = self._bn(u2, p + '.dres3.conv6.1', ACT_NONE, None, c0)
        u3, _, _ = self._hourglass(o2, p + '.dres4', pre1, post2)
        o3 = self._bn(u3, p + '.dres4.conv6.1', ACT_NONE, None, c0)

        def head(x, q):
            y = self._convbn3(x, q + '.0', 1, ACT_RELU)
            return ops.conv3d(y, P[q + '.2.weight'], None, 1, 1, 1)

        k1 = head(o1, p + '.classif1')
        k2 = ops.norm_act(head(o2, p + '.classif2'), res=k1)                           # classif2 + cost1
        k3 = ops.norm_act(head(o3, p + '.classif3'), res=k2)
        if self.training:
            return [k3, k2, k1], [o3, o2, o1]
        return [k3], [o3]


def build_spec(opt):
    m = opt.model
    c = m.inplanes
    s = Spec()
    fe = 'feature_extraction'
    # feature_extraction (modules.py:56-91)
    s.convbn2(fe + '.firstconv.0', m.input_channel, c)
    s.convbn2(fe + '.firstconv.2', c, c)
    s.convbn2(fe + '.firstconv.4', c, c)
    _dpblock_spec(s, fe + '.block1', c, 1)
    for i in range(m.block_stack):
        _dpblock_spec(s, fe + '.interblock1.%d' % i, c, 1)
    _dpblock_spec(s, fe + '.block2', c, 2)
    for i in range(m.block_stack):
        _dpblock_spec(s, fe + '.interblock2.%d' % i, 2 * c, 1)
    _dpblock_spec(s, fe + '.block3', 2 * c, 2)
    for i, cin in enumerate((c, 2 * c, 4 * c)):
        s.conv(fe + '.fpn.inner_blocks.%d' % i, c, cin, (1, 1), bias=('const', 0.0))
    for i in range(3):
        s.conv(fe + '.fpn.layer_blocks.%d' % i, c, c, (3, 3), bias=('const', 0.0))
    # torchvision registers inner/layer blocks interleaved per ModuleList: inner_blocks.* first, then layer_blocks.*
    s.convbn2(fe + '.lastconv.0', 3 * c, 2 * c)
    s.convbn2(fe + '.lastconv.2', 2 * c, c)
    # cost_volume.attention_layer (asm.py:131-146); `normalize` is registered twice (alias keys)
    at = 'cost_volume.attention_layer'
    s.add(at + '.normalize.weight', (c,), 'param', ('const', 1.0))
    s.add(at + '.normalize.bias', (c,), 'param', ('const', 0.0))
    s.conv(at + '.mask_convs.0', c, c, (1, 3, 3))
    s.bn(at + '.mask_convs.1', c)
    s.conv(at + '.mask_convs.3.0', c, c, (1, 1, 1))
    s.add(at + '.mask_convs.3.1.weight', (c,), 'alias', at + '.normalize.weight')
    s.add(at + '.mask_convs.3.1.bias', (c,), 'alias', at + '.normalize.bias')
    if not (m.nearest or m.bilinear or m.phase):
        raise ValueError('the ASM needs at least one of nearest / bilinear / phase (the reference fails in torch.cat of an empty list)')
    if m.asm_activation == 'relu':
        s.prelu(at + '.activation')                       # nn.PReLU(init=0.05) gate (asm.py:151-152); the reference's init loop skips it
    elif m.asm_activation != 'sigmoid':
        raise NotImplementedError('activation type is not implemented')
    HourglassAggregation.aggregation_spec(s, 2 * c, c)
    # normal_estimator (normal_module.py:32-78)
    if m.predict_normal:
        ne = 'normal_estimator'
        s.add(ne + '.costrange', (1, m.level, 1, 1), 'frozen', cost_levels(m.mindisp, m.maxdisp, m.level))
        if m.use_deform:
            for n, act, cin in (('deform_conv1', 'act1', c + 3), ('deform_conv2', 'act2', 2 * c)):
                fan = cin * 27
                s.add('%s.%s.weight' % (ne, n), (2 * c, cin, 3, 3, 3), 'param', ('uniform', 1.0 / math.sqrt(fan)))
                s.add('%s.%s.bias' % (ne, n), (2 * c,), 'param', ('uniform', 1.0 / math.sqrt(fan)))
                s.conv('%s.%s.conv_offset' % (ne, n), 81, cin, (3, 3, 3), bias=('const', 0.0))   # re-initialised, SURVEY Q4
                s.bn('%s.%s.0' % (ne, act), 2 * c)
        else:
            s.convbn3(ne + '.original_conv.0', c + 3, 2 * c)
            s.convbn3(ne + '.original_conv.2', 2 * c, 2 * c)
        for i, (ci, co) in enumerate(((2 * c, 3 * c), (3 * c, 3 * c), (3 * c, 2 * c), (2 * c, 2 * c), (2 * c, c), (c, 3))):
            s.conv('%s.n_convs.%d.0' % (ne, i), co, ci, (3, 3))
    return s


# left / right feature passes on two HIP streams in training (224.1 -> 221.5 ms per step); DPF_FEATURES_TWO_STREAMS=0: one after the other
FEATURES_TWO_STREAMS = os.environ.get('DPF_FEATURES_TWO_STREAMS', '1') == '1'


class two_stream_grad_warning_off(object):
    """The shared feature extractor's parameters receive gradients from both streams of the two-stream step: intended.  torch's
    accumulate-grad stream-mismatch warning is switched off only around that step (plugin.train_step) and restored afterwards, so a host
    application embedding the plugin keeps the diagnostic for its own models."""

    def __enter__(self):
        self.had = None
        g = torch.autograd.graph
        if FEATURES_TWO_STREAMS and hasattr(g, 'set_warn_on_accumulate_grad_stream_mismatch'):
            probe = getattr(torch._C, '_warn_on_accumulate_grad_stream_mismatch', None)      # the current setting (default: warn)
            self.had = bool(probe()) if callable(probe) else True
            g.set_warn_on_accumulate_grad_stream_mismatch(False)
        return self

    def __exit__(self, *exc):
        if self.had is not None:
            torch.autograd.graph.set_warn_on_accumulate_grad_stream_mismatch(self.had)
        return False


class StereoDPNetCore(HourglassAggregation, ArenaModule):
    """The straight-line HIP forward of StereoDPNet over the flat arena.  ``plugin.STEREODPNET`` adds the plugin hooks."""

    grid_owner = 'normal_estimator'
    _spec = staticmethod(build_spec)

    def __init__(self, option):
        super(StereoDPNetCore, self).__init__(option)
        m = option.model
        set_levels(self, m.mindisp, m.maxdisp, m.level, 4 * int(m.level))
        self.grid_cache_compat = bool(getattr(m, 'asm_grid_cache_compat', True))
        self._tables = {}

    def _repack(self):
        super(StereoDPNetCore, self)._repack()
        self._tables = {}                  # (a device move: the sampler tables are rebuilt where the parameters now live)

    def _shape_constants(self):
        return [t for tables, phase in self._tables.values() for t in tuple(tables) + tuple(phase or ()) if torch.is_tensor(t)]

    def _capture_key(self):
        return (FEATURES_TWO_STREAMS,)

    def _convbn2_concat(self, x, prefixes, dilations):
        """torch.cat([convbn(x; dilation d) for d], 1) (DPBlock.conv_dilate, modules.py:43-45): every branch's BatchNorm writes its
        channel slice of the concatenated tensor directly."""
        P, B = self._P, self._B
        sync = self.stat_exchange if self.training else None
        # DPF_CONV_BN_CAT=1: conv + BatchNorm + cat as ONE autograd node whose backward sums the three data gradients in the transposed-conv
        # epilogue (ops.ConvBnCatFn).  Measured +0.2 % on the step (the epilogue's read-modify-write costs what the two add passes cost), so
        # the default keeps the convolutions as plain launches and only fuses BatchNorm + cat.
        if sync is not None or self.bf16_2d or self.bf16_all or os.environ.get('DPF_CONV_BN_CAT', '0') != '1':
            branches = []
            for q, d in zip(prefixes, dilations):
                y = ops.conv2d(x, P[q + '.0.weight'], None, 1, d if d > 1 else 1, d, bf16=self.bf16_2d)
                if self.training:
                    self._count(q + '.1.num_batches_tracked')
                branches.append((y, P[q + '.1.weight'], P[q + '.1.bias'], B[q + '.1.running_mean'], B[q + '.1.running_var'], None))
            # (SyncBatchNorm: the three independent branches exchange their statistics in ONE all-gather, and one all-reduce in backward)
            return ops.norm_act_concat(branches, 1 if self.training else 2, ACT_NONE, exchange=sync)
        branches = []
        for q in prefixes:
            if self.training:
                self._count(q + '.1.num_batches_tracked')
            branches.append((P[q + '.0.weight'], P[q + '.1.weight'], P[q + '.1.bias'], B[q + '.1.running_mean'], B[q + '.1.running_var']))
        # one autograd node: no cat copies, and the three data gradients are summed in the transposed-conv epilogue
        return ops.conv_bn_concat(x, branches, [d if d > 1 else 1 for d in dilations], self.training)

    # ------------------------------------------------------------------ feature extractor (modules.py:21-134)
    def _dpblock(self, x, p, s):
        P = self._P
        o1 = self._convbn2(x, p + '.conv1.0', act=ACT_PRELU, slope=P[p + '.conv1.1.weight'])
        o2 = self._convbn2(o1, p + '.conv2.0', act=ACT_PRELU, slope=P[p + '.conv2.1.weight'])
        o2 = self._convbn2_concat(o2, [p + '.conv_dilate.%d' % i for i in range(3)], [2 * i + 1 for i in range(3)])
        o = self._convbn2(o2, p + '.conv3', act=ACT_PRELU, slope=P[p + '.prelu.weight'], res=o1)       # prelu(conv3 + out1)
        o = self._convbn2(o, p + '.conv4.0', s, s, 2, act=ACT_PRELU, slope=P[p + '.conv4.1.weight'])
        d = ops.depthwise_conv3x3(o, P[p + '.conv5.depthwise.weight'])
        d = self._conv2d(d, P[p + '.conv5.pointwise.weight'])
        skip = self._conv2d(x, P[p + '.conv_skip.weight'], P[p + '.conv_skip.bias'], s)
        return self._bn(d, p + '.conv5.bn', ACT_PRELU, P[p + '.conv5.prelu.weight'], None, skip)       # prelu(bn) + skip

    def _features(self, img):
        P, p = self._P, 'feature_extraction'
        x = self._convbn2(img, p + '.firstconv.0', 2, 1, 1, ACT_RELU)
        x = self._convbn2(x, p + '.firstconv.2', act=ACT_RELU)
        x = self._convbn2(x, p + '.firstconv.4', act=ACT_RELU)
        o1 = self._dpblock(x, p + '.block1', 2)
        o2 = o1
        for i in range(self.option.model.block_stack):
            o2 = self._dpblock(o2, p + '.interblock1.%d' % i, 1)
        o2 = self._dpblock(o2, p + '.block2', 2)
        o3 = o2
        for i in range(self.option.model.block_stack):
            o3 = self._dpblock(o3, p + '.interblock2.%d' % i, 1)
        o3 = self._dpblock(o3, p + '.block3', 2)
        # feature pyramid (torchvision FeaturePyramidNetwork semantics; call site modules.py:83-85,119)
        lat = lambda i, t: self._conv2d(t, P['%s.fpn.inner_blocks.%d.weight' % (p, i)], P['%s.fpn.inner_blocks.%d.bias' % (p, i)])
        out = lambda i, t: self._conv2d(t, P['%s.fpn.layer_blocks.%d.weight' % (p, i)], P['%s.fpn.layer_blocks.%d.bias' % (p, i)], 1, 1)
        last = lat(2, o3)
        lo = out(2, last)
        last = ops.nearest_up_add(lat(1, o2), last)
        mid = out(1, last)
        last = ops.nearest_up_add(lat(0, o1), last)
        hi = out(0, last)
        x = ops.concat_channels([hi, ops.upsample_bilinear(mid, 2), ops.upsample_bilinear(lo, 4)])
        x = self._convbn2(x, p + '.lastconv.0', act=ACT_RELU)
        return self._convbn2(x, p + '.lastconv.2', act=ACT_RELU)

    # ------------------------------------------------------------------ cost volume (modules.py:137-200, asm.py)
    def _shift_tables(self, h, w, delta, device):
        key = (h, w, float(delta), str(device))
        if key not in self._tables:
            m = self.option.model
            tables = tuple(t.to(device) for t in build_shift_tables(h, w, delta, m.nearest, m.bilinear, m.phase))
            phase = None
            if m.phase and is_fractional(delta):                  # per-level shifts only (asm_grid_cache_compat = false)
                phase = tuple(t.to(device) if torch.is_tensor(t) else t for t in build_phase_tables(h, w, delta))
            self._tables[key] = (tables, phase)
        return self._tables[key]

    def _attention_parts(self, fea, delta, stat_sink=None):
        """shifted copies (M = the enabled modes) + MaskingAttention up to the gate activation (asm.py:87-127,141-162).

        ``stat_sink`` = (zeroed mean buffer, zeroed var buffer): the BatchNorm EMA of this call is redirected there
        (it then holds momentum * batch statistic) so the caller can replay the reference's update sequence."""
        P, Bf, p = self._P, self._B, 'cost_volume.attention_layer'
        x3 = ops.shift_triple(fea, *self._shift_tables(fea.shape[2], fea.shape[3], delta, fea.device))  # [B,C,M,h,w]
        st = self._stats_holder()
        mk = ops.conv3d(x3, P[p + '.mask_convs.0.weight'], None, 1, (0, 1, 1), 1, stats=st)
        q = p + '.mask_convs.1'
        if self.training:
            rm, rv = stat_sink if stat_sink is not None else (Bf[q + '.running_mean'], Bf[q + '.running_var'])
            mk = ops.norm_act(mk, P[q + '.weight'], P[q + '.bias'], None, None, None, rm, rv, 1, ACT_RELU, exchange=self.stat_exchange,
                              stats=st)
        else:
            mk = ops.norm_act(mk, P[q + '.weight'], P[q + '.bias'], None, None, None, Bf[q + '.running_mean'], Bf[q + '.running_var'], 2,
                              ACT_RELU)
        mk = ops.conv3d(mk, P[p + '.mask_convs.3.0.weight'])
        if self.option.model.asm_activation == 'relu':
            s = ops.norm_act(mk, P[p + '.normalize.weight'], P[p + '.normalize.bias'], P[p + '.activation.weight'], mode=3, act=ACT_PRELU)
        else:
            s = ops.norm_act(mk, P[p + '.normalize.weight'], P[p + '.normalize.bias'], mode=3, act=ACT_SIGMOID)
        return x3, s

    def _cost_volume(self, ref, tar):
        """CostVolume.build_concat_volume (modules.py:181-197)."""
        L = int(self.level)
        q = 'cost_volume.attention_layer.mask_convs.1'
        fetch = bool(self.option.model.feature_fetch)             # the variance over the copies instead of their mean (asm.py:165-169)
        if self.grid_cache_compat:
            # The reference's shift-grid cache is keyed on nothing: every level reuses costrange[0], so its
            # 2*L attention calls are L identical (ref, target) pairs.  Compute the pair once, write it to all levels,
            # and replay the 2*L BatchNorm EMA updates in closed form:
            #   r <- 0.9 r + 0.1 s_ref ; r <- 0.9 r + 0.1 s_tar ; ... (L times)
            sink = None
            if self.training:
                C = ref.shape[1]
                z = torch.zeros(4, C, dtype=torch.float32, device=ref.device)
                sink = ((z[0], z[1]), (z[2], z[3]))
            x3f, sf = self._attention_parts(ref, +self.costrange[0], sink[0] if sink else None)
            x3b, sb = self._attention_parts(tar, -self.costrange[0], sink[1] if sink else None)
            if self.training:
                keep = 1.0 - ops.BN_MOMENTUM
                G = sum((keep * keep) ** j for j in range(L))
                for name, a_f, a_b in (('.running_mean', z[0], z[2]), ('.running_var', z[1], z[3])):
                    ops.bn_replay(self._B[q + name], a_f, a_b, keep ** (2 * L), keep * G, G)
                self._count(q + '.num_batches_tracked', 2 * L)
            return ops.cv_select(L, [(1 << L) - 1], [x3f, sf, x3b, sb], fetch)
        tensors, masks = [], []
        for i, delta in enumerate(self.costrange):
            x3f, sf = self._attention_parts(ref, +delta)
            x3b, sb = self._attention_parts(tar, -delta)
            if self.training:
                self._count(q + '.num_batches_tracked', 2)
            tensors += [x3f, sf, x3b, sb]
            masks.append(1 << i)
        return ops.cv_select(L, masks, tensors, fetch)

    # ------------------------------------------------------------------ normal module (normal_module.py:140-194)
    def _deform(self, x, p, gi_channels=None):
        P = self._P
        off = ops.conv3d(x, P[p + '.conv_offset.weight'], P[p + '.conv_offset.bias'], 1, 1, 1, gi_channels=gi_channels)
        return ops.deform_conv3d(x, off, P[p + '.weight'], P[p + '.bias'], gi_channels=gi_channels), off

    def _normals(self, cost, disp_full, batch):
        P, p, m = self._P, 'normal_estimator', self.option.model
        B, C, D, h, w = cost.shape
        abvalue = geometry_abvalue(batch, 'StereoDPNet with predict_normal')
        self._register_grid(p, h, w, cost.device)                                       # lazy, resolution specific
        if not m.use_sampling:
            raise NotImplementedError('use_sampling=false is not on the StereoDPNet hot path')
        vol, idx = ops.anm_volume(cost, disp_full, batch['K'].float(), abvalue, self.costrange, int(m.dsample_num),
                                  getattr(self, 'anm_idx_override', None))      # (diagnostic hook of the parity tests, see ops.AnmVolumeFn)
        self.last_anm_idx = idx                  # selected cost levels [B, k, h, w] (diagnostics / tests)
        if m.use_deform:
            # the 3 XYZ channels of `vol` are constants of the batch (no gradient consumer): skip their grad_input
            v1, off1 = self._deform(vol, p + '.deform_conv1', gi_channels=C)
            v1 = self._bn(v1, p + '.act1.0', ACT_RELU)
            v2, off2 = self._deform(v1, p + '.deform_conv2')
            v2 = self._bn(v2, p + '.act2.0', ACT_RELU)
        else:
            v1 = self._convbn3(vol, p + '.original_conv.0', 1, ACT_RELU)
            v2 = self._convbn3(v1, p + '.original_conv.2', 1, ACT_RELU)
            off1 = off2 = None
        Dn = v2.shape[2]
        f = ops.swap_axes12(v2).view(B * Dn, v2.shape[1], h, w)
        for i, dil in enumerate((1, 2, 4, 8, 1, 1)):
            f = self._conv2d(f, P['%s.n_convs.%d.0.weight' % (p, i)], None, 1, dil, dil)
            f = ops.norm_act(f, act=ACT_LEAKY, slope_const=0.1)
        f = ops.upsample_bilinear(f, 4)
        return ops.sigmoid_mean(f, B, Dn), off1, off2

    # ------------------------------------------------------------------ whole network (mainmodel.py:67-104)
    def _network(self, batch):
        opt = self.option
        if opt.model.predict_normal:
            geometry_abvalue(batch, 'StereoDPNet with predict_normal')         # refuse before anything is enqueued
        a, b = self._views(batch)
        if FEATURES_TWO_STREAMS and getattr(self, '_two_streams_ok', False) and self.training and self.stat_exchange is None and a.is_cuda:
            # (enabled by train_step, which sets _two_streams_ok; plain forward() callers stay on one stream)
            # the two feature passes are independent (Q8): the second one runs on its own HIP stream, so that its HBM-bound normalisation
            # kernels overlap the first one's MFMA-bound convolutions (and the other way round); autograd runs each pass's backward on
            # the stream of its forward.  Running statistics stay in the reference's order: every BatchNorm of the second pass waits
            # for the first pass's update of the same layer (ops.BN_ORDER).
            main = torch.cuda.current_stream()
            side = self._feature_stream = getattr(self, '_feature_stream', None) or ops.shared_stream(a.device, 'features')
            events = {}
            side.wait_stream(main)
            ops.BN_ORDER = ('record', events)
            try:
                ref = self._features(a)
                ops.BN_ORDER = ('wait', events)
                # the image was allocated on the caller's stream and is read on `side` -- in forward and again by the first conv's weight
                # gradient in backward: tell the caching allocator, or a caller that drops its batch early gets the block back while that
                # kernel still reads it (seen as a corrupted firstconv.0.0.weight gradient, tools/debug/two_rank_probe.py)
                b.record_stream(side)
                with torch.cuda.stream(side):
                    tar = self._features(b)
            finally:
                ops.BN_ORDER = None
            main.wait_stream(side)
            tar.record_stream(main)
        else:
            ref = self._features(a)
            tar = self._features(b)
        stage = getattr(self, '_grad_stage', None)          # data-parallel step: gradient buckets are exchanged as they complete
        if stage is not None and ref.requires_grad:
            # stage 'aggregation' (cost volume + aggregation stack) is complete once the gradients of BOTH feature maps exist
            left = [2]

            def feat_hook(g):
                left[0] -= 1
                if left[0] == 0:
                    stage('aggregation')
                return g
            ref.register_hook(feat_hook)
            tar.register_hook(feat_hook)
        vol = self._cost_volume(ref, tar)
        logits, costs = self._aggregate(vol)
        preds, pred_all, prob_all = ops.softargmin_heads(logits, self.disp_values, 4, True)
        normal = None
        if opt.model.predict_normal:
            if stage is not None and costs[0].requires_grad:
                # stage 'normal' (normal head): done when the (summed) gradient of its input reaches the aggregation stack
                costs[0].register_hook(lambda g: (stage('normal'), g)[1])
            normal, _, _ = self._normals(costs[0], preds[0], batch)
        return {'pred_depth': pred_all, 'prob_depth': prob_all,
                'pred_normal': normal.unsqueeze(1) if normal is not None else None,
                'ref_feature': ops.channel_max(ref), '_taps': {'fea_ref': ref, 'fea_tar': tar, 'volume': vol, 'out3': costs[0]},
                '_heads': {'logits': logits, 'disp_values': self.disp_values, 'scale': 4, 'align_corners': True}}
