"""DPNet (the reference's src/model/dpnet/, "Learning Single Camera Depth Estimation using Dual-Pixels", ICCV'19 -- the dual-pixel
baseline of the DualPixelFace comparison) behind the same plugin surface: mainmodel.py:29-204 (DPNET) and
modules.py:7-114 (Encoder, Encoder2, Decoder, Decoder2) on the HIP operator layer.

The two views are concatenated (6 channels); a 7x7 stride-2 stem runs beside a 7x7 stride-2 max-pool of the input; fourteen encoder
blocks ``prelu(conv2(conv1(x)) + maxpool(skip(x)))`` reach 1/32 resolution; four k4 s2 transposed-conv decoders with depthwise-separable
tails climb back, each joined to a depthwise-separable skip by the MODEL-LEVEL shared PReLU and widened by a bias-free padded 1x1 conv;
five 7x7 heads (BN + PReLU) are upsampled (align_corners) to the input size.  Kernels new with this family: max-pool (pool.hip), the
general depthwise window (conv_depthwise.hip), 7x7 convolutions (conv_wide.hip), ConvTranspose2d k4 s2 with padding 1 / 2 / 4.
"""
import math

from . import ops
from .core import ArenaModule, Spec
from .ops import ACT_PRELU

# (name, in, infilter, outfilter, stride, pad_basic): mainmodel.py:43-59
ENCODERS = (('enc_layer1_2', None, 11, 11, 1, 1),
            ('enc_layer2_1', 11, 16, 32, 2, 0), ('enc_layer2_2', 32, 16, 32, 1, 1), ('enc_layer2_3', 32, 16, 32, 1, 1),
            ('enc_layer3_1', 32, 16, 64, 2, 2), ('enc_layer3_2', 64, 16, 64, 1, 1), ('enc_layer3_3', 64, 16, 64, 1, 1),
            ('enc_layer4_1', 64, 32, 128, 2, 1), ('enc_layer4_2', 128, 32, 128, 1, 1), ('enc_layer4_3', 128, 32, 128, 1, 1),
            ('enc_layer5_1', 128, 32, 128, 2, 1), ('enc_layer5_2', 128, 32, 128, 1, 1), ('enc_layer5_3', 128, 32, 128, 1, 1))
# name -> (in, infilter, pad_basic, pad_1, pad_2, pad_3): mainmodel.py:62-65
DECODERS = {'dec_layer1': (32, 16, 4, 1, 0, 1), 'dec_layer2': (64, 16, 4, 0, 0, 0), 'dec_layer3': (128, 16, 2, 0, 1, 0),
            'dec_layer4': (128, 32, 1, 1, 1, 1)}
SKIPS = {'skip_layer1': (11, 16, 3), 'skip_layer2': (32, 16, 3), 'skip_layer3': (64, 16, 3), 'skip_layer4': (128, 32, 2)}   # mainmodel.py:68-71
EXPANDERS = {'dec_layer1_b': (16, 32), 'dec_layer2_b': (16, 32), 'dec_layer3_b': (16, 64), 'dec_layer4_b': (32, 128)}         # mainmodel.py:74-77
LAST = (32, 8, 8, 4, 1, 0, 1)                                                                                                  # mainmodel.py:80
HEADS = (('conv_last_layer5', 128, 1), ('conv_last_layer4', 64, 0), ('conv_last_layer3', 32, 1), ('conv_last_layer2', 32, 1),
         ('conv_last_layer1', 8, 1))                                                                                           # mainmodel.py:81-85


def _xavier(shape):
    """nn.init.xavier_uniform_ (mainmodel.py:112-117 overwrites the normal-by-fan-out fill of every Conv2d / ConvTranspose2d)."""
    rf = 1
    for k in shape[2:]:
        rf *= k
    return ('uniform', math.sqrt(6.0 / float(shape[1] * rf + shape[0] * rf)))


def _conv(s, name, shape):
    s.add(name + '.weight', shape, 'param', _xavier(shape))


def _basic(s, p, cin, cout, k, deconv=False, bn=True, relu=True):
    """BasicBlock (src/module/asm/basics.py:61-95): the PReLU is registered before the convolution."""
    if relu:
        s.prelu(p + '.prelu')
    _conv(s, p + '.conv', (cin, cout, k, k) if deconv else (cout, cin, k, k))
    if bn:
        s.bn(p + '.bn', cout)


def _dsc(s, p, cin, cout, k):
    """depthwise_separable_conv (basics.py:39-58)."""
    _conv(s, p + '.depthwise', (cin, 1, k, k))
    _conv(s, p + '.pointwise', (cout, cin, 1, 1))
    s.bn(p + '.bn', cout)
    s.prelu(p + '.prelu')


def _decoder(s, p, cin, f):
    _basic(s, p + '.conv1.0', cin, f, 4, deconv=True)
    for i, k in ((1, 3), (2, 1), (3, 3)):
        _dsc(s, '%s.conv1.%d' % (p, i), f, f, k)


def build_dpnet_spec(opt):
    c2 = 2 * int(opt.model.input_channel)
    s = Spec()
    _basic(s, 'enc_layer1_1.conv1', c2, 8, 7)
    for name, cin, f, cout, stride, pad in ENCODERS:
        cin = 8 + c2 if cin is None else cin
        _basic(s, name + '.conv1.0', cin, f, 3)
        _dsc(s, name + '.conv1.1', f, f, 3)
        _basic(s, name + '.conv2', f, cout, 1)
        _basic(s, name + '.skip_connection.0', cin, cout, 1)
        s.prelu(name + '.prelu')
    for name in ('dec_layer1', 'dec_layer2', 'dec_layer3', 'dec_layer4'):
        _decoder(s, name, DECODERS[name][0], DECODERS[name][1])
    for name in ('skip_layer1', 'skip_layer2', 'skip_layer3', 'skip_layer4'):
        _dsc(s, name, SKIPS[name][0], SKIPS[name][1], 3)
    for name in ('dec_layer1_b', 'dec_layer2_b', 'dec_layer3_b', 'dec_layer4_b'):
        _basic(s, name, EXPANDERS[name][0], EXPANDERS[name][1], 1, bn=False, relu=False)
    _decoder(s, 'last_layer', LAST[0], LAST[1])
    _basic(s, 'last_layer.conv1.4', LAST[1], LAST[2], 1, bn=False, relu=False)
    for name, cin, _ in HEADS:
        _basic(s, name, cin, 1, 7)
    s.prelu('prelu')
    return s


def _o(i, k, s, p):
    return (i + 2 * p - k) // s + 1


def dpnet_shapes(H, W):
    """The spatial extents of DPNET.forward for an H x W input (the comments of mainmodel.py:162-177): {'x_layer1' ... 'x_layer5',
    'y_layer5' ... 'y_layer1', 'head5' ... 'head1' (before the upsampling), 'out5' ... 'out1'}."""
    def both(f):
        return lambda hw: (f(hw[0]), f(hw[1]))
    out = {}
    cur = both(lambda i: _o(i, 7, 2, 1))((H, W))
    enc = {}
    for name, _, _, _, stride, pad in ENCODERS:
        cur = both(lambda i: _o(i, 3, stride, pad))(cur)
        enc[name] = cur
    for i, name in enumerate(('enc_layer1_2', 'enc_layer2_3', 'enc_layer3_3', 'enc_layer4_3', 'enc_layer5_3')):
        out['x_layer%d' % (i + 1)] = enc[name]

    def decoder(hw, cfg):
        pb, p1, p2, p3 = cfg
        hw = both(lambda i: (i - 1) * 2 - 2 * pb + 4)(hw)
        for k, p in ((3, p1), (1, p2), (3, p3)):
            hw = both(lambda i: _o(i, k, 1, p))(hw)
        return hw

    cur = out['x_layer5']
    for lvl, dec in ((5, 'dec_layer4'), (4, 'dec_layer3'), (3, 'dec_layer2'), (2, 'dec_layer1')):
        cur = decoder(cur, DECODERS[dec][2:])
        skip = both(lambda i: _o(i, 3, 1, SKIPS['skip_layer%d' % (lvl - 1)][2]))(out['x_layer%d' % (lvl - 1)])
        if skip != cur:
            raise ValueError('DPNet: decoder %s gives %s, its skip %s (H, W must be multiples of 16)' % (dec, cur, skip))
        cur = (cur[0] + 2, cur[1] + 2)                               # the padded 1x1 expander
        out['y_layer%d' % lvl] = cur
    cur = decoder(cur, LAST[3:])
    out['y_layer1'] = (cur[0] + 2, cur[1] + 2)
    for (name, _, pad), lvl, scale in zip(HEADS, (5, 4, 3, 2, 1), (16, 8, 4, 2, 1)):
        h = both(lambda i: _o(i, 7, 1, pad))(out['y_layer%d' % lvl])
        out['head%d' % lvl] = h
        out['out%d' % lvl] = (h[0] * scale, h[1] * scale)
    return out


class DPNetCore(ArenaModule):
    _spec = staticmethod(build_dpnet_spec)

    # ------------------------------------------------------------------ blocks
    def _basic(self, x, p, stride=1, pad=1, deconv=False, res2=None):
        """BasicBlock.forward with BN and PReLU: prelu(bn(conv(x))) (+ res2)."""
        P = self._P
        if deconv:
            st = None
            y = ops.conv_transpose2d(x, P[p + '.conv.weight'], stride, pad)
        else:
            st = self._stats_holder()
            y = ops.conv2d(x, P[p + '.conv.weight'], None, stride, pad, 1, stats=st)
        return self._bn(y, p + '.bn', ACT_PRELU, P[p + '.prelu.weight'], None, res2, stats=st)

    def _dsc(self, x, p, pad, res2=None):
        """depthwise_separable_conv.forward: prelu(bn(pointwise(depthwise(x)))) (+ res2)."""
        P = self._P
        w = P[p + '.depthwise.weight']
        d = ops.depthwise_conv3x3(x, w) if (w.shape[2] == 3 and pad == 1) else ops.depthwise_conv2d(x, w, pad)
        y = ops.conv2d(d, P[p + '.pointwise.weight'])
        return self._bn(y, p + '.bn', ACT_PRELU, P[p + '.prelu.weight'], None, res2)

    def _encoder(self, x, p, stride, pad):
        """Encoder.forward (modules.py:25-36): prelu(conv2(conv1(x)) + maxpool(skip(x)))."""
        skip = ops.max_pool2d(self._basic(x, p + '.skip_connection.0', 1, pad), 3, stride, 0)
        y = self._basic(x, p + '.conv1.0', stride, pad)
        y = self._dsc(y, p + '.conv1.1', 1)
        y = self._basic(y, p + '.conv2', 1, 0, res2=skip)
        return ops.norm_act(y, slope=self._P[p + '.prelu.weight'], act=ACT_PRELU)

    def _decoder(self, x, p, cfg, res2=None):
        """Decoder.forward (modules.py:79-84, mode None): transposed conv + three depthwise-separable convs."""
        pb, p1, p2, p3 = cfg
        y = self._basic(x, p + '.conv1.0', 2, pb, deconv=True)
        y = self._dsc(y, p + '.conv1.1', p1)
        y = self._dsc(y, p + '.conv1.2', p2)
        return self._dsc(y, p + '.conv1.3', p3, res2=res2)

    def _expand(self, x, p):
        return ops.conv2d(x, self._P[p + '.conv.weight'], None, 1, 1, 1)           # BasicBlock(k1, pad 1, no BN, no PReLU)

    # ------------------------------------------------------------------ whole network (mainmodel.py:119-197)
    def _network(self, batch):
        P = self._P
        x = ops.concat_channels(list(self._views(batch)))
        H, W = x.shape[2], x.shape[3]
        dpnet_shapes(H, W)      # a size whose decoders and skips do not meet is refused here, before a join reads past the smaller of the two
        # Encoder2 (modules.py:48-56): the stem beside a max-pool of the raw input
        x = ops.concat_channels([self._basic(x, 'enc_layer1_1.conv1', 2, 1), ops.max_pool2d(x, 7, 2, 1)])
        xs = {}
        for name, _, _, _, stride, pad in ENCODERS:
            x = self._encoder(x, name, stride, pad)
            xs[name] = x
        x1, x2, x3, x4, x5 = (xs[n] for n in ('enc_layer1_2', 'enc_layer2_3', 'enc_layer3_3', 'enc_layer4_3', 'enc_layer5_3'))
        ys = {}
        y = x5
        for lvl, dec, skip_in in ((5, 'dec_layer4', x4), (4, 'dec_layer3', x3), (3, 'dec_layer2', x2), (2, 'dec_layer1', x1)):
            skip = self._dsc(skip_in, 'skip_layer%d' % (lvl - 1), SKIPS['skip_layer%d' % (lvl - 1)][2])
            y = self._decoder(y, dec, DECODERS[dec][2:], res2=skip)
            y = ops.norm_act(y, slope=P['prelu.weight'], act=ACT_PRELU)            # the model-level PReLU, shared by the four joins
            y = self._expand(y, dec + '_b')
            ys[lvl] = y
        y = self._decoder(y, 'last_layer', LAST[3:])
        ys[1] = self._expand(y, 'last_layer.conv1.4')
        outs = []
        for (name, _, pad), lvl in zip(HEADS, (5, 4, 3, 2, 1)):
            h = self._basic(ys[lvl], name, 1, pad)
            if lvl > 1:
                s = 2 ** (lvl - 1)
                h = ops.resize_bilinear(h, h.shape[2] * s, h.shape[3] * s, align_corners=True)
            if h.shape[2] != H or h.shape[3] != W:
                raise ValueError('DPNet: head %d comes out at %s for a %dx%d input (H, W must be multiples of 16)' % (lvl, tuple(h.shape[2:]), H, W))
            outs.append(h.squeeze(1))
        return {'pred_depth': ops.stack_dim1(outs[::-1]), 'ref_feature': ops.channel_max(x1),
                '_taps': {'x_layer1': x1, 'x_layer5': x5, 'y_layer5': ys[5], 'y_layer2': ys[2]}}
