"""Operator layer: torch.autograd.Functions whose forward/backward enqueue libdpf_hip kernels.

PyTorch is plumbing here (device memory, the current HIP stream, the autograd tape); every arithmetic
step runs in the hand-written HIP kernels reached through the C ABI (include/dpf_hip.h).  No function in
this file has a CPU or eager-PyTorch fallback: tensors must be fp32, contiguous and on the GPU.
"""
import collections
import ctypes
import os

import torch

from ._lib import lib, DpfError, ERRORS

ACT_NONE, ACT_RELU, ACT_PRELU, ACT_LEAKY, ACT_SIGMOID = 0, 1, 2, 3, 4
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
# BatchNorm statistics from the producing convolution's epilogue (dpf_conv_forward_stats) instead of a pass over its output
FUSE_BN_STATS = os.environ.get('DPF_FUSE_BN_STATS', '1') != '0'

_scratch = {}

# Optional live kernel timing (bench.py): a list that receives (family, algorithmic_flops, start_event, end_event) for
# every dense-convolution launch; events are recorded on the stream the kernels are launched on.
PROFILE = None
# bench.py sets this for a few extra (untimed) steps: the HBM-bound normalisation / activation launches are timed too (744 per step --
# kept out of the timed region so that their event records cannot perturb the headline number)
PROFILE_DETAIL = False


class _Timed(object):
    def __init__(self, family, flops, tag='', nbytes=0.0):
        self.family, self.flops, self.tag, self.nbytes = family, flops, tag, nbytes

    def __enter__(self):
        if PROFILE is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *a):
        if PROFILE is not None:
            self.e1.record()
            PROFILE.append((self.family, self.flops, self.e0, self.e1, self.tag, self.nbytes))
        return False


class _Off(object):
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


_Timed.OFF = _Off()


def _detail(tag, nbytes=0.0):
    """The timer of one normalisation / activation launch group: live only in bench.py's detail steps (PROFILE_DETAIL)."""
    return _Timed('norm_act', 0.0, tag, nbytes) if PROFILE_DETAIL else _Timed.OFF


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_F32 = (torch.float32,)


def _need(*ts, dtypes=(torch.float32, torch.int32), contiguous=True):
    """THE operand check: every entry that is not None is a tensor on the GPU with one of `dtypes`, contiguous unless the caller makes
    it so afterwards (contiguous=False)."""
    for t in ts:
        if t is None:
            continue
        if not torch.is_tensor(t) or not t.is_cuda:
            raise DpfError('dualpixelface_amd ops need GPU tensors (no CPU fallback)')
        if t.dtype not in dtypes:
            raise DpfError('unsupported dtype %s' % t.dtype)
        if contiguous and not t.is_contiguous():
            raise DpfError('non-contiguous tensor passed to a HIP op')


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def _int_arg(op, name, value, allowed=None):
    """An integer argument as it is (a bool, a string or a float such as 2.7 is refused, not truncated), one of `allowed` when given."""
    if not isinstance(value, bool) and hasattr(value, '__index__') and (allowed is None or value.__index__() in allowed):
        return value.__index__()
    what = 'an integer' if allowed is None else '%s or %d' % (', '.join(str(v) for v in allowed[:-1]), allowed[-1])
    raise DpfError('%s: %s must be %s, got %r' % (op, name, what, value))


def _match_pred(op, pred, *named):
    """named: (name, tensor or None, shape) -- every tensor there has that shape, the one pred's shape asks for."""
    for name, t, shape in named:
        if t is not None and tuple(t.shape) != tuple(shape):
            raise DpfError('%s: %s %s does not match pred %s (want %s)' % (op, name, tuple(t.shape), tuple(pred.shape), list(shape)))


def _batch_view(pred, min_stride):
    """(pred, its batch stride in floats) for a kernel that walks the samples of pred [B, ...] through that stride: a slice along dim 0 or
    1 of a wider tensor is taken as it is, contiguous samples at least min_stride apart; anything else is copied."""
    B = pred.shape[0]
    if not (pred[0].is_contiguous() and (B == 1 or pred.stride(0) >= min_stride)):
        pred = pred.contiguous()
    return pred, pred.stride(0) if B > 1 else pred[0].numel()


def scratch(nfloats, device, tag='ws'):
    """Stream-ordered reusable scratch, one buffer per (device, tag, current stream): launches on the side stream of
    DPF_WGRAD_ASYNC never share a slab with launches on the main stream, and a buffer that grows is replaced only for its
    own stream (the old one is released stream-ordered by the caching allocator, which was told who used it)."""
    s = torch.cuda.current_stream(device)
    key = (device, tag, s.cuda_stream)
    buf = _scratch.get(key)
    if buf is None or buf.numel() < nfloats:
        buf = torch.empty(max(int(nfloats), 1024), dtype=torch.float32, device=device)
        buf.record_stream(s)
        _scratch[key] = buf
    return buf


def _workspace(query, what, *shape, device, tag=None):
    """(tensor, nbytes) for what the C side's `query`(*shape) asks: the scratch() slab of `tag`, or without a tag a fresh float64 tensor
    (what a captured call needs to keep its buffer alive).  A negative answer raises DpfError(what % shape)."""
    nbytes = lib().call(query, *shape)
    if nbytes < 0:
        raise DpfError(what % shape)
    if tag is None:
        return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device), nbytes
    return scratch((nbytes + 3) // 4, device, tag), nbytes


_zero_arena = {}


def zero_slot(nfloats, device):
    """A zero-filled scratch slot that is handed out once per zeroing: slots are carved from a large arena that is cleared by ONE fill
    when it runs out, instead of one memset per BatchNorm backward (121 tiny memsets per step).  Stream-ordered like `scratch`."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)       # one arena per stream: a fill never races another stream's slots
    st = _zero_arena.get(key)
    n = (int(nfloats) + 31) & ~31
    if st is None or st[1] + n > st[0].numel():
        size = max(1 << 20, 4 * n)
        buf = st[0] if st is not None and st[0].numel() >= size else torch.empty(size, dtype=torch.float32, device=device)
        buf.zero_()
        st = [buf, 0]
        _zero_arena[key] = st
    slot = st[0][st[1]:st[1] + n]
    st[1] += n
    return slot


def workspace_buffers():
    """Every buffer `scratch` and `zero_slot` currently hand out (all devices, tags and streams).  A captured graph bakes their addresses
    in while the dicts above may replace them later: the train step's graph states hold these references (plugin._graph_step)."""
    return list(_scratch.values()) + [st[0] for st in _zero_arena.values()]


def _host_floats(vals):
    return (ctypes.c_float * len(vals))(*[float(v) for v in vals])


def _host_ints(vals):
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


def _t3(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v, v)


# ----------------------------------------------------------------------------------------------- deterministic mode
def set_deterministic(on):
    """dpf_set_deterministic: every merge of partial results becomes order-independent (include/dpf_hip.h), so two runs of the same step
    produce the same bits; slower.  DPF_DETERMINISTIC=1 in the environment makes it the default."""
    lib().call('dpf_set_deterministic', int(bool(on)))


def deterministic():
    return bool(lib().cdll.dpf_get_deterministic())


class deterministic_mode(object):
    """``with deterministic_mode():`` -- the mode is on inside and restored afterwards."""

    def __init__(self, on=True):
        self.on = bool(on)

    def __enter__(self):
        self.prev = deterministic()
        set_deterministic(self.on)
        return self

    def __exit__(self, *exc):
        set_deterministic(self.prev)
        return False


# ----------------------------------------------------------------------------------------------- convolution
CONV_OPERANDS_BF16 = False      # current operand precision of the dense conv kernels; the autograd functions capture it at forward time


def set_f32_matrix_path(path):
    """How precision-32 products are formed (dpf_set_f32_matrix_path): 2 = three f16 partial products of block-scaled two-way operand splits
    (default), 1 = six bf16 partial products of exact three-way splits, 0 = the fp32 matrix instructions.  Process-wide."""
    lib().call('dpf_set_f32_matrix_path', int(path))


def f32_matrix_path():
    return int(lib().cdll.dpf_get_f32_matrix_path())


class conv_operands(object):
    """``with conv_operands(True):`` dense convolutions launched inside round their operands to bf16 while staging them (fp32
    accumulation, fp32 tensors): the reference's ``precision: 16`` for its Conv2d / Conv3d layers.  Backward passes re-enter the
    precision their forward ran with."""

    def __init__(self, bf16):
        self.bf16 = bool(bf16)

    def __enter__(self):
        global CONV_OPERANDS_BF16
        self.prev = CONV_OPERANDS_BF16
        if self.bf16 != self.prev:
            lib().call('dpf_set_conv_operand_precision', int(self.bf16))
            CONV_OPERANDS_BF16 = self.bf16
        return self

    def __exit__(self, *exc):
        global CONV_OPERANDS_BF16
        if self.bf16 != self.prev:
            lib().call('dpf_set_conv_operand_precision', int(self.prev))
            CONV_OPERANDS_BF16 = self.prev
        return False


def _out_dim(i, k, s, p, d):
    return (i + 2 * p - (d * (k - 1) + 1)) // s + 1


def _supported(name, *args):
    """Calls an entry point that may decline a shape: True when it ran, False on DPF_ERR_UNSUPPORTED (the caller falls through to the
    general launch); any other code raises."""
    rc = getattr(lib().cdll, name)(*args)
    if rc not in (0, -3):
        raise DpfError('%s failed: %s' % (name, ERRORS.get(rc, rc)))
    return rc == 0


def _conv_ws(ksize, C, K, device):
    """The workspace slab of the dense forward / transposed conv kernels."""
    return scratch(lib().call('dpf_conv_workspace_floats', ksize[0] * ksize[1] * ksize[2], C, K), device, 'convw')


def _dense_timed(kind, x, K, ksize, stride, dil, sites, nfloats):
    """The PROFILE record of a dense-conv launch.  kind: 'fwd', 'tr ' (transposed) or 'wg ' (weight gradient); x: the tensor whose grid
    the tag names; sites: output positions of the underlying forward conv (the FLOP count's spatial factor); nfloats: floats moved."""
    N, C = x.shape[0], x.shape[1]
    T = ksize[0] * ksize[1] * ksize[2]
    family = 'conv_pointwise' if T == 1 else ('conv_wgrad' if kind == 'wg ' else 'conv_igemm')
    tag = '%s N%d C%d K%d %s%dx%dx%d k%d%d%d s%d d%d' % ((kind, N, C, K, 'x' if kind == 'wg ' else 'in') + tuple(x.shape[2:]) + tuple(ksize)
                                                        + (stride[2], dil[2]))
    return _Timed(family, 2.0 * N * K * C * T * sites, tag, 4.0 * nfloats)


def _conv_fwd_raw(x, w, bias, stride, pad, dil, stats=None):
    """stats: a dict the caller hands to the following training BatchNorm (norm_act(..., stats=...)); when the launch runs on the
    LDS-DMA kernel its epilogue leaves per-tile channel sums there and the BatchNorm skips its own statistics pass."""
    N, C, ID, IH, IW = x.shape
    K, _, kd, kh, kw = w.shape
    od = _out_dim(ID, kd, stride[0], pad[0], dil[0])
    oh = _out_dim(IH, kh, stride[1], pad[1], dil[1])
    ow = _out_dim(IW, kw, stride[2], pad[2], dil[2])
    out = torch.empty((N, K, od, oh, ow), dtype=torch.float32, device=x.device)
    L = lib()
    if K <= 4 and stride[2] == 1 and dil[2] == 1 and kw <= 3:
        with _Timed('conv_smallk', 2.0 * N * K * C * kd * kh * kw * od * oh * ow, 'skf N%d C%d K%d in%dx%dx%d' % (N, C, K, ID, IH, IW)):
            L.call('dpf_conv_smallk_forward', _ptr(x), _ptr(w), _ptr(bias), _ptr(out), N, C, ID, IH, IW, K, kd, kh, kw, *stride, *pad, *dil,
                   _stream())
        return out
    ws = _conv_ws((kd, kh, kw), C, K, x.device)
    with _dense_timed('fwd', x, K, (kd, kh, kw), stride, dil, od * oh * ow, x.numel() + out.numel() + w.numel()):
        if stats is not None and FUSE_BN_STATS and K <= 128 and IW % 4 == 0 and kd * kh * kw > 1:
            cap = int(L.call('dpf_conv_stats_slab_doubles', N, K, od, oh, ow))
            slab = torch.empty(cap, dtype=torch.float64, device=x.device)
            parts = ctypes.c_int(0)
            if _supported('dpf_conv_forward_stats', _ptr(x), _ptr(w), _ptr(bias), _ptr(out), _ptr(ws), N, C, ID, IH, IW, K, kd, kh, kw,
                          *stride, *pad, *dil, _ptr(slab), cap, ctypes.byref(parts), _stream()):
                stats.update(slab=slab, parts=int(parts.value), count=N * od * oh * ow, channels=K, ptr=out.data_ptr())
                return out
        L.call('dpf_conv_forward', _ptr(x), _ptr(w), _ptr(bias), _ptr(out), _ptr(ws), N, C, ID, IH, IW, K, kd, kh, kw,
               *stride, *pad, *dil, _stream())
    return out


def _conv_transpose_raw(x, w, bias, out_dims, ksize, stride, pad, dil, k_needed=None):
    """x on the strided grid [N,C,...] -> out [N,K,*out_dims]; w is [C][K][T] in memory.  ``k_needed`` < K: only the first k_needed
    output channels are computed (the others are zero)."""
    N, C, ID, IH, IW = x.shape
    K = w.shape[1]
    kd, kh, kw = ksize
    out = torch.empty((N, K) + tuple(out_dims), dtype=torch.float32, device=x.device)
    L = lib()
    if (C <= 4 and bias is None and k_needed is None and tuple(stride) == (1, 1, 1) and tuple(dil) == (1, 1, 1) and kh == 3 and kw == 3
            and out_dims[2] % 4 == 0):
        # data gradient of a conv with <= 4 output channels (cost heads, normal conv): register-window kernel instead of an MFMA tile
        # with one real reduction channel
        with _Timed('conv_smallk', 2.0 * N * K * C * kd * kh * kw * ID * IH * IW, 'skd N%d C%d K%d in%dx%dx%d' % (N, C, K, ID, IH, IW)):
            done = _supported('dpf_conv_smallk_dgrad', _ptr(x), _ptr(w), _ptr(out), N, K, *out_dims, C, kd, kh, kw, *pad, _stream())
        if done:
            return out
    kc = K                                  # output channels computed
    if k_needed is not None and 0 < k_needed < K:
        out[:, k_needed:].zero_()
        kc = k_needed
    ws = _conv_ws(ksize, C, K, x.device)
    with _dense_timed('tr ', x, kc, ksize, stride, dil, ID * IH * IW, x.numel() + out.numel() * kc // K + w.numel()):
        L.call('dpf_conv_transpose', _ptr(x), _ptr(w), _ptr(bias), _ptr(out), _ptr(ws), N, C, ID, IH, IW, kc, K, *out_dims, kd, kh, kw,
               *stride, *pad, *dil, 0, _stream())
    return out


def _conv_wgrad_raw(g, x, wshape, stride, pad, dil):
    """dW[K][C][T] for g [N,K,Q...] (strided grid) and x [N,C,I...] (dense grid)."""
    N, C, ID, IH, IW = x.shape
    K, QD, QH, QW = g.shape[1], g.shape[2], g.shape[3], g.shape[4]
    kd, kh, kw = wshape[2:]
    # (the register-window kernels for <= 4 output channels merge their workgroups with float atomics: deterministic mode takes the general
    # kernels, whose slabs are folded in a fixed order)
    smallk = K <= 4 and stride[2] == 1 and dil[2] == 1 and kw <= 3 and 16 * kd * kh <= 256 and not deterministic()
    dw = (torch.zeros if smallk else torch.empty)(wshape, dtype=torch.float32, device=x.device)
    if smallk:
        with _Timed('conv_smallk', 2.0 * N * K * C * kd * kh * kw * QD * QH * QW, 'skw N%d C%d K%d x%dx%dx%d' % (N, C, K, ID, IH, IW)):
            lib().call('dpf_conv_smallk_wgrad', _ptr(g), _ptr(x), _ptr(dw), N, C, ID, IH, IW, K, kd, kh, kw, *stride, *pad, *dil, _stream())
        return dw
    with _dense_timed('wg ', x, K, (kd, kh, kw), stride, dil, QD * QH * QW, x.numel() + g.numel() + dw.numel()):
        L = lib()
        nws = L.call('dpf_conv_wgrad_workspace_floats', kd * kh * kw, C, K)
        ws = scratch(nws, x.device, 'wgradws')
        L.call('dpf_conv_wgrad_ws', _ptr(g), _ptr(x), _ptr(dw), _ptr(ws), nws, N, C, ID, IH, IW, K, QD, QH, QW, kd, kh, kw, *stride, *pad, *dil,
               0, _stream())
    return dw


# Weight gradients are leaves of the backward graph: nothing consumes them before the optimiser.  With a registry installed
# (train_step does) they are launched on a side stream, where the MFMA-bound wgrad kernels share the chip with the HBM-bound
# normalisation / elementwise kernels of the main chain instead of queueing behind them.  Results are handed back by
# wgrad_async_finish(), which joins the side stream before anything reads them.
WGRAD_ASYNC = os.environ.get('DPF_WGRAD_ASYNC', '1') == '1'      # default on (step 236.6 -> 225.1 ms); DPF_WGRAD_ASYNC=0: in line
_wgrad_registry = None
_wgrad_pending = []
_wgrad_side = {}


def wgrad_async_begin(params):
    """params: the leaf weights whose gradients may be deferred (matched by storage address and shape)."""
    global _wgrad_registry
    _wgrad_registry = {p.data_ptr(): p for p in params} if WGRAD_ASYNC else None
    del _wgrad_pending[:]


def wgrad_async_take(want):
    """Mid-backward hand-over (bucketed gradient exchange): join the side stream and return the deferred [(parameter, gradient)] for
    which ``want(parameter)`` holds; the others stay pending."""
    taken = [pg for pg in _wgrad_pending if want(pg[0])]
    if taken:
        _wgrad_pending[:] = [pg for pg in _wgrad_pending if not want(pg[0])]
        torch.cuda.current_stream().wait_stream(_wgrad_side[taken[0][1].device])
    return taken


def wgrad_async_finish():
    """Join the side stream and return [(parameter, gradient)] in launch order."""
    global _wgrad_registry
    _wgrad_registry = None
    out = list(_wgrad_pending)
    del _wgrad_pending[:]
    if out:
        torch.cuda.current_stream().wait_stream(_wgrad_side[out[0][1].device])
    return out


_shared_streams = {}


def shared_stream(device, role):
    """ONE stream per (device, role) for the whole process ('step': the fused train step and its graph, 'features': the second feature pass,
    'wgrad': the deferred weight gradients).  torch.cuda.Stream() hands out a pool of 32 handles per device round-robin: a stream per MODEL
    -- two for every model a process ever builds -- wraps around that pool, and a later model's step stream then IS an older object's side
    stream (same handle).  After 70+ stream creations the GPU test suite crashed inside hipStreamEndCapture; with three streams per
    process the roles can never alias."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    key = (device.index, role)
    st = _shared_streams.get(key)
    if st is None:
        st = _shared_streams[key] = torch.cuda.Stream(device=device)
    return st


def _wgrad_dispatch(w, g, x, wshape, stride, pad, dil):
    """The weight gradient, or None when it was deferred to the side stream."""
    p = _wgrad_registry.get(w.data_ptr()) if _wgrad_registry is not None else None
    if p is None or p.numel() != w.numel():
        return _conv_wgrad_raw(g, x, wshape, stride, pad, dil)
    side = _wgrad_side.get(x.device)
    if side is None:
        side = _wgrad_side[x.device] = shared_stream(x.device, 'wgrad')
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gw = _conv_wgrad_raw(g, x, wshape, stride, pad, dil)
    g.record_stream(side)
    x.record_stream(side)
    _wgrad_pending.append((p, gw.view(p.shape)))
    return None


def _channel_sum(g):
    N, C = g.shape[0], g.shape[1]
    S = g.numel() // (N * C)
    out = torch.zeros(C, dtype=torch.float32, device=g.device)
    lib().call('dpf_channel_sum', _ptr(g), _ptr(out), N, C, S, _stream())
    return out


class ConvFn(torch.autograd.Function):
    """nn.Conv3d semantics on [N,C,D,H,W] (2-D callers use depth 1)."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, pad, dil, gi_channels=None, stats=None):
        x, w = _c(x), _c(w)
        _need(x, w, bias)
        ctx.cfg = (stride, pad, dil)
        ctx.gi_channels = gi_channels
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        ctx.bf16 = CONV_OPERANDS_BF16
        return _conv_fwd_raw(x, w, bias, stride, pad, dil, stats)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        stride, pad, dil = ctx.cfg
        gy = _c(gy)
        gx = gw = gb = None
        with conv_operands(ctx.bf16):
            if ctx.needs_input_grad[0]:
                gx = _conv_transpose_raw(gy, w, None, x.shape[2:], w.shape[2:], stride, pad, dil, k_needed=ctx.gi_channels)
            if ctx.needs_input_grad[1]:      # (enqueueing it BEFORE the data gradient, so that the two MFMA kernels overlap, measured +-0)
                gw = _wgrad_dispatch(w, gy, x, w.shape, stride, pad, dil)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = _channel_sum(gy)
        return gx, gw, gb, None, None, None, None, None


class ConvTransposeFn(torch.autograd.Function):
    """nn.ConvTranspose3d semantics; w is [C_in, C_out, kd, kh, kw]."""

    @staticmethod
    def forward(ctx, x, w, stride, pad, outpad):
        x, w = _c(x), _c(w)
        _need(x, w)
        ks = tuple(w.shape[2:])
        dil = (1, 1, 1)
        out_dims = tuple((x.shape[2 + i] - 1) * stride[i] - 2 * pad[i] + ks[i] + outpad[i] for i in range(3))
        ctx.cfg = (stride, pad, dil)
        ctx.save_for_backward(x, w)
        ctx.bf16 = CONV_OPERANDS_BF16
        return _conv_transpose_raw(x, w, None, out_dims, ks, stride, pad, dil)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        stride, pad, dil = ctx.cfg
        gy = _c(gy)
        gx = gw = None
        with conv_operands(ctx.bf16):
            if ctx.needs_input_grad[0]:
                gx = _conv_fwd_raw(gy, w, None, stride, pad, dil)          # w read as [K=C_in][C=C_out][T]
            if ctx.needs_input_grad[1]:
                gw = _wgrad_dispatch(w, x, gy, w.shape, stride, pad, dil)  # g := x (strided grid), x := gy (dense grid)
        return gx, gw, None, None, None


def conv3d(x, w, bias=None, stride=1, pad=0, dil=1, gi_channels=None, stats=None):
    """gi_channels: only the first gi_channels input channels need a gradient (the others' data gradient is zero).
    stats: see _conv_fwd_raw."""
    return ConvFn.apply(x, w, bias, _t3(stride), _t3(pad), _t3(dil), gi_channels, stats)


class ConvBf16Fn(torch.autograd.Function):
    """nn.Conv2d with bf16 operands / fp32 accumulation (BASELINE config 5).  Forward and the stride-1 data gradient run on
    the bf16 MFMA kernel; strided data gradients, all weight gradients and the bias gradient stay on the fp32 kernels."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, pad, dil):
        x, w = _c(x), _c(w)
        _need(x, w, bias)
        N, C, IH, IW = x.shape
        K, kh, kw = w.shape[0], w.shape[2], w.shape[3]
        oh, ow = _out_dim(IH, kh, stride, pad, dil), _out_dim(IW, kw, stride, pad, dil)
        out = torch.empty((N, K, oh, ow), dtype=torch.float32, device=x.device)
        L = lib()
        ws = scratch((L.call('dpf_conv2d_bf16_workspace_bytes', C, K, kh * kw) + 3) // 4, x.device, 'convw')
        with _Timed('conv_bf16', 2.0 * N * K * C * kh * kw * oh * ow, 'b16 N%d C%d K%d in%dx%d k%d%d s%d d%d' % (N, C, K, IH, IW, kh, kw, stride, dil)):
            L.call('dpf_conv2d_bf16_forward', _ptr(x), _ptr(w), _ptr(bias), _ptr(out), _ptr(ws), N, C, IH, IW, K, kh, kw, stride, stride, pad, pad,
                   dil, dil, _stream())
        ctx.cfg = (stride, pad, dil)
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        stride, pad, dil = ctx.cfg
        gy = _c(gy)
        N, C, IH, IW = x.shape
        K, kh, kw = w.shape[0], w.shape[2], w.shape[3]
        gx = gw = gb = None
        s3, p3, d3 = (1, stride, stride), (0, pad, pad), (1, dil, dil)
        if ctx.needs_input_grad[0]:
            if stride == 1 and dil * (kh - 1) >= pad and dil * (kw - 1) >= pad:
                gx = torch.empty_like(x)
                L = lib()
                ws = scratch((L.call('dpf_conv2d_bf16_workspace_bytes', C, K, kh * kw) + 3) // 4, x.device, 'convw')
                with _Timed('conv_bf16', 2.0 * N * K * C * kh * kw * IH * IW, 'b16t N%d C%d K%d in%dx%d k%d%d d%d' % (N, K, C, IH, IW, kh, kw, dil)):
                    L.call('dpf_conv2d_bf16_dgrad', _ptr(gy), _ptr(w), _ptr(gx), _ptr(ws), N, C, IH, IW, K, kh, kw, pad, pad, dil, dil, _stream())
            else:
                gx = _conv_transpose_raw(gy.unsqueeze(2), w.unsqueeze(2), None, (1, IH, IW), (1, kh, kw), s3, p3, d3).squeeze(2)
        if ctx.needs_input_grad[1]:
            gw = _conv_wgrad_raw(gy.unsqueeze(2), x.unsqueeze(2), (K, C, 1, kh, kw), s3, p3, d3).squeeze(2)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = _channel_sum(gy)
        return gx, gw, gb, None, None, None


def conv2d(x, w, bias=None, stride=1, pad=0, dil=1, bf16=False, stats=None):
    if bf16 and w.shape[0] > 4:          # the handful-of-channels heads keep their direct fp32 kernels
        return ConvBf16Fn.apply(x, w, bias, int(stride), int(pad), int(dil))
    y = ConvFn.apply(x.unsqueeze(2), w.unsqueeze(2), bias, (1, stride, stride), (0, pad, pad), (1, dil, dil), None, stats)
    return y.squeeze(2)


def conv_transpose3d(x, w, stride=2, pad=1, outpad=1):
    return ConvTransposeFn.apply(x, w, _t3(stride), _t3(pad), _t3(outpad))


def conv_transpose2d(x, w, stride=2, pad=1):
    """nn.ConvTranspose2d(bias=False, output_padding=0); w is [C_in, C_out, kh, kw].  ``pad`` may exceed k - 1: the output is cropped
    (DPNet's k4 s2 decoders use padding 1, 2 and 4: 2 * in, 2 * in - 2, 2 * in - 6)."""
    s, q = int(stride), int(pad)
    return ConvTransposeFn.apply(x.unsqueeze(2), w.unsqueeze(2), (1, s, s), (0, q, q), (0, 0, 0)).squeeze(2)


class DepthwiseGeneralFn(torch.autograd.Function):
    """nn.Conv2d(C, C, k, padding=pad, groups=C, bias=False), k in {1, 3}, 0 <= pad <= 3."""

    @staticmethod
    def forward(ctx, x, w, pad):
        x, w = _c(x), _c(w)
        _need(x, w)
        N, C, H, W = x.shape
        k = int(w.shape[2])
        if w.shape[0] != C or w.shape[1] != 1 or w.shape[3] != k:
            raise DpfError('depthwise_conv2d: weight %s does not fit %d channels' % (tuple(w.shape), C))
        y = torch.empty((N, C, H + 2 * pad - k + 1, W + 2 * pad - k + 1), dtype=torch.float32, device=x.device)
        lib().call('dpf_depthwise_conv2d_forward', _ptr(x), _ptr(w), _ptr(y), N, C, H, W, k, pad, _stream())
        ctx.save_for_backward(x, w)
        ctx.pad = pad
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = _c(gy)
        N, C, H, W = x.shape
        k = int(w.shape[2])
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            lib().call('dpf_depthwise_conv2d_backward_data', _ptr(gy), _ptr(w), _ptr(gx), N, C, H, W, k, ctx.pad, _stream())
        if ctx.needs_input_grad[1]:
            gw = torch.zeros_like(w)
            lib().call('dpf_depthwise_conv2d_backward_weight', _ptr(gy), _ptr(x), _ptr(gw), N, C, H, W, k, ctx.pad, _stream())
        return gx, gw, None


def depthwise_conv2d(x, w, pad):
    return DepthwiseGeneralFn.apply(x, w, int(pad))


def depthwise_conv3x3(x, w):
    return DepthwiseGeneralFn.apply(x, w, 1)


class MaxPoolFn(torch.autograd.Function):
    """nn.MaxPool2d(k, stride, pad) with PyTorch's tie rule; the backward is a gather over the stored arg-max plane (no atomics)."""

    @staticmethod
    def forward(ctx, x, k, stride, pad):
        x = _c(x)
        _need(x)
        N, C, H, W = x.shape
        oh, ow = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        y = torch.empty((N, C, oh, ow), dtype=torch.float32, device=x.device)
        idx = torch.empty((N, C, oh, ow), dtype=torch.int32, device=x.device)
        lib().call('dpf_maxpool2d_forward', _ptr(x), _ptr(y), _ptr(idx), N, C, H, W, k, stride, pad, _stream())
        ctx.save_for_backward(idx)
        ctx.cfg = (N, C, H, W, k, stride, pad)
        ctx.mark_non_differentiable(idx)
        return y, idx

    @staticmethod
    def backward(ctx, gy, _gidx):
        idx, = ctx.saved_tensors
        N, C, H, W, k, stride, pad = ctx.cfg
        gy = _c(gy)
        gx = torch.empty((N, C, H, W), dtype=torch.float32, device=gy.device)
        lib().call('dpf_maxpool2d_backward', _ptr(gy), _ptr(idx), _ptr(gx), N, C, H, W, k, stride, pad, _stream())
        return gx, None, None, None


def max_pool2d(x, k, stride, pad=0, return_indices=False):
    y, idx = MaxPoolFn.apply(x, int(k), int(stride), int(pad))
    return (y, idx) if return_indices else y


# ----------------------------------------------------------------------------------------------- norm + activation
# Two passes of a shared module on two streams (StereoDPNetCore._network: left / right feature extraction): the running-statistics
# updates of a BatchNorm layer must happen in the reference's order (first pass, then second).  BN_ORDER = ('record', events) makes
# every training statistics launch leave an event keyed by its running_mean buffer; ('wait', events) makes it wait for that event first.
BN_ORDER = None


def _bn_order_before(running_mean):
    if BN_ORDER is not None and BN_ORDER[0] == 'wait' and running_mean is not None:
        ev = BN_ORDER[1].get(running_mean.data_ptr())
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)


def _bn_order_after(running_mean):
    if BN_ORDER is not None and BN_ORDER[0] == 'record' and running_mean is not None:
        ev = torch.cuda.Event()
        ev.record()
        BN_ORDER[1][running_mean.data_ptr()] = ev


def _bn_sync_gather(xs, exchange):
    """SyncBatchNorm, first half: every tensor's local {mean, M2} per channel and its element count go into a [2C+1] slice of one packed
    vector -- the tensors are independent, so they travel in ONE all-gather.  -> per tensor (gathered [W, tot], its slice's offset)."""
    offs, tot = [], 0
    for x in xs:
        offs.append(tot)
        tot += 2 * x.shape[1] + 1
    packed = torch.empty(tot, dtype=torch.float32, device=xs[0].device)
    for x, off in zip(xs, offs):
        N, C = x.shape[0], x.shape[1]
        S = x.numel() // (N * C)
        lib().call('dpf_bn_local_moments', _ptr(x), N, C, S, _ptr(packed[off:]), _ptr(scratch(2 * C, x.device)), _stream())
        packed[off + 2 * C] = float(N * S)
    gathered = exchange.all_gather(packed)
    return [(gathered, off) for off in offs]


def _bn_stats(x, mode, running_mean, running_var, holder=None, sync=None):
    """(mean, invstd, read_x) of x [N, C, ...] for mode 1 batch norm (training: the launch also updates the running statistics, in
    BN_ORDER), 2 batch norm (eval), 3 instance norm (one statistic per sample and channel: [N * C]); mode 0 -> (None, None, False).
    holder: the dict the producing convolution got as ``stats`` (_conv_fwd_raw); when it describes exactly this tensor its per-tile
    channel sums replace the pass over x, and it is cleared.  sync: SyncBatchNorm, x's entry of _bn_sync_gather.  read_x: the
    statistics cost a pass over x (byte accounting)."""
    if mode == 0:
        return None, None, False
    N, C = x.shape[0], x.shape[1]
    S = x.numel() // (N * C)
    if mode == 3:
        N, C = 1, N * C
    L = lib()
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    invstd = torch.empty_like(mean)
    read_x = True
    if mode == 1:
        _bn_order_before(running_mean)
    if mode == 2:
        L.call('dpf_bn_eval_stats', _ptr(running_mean), _ptr(running_var), C, BN_EPS, _ptr(mean), _ptr(invstd), _stream())
        read_x = False
    elif mode == 1 and sync is not None:
        gathered, off = sync
        moments = gathered[:, off:off + 2 * C].contiguous()
        counts = gathered[:, off + 2 * C].contiguous()
        L.call('dpf_bn_merge_moments', _ptr(moments), _ptr(counts), gathered.shape[0], C, BN_EPS, BN_MOMENTUM, _ptr(running_mean),
               _ptr(running_var), _ptr(mean), _ptr(invstd), _stream())
    elif mode == 1 and holder and holder.get('ptr') == x.data_ptr() and holder['channels'] == C and holder['count'] == N * S:
        L.call('dpf_bn_finalize_partials', _ptr(holder['slab']), holder['parts'], C, N * S, BN_EPS, BN_MOMENTUM, _ptr(running_mean),
               _ptr(running_var), _ptr(mean), _ptr(invstd), _stream())
        holder.clear()
        read_x = False
    else:
        momentum, rm, rv = (BN_MOMENTUM, running_mean, running_var) if mode == 1 else (0.0, None, None)
        L.call('dpf_bn_stats', _ptr(x), N, C, S, BN_EPS, momentum, _ptr(rm), _ptr(rv), _ptr(mean), _ptr(invstd),
               _ptr(scratch(2 * C, x.device)), _stream())
    if mode == 1:
        _bn_order_after(running_mean)
    return mean, invstd, read_x


# One normalised tensor, as both directions of a node need it.  The first _NORM_TENSORS fields are the tensors a node saves (any of them
# None), the rest is plain data: view = (n, c, S) as the kernels see x (instance norm: (1, N * C, S)), training = the backward's flag,
# dy_slice = (Ctot, c0) when the tensor is the channel slice [c0, c0 + c) of a concatenation, (0, 0) when it is dense.
_Norm = collections.namedtuple('_Norm', 'x mean invstd weight bias slope res wmod view training act slope_const dy_slice')
_NORM_TENSORS = 7
# The outputs a backward call writes; None: not wanted.
_NormGrads = collections.namedtuple('_NormGrads', 'dx dres dweight dbias dslope', defaults=(None,) * 5)


def _norm_apply(x, mean, invstd, weight, bias, wmod, view, res=None, res2=None, slope=None, slope_const=0.0, act=ACT_NONE, into=None):
    """y = act((x - mean) * invstd * weight + bias + res) + res2, THE dpf_norm_act_forward call.  into = (cat, Ctot, c0): y is the channel
    slice [c0, c0 + c) of cat [N, Ctot, ...]; without it a new dense tensor.  -> y (cat in the slice form)."""
    y, Ctot, c0 = into if into is not None else (torch.empty_like(x), 0, 0)
    n, c, S = view
    lib().call('dpf_norm_act_forward', _ptr(x), _ptr(mean), _ptr(invstd), _ptr(weight), _ptr(bias), wmod, _ptr(res), _ptr(res2), act,
               _ptr(slope), float(slope_const), _ptr(y), Ctot, c0, n, c, S, _stream())
    return y


def _norm_backward(r, dy, grads, ws, phase, count):
    """THE dpf_norm_act_backward call for the record r: dy is read dense or as r.dy_slice of the concatenation's gradient, the outputs of
    `grads` (_NormGrads) that are not None are written.  phase / ws / count as in include/dpf_hip.h: 0 everything (ws: 3c floats), 3 the
    same on a ws that is zero already, 1 the local reductions into ws, 2 dx / dres from the summed ws (count -1: the global element
    count is in ws[3c])."""
    x, mean, invstd, weight, bias, slope, res, wmod, (n, c, S), training, act, slope_const, (Ctot, c0) = r
    dx, dres, dweight, dbias, dslope = grads
    lib().call('dpf_norm_act_backward', _ptr(x), _ptr(dy), Ctot, c0, _ptr(mean), _ptr(invstd), _ptr(weight), _ptr(bias), wmod, _ptr(res),
               act, _ptr(slope), slope_const, training, _ptr(dx), _ptr(dres), _ptr(dweight), _ptr(dbias), _ptr(dslope), _ptr(ws), n, c, S,
               phase, count, _stream())


def _norm_backward_local(r, dy, grads):
    """One branch of a concatenation without an exchange: phase 0 on the stream's scratch slab."""
    _norm_backward(r, dy, grads, scratch(3 * r.view[1], r.x.device), 0, 0.0)


def _norm_backward_sync(records, dy, grads, exchange):
    """SyncBatchNorm backward of independent tensors (one, or the branches of a concatenation): the local reductions of every record go
    into its [3c + 1] slice of ONE packed vector, whose last slot carries this rank's element count through the same all-reduce -- uneven
    per-rank batches need no extra collective and no host synchronisation -- then dx with the global counts.  grads: per record its
    _NormGrads.  The vector crosses a collective: a fresh tensor, not a scratch slab."""
    offs, tot = [], 0
    for r in records:
        offs.append(tot)
        tot += 3 * r.view[1] + 1
    ws = torch.empty(tot, dtype=torch.float32, device=dy.device)
    for r, g, off in zip(records, grads, offs):
        n, c, S = r.view
        _norm_backward(r, dy, g, ws[off:], 1, 0.0)
        ws[off + 3 * c] = float(n) * float(S)
    exchange.all_reduce_sum_(ws)
    for r, g, off in zip(records, grads, offs):
        _norm_backward(r, dy, g, ws[off:], 2, -1.0)


def _bn_into_concat(cat, mode, act, branches, moments=None):
    """Every branch's BatchNorm writes its channel slice of cat [N, sum C_i, ...].  branches: (x, weight, bias, running_mean, running_var,
    stats holder or None) each; moments: per branch its entry of _bn_sync_gather.  -> the branches' records."""
    N, Ctot = cat.shape[0], cat.shape[1]
    records, c0 = [], 0
    for i, (x, w, b, rm, rv, holder) in enumerate(branches):
        C = x.shape[1]
        view = (N, C, x.numel() // (N * C))
        mean, invstd, _ = _bn_stats(x, mode, rm, rv, holder, moments[i] if moments else None)
        _norm_apply(x, mean, invstd, w, b, C, view, act=act, into=(cat, Ctot, c0))
        records.append(_Norm(x, mean, invstd, w, b, None, None, C, view, 1 if mode == 1 else 0, act, 0.0, (Ctot, c0)))
        c0 += C
    return records


def _save_norms(ctx, records, *first):
    """ctx keeps `first` and the records' tensors as saved tensors, the records' plain fields beside them."""
    for r in records:
        first += r[:_NORM_TENSORS]
    ctx.save_for_backward(*first)
    ctx.norm_fields = [r[_NORM_TENSORS:] for r in records]


def _saved_norms(ctx):
    """-> (the `first` of _save_norms, the records), from one read of saved_tensors."""
    sv, fields = ctx.saved_tensors, ctx.norm_fields
    k = len(sv) - _NORM_TENSORS * len(fields)
    return sv[:k], [_Norm._make(sv[k + _NORM_TENSORS * i:k + _NORM_TENSORS * (i + 1)] + f) for i, f in enumerate(fields)]


def _groups(seq, k):
    return [seq[i:i + k] for i in range(0, len(seq), k)]


def _like(t, wanted):
    """An output the finalize kernel writes (not accumulates): no zero fill."""
    return torch.empty_like(t) if (t is not None and wanted) else None


class NormActFn(torch.autograd.Function):
    """y = act(norm(x) * w + b + res) + res2 with norm = batch norm (training/eval) or instance norm, or no norm."""

    @staticmethod
    def forward(ctx, x, weight, bias, slope, res, res2, running_mean, running_var, mode, act, slope_const, exchange=None, stats=None):
        # mode: 0 none, 1 batch norm (training), 2 batch norm (eval), 3 instance norm
        # exchange: distributed.StatExchange -> training batch norm uses the statistics of the global batch (SyncBatchNorm)
        x = _c(x)
        res = None if res is None else _c(res)
        res2 = None if res2 is None else _c(res2)
        _need(x, weight, bias, slope, res, res2)
        N, C = x.shape[0], x.shape[1]
        S = x.numel() // (N * C)
        view = (1, N * C, S) if mode == 3 else (N, C, S)
        sync = exchange if mode == 1 else None
        with _detail('naf') as timer:
            moments = _bn_sync_gather([x], sync)[0] if sync is not None else None
            mean, invstd, read_x = _bn_stats(x, mode, running_mean, running_var, stats, moments)
            # algorithmic bytes: statistics pass (unless the conv epilogue made them) + apply (x and residuals in, y out)
            timer.nbytes = 4.0 * x.numel() * (read_x + 2 + (res is not None) + (res2 is not None))
            y = _norm_apply(x, mean, invstd, weight, bias, C, view, res=res, res2=res2, slope=slope, slope_const=slope_const, act=act)
        r = _Norm(x, mean, invstd, weight, bias, slope, res, C, view, 1 if mode in (1, 3) else 0, act, float(slope_const), (0, 0))
        # one record, saved and rebuilt in place: the list form (_save_norms / _saved_norms) costs this node, the one behind most of the
        # step's norm launches, 2 us of Python each way
        ctx.save_for_backward(*r[:_NORM_TENSORS])
        ctx.norm_fields = r[_NORM_TENSORS:]
        ctx.has_res2 = res2 is not None
        ctx.exchange = sync
        return y

    @staticmethod
    def backward(ctx, gy):
        r = _Norm._make(ctx.saved_tensors + ctx.norm_fields)
        gy = _c(gy)
        need = ctx.needs_input_grad
        x, weight, bias, slope = r.x, r.weight, r.bias, r.slope
        g = _NormGrads(torch.empty_like(x) if need[0] else None,
                       torch.empty_like(x) if (r.res is not None and need[4]) else None,
                       torch.empty_like(weight) if (weight is not None and need[1]) else None,
                       torch.empty_like(bias) if (bias is not None and need[2]) else None,
                       torch.empty_like(slope) if (slope is not None and need[3]) else None)
        # algorithmic bytes: reduce pass (x, gy) when the norm trains + apply pass (x, gy in; dx, dres out)
        with _detail('nab', 4.0 * x.numel() * ((2 if r.training else 0) + 2 + (g.dx is not None) + (g.dres is not None))):
            if ctx.exchange is not None:
                _norm_backward_sync([r], gy, [g], ctx.exchange)
            else:
                _norm_backward(r, gy, g, zero_slot(3 * r.view[1], x.device), 3, 0.0)      # pre-zeroed: phase 3 skips the per-layer memset
        dres2 = gy if (ctx.has_res2 and need[5]) else None
        return g.dx, g.dweight, g.dbias, g.dslope, g.dres, dres2, None, None, None, None, None, None, None


def norm_act(x, weight=None, bias=None, slope=None, res=None, res2=None, running_mean=None, running_var=None, mode=0, act=ACT_NONE,
             slope_const=0.0, exchange=None, stats=None):
    return NormActFn.apply(x, weight, bias, slope, res, res2, running_mean, running_var, mode, act, slope_const, exchange, stats)


class NormActCatFn(torch.autograd.Function):
    """torch.cat([act(batch_norm(x_i)) for i], dim=1) without the copies: every branch's normalisation kernel writes its channel
    slice of the concatenated tensor, the backward reads its slice of the incoming gradient (the y_channels / dy_channels arguments)."""

    @staticmethod
    def forward(ctx, mode, act, holders, exchange, *tensors):
        branches = [(_c(x), w, b, rm, rv) for x, w, b, rm, rv in _groups(tensors, 5)]
        xs = [br[0] for br in branches]
        _need(*xs)
        cat = torch.empty((xs[0].shape[0], sum(x.shape[1] for x in xs)) + tuple(xs[0].shape[2:]), dtype=torch.float32, device=xs[0].device)
        sync = exchange if mode == 1 else None
        with _detail('ncf', 4.0 * sum(x.numel() for x in xs) * 2):
            moments = _bn_sync_gather(xs, sync) if sync is not None else None
            records = _bn_into_concat(cat, mode, act, [br + (h,) for br, h in zip(branches, holders or [None] * len(xs))], moments)
        _save_norms(ctx, records)
        ctx.exchange = sync
        return cat

    @staticmethod
    def backward(ctx, gcat):
        _, records = _saved_norms(ctx)
        gcat = _c(gcat)
        with _detail('ncb', 4.0 * gcat.numel() * 5):
            grads = [_NormGrads(dx=_like(r.x, nx), dweight=_like(r.weight, nw), dbias=_like(r.bias, nb))
                     for r, (nx, nw, nb, _, _) in zip(records, _groups(ctx.needs_input_grad[4:], 5))]
            if ctx.exchange is not None:
                _norm_backward_sync(records, gcat, grads, ctx.exchange)
            else:
                for r, g in zip(records, grads):
                    _norm_backward_local(r, gcat, g)
        flat = []
        for g in grads:
            flat += [g.dx, g.dweight, g.dbias, None, None]
        return (None, None, None, None) + tuple(flat)


def _conv_transpose_acc(x, w, out, ksize, stride, pad, dil):
    """out += conv_transpose(x, w) (the data gradient of another consumer of the same tensor), in the kernel epilogue when the shape
    runs on the LDS-DMA kernel, else through a temporary."""
    N, C, ID, IH, IW = x.shape
    K = w.shape[1]
    kd, kh, kw = ksize
    ws = _conv_ws(ksize, C, K, x.device)
    with _dense_timed('tr ', x, K, ksize, stride, dil, ID * IH * IW, x.numel() + 2 * out.numel() + w.numel()):
        done = _supported('dpf_conv_transpose', _ptr(x), _ptr(w), None, _ptr(out), _ptr(ws), N, C, ID, IH, IW, K, K, *out.shape[2:],
                          kd, kh, kw, *stride, *pad, *dil, 1, _stream())
    if not done:
        out.add_(_conv_transpose_raw(x, w, None, out.shape[2:], ksize, stride, pad, dil))
    return out


class ConvBnCatFn(torch.autograd.Function):
    """torch.cat([batch_norm(conv2d(x, w_i, dilation d_i)) for i], 1) as one node (DPBlock.conv_dilate, modules.py:43-45): the
    BatchNorms write their slices of the concatenation (no cat copies), and in the backward the branches' data gradients are summed
    into one tensor by the transposed-conv epilogue (no autograd add passes)."""

    @staticmethod
    def forward(ctx, mode, dils, x, *params):
        x = _c(x)
        _need(x)
        x5 = x.unsqueeze(2)
        branches = []
        for d, (w, bw, bb, rm, rv) in zip(dils, _groups(params, 5)):
            st = {} if mode == 1 else None
            y = _conv_fwd_raw(x5, _c(w).unsqueeze(2), None, (1, 1, 1), (0, d, d), (1, d, d), st)
            branches.append((y, bw, bb, rm, rv, st))
        cat = torch.empty((x.shape[0], sum(br[0].shape[1] for br in branches)) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
        _save_norms(ctx, _bn_into_concat(cat, mode, ACT_NONE, branches), x, *params[0::5])
        ctx.dils = tuple(dils)
        return cat

    @staticmethod
    def backward(ctx, gcat):
        (x, *ws), records = _saved_norms(ctx)
        gcat = _c(gcat)
        x5 = x.unsqueeze(2)
        need_dx = ctx.needs_input_grad[2]
        dx5 = None
        grads = []
        for r, w, d, (nw, nbw, nbb, _, _) in zip(records, ws, ctx.dils, _groups(ctx.needs_input_grad[3:], 5)):
            dy = torch.empty_like(r.x)
            dbw, dbb = _like(r.weight, nbw), _like(r.bias, nbb)
            _norm_backward_local(r, gcat, _NormGrads(dx=dy, dweight=dbw, dbias=dbb))
            # the weight gradient in line, on the main stream's slab: not deferred to the side stream
            w5 = w.unsqueeze(2)
            gw = None
            if nw:
                gw = _conv_wgrad_raw(dy, x5, w5.shape, (1, 1, 1), (0, d, d), (1, d, d)).squeeze(2)
            if need_dx:
                if dx5 is None:
                    dx5 = _conv_transpose_raw(dy, w5, None, x5.shape[2:], w5.shape[2:], (1, 1, 1), (0, d, d), (1, d, d))
                else:
                    _conv_transpose_acc(dy, w5, dx5, w5.shape[2:], (1, 1, 1), (0, d, d), (1, d, d))
            grads += [gw, dbw, dbb, None, None]
        return (None, None, dx5.squeeze(2) if dx5 is not None else None) + tuple(grads)


def conv_bn_concat(x, branches, dilations, training):
    """branches: list of (conv weight [K, C, 3, 3], bn weight, bn bias, running_mean, running_var); padding = dilation."""
    flat = []
    for br in branches:
        flat += list(br)
    return ConvBnCatFn.apply(1 if training else 2, tuple(int(d) for d in dilations), x, *flat)


def norm_act_concat(branches, mode, act=ACT_NONE, exchange=None):
    """branches: list of (x, weight, bias, running_mean, running_var, stats holder or None) with equal batch / spatial shape;
    mode 1 = training batch norm (per-rank statistics, or global-batch statistics through ``exchange`` -- one collective for all
    branches), 2 = eval.  -> [N, sum C_i, ...]."""
    flat = []
    for x, w, b, rm, rv, _ in branches:
        flat += [x, w, b, rm, rv]
    return NormActCatFn.apply(mode, act, [br[5] for br in branches], exchange, *flat)


# ----------------------------------------------------------------------------------------------- resampling
class BilinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, H, W):
        x = _c(x)
        _need(x)
        N, C, h, w = x.shape
        y = torch.empty((N, C, H, W), dtype=torch.float32, device=x.device)
        lib().call('dpf_upsample_bilinear2d_forward', _ptr(x), _ptr(y), N * C, h, w, H, W, _stream())
        ctx.dims = (N, C, h, w, H, W)
        return y

    @staticmethod
    def backward(ctx, gy):
        N, C, h, w, H, W = ctx.dims
        gy = _c(gy)
        dx = torch.empty((N, C, h, w), dtype=torch.float32, device=gy.device)
        lib().call('dpf_upsample_bilinear2d_backward', _ptr(gy), _ptr(dx), N * C, h, w, H, W, _stream())
        return dx, None, None


def upsample_bilinear(x, scale):
    return BilinearFn.apply(x, x.shape[2] * scale, x.shape[3] * scale)


class NearestAddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lat, top):
        lat, top = _c(lat), _c(top)
        _need(lat, top)
        N, C, H, W = lat.shape
        h, w = top.shape[2], top.shape[3]
        y = torch.empty_like(lat)
        lib().call('dpf_upsample_nearest_add_forward', _ptr(lat), _ptr(top), _ptr(y), N * C, h, w, H, W, _stream())
        ctx.dims = (N, C, h, w, H, W)
        return y

    @staticmethod
    def backward(ctx, gy):
        N, C, h, w, H, W = ctx.dims
        gy = _c(gy)
        dtop = torch.empty((N, C, h, w), dtype=torch.float32, device=gy.device)
        lib().call('dpf_upsample_nearest_backward', _ptr(gy), _ptr(dtop), N * C, h, w, H, W, _stream())
        return gy, dtop


def nearest_up_add(lat, top):
    return NearestAddFn.apply(lat, top)


# ----------------------------------------------------------------------------------------------- cost volume
class ShiftTripleFn(torch.autograd.Function):
    """The M row-shifted copies [B,C,M,h,w] of fea; M = tables' first dimension (the enabled shift modes)."""

    @staticmethod
    def forward(ctx, fea, iy, wy, ix, wx, iy_inv, ix_inv):
        fea = _c(fea)
        _need(fea, iy, wy, ix, wx, iy_inv, ix_inv)
        B, C, h, w = fea.shape
        M = int(iy.shape[0])
        out = torch.empty((B, C, M, h, w), dtype=torch.float32, device=fea.device)
        lib().call('dpf_shift_copies_forward', _ptr(fea), _ptr(out), _ptr(iy), _ptr(wy), _ptr(ix), _ptr(wx), B, C, M, h, w, _stream())
        ctx.tables = (iy_inv, wy, ix_inv, wx)
        ctx.dims = (B, C, M, h, w)
        return out

    @staticmethod
    def backward(ctx, g):
        iy_inv, wy, ix_inv, wx = ctx.tables
        B, C, M, h, w = ctx.dims
        g = _c(g)
        dfea = torch.empty((B, C, h, w), dtype=torch.float32, device=g.device)
        # gather form: deterministic, no atomics, no zero fill
        lib().call('dpf_shift_copies_backward_gather', _ptr(g), _ptr(dfea), _ptr(iy_inv), _ptr(wy), _ptr(ix_inv), _ptr(wx), B, C, M, h, w,
                   _stream())
        return dfea, None, None, None, None, None, None


class PhaseShiftIntoFn(torch.autograd.Function):
    """Fills the phase slot of the shifted copies x3 [B,C,M,h,w] with the fractional Fourier-phase shift of fea (dpf_phase_shift).  The
    phase copy is the last enabled mode: slot M - 1, i.e. 2 only when all three modes are on."""

    @staticmethod
    def forward(ctx, x3, fea, mr, hm, scale, mr_t, hm_t):
        fea = _c(fea)
        _need(x3, fea, mr, hm, mr_t, hm_t)
        B, C, h, w = fea.shape
        M = int(x3.shape[2])
        hw = h * w
        tbuf = torch.empty(B * C * w, dtype=torch.float32, device=fea.device)
        slot = ctypes.c_void_p(x3.data_ptr() + (M - 1) * hw * 4)
        lib().call('dpf_phase_shift', _ptr(fea), hw, slot, M * hw, _ptr(mr), _ptr(hm), float(scale), _ptr(tbuf), B * C, h, w, _stream())
        ctx.mark_dirty(x3)
        ctx.tabs = (mr_t, hm_t, float(scale))
        ctx.dims = (B, C, M, h, w)
        return x3

    @staticmethod
    def backward(ctx, g):
        mr_t, hm_t, scale = ctx.tabs
        B, C, M, h, w = ctx.dims
        g = _c(g)
        hw = h * w
        dfea = torch.empty((B, C, h, w), dtype=torch.float32, device=g.device)
        tbuf = torch.empty(B * C * w, dtype=torch.float32, device=g.device)
        slot = ctypes.c_void_p(g.data_ptr() + (M - 1) * hw * 4)
        lib().call('dpf_phase_shift', slot, M * hw, _ptr(dfea), hw, _ptr(mr_t), _ptr(hm_t), scale, _ptr(tbuf), B * C, h, w, _stream())
        # the copies' own phase slot held no taps (zero weights in the table sampler), so its incoming gradient needs no masking
        return g, dfea, None, None, None, None, None


def shift_triple(fea, tables, phase=None):
    """tables: build_shift_tables(...) on the device (M = 1, 2 or 3 enabled modes); phase: build_phase_tables(...) on the device for a
    fractional shift with the phase mode enabled."""
    x3 = ShiftTripleFn.apply(fea, *tables)
    if phase is not None:
        mr, hm, scale, mr_t, hm_t = phase
        x3 = PhaseShiftIntoFn.apply(x3, fea, mr, hm, scale, mr_t, hm_t)
    return x3


class CvSelectFn(torch.autograd.Function):
    """Writes the [B, 2C, L, h, w] volume from groups of (x_ref, s_ref, x_tar, s_tar) [B,C,M,h,w] sharing a level mask.  fetch: the
    variance over the copies instead of their mean (feature_fetch)."""

    @staticmethod
    def forward(ctx, L, masks, fetch, *ts):
        ts = [_c(t) for t in ts]
        _need(*ts)
        B, C, M, h, w = ts[0].shape
        fetch = int(bool(fetch))
        covered = 0
        for m in masks:
            covered |= m
        alloc = torch.empty if covered == (1 << L) - 1 else torch.zeros
        vol = alloc((B, 2 * C, L, h, w), dtype=torch.float32, device=ts[0].device)
        lb = lib()
        for gi, m in enumerate(masks):
            x3f, sf, x3b, sb = ts[4 * gi:4 * gi + 4]
            for x3, s, off in ((x3f, sf, 0), (x3b, sb, C)):
                lb.call('dpf_cv_select_forward', _ptr(x3), _ptr(s), _ptr(vol), B, C, M, h, w, 2 * C, L, off, m, fetch, _stream())
        ctx.save_for_backward(*ts)
        ctx.cfg = (L, tuple(masks), B, C, M, h, w, fetch)
        return vol

    @staticmethod
    def backward(ctx, dvol):
        ts = ctx.saved_tensors
        L, masks, B, C, M, h, w, fetch = ctx.cfg
        dvol = _c(dvol)
        lb = lib()
        grads = []
        for gi, m in enumerate(masks):
            x3f, sf, x3b, sb = ts[4 * gi:4 * gi + 4]
            for x3, s, off in ((x3f, sf, 0), (x3b, sb, C)):
                dx3 = torch.empty_like(x3)
                ds = torch.empty_like(s)
                lb.call('dpf_cv_select_backward', _ptr(x3), _ptr(s), _ptr(dvol), _ptr(dx3), _ptr(ds), B, C, M, h, w, 2 * C, L, off, m, fetch,
                        _stream())
                grads += [dx3, ds]
        return (None, None, None) + tuple(grads)


def cv_select(L, masks, tensors, fetch=False):
    return CvSelectFn.apply(L, list(masks), fetch, *tensors)


class PsmVolumeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ref, tar, shifts, groups):
        ref, tar = _c(ref), _c(tar)
        _need(ref, tar)
        B, C, h, w = ref.shape
        L = len(shifts)
        vol = torch.empty((B, 2 * C + groups, L, h, w), dtype=torch.float32, device=ref.device)
        lib().call('dpf_psm_volume_forward', _ptr(ref), _ptr(tar), _ptr(vol), _host_ints(shifts), B, C, h, w, L, groups, _stream())
        ctx.save_for_backward(ref, tar)
        ctx.cfg = (tuple(int(v) for v in shifts), int(groups))
        return vol

    @staticmethod
    def backward(ctx, gv):
        ref, tar = ctx.saved_tensors
        shifts, groups = ctx.cfg
        gv = _c(gv)
        B, C, h, w = ref.shape
        dref, dtar = torch.empty_like(ref), torch.empty_like(tar)
        lib().call('dpf_psm_volume_backward', _ptr(ref), _ptr(tar), _ptr(gv), _ptr(dref), _ptr(dtar), _host_ints(shifts), B, C, h, w, len(shifts),
                   groups, _stream())
        return dref, dtar, None, None


def psm_volume(ref, tar, shifts, groups=0):
    """PSMNet concat (groups=0) or concat + group-wise correlation volume (psmnet/modules.py:215-262)."""
    return PsmVolumeFn.apply(ref, tar, [int(v) for v in shifts], int(groups))


class DiffVolumeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ref, tar, shifts):
        ref, tar = _c(ref), _c(tar)
        _need(ref, tar)
        B, C, h, w = ref.shape
        L = len(shifts)
        vol = torch.empty((B, C, L, h, w), dtype=torch.float32, device=ref.device)
        lib().call('dpf_diff_volume_forward', _ptr(ref), _ptr(tar), _ptr(vol), _host_ints(shifts), B, C, h, w, L, _stream())
        ctx.cfg = (tuple(int(v) for v in shifts), B, C, h, w)
        return vol

    @staticmethod
    def backward(ctx, gv):
        shifts, B, C, h, w = ctx.cfg
        gv = _c(gv)
        dref = torch.empty((B, C, h, w), dtype=torch.float32, device=gv.device)
        dtar = torch.empty_like(dref)
        lib().call('dpf_diff_volume_backward', _ptr(gv), _ptr(dref), _ptr(dtar), _host_ints(shifts), B, C, h, w, len(shifts), _stream())
        return dref, dtar, None


def diff_volume(ref, tar, shifts):
    """StereoNet's difference volume [B, C, L, h, w] (stereonet/mainmodel.py:97-112)."""
    return DiffVolumeFn.apply(ref, tar, [int(v) for v in shifts])


class AvgPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k):
        x = _c(x)
        _need(x)
        N, C, H, W = x.shape
        y = torch.empty((N, C, H // k, W // k), dtype=torch.float32, device=x.device)
        lib().call('dpf_avg_pool2d_forward', _ptr(x), _ptr(y), N * C, H, W, int(k), _stream())
        ctx.cfg = (N, C, H, W, int(k))
        return y

    @staticmethod
    def backward(ctx, gy):
        N, C, H, W, k = ctx.cfg
        gy = _c(gy)
        dx = torch.empty((N, C, H, W), dtype=torch.float32, device=gy.device)
        lib().call('dpf_avg_pool2d_backward', _ptr(gy), _ptr(dx), N * C, H, W, k, _stream())
        return dx, None


def avg_pool2d(x, k):
    """nn.AvgPool2d((k, k), stride=(k, k))."""
    return AvgPoolFn.apply(x, int(k))


class ResizeBilinearFn(torch.autograd.Function):
    """F.interpolate(x, size=(H, W), mode='bilinear', align_corners=flag)."""

    @staticmethod
    def forward(ctx, x, H, W, align_corners):
        x = _c(x)
        _need(x)
        N, C, h, w = x.shape
        y = torch.empty((N, C, H, W), dtype=torch.float32, device=x.device)
        lib().call('dpf_resize_bilinear2d_forward', _ptr(x), _ptr(y), N * C, h, w, H, W, int(align_corners), _stream())
        ctx.dims = (N, C, h, w, H, W, int(align_corners))
        return y

    @staticmethod
    def backward(ctx, gy):
        N, C, h, w, H, W, ac = ctx.dims
        gy = _c(gy)
        dx = torch.empty((N, C, h, w), dtype=torch.float32, device=gy.device)
        lib().call('dpf_resize_bilinear2d_backward', _ptr(gy), _ptr(dx), N * C, h, w, H, W, ac, _stream())
        return dx, None, None, None


def resize_bilinear(x, H, W, align_corners=True):
    """F.interpolate(x, size=(H, W), mode='bilinear', align_corners=align_corners)."""
    if align_corners:
        return BilinearFn.apply(x, int(H), int(W))
    return ResizeBilinearFn.apply(x, int(H), int(W), False)


class L2NormalizeFn(torch.autograd.Function):
    """F.normalize(x, dim=1)."""

    @staticmethod
    def forward(ctx, x, eps):
        x = _c(x)
        _need(x)
        N, C = x.shape[0], x.shape[1]
        S = x.numel() // (N * C)
        y = torch.empty_like(x)
        lib().call('dpf_l2_normalize_forward', _ptr(x), _ptr(y), N, C, S, float(eps), _stream())
        ctx.save_for_backward(x)
        ctx.cfg = (N, C, S, float(eps))
        return y

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        N, C, S, eps = ctx.cfg
        g = _c(g)
        dx = torch.empty_like(x)
        lib().call('dpf_l2_normalize_backward', _ptr(x), _ptr(g), _ptr(dx), N, C, S, eps, _stream())
        return dx, None


def l2_normalize(x, eps=1e-12):
    return L2NormalizeFn.apply(x, eps)


def xyz_volume_into(vol, choff, sdisp, Kmat, abvalue):
    """Fills channels [choff, choff + 3) of vol [B, CV, K, h, w] with the min-max normalised camera-space coordinates of the
    disparity levels sdisp [B, K, h, w] (constants of the batch: no gradient)."""
    sdisp, Kmat, abvalue = _c(sdisp), _c(Kmat), _c(abvalue)
    _need(vol, sdisp, Kmat, abvalue)
    B, CV, K, h, w = vol.shape
    mm = torch.empty(2 * B, dtype=torch.int32, device=vol.device)
    lib().call('dpf_xyz_volume', _ptr(sdisp), _ptr(Kmat), _ptr(abvalue), _ptr(vol), _ptr(mm), B, int(choff), CV, K, h, w, _stream())
    return vol


# ----------------------------------------------------------------------------------------------- disparity head
class SoftArgminFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, disp_values, scale, want_prob, align_corners=True, prob_into=None):
        logits = _c(logits)
        _need(logits)
        B, _, D, h, w = logits.shape
        Lh, H, W = D * scale, h * scale, w * scale
        pred = torch.empty((B, H, W), dtype=torch.float32, device=logits.device)
        hd = _host_floats(disp_values)
        prob = None
        if prob_into is not None:
            # (stacked [B, n, Lh, H, W], head index): this head's probabilities go straight into their slice of the stacked tensor
            stacked, head = prob_into
            assert stacked.is_contiguous() and tuple(stacked.shape[2:]) == (Lh, H, W) and stacked.shape[0] == B
            prob_ptr, pbs = ctypes.c_void_p(stacked.data_ptr() + 4 * head * Lh * H * W), stacked.shape[1] * Lh * H * W
        else:
            if want_prob:
                prob = torch.empty((B, Lh, H, W), dtype=torch.float32, device=logits.device)
            prob_ptr, pbs = _ptr(prob), 0
        lib().call('dpf_softargmin_forward', _ptr(logits), _ptr(pred), prob_ptr, pbs, hd, B, D, h, w, Lh, H, W, int(align_corners), _stream())
        if prob is None:
            prob = pred.new_empty(0)
        ctx.save_for_backward(logits)
        ctx.cfg = (tuple(disp_values), B, D, h, w, Lh, H, W, int(align_corners))
        ctx.mark_non_differentiable(prob)
        return pred, prob

    @staticmethod
    def backward(ctx, gpred, _gprob):
        (logits,) = ctx.saved_tensors
        disp_values, B, D, h, w, Lh, H, W, ac = ctx.cfg
        gpred = _c(gpred)
        dl = torch.empty_like(logits)
        lib().call('dpf_softargmin_backward', _ptr(logits), _ptr(gpred), _ptr(dl), _host_floats(disp_values), B, D, h, w, Lh, H, W, ac,
                   _stream())
        return dl, None, None, None, None, None


def softargmin(logits, disp_values, scale=4, want_prob=True, align_corners=True, prob_into=None):
    """x`scale` trilinear upsampling of the [B, 1, D, h, w] logits + softmax over the scale * D hypotheses + expectation.
    prob_into = (stacked [B, n, scale * D, H, W], head): write the probabilities into that slice instead of a new tensor."""
    return SoftArgminFn.apply(logits, disp_values, scale, want_prob, align_corners, prob_into)


def softargmin_heads(logit_list, disp_values, scale=4, align_corners=True):
    """All heads of a model: -> (list of pred [B, H, W], pred [B, n, H, W], prob [B, n, scale * D, H, W]); the probability volumes (no
    gradient consumer) are written by each head directly into the stacked tensor."""
    B, _, D, h, w = logit_list[0].shape
    n = len(logit_list)
    prob = torch.empty((B, n, D * scale, h * scale, w * scale), dtype=torch.float32, device=logit_list[0].device)
    preds = [softargmin(l, disp_values, scale, True, align_corners, prob_into=(prob, i))[0] for i, l in enumerate(logit_list)]
    return preds, stack_dim1(preds), prob


# ----------------------------------------------------------------------------------------------- deformable conv
def deform_conv_forward_raw(x, weight, bias, offset, stride, pad, dil, group=1, dgroup=1, step=64):
    B, C, D, H, W = x.shape
    K, _, kd, kh, kw = weight.shape
    L = lib()
    do = _out_dim(D, kd, stride[0], pad[0], dil[0])
    ho = _out_dim(H, kh, stride[1], pad[1], dil[1])
    wo = _out_dim(W, kw, stride[2], pad[2], dil[2])
    out = torch.empty((B, K, do, ho, wo), dtype=torch.float32, device=x.device)
    ws = scratch(L.call('dpf_deform_conv3d_workspace_floats', C, K, kd * kh * kw), x.device, 'convw')
    # algorithmic work: the GEMM part 2 B P K C T FLOP (the 8 C T sample FMAs per voxel are not counted); bytes = x + offset + out once
    with _Timed('dcn_fwd', 2.0 * B * K * C * kd * kh * kw * do * ho * wo, 'dcnf C%d K%d %dx%dx%d' % (C, K, D, H, W),
                4.0 * (x.numel() + offset.numel() + out.numel())):
        L.call('dpf_deform_conv3d_forward', _ptr(x), _ptr(weight), _ptr(bias), _ptr(offset), _ptr(out), _ptr(ws), B, C, D, H, W, K, kd, kh, kw,
               *stride, *pad, *dil, group, dgroup, step, _stream())
    return out


def deform_conv_backward_raw(x, weight, bias, offset, go, stride, pad, dil, group=1, dgroup=1, step=64, gi_channels=None):
    B, C, D, H, W = x.shape
    K, _, kd, kh, kw = weight.shape
    L = lib()
    gi = torch.empty_like(x)
    goff = torch.empty_like(offset)
    gw = torch.empty_like(weight)
    gb = torch.empty_like(bias)
    ws = scratch(L.call('dpf_deform_conv3d_backward_workspace_floats', B, C, D, H, W, K, kd * kh * kw), x.device, 'convw')
    cg = C if gi_channels is None else int(gi_channels)
    # algorithmic work: gcol GEMM for grad_offset (all C) + grad_weight GEMM + gcol GEMM for the cg channels of grad_input; bytes = x, offset,
    # grad_output read, grad_input (cg channels) and grad_offset written, once each
    with _Timed('dcn_bwd', 2.0 * B * K * (2 * C + cg) * kd * kh * kw * go.numel() / (B * K), 'dcnb C%d K%d %dx%dx%d' % (C, K, D, H, W),
                4.0 * (x.numel() + 2 * offset.numel() + go.numel() + gi.numel() * cg // C)):
        L.call('dpf_deform_conv3d_backward', _ptr(x), _ptr(weight), _ptr(bias), _ptr(offset), _ptr(go), _ptr(gi), _ptr(goff), _ptr(gw), _ptr(gb),
               _ptr(ws), B, C, D, H, W, K, kd, kh, kw, *stride, *pad, *dil, group, dgroup, step, cg, _stream())
    return gi, goff, gw, gb


class DeformConvFn(torch.autograd.Function):
    """Same contract as the reference's DeformConvFunction (src/module/dcn3d/functions/deform_conv_func.py:16-59)."""

    @staticmethod
    def forward(ctx, x, offset, weight, bias, stride, pad, dil, gi_channels=None, group=1, deformable_group=1):
        x, offset, weight, bias = _c(x), _c(offset), _c(weight), _c(bias)
        _need(x, offset, weight, bias)
        ctx.cfg = (stride, pad, dil, group, deformable_group)
        ctx.gi_channels = gi_channels
        ctx.save_for_backward(x, offset, weight, bias)
        return deform_conv_forward_raw(x, weight, bias, offset, stride, pad, dil, group, deformable_group)

    @staticmethod
    def backward(ctx, go):
        x, offset, weight, bias = ctx.saved_tensors
        gi, goff, gw, gb = deform_conv_backward_raw(x, weight, bias, offset, _c(go), *ctx.cfg, gi_channels=ctx.gi_channels)
        return gi, goff, gw, gb, None, None, None, None, None, None


def deform_conv3d(x, offset, weight, bias, stride=1, pad=1, dil=1, gi_channels=None, group=1, deformable_group=1):
    """gi_channels: only the first gi_channels input channels need a gradient (the others' grad_input stays zero).
    group / deformable_group: weight [K, C / group, kd, kh, kw], offset [B, deformable_group * 3 T, Do, Ho, Wo] (the reference's semantics)."""
    return DeformConvFn.apply(x, offset, weight, bias, _t3(stride), _t3(pad), _t3(dil), gi_channels, group, deformable_group)


# ----------------------------------------------------------------------------------------------- deformable conv 2-D (plain / modulated)
def _t2(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def deform_conv2d_forward_raw(x, weight, bias, offset, mask, stride, pad, dil, group=1, dgroup=1, out=None):
    """dpf_deform_conv2d_forward: x [B, C, H, W], weight [K, C / group, kh, kw], bias [K] or None, offset [B, dgroup * 2 T, Ho, Wo],
    mask [B, dgroup * T, Ho, Wo] or None (the plain operator) -> [B, K, Ho, Wo] (written into `out` when the caller brings that tensor)."""
    B, C, H, W = x.shape
    K, _, kh, kw = weight.shape
    L = lib()
    ho = _out_dim(H, kh, stride[0], pad[0], dil[0])
    wo = _out_dim(W, kw, stride[1], pad[1], dil[1])
    if out is None:
        out = torch.empty((B, K, max(ho, 0), max(wo, 0)), dtype=torch.float32, device=x.device)
    ws = scratch(L.call('dpf_deform_conv2d_workspace_floats', C, K, kh * kw), x.device, 'convw')
    # algorithmic work: the GEMM part 2 B P K (C / group) T FLOP (the 4 C T sample FMAs per position are not counted)
    with _Timed('dcn2d_fwd', 2.0 * B * K * (C // max(group, 1)) * kh * kw * ho * wo, 'dcn2f C%d K%d %dx%d' % (C, K, H, W),
                4.0 * (x.numel() + offset.numel() + (0 if mask is None else mask.numel()) + out.numel())):
        L.call('dpf_deform_conv2d_forward', _ptr(x), _ptr(weight), _ptr(bias), _ptr(offset), _ptr(mask), _ptr(out), _ptr(ws), B, C, H, W, K, kh, kw,
               *stride, *pad, *dil, group, dgroup, _stream())
    return out


def deform_conv2d_backward_raw(x, weight, bias, offset, mask, go, stride, pad, dil, group=1, dgroup=1, want=(True, True, True, True, True),
                               goff_out=None, gm_out=None):
    """dpf_deform_conv2d_backward -> (grad_input, grad_offset, grad_mask, grad_weight, grad_bias); grad_mask is None without a mask, grad_bias
    without a bias.  want: which of the five to produce -- the C ABI launches no data kernel when none of the first three is wanted, no
    weight kernel without the fourth and no bias reduction without the fifth; an unwanted one comes back as None.  goff_out / gm_out: tensors
    of the caller's that grad_offset / grad_mask are written into."""
    B, C, H, W = x.shape
    K, _, kh, kw = weight.shape
    L = lib()
    data = want[0] or want[1] or (want[2] and mask is not None)
    gi = torch.empty_like(x) if want[0] else None
    goff = (torch.empty_like(offset) if goff_out is None else goff_out) if data else None
    gm = (torch.empty_like(mask) if gm_out is None else gm_out) if data and mask is not None else None
    gw = torch.empty_like(weight) if want[3] else None
    gb = torch.empty_like(bias) if want[4] and bias is not None else None
    ws = scratch(L.call('dpf_deform_conv2d_backward_workspace_floats', B, C, H, W, K, kh * kw), x.device, 'convw')
    cg = C // max(group, 1)
    with _Timed('dcn2d_bwd', 2.0 * K * cg * kh * kw * go.numel() / K * ((1 if data else 0) + (1 if want[3] else 0)), 'dcn2b C%d K%d %dx%d' % (C, K, H, W),
                4.0 * (x.numel() + 2 * offset.numel() + go.numel() + (x.numel() if want[0] else 0))):
        L.call('dpf_deform_conv2d_backward', _ptr(x), _ptr(weight), _ptr(bias), _ptr(offset), _ptr(mask), _ptr(go), _ptr(gi), _ptr(goff), _ptr(gm),
               _ptr(gw), _ptr(gb), _ptr(ws), B, C, H, W, K, kh, kw, *stride, *pad, *dil, group, dgroup, _stream())
    return gi, goff, gm, gw, gb


class DeformConv2dFn(torch.autograd.Function):
    """The reference's DeformConvFunction (mask None) and ModulatedDeformConvFunction (src/module/dcn/deform_conv.py:14-97,100-154) in one."""

    @staticmethod
    def forward(ctx, x, offset, mask, weight, bias, stride, pad, dil, group, deformable_group):
        x, offset, weight = _c(x), _c(offset), _c(weight)
        mask = None if mask is None else _c(mask)
        bias = None if bias is None else _c(bias)
        _need(x, offset, mask, weight, bias)
        ctx.cfg = (stride, pad, dil, group, deformable_group)
        ctx.save_for_backward(x, offset, mask, weight, bias)
        return deform_conv2d_forward_raw(x, weight, bias, offset, mask, stride, pad, dil, group, deformable_group)

    @staticmethod
    def backward(ctx, go):
        x, offset, mask, weight, bias = ctx.saved_tensors
        need = ctx.needs_input_grad
        want = (need[0], need[1], need[2] and mask is not None, need[3], need[4] and bias is not None)
        gi, goff, gm, gw, gb = deform_conv2d_backward_raw(x, weight, bias, offset, mask, _c(go), *ctx.cfg, want=want)
        return gi, goff, gm, gw, gb, None, None, None, None, None


def deform_conv2d(x, offset, mask, weight, bias=None, stride=1, pad=0, dil=1, group=1, deformable_group=1):
    """2-D deformable convolution: mask None = DCN v1 (DeformConv), else the modulated v2 (ModulatedDeformConv).  weight [K, C / group, kh, kw],
    offset [B, deformable_group * 2 T, Ho, Wo] (h, w per tap), mask [B, deformable_group * T, Ho, Wo]: the reference's semantics."""
    return DeformConv2dFn.apply(x, offset, mask, weight, bias, _t2(stride), _t2(pad), _t2(dil), group, deformable_group)


# ----------------------------------------------------------------------------------------------- normal module glue
class AnmVolumeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cost, disp_full, Kmat, abvalue, costrange, ksel, idx_override=None):
        cost, disp_full, Kmat, abvalue = _c(cost), _c(disp_full), _c(Kmat), _c(abvalue)
        _need(cost, disp_full, Kmat, abvalue)
        B, C, L, h, w = cost.shape
        H, W = disp_full.shape[1], disp_full.shape[2]
        dev = cost.device
        lb = lib()
        if idx_override is not None:
            # diagnostic hook (tests): the level selection is a discontinuous function of the predicted disparity -- a comparison against
            # another implementation imposes ITS selection [B, ksel, h, w] so that everything downstream is comparable pixel by pixel
            idx = idx_override.to(device=dev, dtype=torch.int32).contiguous()
            assert tuple(idx.shape) == (B, ksel, h, w)
            sdisp = torch.tensor(list(costrange), dtype=torch.float32, device=dev)[idx.long()].contiguous()
        else:
            idx = torch.empty((B, ksel, h, w), dtype=torch.int32, device=dev)
            sdisp = torch.empty((B, ksel, h, w), dtype=torch.float32, device=dev)
            lb.call('dpf_anm_select', _ptr(disp_full), _ptr(idx), _ptr(sdisp), _host_floats(costrange), B, H, W, h, w, L, ksel, _stream())
        vol = torch.empty((B, C + 3, ksel, h, w), dtype=torch.float32, device=dev)
        mm = torch.empty(2 * B, dtype=torch.int32, device=dev)
        lb.call('dpf_anm_volume_forward', _ptr(cost), _ptr(idx), _ptr(sdisp), _ptr(Kmat), _ptr(abvalue), _ptr(vol), _ptr(mm), B, C, L, ksel,
                h, w, _stream())
        ctx.save_for_backward(idx)
        ctx.dims = (B, C, L, ksel, h, w)
        ctx.mark_non_differentiable(idx)
        return vol, idx

    @staticmethod
    def backward(ctx, dvol, _gidx):
        (idx,) = ctx.saved_tensors
        B, C, L, ksel, h, w = ctx.dims
        dvol = _c(dvol)
        dcost = torch.empty((B, C, L, h, w), dtype=torch.float32, device=dvol.device)
        lib().call('dpf_anm_volume_backward', _ptr(dvol), _ptr(idx), _ptr(dcost), B, C, L, ksel, h, w, _stream())
        return dcost, None, None, None, None, None, None


def anm_volume(cost, disp_full, Kmat, abvalue, costrange, ksel, idx_override=None):
    return AnmVolumeFn.apply(cost, disp_full, Kmat, abvalue, tuple(costrange), ksel, idx_override)


class SigmoidMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, B, Dn):
        u = _c(u)
        _need(u)
        CS = u.numel() // (B * Dn)
        out = torch.empty((B,) + tuple(u.shape[1:]), dtype=torch.float32, device=u.device)
        lib().call('dpf_sigmoid_mean_forward', _ptr(u), _ptr(out), B, Dn, CS, _stream())
        ctx.save_for_backward(u)
        ctx.dims = (B, Dn, CS)
        return out

    @staticmethod
    def backward(ctx, g):
        (u,) = ctx.saved_tensors
        B, Dn, CS = ctx.dims
        g = _c(g)
        du = torch.empty_like(u)
        lib().call('dpf_sigmoid_mean_backward', _ptr(u), _ptr(g), _ptr(du), B, Dn, CS, _stream())
        return du, None, None


def sigmoid_mean(u, B, Dn):
    return SigmoidMeanFn.apply(u, B, Dn)


# ----------------------------------------------------------------------------------------------- tensor plumbing
def _copy_channels(src, dst, cs0, cd0, ncopy, accumulate=0):
    N, Cs, Cd = src.shape[0], src.shape[1], dst.shape[1]
    S = src.numel() // (N * Cs)
    lib().call('dpf_copy_channels', _ptr(src), _ptr(dst), N, Cs, cs0, Cd, cd0, ncopy, S, accumulate, _stream())


class ConcatFn(torch.autograd.Function):
    """torch.cat(tensors, dim=1) for [N, C_i, ...] tensors with equal trailing dims."""

    @staticmethod
    def forward(ctx, *ts):
        ts = [_c(t) for t in ts]
        _need(*ts)
        chans = [t.shape[1] for t in ts]
        out = torch.empty((ts[0].shape[0], sum(chans)) + tuple(ts[0].shape[2:]), dtype=torch.float32, device=ts[0].device)
        off = 0
        for t, c in zip(ts, chans):
            _copy_channels(t, out, 0, off, c)
            off += c
        ctx.chans = chans
        ctx.shapes = [tuple(t.shape) for t in ts]
        return out

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        outs, off = [], 0
        for c, shp in zip(ctx.chans, ctx.shapes):
            d = torch.empty(shp, dtype=torch.float32, device=g.device)
            _copy_channels(g, d, off, 0, c)
            outs.append(d)
            off += c
        return tuple(outs)


def concat_channels(tensors):
    return ConcatFn.apply(*tensors)


def stack_dim1(tensors):
    """torch.stack(tensors, 1) for [N, ...] tensors."""
    return ConcatFn.apply(*[t.unsqueeze(1) for t in tensors])


class SwapAxesFn(torch.autograd.Function):
    """[B, A, Bd, *S] -> [B, Bd, A, *S] (contiguous)."""

    @staticmethod
    def forward(ctx, x):
        x = _c(x)
        _need(x)
        B, A, Bd = x.shape[:3]
        S = x.numel() // (B * A * Bd)
        y = torch.empty((B, Bd, A) + tuple(x.shape[3:]), dtype=torch.float32, device=x.device)
        lib().call('dpf_swap_axes', _ptr(x), _ptr(y), B, A, Bd, S, _stream())
        return y

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        B, Bd, A = g.shape[:3]
        S = g.numel() // (B * A * Bd)
        dx = torch.empty((B, A, Bd) + tuple(g.shape[3:]), dtype=torch.float32, device=g.device)
        lib().call('dpf_swap_axes', _ptr(g), _ptr(dx), B, Bd, A, S, _stream())
        return dx


def swap_axes12(x):
    return SwapAxesFn.apply(x)


def channel_max(x):
    """x.max(1)[0] (no gradient: visualisation output only)."""
    x = _c(x.detach())
    _need(x)
    N, C = x.shape[0], x.shape[1]
    S = x.numel() // (N * C)
    y = torch.empty((N,) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    lib().call('dpf_channel_max', _ptr(x), _ptr(y), N, C, S, _stream())
    return y


def bn_replay(running, a_f, a_b, decay, cf, cb):
    _need(running, a_f, a_b)
    lib().call('dpf_bn_replay', _ptr(running), _ptr(a_f), _ptr(a_b), running.numel(), float(decay), float(cf), float(cb), _stream())


# ----------------------------------------------------------------------------------------------- loss / optimiser
class LossFn(torch.autograd.Function):
    """-> tensor [3] = (smoothL1_loss, cosine_loss, final_loss)."""

    @staticmethod
    def forward(ctx, pred_depth, pred_normal, disp, normal, mask, head_weights, lam_d, lam_n):
        # either prediction may be None (a loss used on its own: losses.SMOOTHL1Loss / COSINELoss)
        pred_depth = None if pred_depth is None else _c(pred_depth)
        disp = None if disp is None else _c(disp)
        mask = _c(mask)
        pred_normal = None if pred_normal is None else _c(pred_normal)
        normal = None if normal is None else _c(normal)
        _need(pred_depth, pred_normal, disp, normal, mask)
        if pred_depth is not None:
            B, n, H, W = pred_depth.shape
        else:
            (B, _, H, W), n = pred_normal.shape, 0
        acc = torch.empty(n + 2, dtype=torch.float32, device=mask.device)
        out = torch.empty(3, dtype=torch.float32, device=mask.device)
        lib().call('dpf_loss_forward', _ptr(pred_depth), _ptr(pred_normal), _ptr(disp), _ptr(normal), _ptr(mask), _ptr(acc), _ptr(out), B, n,
                   H, W, _host_floats(head_weights if n else [0.0]), float(lam_d), float(lam_n), _stream())
        ctx.save_for_backward(pred_depth, pred_normal, disp, normal, mask, acc)
        ctx.cfg = (tuple(head_weights), float(lam_d), float(lam_n), B, n, H, W)
        return out

    @staticmethod
    def backward(ctx, gout):
        pred_depth, pred_normal, disp, normal, mask, acc = ctx.saved_tensors
        head_weights, lam_d, lam_n, B, n, H, W = ctx.cfg
        gout = _c(gout)
        dpd = torch.empty_like(pred_depth) if pred_depth is not None else None
        dpn = torch.empty_like(pred_normal) if pred_normal is not None else None
        lib().call('dpf_loss_backward', _ptr(pred_depth), _ptr(pred_normal), _ptr(disp), _ptr(normal), _ptr(mask), _ptr(acc), _ptr(gout),
                   _ptr(dpd), _ptr(dpn), B, n, H, W, _host_floats(head_weights if n else [0.0]), lam_d, lam_n, _stream())
        return dpd, dpn, None, None, None, None, None, None


def stereo_losses(pred_depth, pred_normal, disp, normal, mask, head_weights, lam_d, lam_n):
    return LossFn.apply(pred_depth, pred_normal, disp, normal, mask, tuple(head_weights), lam_d, lam_n)


LOSS_KIND = {'smoothL1': 0, 'silog': 1}
LOSS_TRANSFORM = {'identity': 0, 'reciprocal': 1}
LOSS_STATS = 17             # doubles the forward leaves for the backward: M, mean d per head, sqrt of the variance term per head


# What one head loss is to HeadLossFn.  name: the public function's, for messages; stem: the C symbols are <stem>_workspace_bytes, _forward
# and _backward; dims: which of B, n, H, W the workspace query takes; stats: doubles the forward leaves for the backward; aux: the
# (B, n, H, W) -> shapes of the float32 planes the forward fills and the backward reads again; extras: likewise -> (shape, dtype) of the
# non-differentiable outputs a caller may ask for.
class _HeadLoss(object):
    def __init__(self, name, stem, dims, stats, aux=None, extras=None):
        self.query, self.fwd, self.bwd = stem + '_workspace_bytes', stem + '_forward', stem + '_backward'
        self.what = '%s: shape %s is not supported' % (name, ' '.join(d + '=%d' for d in dims))
        self.dims = tuple('BnHW'.index(d) for d in dims)
        self.stats, self.aux, self.extras = stats, aux, extras


class HeadLossFn(torch.autograd.Function):
    """The four losses over the heads of pred [B, n, H, W] (csrc/loss_bank.hip, normal_geo.hip, photometric.hip) -> 0-dim loss, and with
    want_extras the operator's extras (for tests and tools).  The C argument orders agree: forward `lead | ws, nbytes | aux | stats, out |
    extras`, backward `lead | aux | stats, gout, dpred`; `lead` is built once by the caller and `held` are the tensors it points into
    beside pred.  Workspace, stats and the auxiliary planes are fresh tensors (planes and stats are saved for the backward, the workspace
    is not needed again), gout is read on the device and nothing is read on the host, so the call is capturable inside the train-step
    graph like LossFn.  Only pred receives a gradient."""

    @staticmethod
    def forward(ctx, pred, op, held, lead, want_extras):
        shape, dev = pred.shape, pred.device
        ws, nbytes = _workspace(op.query, op.what, *[shape[i] for i in op.dims], device=dev)
        stats = torch.empty(op.stats, dtype=torch.float64, device=dev)
        out = torch.empty((), dtype=torch.float32, device=dev)
        aux = [torch.empty(s, dtype=torch.float32, device=dev) for s in op.aux(*shape)] if op.aux else []
        extras = []
        if op.extras:
            extras = [torch.empty(s, dtype=dtype, device=dev) if want_extras else None for s, dtype in op.extras(*shape)]
        lib().call(op.fwd, *lead, _ptr(ws), nbytes, *[_ptr(t) for t in aux], _ptr(stats), _ptr(out), *[_ptr(t) for t in extras], _stream())
        ctx.save_for_backward(pred, stats, *aux, *held)
        ctx.op, ctx.lead, ctx.naux = op, lead, len(aux)
        if want_extras:
            ctx.mark_non_differentiable(*extras)
            return (out,) + tuple(extras)
        return out

    @staticmethod
    def backward(ctx, gout, *unused):
        saved = ctx.saved_tensors
        pred, stats, aux = saved[0], saved[1], saved[2:2 + ctx.naux]
        gout = _c(gout)
        _need(gout)
        dpred = torch.empty_like(pred)
        lib().call(ctx.op.bwd, *ctx.lead, *[_ptr(t) for t in aux], _ptr(stats), _ptr(gout), _ptr(dpred), _stream())
        return dpred, None, None, None, None


_DEPTH_LOSS = _HeadLoss('depth_loss', 'dpf_depth_loss', 'BHW', LOSS_STATS)


def depth_loss(pred, target, mask=None, conf=None, head_weights=(1.0,), kind='smoothL1', transform='identity', variance_focus=0.0,
               target_ab=None):
    """pred [B, n <= 8, H, W] against target [B, H, W] over the pixels with mask > 0 (None: all), both sides times conf (None: no product);
    kind 'smoothL1' | 'silog', transform 'identity' | 'reciprocal' (of pred; non-finite -> 0 with a zero gradient) -> 0-dim loss.
    With target_ab [B, 2] = [b, a], `target` is the depth map and the kernels compare against a / depth + b (non-finite -> -100); no
    gradient reaches target_ab."""
    pred, target = _c(pred), _c(target)
    mask = None if mask is None else _c(mask)
    conf = None if conf is None else _c(conf)
    target_ab = None if target_ab is None else _c(target_ab.detach())
    _need(pred, target, mask, conf, target_ab)
    B, n, H, W = pred.shape
    if target_ab is not None and (tuple(target_ab.shape) != (B, 2) or target_ab.dtype != torch.float32):
        raise DpfError('depth_loss: target_ab %s %s, float32 [%d, 2] expected' % (tuple(target_ab.shape), target_ab.dtype, B))
    _match_pred('depth_loss', pred, ('target', target, (B, H, W)), ('mask', mask, (B, H, W)), ('conf', conf, (B, H, W)))
    if len(head_weights) != n:
        raise DpfError('depth_loss: %d head weights for %d heads' % (len(head_weights), n))
    held = (target, target_ab, mask, conf)
    lead = (LOSS_KIND[kind], LOSS_TRANSFORM[transform], _ptr(pred), *[_ptr(t) for t in held], B, n, H, W, _host_floats(head_weights),
            float(variance_focus))
    return HeadLossFn.apply(pred, _DEPTH_LOSS, held, lead, False)


AFFINE_FIT_F_SCALE, AFFINE_FIT_MAX_ITERS, AFFINE_FIT_TOL = 0.1, 48, 1e-7      # DESIGN.md section 11 has the probe behind the last two
AFFINE_FIT_INFO = 6         # doubles per sample: A, B, reweighted solves used, valid pixels, objective at (A, B), objective at the start


def affine_fit(pred, idepth, f_scale=AFFINE_FIT_F_SCALE, max_iters=AFFINE_FIT_MAX_ITERS, tol=AFFINE_FIT_TOL, return_info=False):
    """src/utils/geometry.py::regress_affine on the device (csrc/affine_fit.hip): per sample the soft-L1 line pred[:, 0] = a * idepth + b over
    the pixels with idepth > 0 -> detached float32 [B, 2] = [b, a]; with return_info also the fp64 [B, 6] record.  Workspace and results are
    fresh tensors and nothing is read on the host, so the call is capturable inside the train-step graph like HeadLossFn."""
    pred, idepth = _c(pred.detach()), _c(idepth.detach())
    _need(pred, idepth, dtypes=_F32)
    if pred.dim() != 4:
        raise DpfError('affine_fit: pred %s is not [B, n, H, W]' % (tuple(pred.shape),))
    B, n, H, W = pred.shape
    _match_pred('affine_fit', pred, ('idepth', idepth, (B, H, W)))
    ws, nbytes = _workspace('dpf_affine_fit_workspace_bytes', 'affine_fit: shape B=%d H=%d W=%d is not supported', B, H, W,
                            device=pred.device)
    ab = torch.empty((B, 2), dtype=torch.float32, device=pred.device)
    info = torch.empty((B, AFFINE_FIT_INFO), dtype=torch.float64, device=pred.device)
    lib().call('dpf_affine_fit', _ptr(pred), n * H * W, _ptr(idepth), B, H, W, float(f_scale), int(max_iters), float(tol), _ptr(ws), nbytes,
               _ptr(ab), _ptr(info), _stream())
    return (ab, info) if return_info else ab


def _normalizer_floats():
    """The Normalizer's mean and std as six host floats."""
    from .facedp import IMAGENET_MEAN, IMAGENET_STD          # the data path's Normalizer: the one place these constants live
    return _host_floats(tuple(IMAGENET_MEAN) + tuple(IMAGENET_STD))


def _filter_operands(name, pred, guide_rgb):
    """The operands both post-processing filters share: pred [B, n, H, W] (a slice along dim 0 or 1 of a wider tensor is taken as it is,
    through its batch stride), guide_rgb [B, 3, H, W], the Normalizer's constants as six host floats, and a fresh output."""
    _need(pred, guide_rgb, dtypes=_F32, contiguous=False)
    pred, guide_rgb = pred.detach(), guide_rgb.detach()
    if pred.dim() != 4:
        raise DpfError('%s: pred %s is not [B, n, H, W]' % (name, tuple(pred.shape)))
    B, n, H, W = pred.shape
    _match_pred(name, pred, ('guide', guide_rgb, (B, 3, H, W)))
    pred, stride = _batch_view(pred, n * H * W)
    out = torch.empty((B, n, H, W), dtype=torch.float32, device=pred.device)
    return pred, _c(guide_rgb), stride, _normalizer_floats(), out


def guided_filter(pred, guide_rgb, radius, eps):
    """The guided filter of csrc/postprocess.hip (He et al., grey guide, clipped square window of `radius`, 1 <= radius <= 32, eps > 0) on
    every head of pred [B, n, H, W], guided by the luminance of the normalised image guide_rgb [B, 3, H, W] -> a fresh [B, n, H, W].  An
    inference-time operator, not an autograd node: the inputs are detached.  Scratch comes through scratch(), nothing waits on the host."""
    radius = _int_arg('guided_filter', 'radius', radius)
    with torch.no_grad():
        pred, guide_rgb, stride, norm, out = _filter_operands('guided_filter', pred, guide_rgb)
        B, n, H, W = pred.shape
        ws, nbytes = _workspace('dpf_guided_filter_workspace_bytes',
                                'guided_filter: B=%d n=%d H=%d W=%d radius=%d is not supported (1 <= radius <= 32)', B, n, H, W, radius,
                                device=pred.device, tag='postprocess')
        lib().call('dpf_guided_filter', _ptr(pred), stride, _ptr(guide_rgb), B, n, H, W, radius, float(eps), norm, _ptr(ws), nbytes,
                   _ptr(out), _stream())
    return out


def joint_bilateral_filter(pred, guide_rgb, radius, sigma_space, sigma_color):
    """The joint bilateral filter of csrc/postprocess.hip (clipped (2 radius + 1)^2 window, 1 <= radius <= 16, Gaussian weights in space and
    in the guide's luminance) on every head of pred [B, n, H, W] -> a fresh [B, n, H, W].  Detached like guided_filter; needs no scratch."""
    radius = _int_arg('joint_bilateral_filter', 'radius', radius)
    with torch.no_grad():
        pred, guide_rgb, stride, norm, out = _filter_operands('joint_bilateral_filter', pred, guide_rgb)
        B, n, H, W = pred.shape
        lib().call('dpf_joint_bilateral_filter', _ptr(pred), stride, _ptr(guide_rgb), B, n, H, W, radius, float(sigma_space),
                   float(sigma_color), norm, _ptr(out), _stream())
    return out


TARGET_TYPES = {'disp': 0, 'idepth': 1, 'depth': 2}       # the codes of csrc/reconstruct.hip, normal_geo.hip and metrics.hip
MESH_STRIDES = (1, 2, 4, 8)


def _target_code(name, target_type, ab):
    """The code of a known target type; every type but 'depth' needs ab."""
    if target_type not in TARGET_TYPES:
        raise DpfError('%s: target_type must be one of %s, got %r' % (name, sorted(TARGET_TYPES), target_type))
    if ab is None and target_type != 'depth':
        raise DpfError('%s: target_type %r needs ab [B, 2] = [b, a]' % (name, target_type))
    return TARGET_TYPES[target_type]


def _scene_operands(name, pred, target_type, ab, Kmat, mask, near, far):
    """The operands the three surface operators share -> (the leading arguments of the C call, the tensors behind its pointers, (B, H, W)):
    head 0 of pred [B, n, H, W] (or a [B, H, W] map; a slice of a wider tensor is taken as it is, through its batch stride), ab [B, 2] =
    [b, a] (None with target type 'depth'), Kmat [B, 3, 3], mask [B, H, W] or None, and the depth limits (far None: no limit).  The caller
    holds the tensors until its launches are enqueued."""
    code = _target_code(name, target_type, ab)
    _need(pred, Kmat, ab, mask, dtypes=_F32, contiguous=False)
    pred = pred.detach()
    if pred.dim() == 3:
        pred = pred.unsqueeze(1)
    if pred.dim() != 4:
        raise DpfError('%s: pred %s is neither [B, n, H, W] nor [B, H, W]' % (name, tuple(pred.shape)))
    B, n, H, W = pred.shape
    _match_pred(name, pred, ('K', Kmat, (B, 3, 3)), ('ab', ab, (B, 2)), ('mask', mask, (B, H, W)))
    pred, stride = _batch_view(pred, H * W)
    held = (pred, None if ab is None else _c(ab.detach()), _c(Kmat.detach()), None if mask is None else _c(mask.detach()))
    head = (_ptr(held[0]), stride, code, _ptr(held[1]), _ptr(held[2]), _ptr(held[3]), B, H, W, float(near),
            float('inf') if far is None else float(far))
    return head, held, (B, H, W)


def backproject(pred, Kmat, ab=None, mask=None, target_type='disp', near=0.0, far=None):
    """csrc/reconstruct.hip: head 0 of pred [B, n, H, W] (or [B, H, W]) -> points [B, 3, H, W] fp32 = z K^-1 [x, y, 1] (0 where invalid) and
    valid [B, H, W] uint8.  z = a / (pred - b) with ab [B, 2] = [b, a] for 'disp' / 'idepth', z = pred for 'depth'; valid where z is finite,
    near < z < far and mask (None: everywhere) > 0.  An inference-time operator: detached, fresh outputs, nothing read on the host."""
    with torch.no_grad():
        head, held, (B, H, W) = _scene_operands('backproject', pred, target_type, ab, Kmat, mask, near, far)
        points = torch.empty((B, 3, H, W), dtype=torch.float32, device=held[0].device)
        valid = torch.empty((B, H, W), dtype=torch.uint8, device=held[0].device)
        lib().call('dpf_backproject', *head, _ptr(points), _ptr(valid), _stream())
    return points, valid


def depth_normals(pred, Kmat, ab=None, mask=None, target_type='disp', near=0.0, far=None, max_edge_ratio=0.01, towards_camera=True):
    """csrc/reconstruct.hip: geometric normals of the depth of head 0 of pred -> normal [B, 3, H, W] fp32 (unit, or 0 where there is none) and
    normal_valid [B, H, W] uint8.  Per image axis the central step where a pixel is connected to both neighbours
    (|z_p - z_q| <= max_edge_ratio min(z_p, z_q)), the one-sided step to the single connected one otherwise; operands as backproject."""
    with torch.no_grad():
        head, held, (B, H, W) = _scene_operands('depth_normals', pred, target_type, ab, Kmat, mask, near, far)
        normal = torch.empty((B, 3, H, W), dtype=torch.float32, device=held[0].device)
        nvalid = torch.empty((B, H, W), dtype=torch.uint8, device=held[0].device)
        lib().call('dpf_depth_normals', *head, float(max_edge_ratio), int(bool(towards_camera)), _ptr(normal), _ptr(nvalid), _stream())
    return normal, nvalid


def depth_mesh(pred, Kmat, normal_map, ab=None, mask=None, view=None, target_type='disp', stride=1, near=0.0, far=None, max_edge_ratio=0.01,
               towards_camera=True, out=None):
    """csrc/reconstruct.hip: the compacted triangle mesh over every `stride`-th pixel (1, 2, 4 or 8) of head 0 of pred ->
    (vertices [B, Hs Ws, 3] fp32, vertex_normals [B, Hs Ws, 3] fp32 gathered from normal_map [B, 3, H, W], vertex_colours [B, Hs Ws, 3] uint8
    from the normalised view [B, 3, H, W] (None: 255), faces [B, 2 (Hs - 1)(Ws - 1), 3] int32 with sample-local indices, counts [B, 2] int32 =
    (vertices, faces)).  The buffers are worst-case sized and entries past the counts are left as torch.empty (or `out`, a tuple of the five
    to write into) had them; counts stays on the device: nothing is read on the host."""
    stride = _int_arg('depth_mesh', 'stride', stride)
    with torch.no_grad():
        head, held, (B, H, W) = _scene_operands('depth_mesh', pred, target_type, ab, Kmat, mask, near, far)
        _need(normal_map, view, dtypes=_F32, contiguous=False)
        if normal_map is None:
            raise DpfError('depth_mesh: normal_map [B, 3, H, W] is needed')
        _match_pred('depth_mesh', held[0], ('normal_map', normal_map, (B, 3, H, W)), ('view', view, (B, 3, H, W)))
        nmap, view = _c(normal_map.detach()), None if view is None else _c(view.detach())
        dev = held[0].device
        ws, nbytes = _workspace('dpf_depth_mesh_workspace_bytes', 'depth_mesh: B=%d H=%d W=%d stride=%d is not supported (stride 1, 2, 4 or 8)',
                                B, H, W, stride, device=dev, tag='reconstruct')
        Hs, Ws = -(-H // stride), -(-W // stride)
        if out is None:
            out = (torch.empty((B, Hs * Ws, 3), dtype=torch.float32, device=dev), torch.empty((B, Hs * Ws, 3), dtype=torch.float32, device=dev),
                   torch.empty((B, Hs * Ws, 3), dtype=torch.uint8, device=dev),
                   torch.empty((B, 2 * (Hs - 1) * (Ws - 1), 3), dtype=torch.int32, device=dev), torch.empty((B, 2), dtype=torch.int32, device=dev))
        want = ((B, Hs * Ws, 3), (B, Hs * Ws, 3), (B, Hs * Ws, 3), (B, 2 * (Hs - 1) * (Ws - 1), 3), (B, 2))
        kinds = (torch.float32, torch.float32, torch.uint8, torch.int32, torch.int32)
        for t, shape, kind in zip(out, want, kinds):
            if tuple(t.shape) != shape or t.dtype != kind or not t.is_cuda or not t.is_contiguous():
                raise DpfError('depth_mesh: an output buffer %s %s is not the contiguous %s %s the shape asks for'
                               % (tuple(t.shape), t.dtype, shape, kind))
        vertices, vnormals, vcolours, faces, counts = out
        lib().call('dpf_depth_mesh', *head[:6], _ptr(nmap), _ptr(view), _normalizer_floats(), *head[6:9], stride, head[9], head[10],
                   float(max_edge_ratio), int(bool(towards_camera)), _ptr(ws), nbytes, _ptr(vertices), _ptr(vnormals), _ptr(vcolours),
                   _ptr(faces), _ptr(counts), _stream())
    return vertices, vnormals, vcolours, faces, counts


NORMAL_REFINE_MAX_ITERATIONS = 256
NORMAL_REFINE_STATS = 3     # doubles per sample ahead of rho_1 .. rho_iterations: valid pixels, edges, rho_0


def normal_refine(pred, Kmat, normal, ab=None, mask=None, target_type='disp', near=0.0, far=None, max_edge_ratio=0.01, min_cos=0.1, lam=0.1,
                  iterations=32, normal_signs=(1, 1, 1), stats=False, out=None):
    """csrc/normal_refine.hip: head 0 of pred [B, n, H, W] (or [B, H, W]) brought into agreement with normal [B, 3, H, W] -> a fresh tensor of
    pred's shape (or `out`, a contiguous one of that shape), the other heads copied.  Per sample the log-depth correction delta minimising
    lam sum delta^2 + sum over the edges of (delta_q - delta_p - e_pq)^2, e_pq the difference between the step the normals predict and the
    one the depth takes (include/dpf_hip.h), by `iterations` (1 .. 256) of Jacobi-preconditioned conjugate gradients on the device; edges
    join valid neighbours within max_edge_ratio of each other whose normal (normal_signs * normal) meets both rays at a cosine of at
    least min_cos.  Invalid pixels keep their value bit for bit.  With stats also float64 [B, 3 + iterations]: valid pixels, edges,
    rho_0 .. rho_iterations.  An inference-time operator: detached, no gradient, nothing read on the host."""
    iterations = _int_arg('normal_refine', 'iterations', iterations)
    signs = tuple(float(v) for v in normal_signs)
    if len(signs) != 3 or any(v not in (1.0, -1.0) for v in signs):
        raise DpfError('normal_refine: normal_signs must be three values of +1 or -1, got %r' % (normal_signs,))
    for name, v, ok in (('max_edge_ratio', max_edge_ratio, float(max_edge_ratio) > 0), ('lam', lam, 0 < float(lam) < float('inf')),
                        ('min_cos', min_cos, 0 <= float(min_cos) < 1),
                        ('iterations', iterations, 1 <= iterations <= NORMAL_REFINE_MAX_ITERATIONS)):
        if not ok:
            raise DpfError('normal_refine: %s = %r is outside its range (max_edge_ratio > 0, lam > 0, 0 <= min_cos < 1, iterations 1 .. %d)'
                           % (name, v, NORMAL_REFINE_MAX_ITERATIONS))
    with torch.no_grad():
        head, held, (B, H, W) = _scene_operands('normal_refine', pred, target_type, ab, Kmat, mask, near, far)
        _need(normal, out, dtypes=_F32, contiguous=False)
        if normal is None:
            raise DpfError('normal_refine: normal [B, 3, H, W] is needed')
        _match_pred('normal_refine', held[0], ('normal', normal, (B, 3, H, W)))
        shape = tuple(pred.shape)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=held[0].device)
        elif tuple(out.shape) != shape or not out.is_contiguous():
            raise DpfError('normal_refine: out %s is not a contiguous tensor of pred\'s shape %s' % (tuple(out.shape), shape))
        nmap = _c(normal.detach())
        planes = out.view(B, -1, H, W)
        if planes.shape[1] > 1:
            planes[:, 1:].copy_(pred.detach()[:, 1:])
        ws, nbytes = _workspace('dpf_normal_refine_workspace_bytes', 'normal_refine: B=%d H=%d W=%d is not supported', B, H, W,
                                device=held[0].device, tag='normal_refine')
        record = torch.empty((B, NORMAL_REFINE_STATS + iterations), dtype=torch.float64, device=held[0].device) if stats else None
        lib().call('dpf_normal_refine', *head[:6], _ptr(nmap), _host_floats(signs), *head[6:], float(max_edge_ratio), float(min_cos),
                   float(lam), iterations, _ptr(ws), nbytes, _ptr(out), planes.shape[1] * H * W, _ptr(record), _stream())
    return (out, record) if stats else out


SHADING_STATS = 16          # doubles per sample: counted, valid, passes, sum w, RMS pass 0 [4, 7), RMS last [7, 10), albedo error [10, 13), compared
SHADING_MAX_ITERATIONS = 8
SHADING_ORDERS = (1, 2)
SHADING_SIGN_PARITY = (1, -1, 1, 1, -1, -1, 1, 1, 1)      # what normal_signs [1, -1, 1] does to the nine coefficients: the basis odd in y
SHADING_CHUNK, SHADING_MAX_ROWS, SHADING_FOLD = 1024, 512, 256      # kChunk, kMaxRows of csrc/shading.hip and the fold's threads (dpf_reduce.h)


def shading_rows(H, W):
    """(partial rows per sample, pixels per workgroup) of csrc/shading.hip's passes over an H x W plane: a workgroup walks at least
    SHADING_CHUNK pixels, more (a multiple of 256) once a sample would need more than SHADING_MAX_ROWS rows."""
    n = H * W
    rows = min(max(-(-n // SHADING_CHUNK), 1), SHADING_MAX_ROWS)
    per_block = -(-(-(-n // rows)) // 256) * 256
    return -(-n // per_block), per_block


def _shading_operands(name, view, normal, mask, normal_signs, order, gamma, min_value, max_value):
    """The operands both shading calls share -> (the leading arguments of the C call, the tensors behind its pointers, (B, H, W)):
    the normalised view and the normal map, both [B, 3, H, W], mask [B, H, W] or None, the Normalizer's six host floats and the signs."""
    order = _int_arg(name, 'order', order, SHADING_ORDERS)
    signs = tuple(float(v) for v in normal_signs)
    if len(signs) != 3 or any(v not in (1.0, -1.0) for v in signs):
        raise DpfError('%s: normal_signs must be three values of +1 or -1, got %r' % (name, normal_signs))
    _need(view, normal, mask, dtypes=_F32, contiguous=False)
    if view is None or normal is None or view.dim() != 4 or view.shape[1] != 3:
        raise DpfError('%s: view [B, 3, H, W] and normal [B, 3, H, W] are needed' % name)
    B, _, H, W = view.shape
    _match_pred(name, view, ('normal', normal, (B, 3, H, W)), ('mask', mask, (B, H, W)))
    held = (_c(view.detach()), _c(normal.detach()), None if mask is None else _c(mask.detach()))
    head = (_ptr(held[0]), _ptr(held[1]), _ptr(held[2]), _normalizer_floats(), _host_floats(signs))
    return head, held, (B, H, W), (order, float(gamma), float(min_value), float(max_value))


def shading_fit(view, normal, mask=None, order=2, gamma=2.2, min_value=0.02, max_value=0.98, iterations=3, f_scale=0.05, ridge=1e-6,
                min_pixels=72, normal_signs=(1, 1, 1), gram=False):
    """csrc/shading.hip: per sample the spherical-harmonics lighting (order 1: 4 coefficients, order 2: 9) that explains the linear
    intensity of the normalised view [B, 3, H, W] under normal [B, 3, H, W] (normal_signs * normal, normalised) -> (light [B, 3, 9] fp32,
    stats [B, 16] fp64), and with `gram` also the [B, 16, 16] fp64 Gram matrix of the last pass.  Iteratively reweighted least squares
    with `iterations` (0 .. 8) reweighted passes over the pixels with mask > 0 (None: all), a usable normal and every channel within
    [min_value, max_value]; the definitions are in include/dpf_hip.h.  A sample with fewer than min_pixels such pixels, or a singular
    system, gets light 0 and stats[:, 1] = 0.  An inference-time operator: detached, nothing read on the host."""
    iterations, min_pixels = _int_arg('shading_fit', 'iterations', iterations), _int_arg('shading_fit', 'min_pixels', min_pixels)
    with torch.no_grad():
        head, held, (B, H, W), pix = _shading_operands('shading_fit', view, normal, mask, normal_signs, order, gamma, min_value, max_value)
        dev = held[0].device
        ws, nbytes = _workspace('dpf_shading_workspace_bytes', 'shading_fit: B=%d H=%d W=%d is not supported', B, H, W, device=dev, tag='shading')
        light = torch.empty((B, 3, 9), dtype=torch.float32, device=dev)
        stats = torch.empty((B, SHADING_STATS), dtype=torch.float64, device=dev)
        G = torch.empty((B, 16, 16), dtype=torch.float64, device=dev) if gram else None
        lib().call('dpf_shading_fit', *head, B, H, W, *pix, iterations, float(f_scale), float(ridge), min_pixels, _ptr(ws), nbytes,
                   _ptr(light), _ptr(stats), _ptr(G), _stream())
    return (light, stats, G) if gram else (light, stats)


def shading_rotation(rotate_deg):
    """R = Rz Ry Rx of the three angles in degrees, formed in fp64 -> nine row-major numbers."""
    import math
    ax, ay, az = (math.radians(float(v)) for v in rotate_deg)
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = ((1.0, 0.0, 0.0), (0.0, cx, -sx), (0.0, sx, cx))
    Ry = ((cy, 0.0, sy), (0.0, 1.0, 0.0), (-sy, 0.0, cy))
    Rz = ((cz, -sz, 0.0), (sz, cz, 0.0), (0.0, 0.0, 1.0))
    mul = lambda P, Q: tuple(tuple(sum(P[i][k] * Q[k][j] for k in range(3)) for j in range(3)) for i in range(3))
    return tuple(v for row in mul(Rz, mul(Ry, Rx)) for v in row)


def shading_apply(view, normal, light, mask=None, stats=None, albedo_label=None, order=2, gamma=2.2, min_value=0.02, max_value=0.98,
                  shade_floor=0.05, albedo_max=4.0, normal_signs=(1, 1, 1), relight=False, rotate_deg=(0, 0, 0), coefficients=None, gain=1.0):
    """csrc/shading.hip: the planes of light [B, 3, 9] (shading_fit's) over the view and the normals it was fitted to -> a dict of
    'shading' and 'albedo' [B, 3, H, W] fp32, 'shading_valid' [B, H, W] uint8 and, with `relight`, 'relit' [B, 3, H, W]: the encoded view
    in [0, 1] under the light rotated by rotate_deg (degrees about x, y, z; R = Rz Ry Rx) or replaced by `coefficients` ([3][9] numbers),
    times gain.  stats: shading_fit's record -- samples it flags invalid get planes of 0 and keep their view -- and with albedo_label
    ([B, 3, H, W] or [B, H, W]) its entries 10..13 receive the scale-invariant albedo error.  Detached, nothing read on the host."""
    with torch.no_grad():
        head, held, (B, H, W), pix = _shading_operands('shading_apply', view, normal, mask, normal_signs, order, gamma, min_value, max_value)
        _need(light, albedo_label, dtypes=_F32, contiguous=False)
        _need(stats, dtypes=(torch.float64,))
        if light is None:
            raise DpfError('shading_apply: light [B, 3, 9] is needed')
        _match_pred('shading_apply', held[0], ('light', light, (B, 3, 9)), ('stats', stats, (B, SHADING_STATS)))
        channels = 3
        if albedo_label is not None:
            if albedo_label.dim() == 3:
                albedo_label = albedo_label.unsqueeze(1)
            channels = albedo_label.shape[1] if albedo_label.dim() == 4 else 0
            if channels not in (1, 3):
                raise DpfError('shading_apply: albedo_label %s is neither [B, 3, H, W] nor [B, H, W]' % (tuple(albedo_label.shape),))
            _match_pred('shading_apply', held[0], ('albedo_label', albedo_label, (B, channels, H, W)))
            albedo_label = _c(albedo_label.detach())
        coeff = None
        if coefficients is not None:
            flat = [float(v) for row in coefficients for v in row]
            if len(coefficients) != 3 or len(flat) != 27:
                raise DpfError('shading_apply: coefficients must be [3][9] numbers')
            coeff = _host_floats(flat)
        dev = held[0].device
        light = _c(light.detach())
        ws, nbytes = _workspace('dpf_shading_workspace_bytes', 'shading_apply: B=%d H=%d W=%d is not supported', B, H, W, device=dev, tag='shading')
        out = {'shading': torch.empty((B, 3, H, W), dtype=torch.float32, device=dev),
               'albedo': torch.empty((B, 3, H, W), dtype=torch.float32, device=dev),
               'shading_valid': torch.empty((B, H, W), dtype=torch.uint8, device=dev)}
        if relight:
            out['relit'] = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
        lib().call('dpf_shading_apply', *head, _ptr(light), _ptr(stats), _ptr(albedo_label), channels, B, H, W, *pix, float(shade_floor),
                   float(albedo_max), int(bool(relight)), coeff, _host_floats(shading_rotation(rotate_deg)), float(gain), _ptr(ws), nbytes,
                   _ptr(out['shading']), _ptr(out['albedo']), _ptr(out['shading_valid']), _ptr(out.get('relit')), _stream())
    return out


REFOCUS_STATS = 8           # doubles per sample: d_f, counted pixels, valid flag, near sign used, min c, max c, then 0
REFOCUS_FOCUS = {'mask_mean': 0, 'point': 1, 'value': 2}      # the focus codes of csrc/refocus.hip
REFOCUS_RADII = range(1, 33)
REFOCUS_TILE = 16           # kCell of csrc/refocus.hip: the side of a plan cell and of a render tile


def refocus_focus_pixel(focus_point, H, W):
    """The pixel (x, y) nearest focus_point = [u, v], fractions of width and height (pixel centres at (x + 0.5) / W)."""
    import math
    u, v = (float(f) for f in focus_point)
    return min(W - 1, max(0, int(math.floor(u * W)))), min(H - 1, max(0, int(math.floor(v * H))))


def refocus(view, disparity, mask=None, ab=None, target_type='disp', source=None, focus='mask_mean', focus_point=(0.5, 0.5), focus_value=0.0,
            aperture=4.0, max_radius=16, near_sign='auto', gamma=2.2, gain=1.0):
    """csrc/refocus.hip: the normalised view [B, 3, H, W] rendered again through a virtual aperture, from head 0 of disparity [B, n, H, W]
    (or [B, H, W]; a slice of a wider tensor is taken as it is) -> a dict of 'refocused' [B, 3, H, W] fp32 in [0, 1], 'defocus' [B, H, W]
    fp32 (the signed blur radius c in pixels) and 'refocus_stats' [B, 8] fp64 (REFOCUS_STATS).  Under target_type 'disp' the map is the
    defocus disparity d = a / z + b itself, and so it is under 'idepth' (backproject reads both as z = a / (map - b)); under 'depth'
    d = a / map + b.  ab [B, 2] = [b, a] is needed for 'idepth' and 'depth', and decides the near sign under 'auto'.  `source`: an encoded image [B, 3, H, W] in
    [0, 1] (results['relit']) that is refocused in place of the view.  focus: 'mask_mean' (d_f = the mean of d over mask > 0 and finite),
    'point' (d at the pixel nearest focus_point) or 'value' (focus_value).  near_sign: 'auto' (the sign of a where ab is given, else +1),
    1 or -1.  The definitions are in include/dpf_hip.h.  An inference-time operator: detached, scratch through scratch(), nothing read
    on the host."""
    max_radius = _int_arg('refocus', 'max_radius', max_radius)
    if max_radius not in REFOCUS_RADII:
        raise DpfError('refocus: max_radius must be an integer from 1 to 32, got %r' % (max_radius,))
    if focus not in REFOCUS_FOCUS:
        raise DpfError('refocus: focus must be one of %s, got %r' % (sorted(REFOCUS_FOCUS), focus))
    if near_sign != 'auto' and (isinstance(near_sign, bool) or near_sign not in (1, -1)):
        raise DpfError("refocus: near_sign must be 'auto', 1 or -1, got %r" % (near_sign,))
    if target_type not in TARGET_TYPES:
        raise DpfError('refocus: target_type must be one of %s, got %r' % (sorted(TARGET_TYPES), target_type))
    if ab is None and target_type != 'disp':
        raise DpfError('refocus: target_type %r needs ab [B, 2] = [b, a] to become a defocus disparity' % (target_type,))
    code = TARGET_TYPES[target_type]
    with torch.no_grad():
        _need(view, disparity, mask, ab, source, dtypes=_F32, contiguous=False)
        if view is None or disparity is None or view.dim() != 4 or view.shape[1] != 3:
            raise DpfError('refocus: view [B, 3, H, W] and disparity [B, n, H, W] are needed')
        B, _, H, W = view.shape
        pred = disparity.detach()
        if pred.dim() == 3:
            pred = pred.unsqueeze(1)
        if pred.dim() != 4 or (pred.shape[0], pred.shape[2], pred.shape[3]) != (B, H, W):
            raise DpfError('refocus: disparity %s is neither [B, n, H, W] nor [B, H, W] of view %s' % (tuple(disparity.shape), tuple(view.shape)))
        _match_pred('refocus', view, ('mask', mask, (B, H, W)), ('ab', ab, (B, 2)), ('source', source, (B, 3, H, W)))
        pred, stride = _batch_view(pred, H * W)
        image = _c((view if source is None else source).detach())
        mask, ab = None if mask is None else _c(mask.detach()), None if ab is None else _c(ab.detach())
        fx, fy = refocus_focus_pixel(focus_point, H, W)
        dev = image.device
        ws, nbytes = _workspace('dpf_refocus_workspace_bytes', 'refocus: B=%d H=%d W=%d is not supported', B, H, W, device=dev, tag='refocus')
        out = {'refocused': torch.empty((B, 3, H, W), dtype=torch.float32, device=dev),
               'defocus': torch.empty((B, H, W), dtype=torch.float32, device=dev),
               'refocus_stats': torch.empty((B, REFOCUS_STATS), dtype=torch.float64, device=dev)}
        lib().call('dpf_refocus_plan', _ptr(pred), stride, code, _ptr(ab), _ptr(mask), B, H, W, REFOCUS_FOCUS[focus], fx, fy, float(focus_value),
                   float(aperture), max_radius, 0 if near_sign == 'auto' else int(near_sign), _ptr(ws), nbytes, _ptr(out['defocus']),
                   _ptr(out['refocus_stats']), _stream())
        lib().call('dpf_refocus_render', _ptr(image), int(source is None), _normalizer_floats(), _ptr(out['defocus']), _ptr(out['refocus_stats']),
                   B, H, W, max_radius, float(gamma), float(gain), _ptr(ws), nbytes, _ptr(out['refocused']), _stream())
    return out


DP_RENDER_STATS = 8         # doubles per sample: finite pixels, pixels clamped at max_radius, min c, max c, then 0
DP_RENDER_RADII = range(1, 33)
DP_RENDER_TILE = 16         # kCell of csrc/dp_render.hip: the side of a plan cell and of a render tile
DP_RENDER_OUTPUTS = ('normalised', 'encoded')
DP_RENDER_SHIFT = (0.0, -2.0)                                   # the photometric block's default
DP_RENDER_HALF_DISC = 3.0 * 3.14159265358979323846 / 8.0       # radius_scale / |shift|: the centroid of a half disc is 4 r / (3 pi) off centre


def dp_render_radius_scale(shift, radius_scale=None):
    """rho: radius_scale, or (3 pi / 8) |shift| for None -- the half discs of radius rho |d| then have centroids |shift| |d| apart."""
    import math
    return DP_RENDER_HALF_DISC * math.hypot(float(shift[0]), float(shift[1])) if radius_scale is None else float(radius_scale)


def dp_render(image, disparity, shift=DP_RENDER_SHIFT, radius_scale=None, max_radius=16, near_sign=1, gamma=2.2, normalised=True,
              output='normalised'):
    """csrc/dp_render.hip: the two half-aperture views of the all-in-focus image [B, 3, H, W] (normalised, or encoded in [0, 1] under
    normalised=False) under the signed defocus disparity [B, H, W] (zero in focus; a pixel that is not finite is copied through) -> a dict
    of 'reference' and 'target' [B, 3, H, W] fp32 (normalised again, or encoded under output 'encoded'), 'radius' [B, H, W] fp32 (the
    signed blur radius c in pixels) and 'dp_stats' [B, 8] fp64 (DP_RENDER_STATS).  reference(p) is target(p + shift d): what
    photometric_loss samples under the same shift.  near_sign (+1: larger d is nearer) enters the occlusion rule only.  The definitions
    are in include/dpf_hip.h.  No gradient: detached, scratch through scratch(), nothing read on the host."""
    import math
    max_radius = _int_arg('dp_render', 'max_radius', max_radius)
    if max_radius not in DP_RENDER_RADII:
        raise DpfError('dp_render: max_radius must be an integer from 1 to 32, got %r' % (max_radius,))
    if isinstance(near_sign, bool) or near_sign not in (1, -1):
        raise DpfError('dp_render: near_sign must be 1 or -1, got %r' % (near_sign,))
    if output not in DP_RENDER_OUTPUTS:
        raise DpfError('dp_render: output must be one of %s, got %r' % (list(DP_RENDER_OUTPUTS), output))
    try:
        sx, sy = (float(v) for v in shift)
    except (TypeError, ValueError):
        raise DpfError('dp_render: shift must be two finite numbers (x, y), not both 0, got %r' % (shift,))
    if not (math.isfinite(sx) and math.isfinite(sy)) or (sx == 0 and sy == 0):
        raise DpfError('dp_render: shift must be two finite numbers (x, y), not both 0, got %r' % (shift,))
    rho = dp_render_radius_scale((sx, sy), radius_scale)
    with torch.no_grad():
        _need(image, disparity, dtypes=_F32, contiguous=False)
        if image is None or disparity is None or image.dim() != 4 or image.shape[1] != 3:
            raise DpfError('dp_render: image [B, 3, H, W] and disparity [B, H, W] are needed')
        B, _, H, W = image.shape
        if tuple(disparity.shape) != (B, H, W):
            raise DpfError('dp_render: disparity %s is not [B, H, W] of image %s' % (tuple(disparity.shape), tuple(image.shape)))
        image, disparity = _c(image.detach()), _c(disparity.detach())
        dev = image.device
        ws, nbytes = _workspace('dpf_dp_render_workspace_bytes', 'dp_render: B=%d H=%d W=%d is not supported', B, H, W, device=dev, tag='dp_render')
        out = {'reference': torch.empty((B, 3, H, W), dtype=torch.float32, device=dev),
               'target': torch.empty((B, 3, H, W), dtype=torch.float32, device=dev),
               'radius': torch.empty((B, H, W), dtype=torch.float32, device=dev),
               'dp_stats': torch.empty((B, DP_RENDER_STATS), dtype=torch.float64, device=dev)}
        lib().call('dpf_dp_render_plan', _ptr(disparity), B, H, W, rho, max_radius, _ptr(ws), nbytes, _ptr(out['radius']), _ptr(out['dp_stats']),
                   _stream())
        lib().call('dpf_dp_render', _ptr(image), int(bool(normalised)), _normalizer_floats(), _ptr(disparity), _ptr(out['radius']), B, H, W, sx, sy,
                   max_radius, int(near_sign), float(gamma), int(output == 'normalised'), _ptr(ws), nbytes, _ptr(out['reference']),
                   _ptr(out['target']), _stream())
    return out


NORMAL_GEO_STEPS = (1, 2, 4)
NORMAL_GEO_STATS = 16      # doubles the forward leaves for the backward: count per head [0, 8), term sum per head [8, 16)


_NORMAL_GEO = _HeadLoss('normal_geo_loss', 'dpf_normal_geo', 'BnHW', NORMAL_GEO_STATS,
                        extras=lambda B, n, H, W: (((B, n, 3, H, W), torch.float32), ((B, n, H, W), torch.uint8)))


def normal_geo_loss(pred, depth, normal, Kmat, ab=None, mask=None, head_weights=(1.0,), target_type='disp', max_edge_ratio=0.01, step=1,
                    towards_camera=True, target_signs=(1, 1, 1), return_normals=False):
    """csrc/normal_geo.hip: the normals of the depth every head of pred [B, n <= 8, H, W] predicts against normal [B, 3, H, W] -> the 0-dim
    loss sum_h w_h mean over the counted pixels of 1 - clamp(n . g^, -1, 1), g = target_signs * normal.  depth
    [B, H, W] is the target depth: it decides which pixels are usable and which neighbours (`step` = 1, 2 or 4 pixels away) lie on one
    surface, the predicted depth a / (pred - b) (ab [B, 2] = [b, a]; pred itself for target type 'depth') gives the step vectors.  The
    gradient reaches pred only.  With return_normals also normal [B, n, 3, H, W] fp32 and counted [B, n, H, W] uint8."""
    code = _target_code('normal_geo_loss', target_type, ab)
    _need(pred, depth, normal, Kmat, ab, mask, dtypes=_F32, contiguous=False)
    if pred.dim() != 4:
        raise DpfError('normal_geo_loss: pred %s is not [B, n, H, W]' % (tuple(pred.shape),))
    B, n, H, W = pred.shape
    _match_pred('normal_geo_loss', pred, ('depth', depth, (B, H, W)), ('normal', normal, (B, 3, H, W)), ('K', Kmat, (B, 3, 3)), ('ab', ab, (B, 2)),
                ('mask', mask, (B, H, W)))
    if len(head_weights) != n:
        raise DpfError('normal_geo_loss: %d head weights for %d heads' % (len(head_weights), n))
    step = _int_arg('normal_geo_loss', 'step', step, NORMAL_GEO_STEPS)
    signs = tuple(float(v) for v in target_signs)
    if len(signs) != 3 or any(v not in (1.0, -1.0) for v in signs):
        raise DpfError('normal_geo_loss: target_signs must be three values of +1 or -1, got %r' % (target_signs,))
    if not float(max_edge_ratio) > 0:
        raise DpfError('normal_geo_loss: max_edge_ratio must be positive, got %r' % (max_edge_ratio,))
    pred = _c(pred)
    held = tuple(None if t is None else _c(t.detach()) for t in (depth, normal, Kmat, None if target_type == 'depth' else ab, mask))
    lead = (_ptr(pred), *[_ptr(t) for t in held], B, n, H, W, code, float(max_edge_ratio), step, int(bool(towards_camera)),
            _host_floats(signs), _host_floats(head_weights))
    return HeadLossFn.apply(pred, _NORMAL_GEO, held, lead, bool(return_normals))


PHOTOMETRIC_STATS = 16      # doubles: count per head [0, 8), term sum per head [8, 16)
SMOOTHNESS_STATS = 32       # doubles: x-pair count [0, 8) and sum [8, 16), y-pair count [16, 24) and sum [24, 32)


_PHOTOMETRIC = _HeadLoss('photometric_loss', 'dpf_photometric', 'BnHW', PHOTOMETRIC_STATS,
                         aux=lambda B, n, H, W: ((2, B, H, W),),      # the luminance planes of both views
                         extras=lambda B, n, H, W: (((B, n, H, W), torch.float32), ((B, n, H, W), torch.uint8)))
_SMOOTHNESS = _HeadLoss('smoothness_loss', 'dpf_smoothness', 'BnHW', SMOOTHNESS_STATS, aux=lambda B, n, H, W: ((B, H, W),))


def _label_free_operands(name, pred, images, ab, mask, head_weights):
    """The operands the two label-free losses share, checked: pred [B, n, H, W], the named images [B, 3, H, W], ab [B, 2], mask [B, H, W]
    and one weight per head -> (contiguous pred, the detached contiguous images, ab, mask, the weights as floats)."""
    _need(pred, ab, mask, *[t for _, t in images], dtypes=_F32, contiguous=False)
    if pred.dim() != 4:
        raise DpfError('%s: pred %s is not [B, n, H, W]' % (name, tuple(pred.shape)))
    B, n, H, W = pred.shape
    for key, t in images:
        if t is None:
            raise DpfError('%s: %s [B, 3, H, W] is needed' % (name, key))
    _match_pred(name, pred, *[(key, t, (B, 3, H, W)) for key, t in images], ('ab', ab, (B, 2)), ('mask', mask, (B, H, W)))
    if len(head_weights) != n:
        raise DpfError('%s: %d head weights for %d heads' % (name, len(head_weights), n))
    held = [None if t is None else _c(t.detach()) for t in [t for _, t in images] + [ab, mask]]
    return _c(pred), held[:-2], held[-2], held[-1], tuple(float(w) for w in head_weights)


def photometric_loss(pred, ref_rgb, tgt_rgb, ab=None, mask=None, head_weights=(1.0,), target_type='disp', shift=(0.0, -2.0), alpha=0.85,
                     eps=1e-3, return_warped=False):
    """csrc/photometric.hip: the luminance of tgt_rgb [B, 3, H, W] sampled bilinearly at (x + shift[0] D, y + shift[1] D) against the
    luminance of ref_rgb, for every head of pred [B, n <= 8, H, W] -> the 0-dim loss sum_h w_h mean over the counted pixels of
    alpha clamp((1 - SSIM_3x3) / 2, 0, 1) + (1 - alpha) sqrt((J - I)^2 + eps^2).  D = pred for 'disp' / 'idepth',
    a / pred + b for 'depth' (ab [B, 2] = [b, a], needed then only).  A pixel is counted when the nine pixels of its window are warpable:
    pred finite, mask (None: everywhere) > 0, the sample point inside the image.  The gradient reaches pred only.  With return_warped also
    the warped luminance [B, n, H, W] fp32 (0 where not warpable) and counted [B, n, H, W] uint8."""
    code = _target_code('photometric_loss', target_type, ())       # the name only: here the conversion is needed the other way round,
    if target_type == 'depth' and ab is None:                      # from a depth to the displacement
        raise DpfError("photometric_loss: target_type 'depth' needs ab [B, 2] = [b, a]")
    pred, (ref_rgb, tgt_rgb), ab, mask, weights = _label_free_operands('photometric_loss', pred, (('ref_rgb', ref_rgb), ('tgt_rgb', tgt_rgb)),
                                                                       ab if target_type == 'depth' else None, mask, head_weights)
    shift = tuple(float(v) for v in shift)
    if len(shift) != 2 or any(v != v or v in (float('inf'), -float('inf')) for v in shift) or shift == (0.0, 0.0):
        raise DpfError('photometric_loss: shift must be two finite numbers (x, y), not both 0, got %r' % (shift,))
    if not 0.0 <= float(alpha) <= 1.0:
        raise DpfError('photometric_loss: alpha must lie in [0, 1], got %r' % (alpha,))
    if not 0.0 < float(eps) < float('inf'):
        raise DpfError('photometric_loss: eps must be positive, got %r' % (eps,))
    held = (ref_rgb, tgt_rgb, ab, mask)
    lead = (_ptr(pred), *[_ptr(t) for t in held], *pred.shape, code, shift[0], shift[1], float(alpha), float(eps), _normalizer_floats(),
            _host_floats(weights))
    return HeadLossFn.apply(pred, _PHOTOMETRIC, held, lead, bool(return_warped))


def smoothness_loss(pred, guide_rgb, mask=None, head_weights=(1.0,), gamma=10.0, eps=1e-3):
    """csrc/photometric.hip: the edge-aware first-order smoothness of every head of pred [B, n <= 8, H, W] under the luminance Y of
    guide_rgb [B, 3, H, W] -> the 0-dim loss sum_h w_h (mean over the x-pairs + mean over the y-pairs) of
    sqrt((pred_q - pred_p)^2 + eps^2) exp(-gamma |Y_q - Y_p|), a pair being two pixels one apart whose pred are finite and whose mask
    (None: everywhere) is > 0.  The gradient reaches pred only."""
    pred, (guide_rgb,), _, mask, weights = _label_free_operands('smoothness_loss', pred, (('guide_rgb', guide_rgb),), None, mask, head_weights)
    if not 0.0 <= float(gamma) < float('inf'):
        raise DpfError('smoothness_loss: gamma must be a finite number >= 0, got %r' % (gamma,))
    if not 0.0 < float(eps) < float('inf'):
        raise DpfError('smoothness_loss: eps must be positive, got %r' % (eps,))
    held = (guide_rgb, mask)
    lead = (_ptr(pred), *[_ptr(t) for t in held], *pred.shape, float(gamma), float(eps), _normalizer_floats(), _host_floats(weights))
    return HeadLossFn.apply(pred, _SMOOTHNESS, held, lead, False)


MULTIVIEW_STATS = 136       # doubles: count per (head, view) [8 h + v], term sums [64 + 8 h + v], views counted per head [128 + h]
MULTIVIEW_MAX_VIEWS = 8


class MultiviewFn(torch.autograd.Function):
    """HeadLossFn for the loss whose shape has a view axis beside pred's (csrc/multiview.hip): -> 0-dim loss, and with want_extras
    warped, counted, sample_xy and the luminance planes.  The C argument orders agree as in that family: forward `lead | ws, nbytes | luma
    | stats, out | extras`, backward `lead | luma | stats, gout, dpred`.  The rig, the workspace, stats and the planes are fresh tensors
    (rig, planes and stats are saved for the backward), gout is read on the device and nothing is read on the host, so the call is
    capturable inside the train-step graph.  Only pred receives a gradient."""

    @staticmethod
    def forward(ctx, pred, held, rig, lead, dims, want_extras):
        B, n, S, H, W, Hs, Ws = dims
        dev = pred.device
        ws, nbytes = _workspace('dpf_multiview_workspace_bytes', 'multiview_loss: shape B=%d n=%d S=%d H=%d W=%d is not supported', B, n, S, H, W,
                                device=dev)
        stats = torch.empty(MULTIVIEW_STATS, dtype=torch.float64, device=dev)
        out = torch.empty((), dtype=torch.float32, device=dev)
        luma = torch.empty(B * H * W + B * S * Hs * Ws, dtype=torch.float32, device=dev)
        extras = [None, None, None]
        if want_extras:
            extras = [torch.empty((B, n, S, H, W), dtype=torch.float32, device=dev), torch.empty((B, n, S, H, W), dtype=torch.uint8, device=dev),
                      torch.empty((B, n, S, 2, H, W), dtype=torch.float32, device=dev)]
        lib().call('dpf_multiview_forward', *lead, _ptr(ws), nbytes, _ptr(luma), _ptr(stats), _ptr(out), *[_ptr(t) for t in extras], _stream())
        ctx.save_for_backward(pred, stats, luma, rig, *held)
        ctx.lead = lead
        if want_extras:
            planes = (luma[:B * H * W].view(B, H, W), luma[B * H * W:].view(B, S, Hs, Ws))
            ctx.mark_non_differentiable(*extras, *planes)
            return (out,) + tuple(extras) + planes
        return out

    @staticmethod
    def backward(ctx, gout, *unused):
        pred, stats, luma = ctx.saved_tensors[:3]
        gout = _c(gout)
        _need(gout)
        dpred = torch.empty_like(pred)
        lib().call('dpf_multiview_backward', *ctx.lead, _ptr(luma), _ptr(stats), _ptr(gout), _ptr(dpred), _stream())
        return dpred, None, None, None, None, None


MULTIVIEW_REDUCE = {'mean': 0, 'min': 1}
MULTIVIEW_VISIBILITY = {'none': 0, 'zbuffer': 1}
MULTIVIEW_CELLS = (1, 2, 4)


class MultiviewOccFn(torch.autograd.Function):
    """MultiviewFn with occlusion handling on (reduce 'min' and / or visibility 'zbuffer'; csrc/multiview.hip): the same argument orders
    with `mode` = (reduce, visibility, cell, tolerance) after the lead, the z-buffer and the selection plane after luma.  Both are fresh
    tensors saved for the backward beside the planes (None where their mode is off); the workspace may be overwritten between the passes.
    With want_extras the plain extras, then visible, selected (reduce 'min') and zbuffer (visibility 'zbuffer')."""

    @staticmethod
    def forward(ctx, pred, held, rig, lead, dims, mode, want_extras):
        B, n, S, H, W, Hs, Ws = dims
        reduce, visibility, cell, tolerance = mode
        dev = pred.device
        ws, nbytes = _workspace('dpf_multiview_occ_workspace_bytes', 'multiview_loss: shape B=%d n=%d S=%d H=%d W=%d (reduce %d) is not supported',
                                B, n, S, H, W, reduce, device=dev)
        stats = torch.empty(MULTIVIEW_STATS, dtype=torch.float64, device=dev)
        out = torch.empty((), dtype=torch.float32, device=dev)
        luma = torch.empty(B * H * W + B * S * Hs * Ws, dtype=torch.float32, device=dev)
        zbuf = torch.empty((B, n, S, -(-Hs // cell), -(-Ws // cell)), dtype=torch.float32, device=dev) if visibility else None
        sel = torch.empty((B, n, H, W), dtype=torch.uint8, device=dev) if reduce else None
        extras = [None, None, None, None]
        if want_extras:
            extras = [torch.empty((B, n, S, H, W), dtype=torch.float32, device=dev), torch.empty((B, n, S, H, W), dtype=torch.uint8, device=dev),
                      torch.empty((B, n, S, 2, H, W), dtype=torch.float32, device=dev), torch.empty((B, n, S, H, W), dtype=torch.uint8, device=dev)]
        lib().call('dpf_multiview_occ_forward', *lead, *mode, _ptr(ws), nbytes, _ptr(luma), _ptr(zbuf), _ptr(sel), _ptr(stats), _ptr(out),
                   *[_ptr(t) for t in extras], _stream())
        ctx.save_for_backward(pred, stats, luma, rig, *[t for t in (zbuf, sel) + tuple(held) if t is not None])
        ctx.lead, ctx.mode = lead, mode
        if want_extras:
            planes = (luma[:B * H * W].view(B, H, W), luma[B * H * W:].view(B, S, Hs, Ws))
            more = tuple(t for t in (sel, zbuf) if t is not None)
            ctx.mark_non_differentiable(*extras, *planes, *more)
            return (out,) + tuple(extras[:3]) + planes + (extras[3],) + more
        return out

    @staticmethod
    def backward(ctx, gout, *unused):
        pred, stats, luma = ctx.saved_tensors[:3]
        rest = list(ctx.saved_tensors[4:])
        zbuf = rest.pop(0) if ctx.mode[1] else None
        sel = rest.pop(0) if ctx.mode[0] else None
        gout = _c(gout)
        _need(gout)
        dpred = torch.empty_like(pred)
        lib().call('dpf_multiview_occ_backward', *ctx.lead, *ctx.mode, _ptr(luma), _ptr(zbuf), _ptr(sel), _ptr(stats), _ptr(gout), _ptr(dpred),
                   _stream())
        return dpred, None, None, None, None, None, None


def multiview_rig(Kmat, Pmat, Ks, Ps):
    """csrc/multiview.hip: the twelve fp32 numbers per (sample, view) that carry a pixel of the target view and its depth into a
    neighbouring view, from K [B, 3, 3], P [B, 4, 4], Ks [B, S, 3, 3], Ps [B, S, 4, 4] (device float32) -> rig [B, S, 12] = (M row-major,
    t), M = Ks T[:3, :3] K^-1 and t = Ks T[:3, 3] with T = Ps P^-1, formed in fp64 on the device.  Nothing is read on the host."""
    _need(Kmat, Pmat, Ks, Ps, dtypes=_F32, contiguous=False)
    if Ks is None or Ks.dim() != 4:
        raise DpfError('multiview_rig: Ks %s is not [B, S, 3, 3]' % (None if Ks is None else tuple(Ks.shape),))
    B, S = Ks.shape[:2]
    if not 1 <= S <= MULTIVIEW_MAX_VIEWS:
        raise DpfError('multiview_rig: %d views, 1 to %d are supported' % (S, MULTIVIEW_MAX_VIEWS))
    for name, t, shape in (('K', Kmat, (B, 3, 3)), ('P', Pmat, (B, 4, 4)), ('Ks', Ks, (B, S, 3, 3)), ('Ps', Ps, (B, S, 4, 4))):
        if t is None or tuple(t.shape) != shape:
            raise DpfError('multiview_rig: %s %s, %s expected' % (name, None if t is None else tuple(t.shape), list(shape)))
    held = [_c(t.detach()) for t in (Kmat, Pmat, Ks, Ps)]
    rig = torch.empty((B, S, 12), dtype=torch.float32, device=Ks.device)
    lib().call('dpf_multiview_rig', *[_ptr(t) for t in held], B, S, _ptr(rig), _stream())
    return rig


def multiview_loss(pred, tgt_rgb, src_rgb, Kmat, Pmat, Ks, Ps, ab=None, mask=None, head_weights=(1.0,), target_type='disp', weight_ssim=0.8,
                   alpha=1.0, scale=0.1, min_depth=1e-3, return_warped=False, reduce='mean', visibility='none', cell=2, tolerance=0.01):
    """csrc/multiview.hip: the luminance of the source images src_rgb [B, S <= 8, 3, Hs, Ws] (a slice along dim 1 of a wider tensor is
    taken as it is) sampled bilinearly where the depth every head of pred [B, n <= 8, H, W] predicts sends the pixels of the target
    view, against the luminance of tgt_rgb [B, 3, H, W] -> the 0-dim loss sum_h w_h mean over the views that count a pixel of (mean over
    the counted pixels of weight_ssim clamp((1 - SSIM_3x3) / 2, 0, 1) + (1 - weight_ssim) rho(J - I; alpha, scale)), rho Barron's general
    robust loss.  The depth is a / (pred - b) for 'disp' (ab [B, 2] = [b, a], needed then only), 1 / pred for
    'idepth', pred for 'depth'; a pixel is usable where pred and the depth are finite, the depth >= min_depth and mask (None: everywhere)
    > 0; the geometry is multiview_rig's.  The gradient reaches pred only.  With return_warped also warped [B, n, S, H, W] fp32 (0 where
    not warpable), counted [B, n, S, H, W] uint8, sample_xy [B, n, S, 2, H, W] fp32 and the luminance planes [B, H, W], [B, S, Hs, Ws].

    Occlusion handling, off by default (then the call is MultiviewFn's, as it was).  visibility 'zbuffer': a warpable pixel is seen by a
    view where its depth in that view is at most (1 + tolerance) x the smallest depth any usable pixel of the head splats into its cell
    of cell x cell source pixels (cell 1, 2 or 4), and 'seen' stands for 'warpable' in the rule above; only usable pixels splat, so a
    masked-out occluder hides nothing.  reduce 'min': per head and pixel the smallest term over the views that count it (the lowest view
    wins a tie), averaged over the pixels some view counts.  cell 2 and tolerance 0.01 are conventional starting values, not tuned on
    face data.  With return_warped and one of them on the tuple goes on with visible [B, n, S, H, W] uint8 (seen), selected [B, n, H, W]
    uint8 (reduce 'min': the winning view, 255 none) and zbuffer [B, n, S, ceil(Hs / cell), ceil(Ws / cell)] fp32 (visibility
    'zbuffer'; +inf where nothing landed)."""
    code = _target_code('multiview_loss', target_type, ())
    if reduce not in MULTIVIEW_REDUCE:
        raise DpfError("multiview_loss: reduce must be 'mean' or 'min', got %r" % (reduce,))
    if visibility not in MULTIVIEW_VISIBILITY:
        raise DpfError("multiview_loss: visibility must be 'none' or 'zbuffer', got %r" % (visibility,))
    cell = _int_arg('multiview_loss', 'cell', cell, MULTIVIEW_CELLS)
    if isinstance(tolerance, bool) or not isinstance(tolerance, (int, float)) or not 0.0 <= float(tolerance) < float('inf'):
        raise DpfError('multiview_loss: tolerance must be a finite number >= 0, got %r' % (tolerance,))
    if target_type == 'disp' and ab is None:
        raise DpfError("multiview_loss: target_type 'disp' needs ab [B, 2] = [b, a]")
    ab = ab if target_type == 'disp' else None
    _need(pred, tgt_rgb, src_rgb, ab, mask, dtypes=_F32, contiguous=False)
    if pred.dim() != 4:
        raise DpfError('multiview_loss: pred %s is not [B, n, H, W]' % (tuple(pred.shape),))
    if tgt_rgb is None or src_rgb is None or src_rgb.dim() != 5 or src_rgb.shape[2] != 3:
        raise DpfError('multiview_loss: tgt_rgb [B, 3, H, W] and src_rgb [B, S, 3, Hs, Ws] are needed')
    B, n, H, W = pred.shape
    S, Hs, Ws = src_rgb.shape[1], src_rgb.shape[3], src_rgb.shape[4]
    _match_pred('multiview_loss', pred, ('tgt_rgb', tgt_rgb, (B, 3, H, W)), ('src_rgb', src_rgb, (B, S, 3, Hs, Ws)), ('ab', ab, (B, 2)),
                ('mask', mask, (B, H, W)))
    if len(head_weights) != n:
        raise DpfError('multiview_loss: %d head weights for %d heads' % (len(head_weights), n))
    if not 0.0 <= float(weight_ssim) <= 1.0:
        raise DpfError('multiview_loss: weight_ssim must lie in [0, 1], got %r' % (weight_ssim,))
    if float(alpha) != float(alpha) or float(alpha) in (float('inf'), -float('inf')):
        raise DpfError('multiview_loss: alpha must be finite (the limits at +-infinity are not built), got %r' % (alpha,))
    for name, v in (('scale', scale), ('min_depth', min_depth)):
        if not 0.0 < float(v) < float('inf'):
            raise DpfError('multiview_loss: %s must be positive, got %r' % (name, v))
    rig = multiview_rig(Kmat, Pmat, Ks, Ps)
    if tuple(rig.shape[:2]) != (B, S):
        raise DpfError('multiview_loss: Ks %s does not match src_rgb %s' % (tuple(Ks.shape), tuple(src_rgb.shape)))
    pred = _c(pred)
    src, stride = _batch_view(src_rgb.detach(), S * 3 * Hs * Ws)
    held = (_c(tgt_rgb.detach()), src, None if ab is None else _c(ab.detach()), None if mask is None else _c(mask.detach()))
    lead = (_ptr(pred), _ptr(held[0]), _ptr(src), stride, _ptr(rig), _ptr(held[2]), _ptr(held[3]), B, n, S, H, W, Hs, Ws, code,
            float(weight_ssim), float(alpha), float(scale), float(min_depth), _normalizer_floats(), _host_floats(head_weights))
    mode = (MULTIVIEW_REDUCE[reduce], MULTIVIEW_VISIBILITY[visibility], cell, float(tolerance))
    if mode[0] or mode[1]:
        return MultiviewOccFn.apply(pred, held, rig, lead, (B, n, S, H, W, Hs, Ws), mode, bool(return_warped))
    return MultiviewFn.apply(pred, held, rig, lead, (B, n, S, H, W, Hs, Ws), bool(return_warped))


UNIMODAL_STATS = 16         # doubles: count per head [0, 8), term sum per head [8, 16)
UNIMODAL_MAX_HEADS, UNIMODAL_MAX_D, UNIMODAL_MAX_L = 8, 8, 32


def _host_ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


class UnimodalFn(torch.autograd.Function):
    """HeadLossFn for a loss that reads the heads' logits, a list of separate tensors, instead of pred [B, n, H, W] (csrc/unimodal.hip):
    -> 0-dim loss, and with want_extras counted and expect.  The C argument orders agree as in that family: forward `lead | ws, nbytes |
    logsum | stats, out | extras`, backward `lead | logsum | stats, gout, dlogits`.  Workspace, stats and the log-sum planes are fresh tensors (planes
    and stats are saved for the backward, the workspace is not needed again), gout is read on the device and nothing is read on the host,
    so the call is capturable inside the train-step graph.  One gradient per logit tensor, every element written; nothing else gets one."""

    @staticmethod
    def forward(ctx, held, tail, want_extras, *logits):
        B, _, D, h, w = logits[0].shape
        n, (L, H, W) = len(logits), tail[:3]
        dev = logits[0].device
        ws, nbytes = _workspace('dpf_unimodal_workspace_bytes', 'unimodal_loss: shape B=%d n=%d H=%d W=%d is not supported', B, n, H, W,
                                device=dev)
        stats = torch.empty(UNIMODAL_STATS, dtype=torch.float64, device=dev)
        out = torch.empty((), dtype=torch.float32, device=dev)
        logsum = torch.empty((B, n, H, W), dtype=torch.float32, device=dev)
        extras = [None, None]
        if want_extras:
            extras = [torch.empty((B, n, H, W), dtype=torch.uint8, device=dev), torch.empty((B, n, H, W), dtype=torch.float32, device=dev)]
        lead = (*[_ptr(t) for t in held], B, n, D, h, w, *tail)
        lib().call('dpf_unimodal_forward', _host_ptrs(logits), *lead, _ptr(ws), nbytes, _ptr(logsum), _ptr(stats), _ptr(out),
                   *[_ptr(t) for t in extras], _stream())
        ctx.save_for_backward(logsum, stats, *[t for t in held if t is not None], *logits)
        ctx.lead, ctx.n = lead, n
        if want_extras:
            ctx.mark_non_differentiable(*extras)
            return (out,) + tuple(extras)
        return out

    @staticmethod
    def backward(ctx, gout, *unused):
        saved = ctx.saved_tensors
        logsum, stats, logits = saved[0], saved[1], saved[len(saved) - ctx.n:]
        gout = _c(gout)
        _need(gout)
        grads = [torch.empty_like(t) for t in logits]
        lib().call('dpf_unimodal_backward', _host_ptrs(logits), *ctx.lead, _ptr(logsum), _ptr(stats), _ptr(gout), _host_ptrs(grads), _stream())
        return (None, None, None) + tuple(grads)


def unimodal_loss(logits, disp_values, target, mask=None, target_ab=None, head_weights=(1.0,), scale=4, align_corners=True,
                  laplace_scale=None, return_extras=False):
    """csrc/unimodal.hip (not in the reference): the cross-entropy between the hypothesis distribution of every
    disparity head and a Laplace distribution centred on the label -> the 0-dim loss sum_h w_h mean over the counted pixels of
    -sum_l P_l log p_l.  logits: a list of n <= 8 tensors [B, 1, D <= 8, h, w], the heads' cost logits; p is the softmax over the
    L = scale * D <= 32 hypotheses of their trilinear upsample, exactly the soft-argmin's (ops.softargmin with the same disp_values, scale
    and align_corners), recomputed inside the kernels; P_l ~ exp(-|d_l - t| / laplace_scale) over the strictly ascending disp_values
    (None: d_1 - d_0).  t is target [B, H, W], or with target_ab [B, 2] = [b, a] a / target + b of the depth map `target`.  A pixel is
    counted when mask (None: everywhere) > 0, t is finite and d_0 <= t <= d_{L-1}.  One gradient per logit tensor, every element written,
    the same bits on every call; nothing flows to target, mask, target_ab or disp_values.  With return_extras also counted
    [B, n, H, W] uint8 and expect [B, n, H, W] fp32, the soft-argmin's value sum_l p_l d_l."""
    name = 'unimodal_loss'
    if not isinstance(logits, (list, tuple)) or not 1 <= len(logits) <= UNIMODAL_MAX_HEADS:
        raise DpfError('%s: logits must be a list of 1..%d tensors [B, 1, D, h, w], got %r' %
                       (name, UNIMODAL_MAX_HEADS, len(logits) if isinstance(logits, (list, tuple)) else type(logits).__name__))
    _need(*logits, target, mask, target_ab, dtypes=_F32, contiguous=False)
    first = logits[0]
    if first.dim() != 5 or first.shape[1] != 1:
        raise DpfError('%s: logits[0] %s is not [B, 1, D, h, w]' % (name, tuple(first.shape)))
    for i, t in enumerate(logits):
        if tuple(t.shape) != tuple(first.shape):
            raise DpfError('%s: logits[%d] %s does not match logits[0] %s' % (name, i, tuple(t.shape), tuple(first.shape)))
    B, _, D, h, w = first.shape
    scale = _int_arg(name, 'scale', scale)
    disp = [float(v) for v in disp_values]
    L, H, W = scale * D, scale * h, scale * w
    if scale < 1 or D > UNIMODAL_MAX_D or L > UNIMODAL_MAX_L:
        raise DpfError('%s: D=%d levels at scale %r are not supported (D <= %d, scale * D <= %d)' % (name, D, scale, UNIMODAL_MAX_D,
                                                                                                       UNIMODAL_MAX_L))
    if len(disp) != L:
        raise DpfError('%s: %d disp_values for %d hypotheses (scale %d x D %d)' % (name, len(disp), L, scale, D))
    if any(v != v or v in (float('inf'), -float('inf')) for v in disp) or any(b <= a for a, b in zip(disp, disp[1:])):
        raise DpfError('%s: disp_values must be finite and strictly ascending' % name)
    if target is None:
        raise DpfError('%s: target [B, H, W] is needed' % name)
    _match_pred(name, first, ('target', target, (B, H, W)), ('mask', mask, (B, H, W)), ('target_ab', target_ab, (B, 2)))
    if len(head_weights) != len(logits):
        raise DpfError('%s: %d head weights for %d heads' % (name, len(head_weights), len(logits)))
    if laplace_scale is None:
        if L < 2:
            raise DpfError('%s: one hypothesis has no spacing, laplace_scale is needed' % name)
        laplace_scale = disp[1] - disp[0]
    if not 0.0 < float(laplace_scale) < float('inf'):
        raise DpfError('%s: laplace_scale must be a positive finite number, got %r' % (name, laplace_scale))
    held = tuple(None if t is None else _c(t.detach()) for t in (target, mask, target_ab))
    tail = (L, H, W, int(bool(align_corners)), _host_floats(disp), float(laplace_scale), _host_floats(head_weights))
    return UnimodalFn.apply(held, tail, bool(return_extras), *[_c(t) for t in logits])


CONFIDENCE_PLANES = ('peak', 'entropy', 'mass', 'spread', 'modal', 'lstar')      # the output order of dpf_head_confidence
CONFIDENCE_MAX_WINDOW, CONFIDENCE_MAX_BINS = 32, 64


def head_confidence(logit_list, disp_values, scale=4, align_corners=True, window=1, want=CONFIDENCE_PLANES):
    """csrc/head_confidence.hip (not in the reference): confidence measures and a modal estimate from the hypothesis
    distribution p of every disparity head, the softmax the soft-argmin takes its expectation of, recomputed inside the kernel from the
    n <= 8 logit tensors [B, 1, D <= 8, h, w] (operands as in unimodal_loss) -> a dict of the planes named in `want`, each [B, n, H, W]:
    'peak' max_l p_l, 'entropy' 1 - H(p) / log(L) in [0, 1], 'mass' the probability within `window` hypotheses of the peak, 'spread' the
    standard deviation of p in disparity units, 'modal' the expectation over that window alone (fp32), and 'lstar' the peak's index
    (int32).  A pixel whose distribution is not finite gets peak = entropy = mass = 0 and spread = modal = NaN.  One launch, no host
    read; what a plane holds does not depend on which others are asked for.  No gradient."""
    name = 'head_confidence'
    if not isinstance(logit_list, (list, tuple)) or not 1 <= len(logit_list) <= UNIMODAL_MAX_HEADS:
        raise DpfError('%s: logits must be a list of 1..%d tensors [B, 1, D, h, w], got %r' %
                       (name, UNIMODAL_MAX_HEADS, len(logit_list) if isinstance(logit_list, (list, tuple)) else type(logit_list).__name__))
    _need(*logit_list, dtypes=_F32, contiguous=False)
    first = logit_list[0]
    if first.dim() != 5 or first.shape[1] != 1:
        raise DpfError('%s: logits[0] %s is not [B, 1, D, h, w]' % (name, tuple(first.shape)))
    for i, t in enumerate(logit_list):
        if tuple(t.shape) != tuple(first.shape):
            raise DpfError('%s: logits[%d] %s does not match logits[0] %s' % (name, i, tuple(t.shape), tuple(first.shape)))
    B, _, D, h, w = first.shape
    scale = _int_arg(name, 'scale', scale)
    window = _int_arg(name, 'window', window)
    if not 0 <= window <= CONFIDENCE_MAX_WINDOW:
        raise DpfError('%s: window must be an integer from 0 to %d, got %r' % (name, CONFIDENCE_MAX_WINDOW, window))
    disp = [float(v) for v in disp_values]
    L, H, W = scale * D, scale * h, scale * w
    if scale < 1 or D > UNIMODAL_MAX_D or L > UNIMODAL_MAX_L or L < 2:
        raise DpfError('%s: D=%d levels at scale %r are not supported (D <= %d, 2 <= scale * D <= %d)' % (name, D, scale, UNIMODAL_MAX_D,
                                                                                                            UNIMODAL_MAX_L))
    if len(disp) != L:
        raise DpfError('%s: %d disp_values for %d hypotheses (scale %d x D %d)' % (name, len(disp), L, scale, D))
    if any(v != v or v in (float('inf'), -float('inf')) for v in disp) or any(b <= a for a, b in zip(disp, disp[1:])):
        raise DpfError('%s: disp_values must be finite and strictly ascending' % name)
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(k not in CONFIDENCE_PLANES for k in want):
        raise DpfError('%s: want must name at least one of %s, got %r' % (name, ', '.join(CONFIDENCE_PLANES), want))
    logits = [_c(t.detach()) for t in logit_list]
    out = {k: torch.empty((B, len(logits), H, W), dtype=torch.int32 if k == 'lstar' else torch.float32, device=first.device)
           for k in CONFIDENCE_PLANES if k in want}
    lib().call('dpf_head_confidence', _host_ptrs(logits), B, len(logits), D, h, w, L, H, W, int(bool(align_corners)), _host_floats(disp),
               window, *[_ptr(out.get(k)) for k in CONFIDENCE_PLANES], _stream())
    return out


def confidence_curve(conf, pred, target, mask=None, target_ab=None, bins=16, into=None):
    """csrc/head_confidence.hip: the sparsification table of a confidence map -> curve [bins, 2] float64 = (count, sum |pred - t|) per
    confidence bin, bin = min(bins - 1, int(conf * bins)).  conf and pred [B, H, W] (a head of a [B, n, H, W] tensor is read in place),
    target [B, H, W], t = target or with target_ab [B, 2] = [b, a] a / target + b; a pixel is counted when mask (None: everywhere) > 0
    and t, pred, conf are finite.  `into`: a [bins, 2] float64 table the result is ADDED to (and which is returned); without it a fresh
    table.  The same bits on every call; nothing is read on the host.  No gradient."""
    name = 'confidence_curve'
    _need(conf, pred, target, mask, target_ab, dtypes=_F32, contiguous=False)
    _need(into, dtypes=(torch.float64,))
    if conf is None or pred is None or target is None:
        raise DpfError('%s: conf, pred and target [B, H, W] are needed' % name)
    if conf.dim() != 3:
        raise DpfError('%s: conf %s is not [B, H, W]' % (name, tuple(conf.shape)))
    B, H, W = conf.shape
    bins = _int_arg(name, 'bins', bins)
    if not 1 <= bins <= CONFIDENCE_MAX_BINS:
        raise DpfError('%s: bins must be an integer from 1 to %d, got %r' % (name, CONFIDENCE_MAX_BINS, bins))
    _match_pred(name, conf, ('pred', pred, (B, H, W)), ('target', target, (B, H, W)), ('mask', mask, (B, H, W)), ('target_ab', target_ab, (B, 2)),
                ('into', into, (bins, 2)))
    conf, cbs = _batch_view(conf.detach(), H * W)
    pred, pbs = _batch_view(pred.detach(), H * W)
    target, mask, target_ab = [None if t is None else _c(t.detach()) for t in (target, mask, target_ab)]
    ws, nbytes = _workspace('dpf_confidence_curve_workspace_bytes', 'confidence_curve: shape B=%d H=%d W=%d bins=%d is not supported',
                            B, H, W, bins, device=conf.device)
    curve = into if into is not None else torch.empty((bins, 2), dtype=torch.float64, device=conf.device)
    lib().call('dpf_confidence_curve', _ptr(conf), cbs, _ptr(pred), pbs, _ptr(target), _ptr(mask), _ptr(target_ab), B, H, W, bins,
               int(into is not None), _ptr(ws), nbytes, _ptr(curve), _stream())
    return curve


def adam_step(param, grad, exp_avg, exp_avg_sq, step, lr, beta1=0.9, beta2=0.999, eps=1e-5, gscale=1.0):
    _need(param, grad, exp_avg, exp_avg_sq)
    lib().call('dpf_adam_step', _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(), int(step), float(lr), float(beta1),
               float(beta2), float(eps), float(gscale), _stream())


def adam_hyper(step, lr, beta1=0.9, beta2=0.999):
    """The two step-dependent scalars of dpf_adam_step as float32, computed as the C side computes them."""
    import numpy as np
    bc1 = 1.0 - beta1 ** int(step)
    bc2 = 1.0 - beta2 ** int(step)
    return np.float32(float(lr) / bc1), np.float32(1.0 / (bc2 ** 0.5))


def adam_step_hyper(param, grad, exp_avg, exp_avg_sq, hyper, beta1=0.9, beta2=0.999, eps=1e-5, gscale=1.0):
    """adam_step with the step-dependent scalars in device memory (hyper: 2 floats) -- the launch a captured train-step graph replays."""
    _need(param, grad, exp_avg, exp_avg_sq, hyper)
    lib().call('dpf_adam_step_hyper', _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(), _ptr(hyper), float(beta1),
               float(beta2), float(eps), float(gscale), _stream())


def sgd_step(param, grad, momentum_buf, lr, momentum=0.9, weight_decay=2e-4, gscale=1.0, live=None):
    """torch.optim.SGD(momentum, weight_decay) over the flat arenas.  live: uint8 per element, 0 = belongs to a parameter without a gradient
    this step and stays untouched, buffer included (None: every element is live)."""
    _need(param, grad, momentum_buf)
    lib().call('dpf_sgd_step', _ptr(param), _ptr(grad), _ptr(momentum_buf), _ptr(_live_mask(live, param)), param.numel(), float(lr),
               float(momentum), float(weight_decay), float(gscale), _stream())


def sgd_step_lr(param, grad, momentum_buf, lr_dev, momentum=0.9, weight_decay=2e-4, gscale=1.0, live=None):
    """sgd_step with the rate in device memory (lr_dev: one float) -- the launch a captured train-step graph replays."""
    _need(param, grad, momentum_buf, lr_dev)
    lib().call('dpf_sgd_step_lr', _ptr(param), _ptr(grad), _ptr(momentum_buf), _ptr(_live_mask(live, param)), param.numel(), _ptr(lr_dev),
               float(momentum), float(weight_decay), float(gscale), _stream())


def _live_mask(live, param):
    if live is not None and not (live.is_cuda and live.dtype == torch.uint8 and live.is_contiguous() and live.numel() == param.numel()):
        raise DpfError('live mask: one contiguous uint8 per arena element on the GPU expected')
    return live


def rmsprop_step(param, grad, square_avg, lr, alpha=0.99, eps=1e-5, gscale=1.0):
    """torch.optim.RMSprop(alpha, eps; no momentum, not centred) over the flat arenas."""
    _need(param, grad, square_avg)
    lib().call('dpf_rmsprop_step', _ptr(param), _ptr(grad), _ptr(square_avg), param.numel(), float(lr), float(alpha), float(eps),
               float(gscale), _stream())


def rmsprop_step_lr(param, grad, square_avg, lr_dev, alpha=0.99, eps=1e-5, gscale=1.0):
    """rmsprop_step with the rate in device memory (lr_dev: one float)."""
    _need(param, grad, square_avg, lr_dev)
    lib().call('dpf_rmsprop_step_lr', _ptr(param), _ptr(grad), _ptr(square_avg), param.numel(), _ptr(lr_dev), float(alpha), float(eps),
               float(gscale), _stream())


# ---- gradient accumulation and global-norm clipping (csrc/grad_ctl.hip).  ctl: the control record, GRAD_CTL_FLOATS device floats --
# [0:2] the optimiser's per-step scalars, [2] first, [3] apply (the host's), [4] gmul, [5] grad_norm (grad_finish's)
GRAD_CTL_FLOATS = 8
GRAD_CTL_FIRST, GRAD_CTL_APPLY, GRAD_CTL_GMUL, GRAD_CTL_NORM = 2, 3, 4, 5


def _grad_ws(n, device):
    return _workspace('dpf_grad_ctl_workspace_bytes', 'grad_ctl: an arena of %d elements is not supported', n, device=device, tag='grad_ctl')


def _need_ctl(ctl):
    _need(ctl)
    if ctl.dtype != torch.float32 or ctl.numel() < GRAD_CTL_FLOATS:
        raise DpfError('grad_ctl: the control record is %d float32 on the GPU' % GRAD_CTL_FLOATS)


def grad_fold(acc, grad, ctl, partials=False):
    """acc = grad when ctl[first] is set, else acc + grad, in fp32; with `partials` and ctl[apply] set the same pass leaves the sums of
    squares of the new acc for grad_finish."""
    _need(acc, grad)
    _need_ctl(ctl)
    if acc.numel() != grad.numel() or acc.dtype != torch.float32 or grad.dtype != torch.float32:
        raise DpfError('grad_fold: two float32 arenas of one length expected')
    ws, nbytes = _grad_ws(acc.numel(), acc.device) if partials else (None, 0)
    lib().call('dpf_grad_fold', _ptr(acc), _ptr(grad), acc.numel(), _ptr(ctl), _ptr(ws), nbytes, _stream())


def grad_sumsq(grad):
    """The per-workgroup fp64 sums of squares of an arena, left for grad_finish."""
    _need(grad)
    ws, nbytes = _grad_ws(grad.numel(), grad.device)
    lib().call('dpf_grad_sumsq', _ptr(grad), grad.numel(), _ptr(ws), nbytes, _stream())


def grad_finish(n, ctl, gscale=1.0, clip=0.0):
    """After grad_fold(partials=True) or grad_sumsq over n elements on this stream: ctl[grad_norm] = gscale * sqrt(sum),
    ctl[gmul] = gscale * min(1, clip / (norm + 1e-6)) (clip 0: gscale); nothing when ctl[apply] is 0."""
    _need_ctl(ctl)
    ws, nbytes = _grad_ws(n, ctl.device)
    lib().call('dpf_grad_finish', _ptr(ws), nbytes, n, float(gscale), float(clip), _ptr(ctl), _stream())


def adam_step_ctl(param, grad, exp_avg, exp_avg_sq, ctl, beta1=0.9, beta2=0.999, eps=1e-5):
    """adam_step_hyper behind the control record: scalars from ctl[0:2], the gradient times ctl[gmul], a no-op when ctl[apply] is 0."""
    _need(param, grad, exp_avg, exp_avg_sq)
    _need_ctl(ctl)
    lib().call('dpf_adam_step_ctl', _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(), _ptr(ctl), float(beta1),
               float(beta2), float(eps), _stream())


def sgd_step_ctl(param, grad, momentum_buf, ctl, momentum=0.9, weight_decay=2e-4, live=None):
    """sgd_step_lr behind the control record (the rate in ctl[0])."""
    _need(param, grad, momentum_buf)
    _need_ctl(ctl)
    lib().call('dpf_sgd_step_ctl', _ptr(param), _ptr(grad), _ptr(momentum_buf), _ptr(_live_mask(live, param)), param.numel(), _ptr(ctl),
               float(momentum), float(weight_decay), _stream())


def rmsprop_step_ctl(param, grad, square_avg, ctl, alpha=0.99, eps=1e-5):
    """rmsprop_step_lr behind the control record (the rate in ctl[0])."""
    _need(param, grad, square_avg)
    _need_ctl(ctl)
    lib().call('dpf_rmsprop_step_ctl', _ptr(param), _ptr(grad), _ptr(square_avg), param.numel(), _ptr(ctl), float(alpha), float(eps),
               _stream())


# ---- validation metrics (csrc/metrics.hip): raw wrappers; results stay on the device, nothing here reads the host
def _metric_ws(query, B, n, device):
    return _workspace(query, query + ': shape B=%d n=%d is not supported', B, n, device=device, tag='metric')


def metric_absolute_dp(pred, abvalue, target, mask=None, target_type='disp', threshold=1.01, out=None):
    """pred / target / mask [B, H, W] -> device row [abs_rel, abs_diff, sq_rel, rmse, rmse_log, a1, a2, a3] (metrics.depth_errors, after
    metrics.disp2depth unless target_type == 'depth'); abvalue [B, 2] = [b, a]."""
    _need(pred, abvalue, target, mask)
    B, n = pred.shape[0], pred[0].numel()
    out = torch.empty(8, dtype=torch.float32, device=pred.device) if out is None else out
    ws, nbytes = _metric_ws('dpf_metric_absolute_dp_workspace_bytes', B, n, pred.device)
    lib().call('dpf_metric_absolute_dp', _ptr(pred), _ptr(abvalue), _ptr(target), _ptr(mask), B, n, TARGET_TYPES[target_type],
               float(threshold), _ptr(out), _ptr(ws), nbytes, _stream())
    return out


def metric_normal_dp(pred, target, mask=None, out=None):
    """pred / target [B, 3, H, W], mask [B, H, W] -> device row [mean, rms] angular error in degrees."""
    _need(pred, target, mask)
    B, n = pred.shape[0], pred[0, 0].numel()
    out = torch.empty(2, dtype=torch.float32, device=pred.device) if out is None else out
    ws, nbytes = _metric_ws('dpf_metric_normal_dp_workspace_bytes', B, n, pred.device)
    lib().call('dpf_metric_normal_dp', _ptr(pred), _ptr(target), _ptr(mask), B, n, _ptr(out), _ptr(ws), nbytes, _stream())
    return out


def metric_ranks(values, negate=False, out=None):
    """values [B, n] -> int32 [B, n]: argsort(argsort(z, stable), stable) per row, of -z with ``negate``."""
    _need(values)
    B, n = values.shape[0], values[0].numel()
    out = torch.empty((B, n), dtype=torch.int32, device=values.device) if out is None else out
    ws, nbytes = _metric_ws('dpf_metric_ranks_workspace_bytes', B, n, values.device)
    lib().call('dpf_metric_ranks', _ptr(values), _ptr(out), B, n, int(bool(negate)), _ptr(ws), nbytes, _stream())
    return out


def metric_affine_dp(pred, target, weight, rank_pred, rank_negpred, rank_target, irls_iters=5, epsilon=1e-3, out=None):
    """pred / target / weight [B, n] and the three rank arrays -> device row [wmae, wrmse, 1 - spearman], batch means."""
    _need(pred, target, weight, rank_pred, rank_negpred, rank_target)
    B, n = pred.shape[0], pred[0].numel()
    out = torch.empty(3, dtype=torch.float32, device=pred.device) if out is None else out
    ws, nbytes = _metric_ws('dpf_metric_affine_dp_workspace_bytes', B, n, pred.device)
    lib().call('dpf_metric_affine_dp', _ptr(pred), _ptr(target), _ptr(weight), _ptr(rank_pred), _ptr(rank_negpred), _ptr(rank_target), B, n,
               int(irls_iters), float(epsilon), _ptr(out), _ptr(ws), nbytes, _stream())
    return out


def reset_zero_arenas():
    """Forget what is left of the pre-zeroed arenas: the next zero_slot() clears its arena again.  A graph capture of the train step starts
    with this, so that the clearing fill is PART of the captured work (a replay finds the slots zero, as the eager step does)."""
    for st in _zero_arena.values():
        st[1] = st[0].numel()
