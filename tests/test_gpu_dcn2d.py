"""GPU parity tests of the 2-D deformable convolution, plain (DCN v1) and modulated (v2) (csrc/dcn2d.hip over the rank-2 kernels of
csrc/dcn_gather.hip), called through the C ABI wrappers (ops.deform_conv2d_forward_raw / ops.deform_conv2d_backward_raw), against the fp64
restatement tests/dcn2d_cpu.py and its autograd (tests/test_dcn2d_host.py pins that to the 3-D oracle at depth 1, to F.conv2d and to shifted taps).

Tolerances: those of the project's fp32-matrix-instruction deformable tier at these operand scales (x 1, weight 0.1, bias 1;
tests/test_gpu_dcn_grouped.py): forward 1e-4, every gradient 2e-4 of the reference tensor's maximum.  Known answers: 1e-5.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import dcn2d_cpu as ref2d
from tests import support
from tests.support import DEV, close, rnd

pytestmark = pytest.mark.gpu

GRADS = ('grad_input', 'grad_offset', 'grad_mask', 'grad_weight', 'grad_bias')


# (B, C, K, H, W), (kh, kw), stride, pad, dil, (group, dg)
CASES = [
    ((2, 16, 8, 9, 13), (3, 3), (1, 1), (1, 1), (1, 1), (1, 1)),      # two tiles with a tail, batch 2
    ((2, 16, 8, 9, 13), (3, 3), (1, 1), (1, 1), (1, 1), (2, 4)),      # same with groups
    ((1, 12, 6, 7, 11), (3, 3), (1, 1), (1, 1), (1, 1), (3, 2)),      # conv group straddles two offset groups
    ((1, 12, 6, 7, 11), (3, 3), (1, 1), (1, 1), (1, 1), (2, 3)),      # offset group straddles two conv groups
    ((2, 10, 4, 10, 21), (3, 3), (1, 1), (1, 1), (1, 1), (2, 5)),     # odd C / group, 210 positions
    ((1, 8, 16, 6, 12), (3, 3), (1, 1), (1, 1), (1, 1), (8, 8)),      # depthwise
    ((2, 16, 8, 17, 25), (3, 3), (2, 2), (1, 1), (1, 1), (2, 2)),     # strided
    ((1, 16, 8, 11, 14), (3, 3), (1, 1), (2, 2), (2, 2), (1, 4)),     # dilated
    ((1, 8, 8, 8, 12), (1, 3), (1, 1), (0, 1), (1, 1), (1, 2)),       # non-square window
    ((1, 8, 8, 9, 10), (1, 1), (1, 1), (0, 0), (1, 1), (2, 1)),       # 1 x 1 window
    ((1, 8, 8, 12, 15), (5, 5), (1, 1), (2, 2), (1, 1), (1, 1)),      # 5 x 5 window
    ((1, 6, 4, 13, 16), (7, 7), (1, 1), (3, 3), (1, 1), (1, 2)),      # T = 49
    ((1, 8, 8, 10, 12), (3, 3), (1, 1), (0, 0), (1, 1), (1, 1)),      # no padding
    ((1, 96, 96, 6, 12), (3, 3), (1, 1), (1, 1), (1, 1), (2, 3)),     # more than one 32-row matrix tile per group
    ((1, 256, 256, 4, 8), (3, 3), (1, 1), (1, 1), (1, 1), (4, 8)),    # channel limit, less than one tile
    ((3, 5, 3, 8, 9), (3, 3), (1, 1), (1, 1), (1, 1), (1, 1)),        # odd C, K < 4
    ((1, 64, 64, 4, 8), (3, 3), (1, 1), (1, 1), (1, 1), (2, 2)),      # K = 64: four forward tiles, one accumulator on every wave
]
THREE_TILES = ((2, 16, 8, 10, 16), (3, 3), (1, 1), (1, 1), (1, 1), (2, 4))     # 160 positions: two full tiles and a tail of 32
INT_CASE = ((2, 8, 8, 9, 13), (3, 3), (1, 1), (1, 1), (1, 1), (2, 2))


def _id(case):
    shape, k, s, p, d, g = case
    return 'x'.join(map(str, shape)) + '-k%dx%d-s%d-p%d-d%d-g%d-dg%d' % (k + (s[1], p[1], d[1]) + g)


@functools.lru_cache(maxsize=None)
def _problem(case, modulated, integer_offsets=False):
    """-> inputs (fp32, CPU; mask and grad_mask None for the plain operator), grad_output, the helper's fp64 forward and its fp64 autograd
    gradients in GRADS order; computed once per (case, variant) and shared, never modified."""
    (B, C, K, H, W), (kh, kw), s, p, d, (group, dg) = case
    T = kh * kw
    Ho, Wo = ref2d.out_size(H, W, kh, kw, s, p, d)
    x = rnd(B, C, H, W, seed=340)
    w, b = rnd(K, C // group, kh, kw, seed=342, scale=0.1), rnd(K, seed=343)
    if integer_offsets:
        off = torch.randint(-2, 3, (B, dg * 2 * T, Ho, Wo), generator=torch.Generator().manual_seed(341)).float()
    else:
        off = rnd(B, dg * 2 * T, Ho, Wo, seed=341, scale=1.5)
    mask = None
    if modulated:
        mask = torch.sigmoid(rnd(B, dg * T, Ho, Wo, seed=345))
        mask[torch.rand(mask.shape, generator=torch.Generator().manual_seed(346)) < 0.1] = 0.0
    go = rnd(B, K, Ho, Wo, seed=344)
    leaves = [None if t is None else t.double().requires_grad_() for t in (x, off, mask, w, b)]
    y_ref = ref2d.deform_conv2d_ref(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], s, p, d, group, dg)
    g = torch.autograd.grad(y_ref, [l for l in leaves if l is not None], go.double())
    g = list(g)
    if not modulated:
        g.insert(2, None)
    return (x, off, mask, w, b, go), y_ref.detach(), tuple(g)


def _gpu(ts):
    return [None if t is None else t.to(DEV) for t in ts]


def _compare_grads(got, g_ref, tol, tag, names=GRADS):
    for a, r, nm in zip(got, g_ref, GRADS):
        if nm not in names:
            continue
        if r is None:
            assert a is None, nm
        else:
            close(a, r, tol, '%s %s' % (tag, nm))


@pytest.mark.parametrize('modulated', [False, True], ids=['plain', 'modulated'])
@pytest.mark.parametrize('case', CASES, ids=_id)
def test_parity_forward_and_gradients(case, modulated):
    """Forward and every gradient against the fp64 helper; the inputs put 5-40 % of the samples wholly outside the image and at least 5 % on
    its border (some corners outside), asserted here on the CPU."""
    ops = support.ops()
    (B, C, K, H, W), (kh, kw), s, p, d, (group, dg) = case
    (x, off, mask, w, b, go), y_ref, g_ref = _problem(case, modulated)
    out_all, out_some = ref2d.outside_fractions(off, H, W, kh, kw, s, p, d, dg)
    print('samples wholly outside %.3f, partly outside %.3f' % (out_all, out_some))
    assert 0.05 <= out_all <= 0.40 and out_some >= 0.05
    xg, og, mg, wg, bg, gg = _gpu((x, off, mask, w, b, go))
    y = ops.deform_conv2d_forward_raw(xg, wg, bg, og, mg, s, p, d, group, dg)
    close(y, y_ref, 1e-4, 'dcn2d fwd')
    _compare_grads(ops.deform_conv2d_backward_raw(xg, wg, bg, og, mg, gg, s, p, d, group, dg), g_ref, 2e-4, 'dcn2d')


@pytest.mark.parametrize('group,dg', [(1, 1), (2, 4), (4, 16)])
def test_zero_offsets_and_unit_mask_equal_the_plain_convolution(group, dg):
    """Zero offsets, mask 1: F.conv2d(groups) whatever deformable_group is (plain fp32 summation: 1e-5 of the maximum); strided and dilated."""
    B, C, K, H, W = 2, 16, 8, 11, 13
    x, w, b = rnd(B, C, H, W, seed=350), rnd(K, C // group, 3, 3, seed=351, scale=0.1), rnd(K, seed=352)
    for s, d in ((1, 1), (2, 1), (1, 2)):
        ref = F.conv2d(x.double(), w.double(), b.double(), stride=s, padding=d, dilation=d, groups=group)
        Ho, Wo = ref.shape[2:]
        off, mask = torch.zeros(B, dg * 18, Ho, Wo), torch.ones(B, dg * 9, Ho, Wo)
        xg, og, mg, wg, bg = _gpu((x, off, mask, w, b))
        for m in (None, mg):
            y = support.ops().deform_conv2d_forward_raw(xg, wg, bg, og, m, (s, s), (d, d), (d, d), group, dg)
            close(y, ref, 1e-5, 'zero offsets s%d d%d %s' % (s, d, 'plain' if m is None else 'mask 1'))


@pytest.mark.parametrize('modulated', [False, True], ids=['plain', 'modulated'])
def test_integer_offsets_and_the_validity_rule(modulated):
    """Integer offsets in [-2, 2] put samples on pixel centres, on coordinate -1 and on the far border.  Every sample is one pixel or nothing:
    forward, grad_input and grad_weight to 1e-5.  (The coordinate gradient is one-sided there and is left to the parity cases.)"""
    ops = support.ops()
    _, _, s, p, d, (group, dg) = INT_CASE
    (x, off, mask, w, b, go), y_ref, g_ref = _problem(INT_CASE, modulated, True)
    xg, og, mg, wg, bg, gg = _gpu((x, off, mask, w, b, go))
    close(ops.deform_conv2d_forward_raw(xg, wg, bg, og, mg, s, p, d, group, dg), y_ref, 1e-5, 'integer offsets fwd')
    got = ops.deform_conv2d_backward_raw(xg, wg, bg, og, mg, gg, s, p, d, group, dg)
    _compare_grads(got, g_ref, 1e-5, 'integer offsets', names=('grad_input', 'grad_weight'))


def test_plain_operator_equals_the_3d_entry_at_depth_one():
    """One plain case through dpf_deform_conv3d_* on a depth-1 volume with zero depth offsets, on the GPU: the same bars, and the forward bit for
    bit (corners 0-3 of the depth-1 trilinear rule carry the weight 1 a b in the bilinear rule's order, and a tile accumulates in one order)."""
    ops = support.ops()
    case = CASES[1]
    (B, C, K, H, W), (kh, kw), s, p, d, (group, dg) = case
    T = kh * kw
    (x, off, _, w, b, go), _, _ = _problem(case, False)
    xg, og, _, wg, bg, gg = _gpu((x, off, None, w, b, go))
    Ho, Wo = off.shape[2:]
    off3 = torch.zeros(B, dg, T, 3, 1, Ho, Wo, device=DEV)
    off3[:, :, :, 1:, 0] = og.reshape(B, dg, T, 2, Ho, Wo)
    off3 = off3.reshape(B, dg * 3 * T, 1, Ho, Wo)
    s3, p3, d3 = (1,) + s, (0,) + p, (1,) + d
    x3, w3, go3 = xg.unsqueeze(2).contiguous(), wg.unsqueeze(2).contiguous(), gg.unsqueeze(2).contiguous()
    y3 = ops.deform_conv_forward_raw(x3, w3, bg, off3, s3, p3, d3, group, dg)
    gi3, goff3, gw3, gb3 = ops.deform_conv_backward_raw(x3, w3, bg, off3, go3, s3, p3, d3, group, dg)
    y = ops.deform_conv2d_forward_raw(xg, wg, bg, og, None, s, p, d, group, dg)
    gi, goff, gm, gw, gb = ops.deform_conv2d_backward_raw(xg, wg, bg, og, None, gg, s, p, d, group, dg)
    assert gm is None
    close(y, y3.squeeze(2), 1e-4, '2d vs 3d fwd')
    assert torch.equal(y, y3.squeeze(2))
    close(gi, gi3.squeeze(2), 2e-4, '2d vs 3d grad_input')
    close(goff, goff3.reshape(B, dg, T, 3, Ho, Wo)[:, :, :, 1:].reshape(goff.shape), 2e-4, '2d vs 3d grad_offset')
    close(gw, gw3.squeeze(2), 2e-4, '2d vs 3d grad_weight')
    close(gb, gb3, 2e-4, '2d vs 3d grad_bias')


def test_null_mask_and_null_bias():
    """mask = NULL with bias = NULL: the plain operator without a bias; grad_mask and grad_bias are not produced."""
    ops = support.ops()
    case = CASES[1]
    _, _, s, p, d, (group, dg) = case
    (x, off, _, w, b, go), y_ref, g_ref = _problem(case, False)
    xg, og, _, wg, bg, gg = _gpu((x, off, None, w, b, go))
    y = ops.deform_conv2d_forward_raw(xg, wg, None, og, None, s, p, d, group, dg)
    close(y, y_ref - b.double().view(1, -1, 1, 1), 1e-4, 'no bias fwd')
    gi, goff, gm, gw, gb = ops.deform_conv2d_backward_raw(xg, wg, None, og, None, gg, s, p, d, group, dg)
    assert gm is None and gb is None
    _compare_grads((gi, goff, None, gw), g_ref, 2e-4, 'no bias', names=('grad_input', 'grad_offset', 'grad_weight'))


@pytest.mark.parametrize('C,K,kh,kw,group,dg,code', [
    (16, 8, 3, 3, 3, 1, 'DPF_ERR_INVALID_ARG'), (16, 6, 3, 3, 4, 1, 'DPF_ERR_INVALID_ARG'), (16, 8, 3, 3, 1, 3, 'DPF_ERR_INVALID_ARG'),
    (260, 8, 3, 3, 1, 1, 'DPF_ERR_UNSUPPORTED'), (8, 264, 3, 3, 1, 1, 'DPF_ERR_UNSUPPORTED'), (8, 8, 7, 8, 1, 1, 'DPF_ERR_UNSUPPORTED'),
])
def test_refusals_write_nothing(C, K, kh, kw, group, dg, code):
    """A grouping that does not divide: DPF_ERR_INVALID_ARG; C or K > 256 or more than 49 taps: DPF_ERR_UNSUPPORTED.  Nothing is launched:
    every output buffer keeps its sentinel."""
    from dualpixelface_amd._lib import DpfError, lib
    L = lib()
    B, H, W, T = 1, 8, 9, kh * kw
    ph, pw = kh // 2, kw // 2
    Ho, Wo = ref2d.out_size(H, W, kh, kw, 1, (ph, pw), 1)
    x, off, mask = [rnd(*sh, seed=360).to(DEV) for sh in ((B, C, H, W), (B, dg * 2 * T, Ho, Wo), (B, dg * T, Ho, Wo))]
    w, b, go = [rnd(*sh, seed=361).to(DEV) for sh in ((K, max(C // group, 1), kh, kw), (K,), (B, K, Ho, Wo))]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.empty(max(L.call('dpf_deform_conv2d_backward_workspace_floats', B, C, H, W, K, T), 1024), device=DEV)
    geo = (B, C, H, W, K, kh, kw, 1, 1, ph, pw, 1, 1, group, dg)
    out, gi, goff, gm, gw, gb = [torch.full_like(t, -7.25) for t in (go, x, off, mask, w, b)]
    with pytest.raises(DpfError, match=code):
        L.call('dpf_deform_conv2d_forward', ptr(x), ptr(w), ptr(b), ptr(off), ptr(mask), ptr(out), ptr(ws), *geo, st)
    with pytest.raises(DpfError, match=code):
        L.call('dpf_deform_conv2d_backward', ptr(x), ptr(w), ptr(b), ptr(off), ptr(mask), ptr(go), ptr(gi), ptr(goff), ptr(gm), ptr(gw), ptr(gb),
               ptr(ws), *geo, st)
    torch.cuda.synchronize()
    for t in (out, gi, goff, gm, gw, gb):
        assert (t == -7.25).all()


@pytest.mark.parametrize('modulated', [False, True], ids=['plain', 'modulated'])
def test_reproducibility(modulated):
    """Three tiles: grad_offset and grad_mask are stored once per element, so two backward calls agree bitwise in every mode; grad_input and
    grad_weight agree bitwise under deterministic mode, where the first call also meets the parity bars.  The mode is restored."""
    ops = support.ops()
    _, _, s, p, d, (group, dg) = THREE_TILES
    (x, off, mask, w, b, go), _, g_ref = _problem(THREE_TILES, modulated)
    xg, og, mg, wg, bg, gg = _gpu((x, off, mask, w, b, go))
    run = lambda: [None if t is None else t.clone() for t in ops.deform_conv2d_backward_raw(xg, wg, bg, og, mg, gg, s, p, d, group, dg)]
    before = ops.deterministic()
    a, c = run(), run()
    assert torch.equal(a[1], c[1])
    assert modulated == (a[2] is not None) and (a[2] is None or torch.equal(a[2], c[2]))
    with ops.deterministic_mode():
        a, c = run(), run()
    assert ops.deterministic() == before
    _compare_grads(a, g_ref, 2e-4, 'deterministic')
    for u, v, nm in zip(a, c, GRADS):
        assert (u is None and v is None) or torch.equal(u, v), nm


@pytest.mark.parametrize('modulated', [False, True], ids=['plain', 'modulated'])
def test_autograd_equals_the_raw_backward(modulated):
    """ops.deform_conv2d(...).backward(): the tensors' .grad are the raw backward's results (same kernels; grad_offset and grad_mask, which are
    reproducible in every mode, bitwise)."""
    ops = support.ops()
    _, _, s, p, d, (group, dg) = THREE_TILES
    (x, off, mask, w, b, go), y_ref, g_ref = _problem(THREE_TILES, modulated)
    ts = _gpu((x, off, mask, w, b))
    leaves = [None if t is None else t.clone().requires_grad_() for t in ts]
    y = ops.deform_conv2d(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], s, p, d, group, dg)
    close(y, y_ref, 1e-4, 'autograd fwd')
    y.backward(go.to(DEV))
    raw = ops.deform_conv2d_backward_raw(ts[0], ts[3], ts[4], ts[1], ts[2], go.to(DEV), s, p, d, group, dg)
    for l, r, ref, nm in zip(leaves, raw, g_ref, GRADS):
        if l is None:
            assert r is None
            continue
        close(l.grad, ref, 2e-4, 'autograd ' + nm)
        close(l.grad, r, 1e-5, 'autograd vs raw ' + nm)
        if nm in ('grad_offset', 'grad_mask'):
            assert torch.equal(l.grad, r), nm
    # only the weight wants a gradient: the data kernel is skipped, nothing else comes back
    wl = ts[3].clone().requires_grad_()
    ops.deform_conv2d(ts[0], ts[1], ts[2], wl, ts[4], s, p, d, group, dg).backward(go.to(DEV))
    close(wl.grad, g_ref[3], 2e-4, 'weight-only grad_weight')


def test_compat_module_plain_call_sequence():
    """deform_conv_cuda's plain three exactly as DeformConvFunction calls them (deform_conv.py:39-46,62-77): empty buffer tensors, zero-filled
    gradient tensors, kW before kH; then once more into a non-zero gradWeight: the result is added, scaled by `scale`."""
    import dualpixelface_amd.dcn2d_compat as D
    case = CASES[8]                                               # the non-square window: kW / kH and padW / padH must not be swapped
    (B, C, K, H, W), (kh, kw), s, p, d, (group, dg) = case
    (x, off, _, w, b, go), y_ref, g_ref = _problem(case, False)
    input, offset, weight, grad_output = _gpu((x, off, w, go))
    step = min(64, B)
    output = input.new_empty(y_ref.shape)
    bufs = [input.new_empty(0), input.new_empty(0)]
    D.deform_conv_forward_cuda(input, weight, offset, output, bufs[0], bufs[1], weight.size(3), weight.size(2), s[1], s[0], p[1], p[0], d[1], d[0],
                               group, dg, step)
    close(output, y_ref - b.double().view(1, -1, 1, 1), 1e-4, 'compat fwd')
    grad_input, grad_offset = torch.zeros_like(input), torch.zeros_like(offset)
    D.deform_conv_backward_input_cuda(input, offset, grad_output, grad_input, grad_offset, weight, bufs[0], weight.size(3), weight.size(2),
                                      s[1], s[0], p[1], p[0], d[1], d[0], group, dg, step)
    grad_weight = torch.zeros_like(weight)
    D.deform_conv_backward_parameters_cuda(input, offset, grad_output, grad_weight, bufs[0], bufs[1], weight.size(3), weight.size(2), s[1], s[0],
                                           p[1], p[0], d[1], d[0], group, dg, 1, step)
    close(grad_input, g_ref[0], 2e-4, 'compat grad_input')
    close(grad_offset, g_ref[1], 2e-4, 'compat grad_offset')
    close(grad_weight, g_ref[3], 2e-4, 'compat grad_weight')
    seeded = torch.full_like(weight, 3.0)
    D.deform_conv_backward_parameters_cuda(input, offset, grad_output, seeded, bufs[0], bufs[1], weight.size(3), weight.size(2), s[1], s[0],
                                           p[1], p[0], d[1], d[0], group, dg, 0.5, step)
    close(seeded, 3.0 + 0.5 * g_ref[3], 2e-4, 'compat grad_weight added into, scale 0.5')
    with pytest.raises(RuntimeError, match='im2col step'):
        D.deform_conv_forward_cuda(input.repeat(3, 1, 1, 1), weight, offset.repeat(3, 1, 1, 1), output.repeat(3, 1, 1, 1), bufs[0], bufs[1],
                                   weight.size(3), weight.size(2), s[1], s[0], p[1], p[0], d[1], d[0], group, dg, 2)


@pytest.mark.parametrize('with_bias', [True, False])
def test_compat_module_modulated_call_sequence(with_bias):
    """The modulated two exactly as ModulatedDeformConvFunction calls them (deform_conv.py:114-119,128-137)."""
    import dualpixelface_amd.dcn2d_compat as D
    case = CASES[1]
    (B, C, K, H, W), (kh, kw), s, p, d, (group, dg) = case
    assert s[0] == s[1] and p[0] == p[1] and d[0] == d[1]        # the reference's modulated layer takes one int each
    (x, off, m, w, b, go), y_ref, g_ref = _problem(case, True)
    input, offset, mask, weight, bias, grad_output = _gpu((x, off, m, w, b, go))
    if not with_bias:
        bias = input.new_empty(1)  # fake tensor
    output = input.new_empty(y_ref.shape)
    bufs = [input.new_empty(0), input.new_empty(0)]
    D.modulated_deform_conv_cuda_forward(input, weight, bias, bufs[0], offset, mask, output, bufs[1], weight.shape[2], weight.shape[3], s[0], s[0],
                                         p[0], p[0], d[0], d[0], group, dg, with_bias)
    close(output, y_ref if with_bias else y_ref - b.double().view(1, -1, 1, 1), 1e-4, 'compat modulated fwd')
    grad_input, grad_offset, grad_mask = torch.zeros_like(input), torch.zeros_like(offset), torch.zeros_like(mask)
    grad_weight, grad_bias = torch.zeros_like(weight), torch.zeros_like(bias)
    D.modulated_deform_conv_cuda_backward(input, weight, bias, bufs[0], offset, mask, bufs[1], grad_input, grad_weight, grad_bias, grad_offset,
                                          grad_mask, grad_output, weight.shape[2], weight.shape[3], s[0], s[0], p[0], p[0], d[0], d[0], group, dg,
                                          with_bias)
    got = (grad_input, grad_offset, grad_mask, grad_weight, grad_bias)
    _compare_grads(got, g_ref, 2e-4, 'compat modulated', names=GRADS if with_bias else GRADS[:4])
    if not with_bias:
        assert (grad_bias == 0).all()


def test_compat_module_rejects_wrong_window_and_groups_through_its_functions():
    """The five public functions, on GPU tensors: a window that is not the weight's (kH and kW given the wrong way round for a 1 x 3 weight) and
    a group count that does not divide raise RuntimeError, and the result tensors keep their sentinel."""
    import dualpixelface_amd.dcn2d_compat as D
    case = CASES[8]                                               # 1 x 3 window
    (B, C, K, H, W), (kh, kw), s, p, d, (group, dg) = case
    (x, off, m, w, b, go), y_ref, _ = _problem(case, True)
    input, offset, mask, weight, bias, grad_output = _gpu((x, off, m, w, b, go))
    e = input.new_empty(0)
    output = torch.full(y_ref.shape, -7.25, device=DEV)
    gi, goff, gm, gw, gb = [torch.full_like(t, -7.25) for t in (input, offset, mask, weight, bias)]
    plain = (s[1], s[0], p[1], p[0], d[1], d[0])
    mod = (s[0], s[1], p[0], p[1], d[0], d[1])
    # the window the wrong way round -- (kW, kH) = (1, 3) in the plain three, (kernel_h, kernel_w) = (3, 1) in the modulated two; then the right
    # window with group 3, which does not divide 8 channels
    for pwin, mwin, grp, match in (((kh, kw), (kw, kh), group, 'kernel shape'), ((kw, kh), (kh, kw), 3, 'divide')):
        with pytest.raises(RuntimeError, match=match):
            D.deform_conv_forward_cuda(input, weight, offset, output, e, e, *pwin, *plain, grp, dg, 1)
        with pytest.raises(RuntimeError, match=match):
            D.deform_conv_backward_input_cuda(input, offset, grad_output, gi, goff, weight, e, *pwin, *plain, grp, dg, 1)
        with pytest.raises(RuntimeError, match=match):
            D.deform_conv_backward_parameters_cuda(input, offset, grad_output, gw, e, e, *pwin, *plain, grp, dg, 1.0, 1)
        with pytest.raises(RuntimeError, match=match):
            D.modulated_deform_conv_cuda_forward(input, weight, bias, e, offset, mask, output, e, *mwin, *mod, grp, dg, True)
        with pytest.raises(RuntimeError, match=match):
            D.modulated_deform_conv_cuda_backward(input, weight, bias, e, offset, mask, e, gi, gw, gb, goff, gm, grad_output, *mwin, *mod, grp, dg, True)
    torch.cuda.synchronize()
    for t in (output, gi, goff, gm, gw, gb):
        assert (t == -7.25).all()


def test_grad_bias_of_a_batch_beyond_one_channel_sum_launch():
    """B K = 256 x 256 > 65535 rows: grad_bias is reduced in two slices of whole images (255 + 1) and equals the plain sum of grad_output
    (2e-4 of its maximum, the bar of every gradient here); outside deterministic mode its partial sums meet in float atomics, so it is
    compared, not required to repeat bitwise."""
    ops = support.ops()
    B, C, K, H, W = 256, 2, 256, 3, 3
    x, off, w, b = rnd(B, C, H, W, seed=380), rnd(B, 2, H, W, seed=381), rnd(K, C, 1, 1, seed=382, scale=0.1), rnd(K, seed=383)
    go = rnd(B, K, H, W, seed=384)
    xg, og, wg, bg, gg = _gpu((x, off, w, b, go))
    got = ops.deform_conv2d_backward_raw(xg, wg, bg, og, None, gg, (1, 1), (0, 0), (1, 1), want=(False, False, False, False, True))
    assert all(t is None for t in got[:4])
    close(got[4], go.double().sum(dim=(0, 2, 3)), 2e-4, 'grad_bias, 256 images x 256 channels')
