"""Host-side tests of the 2-D deformable convolution: the fp64 helper of the GPU parity tests (tests/dcn2d_cpu.py) is pinned to three
independent statements of the operator, and the argument checks of the drop-in module, the workspace queries and the header run without a GPU.
"""
import ctypes
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from tests import dcn2d_cpu as ref2d
from tests import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


rnd = functools.partial(support.rnd, dtype=torch.float64)


def maxerr(a, b):
    return (a - b).abs().max().item()


# (B, C, K, H, W), (kh, kw), stride, pad, dil, (group, dg)
ORACLE_CASES = [
    ((2, 8, 4, 7, 9), (3, 3), (1, 1), (1, 1), (1, 1), (1, 1)),
    ((1, 8, 4, 7, 9), (3, 3), (1, 1), (1, 1), (1, 1), (2, 4)),
    ((1, 12, 6, 6, 8), (3, 3), (2, 2), (1, 1), (1, 1), (3, 2)),
    ((1, 8, 8, 9, 8), (3, 3), (1, 1), (2, 2), (2, 2), (2, 1)),
    ((1, 6, 4, 6, 9), (1, 3), (1, 2), (0, 1), (1, 1), (2, 3)),
]


@pytest.mark.parametrize('case', ORACLE_CASES, ids=lambda c: 'x'.join(map(str, c[0])) + '-k%dx%d-g%d-dg%d' % (c[1] + c[5]))
def test_helper_equals_the_3d_oracle_at_depth_one(case):
    """Mask absent: forward and all four gradients equal oracle.dcn3d.deform_conv3d_forward_grouped on a depth-1 volume with zero depth
    offsets (<= 1e-12; both are fp64)."""
    from oracle import dcn3d
    (B, C, K, H, W), (kh, kw), s, p, d, (group, dg) = case
    T = kh * kw
    Ho, Wo = ref2d.out_size(H, W, kh, kw, s, p, d)
    x, w, b = rnd(B, C, H, W, seed=1), rnd(K, C // group, kh, kw, seed=2, scale=0.1), rnd(K, seed=3)
    off = rnd(B, dg * 2 * T, Ho, Wo, seed=4, scale=2.5)
    go = rnd(B, K, Ho, Wo, seed=5)
    leaves = [t.clone().requires_grad_() for t in (x, off, w, b)]
    y = ref2d.deform_conv2d_ref(leaves[0], leaves[1], None, leaves[2], leaves[3], s, p, d, group, dg)
    g = torch.autograd.grad(y, leaves, go)

    off3 = torch.zeros(B, dg, T, 3, 1, Ho, Wo, dtype=torch.float64)
    off3[:, :, :, 1:, 0] = off.reshape(B, dg, T, 2, Ho, Wo)
    leaves3 = [t.clone().requires_grad_() for t in (x.unsqueeze(2), off3.reshape(B, dg * 3 * T, 1, Ho, Wo), w.unsqueeze(2), b)]
    y3 = dcn3d.deform_conv3d_forward_grouped(*leaves3, stride=(1,) + s, pad=(0,) + p, dil=(1,) + d, group=group, deformable_group=dg)
    g3 = torch.autograd.grad(y3, leaves3, go.unsqueeze(2))
    assert maxerr(y, y3.squeeze(2)) <= 1e-12
    assert maxerr(g[0], g3[0].squeeze(2)) <= 1e-12
    assert maxerr(g[1], g3[1].reshape(B, dg, T, 3, Ho, Wo)[:, :, :, 1:].reshape(off.shape)) <= 1e-12
    assert maxerr(g[2], g3[2].squeeze(2)) <= 1e-12
    assert maxerr(g[3], g3[3]) <= 1e-12


@pytest.mark.parametrize('group,stride,dil,dg', [(1, 1, 1, 1), (2, 2, 1, 4), (4, 1, 2, 2)])
def test_helper_with_zero_offsets_is_the_plain_convolution(group, stride, dil, dg):
    """Zero offsets and a constant mask of 0.5: 0.5 F.conv2d(groups) without the bias, whatever deformable_group is."""
    B, C, K, H, W = 2, 8, 8, 9, 11
    x, w, b = rnd(B, C, H, W, seed=6), rnd(K, C // group, 3, 3, seed=7), rnd(K, seed=8)
    Ho, Wo = ref2d.out_size(H, W, 3, 3, stride, dil, dil)
    off = torch.zeros(B, dg * 18, Ho, Wo, dtype=torch.float64)
    mask = torch.full((B, dg * 9, Ho, Wo), 0.5, dtype=torch.float64)
    y = ref2d.deform_conv2d_ref(x, off, mask, w, b, stride, dil, dil, group, dg)
    want = 0.5 * F.conv2d(x, w, None, stride, dil, dil, group) + b.view(1, K, 1, 1)
    assert maxerr(y, want) <= 1e-12
    assert maxerr(ref2d.deform_conv2d_ref(x, off, None, w, b, stride, dil, dil, group, dg), F.conv2d(x, w, b, stride, dil, dil, group)) <= 1e-12


def shifted_taps_reference(x, off, mask, w, b, pad):
    """Integer offsets, stride 1, dilation 1, one deformable group: every tap gathered explicitly from a zero-padded copy of the image."""
    B, C, H, W = x.shape
    K, _, kh, kw = w.shape
    Ho, Wo = off.shape[2:]
    R = 8                                                       # wider than any |offset| + window used
    xp = F.pad(x, (R, R, R, R))
    ys = torch.arange(Ho).view(1, Ho, 1)
    xs = torch.arange(Wo).view(1, 1, Wo)
    out = torch.zeros(B, K, Ho, Wo, dtype=x.dtype)
    for t in range(kh * kw):
        i, j = t // kw, t % kw
        hh = (ys - pad + i + off[:, 2 * t].long()).clamp(-R, H - 1 + R) + R
        ww = (xs - pad + j + off[:, 2 * t + 1].long()).clamp(-R, W - 1 + R) + R
        bi = torch.arange(B).view(B, 1, 1).expand(B, Ho, Wo)
        tap = xp[bi, :, hh, ww].permute(0, 3, 1, 2)             # [B, C, Ho, Wo]
        if mask is not None:
            tap = tap * mask[:, t].unsqueeze(1)
        out = out + torch.einsum('bchw,kc->bkhw', tap, w[:, :, i, j])
    return out + b.view(1, K, 1, 1)


def test_helper_with_integer_offsets_reads_shifted_zero_padded_taps():
    B, C, K, H, W = 2, 4, 3, 7, 9
    x, w, b = rnd(B, C, H, W, seed=9), rnd(K, C, 3, 3, seed=10), rnd(K, seed=11)
    off = torch.randint(-3, 4, (B, 18, H, W), generator=torch.Generator().manual_seed(12)).double()
    mask = torch.sigmoid(rnd(B, 9, H, W, seed=13))
    for m in (None, mask):
        assert maxerr(ref2d.deform_conv2d_ref(x, off, m, w, b, 1, 1, 1), shifted_taps_reference(x, off, m, w, b, 1)) <= 1e-12


def test_helper_output_is_linear_in_the_mask():
    B, C, K, H, W, dg = 1, 8, 4, 6, 7, 2
    x, w = rnd(B, C, H, W, seed=14), rnd(K, C // 2, 3, 3, seed=15)
    off = rnd(B, dg * 18, H, W, seed=16, scale=1.5)
    m1, m2 = rnd(B, dg * 9, H, W, seed=17), rnd(B, dg * 9, H, W, seed=18)
    f = lambda m: ref2d.deform_conv2d_ref(x, off, m, w, None, 1, 1, 1, 2, dg)
    assert maxerr(f(0.3 * m1 - 1.7 * m2), 0.3 * f(m1) - 1.7 * f(m2)) <= 1e-12
    assert maxerr(f(torch.zeros_like(m1)), torch.zeros(B, K, H, W, dtype=torch.float64)) == 0.0


# ------------------------------------------------------------------------------------------ drop-in module, argument checks (no GPU)
def _plain_args(B=2, C=4, K=4, H=6, W=7, group=1, dg=1):
    x, w = torch.randn(B, C, H, W), torch.randn(K, C // group, 3, 3)
    off, out = torch.randn(B, dg * 18, H, W), torch.empty(B, K, H, W)
    return x, w, off, out


def test_compat_rejects_cpu_tensors():
    import dualpixelface_amd.dcn2d_compat as D
    x, w, off, out = _plain_args()
    e = x.new_empty(0)
    with pytest.raises(RuntimeError, match='CUDA'):
        D.deform_conv_forward_cuda(x, w, off, out, e, e, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 2)
    with pytest.raises(RuntimeError, match='CUDA'):
        D.deform_conv_backward_input_cuda(x, off, out, torch.zeros_like(x), torch.zeros_like(off), w, e, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 2)
    with pytest.raises(RuntimeError, match='CUDA'):
        D.deform_conv_backward_parameters_cuda(x, off, out, torch.zeros_like(w), e, e, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1.0, 2)
    mask, b = torch.rand(2, 9, 6, 7), torch.randn(4)
    with pytest.raises(RuntimeError, match='CUDA'):
        D.modulated_deform_conv_cuda_forward(x, w, b, e, off, mask, out, e, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, True)
    with pytest.raises(RuntimeError, match='CUDA'):
        D.modulated_deform_conv_cuda_backward(x, w, b, e, off, mask, e, torch.zeros_like(x), torch.zeros_like(w), torch.zeros_like(b),
                                              torch.zeros_like(off), torch.zeros_like(mask), out, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, True)


def test_compat_rejects_non_contiguous_tensors():
    """(checked before the device, so it shows here)"""
    import dualpixelface_amd.dcn2d_compat as D
    x, w, off, out = _plain_args()
    e = x.new_empty(0)
    xt = torch.randn(2, 4, 7, 6).transpose(2, 3)
    assert not xt.is_contiguous()
    with pytest.raises(RuntimeError, match='contiguous'):
        D.deform_conv_forward_cuda(xt, w, off, out, e, e, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 2)
    with pytest.raises(RuntimeError, match='contiguous'):
        D.modulated_deform_conv_cuda_forward(x, w, torch.randn(4), e, off, torch.rand(2, 6, 7, 9).permute(0, 3, 1, 2), out, e, 3, 3, 1, 1, 1, 1,
                                             1, 1, 1, 1, True)


def test_compat_rejects_wrong_window_groups_and_step():
    import dualpixelface_amd.dcn2d_compat as D
    x, w, off, _ = _plain_args()
    geo = lambda kH, kW, group, dg, o=off, m=None: D._geometry(x, w, o, m, kH, kW, 1, 1, 1, 1, 1, 1, group, dg)
    assert geo(3, 3, 1, 1) == ((1, 1), (1, 1), (1, 1), (2, 4, 6, 7))
    with pytest.raises(RuntimeError, match='kernel shape'):
        geo(3, 5, 1, 1)
    with pytest.raises(RuntimeError, match='divide'):
        geo(3, 3, 3, 1)
    with pytest.raises(RuntimeError, match='divide'):
        geo(3, 3, 1, 3)
    with pytest.raises(RuntimeError, match='kernel channels'):
        geo(3, 3, 2, 1)                                         # the weight has C channels per group, not C / 2
    with pytest.raises(RuntimeError, match='offset shape'):
        geo(3, 3, 1, 2)                                         # two deformable groups need 36 offset channels
    with pytest.raises(RuntimeError, match='mask shape'):
        geo(3, 3, 1, 1, m=torch.rand(2, 18, 6, 7))
    D._step(1, 4), D._step(2, 4), D._step(4, 4)
    for step in (3, 8, 0):
        with pytest.raises(RuntimeError, match='im2col step'):
            D._step(step, 4)


# ------------------------------------------------------------------------------------------ C ABI without a GPU
def test_workspace_queries_are_positive_and_monotone():
    from dualpixelface_amd._lib import lib
    L = lib()
    fwd = lambda C, K, T: L.call('dpf_deform_conv2d_workspace_floats', C, K, T)
    bwd = lambda B, C, H, W, K, T: L.call('dpf_deform_conv2d_backward_workspace_floats', B, C, H, W, K, T)
    grid = [1, 2, 3, 5, 16, 31, 32, 33, 64, 100, 255, 256]
    for vary in range(3):
        prev = 0
        for v in grid:
            args = [12, 20, 9]
            args[vary] = min(v, 49) if vary == 2 else v
            cur = fwd(*args)
            assert cur > 0 and cur >= prev, (vary, v, cur, prev)
            prev = cur
    for det in (0, 1):
        L.call('dpf_set_deterministic', det)
        try:
            for vary in range(6):
                prev = 0
                for v in grid:
                    args = [2, 12, 9, 11, 20, 9]
                    args[vary] = min(v, 49) if vary == 5 else v
                    cur = bwd(*args)
                    assert cur > 0 and cur >= prev and cur >= fwd(args[1], args[4], args[5]), (det, vary, v, cur, prev)
                    prev = cur
        finally:
            L.call('dpf_set_deterministic', 0)


def test_header_declares_the_2d_entry_points():
    from dualpixelface_amd import _lib
    protos = _lib.parse_header()
    names = ['dpf_deform_conv2d_workspace_floats', 'dpf_deform_conv2d_backward_workspace_floats', 'dpf_deform_conv2d_forward',
             'dpf_deform_conv2d_backward']
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert n in protos and hasattr(cdll, n), n
    fwd = [a for _, a in protos['dpf_deform_conv2d_forward'][1]]
    assert fwd[:7] == ['input', 'weight', 'bias', 'offset', 'mask', 'output', 'ws'] and fwd[-3:] == ['group', 'deformable_group', 'stream']
    bwd = [a for _, a in protos['dpf_deform_conv2d_backward'][1]]
    assert bwd[:12] == ['input', 'weight', 'bias', 'offset', 'mask', 'grad_output', 'grad_input', 'grad_offset', 'grad_mask', 'grad_weight',
                        'grad_bias', 'ws']
    assert bwd[12:] == fwd[7:]
