"""The operators DPNet adds (run with ``-m gpu``), each against fp32 PyTorch on the CPU with the bounds of tests/test_gpu_ops.py:
max-pool (bitwise, ties and NaN included), the general depthwise window, 28...49-tap convolutions under every fp32 matrix path,
ConvTranspose2d k4 s2 with padding 1 / 2 / 4, padded 1x1 convolutions without BatchNorm, and the smooth-L1 loss over up to eight heads."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import support
from tests.support import DEV, close, close_elem, rnd

pytestmark = pytest.mark.gpu


def int_bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ max-pool
POOLS = [(3, 1, 0), (3, 2, 0), (7, 2, 1)]
POOL_SIZES = [(2, 5, 17, 23), (1, 3, 32, 300), (2, 11, 30, 46), (1, 2, 9, 10)]          # odd / even, W % 4 != 0, W > 256


def _pool_input(kind, shape, seed):
    x = rnd(*shape, seed=seed)
    if kind == 'ties':                   # four levels and a constant border: ties are the common case
        x = torch.round(x.clamp(-1.5, 1.5))
        x = (x * 0.5).clamp(-0.5, 1.0)
        x[..., 0, :] = 0.25
        x[..., -1, :] = 0.25
        x[..., :, 0] = 0.25
        x[..., :, -1] = 0.25
    elif kind == 'nan':
        x[0, 0, shape[2] // 2, shape[3] // 2] = float('nan')
        x[-1, -1, 1, 1] = float('nan')
    return x


@pytest.mark.parametrize('kind', ['random', 'ties', 'nan'])
@pytest.mark.parametrize('shape', POOL_SIZES)
@pytest.mark.parametrize('k,s,p', POOLS)
def test_maxpool_bitwise(k, s, p, shape, kind):
    ops = support.ops()
    x = _pool_input(kind, shape, seed=3).requires_grad_()
    y_ref, i_ref = F.max_pool2d(x, k, s, p, return_indices=True)
    g = torch.randint(-3, 4, y_ref.shape, generator=torch.Generator().manual_seed(4)).float()   # integer-valued: every sum is exact
    gx_ref, = torch.autograd.grad(y_ref, x, g)
    xg = x.detach().to(DEV).requires_grad_()
    y, idx = ops.max_pool2d(xg, k, s, p, return_indices=True)
    assert y.shape == y_ref.shape
    assert torch.equal(int_bits(y), int_bits(y_ref))
    assert torch.equal(idx.cpu().long(), i_ref)
    gx, = torch.autograd.grad(y, xg, g.to(DEV), retain_graph=True)
    assert torch.equal(int_bits(gx), int_bits(gx_ref))
    gx2, = torch.autograd.grad(y, xg, g.to(DEV))                      # (no deterministic mode: the backward is a gather)
    assert torch.equal(int_bits(gx), int_bits(gx2))


def test_maxpool_backward_reproducible_on_real_gradients():
    ops = support.ops()
    assert not ops.deterministic()
    x = _pool_input('ties', (2, 16, 64, 260), seed=5).to(DEV).requires_grad_()
    g = rnd(2, 16, 31, 129, seed=6).to(DEV)
    y = ops.max_pool2d(x, 3, 2, 0)
    a, = torch.autograd.grad(y, x, g, retain_graph=True)
    b, = torch.autograd.grad(y, x, g)
    assert torch.equal(int_bits(a), int_bits(b))
    xc = x.detach().cpu().requires_grad_()
    ref, = torch.autograd.grad(F.max_pool2d(xc, 3, 2, 0), xc, g.cpu())
    close_elem(a, ref, 'pool backward')


def test_maxpool_refuses_unsupported_windows():
    from dualpixelface_amd._lib import DpfError
    ops = support.ops()
    x = rnd(1, 1, 16, 16).to(DEV)
    for k, s, p in ((9, 1, 0), (3, 3, 0), (3, 1, 2)):
        with pytest.raises(DpfError):
            ops.max_pool2d(x, k, s, p)


# ------------------------------------------------------------------------------------------------ depthwise, general window
@pytest.mark.parametrize('C', [11, 16, 128])
@pytest.mark.parametrize('k,pad', [(3, 0), (3, 1), (3, 2), (3, 3), (1, 0), (1, 1)])
def test_depthwise_general(k, pad, C):
    ops = support.ops()
    x = rnd(2, C, 9, 14, seed=8).requires_grad_()
    w = rnd(C, 1, k, k, seed=9).requires_grad_()
    y_ref = F.conv2d(x, w, None, 1, pad, 1, C)
    go = rnd(*y_ref.shape, seed=10)
    gx_r, gw_r = torch.autograd.grad(y_ref, (x, w), go)
    xg, wg = x.detach().to(DEV).requires_grad_(), w.detach().to(DEV).requires_grad_()
    y = ops.depthwise_conv2d(xg, wg, pad)
    close_elem(y, y_ref, 'dw fwd')
    gx, gw = torch.autograd.grad(y, (xg, wg), go.to(DEV))
    close_elem(gx, gx_r, 'dw dgrad')
    close(gw, gw_r, 1e-4, 'dw wgrad')
    with ops.deterministic_mode():
        a = torch.autograd.grad(ops.depthwise_conv2d(xg, wg, pad), wg, go.to(DEV))[0]
        b = torch.autograd.grad(ops.depthwise_conv2d(xg, wg, pad), wg, go.to(DEV))[0]
        assert torch.equal(int_bits(a), int_bits(b))
        close(a, gw_r, 1e-4, 'dw wgrad (deterministic)')
    if (k, pad) == (3, 1):                 # the existing call keeps its kernels: the same bits through either entry
        y3 = ops.depthwise_conv3x3(xg, wg)
        assert torch.equal(int_bits(y), int_bits(y3))
        gx3, _ = torch.autograd.grad(y3, (xg, wg), go.to(DEV))
        assert torch.equal(int_bits(gx), int_bits(gx3))


def test_depthwise_wide_rows():
    ops = support.ops()
    x = rnd(1, 16, 6, 301, seed=18).requires_grad_()
    w = rnd(16, 1, 3, 3, seed=19).requires_grad_()
    y_ref = F.conv2d(x, w, None, 1, 3, 1, 16)
    go = rnd(*y_ref.shape, seed=20)
    gx_r, gw_r = torch.autograd.grad(y_ref, (x, w), go)
    xg, wg = x.detach().to(DEV).requires_grad_(), w.detach().to(DEV).requires_grad_()
    y = ops.depthwise_conv2d(xg, wg, 3)
    close_elem(y, y_ref, 'dw fwd')
    gx, gw = torch.autograd.grad(y, (xg, wg), go.to(DEV))
    close_elem(gx, gx_r, 'dw dgrad')
    close(gw, gw_r, 1e-4, 'dw wgrad')


# ------------------------------------------------------------------------------------------------ wide-window dense conv
# C, K, (kh, kw), stride, pad: DPNet's six 7x7 shapes (modules.py:44, mainmodel.py:81-85), then a 6x6 and a 5x7 window
WIDE = [(6, 8, (7, 7), 2, 1), (128, 1, (7, 7), 1, 1), (64, 1, (7, 7), 1, 0), (32, 1, (7, 7), 1, 1), (32, 1, (7, 7), 1, 1), (8, 1, (7, 7), 1, 1),
        (5, 3, (6, 6), 1, 2), (7, 9, (5, 7), 2, 3)]
WIDE_IDS = ['stem', 'head5', 'head4', 'head3', 'head2', 'head1', 'k6x6', 'k5x7']


@pytest.mark.parametrize('path', [2, 1, 0])
@pytest.mark.parametrize('bias', [False, True])
@pytest.mark.parametrize('hw', [(20, 28), (33, 71)])
@pytest.mark.parametrize('case', WIDE, ids=WIDE_IDS)
def test_wide_conv(case, hw, bias, path):
    ops = support.ops()
    C, K, (kh, kw), s, p = case
    x = rnd(2, C, hw[0], hw[1], seed=30).requires_grad_()
    w = rnd(K, C, kh, kw, seed=31, scale=(2.0 / (C * kh * kw)) ** 0.5).requires_grad_()
    b = rnd(K, seed=32).requires_grad_() if bias else None
    y_ref = F.conv2d(x, w, b, s, p)
    go = rnd(*y_ref.shape, seed=33)
    refs = torch.autograd.grad(y_ref, (x, w) + ((b,) if bias else ()), go)
    xg, wg = x.detach().to(DEV).requires_grad_(), w.detach().to(DEV).requires_grad_()
    bg = b.detach().to(DEV).requires_grad_() if bias else None
    prev = ops.f32_matrix_path()
    ops.set_f32_matrix_path(path)
    try:
        y = ops.conv2d(xg, wg, bg, s, p)
        got = torch.autograd.grad(y, (xg, wg) + ((bg,) if bias else ()), go.to(DEV))
        st = {}
        y_st = ops.conv2d(xg, wg, bg, s, p, stats=st)               # a BatchNorm's statistics request is declined, not mishandled
        assert not st and torch.equal(int_bits(y_st), int_bits(y))
        with ops.deterministic_mode():
            a = torch.autograd.grad(ops.conv2d(xg, wg, bg, s, p), wg, go.to(DEV))[0]
            c = torch.autograd.grad(ops.conv2d(xg, wg, bg, s, p), wg, go.to(DEV))[0]
    finally:
        ops.set_f32_matrix_path(prev)
    close(y, y_ref, 1e-4, 'wide fwd')
    close(got[0], refs[0], 1e-4, 'wide dgrad')
    close(got[1], refs[1], 2e-4, 'wide wgrad')
    if bias:
        close(got[2], refs[2], 1e-4, 'wide bias grad')
    assert torch.equal(int_bits(a), int_bits(c))
    close(a, refs[1], 2e-4, 'wide wgrad (deterministic)')


def test_wide_conv_same_bits_on_every_matrix_path():
    ops = support.ops()
    x, w = rnd(1, 8, 24, 40, seed=34).to(DEV), rnd(1, 8, 7, 7, seed=35).to(DEV)
    prev = ops.f32_matrix_path()
    try:
        outs = []
        for path in (0, 1, 2):
            ops.set_f32_matrix_path(path)
            outs.append(ops.conv2d(x, w, None, 1, 1))
    finally:
        ops.set_f32_matrix_path(prev)
    assert torch.equal(int_bits(outs[0]), int_bits(outs[1])) and torch.equal(int_bits(outs[0]), int_bits(outs[2]))


# ------------------------------------------------------------------------------------------------ transposed 2-D conv, padded 1x1
@pytest.mark.parametrize('hw', [(6, 8), (9, 13)])
@pytest.mark.parametrize('cin,cout,pad', [(128, 32, 1), (128, 16, 2), (64, 16, 4), (32, 8, 4)])
def test_conv_transpose2d(cin, cout, pad, hw):
    ops = support.ops()
    x = rnd(2, cin, hw[0], hw[1], seed=40).requires_grad_()
    w = rnd(cin, cout, 4, 4, seed=41, scale=(2.0 / (cin * 4)) ** 0.5).requires_grad_()
    y_ref = F.conv_transpose2d(x, w, None, 2, pad)
    assert y_ref.shape[2] == 2 * hw[0] + 2 - 2 * pad
    go = rnd(*y_ref.shape, seed=42)
    gx_r, gw_r = torch.autograd.grad(y_ref, (x, w), go)
    xg, wg = x.detach().to(DEV).requires_grad_(), w.detach().to(DEV).requires_grad_()
    y = ops.conv_transpose2d(xg, wg, 2, pad)
    close(y, y_ref, 1e-4, 'deconv fwd')
    gx, gw = torch.autograd.grad(y, (xg, wg), go.to(DEV))
    close(gx, gx_r, 1e-4, 'deconv dgrad')
    close(gw, gw_r, 2e-4, 'deconv wgrad')


@pytest.mark.parametrize('hw', [(8, 12), (7, 10)])
@pytest.mark.parametrize('cin,cout,pad', [(16, 32, 1), (32, 128, 1), (32, 64, 2), (14, 11, 1)])
def test_padded_pointwise_conv(cin, cout, pad, hw):
    ops = support.ops()
    x = rnd(2, cin, hw[0], hw[1], seed=50).requires_grad_()
    w = rnd(cout, cin, 1, 1, seed=51, scale=(2.0 / cin) ** 0.5).requires_grad_()
    y_ref = F.conv2d(x, w, None, 1, pad)
    go = rnd(*y_ref.shape, seed=52)
    gx_r, gw_r = torch.autograd.grad(y_ref, (x, w), go)
    xg, wg = x.detach().to(DEV).requires_grad_(), w.detach().to(DEV).requires_grad_()
    y = ops.conv2d(xg, wg, None, 1, pad)
    close(y, y_ref, 1e-4, '1x1 fwd')
    assert float(y.detach()[:, :, 0].abs().max()) == 0.0              # the border the padding adds: exact zeros (no bias)
    gx, gw = torch.autograd.grad(y, (xg, wg), go.to(DEV))
    close(gx, gx_r, 1e-4, '1x1 dgrad')
    close(gw, gw_r, 2e-4, '1x1 wgrad')


# ------------------------------------------------------------------------------------------------ loss heads
@pytest.mark.parametrize('n', [5, 8])
def test_smooth_l1_many_heads(n):
    ops = support.ops()
    wts = [1.0, 0.75294, 0.18824, 0.047059, 0.011765, 0.5, 0.25, 0.125][:n]
    pd = (rnd(2, n, 24, 36, seed=60) * 2).requires_grad_()
    disp = rnd(2, 24, 36, seed=61)
    mask = (torch.rand(2, 24, 36, generator=torch.Generator().manual_seed(62)) < 0.8).float()
    d = pd.double() - disp.double().unsqueeze(1)
    per = torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5) * mask.double().unsqueeze(1)
    ref = sum(wts[k] * per[:, k].sum() / mask.double().sum() for k in range(n))
    gref, = torch.autograd.grad(ref, pd)
    pg = pd.detach().to(DEV).requires_grad_()
    out = ops.stereo_losses(pg, None, disp.to(DEV), None, mask.to(DEV), wts, 1.0, 0.0)
    close(out[0], ref.float(), 1e-5, 'smoothL1')
    close(out[2], ref.float(), 1e-5, 'final')
    g, = torch.autograd.grad(out[2], pg)
    close_elem(g, gref.float(), 'd pred_depth')


def test_more_than_eight_heads_is_an_error():
    from dualpixelface_amd._lib import DpfError
    ops = support.ops()
    with pytest.raises(DpfError):
        ops.stereo_losses(torch.zeros(1, 9, 8, 8, device=DEV), None, torch.zeros(1, 8, 8, device=DEV), None, torch.ones(1, 8, 8, device=DEV),
                          [1.0] * 9, 1.0, 0.0)


@pytest.mark.parametrize('mode', ['ones', 'bern'])
def test_up_to_four_heads_keep_their_bits(mode, golden_dir):
    """tests/golden/loss.npz through the eight-head build: the fixture's values at the fixture's bound (the per-head sums are formed
    and added in the same order as before), and the same bits on a second run in deterministic mode."""
    ops = support.ops()
    g = np.load(golden_dir + '/loss.npz')
    t = lambda k: torch.from_numpy(g[mode + '_' + k]).to(DEV)
    with ops.deterministic_mode():
        out = ops.stereo_losses(t('pred_depth'), t('pred_normal')[:, 0], t('disp'), t('normal'), t('mask'), [1.0, 0.7, 0.5], 1.0, 1.0)
        again = ops.stereo_losses(t('pred_depth'), t('pred_normal')[:, 0], t('disp'), t('normal'), t('mask'), [1.0, 0.7, 0.5], 1.0, 1.0)
    for i, k in enumerate(('smoothL1_loss', 'cosine_loss', 'final_loss')):
        close(out[i], torch.from_numpy(g[mode + '_' + k]), 1e-5, k)
    assert torch.equal(int_bits(out), int_bits(again))
