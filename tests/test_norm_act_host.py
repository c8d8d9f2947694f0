"""tests/norm_act_cpu.py (the closed-form fp64 yardstick of test_gpu_norm_act.py) against torch.autograd in fp64, on small shapes, for every
mode / activation / operand-subset combination the GPU tests use.  Bar: 1e-12 of each tensor's scale.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import norm_act_cpu as na

N, C, S = 3, 4, 7

# (mode, act, weight and bias, res, res2) -- the combinations of test_gpu_norm_act.py
COMBOS = [
    (1, na.ACT_PRELU, True, True, True),        # row chunks
    (3, na.ACT_SIGMOID, True, False, False),
    (2, na.ACT_RELU, True, False, False),
    (1, na.ACT_RELU, True, False, False),       # reduce chunk, SyncBatchNorm, hard statistics
    (1, na.ACT_NONE, True, False, False),       # norm_act_concat, training and eval
    (2, na.ACT_NONE, True, False, False),
    (1, na.ACT_PRELU, True, True, False),       # operand subsets
    (1, na.ACT_PRELU, True, False, True),
    (1, na.ACT_PRELU, True, False, False),
    (3, na.ACT_RELU, False, False, False),
    (3, na.ACT_SIGMOID, True, True, True),
    (0, na.ACT_PRELU, False, True, False),
    (0, na.ACT_PRELU, False, False, False),
    (0, na.ACT_LEAKY, False, False, False),
    (0, na.ACT_LEAKY, False, False, True),
]


def _rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _autograd(x, w, b, slope, res, res2, rm, rv, mode, act, slope_const):
    if mode == 1:
        z = F.batch_norm(x, rm, rv, w, b, True, 0.1, 1e-5)
    elif mode == 2:
        z = F.batch_norm(x, rm, rv, w, b, False, 0.1, 1e-5)
    elif mode == 3:
        z = F.instance_norm(x, None, None, w, b, True, 0.1, 1e-5)
    else:
        z = x
    if res is not None:
        z = z + res
    y = {na.ACT_NONE: lambda t: t, na.ACT_RELU: F.relu, na.ACT_PRELU: lambda t: F.prelu(t, slope),
         na.ACT_LEAKY: lambda t: F.leaky_relu(t, slope_const), na.ACT_SIGMOID: torch.sigmoid}[act](z)
    return y + res2 if res2 is not None else y


def _close(a, b, name):
    assert a.shape == b.shape, (name, a.shape, b.shape)
    scale = max(b.abs().max().item(), 1e-6)
    err = (a - b).abs().max().item()
    assert err <= 1e-12 * scale, '%s: max err %.3e vs scale %.3e' % (name, err, scale)


@pytest.mark.parametrize('combo', COMBOS, ids=lambda c: 'mode%d-act%d-wb%d-res%d-res2%d' % c)
def test_closed_form_matches_autograd(combo):
    mode, act, has_wb, has_res, has_res2 = combo
    leaf = lambda t: t.requires_grad_()
    x = leaf(_rnd(N, C, S, seed=1) * 2 + 0.7)
    w = leaf(torch.rand(C, generator=torch.Generator().manual_seed(2), dtype=torch.float64) + 0.5) if has_wb else None
    b = leaf(_rnd(C, seed=3)) if has_wb else None
    slope = leaf(torch.tensor([0.17], dtype=torch.float64)) if act == na.ACT_PRELU else None
    res = leaf(_rnd(N, C, S, seed=4)) if has_res else None
    res2 = leaf(_rnd(N, C, S, seed=5)) if has_res2 else None
    rm, rv = _rnd(C, seed=6) * 0.1, torch.rand(C, generator=torch.Generator().manual_seed(7), dtype=torch.float64) + 0.5
    rm_r, rv_r = rm.clone(), rv.clone()
    go = _rnd(N, C, S, seed=8) + 0.5
    y_ref = _autograd(x, w, b, slope, res, res2, rm_r if mode in (1, 2) else None, rv_r if mode in (1, 2) else None, mode, act, 0.1)
    names = ('dx', 'dw', 'db', 'dslope', 'dres', 'dres2')
    leaves = (x, w, b, slope, res, res2)
    wanted = [(nm, t) for nm, t in zip(names, leaves) if t is not None]
    grads = dict(zip([nm for nm, _ in wanted], torch.autograd.grad(y_ref, [t for _, t in wanted], go)))
    out = na.norm_act(x, w, b, slope, res, res2, rm, rv, mode, act, 0.1, go)
    _close(out['y'], y_ref.detach(), 'y')
    if mode in (1, 2):
        _close(out['running_mean'], rm_r, 'running_mean')
        _close(out['running_var'], rv_r, 'running_var')
        assert (mode == 1) != torch.equal(rm_r, rm)                  # training moved them, eval did not
    for nm in names:
        if nm in grads:
            _close(out[nm], grads[nm], nm)
        else:
            assert out[nm] is None, nm


def test_statistics_are_taken_over_the_right_axes():
    """Batch norm: one statistic per channel over samples and positions; instance norm: one per sample and channel."""
    x = _rnd(N, C, S, seed=11) * torch.arange(1, N + 1, dtype=torch.float64).view(N, 1, 1) + 3.0
    y1 = na.norm_act(x, mode=1)['y']
    y3 = na.norm_act(x, mode=3)['y']
    assert y1.mean((0, 2)).abs().max() < 1e-12 and (y1.var((0, 2), unbiased=False) - 1).abs().max() < 1e-4
    assert y3.mean(2).abs().max() < 1e-12 and (y3.var(2, unbiased=False) - 1).abs().max() < 1e-4
    assert y1.mean(2).abs().max() > 1e-3


def test_close_channels_sees_a_small_channel_behind_a_large_one():
    b = torch.ones(2, 3, 5, dtype=torch.float64)
    b[:, 0] *= 1e4
    a = b.clone()
    a[1, 2, 3] += 1e-3                                               # 1e-7 of the tensor's scale, 1e-3 of its channel's
    na.close_channels(b, b, 1e-5)
    with pytest.raises(AssertionError):
        na.close_channels(a, b, 1e-5, 'small channel')
    na.close_channels(a, b, 1e-5, bars=[0.0, 0.0, 2e-3])             # a per-channel bar replaces the bound where it is larger
    v = torch.tensor([1e4, 1.0])
    with pytest.raises(AssertionError):
        na.close_channels(v + torch.tensor([0.0, 1e-3]), v, 1e-5, 'vector element')
