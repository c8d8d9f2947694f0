"""Deformable conv backward, weight-gradient partial dW[k][c][t] = sum_v go[k][v] S[c][v] of dcn_lean_bwd_offset_kernel on matrix path 2
(two f16 components per operand, three partial products on v_mfma_f32_16x16x32_f16; go rows and x channels carry their own exponent)
against the fp64 oracle, with the fp32 matrix instruction (dpf_set_f32_matrix_path(0)) as the yardstick measured in the same test.

Error metric of a grad_weight element: |dW - dW64| / den, den = the oracle's grad_weight for (|x|, |go|) = sum |go| S(|x|) -- the element's
own inputs, not the tensor's maximum."""
import functools

import pytest
import torch

from tests import support
from tests.support import DEV, close, rnd
from tests.test_gpu_ops import _spread

pytestmark = pytest.mark.gpu

SHAPES = [(1, 35, 64, 4, 12, 36), (1, 64, 64, 4, 8, 36)]      # 12- and 16-wide chunks, several tiles, a partial tile column
LAYOUTS = ['xchan', 'gochan', 'xwbands', 'plain']


@functools.lru_cache(maxsize=None)
def _wgrad_case(cfg, layout):
    """Inputs and fp64 references of one (shape, layout); computed once, shared, never modified."""
    from oracle import dcn3d
    B, C, K, D, H, W = cfg
    x, off = rnd(B, C, D, H, W, seed=430), rnd(B, 81, D, H, W, seed=431, scale=0.7)
    wt, bs = rnd(K, C, 3, 3, 3, seed=432, scale=0.1), rnd(K, seed=433)
    go_plain = rnd(B, K, D, H, W, seed=434)
    go = go_plain
    if layout == 'xchan':
        x = _spread(x, 'chan', seed=435)
    if layout == 'xwbands':
        x = _spread(x, 'wbands', seed=435)
    if layout == 'gochan':
        go = _spread(go_plain, 'chan', seed=436)
    xd, od, wd, bd, gd = x.double(), off.double(), wt.double(), bs.double(), go.double()
    gi_ref, goff_ref, dw_ref, _ = dcn3d.deform_conv3d_backward(xd, od, wd, bd, gd)
    dw_den = dcn3d.deform_conv3d_backward(xd.abs(), od, wd, bd, gd.abs())[2]
    gi_den = dcn3d.deform_conv3d_backward(xd, od, wd.abs(), bd, gd.abs())[0]
    goff_plain = goff_ref if go is go_plain else dcn3d.deform_conv3d_backward(xd, od, wd, bd, go_plain.double())[1]
    band = gd.abs().sum(dim=1, keepdim=True) / go_plain.double().abs().sum(dim=1, keepdim=True)
    goff_den = band * goff_plain.pow(2).mean().sqrt()
    return dict(x=x, off=off, wt=wt, bs=bs, go=go, gi_ref=gi_ref, goff_ref=goff_ref, dw_ref=dw_ref, dw_den=dw_den, gi_den=gi_den,
                goff_den=goff_den)


def _backward(c):
    ops = support.ops()
    xg, og, wg, bg = [c[k].to(DEV).requires_grad_() for k in ('x', 'off', 'wt', 'bs')]
    y = ops.deform_conv3d(xg, og, wg, bg)
    return torch.autograd.grad(y, (xg, og, wg, bg), c['go'].to(DEV))


def _errors(c, grads):
    gi, goff, dw = [g.double().cpu() for g in grads[:3]]
    nz = c['gi_den'] > 0
    return (((dw - c['dw_ref']).abs() / c['dw_den']).max().item(),
            ((gi - c['gi_ref']).abs()[nz] / c['gi_den'][nz]).max().item(),
            ((goff - c['goff_ref']).abs() / c['goff_den']).max().item())


def _on_path(path, fn):
    from dualpixelface_amd._lib import lib
    prev = lib().cdll.dpf_get_f32_matrix_path()
    try:
        lib().call('dpf_set_f32_matrix_path', path)
        return fn()
    finally:
        lib().call('dpf_set_f32_matrix_path', prev)


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('cfg', SHAPES)
def test_grad_weight_f16_component_path_relative_to_own_inputs(cfg, layout):
    """x channels / go rows / x column bands at 1 .. 2^-34 of the tile's maximum, and plain data: every grad_weight element within 2 x the
    worst element of the fp32 matrix instruction (+ 1e-7) relative to sum |go| S(|x|); grad_input and grad_offset keep the bars of
    test_deform_conv_backward_f16_component_path_in_block_dynamic_range (the packed sample tile feeds neither)."""
    c = _wgrad_case(cfg, layout)
    assert (c['dw_den'] > 0).all()               # a condition on the inputs: every element has a non-zero scale of its own
    errs = {path: _on_path(path, lambda: _errors(c, _backward(c))) for path in (0, 2)}
    print('grad_weight / grad_input / grad_offset errors, path 0 and path 2:', cfg, layout, errs)
    assert errs[2][0] <= 2 * errs[0][0] + 1e-7, errs
    assert errs[2][1] <= 2 * errs[0][1] + 1e-7, errs
    assert errs[2][2] <= 2 * errs[0][2] + 1e-7, errs
    assert errs[0][2] <= 5e-5, errs


@pytest.mark.parametrize('cfg', [(1, 20, 40, 3, 9, 20, 1.5),      # K no multiple of 16, D < 4, 12-wide chunks, partial tile rows
                                 (1, 16, 24, 4, 7, 44, 4.0)])     # offsets past the staged halo: the cooperative slow path writes the tile
def test_grad_weight_f16_component_path_masks(cfg):
    from oracle import dcn3d
    B, C, K, D, H, W, oscale = cfg
    c = dict(x=rnd(B, C, D, H, W, seed=440), off=rnd(B, 81, D, H, W, seed=441, scale=oscale), wt=rnd(K, C, 3, 3, 3, seed=442, scale=0.1),
             bs=rnd(K, seed=443), go=rnd(B, K, D, H, W, seed=444))
    ref = dcn3d.deform_conv3d_backward(c['x'], c['off'], c['wt'], c['bs'], c['go'])
    got = _on_path(2, lambda: _backward(c))
    for a, r, nm in zip(got, ref, ('grad_input', 'grad_offset', 'grad_weight', 'grad_bias')):
        close(a, r, 2e-4, 'dcn ' + nm)


def test_grad_weight_f16_component_path_zero_channel_and_zero_row():
    """An x channel and a go row of zeros take the smallest exponent the scales allow: their grad_weight slices are exact zeros and
    nothing else is disturbed."""
    from oracle import dcn3d
    B, C, K, D, H, W = 1, 16, 24, 4, 8, 16
    c = dict(x=rnd(B, C, D, H, W, seed=450), off=rnd(B, 81, D, H, W, seed=451, scale=1.5), wt=rnd(K, C, 3, 3, 3, seed=452, scale=0.1),
             bs=rnd(K, seed=453), go=rnd(B, K, D, H, W, seed=454))
    c['x'][:, 3] = 0
    c['go'][:, 5] = 0
    ref = dcn3d.deform_conv3d_backward(c['x'], c['off'], c['wt'], c['bs'], c['go'])
    got = _on_path(2, lambda: _backward(c))
    dw = got[2].cpu()
    assert (dw[:, 3] == 0).all() and (dw[5] == 0).all()
    for a, r, nm in zip(got, ref, ('grad_input', 'grad_offset', 'grad_weight', 'grad_bias')):
        assert torch.isfinite(a).all(), nm
        close(a, r, 2e-4, 'dcn ' + nm)


@pytest.mark.parametrize('layout', ['xchan', 'gochan'])
@pytest.mark.parametrize('cfg', SHAPES)
def test_grad_weight_f16_component_path_reproducible(cfg, layout):
    """Deterministic mode, x channels resp. go rows at 1 .. 2^-34: five backward launches return the same grad_weight bits (the channel
    exponents are found through LDS atomics; an integer max does not depend on their order), and the first one meets the accuracy bar.
    (The spread sits in ONE operand per case: deterministic mode sums in fixed point with a unit of 2^-56, on every matrix path, so
    products of two operands that are both 2^-34 down lie below what it can hold.)"""
    ops = support.ops()
    c = _wgrad_case(cfg, layout)
    assert (c['dw_den'] > 0).all()

    def five():
        with ops.deterministic_mode():
            first = _backward(c)
            for i in range(4):
                again = _backward(c)[2]
                assert torch.equal(again, first[2]), (i, (again - first[2]).abs().max().item())
        return _errors(c, first)

    e2 = _on_path(2, five)
    e0 = _on_path(0, lambda: _errors(c, _backward(c)))
    print('grad_weight error, deterministic path 2 and path 0:', cfg, layout, e2[0], e0[0])
    assert e2[0] <= 2 * e0[0] + 1e-7, (e2, e0)


@pytest.mark.parametrize('det', [False, True])
def test_grad_weight_f16_component_path_slow_samples_beyond_the_channel_scale(det):
    """A channel's exponent covers the cells staged for its tile.  Channel 3 is 2^-20 inside the staged box of the middle tile column
    (columns 12 .. 35 of 44: tile 16 .. 31 plus its halo) and O(1) outside, and the offsets (sigma 4) carry about a quarter of that tile's
    samples outside the box: those samples are 2^20 above the channel's scale, cannot enter the f16 tile, and are added to grad_weight
    directly -- in default mode with float atomics, in deterministic mode through the integer shadow.  All gradients within
    test_deform_conv's 2e-4, and grad_weight per element within 2 x the fp32 matrix instruction relative to sum |go| S(|x|)."""
    from oracle import dcn3d
    ops = support.ops()
    B, C, K, D, H, W = 1, 16, 24, 4, 7, 44
    c = dict(x=rnd(B, C, D, H, W, seed=460), off=rnd(B, 81, D, H, W, seed=461, scale=4.0), wt=rnd(K, C, 3, 3, 3, seed=462, scale=0.1),
             bs=rnd(K, seed=463), go=rnd(B, K, D, H, W, seed=464))
    c['x'][:, 3, :, :, 12:36] *= 2.0 ** -20
    xd, od, wd, bd, gd = [c[k].double() for k in ('x', 'off', 'wt', 'bs', 'go')]
    ref = dcn3d.deform_conv3d_backward(xd, od, wd, bd, gd)
    den = dcn3d.deform_conv3d_backward(xd.abs(), od, wd, bd, gd.abs())[2]
    assert (den > 0).all()

    def run():
        if det:
            with ops.deterministic_mode():
                return _backward(c)
        return _backward(c)

    got = {path: _on_path(path, run) for path in (0, 2)}
    for a, r, nm in zip(got[2], ref, ('grad_input', 'grad_offset', 'grad_weight', 'grad_bias')):
        close(a, r, 2e-4, 'dcn ' + nm)
    err = {path: ((got[path][2].double().cpu() - ref[2]).abs() / den).max().item() for path in (0, 2)}
    print('grad_weight error with slow samples above the channel scale, path 0 and path 2:', 'deterministic' if det else 'atomic', err)
    assert err[2] <= 2 * err[0] + 1e-7, err
