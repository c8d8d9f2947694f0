"""GPU parity tests of rank 3 of the gather family (csrc/dcn_gather.hip) for every grouping: the deformable 3-D convolution with group /
deformable_group > 1, and with (1, 1) at shapes that the lean, region and packed-scatter tiers of csrc/dcn3d.hip decline (K > 64), so that the
family's backward serves them as the single-group fallback (their forward is the gather kernel of csrc/dcn3d.hip).  Called through the C ABI (ops.deform_conv_forward_raw / ops.deform_conv_backward_raw),
against oracle.dcn3d.deform_conv3d_forward_grouped in fp64 and its fp64 autograd (tests/test_oracle_dcn.py pins that to F.conv3d(groups)).

Tolerances: the operator's own at these operand scales (x 1, offset 1.2, weight 0.1, bias 1; tests/test_gpu_ops.py): forward 1e-4, every
gradient 2e-4 of the reference tensor's maximum.  Known answers with plain fp32 summation: 1e-5.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import support
from tests.support import DEV, close, rnd

pytestmark = pytest.mark.gpu

GRADS = ('grad_input', 'grad_offset', 'grad_weight', 'grad_bias')


K3, ONE = (3, 3, 3), (1, 1, 1)
BASE = (2, 16, 8, 3, 6, 12)     # 216 voxels: three full 64-voxel tiles and a tail of 24
# Single-group fallback.  K = 96 > 64: dcn_lean_forward and dcn_fwd_region (forward), dcn_bwd_grad_input and dcn_bwd_offset_weight (backward)
# all decline on K > 64, so with no switch set the forward comes from the gather kernel of dcn3d.hip and all four gradients from the family,
# grad_input by atomics.  Three row tiles.
SINGLE = ((1, 16, 96, 2, 6, 12), K3, ONE, ONE, ONE, (1, 1))


def _cases():
    rows = [
        (BASE, K3, ONE, ONE, ONE, [(2, 1), (1, 2), (2, 2), (2, 4), (4, 2)]),
        ((1, 16, 8, 3, 6, 12), K3, ONE, ONE, ONE, [(2, 1), (1, 2), (2, 2), (2, 4), (4, 2)]),
        # (3, 2): conv group 1 straddles two offset groups; (2, 3): offset group 1 straddles two conv groups
        ((1, 12, 6, 2, 5, 9), K3, ONE, ONE, ONE, [(3, 2), (1, 3), (3, 1), (2, 3)]),
        ((2, 10, 4, 3, 7, 10), K3, ONE, ONE, ONE, [(2, 5), (2, 1)]),                        # C / group = 5 is odd; 210 voxels
        ((1, 8, 16, 2, 5, 9), K3, ONE, ONE, ONE, [(8, 1), (8, 8), (4, 8)]),                 # depthwise: one input channel per group, two outputs
        ((2, 16, 8, 2, 9, 13), (1, 3, 3), (1, 2, 2), (0, 1, 1), ONE, [(2, 2), (4, 1)]),     # strided, 9 taps
        ((1, 16, 8, 4, 8, 11), K3, ONE, (2, 2, 2), (2, 2, 2), [(2, 4)]),                    # dilated
        ((1, 96, 96, 2, 6, 12), K3, ONE, ONE, ONE, [(2, 3)]),                               # more than one 32-row matrix tile per group
        ((1, 128, 128, 1, 4, 8), K3, ONE, ONE, ONE, [(4, 2)]),                              # the channel limit
        ((1, 64, 64, 1, 4, 8), K3, ONE, ONE, ONE, [(2, 2)]),                                # K = 64: four forward tiles, one accumulator on every wave
        # (1, 1) on the single-group entry; each has K > 64, which every other tier declines (see SINGLE)
        SINGLE[:5] + ([SINGLE[5]],),
        ((1, 128, 128, 1, 4, 8), K3, ONE, ONE, ONE, [(1, 1)]),                              # the channel limit: 16 weight-gradient tiles (NA = 4), 8 gcol tiles
        ((1, 15, 96, 2, 9, 13), (1, 3, 3), (1, 2, 2), (0, 1, 1), ONE, [(1, 1)]),            # odd C (the zeroed pad row), stride 2, 9 taps, a tail tile
    ]
    return [(shape, k, s, p, d, g) for shape, k, s, p, d, gs in rows for g in gs]


def _id(case):
    shape, k, s, p, d, g = case
    return 'x'.join(map(str, shape)) + '-k%d%d%d-s%d-d%d-g%d-dg%d' % (k + (s[2], d[2]) + g)


@functools.lru_cache(maxsize=None)
def _problem(case, integer_offsets=False):
    """-> inputs (fp32, CPU), grad_output, the oracle's fp64 forward and its four fp64 autograd gradients; computed once per case and shared."""
    from oracle import dcn3d
    (B, C, K, D, H, W), k, s, p, d, (group, dg) = case
    T = k[0] * k[1] * k[2]
    x = rnd(B, C, D, H, W, seed=340)
    w, b = rnd(K, C // group, *k, seed=342, scale=0.1), rnd(K, seed=343)
    xd, wd, bd = [t.double().requires_grad_() for t in (x, w, b)]
    # (the offset tensor has the output's spatial size: take it from a zero-offset pass of the plain grouped convolution)
    osp = F.conv3d(x[:1, :1], torch.zeros(1, 1, *k), stride=s, padding=p, dilation=d).shape[2:]
    if integer_offsets:
        off = torch.randint(-2, 3, (B, dg * 3 * T) + tuple(osp), generator=torch.Generator().manual_seed(341)).float()
    else:
        off = rnd(B, dg * 3 * T, *osp, seed=341, scale=1.2)
    od = off.double().requires_grad_()
    y_ref = dcn3d.deform_conv3d_forward_grouped(xd, od, wd, bd, stride=s, pad=p, dil=d, group=group, deformable_group=dg)
    go = rnd(*y_ref.shape, seed=344)
    g_ref = torch.autograd.grad(y_ref, (xd, od, wd, bd), go.double())
    return (x, off, w, b, go), y_ref.detach(), tuple(g.detach() for g in g_ref)


def _gpu(ts):
    return [t.to(DEV) for t in ts]


def _check_case(case, integer_offsets=False):
    ops = support.ops()
    _, _, s, p, d, (group, dg) = case
    (x, off, w, b, go), y_ref, g_ref = _problem(case, integer_offsets)
    xg, og, wg, bg, gg = _gpu((x, off, w, b, go))
    y = ops.deform_conv_forward_raw(xg, wg, bg, og, s, p, d, group, dg)
    close(y, y_ref, 1e-4, 'grouped dcn fwd')
    got = ops.deform_conv_backward_raw(xg, wg, bg, og, gg, s, p, d, group, dg)
    for a, r, nm in zip(got, g_ref, GRADS):
        close(a, r, 2e-4, 'grouped dcn ' + nm)


@pytest.mark.parametrize('case', _cases(), ids=_id)
def test_grouped_parity_forward_and_gradients(case):
    """Forward and all four gradients of the native grouped path against the oracle (fp64) and its autograd."""
    _check_case(case)


def _fwd(x, off, w, b, group, dg):
    return support.ops().deform_conv_forward_raw(x.to(DEV), w.to(DEV), b.to(DEV), off.to(DEV), ONE, ONE, ONE, group, dg)


@pytest.mark.parametrize('group', [2, 4])
def test_zero_offsets_equal_the_plain_grouped_convolution(group):
    """Zero offsets: F.conv3d(groups=group) whatever deformable_group is (plain fp32 summation: 1e-5 of the maximum)."""
    B, C, K, D, H, W = BASE
    x, w, b = rnd(B, C, D, H, W, seed=350), rnd(K, C // group, 3, 3, 3, seed=351, scale=0.1), rnd(K, seed=352)
    ref = F.conv3d(x.double(), w.double(), b.double(), padding=1, groups=group)
    for dg in (1, 2, 4, 16):
        close(_fwd(x, torch.zeros(B, dg * 81, D, H, W), w, b, group, dg), ref, 1e-5, 'zero offsets, deformable_group %d' % dg)


def test_integer_offset_to_one_deformable_group_shifts_its_channels():
    """Offset +1 along w given to deformable group 1 of 2 only: the grouped convolution of an input whose channels C/2 .. C-1 are shifted by one
    voxel with zero fill (the validity rule of cuh:248 supplies the zeros).  As in tests/test_oracle_dcn.py:123-131 the FIRST column is left
    out: its left tap reads x[0] through the offset but the padding of the shifted tensor in the plain convolution; the last column is
    compared."""
    B, C, K, D, H, W = BASE
    group = 2
    x, w, b = rnd(B, C, D, H, W, seed=353), rnd(K, C // group, 3, 3, 3, seed=354, scale=0.1), rnd(K, seed=355)
    off = torch.zeros(B, 2 * 81, D, H, W)
    off[:, 81 + 2::3] = 1.0                              # offset channel 3 tap + 2 = the w coordinate, second deformable group
    xs = x.clone()
    xs[:, C // 2:, :, :, :-1] = x[:, C // 2:, :, :, 1:]
    xs[:, C // 2:, :, :, -1] = 0
    ref = F.conv3d(xs.double(), w.double(), b.double(), padding=1, groups=group)
    close(_fwd(x, off, w, b, group, 2)[..., 1:], ref[..., 1:], 1e-5, 'shifted deformable group')


def test_integer_offsets_and_the_validity_rule():
    """Random integer offsets in [-2, 2] put samples on voxel centres, on coordinate -1 and on the far border: a sample outside the OPEN interval
    (-1, size) has no value and no coordinate derivative (deform_im2col_cuda.cuh:248) -- forward and gradients against the oracle."""
    _check_case(((1, 8, 8, 3, 5, 6), K3, ONE, ONE, ONE, (2, 2)), integer_offsets=True)
    _check_case(((1, 8, 96, 3, 5, 6), K3, ONE, ONE, ONE, (1, 1)), integer_offsets=True)     # K > 64: the single-group fallback


@pytest.mark.parametrize('case', [(BASE, K3, ONE, ONE, ONE, (2, 2)), SINGLE], ids=_id)
def test_grad_input_channels_cut_inside_a_group(case):
    """gi_channels = 10 of 16 with (2, 2): the cut falls inside conv group 1 and offset group 1; with (1, 1) on the single-group fallback it
    falls inside the one group.  grad_input[:, :10] is the oracle's, grad_input[:, 10:] exactly zero, the other three gradients are unchanged."""
    ops = support.ops()
    (x, off, w, b, go), _, g_ref = _problem(case)
    xg, og, wg, bg, gg = _gpu((x, off, w, b, go))
    gi, goff, gw, gb = ops.deform_conv_backward_raw(xg, wg, bg, og, gg, ONE, ONE, ONE, *case[5], gi_channels=10)
    close(gi[:, :10], g_ref[0][:, :10], 2e-4, 'grad_input[:, :10]')
    assert (gi[:, 10:] == 0).all()
    for a, r, nm in zip((goff, gw, gb), g_ref[1:], GRADS[1:]):
        close(a, r, 2e-4, 'gi_channels: ' + nm)


@pytest.mark.parametrize('case', [(BASE, K3, ONE, ONE, ONE, (2, 4)), (BASE, K3, ONE, ONE, ONE, (4, 2)), SINGLE], ids=_id)
def test_deterministic_mode_is_bitwise_reproducible(case):
    """Under ops.deterministic_mode() five backward launches return the same bits for all four gradients (the first meets the parity
    tolerances); outside it grad_offset is still bitwise equal over five launches: every element is written once, by one workgroup."""
    ops = support.ops()
    groups = case[5]
    (x, off, w, b, go), _, g_ref = _problem(case)
    xg, og, wg, bg, gg = _gpu((x, off, w, b, go))
    with ops.deterministic_mode():
        runs = [[t.clone() for t in ops.deform_conv_backward_raw(xg, wg, bg, og, gg, ONE, ONE, ONE, *groups)] for _ in range(5)]
    for a, r, nm in zip(runs[0], g_ref, GRADS):
        close(a, r, 2e-4, 'deterministic ' + nm)
    for other in runs[1:]:
        for a, o, nm in zip(runs[0], other, GRADS):
            assert torch.equal(a, o), nm
    goffs = [ops.deform_conv_backward_raw(xg, wg, bg, og, gg, ONE, ONE, ONE, *groups)[1].clone() for _ in range(5)]
    for o in goffs[1:]:
        assert torch.equal(goffs[0], o)


@pytest.mark.parametrize('C,K,group,dg', [(16, 8, 3, 1), (16, 6, 4, 1), (16, 8, 1, 3)])
def test_refused_groupings_write_nothing(C, K, group, dg):
    """A group count that does not divide C or K, or a deformable_group that does not divide C: DPF_ERR_INVALID_ARG, nothing launched, the
    output buffers keep their contents."""
    import ctypes
    from dualpixelface_amd._lib import DpfError, lib
    ops = support.ops()
    B, D, H, W = 1, 2, 4, 6
    x, off = rnd(B, C, D, H, W, seed=360).to(DEV), rnd(B, dg * 81, D, H, W, seed=361).to(DEV)
    w, b = rnd(K, max(C // group, 1), 3, 3, 3, seed=362).to(DEV), rnd(K, seed=363).to(DEV)
    go = rnd(B, K, D, H, W, seed=364).to(DEV)
    with pytest.raises(DpfError, match='DPF_ERR_INVALID_ARG'):
        ops.deform_conv_forward_raw(x, w, b, off, ONE, ONE, ONE, group, dg)
    with pytest.raises(DpfError, match='DPF_ERR_INVALID_ARG'):
        ops.deform_conv_backward_raw(x, w, b, off, go, ONE, ONE, ONE, group, dg)
    # the same calls with buffers of our own, pre-filled with a sentinel
    L = lib()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.empty(max(L.call('dpf_deform_conv3d_backward_workspace_floats', B, C, D, H, W, K, 27), 1024), device=DEV)
    geo = (B, C, D, H, W, K, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, group, dg, 64)
    out, gi, goff, gw, gb = [torch.full_like(t, -7.25) for t in (go, x, off, w, b)]
    with pytest.raises(DpfError, match='DPF_ERR_INVALID_ARG'):
        L.call('dpf_deform_conv3d_forward', ptr(x), ptr(w), ptr(b), ptr(off), ptr(out), ptr(ws), *geo, st)
    with pytest.raises(DpfError, match='DPF_ERR_INVALID_ARG'):
        L.call('dpf_deform_conv3d_backward', ptr(x), ptr(w), ptr(b), ptr(off), ptr(go), ptr(gi), ptr(goff), ptr(gw), ptr(gb), ptr(ws), *geo, C,
               st)
    torch.cuda.synchronize()
    for t in (out, gi, goff, gw, gb):
        assert (t == -7.25).all()


def test_autograd_surface_takes_the_grouping():
    """ops.deform_conv3d(..., group=2, deformable_group=2): torch.autograd.grad matches the oracle's gradients."""
    ops = support.ops()
    case = (BASE, K3, ONE, ONE, ONE, (2, 2))
    (x, off, w, b, go), y_ref, g_ref = _problem(case)
    xg, og, wg, bg = [t.to(DEV).requires_grad_() for t in (x, off, w, b)]
    y = ops.deform_conv3d(xg, og, wg, bg, group=2, deformable_group=2)
    close(y, y_ref, 1e-4, 'autograd fwd')
    for a, r, nm in zip(torch.autograd.grad(y, (xg, og, wg, bg), go.to(DEV)), g_ref, GRADS):
        close(a, r, 2e-4, 'autograd ' + nm)


def test_dcn_compat_allocates_nothing_per_piece():
    """After a warm call, DCN.deform_conv_forward with (2, 4) performs no more allocations than the same call with (1, 1): the output tensor
    and nothing per group."""
    import dualpixelface_amd.dcn_compat as DCN
    B, C, K, D, H, W = BASE

    def allocations(group, dg):
        x, off = rnd(B, C, D, H, W, seed=370).to(DEV), rnd(B, dg * 81, D, H, W, seed=371).to(DEV)
        w, b = rnd(K, C // group, 3, 3, 3, seed=372, scale=0.1).to(DEV), rnd(K, seed=373).to(DEV)
        ints = (3, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, group, dg, 64)
        DCN.deform_conv_forward(x, w, b, off, *ints)     # warm: library, scratch
        torch.cuda.synchronize()
        n0 = torch.cuda.memory_stats()['allocation.all.allocated']
        y = DCN.deform_conv_forward(x, w, b, off, *ints)
        torch.cuda.synchronize()
        return torch.cuda.memory_stats()['allocation.all.allocated'] - n0, y

    single, _ = allocations(1, 1)
    grouped, _ = allocations(2, 4)
    print('allocations per call: (1, 1) %d, (2, 4) %d' % (single, grouped))
    assert grouped <= single
