"""The photometric and smoothness losses on the GPU (run with ``-m gpu``): csrc/photometric.hip through ops.photometric_loss and
ops.smoothness_loss against the restatements of tests/photometric_cpu.py.

Exact: the warped luminance and the counted map equal the fp32 numpy restatement bit for bit.  Bounded: the loss against the fp64
restatement within 2 x (the fp32 restatement's own deviation from fp64) + one fp32 ulp of the value (the kernel hands back an fp32
scalar); d pred against the fp64 autograd gradient, element-wise, within 2 x (the largest deviation of the fp32 autograd gradient from it)
+ 1e-6 of the largest gradient magnitude.  The fp32 figures are computed here, on the same input, not fixed in advance.
"""
import numpy as np
import pytest
import torch

from tests import photometric_cpu as pc
from tests import support
from tests.support import DEV, bits, tensor

pytestmark = pytest.mark.gpu


def _call_photometric(c, gout=None, backward=True, **over):
    """The photometric operator on a case dict (fields replaced by `over`) -> (loss as a float, warped, counted, d pred) as numpy arrays."""
    c = dict(c, **over)
    p = tensor(c['pred']).requires_grad_(True)
    loss, warped, cnt = support.ops().photometric_loss(p, tensor(c['ref_rgb']), tensor(c['tgt_rgb']), ab=tensor(c['ab']),
                                                       mask=tensor(c['mask']), head_weights=c['head_weights'], target_type=c['target_type'],
                                                       shift=c['shift'], alpha=c['alpha'], eps=c['eps'], return_warped=True)
    assert loss.shape == () and loss.dtype == torch.float32 and warped.dtype == torch.float32 and cnt.dtype == torch.uint8
    grad = None
    if backward:
        (loss if gout is None else loss * gout).backward()
        grad = p.grad.cpu().numpy()
    return float(loss.detach().double()), warped.cpu().numpy(), cnt.cpu().numpy(), grad


def _smooth(c, **over):
    """The smoothness operator on a case dict -> (loss as a float, d pred)."""
    c = dict(c, **over)
    p = tensor(c['pred']).requires_grad_(True)
    loss = support.ops().smoothness_loss(p, tensor(c['ref_rgb']), mask=tensor(c['mask']), head_weights=c['head_weights'], gamma=c['gamma'],
                                         eps=c['eps'])
    assert loss.shape == () and loss.dtype == torch.float32
    loss.backward()
    return float(loss.detach().double()), p.grad.cpu().numpy()


def _bounded(tag, ref, loss, grad, r32_loss):
    own_loss = abs(r32_loss - ref['loss64'])
    err_loss = abs(loss - ref['loss64'])
    g64, g32 = ref['grad64'], ref['grad32']
    own = float(np.abs(g32 - g64).max())
    bar = 2.0 * own + 1e-6 * float(np.abs(g64).max())
    err = float(np.abs(grad.astype(np.float64) - g64).max())
    print('%s: loss %.9g, |loss - fp64| %.3e (bar 2 x %.3e + ulp %.3e); max |d pred - fp64 autograd| %.3e (bar %.3e = 2 x %.3e + 1e-6 x %.3e)'
          % (tag, loss, err_loss, own_loss, support.ulp_of(ref['loss64']), err, bar, own, np.abs(g64).max()))
    assert np.isfinite(grad).all()
    assert err_loss <= 2.0 * own_loss + support.ulp_of(ref['loss64'])
    assert (np.abs(grad.astype(np.float64) - g64) <= bar).all(), (err, bar)
    assert not grad[g64 == 0].any()                                  # every element is written: exactly 0 where nothing reaches it


# ---- 1. the forward, exactly
@pytest.mark.parametrize('name', sorted(pc.CASES))
def test_warped_values_and_counted_map_equal_the_fp32_restatement(name):
    ref = pc.case(name)
    loss, warped, cnt, _ = _call_photometric(ref['case'], backward=False)
    r32 = ref['r32']
    assert np.array_equal(cnt, r32['counted'])
    assert np.array_equal(bits(warped), bits(r32['warped'])), float(np.abs(warped - r32['warped']).max())
    print('forward %s: %d of %d pixels counted, loss %.9g (fp32 restatement %.9g)' % (name, cnt.sum(), cnt.size, loss, r32['loss']))


def test_identical_views_at_zero_displacement_warp_to_the_reference_luminance():
    c = pc.case('multi-tile-19x70')['case']
    pred = np.zeros_like(c['pred'])
    _, warped, cnt, _ = _call_photometric(c, tgt_rgb=c['ref_rgb'], pred=pred, backward=False)
    Y = pc.luma(c['ref_rgb'])
    on = c['mask'] > 0                                               # pred = 0 sends every sample to its own pixel: warpable = the mask
    for h in range(pred.shape[1]):
        assert np.array_equal(bits(warped[:, h][on]), bits(Y[on])) and not warped[:, h][~on].any()
    assert 0 < cnt.sum() < cnt.size


# ---- 2. loss and gradient against fp64
@pytest.mark.parametrize('name', sorted(pc.CASES))
def test_loss_and_gradient_against_the_fp64_restatement(name):
    ref = pc.case(name)
    loss, _, cnt, grad = _call_photometric(ref['case'])
    _bounded('photometric ' + name, ref, loss, grad, ref['r32']['loss'])
    assert (ref['grad64'] == 0).any() and cnt.sum() < cnt.size


# ---- 3. closed forms
def _closed(c):
    """(1 - alpha) eps sum w with the fp32 alpha, eps and weights"""
    return (1.0 - float(np.float32(c['alpha']))) * float(np.float32(c['eps'])) * sum(float(np.float32(w)) for w in c['head_weights'])


def test_identical_views_at_zero_displacement_give_one_minus_alpha_times_eps():
    """SSIM of a window with itself is exactly 1 in fp32 (numerator and denominator are the same numbers), the intensity term is
    sqrt(eps^2); what is left are the roundings of eps * eps, the root, the product with 1 - alpha and the fp32 result: 4 x 2^-24."""
    c = pc.case('multi-tile-19x70')['case']
    loss, _, cnt, grad = _call_photometric(c, tgt_rgb=c['ref_rgb'], pred=np.zeros_like(c['pred']))
    want = _closed(c)
    print('identical views: loss %.9g, closed form %.9g, relative error %.3e' % (loss, want, abs(loss - want) / want))
    assert cnt.any() and abs(loss - want) <= 4 * 2.0 ** -24 * want
    assert np.isfinite(grad).all()


def _ramp_case(offset=0.0):
    """A target whose luminance is the ramp 0.2 + 0.02 y, the reference generated from the field D0 (|D0| <= 1) by ref(y) = tgt(y - 2 D0),
    both grey, and pred = D0 + offset on two heads.  The bilinear sample of a ramp is the ramp, so at pred = D0 the views agree to
    rounding."""
    B, n, H, W = 1, 2, 24, 40
    rng = np.random.RandomState(5)
    D0 = 2 * pc.smooth_noise(rng, (B,), H, W, cells=3) - 1
    ys = np.arange(H, dtype=np.float64)[None, :, None]
    tgt = np.broadcast_to(0.2 + 0.02 * ys, (B, H, W))
    ref = 0.2 + 0.02 * (ys - 2.0 * D0)
    grey = lambda y: pc.normalise(np.repeat(y[:, None], 3, 1))                                     # noqa: E731
    pred = np.repeat((D0 + offset)[:, None], n, 1).astype(np.float32)
    return dict(pred=pred, ref_rgb=grey(ref), tgt_rgb=grey(tgt), ab=None, mask=None, head_weights=(1.0, 0.5), target_type='disp',
                shift=(0.0, -2.0), alpha=0.85, eps=1e-3, gamma=10.0)


def test_a_ramp_warped_by_the_true_field_gives_the_closed_form_and_offsets_pull_back():
    """At pred = D0 the loss is (1 - alpha) eps sum w up to what fp32 costs: the bar is 2 x (the fp32 restatement's own distance from the
    closed form) + one ulp.  At pred = D0 +- 0.25 the warped ramp is off by -+0.01 everywhere, far from both ends of the clamp, and the
    gradient has the sign of the offset on every counted pixel."""
    c = _ramp_case()
    want = _closed(c)
    r32, r64 = pc.run(c), pc.run(c, np.float64)
    loss, _, cnt, _ = _call_photometric(c)
    own = abs(r32['loss'] - want)
    print('ramp at D0: loss %.9g, closed form %.9g, error %.3e (bar 2 x %.3e + ulp), fp64 restatement %.9g' % (loss, want, abs(loss - want), own,
                                                                                                            r64['loss']))
    assert cnt.sum() >= cnt.size // 4 and np.array_equal(cnt, r32['counted'])
    assert abs(r64['loss'] - want) <= 1e-3 * want                    # the scene does what it says
    assert abs(loss - want) <= 2.0 * own + support.ulp_of(want)
    for sign in (1.0, -1.0):
        c = _ramp_case(0.25 * sign)
        loss_o, _, cnt, grad = _call_photometric(c)
        r = pc.run(c, np.float64)
        assert not any(k.any() for k in r['clamped']) and cnt.any() and loss_o > 10 * want
        assert (grad[cnt > 0] * sign > 0).all()


def test_a_displacement_that_throws_every_sample_out_gives_zero_loss_and_zero_gradient():
    c = pc.case('diagonal-33x40')['case']
    loss, warped, cnt, grad = _call_photometric(c, pred=np.full_like(c['pred'], 1e4))
    assert loss == 0.0 and not cnt.any() and not warped.any() and not grad.any() and np.isfinite(grad).all()
    # one head with pixels, one without: the empty head adds 0, not NaN
    pred = c['pred'].copy()
    pred[:, 1] = -1e4
    loss2, _, cnt2, grad2 = _call_photometric(c, pred=pred)
    one = pc.run(dict(c, pred=pred[:, :1], head_weights=(1.0,)))
    assert cnt2[:, 0].any() and not cnt2[:, 1].any() and not grad2[:, 1].any() and grad2[:, 0].any()
    assert np.isfinite(loss2) and abs(loss2 - one['loss']) <= 2e-7 * one['loss']


# ---- 4. what must not reach a sum
def test_junk_under_the_mask_never_reaches_a_sum():
    c = pc.make_case(B=1, n=1, H=24, W=40, seed=44, masked=True)
    clean = _call_photometric(c)
    pred = c['pred'].copy()
    off = np.argwhere(~(c['mask'][0] > 0))
    assert len(off) >= 6
    for k, v in enumerate((np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0)):
        pred[0, 0, off[k][0], off[k][1]] = v
    junk = _call_photometric(c, pred=pred)
    assert junk[0] == clean[0] and np.array_equal(bits(junk[3]), bits(clean[3])) and np.array_equal(junk[2], clean[2])
    assert np.array_equal(bits(junk[1]), bits(clean[1]))
    s_clean, s_junk = _smooth(c), _smooth(c, pred=pred)
    assert s_junk[0] == s_clean[0] and np.array_equal(bits(s_junk[1]), bits(s_clean[1]))


def test_a_nan_prediction_removes_its_pixel_and_the_nine_windows_through_it():
    c = pc.make_case(B=1, n=1, H=24, W=40, seed=44, masked=True)
    before = pc.run(c)['counted'][0, 0]
    inner = [p for p in np.argwhere(before > 0) if before[p[0] - 1:p[0] + 2, p[1] - 1:p[1] + 2].all()]
    y, x = inner[5]
    pred = c['pred'].copy()
    pred[0, 0, y, x] = np.nan
    got = _call_photometric(c, pred=pred)
    mask = c['mask'].copy()
    mask[0, y, x] = 0.0
    want = _call_photometric(c, mask=mask)                                       # the same pixel taken out by the mask instead
    assert np.isfinite(got[0]) and np.isfinite(got[3]).all() and np.isfinite(got[1]).all()
    assert got[0] == want[0] and np.array_equal(got[2], want[2]) and np.array_equal(bits(got[1]), bits(want[1]))
    assert np.array_equal(bits(got[3]), bits(want[3])) and got[3][0, 0, y, x] == 0.0 and got[1][0, 0, y, x] == 0.0
    assert not got[2][0, 0, y - 1:y + 2, x - 1:x + 2].any() and got[2].sum() == before.sum() - 9


# ---- 5. the bits repeat
def _abi_args(c):
    ops = support.ops()
    held = [tensor(c['pred']), tensor(c['ref_rgb']), tensor(c['tgt_rgb']), tensor(c['ab']), tensor(c['mask'])]
    B, n, H, W = c['pred'].shape
    tail = (B, n, H, W, ops.TARGET_TYPES[c['target_type']], c['shift'][0], c['shift'][1], c['alpha'], c['eps'], ops._normalizer_floats(),
            ops._host_floats(c['head_weights']))
    return held, tuple(ops._ptr(t) for t in held) + tail


def test_two_calls_return_the_same_bits_whatever_the_scratch_held():
    from dualpixelface_amd._lib import lib
    ops = support.ops()
    ref = pc.case('multi-tile-19x70')
    c = ref['case']
    held, args = _abi_args(c)
    B, n, H, W = c['pred'].shape
    nbytes = lib().call('dpf_photometric_workspace_bytes', B, n, H, W)
    assert nbytes == n * B * 3 * 3 * 16
    outs = []
    for poison in (float('nan'), -3e30):
        ws = torch.full(((nbytes + 7) // 8,), poison, dtype=torch.float64, device=DEV)
        stats = torch.full((ops.PHOTOMETRIC_STATS,), poison, dtype=torch.float64, device=DEV)
        luma = torch.full((2, B, H, W), poison, dtype=torch.float32, device=DEV)
        out = torch.full((), poison, dtype=torch.float32, device=DEV)
        dpred = torch.full(c['pred'].shape, poison, dtype=torch.float32, device=DEV)
        gout = torch.ones((), dtype=torch.float32, device=DEV)
        lib().call('dpf_photometric_forward', *args, ops._ptr(ws), nbytes, ops._ptr(luma), ops._ptr(stats), ops._ptr(out), None, None,
                   ops._stream())
        ws.fill_(poison)                                             # the backward needs the planes and the stats, not the workspace
        lib().call('dpf_photometric_backward', *args, ops._ptr(luma), ops._ptr(stats), ops._ptr(gout), ops._ptr(dpred), ops._stream())
        outs.append((out.cpu().numpy(), stats.cpu().numpy(), dpred.cpu().numpy(), luma.cpu().numpy()))
    (o1, s1, d1, l1), (o2, s2, d2, l2) = outs
    assert np.isfinite(o1) and np.isfinite(d1).all() and np.isfinite(s1).all()
    assert bits(o1) == bits(o2) and np.array_equal(s1, s2) and np.array_equal(bits(d1), bits(d2)) and np.array_equal(bits(l1), bits(l2))
    assert np.array_equal(bits(l1[0]), bits(ref['r32']['Y_ref'])) and np.array_equal(bits(l1[1]), bits(ref['r32']['Y_tgt']))
    loss, _, _, grad = _call_photometric(c)                                      # and the operator, with whatever the allocator hands it
    assert np.float32(loss) == o1 and np.array_equal(bits(grad), bits(d1))
    assert s1[:3].tolist() == ref['r32']['count'] and not s1[3:8].any()


def test_another_operators_call_between_forward_and_backward_does_not_change_the_gradient():
    ops = support.ops()
    ref = pc.case('multi-tile-19x70')
    c = ref['case']
    _, _, _, plain = _call_photometric(c)
    _, s_plain = _smooth(c)
    p = tensor(c['pred']).requires_grad_(True)
    q = tensor(c['pred']).requires_grad_(True)
    fixed = [tensor(c[k]) for k in ('ref_rgb', 'tgt_rgb', 'mask')]
    loss = ops.photometric_loss(p, fixed[0], fixed[1], mask=fixed[2], head_weights=c['head_weights'], shift=c['shift'])
    sl = ops.smoothness_loss(q, fixed[0], mask=fixed[2], head_weights=c['head_weights'])
    # the same operators on other data, a filter that takes the shared scratch, and a sweep over whatever the allocator freed
    other = pc.case('horizontal')['case']
    _call_photometric(other)
    _smooth(other)
    ops.guided_filter(tensor(other['pred']), tensor(other['ref_rgb']), 2, 1e-2)
    for buf in ops._scratch.values():                                # (not the zero arenas: their slots are promised to be 0)
        buf.fill_(float('nan'))
    torch.full((1 << 20,), float('nan'), device=DEV)
    loss.backward()
    sl.backward()
    assert np.array_equal(bits(p.grad.cpu().numpy()), bits(plain)) and np.array_equal(bits(q.grad.cpu().numpy()), bits(s_plain))


def test_a_captured_call_replays_the_eager_bits():
    ops = support.ops()
    c = pc.case('multi-tile-19x70')['case']
    eager_loss, _, _, eager_grad = _call_photometric(c)
    s_loss, s_grad = _smooth(c)
    p = tensor(c['pred']).requires_grad_(True)
    fixed = [tensor(c[k]) for k in ('ref_rgb', 'tgt_rgb', 'mask')]

    def run():
        loss = ops.photometric_loss(p, fixed[0], fixed[1], mask=fixed[2], head_weights=c['head_weights'], shift=c['shift'])
        sl = ops.smoothness_loss(p, fixed[0], mask=fixed[2], head_weights=c['head_weights'])
        return loss, torch.autograd.grad(loss, p)[0], sl, torch.autograd.grad(sl, p)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for _ in range(2):
        for t in outs:
            t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert float(outs[0].detach().double()) == eager_loss and np.array_equal(bits(outs[1].cpu().numpy()), bits(eager_grad))
        assert float(outs[2].detach().double()) == s_loss and np.array_equal(bits(outs[3].cpu().numpy()), bits(s_grad))


def test_gout_scales_the_gradient_to_within_one_ulp():
    c = pc.case('diagonal-33x40')['case']
    _, _, _, g1 = _call_photometric(c)
    _, _, _, gs = _call_photometric(c, gout=0.37)
    want = g1.astype(np.float64) * 0.37
    assert (np.abs(gs.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32))).all()
    assert np.array_equal(gs == 0, g1 == 0) and gs.any()


# ---- 6. the C ABI's refusals
def test_abi_refusals_leave_the_outputs_untouched():
    from dualpixelface_amd._lib import lib, DpfError
    ops = support.ops()
    c = pc.case('tiny-7x9')['case']
    held, args = _abi_args(c)
    for name, per in (('dpf_photometric_workspace_bytes', 16), ('dpf_smoothness_workspace_bytes', 32)):
        q = lambda *a: lib().call(name, *a)                                                        # noqa: E731
        assert q(1, 1, 7, 9) == per and q(2, 3, 19, 70) == 2 * 3 * 9 * per and q(1, 1, 8, 32) == per and q(1, 1, 9, 33) == 4 * per
        assert q(0, 1, 7, 9) == -1 and q(1, 9, 7, 9) == -1 and q(1, 0, 7, 9) == -1 and q(1, 1, 0, 9) == -1 and q(8192, 8, 7, 9) == -1
        assert q(40000, 1, 7, 9) == -1                                                             # 2 B luminance planes on one grid axis
    ws = torch.zeros(2, dtype=torch.float64, device=DEV)
    stats = torch.full((ops.PHOTOMETRIC_STATS,), 7.0, dtype=torch.float64, device=DEV)
    luma = torch.full((2, 1, 7, 9), 7.0, dtype=torch.float32, device=DEV)
    out = torch.full((), 7.0, dtype=torch.float32, device=DEV)
    warped = torch.full((1, 1, 7, 9), 7.0, dtype=torch.float32, device=DEV)
    dpred = torch.full((1, 1, 7, 9), 7.0, dtype=torch.float32, device=DEV)
    tail = (ops._ptr(ws), 16, ops._ptr(luma), ops._ptr(stats), ops._ptr(out), None, None, ops._stream())

    def refused(a, t, code, entry='dpf_photometric_forward'):
        with pytest.raises(DpfError, match=code):
            lib().call(entry, *a, *t)

    a = list(args)
    inv = 'DPF_ERR_INVALID_ARG'
    refused(a[:6] + [9] + a[7:], tail, inv)                                                        # n = 9
    refused(a[:6] + [0] + a[7:], tail, inv)                                                        # n = 0
    refused(a[:9] + [3] + a[10:], tail, inv)                                                       # target type 3
    refused(a[:9] + [2] + a[10:], tail, inv)                                                       # a depth model without ab
    refused(a[:10] + [0.0, 0.0] + a[12:], tail, inv)                                               # both shift components 0
    refused(a[:10] + [float('nan'), 1.0] + a[12:], tail, inv)                                      # a shift that is not finite
    refused(a[:10] + [0.0, float('inf')] + a[12:], tail, inv)
    refused(a[:12] + [1.5] + a[13:], tail, inv)                                                    # alpha outside [0, 1]
    refused(a[:12] + [-0.1] + a[13:], tail, inv)
    refused(a[:13] + [0.0] + a[14:], tail, inv)                                                    # eps <= 0
    refused([None] + a[1:], tail, inv)                                                             # a NULL operand
    refused(a[:2] + [None] + a[3:], tail, inv)
    refused(a[:14] + [None] + a[15:], tail, inv)
    refused(a, (ops._ptr(ws), 8) + tail[2:], inv)                                                  # workspace too small
    refused(a, (support.offset_ptr(ws, 4), 16) + tail[2:], inv)                                         # workspace misaligned
    refused(a, tail[:2] + (None,) + tail[3:], inv)                                                 # no luminance planes
    refused(a, tail[:5] + (ops._ptr(warped), None) + tail[7:], inv)                                # one of the optional pair
    refused(a[:5] + [40000] + a[6:], tail, 'DPF_ERR_UNSUPPORTED')                                  # the grid's limit
    btail = (ops._ptr(luma), ops._ptr(stats), ops._ptr(out), ops._ptr(dpred), ops._stream())
    refused(a, btail[:2] + (None,) + btail[3:], inv, 'dpf_photometric_backward')                   # no gout
    refused(a[:12] + [2.0] + a[13:], btail, inv, 'dpf_photometric_backward')
    # smoothness
    sa = [ops._ptr(held[0]), ops._ptr(held[1]), None, 1, 1, 7, 9, 10.0, 1e-3, ops._normalizer_floats(), ops._host_floats((1.0,))]
    stats32 = torch.full((ops.SMOOTHNESS_STATS,), 7.0, dtype=torch.float64, device=DEV)
    ws4 = torch.zeros(4, dtype=torch.float64, device=DEV)
    stail = (ops._ptr(ws4), 32, ops._ptr(luma), ops._ptr(stats32), ops._ptr(out), ops._stream())
    refused(sa[:7] + [-1.0] + sa[8:], stail, inv, 'dpf_smoothness_forward')                        # gamma < 0
    refused(sa[:8] + [0.0] + sa[9:], stail, inv, 'dpf_smoothness_forward')                         # eps <= 0
    refused(sa[:4] + [9] + sa[5:], stail, inv, 'dpf_smoothness_forward')                           # n = 9
    refused(sa, (ops._ptr(ws4), 16) + stail[2:], inv, 'dpf_smoothness_forward')                    # workspace too small
    refused(sa[:7] + [-1.0] + sa[8:], btail, inv, 'dpf_smoothness_backward')
    torch.cuda.synchronize()
    for t in (out, luma, stats, stats32, warped, dpred):                                           # a refusal launches nothing
        assert (t == 7.0).all()
    with pytest.raises(DpfError, match='shift'):
        _call_photometric(c, shift=(0.0, 0.0))
    with pytest.raises(DpfError, match='alpha'):
        _call_photometric(c, alpha=1.5)
    with pytest.raises(DpfError, match='gamma'):
        _smooth(c, gamma=-1.0)


# ---- 7. smoothness
def test_smoothness_loss_and_gradient_against_the_fp64_restatement():
    ref = pc.smooth_case('multi-tile-19x70')
    loss, grad = _smooth(ref['case'])
    _bounded('smoothness multi-tile-19x70', ref, loss, grad, ref['r32']['loss'])
    assert (ref['grad64'] == 0).any()
    assert ref['r32']['count_x'][0] < 2 * 19 * 69 and ref['r32']['count_y'][0] < 2 * 18 * 70


def _flat_case(pred, luma_plane):
    """pred [B, n, H, W] under a grey guide of the given luminance [B, H, W]"""
    n = pred.shape[1]
    return dict(pred=pred.astype(np.float32), ref_rgb=pc.normalise(np.repeat(luma_plane[:, None], 3, 1)), mask=None,
                head_weights=tuple([1.0, 0.5, 0.25][:n]), gamma=10.0, eps=1e-3)


def test_smoothness_closed_forms():
    """Constant pred: every pair gives sqrt(eps^2) under weight exp(0) = 1, so 2 eps sum w (roundings: eps * eps, the root, the fp32 result:
    3 x 2^-24) and an all-zero gradient.  A ramp of slope s along x under a constant image: sqrt(s^2 + eps^2) + eps per head; the fp32
    differences of the ramp 0.37 x (x < 40) are off by up to an ulp of 14.8 = 9.5e-7, relative to s 2.6e-6, plus those roundings."""
    B, n, H, W = 2, 3, 19, 40
    flat = np.full((B, H, W), 0.5)
    c = _flat_case(np.full((B, n, H, W), 3.25), flat)
    loss, grad = _smooth(c)
    eps, wsum = float(np.float32(1e-3)), 1.75
    print('smoothness, constant pred: loss %.9g against %.9g' % (loss, 2 * eps * wsum))
    assert abs(loss - 2 * eps * wsum) <= 3 * 2.0 ** -24 * 2 * eps * wsum and not grad.any()
    s = 0.37
    ramp = np.broadcast_to(s * np.arange(W, dtype=np.float64), (B, n, H, W))
    loss, grad = _smooth(_flat_case(ramp, flat))
    want = (np.sqrt(s * s + eps * eps) + eps) * wsum
    print('smoothness, ramp: loss %.9g against %.9g, relative error %.3e' % (loss, want, abs(loss - want) / want))
    assert abs(loss - want) <= (2.6e-6 + 3 * 2.0 ** -24) * want
    assert np.isfinite(grad).all() and (grad[:, :, :, 0] < 0).all() and (grad[:, :, :, -1] > 0).all()


def test_a_luminance_step_weights_exactly_the_pairs_across_it():
    """A step of delta in the guide between columns 16 and 17 multiplies the x-pairs across it, one per row, by exp(-gamma delta) and no
    other: on the x-ramp the loss drops by w_sum (1 - exp(-gamma delta)) sqrt(s^2 + eps^2) / (W - 1).  The bar is 2e-6 of the loss for
    the fp32 luminance, exponential and ramp differences (as above)."""
    B, n, H, W = 1, 2, 19, 40
    s, delta, eps, wsum = 0.37, 0.1, float(np.float32(1e-3)), 1.5
    ramp = np.broadcast_to(s * np.arange(W, dtype=np.float64), (B, n, H, W))
    flat = np.full((B, H, W), 0.5)
    step = flat.copy()
    step[:, :, 17:] += delta
    base, _ = _smooth(_flat_case(ramp, flat))
    loss, grad = _smooth(_flat_case(ramp, step))
    drop = wsum * (1 - np.exp(-10.0 * delta)) * np.sqrt(s * s + eps * eps) / (W - 1)
    print('smoothness, luminance step: loss %.9g, base %.9g, drop %.6e against %.6e' % (loss, base, base - loss, drop))
    assert abs((base - loss) - drop) <= 2e-6 * base + 2e-6 * drop
    # the gradient of the ramp under a flat guide vanishes inside; with the step the two columns beside it keep the difference
    inner = np.ones(W, bool)
    inner[[0, 16, 17, W - 1]] = False
    assert (np.abs(grad[:, :, :, inner]) <= 1e-6 * np.abs(grad).max()).all() and (grad[:, :, :, 16] > 0).all() and (grad[:, :, :, 17] < 0).all()


# ---- 8. the whole step
def _batch():
    from dualpixelface_amd.recipe import synthetic_batch
    return {k: v.to(DEV) for k, v in synthetic_batch(2, 64, 96, seed=7, mask_mode='bern').items()}


def test_dpnet_trains_on_the_two_views_alone_graph_equals_eager(monkeypatch):
    ops = support.ops()
    full = _batch()
    batch = {'left': full['left'], 'right': full['right']}
    cfg = dict(loss_type=['photometric', 'smoothness'], lambdas=[1.0, 0.1])
    with ops.deterministic_mode():
        monkeypatch.setenv('DPF_STEP_GRAPH', '0')
        b = support.dpnet(**cfg)
        assert b.loss_model.label_free()
        eager = support.loss_steps(b, batch, 4, abvalue_only_if_given=True)
        monkeypatch.setenv('DPF_STEP_GRAPH', '1')
        a = support.dpnet(**cfg)
        graphed = support.loss_steps(a, batch, 4, abvalue_only_if_given=True)        # two warm-up steps, the capture, one replay
        assert a._graph_state.get('graph') is not None and not a._graph_state.get('failed')
    assert graphed == eager, (graphed, eager)
    assert torch.equal(a.flat_parameters(), b.flat_parameters())
    for step in eager:
        assert set(step) == {'photometric_loss', 'smoothness_loss', 'final_loss'} and all(np.isfinite(v) for v in step.values())
        assert step['photometric_loss'] > 0 and step['smoothness_loss'] > 0
        want = float(torch.tensor(step['photometric_loss'], dtype=torch.float32) * 1.0 + torch.tensor(step['smoothness_loss'], dtype=torch.float32) * 0.1)
        assert step['final_loss'] == want, (step, want)
    assert eager[0] != eager[1]                                      # the step moves the weights


def test_photometric_next_to_smoothl1_trains_and_changes_the_first_gradient(monkeypatch):
    ops = support.ops()
    batch = _batch()
    monkeypatch.setenv('DPF_STEP_GRAPH', '0')
    with ops.deterministic_mode():
        plain, both = support.dpnet(), support.dpnet(loss_type=['smoothL1', 'photometric'], lambdas=[1.0, 1.0])
        assert not both.loss_model.label_free()
        first_plain = support.loss_steps(plain, batch, 1, abvalue_only_if_given=True)
        ga = plain.flat_gradients(zero=False).clone()
        first = support.loss_steps(both, batch, 1, abvalue_only_if_given=True)
        gb = both.flat_gradients(zero=False).clone()
        more = support.loss_steps(both, batch, 2, abvalue_only_if_given=True)
    assert set(first[0]) == {'smoothL1_loss', 'photometric_loss', 'final_loss'} and first[0]['smoothL1_loss'] == first_plain[0]['smoothL1_loss']
    assert all(np.isfinite(v) for step in first + more for v in step.values()) and more[0] != first[0]
    assert torch.isfinite(gb).all() and not torch.equal(ga, gb) and float((ga - gb).abs().max()) > 0


def test_stereodpnet_with_a_normal_head_still_names_the_missing_abvalue(monkeypatch):
    from dualpixelface_amd import load_option
    from dualpixelface_amd.plugin import STEREODPNET
    from dualpixelface_amd.recipe import fill_by_recipe, synthetic_batch
    monkeypatch.setenv('DPF_STEP_GRAPH', '0')
    opt = load_option('train_faceDP', loss_type=['photometric', 'smoothness'], lambdas=[1.0, 0.1])
    assert opt.model.predict_normal
    model = STEREODPNET(opt)
    fill_by_recipe(model)
    model.to(DEV).train()
    full = synthetic_batch(1, 32, 48, seed=5, mask_mode='bern')
    with pytest.raises(NotImplementedError, match='abvalue'):
        model.train_step({k: full[k].to(DEV) for k in ('left', 'right')})
