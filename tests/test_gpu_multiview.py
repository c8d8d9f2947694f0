"""The multi-view photometric loss on the GPU (run with ``-m gpu``): csrc/multiview.hip through ops.multiview_loss against the
restatements of tests/multiview_cpu.py.

Exact: the rig, the sample coordinates, the warped luminance and the counted map equal the fp32 numpy restatement bit for bit.  Bounded:
the loss against the fp64 restatement within 2 x (the fp32 restatement's own deviation from fp64) + one fp32 ulp of the value (the kernel
hands back an fp32 scalar); d pred against the fp64 autograd gradient, element-wise, within 2 x (the largest deviation of the fp32
autograd gradient from it) + 1e-6 of the largest gradient magnitude.  The fp32 figures are computed here, on the same input, not fixed in
advance.  The fp64 restatement takes its discrete decisions (warpable, taps, counted) from the fp32 one, so no counted pixel is left out
of the comparison (tests/test_multiview_host.py checks that both restatements count the same pixels).
"""
import numpy as np
import pytest
import torch

from tests import multiview_cpu as mc
from tests import support
from tests.support import DEV, bits, tensor

pytestmark = pytest.mark.gpu

RIG_KEYS = ('K', 'P', 'Ks', 'Ps')


def _call(c, gout=None, backward=True, **over):
    """The operator on a case dict (fields replaced by `over`) -> dict(loss float, warped, counted, xy, Y_tgt, Y_src, grad) numpy."""
    c = dict(c, **over)
    p = tensor(c['pred']).requires_grad_(True)
    loss, warped, cnt, xy, yt, ys = support.ops().multiview_loss(
        p, tensor(c['tgt_rgb']), tensor(c['src_rgb']), *[tensor(c[k]) for k in RIG_KEYS], ab=tensor(c['ab']), mask=tensor(c['mask']),
        head_weights=c['head_weights'], target_type=c['target_type'], weight_ssim=c['weight_ssim'], alpha=c['alpha'], scale=c['scale'],
        min_depth=c['min_depth'], return_warped=True)
    assert loss.shape == () and loss.dtype == torch.float32 and warped.dtype == torch.float32 and cnt.dtype == torch.uint8
    grad = None
    if backward:
        (loss if gout is None else loss * gout).backward()
        grad = p.grad.cpu().numpy()
    return dict(loss=float(loss.detach().double()), warped=warped.cpu().numpy(), counted=cnt.cpu().numpy(), xy=xy.cpu().numpy(),
                Y_tgt=yt.cpu().numpy(), Y_src=ys.cpu().numpy(), grad=grad)


def _bounded(tag, ref, got):
    loss, grad = got['loss'], got['grad']
    own_loss = abs(ref['r32']['loss'] - ref['loss64'])
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
@pytest.mark.parametrize('name', sorted(mc.CASES))
def test_rig_sample_points_warped_values_and_counted_map_equal_the_fp32_restatement(name):
    ref = mc.case(name)
    c, r32 = ref['case'], ref['r32']
    rig = support.ops().multiview_rig(*[tensor(c[k]) for k in RIG_KEYS]).cpu().numpy()
    assert np.array_equal(bits(rig), bits(r32['rig'])), float(np.abs(rig - r32['rig']).max())
    got = _call(c, backward=False)
    assert np.array_equal(bits(got['Y_tgt']), bits(r32['Y_tgt'])) and np.array_equal(bits(got['Y_src']), bits(r32['Y_src']))
    assert np.array_equal(got['counted'], r32['counted'])
    assert np.array_equal(bits(got['xy']), bits(r32['xy'])), float(np.abs(got['xy'] - r32['xy']).max())
    assert np.array_equal(bits(got['warped']), bits(r32['warped'])), float(np.abs(got['warped'] - r32['warped']).max())
    print('forward %s: counted per view %s of %d, loss %.9g (fp32 restatement %.9g)'
          % (name, got['counted'].sum(axis=(0, 1, 3, 4)).tolist(), got['counted'][:, :, 0].size, got['loss'], r32['loss']))


# ---- 2. loss and gradient against fp64
@pytest.mark.parametrize('name', sorted(mc.CASES))
def test_loss_and_gradient_against_the_fp64_restatement(name):
    ref = mc.case(name)
    got = _call(ref['case'])
    _bounded('multiview ' + name, ref, got)
    assert got['counted'].sum() < got['counted'].size              # (the border never counts; a masked case has exact zeros inside too)


# ---- 3. closed forms
def test_identity_pose_with_equal_intrinsics_gives_the_image_itself_for_any_depth():
    """M = K K^-1 and t = 0, so q = z [x, y, 1] and (u, v) = (z x / z, z y / z): the pixel itself up to one rounding of the product and
    one of the quotient, |u - x| <= 2^-23 x.  J is then I up to slope x that, far below the scale of the robust term: at alpha = 1,
    rho = sqrt(s + 1) - 1 with s <= (2^-23 W / scale)^2 ~ 1e-9 rounds to exactly 0.  What is left of the loss is 1 - SSIM of two windows
    that agree to rounding: numerator and denominator are a dozen fp32 operations each over the same numbers, |1 - SSIM| <= 16 x 2^-24,
    so the loss is at most weight_ssim x 8 x 2^-24 x sum w.  The gradient is exactly 0 in exact arithmetic (m_x q_z - q_x m_z = 0 without
    a translation); computed, it is rounding residue of terms that cancel, held here to 2^-20 of the largest gradient the same scene
    has once the neighbour is moved by half a unit."""
    c = mc.identity_case()
    r32 = mc.forward(c)
    got = _call(c)
    assert np.array_equal(bits(got['warped']), bits(r32['warped'])) and np.array_equal(got['counted'], r32['counted'])
    inner = got['counted'][0, 0, 0] > 0
    assert inner.sum() >= inner.size // 2
    xs = np.arange(c['pred'].shape[3], dtype=np.float64)[None, :]
    ys = np.arange(c['pred'].shape[2], dtype=np.float64)[:, None]
    for h in range(c['pred'].shape[1]):
        ok = got['xy'][0, h, 0, 0] != 0
        assert (np.abs(got['xy'][0, h, 0, 0] - xs)[ok] <= 2.0 ** -23 * xs.max()).all()
        assert (np.abs(got['xy'][0, h, 0, 1] - ys)[got['xy'][0, h, 0, 1] != 0] <= 2.0 ** -23 * ys.max()).all()
        assert np.abs(got['warped'][0, h, 0] - got['Y_tgt'][0])[inner].max() <= 1e-5
    bound = float(np.float32(c['weight_ssim'])) * 8 * 2.0 ** -24 * sum(c['head_weights'])
    Ps = c['Ps'].copy()
    Ps[:, 0, 0, 3] = 0.5
    moved = _call(c, Ps=Ps)
    print('identity pose: loss %.3e (bound %.3e), max |d pred| %.3e against %.3e with the neighbour moved (loss %.3e)'
          % (got['loss'], bound, np.abs(got['grad']).max(), np.abs(moved['grad']).max(), moved['loss']))
    assert 0.0 <= got['loss'] <= bound and moved['loss'] > 1e3 * max(got['loss'], 1e-12)
    assert np.abs(got['grad']).max() <= 2.0 ** -20 * np.abs(moved['grad']).max()


def test_the_plane_scene_at_its_true_depth_gives_the_floor_and_offsets_raise_the_loss_and_are_pulled_back():
    """At the true depth the loss is what the bilinear interpolation of the neighbours' rasters leaves (tests/test_multiview_host.py
    bounds it); the bar against the fp64 restatement is the usual 2 x own + ulp.  A depth 5 % too large or too small raises the loss
    more than tenfold, and the gradient points back: along the offset the loss falls (sum of d pred x sign of the offset > 0 over the
    counted pixels), and at least 9 in 10 counted pixels agree one by one."""
    floor = None
    for offset in (0.0, 0.05, -0.05):
        c = mc.plane_case(H=24, W=40, views=2, seed=3, offset=offset, n=2)
        r32, r64 = mc.forward(c), mc.forward(c, np.float64)
        got = _call(c)
        own = abs(r32['loss'] - r64['loss'])
        print('plane, offset %+.2f: loss %.6e (fp64 %.6e, bar 2 x %.3e + ulp)' % (offset, got['loss'], r64['loss'], own))
        assert np.array_equal(got['counted'], r32['counted']) and got['counted'].sum() >= got['counted'].size // 2
        assert abs(got['loss'] - r64['loss']) <= 2.0 * own + support.ulp_of(r64['loss'])
        if offset == 0.0:
            floor = got['loss']
            continue
        assert got['loss'] > 10 * floor
        seen = got['counted'].max(axis=2) > 0                        # [B, n, H, W]: counted in some view
        g = got['grad'][seen] * np.sign(offset)                       # pred is the depth here: too large -> d loss / d pred > 0
        assert g.sum() > 0 and (g > 0).mean() >= 0.9, (g.sum(), (g > 0).mean())


def test_a_view_that_counts_nothing_adds_zero_and_the_mean_is_over_the_other_views():
    ref = mc.case('one-view-behind')
    c = ref['case']
    both = _call(c)
    assert both['counted'][:, :, 0].any() and not both['counted'][:, :, 1].any() and not both['warped'][:, :, 1].any()
    alone = _call(c, src_rgb=c['src_rgb'][:, :1], Ks=c['Ks'][:, :1], Ps=c['Ps'][:, :1])
    assert both['loss'] == alone['loss'] and np.array_equal(bits(both['grad']), bits(alone['grad'])) and both['grad'].any()
    # no view counts: zero loss, zero gradient, nothing is NaN
    none = _call(c, src_rgb=c['src_rgb'][:, 1:], Ks=c['Ks'][:, 1:], Ps=c['Ps'][:, 1:])
    assert none['loss'] == 0.0 and not none['counted'].any() and not none['grad'].any() and np.isfinite(none['grad']).all()
    # a depth below min_depth or a depth that sends every sample out of the frame does the same
    far = _call(c, pred=np.full_like(c['pred'], 1e-6))
    assert far['loss'] == 0.0 and not far['counted'].any() and not far['grad'].any()


# ---- 4. what must not reach a sum
def test_junk_under_the_mask_never_reaches_a_sum():
    c = mc.make_case(B=1, n=1, S=2, H=24, W=40, Hs=30, Ws=50, seed=44, target_type='depth', masked=True)
    clean = _call(c)
    pred = c['pred'].copy()
    off = np.argwhere(~(c['mask'][0] > 0))
    assert len(off) >= 6
    for k, v in enumerate((np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0)):
        pred[0, 0, off[k][0], off[k][1]] = v
    junk = _call(c, pred=pred)
    assert junk['loss'] == clean['loss'] and np.array_equal(bits(junk['grad']), bits(clean['grad']))
    assert np.array_equal(junk['counted'], clean['counted']) and np.array_equal(bits(junk['warped']), bits(clean['warped']))
    # and a NaN under the mask's support takes its pixel and the nine windows through it out, like the mask would
    inner = [p for p in np.argwhere(clean['counted'][0, 0, 0] > 0) if clean['counted'][0, 0, 0, p[0] - 1:p[0] + 2, p[1] - 1:p[1] + 2].all()]
    y, x = inner[5]
    pred = c['pred'].copy()
    pred[0, 0, y, x] = np.nan
    got = _call(c, pred=pred)
    mask = c['mask'].copy()
    mask[0, y, x] = 0.0
    want = _call(c, mask=mask)
    assert np.isfinite(got['loss']) and np.isfinite(got['grad']).all() and got['loss'] == want['loss']
    assert np.array_equal(got['counted'], want['counted']) and np.array_equal(bits(got['grad']), bits(want['grad']))
    assert got['grad'][0, 0, y, x] == 0.0 and not got['counted'][0, 0, :, y - 1:y + 2, x - 1:x + 2].any()


# ---- 5. the bits repeat
def _abi_args(c):
    ops = support.ops()
    B, n, H, W = c['pred'].shape
    S, Hs, Ws = c['src_rgb'].shape[1], c['src_rgb'].shape[3], c['src_rgb'].shape[4]
    rig = ops.multiview_rig(*[tensor(c[k]) for k in RIG_KEYS])
    held = [tensor(c['pred']), tensor(c['tgt_rgb']), tensor(c['src_rgb']), rig, tensor(c['ab']), tensor(c['mask'])]
    args = (ops._ptr(held[0]), ops._ptr(held[1]), ops._ptr(held[2]), S * 3 * Hs * Ws, ops._ptr(rig), ops._ptr(held[4]), ops._ptr(held[5]), B, n,
            S, H, W, Hs, Ws, ops.TARGET_TYPES[c['target_type']], c['weight_ssim'], c['alpha'], c['scale'], c['min_depth'], ops._normalizer_floats(),
            ops._host_floats(c['head_weights']))
    return held, args, (B, n, S, H, W, Hs, Ws)


def test_two_calls_return_the_same_bits_whatever_the_scratch_held():
    from dualpixelface_amd._lib import lib
    ops = support.ops()
    ref = mc.case('multi-tile-19x70')
    c = ref['case']
    held, args, (B, n, S, H, W, Hs, Ws) = _abi_args(c)
    nbytes = lib().call('dpf_multiview_workspace_bytes', B, n, S, H, W)
    assert nbytes == n * S * B * 3 * 3 * 16
    outs = []
    for poison in (float('nan'), -3e30):
        ws = torch.full(((nbytes + 7) // 8,), poison, dtype=torch.float64, device=DEV)
        stats = torch.full((ops.MULTIVIEW_STATS,), poison, dtype=torch.float64, device=DEV)
        luma = torch.full((B * H * W + B * S * Hs * Ws,), poison, dtype=torch.float32, device=DEV)
        out = torch.full((), poison, dtype=torch.float32, device=DEV)
        dpred = torch.full(c['pred'].shape, poison, dtype=torch.float32, device=DEV)
        gout = torch.ones((), dtype=torch.float32, device=DEV)
        lib().call('dpf_multiview_forward', *args, ops._ptr(ws), nbytes, ops._ptr(luma), ops._ptr(stats), ops._ptr(out), None, None, None,
                   ops._stream())
        ws.fill_(poison)                                             # the backward needs the planes, the rig and the stats, not the workspace
        lib().call('dpf_multiview_backward', *args, ops._ptr(luma), ops._ptr(stats), ops._ptr(gout), ops._ptr(dpred), ops._stream())
        outs.append((out.cpu().numpy(), stats.cpu().numpy(), dpred.cpu().numpy(), luma.cpu().numpy()))
    (o1, s1, d1, l1), (o2, s2, d2, l2) = outs
    assert np.isfinite(o1) and np.isfinite(d1).all() and np.isfinite(s1).all()
    assert bits(o1) == bits(o2) and np.array_equal(s1, s2) and np.array_equal(bits(d1), bits(d2)) and np.array_equal(bits(l1), bits(l2))
    got = _call(c)                                                   # and the operator, with whatever the allocator hands it
    assert np.float32(got['loss']) == o1 and np.array_equal(bits(got['grad']), bits(d1))
    r32 = ref['r32']
    for h in range(n):
        assert s1[8 * h:8 * h + S].tolist() == r32['count'][h] and not s1[8 * h + S:8 * h + 8].any() and s1[128 + h] == r32['views'][h]
    assert not s1[8 * n:64].any() and not s1[128 + n:].any()


def test_a_captured_call_replays_the_eager_bits():
    ops = support.ops()
    c = mc.case('multi-tile-19x70')['case']
    eager = _call(c)
    p = tensor(c['pred']).requires_grad_(True)
    fixed = [tensor(c[k]) for k in ('tgt_rgb', 'src_rgb') + RIG_KEYS + ('ab', 'mask')]

    def run():
        loss = ops.multiview_loss(p, *fixed[:6], ab=fixed[6], mask=fixed[7], head_weights=c['head_weights'], target_type=c['target_type'],
                                  weight_ssim=c['weight_ssim'], alpha=c['alpha'], scale=c['scale'], min_depth=c['min_depth'])
        return loss, torch.autograd.grad(loss, p)[0]

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
        assert float(outs[0].detach().double()) == eager['loss'] and np.array_equal(bits(outs[1].cpu().numpy()), bits(eager['grad']))


def test_gout_scales_the_gradient_to_within_one_ulp():
    c = mc.case('depth-33x40')['case']
    g1, gs = _call(c)['grad'], _call(c, gout=0.37)['grad']
    want = g1.astype(np.float64) * 0.37
    assert (np.abs(gs.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32))).all()
    assert np.array_equal(gs == 0, g1 == 0) and gs.any()


def test_a_slice_of_a_wider_centers_tensor_is_taken_through_its_batch_stride():
    """losses.MULTIVIEWLoss hands the first select_view views of batch['centers'] on as a slice along dim 1."""
    c = mc.case('multi-tile-19x70')['case']
    B, S, _, Hs, Ws = c['src_rgb'].shape
    wide = np.concatenate([c['src_rgb'].reshape(B, 3 * S, Hs, Ws), np.full((B, 3, Hs, Ws), np.nan, np.float32)], 1)
    p = tensor(c['pred']).requires_grad_(True)
    src = tensor(wide)[:, :3 * S].view(B, S, 3, Hs, Ws)
    assert not src.is_contiguous()
    loss = support.ops().multiview_loss(p, tensor(c['tgt_rgb']), src, *[tensor(c[k]) for k in RIG_KEYS], ab=tensor(c['ab']), mask=tensor(c['mask']),
                                        head_weights=c['head_weights'], target_type=c['target_type'], weight_ssim=c['weight_ssim'],
                                        alpha=c['alpha'], scale=c['scale'], min_depth=c['min_depth'])
    loss.backward()
    plain = _call(c)
    assert float(loss.detach().double()) == plain['loss'] and np.array_equal(bits(p.grad.cpu().numpy()), bits(plain['grad']))


# ---- 6. the C ABI's refusals
def test_abi_refusals_leave_the_outputs_untouched():
    from dualpixelface_amd._lib import lib, DpfError
    ops = support.ops()
    c = mc.case('tiny-7x9')['case']
    held, args, (B, n, S, H, W, Hs, Ws) = _abi_args(c)
    q = lambda *a: lib().call('dpf_multiview_workspace_bytes', *a)                                  # noqa: E731
    assert q(1, 1, 1, 7, 9) == 16 and q(2, 3, 2, 19, 70) == 2 * 3 * 2 * 9 * 16 and q(1, 1, 8, 9, 33) == 8 * 4 * 16
    assert q(0, 1, 1, 7, 9) == -1 and q(1, 9, 1, 7, 9) == -1 and q(1, 0, 1, 7, 9) == -1 and q(1, 1, 0, 7, 9) == -1 and q(1, 1, 9, 7, 9) == -1
    assert q(1, 1, 1, 0, 9) == -1 and q(1100, 8, 8, 7, 9) == -1 and q(8000, 1, 8, 7, 9) == -1       # B n S, and B (S + 1) planes
    ws = torch.zeros(2, dtype=torch.float64, device=DEV)
    stats = torch.full((ops.MULTIVIEW_STATS,), 7.0, dtype=torch.float64, device=DEV)
    luma = torch.full((B * H * W + B * S * Hs * Ws,), 7.0, dtype=torch.float32, device=DEV)
    out = torch.full((), 7.0, dtype=torch.float32, device=DEV)
    warped = torch.full((1, 1, 1, 7, 9), 7.0, dtype=torch.float32, device=DEV)
    xy = torch.full((1, 1, 1, 2, 7, 9), 7.0, dtype=torch.float32, device=DEV)
    dpred = torch.full((1, 1, 7, 9), 7.0, dtype=torch.float32, device=DEV)
    rig = torch.full((1, 1, 12), 7.0, dtype=torch.float32, device=DEV)
    tail = (ops._ptr(ws), 16, ops._ptr(luma), ops._ptr(stats), ops._ptr(out), None, None, None, ops._stream())

    def refused(a, t, code, entry='dpf_multiview_forward'):
        with pytest.raises(DpfError, match=code):
            lib().call(entry, *a, *t)

    a = list(args)
    inv = 'DPF_ERR_INVALID_ARG'
    # a: 0 pred, 1 tgt, 2 src, 3 stride, 4 rig, 5 ab, 6 mask, 7 B, 8 n, 9 S, 10 H, 11 W, 12 Hs, 13 Ws, 14 type, 15 weight_ssim, 16 alpha,
    # 17 scale, 18 min_depth, 19 norm, 20 weights
    refused(a[:8] + [9] + a[9:], tail, inv)                                                        # n = 9
    refused(a[:8] + [0] + a[9:], tail, inv)                                                        # n = 0
    refused(a[:9] + [9] + a[10:], tail, inv)                                                       # S = 9
    refused(a[:9] + [0] + a[10:], tail, inv)                                                       # S = 0
    refused(a[:12] + [0] + a[13:], tail, inv)                                                      # Hs = 0
    refused(a[:14] + [3] + a[15:], tail, inv)                                                      # target type 3
    refused(a[:14] + [0] + a[15:], tail, inv)                                                      # a disparity model without ab
    refused(a[:15] + [1.5] + a[16:], tail, inv)                                                    # weight_ssim outside [0, 1]
    refused(a[:15] + [-0.1] + a[16:], tail, inv)
    refused(a[:16] + [float('inf')] + a[17:], tail, inv)                                           # alpha not finite
    refused(a[:16] + [float('nan')] + a[17:], tail, inv)
    refused(a[:17] + [0.0] + a[18:], tail, inv)                                                    # scale <= 0
    refused(a[:18] + [0.0] + a[19:], tail, inv)                                                    # min_depth <= 0
    refused(a[:3] + [3 * Hs * Ws - 1] + a[4:], tail, inv)                                          # samples closer than a sample
    refused([None] + a[1:], tail, inv)                                                             # a NULL operand
    refused(a[:2] + [None] + a[3:], tail, inv)
    refused(a[:4] + [None] + a[5:], tail, inv)                                                     # no rig
    refused(a[:19] + [None] + a[20:], tail, inv)
    refused(a, (ops._ptr(ws), 8) + tail[2:], inv)                                                  # workspace too small
    refused(a, (support.offset_ptr(ws, 4), 16) + tail[2:], inv)                                    # workspace misaligned
    refused(a, tail[:2] + (None,) + tail[3:], inv)                                                 # no luminance planes
    refused(a, tail[:5] + (ops._ptr(warped), None, None) + tail[8:], inv)                          # one of the optional pair
    refused(a, tail[:5] + (None, None, ops._ptr(xy)) + tail[8:], inv)                              # sample points without the pair
    refused(a[:7] + [70000] + a[8:], tail, 'DPF_ERR_UNSUPPORTED')                                  # the grid's limit
    btail = (ops._ptr(luma), ops._ptr(stats), ops._ptr(out), ops._ptr(dpred), ops._stream())
    refused(a, btail[:2] + (None,) + btail[3:], inv, 'dpf_multiview_backward')                     # no gout
    refused(a[:15] + [2.0] + a[16:], btail, inv, 'dpf_multiview_backward')
    rig_args = [ops._ptr(tensor(c[k])) for k in RIG_KEYS]
    for bad in (rig_args[:1] + [None] + rig_args[2:] + [1, 1], rig_args + [0, 1], rig_args + [1, 9], rig_args + [1, 0]):
        refused(bad, (ops._ptr(rig), ops._stream()), inv, 'dpf_multiview_rig')
    torch.cuda.synchronize()
    for t in (out, luma, stats, warped, xy, dpred, rig):                                           # a refusal launches nothing
        assert (t == 7.0).all()
    with pytest.raises(DpfError, match='weight_ssim'):
        _call(c, weight_ssim=1.5)
    with pytest.raises(DpfError, match='alpha'):
        _call(c, alpha=float('inf'))
    with pytest.raises(DpfError, match='views'):
        support.ops().multiview_rig(tensor(c['K']), tensor(c['P']), tensor(np.zeros((1, 9, 3, 3), np.float32)), tensor(np.zeros((1, 9, 4, 4), np.float32)))


# ---- 7. the whole step
def _batch():
    from dualpixelface_amd.synthetic_multiview import synthetic_multiview_batch
    return synthetic_multiview_batch(2, 64, 96, views=3, seed=7, device=DEV)


def test_dpnet_trains_on_the_multi_view_batch_graph_equals_eager(monkeypatch):
    ops = support.ops()
    batch = {k: v for k, v in _batch().items() if k not in ('disp', 'depth', 'idepth', 'normal')}    # no label map in the batch
    with ops.deterministic_mode():
        monkeypatch.setenv('DPF_STEP_GRAPH', '0')
        cfg = dict(loss_type=['multiview', 'smoothness'], lambdas=[1.0, 0.1])
        assert support.dpnet('train_faceDP_dpnet_multiview').loss_model.loss_name == ['multiview']
        b = support.dpnet('train_faceDP_dpnet_multiview', **cfg)
        assert b.loss_model.label_free() and b.loss_model.loss_name == ['multiview', 'smoothness']
        eager = support.loss_steps(b, batch, 4, abvalue_only_if_given=True)
        monkeypatch.setenv('DPF_STEP_GRAPH', '1')
        a = support.dpnet('train_faceDP_dpnet_multiview', **cfg)
        graphed = support.loss_steps(a, batch, 4, abvalue_only_if_given=True)        # two warm-up steps, the capture, one replay
        assert a._graph_state.get('graph') is not None and not a._graph_state.get('failed')
    assert graphed == eager, (graphed, eager)
    assert torch.equal(a.flat_parameters(), b.flat_parameters())
    for step in eager:
        assert set(step) == {'multiview_loss', 'smoothness_loss', 'final_loss'} and all(np.isfinite(v) for v in step.values())
        assert step['multiview_loss'] >= 0 and step['smoothness_loss'] > 0
    assert eager[0] != eager[1]                                      # the step moves the weights


def test_multiview_next_to_smoothl1_trains_and_changes_the_first_gradient(monkeypatch):
    ops = support.ops()
    batch = _batch()
    monkeypatch.setenv('DPF_STEP_GRAPH', '0')
    with ops.deterministic_mode():
        plain, both = support.dpnet(), support.dpnet(loss_type=['smoothL1', 'multiview'], lambdas=[1.0, 1.0])
        assert not both.loss_model.label_free()
        first_plain = support.loss_steps(plain, batch, 1, abvalue_only_if_given=True)
        ga = plain.flat_gradients(zero=False).clone()
        first = support.loss_steps(both, batch, 1, abvalue_only_if_given=True)
        gb = both.flat_gradients(zero=False).clone()
        more = support.loss_steps(both, batch, 2, abvalue_only_if_given=True)
    assert set(first[0]) == {'smoothL1_loss', 'multiview_loss', 'final_loss'} and first[0]['smoothL1_loss'] == first_plain[0]['smoothL1_loss']
    assert all(np.isfinite(v) for step in first + more for v in step.values()) and more[0] != first[0]
    assert torch.isfinite(gb).all() and not torch.equal(ga, gb) and float((ga - gb).abs().max()) > 0
