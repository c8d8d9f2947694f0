"""The 'least_square' disparity conversion on the GPU (run with ``-m gpu``): csrc/affine_fit.hip through ops.affine_fit, the depth-target mode
of csrc/loss_bank.hip through ops.depth_loss(target_ab=...), the hooks and the whole DPNet step, against the reference's own vectors
(tests/golden/affine_fit.npz) and the fp64 restatement (tests/affine_fit_cpu.py).

Fit bars, in disparity units (af.dd): against the reference's ab 2 x the reference's own distance from the minimiser as stored in the fixture
(one reference-sized rounding for each side); against the restatement run with the same max_iters / tol, tol (only the order of the fp64 sums
and a one-step difference at the threshold separate the two).  Loss bars: 1e-5 relative and close_elem, as test_gpu_loss_bank.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import affine_fit_cpu as af
from tests import loss_bank_cpu as lb
from tests import support
from tests.support import DEV

pytestmark = pytest.mark.gpu

A0, B0 = -26996.49, 63.0


@pytest.fixture(scope='module')
def fixture(golden_dir):
    return af.Fixture(golden_dir)


def _fit(pred, idepth, **kw):
    ab, info = support.ops().affine_fit(pred.to(DEV), idepth.to(DEV), return_info=True, **kw)
    assert ab.dtype == torch.float32 and tuple(ab.shape) == (pred.shape[0], 2) and not ab.requires_grad
    assert info.dtype == torch.float64 and tuple(info.shape) == (pred.shape[0], 6)
    return ab.cpu(), info.cpu()


def _info_ab(info):
    return info[:, [1, 0]].numpy()                     # [b, a] from the record's (A, B)


def _against_restatement(pred, idepth, info, tag, max_iters=af.MAX_ITERS, tol=af.TOL, bar=None):
    ref_ab, ref = af.affine_fit(pred, idepth, max_iters=max_iters, tol=tol)
    d = af.dd(_info_ab(info), ref_ab, idepth.numpy())
    its = [int(v) for v in info[:, 2]]
    print('%s: dd to the restatement %.3e (bar %.1e), iterations %s against %s' % (tag, d, tol if bar is None else bar, its,
                                                                                    [r['iters'] for r in ref]))
    assert d <= (tol if bar is None else bar)
    for i, r in enumerate(ref):
        assert abs(its[i] - r['iters']) <= 1 and int(info[i, 3]) == r['count']
        f64 = lambda v: torch.tensor(v, dtype=torch.float64)
        support.close(info[i, 4], f64(r['objective']), 1e-9, '%s objective[%d]' % (tag, i))
        support.close(info[i, 5], f64(r['objective0']), 1e-9, '%s objective0[%d]' % (tag, i))
    return ref_ab, ref


def _fit_fields(B, n, H, W, seed, sigma=0.05, frac=0.1, zeros=0.15):
    g = torch.Generator().manual_seed(seed)
    depth = (torch.rand(B, H, W, generator=g) * 800.0 + 700.0) * (torch.rand(B, H, W, generator=g) >= zeros).float()
    idepth = torch.where(depth > 0, 1.0 / torch.where(depth > 0, depth, torch.ones_like(depth)), torch.zeros_like(depth))
    pred = A0 * idepth.unsqueeze(1) + B0 + sigma * torch.randn(B, n, H, W, generator=g)
    pred = pred + (torch.rand(B, n, H, W, generator=g) < frac).float() * (torch.rand(B, n, H, W, generator=g) * 30.0 - 15.0)
    return pred, idepth, depth


# ---- 1. the fit
def test_fit_against_reference_fixture(fixture):
    for fit in fixture.fits:
        pred, idepth, ref_ab = fixture.fields(fit)
        ab, info = _fit(pred, idepth)
        d = af.dd(ab.numpy(), ref_ab.numpy(), idepth.numpy())
        print('%s: dd to the reference %.3e (bar %.3e)' % (fit, d, 2 * fixture.ref_dd))
        assert d <= 2 * fixture.ref_dd
        _against_restatement(pred, idepth, info, fit)
        assert torch.equal(ab, torch.from_numpy(_info_ab(info)).float())          # ab is the record's (B, A) rounded to float32


@pytest.mark.parametrize('shape', [(3, 5, 67, 129), (2, 8, 68, 128), (2, 1, 68, 128)], ids=lambda s: 'x'.join(str(v) for v in s))
def test_fit_shapes(shape):
    """Odd sizes with several workgroups per sample and a head stride (one pixel per load); sizes the 16-byte loads take, with and without
    further heads behind head 0."""
    pred, idepth, _ = _fit_fields(*shape, seed=11)
    _, info = _fit(pred, idepth)
    _against_restatement(pred, idepth, info, str(shape))


def test_fit_two_pixels_exact_line():
    idepth = torch.tensor([[[1e-3, 1.25e-3]]])
    pred = torch.tensor([[[[36.0, 29.25]]]])
    ab, info = _fit(pred, idepth)
    _, ref = _against_restatement(pred, idepth, info, 'two pixels')
    x = idepth.double().view(-1)
    A = (29.25 - 36.0) / float(x[1] - x[0])
    assert abs(float(info[0, 0]) - A) <= 1e-9 * abs(A) and abs(float(info[0, 1]) - (36.0 - A * float(x[0]))) <= 1e-9
    assert float(info[0, 4]) <= 1e-20 and int(info[0, 3]) == 2


def test_fit_mixed_batch_stops_per_sample():
    """A clean sample, a heavy-outlier sample and one without a valid pixel: each stops at its own count, the empty one gives (0, 0) and
    leaves its neighbours as they are on their own."""
    clean, idc, _ = _fit_fields(1, 2, 40, 56, seed=12, sigma=0.05, frac=0.0)
    heavy, idh, _ = _fit_fields(1, 2, 40, 56, seed=13, sigma=0.3, frac=0.2)
    pred = torch.cat([clean, torch.full_like(clean, 7.0), heavy])
    idepth = torch.cat([idc, torch.zeros_like(idc), idh])
    ab, info = _fit(pred, idepth)
    _, ref = _against_restatement(pred, idepth, info, 'mixed')
    its = [int(v) for v in info[:, 2]]
    assert its[1] == 0 and 0 < its[0] < its[2] < af.MAX_ITERS, its
    assert ab[1].tolist() == [0.0, 0.0] and info[1].tolist() == [0.0] * 6
    ab0, info0 = _fit(clean, idc)
    ab2, info2 = _fit(heavy, idh)
    assert torch.equal(ab[0], ab0[0]) and torch.equal(info[0], info0[0]) and torch.equal(ab[2], ab2[0]) and torch.equal(info[2], info2[0])


def test_fit_iteration_cap():
    pred, idepth, _ = _fit_fields(2, 1, 40, 56, seed=14, sigma=0.3, frac=0.2)
    _, info = _fit(pred, idepth, max_iters=2)
    assert [int(v) for v in info[:, 2]] == [2, 2]
    # (no threshold is involved in two forced steps, so only the order of the fp64 sums separates the two: 1e-9 disparity units is ample)
    _against_restatement(pred, idepth, info, 'two steps', max_iters=2, bar=1e-9)
    _, info0 = _fit(pred, idepth, max_iters=0)                      # the least-squares start itself
    _against_restatement(pred, idepth, info0, 'start', max_iters=0, bar=1e-9)
    assert torch.equal(info0[:, 4], info0[:, 5]) and torch.equal(info0[:, 5], info[:, 5])


def test_fit_fold_of_more_rows_than_threads():
    """1024 x 1028: 257 partial rows in the sample's fold, so its first thread adds two of them (every other shape here folds <= 3).
    Two forced steps, as above: only the order of the fp64 sums separates the two sides."""
    pred, idepth, _ = _fit_fields(1, 1, 1024, 1028, seed=17)
    _, info = _fit(pred, idepth, max_iters=2)
    assert [int(v) for v in info[:, 2]] == [2]
    _against_restatement(pred, idepth, info, '1024x1028', max_iters=2, bar=1e-9)


def test_fit_ignores_what_lies_at_invalid_pixels():
    pred, idepth, _ = _fit_fields(2, 2, 40, 56, seed=15)
    ab, info = _fit(pred, idepth)
    bad = pred.clone()
    bad[:, 0][idepth == 0] = float('nan')
    assert int(torch.isnan(bad).sum()) > 100
    idn = idepth.clone()
    off = (idepth == 0).nonzero()
    idn[tuple(off[0].tolist())] = float('nan')                      # a NaN inverse depth is not valid either
    idn[tuple(off[1].tolist())] = -1.0
    ab2, info2 = _fit(bad, idn)
    assert bool(torch.isfinite(ab2).all()) and torch.equal(ab, ab2) and torch.equal(info, info2)


def test_fit_repeats_bit_for_bit():
    pred, idepth, _ = _fit_fields(3, 5, 67, 129, seed=16, sigma=0.3, frac=0.2)
    a, b = _fit(pred, idepth), _fit(pred, idepth)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_fit_abi_refuses_bad_arguments():
    from dualpixelface_amd._lib import lib, DpfError
    B, n, H, W = 2, 2, 8, 8
    pred = torch.ones(B, n, H, W, device=DEV)
    idepth = torch.ones(B, H, W, device=DEV)
    nbytes = lib().call('dpf_affine_fit_workspace_bytes', B, H, W)
    assert nbytes > 0 and lib().call('dpf_affine_fit_workspace_bytes', 0, H, W) == -1
    ws = torch.full((nbytes // 8 + 1,), -7.0, dtype=torch.float64, device=DEV)
    ab = torch.full((B, 2), -7.0, device=DEV)
    info = torch.full((B, 6), -7.0, dtype=torch.float64, device=DEV)
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(pred=ptr(pred), stride=n * H * W, idepth=ptr(idepth), B=B, H=H, W=W, f=0.1, iters=4, tol=1e-7, ws=ptr(ws), nbytes=nbytes,
                ab=ptr(ab), info=ptr(info))
    bad = [dict(pred=None), dict(idepth=None), dict(ws=None), dict(ab=None), dict(info=None), dict(B=0), dict(H=0), dict(W=-1), dict(iters=-1),
           dict(nbytes=nbytes - 8), dict(ws=ctypes.c_void_p(ws.data_ptr() + 4)), dict(f=0.0), dict(tol=-1.0), dict(stride=H * W - 1)]
    for over in bad:
        a = dict(good, **over)
        with pytest.raises(DpfError, match='DPF_ERR_INVALID_ARG'):
            lib().call('dpf_affine_fit', a['pred'], a['stride'], a['idepth'], a['B'], a['H'], a['W'], a['f'], a['iters'], a['tol'], a['ws'],
                       a['nbytes'], a['ab'], a['info'], stream)
    torch.cuda.synchronize()
    assert bool((ws == -7.0).all()) and bool((ab == -7.0).all()) and bool((info == -7.0).all())


# ---- 2. the loss kernels with the target formed from depth
def _loss_cases(fixture):
    return [c for c in fixture.cases if not (c[1] == 'silog' and c[2] == 'depth')]


def test_loss_kernel_against_reference_fixture(fixture):
    """ops.depth_loss(..., target_ab=the reference's ab): the loss kernels alone against the reference's loss and gradient."""
    counted_zero = masked_zero = 0
    for case in _loss_cases(fixture):
        name, kind, tt, n, scene, level, masked, b1 = case
        pred, batch, ab = fixture.inputs(case, DEV)
        pred.requires_grad_()
        transform = 'reciprocal' if (kind == 'smoothL1' and tt == 'depth') else 'identity'
        loss = support.ops().depth_loss(pred, batch['depth'], batch.get('mask'), None, fixture.head_weights(n), kind, transform,
                                 fixture.variance_focus, target_ab=ab)
        grad, = torch.autograd.grad(loss, pred)
        ref_loss, ref_grad = fixture.expected(case)
        support.close(loss, ref_loss, 1e-5, name + ' loss')
        support.close_elem(grad, ref_grad, name + ' grad')
        zero = batch['depth'] == 0
        on = batch['mask'] > 0 if masked else torch.ones_like(zero)
        counted_zero += int((zero & on).sum())
        masked_zero += int((zero & ~on).sum())
        assert bool((grad.transpose(0, 1)[:, ~on] == 0).all())               # under the mask: exactly 0
        if kind == 'smoothL1' and tt != 'depth' and bool((zero & on).any()):
            # a counted depth 0: the target is -100, far outside the quadratic zone, so the gradient is the head's weight over the count
            w0 = fixture.head_weights(n)[0] / float(on.sum())
            assert bool(((grad[:, 0][zero & on] - w0).abs() <= 1e-6 * w0).all())
    assert counted_zero > 0 and masked_zero > 0


def test_loss_kernel_shapes_and_refusals():
    from dualpixelface_amd._lib import DpfError
    pred, idepth, depth = _fit_fields(3, 5, 67, 129, seed=17)
    mask = (torch.rand(3, 67, 129, generator=torch.Generator().manual_seed(18)) < 0.6).float()
    ab = torch.tensor([[63.0, -26996.49], [61.5, -25000.0], [64.0, -28000.0]])
    weights = [1.0, 0.9, 0.8, 0.7, 0.6]
    for kind in ('smoothL1', 'silog'):
        d = depth if kind == 'smoothL1' else torch.where(depth > 0, depth, torch.full_like(depth, 900.0))     # silog: every target positive
        p = (pred if kind == 'smoothL1' else pred.clamp(min=5.0)).to(DEV).requires_grad_()
        loss = support.ops().depth_loss(p, d.to(DEV), mask.to(DEV), None, weights, kind, 'identity', 0.85, target_ab=ab.to(DEV))
        grad, = torch.autograd.grad(loss, p)
        ref_loss, ref_grad = lb.depth_loss(p, af.depth2disp(d, ab), mask, None, weights, kind, 'identity', 0.85)
        assert torch.isfinite(ref_loss)
        support.close(loss, ref_loss, 1e-5, kind + ' loss')
        support.close_elem(grad, ref_grad, kind + ' grad')
    with pytest.raises(DpfError, match='target_ab'):
        support.ops().depth_loss(pred.to(DEV), depth.to(DEV), None, None, weights, 'smoothL1', 'identity', 0.0, target_ab=ab[:2].to(DEV))


# ---- 3. the hooks end to end
def _selector(kind, loss_weight, variance_focus, config='train_faceDP_dpnet'):
    from dualpixelface_amd import load_option
    from dualpixelface_amd.losses import loss_selector
    return loss_selector(load_option(config, loss_type=[kind], lambdas=[1.0], loss_weight=loss_weight, variance_focus=variance_focus))


def _silog_shift_bound(kind, tt, pred, batch, weights, vf, ab, dd_):
    """How far a move of the fit by dd_ disparity units can move the loss.  smooth-L1 is 1-Lipschitz in its target: (sum of the head weights)
    x dd_.  silog: a target g moves log g by at most dd_ / min g, so d_k = w_k (log p - log g) moves by e_k <= w_k dd_ / min g per pixel;
    with m1 = mean d, m2 = mean d^2 and v = m2 - vf m1^2, |dv| <= (2 |d|_max e + e^2) (1 + vf) and |d sqrt(v)| <= |dv| / sqrt(v - |dv|),
    taken from the restatement's own d and v at ab."""
    if kind == 'smoothL1':
        return sum(weights) * dd_
    if tt == 'depth':
        return 0.0                                                  # the target is batch['depth']: the fit does not enter the loss
    g = af.depth2disp(batch['depth'].cpu(), ab).double()
    sel = batch['mask'].cpu() > 0 if 'mask' in batch else torch.ones_like(g, dtype=torch.bool)
    total = 0.0
    for k, w in enumerate(weights):
        d = w * (torch.log(pred.detach().cpu().double()[:, k][sel]) - torch.log(g[sel]))
        v = float((d ** 2).mean() - vf * d.mean() ** 2)
        e = w * dd_ / float(g[sel].min())
        dv = (2.0 * float(d.abs().max()) * e + e * e) * (1.0 + vf)
        assert v > dv
        total += 10.0 * dv / (v - dv) ** 0.5
    return total


def test_hooks_against_restatement_and_fixture(fixture):
    for case in fixture.cases:
        name, kind, tt, n, scene, level, masked, b1 = case
        pred, batch, ref_ab = fixture.inputs(case, DEV)
        assert 'abvalue' not in batch and 'disp' not in batch
        pred.requires_grad_()
        weights = fixture.head_weights(n)
        res = _selector(kind, fixture.loss_weight, fixture.variance_focus).forward({'pred_depth': pred}, batch, tt)
        ab = res['abvalue']
        assert tuple(ab.shape) == (pred.shape[0], 2) and ab.dtype == torch.float32 and not ab.requires_grad
        assert torch.equal(ab, support.ops().affine_fit(pred, batch['idepth'])) and res['final_loss'].dim() == 0
        d = af.dd(ab.cpu().numpy(), ref_ab.cpu().numpy(), batch['idepth'].cpu().numpy())
        assert d <= 2 * fixture.ref_dd, (name, d)
        grad, = torch.autograd.grad(res['final_loss'], pred)
        own_loss, own_grad = af.branch_call(kind, tt, pred, batch, weights, fixture.variance_focus, ab)      # at the device's own ab
        support.close(res[kind + '_loss'], own_loss, 1e-5, name + ' loss at its own ab')
        support.close(res['final_loss'], own_loss, 1e-5, name + ' final_loss at its own ab')
        support.close_elem(grad, own_grad, name + ' grad at its own ab')
        ref_loss, _ = fixture.expected(case)
        bar = 1e-5 * abs(float(ref_loss)) + _silog_shift_bound(kind, tt, pred, batch, weights, fixture.variance_focus, ref_ab, 2 * fixture.ref_dd)
        err = abs(float(res['final_loss'].detach()) - float(ref_loss))
        print('%s: |loss - reference| %.3e (bar %.3e)' % (name, err, bar))
        assert err <= bar


def test_hook_silog_depth_returns_the_fit():
    """silog against 'depth' overwrites prediction and target (silog.py:35-37): the loss is the 'given' one, the abvalue the fit's."""
    pred, idepth, depth = _fit_fields(2, 3, 40, 56, seed=19, zeros=0.0)
    far = (torch.rand(2, 3, 40, 56, generator=torch.Generator().manual_seed(20)) * 800.0 + 700.0).to(DEV).requires_grad_()
    batch = {'idepth': idepth.to(DEV), 'depth': depth.to(DEV)}
    res = _selector('silog', [1.0, 0.7, 0.5], 0.85).forward({'pred_depth': far}, batch, 'depth')
    ref_loss, ref_grad = lb.depth_loss(far, depth, None, None, [1.0, 0.7, 0.5], 'silog', 'identity', 0.85)
    support.close(res['final_loss'], ref_loss, 1e-5, 'loss')
    support.close_elem(torch.autograd.grad(res['final_loss'], far)[0], ref_grad, 'grad')
    assert torch.equal(res['abvalue'], support.ops().affine_fit(far, batch['idepth']))


def test_three_losses_share_one_fit_bit_for_bit():
    """smoothL1 + normal_geo + photometric on a batch without 'abvalue': the selector fits once and hands the result to all three; each
    loss class called alone fits for itself.  Same kernels on the same inputs, so losses, abvalue and the gradient are equal bit for
    bit.  The fields are made so that every loss counts pixels under the fit: head 0 is exactly 2000 batch['idepth'] - 1.5, which sends
    the photometric displacement a / pred + b into [-0.2, 1.4] pixels."""
    from dualpixelface_amd import load_option, losses
    names, lambdas, B, n, H, W = ['smoothL1', 'normal_geo', 'photometric'], [1.0, 0.5, 0.25], 2, 3, 32, 48
    g = torch.Generator().manual_seed(41)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
    depth = (1000.0 + 120.0 * torch.sin(x / 7.0) * torch.cos(y / 5.0)).expand(B, H, W) + torch.rand(B, 1, 1, generator=g) * 200.0
    pred = depth.unsqueeze(1) * (1.0 + 0.002 * torch.randn(B, n, H, W, generator=g))
    normal = torch.randn(B, 3, H, W, generator=g)
    batch = {'depth': depth, 'idepth': (pred[:, 0] + 1.5) / 2000.0, 'normal': normal / normal.norm(dim=1, keepdim=True),
             'K': torch.tensor([[60.0, 0.0, W / 2.0], [0.0, 60.0, H / 2.0], [0.0, 0.0, 1.0]]).expand(B, 3, 3).contiguous(),
             'mask': (torch.rand(B, H, W, generator=g) > 0.1).float(), 'left': torch.rand(B, 3, H, W, generator=g),
             'right': torch.rand(B, 3, H, W, generator=g)}
    batch = {k: v.to(DEV).contiguous() for k, v in batch.items()}
    option = load_option('train_faceDP_dpnet', loss_type=names, lambdas=lambdas, loss_weight=[1.0, 0.7, 0.5])

    def run(forward):
        p = pred.to(DEV).requires_grad_()
        res = forward({'pred_depth': p}, batch, 'depth')
        return res, torch.autograd.grad(res['final_loss'], p)[0]

    def one_by_one(results, batch, target_type):
        res, total = {}, []
        for name, lam in zip(names, lambdas):
            out = losses._BANK[name](option).forward(results, batch, target_type)
            res[name + '_loss'] = out['loss']
            if 'abvalue' in out:
                res['abvalue'] = out['abvalue']
            total.append(lam * out['loss'])
        res['final_loss'] = sum(total)
        return res

    shared, gs = run(losses.loss_selector(option).forward)
    alone, ga = run(one_by_one)
    assert set(shared) == set(alone) == {'smoothL1_loss', 'normal_geo_loss', 'photometric_loss', 'abvalue', 'final_loss'}
    for k in sorted(shared):
        print(k, shared[k].detach().cpu().tolist())
        assert torch.equal(shared[k], alone[k]), k
        assert bool(torch.isfinite(shared[k]).all()) and bool((shared[k] != 0).any()), k
    assert torch.equal(shared['abvalue'], support.ops().affine_fit(pred.to(DEV), batch['idepth']))
    assert torch.equal(gs, ga) and bool(torch.isfinite(gs).all()) and bool((gs != 0).any())


# ---- 4. the whole step
def _batch(strip):
    from dualpixelface_amd.recipe import synthetic_batch
    batch = {k: v.to(DEV) for k, v in synthetic_batch(2, 64, 96, seed=7, mask_mode='bern').items()}
    for k in (('abvalue', 'disp') if strip else ()):
        del batch[k]
    return batch


def test_dpnet_trains_without_abvalue_graph_equals_eager(monkeypatch):
    """'abvalue' and 'disp' deleted from the batch under the default dataset config: the step fits (a, b) inside the captured graph."""
    from dualpixelface_amd import ops
    config, batch = 'train_faceDP_dpnet', _batch(True)
    with ops.deterministic_mode():
        monkeypatch.setenv('DPF_STEP_GRAPH', '1')
        a = support.dpnet(config)
        assert a.option.dataset.dp_conversion == 'given'
        before = a.flat_parameters().clone()
        ra = [a.train_step(batch, None, lr=1e-3) for _ in range(4)]                      # two warm-up steps, the capture, one replay
        la = [float(r['final_loss'].detach()) for r in ra]
        assert a._graph_state.get('graph') is not None and not a._graph_state.get('failed')
        monkeypatch.setenv('DPF_STEP_GRAPH', '0')
        b = support.dpnet(config)
        lb_, weights = [], b.loss_model.loss_func[0].head_weights(5)
        for _ in range(4):
            res = b.train_step(batch, None, lr=1e-3)
            assert res['pred_depth'].shape == (2, 5, 64, 96) and tuple(res['abvalue'].shape) == (2, 2)
            ref_loss, _ = af.branch_call('smoothL1', 'disp', res['pred_depth'], batch, weights, 0.0, res['abvalue'])
            support.close(res['final_loss'], ref_loss, 1e-5, 'step %d final_loss' % len(lb_))
            lb_.append(float(res['final_loss'].detach()))
    assert all(np.isfinite(la)) and la == lb_, (la, lb_)
    assert float((a.flat_parameters() - before).abs().max()) > 0
    assert torch.equal(a.flat_parameters(), b.flat_parameters())


def test_dpnet_evaluates_a_batch_without_abvalue():
    """The shared validation step on a batch without 'abvalue' and 'disp' attaches the fit and logs an absolute_dp row, on the host functions
    and on the device kernels alike.  (DPNet's own validation hooks are no-ops as in the reference, dpnet/mainmodel.py:236-245: its test_step
    is that shared step.  affine_dp compares against batch['disp'], which such a batch does not have, so absolute_dp is the metric configured.)"""
    from dualpixelface_amd import metrics, ops
    batch = _batch(True)
    model = support.dpnet('train_faceDP_dpnet', metric_type=['absolute_dp']).eval()
    bench = model.metric_model.metric_func[0]
    res = model.test_step(batch, 0)
    assert 'final_loss' not in res and tuple(res['abvalue'].shape) == (2, 2) and res['abvalue'].dtype == torch.float32
    assert torch.equal(res['abvalue'], ops.affine_fit(res['pred_depth'], batch['idepth']))
    assert bench.index == 1
    host_row = bench.get_value(0)
    want = metrics.depth_errors(batch['depth'], metrics.disp2depth(res['pred_depth'], res['abvalue'])[:, 0], batch['mask'], 1.01)
    assert np.array_equal(np.asarray(host_row), np.asarray([float(v) for v in want]), equal_nan=True)
    assert metrics.device_metrics_enabled()
    with model.metric_model.deferred():
        res2 = model.test_step(batch, 1)
    model.metric_model.flush()
    assert bench.index == 2 and torch.equal(res2['abvalue'], res['abvalue'])
    print('host row %s\ndevice row %s' % (host_row, bench.get_value(1)))
    # (fp32 means on the host against fp64 two-phase sums on the device: test_gpu_device_metrics.py holds the kernels to the host functions)
    assert np.allclose(np.asarray(bench.get_value(1)), np.asarray(host_row), rtol=1e-4, atol=0.0, equal_nan=True)
    res3 = model.test_step(_batch(False), 2)
    assert 'abvalue' not in res3 and bench.index == 3                  # a batch that brings its abvalue: as before


def test_stereodpnet_with_normals_names_the_missing_abvalue():
    from dualpixelface_amd import load_option
    from dualpixelface_amd.plugin import STEREODPNET
    from dualpixelface_amd.recipe import fill_by_recipe
    model = STEREODPNET(load_option())
    assert model.option.model.predict_normal
    fill_by_recipe(model)
    model = model.to(DEV).train()
    batch = _batch(True)
    with pytest.raises(NotImplementedError, match="batch\\['abvalue'\\]"):
        model.forward(batch)
