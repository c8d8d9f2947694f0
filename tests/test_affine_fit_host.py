"""The 'least_square' disparity conversion, host side (no GPU): the fp64 restatement of the fit that the GPU tests hold the kernels to
(tests/affine_fit_cpu.py) against vectors produced by the reference's regress_affine and loss classes
(tests/golden/make_golden_affine_fit.py); the hooks' branch selection and key contract on stubs."""
import numpy as np
import pytest
import torch

from tests import affine_fit_cpu as af
from tests import support


@pytest.fixture(scope='module')
def fixture(golden_dir):
    return af.Fixture(golden_dir)


def test_restatement_fit_against_reference_fixture(fixture):
    """dd <= 2 x the reference's own distance from the minimiser (one reference-sized rounding for each side)."""
    assert fixture.fits == ['p::outlier10', 'z::clean', 'z::heavy', 'z::outlier10'] and 0 < fixture.ref_dd < 1e-5
    for fit in fixture.fits:
        pred, idepth, ref_ab = fixture.fields(fit)
        ab, info = af.affine_fit(pred, idepth)
        d = af.dd(ab, ref_ab.numpy(), idepth.numpy())
        print('%s: dd %.3e (bar %.3e), iterations %s' % (fit, d, 2 * fixture.ref_dd, [r['iters'] for r in info]))
        assert d <= 2 * fixture.ref_dd
        assert all(0 < r['iters'] < af.MAX_ITERS for r in info)               # every fixture sample stops on tol, not on the cap
        assert [r['count'] for r in info] == [int((idepth[i] > 0).sum()) for i in range(idepth.shape[0])]


def _junk():
    g = torch.Generator().manual_seed(3)
    idepth = 1.0 / (torch.rand(1, 24, 40, generator=g) * 800.0 + 700.0)
    return torch.rand(1, 1, 24, 40, generator=g) * 16.0 - 4.0, idepth


def test_objective_never_rises(fixture):
    fields = [fixture.fields(fit)[:2] for fit in fixture.fits] + [_junk()]
    for pred, idepth in fields:
        _, info = af.affine_fit(pred, idepth, max_iters=64, tol=0.0)
        for r in info:
            tr = np.asarray(r['trace'])
            assert len(tr) == 65 and r['objective0'] == tr[0] and r['objective'] == tr[-1]
            assert bool((np.diff(tr) <= 1e-12 * tr[:-1]).all()), tr            # (1e-12 relative: the fp64 sums' own rounding once it has converged)


def test_degenerate_samples():
    x = np.float32([0.0, -1.0, np.nan, 0.0])
    r = af.fit_sample(x, np.float32([1, 2, 3, 4]))
    assert (r['A'], r['B'], r['iters'], r['count'], r['objective']) == (0.0, 0.0, 0, 0, 0.0)
    r = af.fit_sample(np.float32([0.0, 1e-3, 0.0]), np.float32([7, 30.5, np.nan]))        # one valid pixel: det = 0 -> the weighted mean
    assert r['A'] == 0.0 and r['B'] == 30.5 and r['count'] == 1
    r = af.fit_sample(np.float32([1e-3, 1.25e-3]), np.float32([36.0, 29.25]))             # two pixels: the exact line
    assert abs(r['A'] - (29.25 - 36.0) / (np.float32(1.25e-3) - np.float64(np.float32(1e-3)))) < 1e-6 and r['objective'] < 1e-20


def test_restatement_loss_against_reference_fixture(fixture):
    """The branch's loss and gradient at the reference's own ab: what separates the two is float32 against float64 arithmetic only."""
    assert len(fixture.cases) == 16 and sum(1 for c in fixture.cases if c[7] and not c[6]) == 8
    for case in fixture.cases:
        name, kind, tt, n = case[:4]
        pred, batch, ab = fixture.inputs(case)
        loss, grad = af.branch_call(kind, tt, pred, batch, fixture.head_weights(n), fixture.variance_focus, ab)
        ref_loss, ref_grad = fixture.expected(case)
        support.close(loss, ref_loss, 1e-6, name + ' loss')
        support.close_elem(grad, ref_grad, name + ' grad')


# ---- the hooks on stubs
def _stubs(monkeypatch):
    from dualpixelface_amd import ops
    calls, fit = [], torch.tensor([[5.0, 6.0]])

    def affine_fit(pred, idepth, *a, **k):
        calls.append(('fit', pred, idepth))
        return fit

    def depth_loss(pred, target, mask=None, conf=None, head_weights=(1.0,), kind='smoothL1', transform='identity', variance_focus=0.0,
                   target_ab=None):
        calls.append(('bank', kind, transform, target, target_ab))
        return torch.zeros(())

    def stereo_losses(pred_depth, pred_normal, disp, normal, mask, head_weights, lam_d, lam_n):
        calls.append(('stereo', pred_depth is not None, pred_normal is not None, disp, None))
        return torch.zeros(3)

    monkeypatch.setattr(ops, 'affine_fit', affine_fit)
    monkeypatch.setattr(ops, 'depth_loss', depth_loss)
    monkeypatch.setattr(ops, 'stereo_losses', stereo_losses)
    return calls, fit


def _batch(abvalue=True):
    z = torch.ones(1, 2, 2)
    batch = {'disp': z * 2, 'idepth': z * 3, 'depth': z * 4, 'mask': z, 'abvalue': torch.zeros(1, 2)}
    if not abvalue:
        del batch['abvalue'], batch['disp']
    return batch


@pytest.mark.parametrize('loss', ['silog', 'smoothL1'])
@pytest.mark.parametrize('target_type', ['disp', 'idepth', 'depth'])
def test_batch_without_abvalue_selects_the_fit_branch(loss, target_type, monkeypatch):
    """A batch without 'abvalue' used to be refused; it now fits (a, b) on head 0 and batch['idepth'] and compares against the depth map."""
    from dualpixelface_amd.losses import loss_selector
    calls, fit = _stubs(monkeypatch)
    sel = loss_selector(support.option('train_faceDP_dpnet', loss_type=[loss], variance_focus=0.6))
    batch, pred = _batch(False), torch.ones(1, 1, 2, 2)
    out = sel.forward({'pred_depth': pred}, batch, target_type)
    assert set(out) == {loss + '_loss', 'abvalue', 'final_loss'} and out['abvalue'] is fit
    assert calls[0][0] == 'fit' and calls[0][1] is pred and calls[0][2] is batch['idepth'] and len(calls) == 2
    _, kind, transform, target, target_ab = calls[1]
    assert kind == loss
    if loss == 'silog' and target_type == 'depth':                   # silog.py:35-37: only the returned abvalue changes
        assert target is batch['depth'] and target_ab is None and transform == 'identity'
    else:
        assert target is batch['depth'] and target_ab is fit
        assert transform == ('reciprocal' if (loss == 'smoothL1' and target_type == 'depth') else 'identity')


@pytest.mark.parametrize('loss', ['silog', 'smoothL1'])
def test_batch_with_abvalue_is_not_fitted(loss, monkeypatch):
    from dualpixelface_amd.losses import loss_selector
    calls, fit = _stubs(monkeypatch)
    batch = _batch()
    sel = loss_selector(support.option('train_faceDP_dpnet', loss_type=[loss], variance_focus=0.6))
    out = sel.forward({'pred_depth': torch.ones(1, 1, 2, 2)}, batch, 'disp')
    assert [c[0] for c in calls] in (['bank'], ['stereo']) and calls[0][4] is None and out['abvalue'] is batch['abvalue']


def test_fit_branch_names_the_keys_it_needs():
    from dualpixelface_amd.losses import loss_selector
    sel = loss_selector(support.option('train_faceDP_dpnet', loss_type=['smoothL1']))
    with pytest.raises(NotImplementedError, match="least_square.*batch\\['idepth'\\] and batch\\['depth'\\]"):
        sel.forward({'pred_depth': torch.ones(1, 1, 2, 2)}, {'disp': torch.ones(1, 2, 2)}, 'disp')


def test_fused_pass_is_for_batches_that_bring_abvalue(monkeypatch):
    from dualpixelface_amd import load_option
    from dualpixelface_amd.losses import loss_selector
    calls, fit = _stubs(monkeypatch)
    results = {'pred_depth': torch.ones(1, 1, 2, 2), 'pred_normal': torch.ones(1, 1, 3, 2, 2)}
    sel = loss_selector(load_option())
    assert sel.loss_name == ['smoothL1', 'cosine']
    batch = dict(_batch(), normal=torch.ones(1, 3, 2, 2))
    out = sel.forward(results, batch)
    assert [c[:3] for c in calls] == [('stereo', True, True)] and out['abvalue'] is batch['abvalue']
    del calls[:]
    batch = dict(_batch(False), normal=torch.ones(1, 3, 2, 2))
    out = sel.forward(results, batch)
    assert [c[0] for c in calls] == ['fit', 'bank', 'stereo'] and calls[2][1:3] == (False, True) and out['abvalue'] is fit
    assert set(out) == {'smoothL1_loss', 'abvalue', 'cosine_loss', 'final_loss'}


THREE = ['smoothL1', 'normal_geo', 'photometric']


def _three_losses(monkeypatch):
    """The selector of three losses that all convert, on stubs that record the ab each operator receives."""
    from dualpixelface_amd import ops
    from dualpixelface_amd.losses import loss_selector
    calls, fit = _stubs(monkeypatch)

    def normal_geo_loss(pred, depth, normal, Kmat, ab=None, **k):
        calls.append(('normal_geo', ab))
        return torch.zeros(())

    def photometric_loss(pred, ref_rgb, tgt_rgb, ab=None, **k):
        calls.append(('photometric', ab))
        return torch.zeros(())

    monkeypatch.setattr(ops, 'normal_geo_loss', normal_geo_loss)
    monkeypatch.setattr(ops, 'photometric_loss', photometric_loss)
    sel = loss_selector(support.option('train_faceDP_dpnet', loss_type=THREE, lambdas=[1.0, 0.5, 0.25]))
    z, img = torch.ones(1, 2, 2), torch.ones(1, 3, 2, 2)
    extra = {'K': torch.eye(3).unsqueeze(0), 'normal': img, 'left': img, 'right': img}
    return sel, calls, fit, extra


def test_three_losses_fit_once_per_forward(monkeypatch):
    """One step enqueues the fit once however many losses convert with it, and again at the next step; every loss gets that tensor."""
    sel, calls, fit, extra = _three_losses(monkeypatch)
    batch, pred = dict(_batch(False), **extra), torch.ones(1, 1, 2, 2)
    for _ in range(2):
        del calls[:]
        out = sel.forward({'pred_depth': pred}, batch, 'depth')
        assert [c[0] for c in calls] == ['fit', 'bank', 'normal_geo', 'photometric']
        assert calls[0][1] is pred and calls[0][2] is batch['idepth']
        assert calls[1][4] is fit and calls[3][1] is fit and out['abvalue'] is fit
        assert calls[2][1] is None                                     # (a depth prediction: normal_geo converts nothing)
        assert set(out) == {n + '_loss' for n in THREE} | {'abvalue', 'final_loss'}
    del calls[:]
    out = sel.forward({'pred_depth': pred}, batch, 'idepth')           # here normal_geo converts and photometric does not
    assert [c[0] for c in calls] == ['fit', 'bank', 'normal_geo', 'photometric']
    assert calls[1][4] is fit and calls[2][1] is fit and calls[3][1] is None and out['abvalue'] is fit


def test_three_losses_with_abvalue_do_not_fit(monkeypatch):
    sel, calls, fit, extra = _three_losses(monkeypatch)
    batch = dict(_batch(), **extra)
    out = sel.forward({'pred_depth': torch.ones(1, 1, 2, 2)}, batch, 'depth')
    assert [c[0] for c in calls] == ['bank', 'normal_geo', 'photometric'] and calls[2][1] is batch['abvalue']
    assert out['abvalue'] is batch['abvalue']


@pytest.mark.parametrize('what', ['stereodpnet', 'nnet'])
def test_geometry_models_name_the_missing_key(what):
    from dualpixelface_amd.core import geometry_abvalue
    ab = torch.zeros(1, 2, dtype=torch.float64)
    assert geometry_abvalue({'abvalue': ab}, what).dtype == torch.float32
    with pytest.raises(NotImplementedError, match="batch\\['abvalue'\\]"):
        geometry_abvalue({'idepth': ab}, what)
