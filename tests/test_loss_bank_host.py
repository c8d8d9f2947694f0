"""The depth-target loss bank, host side (no GPU): the fp64 restatement the GPU tests hold the kernels to agrees with vectors produced by
importing the reference's SILOGLoss / SMOOTHL1Loss (tests/golden/make_golden_loss_bank.py); the hooks resolve, refuse what is not built and
keep the fused smoothL1 + cosine pass to the disparity target; the inverse-depth DPNet config loads."""
import os
from runpy import run_path

import pytest
import torch

from tests import loss_bank_cpu as lb
from tests import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_against_reference_fixture(golden_dir):
    fx = lb.Fixture(golden_dir)
    assert len(fx.cases) == 14
    assert {(c[1], c[2], c[3]) for c in fx.cases[:12]} == {(k, t, n) for k in ('silog', 'smoothL1') for t in ('disp', 'idepth', 'depth')
                                                           for n in (1, 3)}
    for case in fx.cases:
        name, kind, tt, n, masked, with_conf = case
        pred, batch = fx.inputs(case)
        assert ('mask' in batch) == masked and ('conf' in batch) == with_conf
        loss, grad = lb.hook_call(kind, tt, pred, batch, fx.head_weights(n), fx.variance_focus)
        ref_loss, ref_grad = fx.expected(case)
        support.close(loss, ref_loss, 1e-6, name + ' loss')
        support.close_elem(grad, ref_grad, name + ' grad')


def test_silog_selects_and_reads_its_options():
    from dualpixelface_amd.losses import SILOGLoss, loss_selector
    sel = loss_selector(support.option('train_faceDP_dpnet', loss_type=['silog'], variance_focus=0.6))
    assert sel.loss_name == ['silog'] and isinstance(sel.loss_func[0], SILOGLoss)
    assert sel.loss_func[0].variance_focus == 0.6
    assert sel.loss_func[0].head_weights(1) == [1.0] and sel.loss_func[0].head_weights(3) == [1.0, 0.75294, 0.18824]


def test_folded_is_still_refused():
    from dualpixelface_amd.losses import loss_selector
    with pytest.raises(NotImplementedError, match='wrong loss type : folded'):
        loss_selector(support.option('train_faceDP_dpnet', loss_type=['folded']))


def test_reference_path_exposes_silog():
    from dualpixelface_amd.losses import SILOGLoss
    assert run_path(os.path.join(ROOT, 'src', 'loss', 'depth', 'silog.py'))['SILOGLoss'] is SILOGLoss


@pytest.mark.parametrize('loss', ['silog', 'smoothL1'])
def test_bad_target_type_asserts(loss):
    from dualpixelface_amd.losses import loss_selector
    sel = loss_selector(support.option('train_faceDP_dpnet', loss_type=[loss], variance_focus=0.6))
    z = torch.ones(1, 1, 2, 2)
    batch = {'disp': z[0], 'idepth': z[0], 'depth': z[0], 'abvalue': torch.zeros(1, 2)}
    with pytest.raises(AssertionError):
        sel.forward({'pred_depth': z}, batch, target_type='inverse')


@pytest.mark.parametrize('loss', ['silog', 'smoothL1'])
def test_least_square_is_refused(loss):
    from dualpixelface_amd.losses import loss_selector
    opt = support.option('train_faceDP_dpnet', loss_type=[loss], variance_focus=0.6)
    opt.dataset.dp_conversion = 'least_square'
    with pytest.raises(NotImplementedError, match='least_square'):
        loss_selector(opt)


def test_silog_refuses_a_batch_without_abvalue():
    from dualpixelface_amd.losses import loss_selector
    sel = loss_selector(support.option('train_faceDP_dpnet', loss_type=['silog'], variance_focus=0.6))
    z = torch.ones(1, 1, 2, 2)
    with pytest.raises(NotImplementedError, match='least_square'):
        sel.forward({'pred_depth': z}, {'disp': z[0]}, target_type='disp')


def test_idepth_config_loads():
    from dualpixelface_amd import load_option
    opt = load_option('train_faceDP_dpnet_idepth')
    assert opt.model.target_type == 'idepth' and opt.model_name == 'dpnet' and opt.model.loss_type == ['smoothL1']
    base = load_option('train_faceDP_dpnet')
    assert not hasattr(base.model, 'target_type')
    for opt_, base_ in ((opt, base), (opt.model, base.model)):
        a = {k: v for k, v in vars(opt_).items() if k not in ('model', 'dataset', 'model_config', 'target_type') and not hasattr(v, '__dict__')}
        b = {k: v for k, v in vars(base_).items() if k not in ('model', 'dataset', 'model_config') and not hasattr(v, '__dict__')}
        assert a == b


def test_fused_shortcut_is_for_the_disparity_target_only(monkeypatch):
    """loss_selector's one-pass smoothL1 + cosine route compares against batch['disp']: another target type must go through the hooks."""
    from dualpixelface_amd import load_option, ops
    from dualpixelface_amd.losses import loss_selector
    calls = []

    def stereo_losses(pred_depth, pred_normal, disp, normal, mask, head_weights, lam_d, lam_n):
        calls.append(('stereo', pred_depth is not None, pred_normal is not None, disp))
        return torch.zeros(3)

    def depth_loss(pred, target, mask, conf, head_weights, kind, transform, variance_focus=0.0):
        calls.append(('bank', kind, transform, target))
        return torch.zeros(())

    monkeypatch.setattr(ops, 'stereo_losses', stereo_losses)
    monkeypatch.setattr(ops, 'depth_loss', depth_loss)
    sel = loss_selector(load_option())
    assert sel.loss_name == ['smoothL1', 'cosine']
    z = torch.ones(1, 1, 2, 2)
    batch = {'disp': z[0] * 2, 'idepth': z[0] * 3, 'depth': z[0] * 4, 'mask': z[0], 'normal': torch.ones(1, 3, 2, 2), 'abvalue': torch.zeros(1, 2)}
    results = {'pred_depth': z, 'pred_normal': torch.ones(1, 1, 3, 2, 2)}
    sel.forward(results, batch)
    assert [(c[0], c[1], c[2]) for c in calls] == [('stereo', True, True)] and calls[0][3] is batch['disp']
    del calls[:]
    out = sel.forward(results, batch, target_type='idepth')
    assert [c[:3] for c in calls] == [('bank', 'smoothL1', 'identity'), ('stereo', False, True)]
    assert calls[0][3] is batch['idepth'] and set(out) == {'smoothL1_loss', 'abvalue', 'cosine_loss', 'final_loss'}
    del calls[:]
    sel.forward(results, batch, target_type='depth')
    assert calls[0][:3] == ('bank', 'smoothL1', 'reciprocal') and calls[0][3] is batch['idepth']
