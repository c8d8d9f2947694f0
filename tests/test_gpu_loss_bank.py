"""The depth-target loss bank on the GPU (run with ``-m gpu``): csrc/loss_bank.hip through losses.loss_selector and ops.depth_loss against
the reference's own vectors (tests/golden/loss_bank.npz) and the fp64 restatement (tests/loss_bank_cpu.py).  Bars: loss 1e-5 relative,
gradients by close_elem -- the bars of test_gpu_ops.py::test_losses_against_reference_fixture."""
import ctypes

import numpy as np
import pytest
import torch

from tests import loss_bank_cpu as lb
from tests import support
from tests.support import DEV

pytestmark = pytest.mark.gpu

CASES = ['%s_%s_n%d' % (k, t, n) for k in ('silog', 'smoothL1') for t in ('disp', 'idepth', 'depth') for n in (1, 3)]
CASES += ['silog_idepth_n3_conf_nomask', 'smoothL1_idepth_n3_conf']


def _selector(kind, loss_weight, variance_focus):
    from dualpixelface_amd import load_option
    from dualpixelface_amd.losses import loss_selector
    return loss_selector(load_option('train_faceDP_dpnet', loss_type=[kind], lambdas=[1.0], loss_weight=loss_weight,
                                     variance_focus=variance_focus))


@pytest.fixture(scope='module')
def fixture(golden_dir):
    return lb.Fixture(golden_dir)


# ---- 1. the reference's vectors through the hooks
@pytest.mark.parametrize('name', CASES)
def test_hooks_against_reference_fixture(name, fixture):
    assert [c[0] for c in fixture.cases] == CASES
    case = fixture.cases[CASES.index(name)]
    _, kind, tt, n, masked, with_conf = case
    pred, batch = fixture.inputs(case, DEV)
    pred.requires_grad_()
    res = _selector(kind, fixture.loss_weight, fixture.variance_focus).forward({'pred_depth': pred}, batch, tt)
    assert res['abvalue'] is batch['abvalue'] and res['final_loss'].dim() == 0
    ref_loss, ref_grad = fixture.expected(case)
    support.close(res[kind + '_loss'], ref_loss, 1e-5, name + ' loss')
    support.close(res['final_loss'], ref_loss, 1e-5, name + ' final_loss')
    grad, = torch.autograd.grad(res['final_loss'], pred)
    support.close_elem(grad, ref_grad, name + ' grad')


# ---- 2. several workgroups per sample, odd sizes (one pixel per load) and sizes the 4-pixel loads take, 1 / 5 / 8 heads
def _loss_fields(B, n, H, W, seed, mask, conf):
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi, *shape: torch.rand(*shape, generator=g) * (hi - lo) + lo
    pred, target = u(0.5, 2.5, B, n, H, W), u(0.5, 2.5, B, H, W)
    m = (torch.rand(B, H, W, generator=g) < 0.6).float() if mask else None
    c = u(0.1, 1.0, B, H, W) if conf else None
    return pred, target, m, c


def _run_depth_loss(pred, target, mask, conf, weights, kind, transform, vf):
    dev = lambda t: None if t is None else t.to(DEV)
    p = pred.to(DEV).requires_grad_()
    loss = support.ops().depth_loss(p, dev(target), dev(mask), dev(conf), weights, kind, transform, vf)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    grad, = torch.autograd.grad(loss, p)
    return loss, grad


WEIGHTS8 = [1.0, 0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3]
SHAPES = [(3, 5, 67, 129), (2, 8, 67, 129), (2, 8, 68, 128), (2, 1, 68, 128)]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
@pytest.mark.parametrize('conf', [False, True], ids=['noconf', 'conf'])
@pytest.mark.parametrize('mask', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('transform', ['identity', 'reciprocal'])
@pytest.mark.parametrize('kind', ['silog', 'smoothL1'])
def test_partial_fold_and_tails(kind, transform, mask, conf, shape):
    B, n, H, W = shape
    pred, target, m, c = _loss_fields(B, n, H, W, 5, mask, conf)
    weights = WEIGHTS8[:n]
    loss, grad = _run_depth_loss(pred, target, m, c, weights, kind, transform, 0.85)
    ref_loss, ref_grad = lb.depth_loss(pred, target, m, c, weights, kind, transform, 0.85)
    assert torch.isfinite(ref_loss)
    tag = '%s %s %s' % (kind, transform, shape)
    support.close(loss, ref_loss, 1e-5, tag + ' loss')
    support.close_elem(grad, ref_grad, tag + ' grad')


@pytest.mark.parametrize('kind', ['silog', 'smoothL1'])
def test_fold_of_more_rows_than_threads(kind):
    """B = 3 at 512 x 704: 88 partial rows per sample, 264 in the one fold, so a fold thread adds more than one row (SHAPES fold <= 9)."""
    pred, target, m, _ = _loss_fields(3, 2, 512, 704, 12, True, False)
    weights = WEIGHTS8[:2]
    loss, grad = _run_depth_loss(pred, target, m, None, weights, kind, 'identity', 0.85)
    ref_loss, ref_grad = lb.depth_loss(pred, target, m, None, weights, kind, 'identity', 0.85)
    assert torch.isfinite(ref_loss)
    support.close(loss, ref_loss, 1e-5, kind + ' 264 rows loss')
    support.close_elem(grad, ref_grad, kind + ' 264 rows grad')


@pytest.mark.parametrize('kind', ['silog', 'smoothL1'])
def test_one_head_weighs_one(kind):
    """One head: weight [1.0] even though loss_weight is longer and starts elsewhere (smoothL1.py:22, silog.py:23)."""
    pred, target, m, _ = _loss_fields(2, 1, 67, 129, 6, True, False)
    batch = {'disp': target.to(DEV), 'idepth': target.to(DEV), 'depth': target.to(DEV), 'mask': m.to(DEV), 'abvalue': torch.zeros(2, 2, device=DEV)}
    p = pred.to(DEV).requires_grad_()
    res = _selector(kind, [0.5, 0.25, 0.125], 0.85).forward({'pred_depth': p}, batch, 'idepth')
    ref_loss, ref_grad = lb.depth_loss(pred, target, m, None, [1.0], kind, 'identity', 0.85)
    support.close(res['final_loss'], ref_loss, 1e-5, kind + ' loss')
    support.close_elem(torch.autograd.grad(res['final_loss'], p)[0], ref_grad, kind + ' grad')


# ---- 3. what lies under the mask stays out
def test_masked_out_values_do_not_leak():
    pred, target, m, _ = _loss_fields(2, 3, 24, 40, 7, True, False)
    off = (m == 0).nonzero()
    on = (m > 0).nonzero()
    (b0, y0, x0), (b1, y1, x1) = off[0].tolist(), off[-1].tolist()
    pred[b0, 1, y0, x0] = -3.0
    pred[b1, 2, y1, x1] = float('nan')
    weights = [1.0, 0.7, 0.5]
    loss, grad = _run_depth_loss(pred, target, m, None, weights, 'silog', 'identity', 0.85)
    ref_loss, ref_grad = lb.depth_loss(pred, target, m, None, weights, 'silog', 'identity', 0.85)
    assert torch.isfinite(loss) and bool(torch.isfinite(grad).all())
    support.close(loss, ref_loss, 1e-5, 'loss')
    support.close_elem(grad, ref_grad, 'grad')
    assert bool((grad.cpu().transpose(0, 1)[:, m == 0] == 0).all()) and float(grad[b0, 1, y0, x0]) == 0.0 and float(grad[b1, 2, y1, x1]) == 0.0
    b2, y2, x2 = on[0].tolist()
    pred[b2, 1, y2, x2] = -3.0                                    # the same value where it counts: NaN, as in the reference (no clamp)
    loss, grad = _run_depth_loss(pred, target, m, None, weights, 'silog', 'identity', 0.85)
    assert bool(torch.isnan(loss))
    assert bool((grad.cpu().transpose(0, 1)[:, m == 0] == 0).all())           # and still nothing is written under the mask but zeros


# ---- 4. predictions that are exactly 0 under the reciprocal
def test_reciprocal_of_zero_predictions():
    pred, target, m, _ = _loss_fields(2, 3, 24, 40, 8, True, False)
    on = (m > 0).nonzero()
    spots = [tuple(on[0].tolist()), tuple(on[-1].tolist())]
    for k, (b, y, x) in zip((0, 2), spots):
        pred[b, k, y, x] = 0.0
    weights = [1.0, 0.7, 0.5]
    batch = {'idepth': target.to(DEV), 'disp': target.to(DEV), 'mask': m.to(DEV), 'abvalue': torch.zeros(2, 2, device=DEV)}
    p = pred.to(DEV).requires_grad_()
    res = _selector('smoothL1', weights, 0.0).forward({'pred_depth': p}, batch, 'depth')
    grad, = torch.autograd.grad(res['final_loss'], p)
    ref_loss, ref_grad = lb.depth_loss(pred, target, m, None, weights, 'smoothL1', 'reciprocal')     # substitutes 0 for 1 / 0
    support.close(res['final_loss'], ref_loss, 1e-5, 'loss')
    assert bool(torch.isfinite(grad).all())
    support.close_elem(grad, ref_grad, 'grad')
    for k, (b, y, x) in zip((0, 2), spots):
        assert float(grad[b, k, y, x]) == 0.0


# ---- 5. the same bits twice
@pytest.mark.parametrize('kind', ['silog', 'smoothL1'])
def test_results_repeat_bit_for_bit(kind):
    pred, target, m, c = _loss_fields(3, 5, 67, 129, 9, True, True)
    a = _run_depth_loss(pred, target, m, c, WEIGHTS8[:5], kind, 'identity', 0.85)
    b = _run_depth_loss(pred, target, m, c, WEIGHTS8[:5], kind, 'identity', 0.85)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 6. nothing counted
@pytest.mark.parametrize('kind', ['silog', 'smoothL1'])
def test_empty_mask(kind):
    pred, target, _, _ = _loss_fields(2, 3, 24, 40, 10, False, False)
    loss, grad = _run_depth_loss(pred, target, torch.zeros(2, 24, 40), None, [1.0, 0.7, 0.5], kind, 'identity', 0.85)     # (a failed call raises)
    assert bool(torch.isnan(loss)) and bool((grad == 0).all())


# ---- 7. the C ABI refuses before it launches
@pytest.mark.parametrize('n,kind,transform', [(0, 0, 0), (9, 1, 0), (3, 2, 0), (3, 0, 2)])
def test_abi_refuses_bad_arguments(n, kind, transform):
    from dualpixelface_amd._lib import lib, DpfError
    B, H, W = 1, 8, 8
    pred = torch.ones(B, 9, H, W, device=DEV)
    target = torch.ones(B, H, W, device=DEV)
    nbytes = lib().call('dpf_depth_loss_workspace_bytes', B, H, W)
    assert nbytes > 0
    ws = torch.zeros(nbytes // 8, dtype=torch.float64, device=DEV)
    stats = torch.full((17,), -7.0, dtype=torch.float64, device=DEV)
    out = torch.full((1,), -7.0, device=DEV)
    dpred = torch.full_like(pred, -7.0)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    weights = (ctypes.c_float * 9)(*([1.0] * 9))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    with pytest.raises(DpfError, match='DPF_ERR_INVALID_ARG'):
        lib().call('dpf_depth_loss_forward', kind, transform, ptr(pred), ptr(target), None, None, None, B, n, H, W, weights, 0.85, ptr(ws), nbytes,
                   ptr(stats), ptr(out), stream)
    with pytest.raises(DpfError, match='DPF_ERR_INVALID_ARG'):
        lib().call('dpf_depth_loss_backward', kind, transform, ptr(pred), ptr(target), None, None, None, B, n, H, W, weights, 0.85, ptr(stats),
                   ptr(out), ptr(dpred), stream)
    torch.cuda.synchronize()
    assert float(out) == -7.0 and bool((stats == -7.0).all()) and bool((dpred == -7.0).all()) and bool((ws == 0).all())


def test_abi_refuses_missing_pointers():
    from dualpixelface_amd._lib import lib, DpfError
    B, n, H, W = 1, 2, 8, 8
    pred = torch.ones(B, n, H, W, device=DEV)
    target = torch.ones(B, H, W, device=DEV)
    nbytes = lib().call('dpf_depth_loss_workspace_bytes', B, H, W)
    ws = torch.zeros(nbytes // 8, dtype=torch.float64, device=DEV)
    stats = torch.zeros(17, dtype=torch.float64, device=DEV)
    out = torch.zeros(1, device=DEV)
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    weights = (ctypes.c_float * n)(1.0, 0.5)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for args in ((None, target, ws, stats, out), (pred, None, ws, stats, out), (pred, target, None, stats, out), (pred, target, ws, None, out),
                 (pred, target, ws, stats, None)):
        p, t, w_, s, o = args
        with pytest.raises(DpfError, match='DPF_ERR_INVALID_ARG'):
            lib().call('dpf_depth_loss_forward', 0, 0, ptr(p), ptr(t), None, None, None, B, n, H, W, weights, 0.0, ptr(w_), nbytes, ptr(s), ptr(o),
                       stream)
    with pytest.raises(DpfError, match='DPF_ERR_INVALID_ARG'):            # a workspace that is too small
        lib().call('dpf_depth_loss_forward', 0, 0, ptr(pred), ptr(target), None, None, None, B, n, H, W, weights, 0.0, ptr(ws), nbytes - 8, ptr(stats),
                   ptr(out), stream)
    assert lib().call('dpf_depth_loss_workspace_bytes', 0, H, W) == -1


# ---- 8. the whole step: DPNet trained on inverse depth
def test_dpnet_trains_on_inverse_depth_graph_equals_eager(monkeypatch):
    from dualpixelface_amd import ops
    from dualpixelface_amd.recipe import synthetic_batch
    batch = {k: v.to(DEV) for k, v in synthetic_batch(2, 64, 96, seed=7, mask_mode='bern').items()}
    with ops.deterministic_mode():
        monkeypatch.setenv('DPF_STEP_GRAPH', '1')
        a = support.dpnet('train_faceDP_dpnet_idepth')
        assert a.option.model.target_type == 'idepth'
        before = a.flat_parameters().clone()
        la = [float(a.train_step(batch, None, lr=1e-3)['final_loss'].detach()) for _ in range(4)]      # two warm-up steps, the capture, one replay
        assert a._graph_state.get('graph') is not None and not a._graph_state.get('failed')
        monkeypatch.setenv('DPF_STEP_GRAPH', '0')
        b = support.dpnet('train_faceDP_dpnet_idepth')
        lb_, weights = [], b.loss_model.loss_func[0].head_weights(5)
        for _ in range(4):
            res = b.train_step(batch, None, lr=1e-3)
            assert res['pred_depth'].shape == (2, 5, 64, 96)
            ref_loss, _ = lb.depth_loss(res['pred_depth'], batch['idepth'], batch['mask'], None, weights, 'smoothL1', 'identity')
            support.close(res['final_loss'], ref_loss, 1e-5, 'step %d final_loss' % len(lb_))
            lb_.append(float(res['final_loss'].detach()))
    assert all(np.isfinite(la)) and la == lb_, (la, lb_)
    assert float((a.flat_parameters() - before).abs().max()) > 0
    assert torch.equal(a.flat_parameters(), b.flat_parameters())


def test_dpnet_constructs_with_silog():
    model = support.dpnet('train_faceDP_dpnet_idepth', loss_type=['silog'], variance_focus=0.6)
    assert model.loss_model.loss_name == ['silog'] and model.loss_model.loss_func[0].variance_focus == 0.6
