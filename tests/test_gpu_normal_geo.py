"""The geometric-normal loss on the GPU (run with ``-m gpu``): csrc/normal_geo.hip through ops.normal_geo_loss against the restatements of
tests/normal_geo_cpu.py.

Exact: the counted pixels and the normals (orientation included) equal the fp32 numpy restatement bit for bit, and with pred = depth they
are ops.depth_normals' own.  Bounded: the loss against the fp64 restatement within 2 x (the fp32 restatement's own deviation from fp64);
d pred against the fp64 autograd gradient, element-wise, within 2 x (the largest deviation of the fp32 autograd gradient from it) + 1e-6
of the largest gradient magnitude.  The fp32 figures are computed here, on the same input, not fixed in advance.
"""
import numpy as np
import pytest
import torch

from tests import normal_geo_cpu as ng
from tests import support
from tests.support import DEV, bits, tensor

pytestmark = pytest.mark.gpu


def _call_normal_geo(c, gout=None, backward=True, **over):
    """The operator on a case dict (fields replaced by `over`) -> (loss as a float, normal, counted, d pred) as numpy arrays."""
    c = dict(c, **over)
    p = tensor(c['pred']).requires_grad_(True)
    loss, nrm, cnt = support.ops().normal_geo_loss(p, tensor(c['depth']), tensor(c['normal']), tensor(c['K']), ab=tensor(c['ab']),
                                                   mask=tensor(c['mask']), head_weights=c['head_weights'], target_type=c['target_type'],
                                                   max_edge_ratio=c['ratio'], step=c['step'], towards_camera=c['towards_camera'],
                                                   target_signs=c['target_signs'], return_normals=True)
    assert loss.shape == () and loss.dtype == torch.float32 and nrm.dtype == torch.float32 and cnt.dtype == torch.uint8
    grad = None
    if backward:
        (loss if gout is None else loss * gout).backward()
        grad = p.grad.cpu().numpy()
    return float(loss.detach().double()), nrm.cpu().numpy(), cnt.cpu().numpy(), grad


# ---- 1. the forward, exactly
@pytest.mark.parametrize('name', sorted(ng.CASES))
def test_counted_pixels_and_normals_equal_the_fp32_restatement(name):
    ref = ng.case(name)
    loss, nrm, cnt, _ = _call_normal_geo(ref['case'], backward=False)
    r32 = ref['r32']
    assert np.array_equal(cnt, r32['counted'])
    assert np.array_equal(bits(nrm), bits(r32['normal'])), float(np.abs(nrm - r32['normal']).max())
    # the orientation: n . P <= 0 under towards_camera on every counted pixel, >= 0 otherwise
    for h in range(cnt.shape[1]):
        dot = (nrm[:, h].astype(np.float64) * r32['dec'][h]['P']).sum(1)[cnt[:, h] > 0]
        assert (dot < 0).all() if ref['case']['towards_camera'] else (dot > 0).all()
    print('forward %s: %d of %d pixels counted, loss %.9g (fp32 restatement %.9g)' % (name, cnt.sum(), cnt.size, loss, r32['loss']))


def test_with_pred_equal_to_depth_the_normals_are_depth_normals_own():
    c = ng.make_case(B=2, n=1, H=19, W=70, seed=41, target_type='depth', masked=True, bad=True)
    c['pred'] = c['depth'][:, None].copy()                           # the junk of the target included: NaN, Inf, 0, negative
    c['normal'] = np.ones_like(c['normal'])                          # every target normal has a length: counted = normal_valid
    _, nrm, cnt, _ = _call_normal_geo(c, backward=False)
    want, valid = support.ops().depth_normals(tensor(c['depth']), tensor(c['K']), mask=tensor(c['mask']), target_type='depth', near=0.0,
                                              far=None, max_edge_ratio=c['ratio'], towards_camera=True)
    want, valid = want.cpu().numpy(), valid.cpu().numpy()
    assert 0 < valid.sum() < valid.size and np.array_equal(cnt[:, 0], valid)
    assert np.array_equal(bits(nrm[:, 0]), bits(want))


# ---- 2. loss and gradient against fp64
@pytest.mark.parametrize('name', sorted(ng.CASES))
def test_loss_and_gradient_against_the_fp64_restatement(name):
    ref = ng.case(name)
    loss, _, cnt, grad = _call_normal_geo(ref['case'])
    own_loss = abs(ref['r32']['loss'] - ref['loss64'])
    err_loss = abs(loss - ref['loss64'])
    g64, g32 = ref['grad64'], ref['grad32']
    own = float(np.abs(g32 - g64).max())
    bar = 2.0 * own + 1e-6 * float(np.abs(g64).max())
    err = float(np.abs(grad.astype(np.float64) - g64).max())
    print('normal_geo %s: loss %.9g, |loss - fp64| %.3e (bar 2 x %.3e); max |d pred - fp64 autograd| %.3e (bar %.3e = 2 x %.3e + 1e-6 x %.3e)'
          % (name, loss, err_loss, own_loss, err, bar, own, np.abs(g64).max()))
    assert np.isfinite(grad).all()
    assert err_loss <= 2.0 * own_loss
    assert (np.abs(grad.astype(np.float64) - g64) <= bar).all(), (err, bar)
    # every element is written: exactly 0 where the pixel is not usable or nothing reaches it
    assert not grad[g64 == 0].any() and (g64 == 0).any() == (cnt.sum() < cnt.size)


# ---- 3. the tilted plane
def test_tilted_plane_gives_zero_and_one_minus_cos_theta():
    """The output is an fp32 scalar, so one fp32 ulp of the expected value is added to 2 x (the fp32 restatement's own error)."""
    c, _ = ng.plane_case(0.0)
    loss, _, cnt, _ = _call_normal_geo(c, backward=False)
    r32 = ng.run(c)['loss']
    print('tilted plane: loss %.3e (fp32 restatement %.3e)' % (loss, r32))
    assert cnt.all() and 0.0 <= loss <= 2.0 * r32
    theta = 0.25
    c, want = ng.plane_case(theta)
    loss, _, _, _ = _call_normal_geo(c, backward=False)
    own = abs(ng.run(c)['loss'] - want)
    print('tilted plane, theta %.2f: loss %.9g, 1 - cos %.9g, error %.3e (bar 2 x %.3e + ulp)' % (theta, loss, want, abs(loss - want), own))
    assert abs(loss - want) <= 2.0 * own + float(np.spacing(np.float32(want)))


# ---- 4. nothing counted, and what must not reach a sum
def test_zero_counted_pixels_give_zero_loss_and_zero_gradient():
    c = ng.make_case(**ng.CASES['holes-40x33-disp'])
    loss, nrm, cnt, grad = _call_normal_geo(c, mask=np.zeros_like(c['depth']))
    assert loss == 0.0 and not cnt.any() and not nrm.any() and not grad.any() and np.isfinite(grad).all()
    # one head with pixels, one without (its prediction converts to negative depths): the empty head adds 0, not NaN
    c2 = ng.make_case(B=1, n=2, H=19, W=70, seed=43, target_type='disp', masked=True, bad=False)
    pred = c2['pred'].copy()
    pred[:, 1] = c2['ab'][0, 0] - 7.0                                # pred - b < 0: z_p < 0 everywhere
    loss2, _, cnt2, grad2 = _call_normal_geo(c2, pred=pred)
    one = ng.run(dict(c2, pred=pred[:, :1], head_weights=(1.0,)))
    assert cnt2[:, 0].any() and not cnt2[:, 1].any() and not grad2[:, 1].any() and grad2[:, 0].any()
    assert np.isfinite(loss2) and abs(loss2 - one['loss']) <= 2e-7 * one['loss']


def test_junk_under_the_mask_never_reaches_a_sum():
    c = ng.make_case(B=1, n=1, H=24, W=40, seed=44, target_type='disp', masked=True, bad=False)
    clean = _call_normal_geo(c)
    pred = c['pred'].copy()
    off = np.argwhere(~(c['mask'][0] > 0))
    assert len(off) >= 6
    for k, v in enumerate((np.nan, np.inf, -np.inf, 1e30, -1e30, c['ab'][0, 0])):
        pred[0, 0, off[k][0], off[k][1]] = v
    junk = _call_normal_geo(c, pred=pred)
    assert junk[0] == clean[0] and np.array_equal(bits(junk[3]), bits(clean[3])) and np.array_equal(junk[2], clean[2])
    assert np.array_equal(bits(junk[1]), bits(clean[1]))


def test_a_nan_prediction_removes_its_pixel_and_the_stencils_through_it():
    c = ng.make_case(B=1, n=1, H=24, W=40, seed=44, target_type='disp', masked=True, bad=False)
    on = np.argwhere(ng.run(c)['counted'][0, 0] > 0)
    y, x = [p for p in on if 2 <= p[0] < 22 and 2 <= p[1] < 38][5]
    pred = c['pred'].copy()
    pred[0, 0, y, x] = np.nan
    got = _call_normal_geo(c, pred=pred)
    mask = c['mask'].copy()
    mask[0, y, x] = 0.0
    want = _call_normal_geo(c, mask=mask)                                       # the same pixel taken out by the mask instead
    assert np.isfinite(got[0]) and np.isfinite(got[3]).all() and np.isfinite(got[1]).all()
    assert got[0] == want[0] and np.array_equal(got[2], want[2]) and np.array_equal(bits(got[1]), bits(want[1]))
    assert np.array_equal(bits(got[3]), bits(want[3])) and got[3][0, 0, y, x] == 0.0 and not got[2][0, 0, y, x]
    assert got[2].sum() < ng.run(c)['counted'].sum()


# ---- 5. the bits repeat
def _abi_args(c):
    held = [tensor(c['pred']), tensor(c['depth']), tensor(c['normal']), tensor(c['K']), tensor(c['ab']), tensor(c['mask'])]
    B, n, H, W = c['pred'].shape
    ops = support.ops()
    tail = (B, n, H, W, ops.TARGET_TYPES[c['target_type']], c['ratio'], c['step'], int(c['towards_camera']),
            ops._host_floats(c['target_signs']), ops._host_floats(c['head_weights']))
    return held, tuple(ops._ptr(t) for t in held) + tail


def test_two_calls_return_the_same_bits_whatever_the_scratch_held():
    from dualpixelface_amd._lib import lib
    ops = support.ops()
    c = ng.case('heads-19x70-idepth-singular1')['case']
    held, args = _abi_args(c)
    B, n, H, W = c['pred'].shape
    nbytes = lib().call('dpf_normal_geo_workspace_bytes', B, n, H, W)
    assert nbytes == n * B * 3 * 3 * 16
    outs = []
    for poison in (float('nan'), -3e30):
        ws = torch.full(((nbytes + 7) // 8,), poison, dtype=torch.float64, device=DEV)
        stats = torch.full((ops.NORMAL_GEO_STATS,), poison, dtype=torch.float64, device=DEV)
        out = torch.full((), poison, dtype=torch.float32, device=DEV)
        dpred = torch.full(c['pred'].shape, poison, dtype=torch.float32, device=DEV)
        gout = torch.ones((), dtype=torch.float32, device=DEV)
        lib().call('dpf_normal_geo_forward', *args, ops._ptr(ws), nbytes, ops._ptr(stats), ops._ptr(out), None, None, ops._stream())
        lib().call('dpf_normal_geo_backward', *args, ops._ptr(stats), ops._ptr(gout), ops._ptr(dpred), ops._stream())
        outs.append((out.cpu().numpy(), stats.cpu().numpy(), dpred.cpu().numpy()))
    (o1, s1, d1), (o2, s2, d2) = outs
    assert np.isfinite(o1) and np.isfinite(d1).all() and np.isfinite(s1).all()
    assert bits(o1) == bits(o2) and np.array_equal(s1, s2) and np.array_equal(bits(d1), bits(d2))
    loss, _, _, grad = _call_normal_geo(c)                                      # and the operator, with whatever the allocator hands it
    assert np.float32(loss) == o1 and np.array_equal(bits(grad), bits(d1))
    ref = ng.case('heads-19x70-idepth-singular1')
    assert s1[:3].tolist() == ref['r32']['count'] and not s1[3:8].any()


def test_a_captured_call_replays_the_eager_bits():
    ops = support.ops()
    c = ng.case('holes-40x33-disp')['case']
    eager_loss, _, _, eager_grad = _call_normal_geo(c)
    p = tensor(c['pred']).requires_grad_(True)
    fixed = [tensor(c[k]) for k in ('depth', 'normal', 'K', 'ab', 'mask')]

    def run():
        loss = ops.normal_geo_loss(p, fixed[0], fixed[1], fixed[2], ab=fixed[3], mask=fixed[4], head_weights=c['head_weights'],
                                   target_type=c['target_type'], max_edge_ratio=c['ratio'], step=c['step'])
        return loss, torch.autograd.grad(loss, p)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, grad = run()
    for _ in range(2):
        loss.fill_(float('nan'))
        grad.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert float(loss.detach().double()) == eager_loss and np.array_equal(bits(grad.cpu().numpy()), bits(eager_grad))


def test_gout_scales_the_gradient_to_within_one_ulp():
    c = ng.case('holes-40x33-disp')['case']
    _, _, _, g1 = _call_normal_geo(c)
    _, _, _, gs = _call_normal_geo(c, gout=0.37)
    want = g1.astype(np.float64) * 0.37
    assert (np.abs(gs.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32))).all()
    assert np.array_equal(gs == 0, g1 == 0) and gs.any()


# ---- 6. the C ABI's refusals
def test_abi_refuses_bad_arguments():
    from dualpixelface_amd._lib import lib, DpfError
    ops = support.ops()
    c = ng.case('tiny-5x7-disp')['case']
    held, args = _abi_args(c)
    q = lambda *a: lib().call('dpf_normal_geo_workspace_bytes', *a)                                # noqa: E731
    assert q(1, 1, 5, 7) == 16 and q(2, 3, 19, 70) == 2 * 3 * 9 * 16 and q(1, 1, 8, 32) == 16 and q(1, 1, 9, 33) == 64
    assert q(0, 1, 5, 7) == -1 and q(1, 9, 5, 7) == -1 and q(1, 0, 5, 7) == -1 and q(1, 1, 0, 7) == -1 and q(8192, 8, 5, 7) == -1
    ws = torch.zeros(2, dtype=torch.float64, device=DEV)
    stats = torch.zeros(ops.NORMAL_GEO_STATS, dtype=torch.float64, device=DEV)
    out = torch.full((), 7.0, dtype=torch.float32, device=DEV)
    tail = (ops._ptr(ws), 16, ops._ptr(stats), ops._ptr(out), None, None, ops._stream())

    def refused(a, t, code):
        with pytest.raises(DpfError, match=code):
            lib().call('dpf_normal_geo_forward', *a, *t)

    a = list(args)
    refused(a[:12] + [3] + a[13:], tail, 'DPF_ERR_UNSUPPORTED')                                   # step 3
    refused(a[:12] + [0] + a[13:], tail, 'DPF_ERR_INVALID_ARG')                                   # step 0
    refused(a[:11] + [0.0] + a[12:], tail, 'DPF_ERR_INVALID_ARG')                                 # max_edge_ratio 0
    refused(a[:10] + [3] + a[11:], tail, 'DPF_ERR_INVALID_ARG')                                   # target type 3
    refused(a[:4] + [None] + a[5:], tail, 'DPF_ERR_INVALID_ARG')                                  # a disp model without ab
    refused(a[:14] + [ops._host_floats((1, 0.5, 1))] + a[15:], tail, 'DPF_ERR_INVALID_ARG')       # a sign that is not +-1
    refused(a, (ops._ptr(ws), 8) + tail[2:], 'DPF_ERR_INVALID_ARG')                               # workspace too small
    nrm = torch.zeros((1, 1, 3, 5, 7), dtype=torch.float32, device=DEV)
    refused(a, tail[:4] + (ops._ptr(nrm), None) + tail[6:], 'DPF_ERR_INVALID_ARG')                # one of the optional pair
    torch.cuda.synchronize()
    assert float(out) == 7.0                                                                       # a refusal launches nothing
    with pytest.raises(DpfError, match='DPF_ERR_INVALID_ARG'):
        lib().call('dpf_normal_geo_backward', *a, ops._ptr(stats), None, ops._ptr(nrm), ops._stream())
    with pytest.raises(DpfError, match='step must be 1, 2 or 4'):
        _call_normal_geo(c, step=3)
    with pytest.raises(DpfError, match='target_signs'):
        _call_normal_geo(c, target_signs=(1, 1, 0))


# ---- 7. the whole step
def test_dpnet_trains_with_normal_geo_graph_equals_eager(monkeypatch):
    ops = support.ops()
    from dualpixelface_amd.recipe import synthetic_batch
    batch = {k: v.to(DEV) for k, v in synthetic_batch(2, 64, 96, seed=7, mask_mode='bern').items()}
    both = dict(loss_type=['smoothL1', 'normal_geo'], lambdas=[1.0, 0.1])
    with ops.deterministic_mode():
        monkeypatch.setenv('DPF_STEP_GRAPH', '0')
        plain = support.dpnet()                                             # smoothL1 alone, before the new loss exists in a model
        plain_losses = support.loss_steps(plain, batch, 3)
        plain_grads = plain.flat_gradients(zero=False).clone()
        b = support.dpnet(**both)
        assert b.loss_model.loss_name == ['smoothL1', 'normal_geo']
        eager = support.loss_steps(b, batch, 4)
        eager_grads = b.flat_gradients(zero=False).clone()
        monkeypatch.setenv('DPF_STEP_GRAPH', '1')
        a = support.dpnet(**both)
        graphed = support.loss_steps(a, batch, 4)                    # two warm-up steps, the capture, one replay
        assert a._graph_state.get('graph') is not None and not a._graph_state.get('failed')
        monkeypatch.setenv('DPF_STEP_GRAPH', '0')
        again = support.dpnet()
        again_losses = support.loss_steps(again, batch, 3)
    assert graphed == eager, (graphed, eager)
    assert torch.equal(a.flat_parameters(), b.flat_parameters())
    for step in eager:
        assert set(step) == {'smoothL1_loss', 'normal_geo_loss', 'final_loss'} and all(np.isfinite(v) for v in step.values())
        assert step['normal_geo_loss'] > 0
        want = float(torch.tensor(step['smoothL1_loss'], dtype=torch.float32) * 1.0 + torch.tensor(step['normal_geo_loss'], dtype=torch.float32) * 0.1)
        assert step['final_loss'] == want, (step, want)
    # the normals reach the weights: after the first step the two runs are different models
    assert eager[0]['smoothL1_loss'] == plain_losses[0]['smoothL1_loss'] and eager[1]['smoothL1_loss'] != plain_losses[1]['smoothL1_loss']
    assert not torch.equal(eager_grads, plain_grads)
    # and a loss_type without it computes what it computed before the loss was constructed in this process
    assert again_losses == plain_losses and torch.equal(again.flat_parameters(), plain.flat_parameters())
    assert torch.equal(again.flat_gradients(zero=False), plain_grads)


def test_first_step_gradient_arena_differs_from_the_smoothl1_only_run(monkeypatch):
    ops = support.ops()
    from dualpixelface_amd.recipe import synthetic_batch
    batch = {k: v.to(DEV) for k, v in synthetic_batch(2, 64, 96, seed=7, mask_mode='bern').items()}
    monkeypatch.setenv('DPF_STEP_GRAPH', '0')
    with ops.deterministic_mode():
        plain, both = support.dpnet(), support.dpnet(loss_type=['smoothL1', 'normal_geo'], lambdas=[1.0, 0.1])
        support.loss_steps(plain, batch, 1)
        support.loss_steps(both, batch, 1)
    ga, gb = plain.flat_gradients(zero=False), both.flat_gradients(zero=False)
    assert torch.isfinite(gb).all() and not torch.equal(ga, gb) and float((ga - gb).abs().max()) > 0


def test_stereodpnet_step_returns_all_three_losses(monkeypatch):
    from dualpixelface_amd import load_option
    from dualpixelface_amd.plugin import STEREODPNET
    from dualpixelface_amd.recipe import fill_by_recipe, synthetic_batch
    monkeypatch.setenv('DPF_STEP_GRAPH', '0')
    model = STEREODPNET(load_option('train_faceDP', loss_type=['smoothL1', 'cosine', 'normal_geo'], lambdas=[1.0, 1.0, 0.1]))
    fill_by_recipe(model)
    model.to(DEV).train()
    batch = {k: v.to(DEV) for k, v in synthetic_batch(1, 32, 48, seed=5, mask_mode='bern').items()}
    res = model.train_step(batch)
    for key in ('smoothL1_loss', 'cosine_loss', 'normal_geo_loss', 'final_loss'):
        assert key in res and np.isfinite(float(res[key].detach())), key
    want = res['smoothL1_loss'] * 1.0 + res['cosine_loss'] * 1.0 + res['normal_geo_loss'] * 0.1
    assert float(res['final_loss'].detach()) == float(want.detach())
