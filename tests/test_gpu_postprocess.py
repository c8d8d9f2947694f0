"""The post_process filters on the GPU (run with ``-m gpu``): csrc/postprocess.hip through ops.guided_filter / ops.joint_bilateral_filter and
through the plugins' evaluation forward, against the fp64 restatement of tests/postprocess_cpu.py.

Bars.  Element-wise: max |q - q64| <= 2 x (max error of the restatement's fp32 variant against fp64 on the same input) + 1e-6, computed
here per case (the factor 2: a different summation order).  Hard statistics (guided, p + 200): 2 x the fp32 variant's error on the
UNSHIFTED input + 2 ulp(200) -- the kernels take their moments about a pixel of the band, so the offset must cost no more than the
roundings of the result itself.  Measured on an MI355X (kernel error / bar): see profiles/postprocess_timings.txt.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import postprocess_cpu as pc
from tests import support
from tests.support import DEV, ptr, stream

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS, SIGMA_COLOR, ULP200 = pc.EPS, pc.SIGMA_COLOR, pc.ULP200
GUIDED, BILATERAL = pc.GUIDED, pc.BILATERAL
_id, _sigma_space, _case, _on_device, _run = pc.case_id, pc.sigma_space, pc.case, pc.on_device, pc.run_filter


def _check(kind, case):
    p, guide, q64, bar = _case(kind, case)
    q = _run(kind, _on_device(p, case[5]), guide.to(DEV), case[4])
    assert q.dtype == torch.float32 and tuple(q.shape) == tuple(p.shape) and q.is_contiguous() and not q.requires_grad
    err = float((q.cpu().double() - q64).abs().max())
    print('%s %s: max |q - q64| %.3e (bar %.3e)' % (kind, _id(case), err, bar))
    assert err <= bar


# ---- 1. against the fp64 restatement
@pytest.mark.parametrize('case', GUIDED, ids=_id)
def test_guided_against_fp64(case):
    _check('guided', case)


@pytest.mark.parametrize('case', BILATERAL, ids=_id)
def test_bilateral_against_fp64(case):
    _check('bilateral', case)


def test_guided_hard_statistics():
    """A disparity-like offset of 200 px on +-8 px of structure, eps = 1e-4, and a guide that is exactly constant left of column W // 3
    (variance 0: a = 0, q = mean p) beside a textured part; three strips."""
    B, n, H, W, r, eps = 1, 2, 70, 300, 8, 1e-4
    p, guide = pc.scene(B, n, H, W, seed=7, constant_left=True)
    I = pc.luminance(guide, torch.float32)
    assert float(I[..., :W // 3].var()) == 0.0 and float(I[..., W // 3:].var()) > 1e-3
    base = float((pc.guided_filter_fp32(p, guide, r, eps).double() - pc.guided_filter(p, guide, r, eps)).abs().max())
    bar = 2.0 * base + 2.0 * ULP200
    shifted = p + 200.0
    q64 = pc.guided_filter(shifted, guide, r, eps)
    naive = float((pc.guided_filter_fp32(shifted, guide, r, eps).double() - q64).abs().max())
    q = support.ops().guided_filter(shifted.to(DEV), guide.to(DEV), r, eps).cpu().double()
    err = float((q - q64).abs().max())
    flat = float((q - q64)[..., :W // 3 - 2 * r].abs().max())
    print('hard statistics: max |q - q64| %.3e (bar %.3e = 2 x %.3e + 2 ulp(200)); where the guide is constant %.3e; '
          'the fp32 variant on the shifted input %.3e' % (err, bar, base, flat, naive))
    assert err <= bar


# ---- 2. the same bits every time
@pytest.mark.parametrize('kind', ['guided', 'bilateral'])
def test_repeats_bit_for_bit_whatever_the_workspace_holds(kind):
    ops = support.ops()
    case = (1, 1, 70, 131, 8, 1)
    p, guide, _, _ = _case(kind, case)
    p, guide = p.to(DEV), guide.to(DEV)
    a = _run(kind, p, guide, 8)
    mine = [buf for key, buf in ops._scratch.items() if key[1] == 'postprocess']
    assert mine or kind == 'bilateral'                           # (the bilateral filter needs no scratch)
    for buf in mine:
        buf.fill_(float('nan'))
    b = _run(kind, p, guide, 8)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    if kind == 'guided':                                         # and through the ABI, on a workspace of this test's own
        from dualpixelface_amd._lib import lib
        nbytes = lib().call('dpf_guided_filter_workspace_bytes', 1, 1, 70, 131, 8)
        assert nbytes == 4 * 3 * 70 * 131 and lib().call('dpf_guided_filter_workspace_bytes', 1, 1, 5, 7, 2) == 424     # 420, 8-byte aligned
        outs = []
        for fill in (float('nan'), 1e30):
            ws = torch.full((nbytes // 4,), fill, device=DEV)
            out = torch.empty_like(p)
            lib().call('dpf_guided_filter', ptr(p), 70 * 131, ptr(guide), 1, 1, 70, 131, 8, EPS, _norm(), ptr(ws), nbytes, ptr(out),
                       stream())
            outs.append(out)
        assert torch.equal(outs[0], a) and torch.equal(outs[1], a)


# ---- 3. tile seams
@pytest.mark.parametrize('kind,off', [('guided', (3, 5)), ('guided', (3, 150)), ('bilateral', (3, 5))], ids=lambda v: str(v))
def test_embedding_in_a_larger_image_moves_the_seams_not_the_result(kind, off):
    """The 70 x 131 image alone, and at offset `off` inside a larger image of unrelated content: where the whole support of a pixel lies in
    both (the window for the bilateral filter, the window of windows, 2 r, for the guided one) the two results agree within the element-wise
    bar.  (3, 150) puts the guided kernels' strip seam at column 240 of the large image across the small one."""
    case = (1, 1, 70, 131, 8, 1)
    p, guide, _, bar = _case(kind, case)
    H, W, r = 70, 131, 8
    bp, bg = pc.scene(1, 1, H + 11, W + 160, seed=41)
    bp[..., off[0]:off[0] + H, off[1]:off[1] + W] = p
    bg[..., off[0]:off[0] + H, off[1]:off[1] + W] = guide
    small = _run(kind, p.to(DEV), guide.to(DEV), r).cpu()
    big = _run(kind, bp.to(DEV), bg.to(DEV), r).cpu()[..., off[0]:off[0] + H, off[1]:off[1] + W]
    m = 2 * r if kind == 'guided' else r
    diff = float((small[..., m:H - m, m:W - m] - big[..., m:H - m, m:W - m]).abs().max())
    outside = float((small - big).abs().max())
    print('%s at %s: inside %.3e (bar %.3e), whole image %.3e' % (kind, off, diff, bar, outside))
    assert diff <= bar and outside > bar                          # (the border does differ: the crop is not vacuous)


# ---- 4. refusals
def _norm():
    return (ctypes.c_float * 6)(0.485, 0.456, 0.406, 0.229, 0.224, 0.225)


def test_abi_refusals_launch_nothing():
    from dualpixelface_amd._lib import lib, DpfError
    B, n, H, W, r = 2, 2, 9, 12, 2
    p = torch.ones(B, n, H, W, device=DEV)
    guide = torch.zeros(B, 3, H, W, device=DEV)
    q = torch.full((B, n, H, W), -7.0, device=DEV)
    nbytes = lib().call('dpf_guided_filter_workspace_bytes', B, n, H, W, r)
    assert nbytes > 0 and nbytes % 8 == 0
    for bad in ((0, n, H, W, r), (B, 0, H, W, r), (B, n, -1, W, r), (B, n, H, 0, r), (B, n, H, W, 0), (B, n, H, W, 33), (65536, 1, H, W, r),
                (256, 256, H, W, r)):
        assert lib().call('dpf_guided_filter_workspace_bytes', *bad) == -1, bad
    assert lib().call('dpf_guided_filter_workspace_bytes', B, n, 3, 3, 32) > 0          # smaller than the window: supported
    ws = torch.full((nbytes // 4 + 2,), -7.0, device=DEV)
    good = dict(p=ptr(p), stride=n * H * W, guide=ptr(guide), B=B, n=n, H=H, W=W, r=r, eps=1e-3, ss=3.0, sc=0.1, norm=_norm(), ws=ptr(ws),
                nbytes=nbytes, q=ptr(q))

    def guided(a):
        lib().call('dpf_guided_filter', a['p'], a['stride'], a['guide'], a['B'], a['n'], a['H'], a['W'], a['r'], a['eps'], a['norm'], a['ws'],
                   a['nbytes'], a['q'], stream())

    def bilateral(a):
        lib().call('dpf_joint_bilateral_filter', a['p'], a['stride'], a['guide'], a['B'], a['n'], a['H'], a['W'], a['r'], a['ss'], a['sc'],
                   a['norm'], a['q'], stream())

    shared = [dict(p=None), dict(guide=None), dict(norm=None), dict(q=None), dict(B=0), dict(n=0), dict(H=0), dict(W=-3), dict(r=0), dict(r=-1),
              dict(stride=n * H * W - 1)]
    invalid = {guided: shared + [dict(ws=None), dict(eps=0.0), dict(eps=-1e-3), dict(eps=float('nan')), dict(eps=1e-60), dict(nbytes=nbytes - 8),
                                 dict(ws=ctypes.c_void_p(ws.data_ptr() + 4))],
               bilateral: shared + [dict(ss=0.0), dict(ss=-1.0), dict(sc=0.0), dict(sc=float('nan')), dict(sc=1e-30)]}
    unsupported = {guided: [dict(r=33), dict(B=65536, n=1), dict(B=256, n=256, stride=256 * H * W)],
                   bilateral: [dict(r=17), dict(r=32), dict(B=65536, n=1)]}
    for table, code in ((invalid, 'DPF_ERR_INVALID_ARG'), (unsupported, 'DPF_ERR_UNSUPPORTED')):
        for fn, cases in table.items():
            for over in cases:
                with pytest.raises(DpfError, match=code):
                    fn(dict(good, **over))
    torch.cuda.synchronize()
    assert bool((q == -7.0).all()) and bool((ws == -7.0).all())
    guided(good)                                                  # and the arguments they were derived from do run
    bilateral(good)
    torch.cuda.synchronize()
    assert bool((q == 1.0).all())                                 # a constant prediction is a fixed point of both


def test_ops_refuse_what_does_not_fit():
    from dualpixelface_amd._lib import DpfError
    ops = support.ops()
    p, guide = torch.zeros(1, 1, 8, 12, device=DEV), torch.zeros(1, 3, 8, 12, device=DEV)
    for bad_guide in (torch.zeros(1, 3, 8, 11, device=DEV), torch.zeros(1, 3, 16, 24, device=DEV), torch.zeros(1, 1, 8, 12, device=DEV),
                      torch.zeros(2, 3, 8, 12, device=DEV)):
        with pytest.raises(DpfError, match='does not match'):
            ops.guided_filter(p, bad_guide, 2, 1e-3)
        with pytest.raises(DpfError, match='does not match'):
            ops.joint_bilateral_filter(p, bad_guide, 2, 3.0, 0.1)
    with pytest.raises(DpfError, match='not supported'):
        ops.guided_filter(p, guide, 33, 1e-3)
    with pytest.raises(DpfError, match='DPF_ERR_UNSUPPORTED'):
        ops.joint_bilateral_filter(p, guide, 17, 3.0, 0.1)
    with pytest.raises(DpfError, match='dtype'):
        ops.guided_filter(p.double(), guide, 2, 1e-3)
    q = ops.guided_filter(p.requires_grad_(), guide, 2, 1e-3)      # detached, not an autograd node
    assert not q.requires_grad and q.grad_fn is None


# ---- 5. capture
def test_both_filters_replay_from_a_graph():
    ops = support.ops()
    case = (1, 1, 70, 131, 8, 1)
    inputs = [pc.scene(1, 1, 70, 131, seed=s) for s in (51, 52, 53)]
    eager = []
    for p, guide in inputs:
        p, guide = p.to(DEV), guide.to(DEV)
        eager.append((ops.guided_filter(p, guide, 8, EPS), ops.joint_bilateral_filter(p, guide, 5, 3.0, SIGMA_COLOR)))
    sp, sg = inputs[0][0].to(DEV).clone(), inputs[0][1].to(DEV).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                 # the side stream's scratch exists before the capture
        ops.guided_filter(sp, sg, 8, EPS)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):                    # one stream: a single chain of launches
        out_g = ops.guided_filter(sp, sg, 8, EPS)
        out_b = ops.joint_bilateral_filter(sp, sg, 5, 3.0, SIGMA_COLOR)
    for (p, guide), (want_g, want_b) in list(zip(inputs, eager))[1:]:
        sp.copy_(p.to(DEV))
        sg.copy_(guide.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_g, want_g) and torch.equal(out_b, want_b)


# ---- 6. the whole path
def _model_with_post_process(cls_name, config, **block):
    opt = support.option(config)
    for k, v in block.items():
        setattr(opt.post_process, k, v)
    return support.build(cls_name, opt)


def _switches(model, bilateral, guided):
    model.option.post_process.use_bilateral, model.option.post_process.use_guided = bilateral, guided


def _eval_path(model, step, bilateral, guided, filt):
    """Evaluation forward with the switches on against the same model with them off, then a deferred metric step on the filtered map."""
    from dualpixelface_amd import ops
    batch = support.batch(1, 64, 96, seed=9, mask_mode='bern')
    model.eval()
    with torch.no_grad(), ops.deterministic_mode():
        _switches(model, False, False)
        off = model.forward(batch)
        assert 'pred_depth_raw' not in off
        for flip in (model.option.dataset.flip_lr, not model.option.dataset.flip_lr):
            model.option.dataset.flip_lr = flip
            _switches(model, False, False)
            raw = model.forward(batch)['pred_depth']
            _switches(model, bilateral, guided)
            res = model.forward(batch)
            guide = batch['right'] if flip else batch['left']         # flip_lr unset: batch['left'], the view the network then predicts for
            assert torch.equal(res['pred_depth_raw'], raw) and not torch.equal(res['pred_depth'], raw)
            assert torch.equal(res['pred_depth'], filt(raw, guide)) and res['pred_depth'].shape == raw.shape
        model.option.dataset.flip_lr = not flip                        # as shipped
        assert torch.equal(off['pred_depth'], model.forward(dict(batch))['pred_depth_raw'])
        bank = model.metric_model
        assert bank.metric_func, 'no metric configured'
        before = [f.index for f in bank.metric_func]
        with bank.deferred():
            res = step(batch, 0)
        bank.flush()
        for f, i0 in zip(bank.metric_func, before):
            assert f.index == i0 + 1
            want = f.measure_device(res, batch, log=False, target_type=model._target_type()).cpu().tolist()
            raw_row = f.measure_device(dict(res, pred_depth=res['pred_depth_raw']), batch, log=False, target_type=model._target_type()).cpu().tolist()
            got = f.get_value(i0)
            print(type(f).__name__, 'filtered', got, 'raw', raw_row)
            assert np.array_equal(np.asarray(got), np.asarray(want), equal_nan=True)
            if 'depth' in type(f).__name__ or 'absolute' in type(f).__name__ or 'affine' in type(f).__name__:
                assert not np.array_equal(np.asarray(got), np.asarray(raw_row), equal_nan=True)
    return batch


def test_stereodpnet_guided_config_end_to_end():
    from dualpixelface_amd import ops
    model = _model_with_post_process('STEREODPNET', 'eval_faceDP_guided')
    assert model.option.post_process.use_guided and model.option.dataset.flip_lr
    batch = _eval_path(model, model.validation_step, False, True, lambda raw, guide: ops.guided_filter(raw, guide, 8, 1e-3))
    # training mode: nothing is filtered and no key appears, whatever the block says
    with ops.deterministic_mode():
        model.train()
        _switches(model, True, True)
        on = model.forward(batch)
        _switches(model, False, False)
        off = model.forward(batch)
    assert 'pred_depth_raw' not in on and set(on) == set(off)
    assert torch.equal(on['pred_depth'], off['pred_depth']) and on['pred_depth'].requires_grad


def test_dpnet_bilateral_end_to_end():
    from dualpixelface_amd import ops
    model = _model_with_post_process('DPNET', 'eval_faceDP_dpnet', use_bilateral=True)
    _eval_path(model, model.test_step, True, False, lambda raw, guide: ops.joint_bilateral_filter(raw, guide, 5, 3.0, 0.1))


def test_both_switches_run_bilateral_then_guided_and_a_missing_prediction_is_named():
    from dualpixelface_amd import ops, postprocess
    batch = support.batch(1, 64, 96, seed=9, mask_mode='bern')
    p = (batch['disp'].unsqueeze(1) * 3.0).contiguous()

    class Opt(object):
        post_process = {'use_bilateral': True, 'use_guided': True, 'guided_radius': 4, 'bilateral_radius': 2}
    res = postprocess.apply(Opt(), {'pred_depth': p}, batch)
    want = ops.guided_filter(ops.joint_bilateral_filter(p, batch['left'], 2, 3.0, 0.1), batch['left'], 4, 1e-3)
    assert torch.equal(res['pred_depth'], want) and res['pred_depth_raw'].data_ptr() == p.data_ptr()
    other = postprocess.apply(Opt(), {'pred_depth': p}, batch, guide=batch['right'])
    assert not torch.equal(other['pred_depth'], want)
    with pytest.raises(NotImplementedError, match='pred_depth'):
        postprocess.apply(Opt(), {'pred_normal': p}, batch)


def _main_rows(config, workspace):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, 'main.py', '--config', config, '--workspace', workspace, '--synthetic', '8', '--height', '64', '--width', '96'],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    import ast
    rows = ast.literal_eval([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    assert rows and all(np.isfinite(v) for row in rows.values() for v in row), rows
    return rows


def test_main_runs_the_guided_config_to_the_metric_table():
    """main.py seeds the weights and the synthetic samples, so eval_faceDP and eval_faceDP_guided differ in the filter alone: the depth rows
    of the table move, the normal rows (nothing filters pred_normal) stay."""
    off = _main_rows('eval_faceDP', 'pytest_unfiltered')
    on = _main_rows('eval_faceDP_guided', 'pytest_guided')
    print('eval_faceDP', off, '\neval_faceDP_guided', on)
    assert set(on) == set(off) and 'absolute_dp' in on
    assert abs(on['absolute_dp'][0] - off['absolute_dp'][0]) > 1e-3 * abs(off['absolute_dp'][0])       # abs_rel
    assert on['affine_dp'] != off['affine_dp']
    assert np.allclose(on['normal_dp'], off['normal_dp'], rtol=1e-5, atol=0.0)
