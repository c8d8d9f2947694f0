"""Normal-guided depth refinement on the GPU (run with ``-m gpu``): csrc/normal_refine.hip through ops.normal_refine, through the plugins'
evaluation forward and through main.py, against the numpy restatement of tests/normal_refine_cpu.py.

Bars.  The counts the edge flags give (valid pixels, edges) equal the restatement exactly; the scenes keep every comparison at least 1e-4
relative from its threshold in fp64 (asserted per case).  delta, read off the refined plane as log(depth out / depth in), against the fp64
restatement: max |delta - delta64| <= 2 x (the fp32 restatement's own worst deviation, read off its plane the same way) + 1e-7, a floor
below the fp32 spacing of an 800 mm depth in log units.  Pixels that are not valid and heads other than head 0 equal the input bit for bit.
Measured on an MI355X: DESIGN.md section 7.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import normal_refine_cpu as nr
from tests import support
from tests.support import DEV, ptr, stream

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(max_edge_ratio=nr.RATIO, min_cos=nr.MIN_COS, lam=nr.LAM, iterations=nr.ITERATIONS)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _operands(ref):
    sc = ref['sc']
    ab = None if sc['target_type'] == 'depth' else _dev(sc['ab'])
    return (_dev(sc['pred']), _dev(sc['K']), _dev(sc['normal'])), dict(KW, ab=ab, mask=_dev(sc['mask']), target_type=sc['target_type'])


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- 1. against the restatement
@pytest.mark.parametrize('case', nr.CASES, ids=nr.case_id)
def test_against_the_restatement(case):
    ref = nr.case(case)
    assert ref['margin'] >= 1e-4 and ref['agree']
    sc, r64 = ref['sc'], ref['r64']
    args, kw = _operands(ref)
    out, stats = support.ops().normal_refine(*args, stats=True, **kw)
    assert out.shape == args[0].shape and out.dtype == torch.float32 and stats.shape == (case[0], 3 + nr.ITERATIONS)
    assert stats.dtype == torch.float64
    got, st = out.cpu().numpy(), stats.cpu().numpy()
    assert np.array_equal(st[:, :2], r64['stats'][:, :2]), (st[:, :2], r64['stats'][:, :2])
    valid = r64['sy']['valid']
    assert np.array_equal(support.bits(got[:, 0])[~valid], support.bits(sc['pred'][:, 0])[~valid])      # untouched pixels, NaN and all
    assert np.array_equal(support.bits(got[:, 1:]), support.bits(sc['pred'][:, 1:]))                    # untouched heads
    assert np.isfinite(got[:, 0][valid]).all() and np.isfinite(st).all()
    delta = nr.recovered_delta(got[:, 0], np.ascontiguousarray(sc['pred'][:, 0]), sc['target_type'], sc['ab'], valid)
    own = float(np.abs(ref['d32'] - ref['d64']).max())
    err = float(np.abs(delta - ref['d64']).max())
    bar = 2.0 * own + 1e-7
    rho = float(np.abs(st[:, 2] - r64['stats'][:, 2]).max() / max(r64['stats'][:, 2].max(), 1e-300))
    print('normal_refine %s: max |delta - delta64| %.3e (bar %.3e = 2 x %.3e + 1e-7), max |delta64| %.3e, counts %s, rho_0 off by %.1e '
          'relative, rho_%d %s' % (nr.case_id(case), err, bar, own, np.abs(ref['d64']).max(), st[:, :2].tolist(), rho, nr.ITERATIONS,
                                   st[:, -1].tolist()))
    assert err <= bar
    # (rho_0 sums fp32 mismatches whose own rounding is some 1e-7 relative)
    assert rho <= 1e-4


def test_plane_is_a_fixed_point_and_the_noisy_sphere_is_smoothed():
    ops = support.ops()
    sc, n = nr.plane()
    out = ops.normal_refine(_dev(sc['pred']).unsqueeze(1), _dev(sc['K']), _dev(n), target_type='depth')
    rel = float((out[:, 0].double() / _dev(sc['pred']).double() - 1).abs().max())
    sc, n, z_true = nr.noisy_sphere(24, 40, seed=0)
    out2 = ops.normal_refine(_dev(sc['pred']).unsqueeze(1), _dev(sc['K']), _dev(n), target_type='depth')
    before = float(np.sqrt(np.mean((sc['pred'].astype(np.float64) - z_true) ** 2)))
    after = float(np.sqrt(np.mean((out2[:, 0].cpu().numpy().astype(np.float64) - z_true) ** 2)))
    print('plane: max |out / in - 1| %.3e (bar 2^-22); noisy sphere: RMSE %.4f -> %.4f mm (x %.3f)' % (rel, before, after, after / before))
    assert rel <= 2.0 ** -22                         # |delta| <= 2^-23 (test_normal_refine_host.py) and one rounding of the product
    assert after <= 0.25 * before


# ---- 2. independent samples, the same bits every time
def test_a_sample_does_not_depend_on_the_rest_of_the_batch():
    ops = support.ops()
    ref = nr.case(nr.CASES[1])
    (pred, K, normal), kw = _operands(ref)
    both, stats = ops.normal_refine(pred, K, normal, stats=True, **kw)
    for b in range(2):
        one = dict(kw, ab=kw['ab'][b:b + 1], mask=kw['mask'][b:b + 1])
        alone, stats1 = ops.normal_refine(pred[b:b + 1], K[b:b + 1], normal[b:b + 1], stats=True, **one)
        assert _same_bits(alone, both[b:b + 1]) and _same_bits(stats1, stats[b:b + 1]), b
    assert not torch.equal(both[0, 0], pred[0, 0])


def test_repeats_bit_for_bit_whatever_the_workspace_holds():
    ops = support.ops()
    ref = nr.case(nr.CASES[3])
    args, kw = _operands(ref)
    first = ops.normal_refine(*args, stats=True, **kw)
    mine = [buf for key, buf in ops._scratch.items() if key[1] == 'normal_refine']
    assert mine
    for fill in (float('nan'), 1e30):
        for buf in mine:
            buf.fill_(fill)
        again = ops.normal_refine(*args, stats=True, **kw)
        assert _same_bits(first[0], again[0]) and _same_bits(first[1], again[1])
    into = torch.full_like(args[0], -7.0)
    assert ops.normal_refine(*args, out=into, **kw) is into and _same_bits(into, first[0])


def test_call_replays_from_a_graph():
    ops = support.ops()
    ref = nr.case(nr.CASES[1])
    (pred, K, normal), kw = _operands(ref)
    eager = ops.normal_refine(pred, K, normal, stats=True, **kw)
    sp, sn = pred.clone(), normal.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                 # the side stream's scratch exists before the capture
        ops.normal_refine(sp, K, sn, **kw)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out, stats = ops.normal_refine(sp, K, sn, stats=True, **kw)
    other_p, other_n = (pred * 1.001).contiguous(), normal.flip(0).contiguous()
    want = ops.normal_refine(other_p, K, other_n, stats=True, **kw)
    assert not torch.equal(want[1], eager[1])
    for (p, n), w in (((other_p, other_n), want), ((pred, normal), eager)):
        sp.copy_(p)
        sn.copy_(n)
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(out, w[0]) and _same_bits(stats, w[1])


# ---- 3. refusals
def test_abi_refusals_launch_nothing():
    from dualpixelface_amd._lib import lib, DpfError
    B, H, W, it = 2, 9, 12, 4
    pred = torch.full((B, H, W), 800.0, device=DEV)
    ab = torch.tensor([[0.0, 1.0]] * B, device=DEV)
    K = torch.tensor([[100.0, 0.0, 6.0], [0.0, 100.0, 4.5], [0.0, 0.0, 1.0]], device=DEV).repeat(B, 1, 1).contiguous()
    mask = torch.ones(B, H, W, device=DEV)
    normal = torch.zeros(B, 3, H, W, device=DEV)
    normal[:, 2] = -1.0
    out = torch.full((B, H, W), -7.0, device=DEV)
    stats = torch.full((B, 3 + it), -7.0, dtype=torch.float64, device=DEV)
    query = 'dpf_normal_refine_workspace_bytes'
    nbytes = lib().call(query, B, H, W)
    tiles, HWp = 1 * 2, 108
    assert nbytes == ((3 * B * tiles + 2 * B) * 8 + B * HWp * 29 + 15) // 16 * 16 == 6400       # 6392 -> 6400: rounded up to 16 bytes
    assert lib().call(query, 1, 5, 7) == ((3 + 2 + 1) * 8 + 36 * 29 + 15) // 16 * 16
    for bad in ((0, H, W), (B, 0, W), (B, H, -1), (65536, H, W), (1, 65536, 32768), (1, 8 * 65535 + 1, 1)):
        assert lib().call(query, *bad) == -1, bad
    ws = torch.full((nbytes // 4 + 4,), -7.0, device=DEV)
    signs = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    good = dict(pred=ptr(pred), pstride=H * W, tt=2, ab=ptr(ab), K=ptr(K), mask=ptr(mask), normal=ptr(normal), signs=signs, B=B, H=H, W=W,
                near=0.0, far=float('inf'), ratio=0.01, min_cos=0.1, lam=0.1, it=it, ws=ptr(ws), nbytes=nbytes, out=ptr(out), ostride=H * W,
                stats=ptr(stats))

    def run(a):
        lib().call('dpf_normal_refine', a['pred'], a['pstride'], a['tt'], a['ab'], a['K'], a['mask'], a['normal'], a['signs'], a['B'], a['H'],
                   a['W'], a['near'], a['far'], a['ratio'], a['min_cos'], a['lam'], a['it'], a['ws'], a['nbytes'], a['out'], a['ostride'],
                   a['stats'], stream())

    invalid = [dict(pred=None), dict(K=None), dict(normal=None), dict(signs=None), dict(out=None), dict(ws=None), dict(tt=0, ab=None),
               dict(tt=1, ab=None), dict(B=0), dict(H=0), dict(W=-3), dict(tt=3), dict(tt=-1), dict(pstride=H * W - 1), dict(ostride=H * W - 1),
               dict(near=-1.0), dict(near=float('nan')), dict(far=0.0), dict(far=float('nan')), dict(near=5.0, far=5.0), dict(ratio=0.0),
               dict(ratio=float('nan')), dict(lam=0.0), dict(lam=-0.1), dict(lam=float('nan')), dict(lam=float('inf')), dict(it=0), dict(it=-1),
               dict(min_cos=-0.01), dict(min_cos=1.0), dict(min_cos=float('nan')), dict(signs=(ctypes.c_float * 3)(1.0, 0.0, 1.0)),
               dict(signs=(ctypes.c_float * 3)(1.0, 1.0, 2.0)), dict(nbytes=nbytes - 16), dict(ws=ctypes.c_void_p(ws.data_ptr() + 8))]
    unsupported = [dict(it=257), dict(B=65536)]
    for cases, code in ((invalid, 'DPF_ERR_INVALID_ARG'), (unsupported, 'DPF_ERR_UNSUPPORTED')):
        for over in cases:
            with pytest.raises(DpfError, match=code):
                run(dict(good, **over))
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((stats == -7.0).all()) and bool((ws == -7.0).all())
    run(good)                                                         # and the arguments they were derived from do run
    run(dict(good, mask=None, stats=None, ab=None))                   # the optional operands
    torch.cuda.synchronize()
    # a fronto-parallel plane under normals along the axis: every edge exists and nothing has to move
    assert stats[:, :2].cpu().tolist() == [[H * W, (H - 1) * W + H * (W - 1)]] * B
    assert float((out / 800.0 - 1.0).abs().max()) <= 2.0 ** -22 and bool((ws[-4:] == -7.0).all())


def test_ops_refuse_what_does_not_fit():
    from dualpixelface_amd._lib import DpfError
    ops = support.ops()
    pred, K, ab = torch.ones(2, 1, 8, 12, device=DEV), torch.eye(3, device=DEV).repeat(2, 1, 1), torch.ones(2, 2, device=DEV)
    normal = torch.zeros(2, 3, 8, 12, device=DEV)
    for kw in (dict(Kmat=K[:1]), dict(ab=ab[:1]), dict(mask=torch.ones(2, 8, 11, device=DEV)), dict(ab=None), dict(normal=normal[:, :2]),
               dict(normal=normal[:, :, :4])):
        args = dict(dict(Kmat=K, ab=ab, normal=normal), **kw)
        with pytest.raises(DpfError, match='does not match|needs ab'):
            ops.normal_refine(pred, **args)
    with pytest.raises(DpfError, match='dtype'):
        ops.normal_refine(pred.double(), K, normal, ab=ab)
    with pytest.raises(DpfError, match='out'):
        ops.normal_refine(pred, K, normal, ab=ab, out=torch.empty(2, 1, 8, 11, device=DEV))
    with pytest.raises(DpfError, match='DPF_ERR_INVALID_ARG'):
        ops.normal_refine(pred, K, normal, ab=ab, near=3.0, far=2.0)
    out = ops.normal_refine(pred.requires_grad_(), K, normal, ab=ab)   # detached, not an autograd node
    assert not out.requires_grad and out.grad_fn is None


# ---- 4. the whole path
def _model(cls_name, config, refine=None, **blocks):
    from dualpixelface_amd.config import Option
    opt = support.option(config)
    if refine is not None:
        opt.normal_refine = Option(dict(refine))
    for name, block in blocks.items():
        setattr(opt, name, Option(dict(block)))
    return support.build(cls_name, opt)


def _equal_results(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k] is None and b[k] is None or _same_bits(a[k], b[k]), k


def test_stereodpnet_evaluation_refines_before_the_surface():
    from dualpixelface_amd import normal_refine, ops
    model = _model('STEREODPNET', 'eval_faceDP', reconstruct=dict(enabled=True))
    batch = support.batch(1, 32, 48, seed=9, mask_mode='bern')
    model.eval()
    with torch.no_grad(), ops.deterministic_mode():
        absent = model.forward(dict(batch))                              # no normal_refine block at all: today's result
        assert not hasattr(model.option, 'normal_refine')
        from dualpixelface_amd.config import Option
        model.option.normal_refine = Option(dict(enabled=False, iterations=8))
        off = model.forward(dict(batch))
        _equal_results(off, absent)
        model.option.normal_refine = Option(dict(enabled=True))
        on = model.forward(dict(batch))
        assert set(on) == set(off) | set(normal_refine.RESULT_KEYS) and not set(off) & set(normal_refine.RESULT_KEYS)
        assert _same_bits(on['pred_depth_unrefined'], off['pred_depth'])
        for k in off:
            if k not in ('pred_depth', 'points', 'points_valid', 'normal_geo', 'normal_geo_valid'):
                assert off[k] is None and on[k] is None or _same_bits(off[k], on[k]), k
        want, stats = ops.normal_refine(off['pred_depth'], batch['K'], on['pred_normal'][:, 0], ab=batch['abvalue'], mask=batch['mask'], stats=True)
        assert _same_bits(on['pred_depth'], want) and _same_bits(on['refine_stats'], stats)
        assert _same_bits(on['pred_depth'][:, 1:], off['pred_depth'][:, 1:]) and not torch.equal(on['pred_depth'][:, 0], off['pred_depth'][:, 0])
        row = stats[0].cpu().tolist()
        print('stereodpnet 1x32x48: %d valid pixels, %d edges, rho %.3e -> %.3e' % (row[0], row[1], row[2], row[-1]))
        assert row[1] > 0
        # reconstruct places the refined map
        points, pvalid = ops.backproject(on['pred_depth'], batch['K'], ab=batch['abvalue'], mask=batch['mask'])
        assert torch.equal(on['points'], points) and torch.equal(on['points_valid'], pvalid) and not torch.equal(points, off['points'])
    # training mode: nothing is refined, whatever the block says
    with ops.deterministic_mode():
        model.train()
        res = model.forward(dict(batch))
    assert not set(res) & set(normal_refine.RESULT_KEYS) and res['pred_depth'].requires_grad


def test_a_model_without_a_normal_head_refines_with_the_batch_normals_only():
    """At 1 x 32 x 64: DPNet's decoders meet their skips only at some sizes (dpnet.dpnet_shapes) and 32 x 48 is not one; there the forward
    refuses the size before it launches anything."""
    from dualpixelface_amd import ops
    model = _model('DPNET', 'eval_faceDP_dpnet', refine=dict(enabled=True))
    batch = support.batch(1, 32, 64, seed=9, mask_mode='bern')
    model.eval()
    with torch.no_grad(), ops.deterministic_mode():
        with pytest.raises(ValueError, match='multiples of 16'):
            model.forward(dict(support.batch(1, 32, 48, seed=9, mask_mode='bern')))
        with pytest.raises(NotImplementedError, match='pred_normal'):
            model.forward(dict(batch))
        model.option.normal_refine.normals = 'batch'
        res = model.forward(dict(batch))
        want = ops.normal_refine(res['pred_depth_unrefined'], batch['K'], batch['normal'], ab=batch['abvalue'], mask=batch['mask'],
                                 target_type=model._target_type())
        assert res.get('pred_normal') is None and _same_bits(res['pred_depth'], want)
        assert res['refine_stats'].shape == (1, 35) and bool(torch.isfinite(res['refine_stats']).all())


def test_main_evaluates_the_refine_config():
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, 'main.py', '--config', 'eval_faceDP_refine', '--workspace', 'pytest_refine', '--synthetic', '4', '--height',
                        '64', '--width', '96'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    for name in ('absolute_dp', 'affine_dp', 'normal_dp'):
        assert name in r.stdout, r.stdout[-2000:]
