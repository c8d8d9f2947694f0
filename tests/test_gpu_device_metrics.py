"""Validation metrics on the device (``-m gpu``): the kernels of csrc/metrics.hip against metrics.py, the deferred selector mode and
Trainer.validate on top of them.

Error yardstick of every floating-point comparison: T = metrics.py on the CPU with float64 inputs, F = metrics.py on the float32
inputs (the incumbent path), kernel result K: |K - T| <= 2 |F - T| + 1e-6 |T|.

The rank tests come first, smallest length first: everything after them that touches affine_dp consumes ranks."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import device_metrics_fixture as fx
from tests import support

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'

RANK_LENGTHS = (2, 63, 64, 65, 255, 256, 257, 4097, 70001)
RANK_SETS = ('seven_values', 'all_equal', 'sorted', 'reversed', 'special')


def _rank_values(n, kind):
    """[2, n] fp32, the two rows of different content."""
    g = torch.Generator().manual_seed(n * 31 + len(kind))
    if kind == 'seven_values':
        return torch.stack([torch.randint(0, 7, (n,), generator=g).float() - 3.0, torch.randint(0, 7, (n,), generator=g).float() * 0.5])
    if kind == 'all_equal':
        return torch.stack([torch.full((n,), 2.5), torch.full((n,), -1.0)])
    if kind == 'sorted':
        return torch.stack([torch.arange(n, dtype=torch.float32), torch.linspace(-5.0, 3.0, n)])
    if kind == 'reversed':
        return torch.stack([torch.arange(n, dtype=torch.float32).flip(0), -torch.linspace(-5.0, 3.0, n)])
    rows = []
    den = float(np.finfo(np.float32).smallest_subnormal)
    special = [0.0, -0.0, den, -den, float('inf'), float('-inf'), 0.0, -0.0, 3 * den, -3 * den]
    for r in range(2):
        v = torch.randn(n, generator=g) * (10.0 if r else 1e-3)
        perm = torch.randperm(n, generator=g)
        for k, s in enumerate(special[r:]):
            if k + 1 < n:
                v[perm[k + 1]] = s
        v[perm[0]] = float('nan')
        rows.append(v)
    return torch.stack(rows)


def _torch_ranks(z):
    return torch.stack([torch.argsort(torch.argsort(row, stable=True), stable=True) for row in z]).to(torch.int32)


@pytest.mark.parametrize('n,kind', [(n, k) for n in RANK_LENGTHS for k in RANK_SETS])
def test_ranks_equal_double_stable_argsort(n, kind):
    from dualpixelface_amd import ops
    z = _rank_values(n, kind)
    got = ops.metric_ranks(z.to(DEV)).cpu()
    got_neg = ops.metric_ranks(z.to(DEV), negate=True).cpu()
    assert torch.equal(got, _torch_ranks(z))
    assert torch.equal(got_neg, _torch_ranks(-z))


# ------------------------------------------------------------------------------------------------------------------ refusals
def _raw(name, *args):
    from dualpixelface_amd._lib import lib
    return getattr(lib().cdll, name)(*args)


def test_refusals_launch_nothing():
    from dualpixelface_amd._lib import lib
    L, _p = lib(), support.ptr
    B, n = 2, 300
    x = torch.rand(B, n, device=DEV) + 1.0
    x3 = torch.rand(B, 3, n, device=DEV)
    ab = torch.tensor([[32.98, -26996.49]] * B, device=DEV)
    ri = torch.zeros(B, n, dtype=torch.int32, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.float32, device=DEV)
    big = ws.numel() * 4
    canary = torch.full((8,), 7.25, device=DEV)
    ranks = torch.full((B, n), -5, dtype=torch.int32, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    INVALID, UNSUPPORTED = -1, -3
    need = {k: L.call('dpf_metric_%s_workspace_bytes' % k, B, n) for k in ('absolute_dp', 'normal_dp', 'ranks', 'affine_dp')}
    assert all(0 < v <= big for v in need.values())

    def absolute(pred=x, abv=ab, tgt=x, B_=B, n_=n, out=canary, w=ws, wb=big, tt=0):
        return _raw('dpf_metric_absolute_dp', _p(pred), _p(abv), _p(tgt), None, B_, n_, tt, 1.01, _p(out), _p(w), wb, st)

    def normal(pred=x3, tgt=x3, B_=B, n_=n, out=canary, w=ws, wb=big):
        return _raw('dpf_metric_normal_dp', _p(pred), _p(tgt), None, B_, n_, _p(out), _p(w), wb, st)

    def rank(v=x, out=ranks, B_=B, n_=n, w=ws, wb=big):
        return _raw('dpf_metric_ranks', _p(v), _p(out), B_, n_, 0, _p(w), wb, st)

    def affine(pred=x, r=ri, B_=B, n_=n, out=canary, w=ws, wb=big, iters=5):
        return _raw('dpf_metric_affine_dp', _p(pred), _p(x), _p(x), _p(r), _p(ri), _p(ri), B_, n_, iters, 1e-3, _p(out), _p(w), wb, st)

    codes = [
        absolute(pred=None), absolute(tgt=None), absolute(out=None), absolute(abv=None), absolute(B_=0), absolute(B_=-1), absolute(n_=0),
        absolute(w=None), absolute(wb=need['absolute_dp'] - 1), absolute(tt=3),
        normal(pred=None), normal(tgt=None), normal(out=None), normal(B_=0), normal(w=None), normal(wb=need['normal_dp'] - 1),
        rank(v=None), rank(out=None), rank(B_=0), rank(n_=0), rank(w=None), rank(wb=need['ranks'] - 1),
        affine(pred=None), affine(r=None), affine(out=None), affine(B_=0), affine(w=None), affine(wb=need['affine_dp'] - 1), affine(iters=0),
    ]
    assert codes == [INVALID] * len(codes), codes
    too_long = 2 ** 31 - 1                                   # indices stay 32-bit: refused before anything is touched
    assert [absolute(n_=too_long), normal(n_=too_long), rank(n_=too_long), affine(n_=too_long), rank(B_=70000)] == [UNSUPPORTED] * 5
    assert L.call('dpf_metric_ranks_workspace_bytes', 1, too_long) == -1 and L.call('dpf_metric_ranks_workspace_bytes', 1, too_long - 1) > 0
    torch.cuda.synchronize()
    assert torch.equal(canary.cpu(), torch.full((8,), 7.25)) and torch.equal(ranks.cpu(), torch.full((B, n), -5, dtype=torch.int32))
    assert absolute() == 0 and rank() == 0                  # the same arguments, nothing withheld: accepted
    torch.cuda.synchronize()
    assert not torch.equal(canary.cpu(), torch.full((8,), 7.25)) and int(ranks.min()) == 0


# ------------------------------------------------------------------------------------------------------- the three families
@functools.lru_cache(maxsize=None)
def _metrics_case(shape, mask):
    pred_, batch = fx.make_case(*shape, mask=mask, seed=sum(shape))
    return pred_, batch, fx.reference_rows(pred_, batch)


def _device_rows(pred_, batch, target_type='disp'):
    from dualpixelface_amd.config import load_option
    from dualpixelface_amd.selectors import metric_selector
    sel = metric_selector(load_option())
    with sel.deferred():
        out = sel.forward(fx.cast(pred_, device=DEV), fx.cast(batch, device=DEV), log=False, target_type=target_type)
    return {n: r.cpu().tolist() for n, r in out.items()}


@pytest.mark.parametrize('mask', fx.MASKS)
@pytest.mark.parametrize('shape', fx.SHAPES)
def test_families_within_the_yardstick(shape, mask):
    pred_, batch, ref = _metrics_case(shape, mask)
    rows = _device_rows(pred_, batch)
    for name in ('absolute_dp', 'normal_dp', 'affine_dp'):
        T, F = ref[name]
        fx.assert_yardstick(rows[name], T, F, '%s %s %s' % (name, shape, mask))
    if mask == 'all_masked':
        assert all(np.isnan(v) for v in rows['absolute_dp'] + rows['normal_dp'] + rows['affine_dp'])
    else:
        # the threshold fractions compare the same fp32 ratio with the same fp32 constants: equal to torch's fp32 result, not just close
        np.testing.assert_array_equal(rows['absolute_dp'][5:], ref['absolute_dp'][1][5:])


def test_fold_of_more_rows_than_threads():
    """B = 2 at 512 x 512: 256 partial rows per sample, 512 in the one fold of absolute_dp and of normal_dp, so every fold thread adds two
    rows (fx.SHAPES fold <= 9).  affine_dp folds per sample and never exceeds 256 rows; it stays out to keep the CPU side short."""
    from dualpixelface_amd.config import load_option
    from dualpixelface_amd.selectors import metric_selector
    pred_, batch = fx.make_case(2, 512, 512, 'bern', seed=11)
    opt = load_option()
    opt.model.metric_type = ['absolute_dp', 'normal_dp']
    T = metric_selector(opt).forward(fx.cast(pred_, torch.float64), fx.cast(batch, torch.float64), log=False)
    F = metric_selector(opt).forward(pred_, batch, log=False)
    sel = metric_selector(opt)
    with sel.deferred():
        out = sel.forward(fx.cast(pred_, device=DEV), fx.cast(batch, device=DEV), log=False)
    rows = {n: r.cpu().tolist() for n, r in out.items()}
    for name in ('absolute_dp', 'normal_dp'):
        fx.assert_yardstick(rows[name], T[name], F[name], '%s 512 rows' % name)
    np.testing.assert_array_equal(rows['absolute_dp'][5:], F['absolute_dp'][5:])


@pytest.mark.parametrize('target_type', ['idepth', 'depth'])
def test_other_target_types_select_the_same_inputs(target_type):
    pred_, batch = fx.make_case(2, 16, 24, 'bern', seed=3)
    if target_type == 'depth':                               # the prediction is a depth already
        from dualpixelface_amd import metrics as M
        pred_ = dict(pred_, pred_depth=M.disp2depth(pred_['pred_depth'], batch['abvalue']))
    else:
        batch['idepth'] = batch['disp'] * 0.5 + 3.0          # affine_dp's target under 'idepth'
    from dualpixelface_amd.config import load_option
    from dualpixelface_amd.selectors import metric_selector
    sel = metric_selector(load_option())
    T = sel.forward(fx.cast(pred_, torch.float64), fx.cast(batch, torch.float64), log=False, target_type=target_type)
    F = sel.forward(pred_, batch, log=False, target_type=target_type)
    rows = _device_rows(pred_, batch, target_type)
    for name in sel.metric_name:
        fx.assert_yardstick(rows[name], T[name], F[name], '%s %s' % (name, target_type))


def test_disparity_equal_to_b_gives_depth_zero_like_torch():
    pred_, batch = fx.make_case(2, 16, 24, 'ones', seed=5)
    b = float(batch['abvalue'][0, 0])
    pred_['pred_depth'][0, 0, 3, 4] = b                      # a / 0 = inf -> 0
    pred_['pred_depth'][1, 0, 0, 0] = float('nan')           # NaN -> 0
    ref = fx.reference_rows(pred_, batch)
    rows = _device_rows(pred_, batch)
    T, F = ref['absolute_dp']
    for k, t, f in zip(rows['absolute_dp'], T, F):           # pred = 0: the ratio terms are inf in torch and here
        assert (np.isinf(t) and np.isinf(k) and np.isinf(f)) or (np.isnan(t) and np.isnan(k)) or abs(k - t) <= 2 * abs(f - t) + 1e-6 * abs(t), (k, t, f)
    assert rows['absolute_dp'][5:] == F[5:]
    assert np.isinf(rows['absolute_dp'][4]) and np.isfinite(rows['absolute_dp'][0])


def test_golden_arrays_meet_the_bar_of_test_metrics(golden_dir):
    from dualpixelface_amd import ops
    gold = np.load(os.path.join(golden_dir, 'metrics.npz'))
    gt, pred, mask = (torch.from_numpy(gold[k]).float() for k in ('gt', 'pred', 'mask'))
    B = gt.shape[0] if gt.dim() == 3 else 1
    out = ops.metric_absolute_dp(pred.reshape(B, -1).to(DEV), None, gt.reshape(B, -1).to(DEV), mask.reshape(B, -1).to(DEV), 'depth', 1.01)
    np.testing.assert_allclose(out.cpu().numpy(), gold['abs_out'], rtol=2e-5)
    gn, pn = torch.from_numpy(gold['gn']).float(), torch.from_numpy(gold['pn']).float()
    out = ops.metric_normal_dp(gn.contiguous().to(DEV), pn.contiguous().to(DEV), mask.reshape(gn.shape[0], -1).to(DEV))
    np.testing.assert_allclose(out.cpu().numpy(), gold['normal_out'], rtol=2e-5)


def _affine_row(x, y, w):
    from dualpixelface_amd import ops
    x, y, w = (t.reshape(1, -1).to(DEV) for t in (x, y, w))
    return ops.metric_affine_dp(x, y, w, ops.metric_ranks(x), ops.metric_ranks(x, negate=True), ops.metric_ranks(y)).cpu().tolist()


def test_affine_dp_closed_forms_on_the_device():
    g = torch.Generator().manual_seed(3)
    x = torch.rand(40, 50, generator=g)
    w = torch.rand(40, 50, generator=g) + 0.1
    for sign in (1.0, -1.0):                                 # the maximum over both rank directions
        wmae, wrmse, spear = _affine_row(x, sign * (2.5 * x - 0.7), w)
        assert wmae <= 1e-5 and wrmse <= 1e-5 and abs(spear) <= 1e-9, (wmae, wrmse, spear)
    # a constant prediction with weights on a 1/8 grid: every moment is exact, det = 0 exactly -> s = 0, t = the weighted mean of the
    # target (the determinant branch), so wrmse is the weighted standard deviation of the target.  The later IRLS fits of a constant
    # prediction divide rounding noise by rounding noise in metrics.py itself (its float64 and float32 figures differ by 1e-2), so wmae is
    # not compared; the ranks of a constant are its indices (ties keep index order), so the Spearman term is an ordinary figure.
    from dualpixelface_amd import metrics as M
    y = torch.rand(40, 50, generator=g)
    w8 = torch.randint(1, 17, (40, 50), generator=g).float() / 8.0
    c = torch.full((40, 50), 0.75)
    T = M.affine_metrics(c[None].double(), y[None].double(), w8[None].double())
    F = M.affine_metrics(c[None], y[None], w8[None])
    K = _affine_row(c, y, w8)
    fx.assert_yardstick(K[1:], T[1:], F[1:], 'constant prediction wrmse, spearman')
    yd, wd = y.double(), w8.double()
    mean = (wd * yd).sum() / wd.sum()
    assert abs(K[1] - float(torch.sqrt((wd * (yd - mean) ** 2).sum() / wd.sum()))) <= 1e-6


def test_ten_calls_return_identical_bits():
    from dualpixelface_amd import ops
    pred_, batch = fx.make_case(3, 33, 65, 'weights', seed=9)
    p = pred_['pred_depth'][:, 0].contiguous().to(DEV)
    d, m, ab = batch['depth'].to(DEV), batch['mask'].to(DEV), batch['abvalue'].to(DEV)
    pn, tn = pred_['pred_normal'][:, 0].contiguous().to(DEV), batch['normal'].to(DEV)
    flat = p.view(3, -1)
    tgt, conf = batch['disp'].to(DEV).view(3, -1), batch['conf'].to(DEV).view(3, -1)

    def once():
        r = [ops.metric_ranks(flat), ops.metric_ranks(flat, negate=True), ops.metric_ranks(tgt)]
        return [ops.metric_absolute_dp(p, ab, d, m), ops.metric_normal_dp(pn, tn, m), ops.metric_affine_dp(flat, tgt, conf, *r)] + r
    first = [t.clone() for t in once()]
    for _ in range(9):
        again = once()
        for a, b in zip(first, again):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))       # bits, not values


# ---------------------------------------------------------------------------------------------------- selector and trainer
def test_deferred_forward_never_waits_on_the_host():
    from dualpixelface_amd.config import load_option
    from dualpixelface_amd.selectors import metric_selector
    pred_, batch, ref = _metrics_case((2, 16, 24), 'bern')
    pred_d, batch_d = fx.cast(pred_, device=DEV), fx.cast(batch, device=DEV)
    sel = metric_selector(load_option())
    with sel.deferred():
        sel.forward(pred_d, batch_d, log=False)              # first call: library load, scratch allocation
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')
        try:
            out = sel.forward(pred_d, batch_d)
        finally:
            torch.cuda.set_sync_debug_mode('default')
    assert all(r.is_cuda for r in out.values()) and all(f.index == 0 for f in sel.metric_func)
    sel.flush()
    assert all(f.index == 1 for f in sel.metric_func)
    for name, f in zip(sel.metric_name, sel.metric_func):     # F: the non-deferred forward() of the same inputs
        T, F = ref[name]
        fx.assert_yardstick(f.get_value(0), T, F, 'deferred ' + name)
    for f in sel.metric_func:
        f.clear()
    assert all(f.index == 0 for f in sel.metric_func)


_VALIDATE_CHILD = '''
import json, sys
sys.path.insert(0, %r)
import torch
from dualpixelface_amd.config import load_option
from dualpixelface_amd.trainer import Trainer
from tests import device_metrics_fixture as fx
model = fx.StubModel().to('cuda')
tr = Trainer(load_option(), '.', rank=0, world_size=1)
rows = tr.validate(model, fx.stub_loader(3))
again = tr.validate(model, fx.stub_loader(3))
print(json.dumps({'rows': rows, 'again': again, 'index': [f.index for f in model.metric_model.metric_func], 'seen': model.seen}))
'''


def _validate_child(device_metrics):
    env = dict(os.environ, DPF_DEVICE_METRICS=device_metrics)
    r = subprocess.run([sys.executable, '-c', _VALIDATE_CHILD % ROOT], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-800:], r.stderr[-1500:])
    return json.loads(lines[0])


def test_trainer_validate_device_rows_track_the_torch_rows():
    torch_path, device_path = _validate_child('0'), _validate_child('1')
    # truth: the per-batch float64 rows averaged over the batches like the trainer's record; incumbent: the torch path's record
    refs = [fx.reference_rows({k: b[k] for k in ('pred_depth', 'pred_normal')}, b) for b in fx.stub_loader(3)]
    for name in ('absolute_dp', 'affine_dp', 'normal_dp'):
        T = np.mean([r[name][0] for r in refs], axis=0)
        fx.assert_yardstick(device_path['rows'][name], T, torch_path['rows'][name], 'validate ' + name)
    for run in (torch_path, device_path):
        assert run['again'] == run['rows'] and run['index'] == [0, 0, 0] and run['seen'] == [0, 1, 2, 0, 1, 2]   # clear() between passes


def _rank_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0')
    import torch.distributed as dist
    from dualpixelface_amd.config import load_option
    from dualpixelface_amd.distributed import init_from_env
    from dualpixelface_amd.trainer import Trainer
    torch.cuda.set_device(0)
    init_from_env('gloo')
    model = fx.StubModel().to('cuda')
    tr = Trainer(load_option(), '.', rank=rank, world_size=world)
    rows = tr.validate(model, fx.stub_loader(3))
    torch.cuda.synchronize()
    out[rank] = (rows, list(model.seen))
    dist.destroy_process_group()


def test_two_ranks_validate_their_own_batches_and_agree_with_one_process():
    import torch.multiprocessing as mp
    from dualpixelface_amd.config import load_option
    from dualpixelface_amd.trainer import Trainer
    out = mp.Manager().dict()
    mp.spawn(_rank_worker, args=(2, 35500 + (os.getpid() % 2000), out), nprocs=2, join=True)
    (rows0, seen0), (rows1, seen1) = out[0], out[1]
    assert seen0 == [0, 2] and seen1 == [1] and rows0 == rows1
    single = Trainer(load_option(), '.', rank=0, world_size=1).validate(fx.StubModel().to(DEV), fx.stub_loader(3))
    for name in single:
        np.testing.assert_allclose(rows0[name], single[name], rtol=1e-6, atol=0)
