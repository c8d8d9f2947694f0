"""Deferred metric mode and all-rank validation without a GPU: on CPU tensors the deferred rows come from metrics.py's torch functions,
so everything around the kernels -- row buffers, flush, Trainer.validate, the cross-rank reduction -- is checked here."""
import os
import subprocess
import sys

import pytest
import torch

from dualpixelface_amd import metrics as M
from dualpixelface_amd.config import load_option
from dualpixelface_amd.selectors import metric_selector
from dualpixelface_amd.trainer import Trainer
from tests import device_metrics_fixture as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_deferred_rows_wait_for_flush_and_equal_the_direct_rows():
    sel, ref = metric_selector(load_option()), metric_selector(load_option())
    cases = [fx.make_case(2, 8, 12, 'bern', seed=s) for s in range(3)]
    with sel.deferred():
        for pred_, batch in cases:
            out = sel.forward(pred_, batch)
            assert all(torch.is_tensor(r) and r.dtype == torch.float64 for r in out.values())
        quiet = sel.forward(*cases[0], log=False)                       # log=False: a row comes back, nothing is queued
    assert set(quiet) == set(sel.metric_name)
    assert all(f.index == 0 and f.pending_rows().shape == (3, len(f.keys)) for f in sel.metric_func)
    for pred_, batch in cases:
        direct = ref.forward(pred_, batch)
    assert [float(v) for v in out['absolute_dp']] == direct['absolute_dp']          # same torch functions on CPU tensors: same figures
    sel.flush()
    for f, g in zip(sel.metric_func, ref.metric_func):
        assert f.index == g.index == 3 and f.metric == g.metric and f.pending_rows() is None
        assert f.get_value() == g.get_value() and f.get_value(1) == g.get_value(1)
    sel.viewer()
    sel.flush()                                                                      # nothing queued: a no-op
    assert sel.metric_func[0].index == 3
    for f in sel.metric_func:
        f.clear()
    assert all(f.index == 0 and f.metric == {k: [] for k in f.keys} for f in sel.metric_func)
    assert sel.forward(*cases[0])['normal_dp'] == ref.forward(*cases[0], log=False)['normal_dp']   # outside the context: python floats again


def test_row_buffer_grows_in_chunks_and_honours_samplenum():
    bench = M.normal_dp_Benchmark(load_option())
    rows = [torch.tensor([float(i), float(-i)], dtype=torch.float64) for i in range(2 * M.ROW_CHUNK + 5)]
    for r in rows:
        bench.update_device(r)
    assert bench._rows.shape[0] == 3 * M.ROW_CHUNK and bench.index == 0
    bench.take_pending(bench.pending_rows())
    assert bench.index == len(rows) and bench.metric['n_err_mean'] == [float(i) for i in range(len(rows))]
    assert bench.metric['n_err_rmse'][7] == -7.0
    capped = M.normal_dp_Benchmark(load_option(), samplenum=3)
    capped.update([9.0, 9.0])                                           # one row logged directly, two more fit
    for r in rows[:6]:
        capped.update_device(r)
    assert capped.pending_rows().shape[0] == 2
    capped.take_pending(capped.pending_rows())
    capped.update_device(rows[0])
    assert capped.index == 3 and capped.pending_rows() is None and capped.metric['n_err_mean'] == [9.0, 0.0, 1.0]
    with pytest.raises(ValueError):
        bench.update_device(torch.zeros(3, dtype=torch.float64))
    pending = M.normal_dp_Benchmark(load_option())
    pending.update_device(rows[1])
    pending.clear()                                                     # clear() drops queued rows too
    assert pending.pending_rows() is None


def test_device_metrics_switch_is_read_per_call(monkeypatch):
    monkeypatch.setenv('DPF_DEVICE_METRICS', '0')
    assert not M.device_metrics_enabled()
    monkeypatch.delenv('DPF_DEVICE_METRICS')
    assert M.device_metrics_enabled()


def test_validate_runs_deferred_flushes_once_and_keeps_its_record():
    model = fx.StubModel()
    loader = fx.stub_loader(3, H=8, W=12)
    sel = model.metric_model
    calls = {'flush': 0, 'deferred': []}
    real_flush, real_forward = sel.flush, sel.forward

    def flush():
        calls['flush'] += 1
        return real_flush()

    def forward(*a, **k):
        calls['deferred'].append(sel._deferred)
        return real_forward(*a, **k)
    sel.flush, sel.forward = flush, forward
    tr = Trainer(load_option(), '.', rank=0, world_size=1)
    rows = tr.validate(model, loader)
    assert calls == {'flush': 1, 'deferred': [True] * 3} and tr.validated_batches == [0, 1, 2] and model.seen == [0, 1, 2]
    ref = metric_selector(load_option())
    for b in loader:
        ref.forward(b, b)
    assert rows == {n: f.get_value() for n, f in zip(ref.metric_name, ref.metric_func)}
    assert all(f.index == 0 for f in sel.metric_func) and model.training            # cleared, back in train mode
    assert not sel._deferred


def _rank_worker(rank, world, port, nbatches, share, out):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    counts = {'all_reduce': 0}
    real = dist.all_reduce

    def counted(*a, **k):
        counts['all_reduce'] += 1
        return real(*a, **k)
    dist.all_reduce = counted
    opt = load_option()
    if not share:
        opt.validate_on_all_ranks = False
    model = fx.StubModel(opt)
    tr = Trainer(opt, '.', rank=rank, world_size=world)
    rows = tr.validate(model, fx.stub_loader(nbatches, H=8, W=12)) if (share or rank == 0) else None
    dist.all_reduce = real
    dist.barrier()
    out[rank] = (rows, list(model.seen), counts['all_reduce'])
    dist.destroy_process_group()


def _single_process_rows(nbatches):
    return Trainer(load_option(), '.', rank=0, world_size=1).validate(fx.StubModel(), fx.stub_loader(nbatches, H=8, W=12))


@pytest.mark.parametrize('nbatches', [3, 1])
def test_two_gloo_ranks_share_validation_and_reproduce_the_single_process_mean(nbatches):
    import torch.multiprocessing as mp
    out = mp.Manager().dict()
    mp.spawn(_rank_worker, args=(2, 36500 + os.getpid() % 2000 + nbatches, nbatches, True, out), nprocs=2, join=True)
    (rows0, seen0, n0), (rows1, seen1, n1) = out[0], out[1]
    assert seen0 == list(range(0, nbatches, 2)) and seen1 == list(range(1, nbatches, 2))     # 1 batch: rank 1 has none and adds zeros
    assert n0 == n1 == 3                                                                      # one collective per benchmark on every rank
    assert rows0 == rows1
    single = _single_process_rows(nbatches)
    assert set(rows0) == set(single)
    for name in single:
        for a, b in zip(rows0[name], single[name]):
            assert abs(a - b) <= 1e-12 * abs(b), (name, a, b)                                 # the same rows in another summation order


def test_validate_on_all_ranks_false_keeps_rank0_only_validation():
    import torch.multiprocessing as mp
    out = mp.Manager().dict()
    mp.spawn(_rank_worker, args=(2, 38500 + os.getpid() % 2000, 3, False, out), nprocs=2, join=True)
    (rows0, seen0, n0), (rows1, seen1, n1) = out[0], out[1]
    assert seen0 == [0, 1, 2] and seen1 == [] and rows1 is None and n0 == n1 == 0
    assert rows0 == _single_process_rows(3)
    opt = load_option()
    assert Trainer(opt, '.', rank=1, world_size=2).validates_on_all_ranks()                   # the default
    assert not Trainer(opt, '.', rank=0, world_size=1).validates_on_all_ranks()


def test_sort_plan_replay_under_host_sanitizers(tmp_path):
    """tools/metrics_plan_check.cpp: the rank sort's histogram / scan / scatter replayed on the CPU with the kernels' own plan header,
    inside a heap block of exactly the queried workspace size, under the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path / 'metrics_plan_check')
    subprocess.check_call(['c++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-I' + os.path.join(ROOT, 'dualpixelface_amd', 'csrc'), os.path.join(ROOT, 'tools', 'metrics_plan_check.cpp'), '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and 'metrics plan check: ok' in r.stdout, r.stdout[-2000:]
