"""Validation-metric timings: metric_selector.forward per family (torch path against the kernels of csrc/metrics.hip, alternating in one
process) and a whole Trainer.validate loop (torch path / device path of this tree, optionally another checkout's trainer and library).

  python tools/metrics_bench.py                       every step below as a child process with its own time limit; stops at the first
                                                      step that fails or runs out of time
  python tools/metrics_bench.py --parent-root DIR     ... and the validate loop of the checkout at DIR (e.g. the parent commit, built)
                                                      alternating with this tree's, three runs each
  python tools/metrics_bench.py --step families --shape 4,1024,1536      one step in this process

Times are wall-clock around a device synchronisation.  The torch path of `families` is metric_selector.forward as it is called outside
deferred mode (host waits included: that is its cost), the device path is the deferred forward plus its share of one flush."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--step', choices=['all', 'families', 'validate'], default='all')
ap.add_argument('--shape', default='4,1024,1536')
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--batches', type=int, default=4, help='batches of the validate loop')
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help='tree to import the package from')
ap.add_argument('--parent-root', default=None)
ap.add_argument('--device-metrics', default=None, help='validate step: 0 / 1 (a tree without the switch ignores it)')
ap.add_argument('--limit', type=int, default=420, help='seconds per child step')
args = ap.parse_args()
args.root = os.path.abspath(args.root)
args.parent_root = os.path.abspath(args.parent_root) if args.parent_root else None


def span(v):
    return '%.3f ms (min %.3f, max %.3f, n=%d)' % (statistics.median(v), min(v), max(v), len(v))


def families():
    sys.path.insert(0, args.root)
    import torch
    from dualpixelface_amd.config import load_option
    from dualpixelface_amd.recipe import synthetic_batch
    from dualpixelface_amd.selectors import metric_selector
    B, H, W = [int(v) for v in args.shape.split(',')]
    batch = synthetic_batch(B, H, W, seed=1, mask_mode='bern', device='cuda')
    g = torch.Generator(device='cuda').manual_seed(3)
    pred = {'pred_depth': (batch['disp'] + 0.05 * torch.randn(B, H, W, device='cuda', generator=g)).unsqueeze(1),
            'pred_normal': batch['normal'].unsqueeze(1) + 0.1 * torch.randn(B, 1, 3, H, W, device='cuda', generator=g)}
    opt = load_option()
    for name in ('absolute_dp', 'normal_dp', 'affine_dp', 'all'):
        opt.model.metric_type = ['absolute_dp', 'affine_dp', 'normal_dp'] if name == 'all' else [name]
        sel = metric_selector(opt)
        times = {'torch': [], 'device': []}
        for rep in range(args.reps + 1):                      # the first repetition warms both paths up
            for path in ('torch', 'device'):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if path == 'torch':
                    sel.forward(pred, batch)
                else:
                    with sel.deferred():
                        sel.forward(pred, batch)
                    sel.flush()
                torch.cuda.synchronize()
                if rep:
                    times[path].append(1e3 * (time.perf_counter() - t0))
            for f in sel.metric_func:
                f.clear()
        print('families %s %-11s torch %s | device %s' % (args.shape, name, span(times['torch']), span(times['device'])), flush=True)


def validate():
    if args.device_metrics is not None:
        os.environ['DPF_DEVICE_METRICS'] = args.device_metrics
    sys.path.insert(0, args.root)
    os.chdir(args.root)
    import torch
    from dualpixelface_amd import load_option
    from dualpixelface_amd.plugin import STEREODPNET
    from dualpixelface_amd.recipe import fill_by_recipe, synthetic_batch
    from dualpixelface_amd.trainer import Trainer
    B, H, W = [int(v) for v in args.shape.split(',')]
    opt = load_option()
    model = STEREODPNET(opt)
    fill_by_recipe(model)
    model.to('cuda')
    loader = [synthetic_batch(B, H, W, seed=20 + i, mask_mode='bern', device='cuda') for i in range(args.batches)]
    tr = Trainer(opt, '.', rank=0, world_size=1)
    whole, forward = [], []
    for rep in range(args.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = tr.validate(model, loader)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        model.eval()
        with torch.no_grad():
            for b in loader:                                   # the same forward without the metric hooks
                model.forward(b)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        model.train()
        if rep:
            whole.append(1e3 * (t1 - t0) / len(loader))
            forward.append(1e3 * (t2 - t1) / len(loader))
    w, f = statistics.median(whole), statistics.median(forward)
    print('validate %s root=%s DPF_DEVICE_METRICS=%s: per batch %s | forward alone %s | metrics share %.1f %%'
          % (args.shape, os.path.basename(os.path.abspath(args.root)), os.environ.get('DPF_DEVICE_METRICS', 'unset'), span(whole), span(forward),
             100.0 * (w - f) / w), flush=True)
    print('validate rows ' + json.dumps({k: [round(v, 6) for v in r] for k, r in rows.items()}), flush=True)


def child(extra):
    cmd = [sys.executable, os.path.abspath(__file__)] + extra
    try:
        rc = subprocess.run(cmd, timeout=args.limit).returncode          # a fresh process and a time limit per GPU step
    except subprocess.TimeoutExpired:
        rc = 124
    if rc != 0:
        print('step %s ended with %d: stopping' % (' '.join(extra), rc), flush=True)
        sys.exit(rc if rc > 0 else 1)


if args.step == 'families':
    families()
elif args.step == 'validate':
    validate()
else:
    for shape in ('2,256,384', '4,1024,1536'):
        child(['--step', 'families', '--shape', shape, '--reps', str(args.reps)])
    for shape in ('2,256,384', '4,1024,1536'):
        for run in range(3 if shape == '4,1024,1536' else 1):      # alternating; three runs per side at the headline size
            for dm in ('0', '1'):
                child(['--step', 'validate', '--shape', shape, '--reps', '3', '--batches', str(args.batches), '--device-metrics', dm])
            if args.parent_root:
                child(['--step', 'validate', '--shape', shape, '--reps', '3', '--batches', str(args.batches), '--root', args.parent_root])
