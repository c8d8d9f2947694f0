#!/usr/bin/env python3
"""Gradient accumulation and global-norm clipping: the kernels of csrc/grad_ctl.hip at the StereoDPNet arena size, and the captured
StereoDPNet train step with the knobs off, with clipping on and under accumulation.

    python tools/grad_ctl_bench.py [--n 3670492] [--reps 200] [--rounds 5] [--step_shape 2,256,384] [--step_reps 30] [--step_rounds 5]
                                   [--parent PATH] [--parent_rounds 3] [--copy_tbs 5.9] [--out profiles/grad_ctl_timings.txt]

Kernels: each launch form is warmed up and `reps` launches of it are captured into one HIP graph on a stream of its own; a replay is timed
between two events and divided by `reps`, the forms alternate for `rounds` rounds and the median is reported with min and max.  (Launched
one by one from Python the same forms take the 8 - 10 us of an enqueue, which is also reported: the kernels are shorter than that.)
Bytes are what the algorithm moves: fold reads two arenas and writes one (12 n), the sums of squares read one (4 n), Adam reads four
and writes three (28 n), RMSprop and SGD read three and write two (20 n).  The rate is
quoted against --copy_tbs, the 1-read-1-write streaming rate profiles/r04_stream_probe.txt records for this card; a 14.7 MB arena fits the
last-level cache, so a rate above it is not an error.  A graph still leaves a gap between two kernels, so a time is an upper bound of
the kernel's own.
Step: plugin.STEREODPNET.train_step on one synthetic batch, wall clock around a synchronised run of `step_reps` graph replays, the
configurations alternating; under accumulation a call is a micro-step, so the figure is per micro-step (every fourth runs the optimiser).
--parent PATH: a built checkout of the parent commit; its knobs-off step is timed in fresh child processes alternating with this build's,
`parent_rounds` each, which gives the parent's own run-to-run spread.  Needs a GPU; there is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

import bench_support
from bench_support import fmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {'off': {}, 'clip': {'gradient_clip_val': 1.0}, 'accum4': {'accumulate_grad_batches': 4}, 'accum4_clip': {'accumulate_grad_batches': 4, 'gradient_clip_val': 1.0}}


def kernel_lines(n, reps, rounds, copy_tbs):
    from dualpixelface_amd import ops
    g = torch.Generator().manual_seed(1)
    p, grad, m, v, acc = (torch.randn(n, generator=g).mul_(1e-2).cuda() for _ in range(5))
    v.abs_()
    ctl = torch.zeros(ops.GRAD_CTL_FLOATS, device='cuda')
    ctl[:2] = torch.tensor([float(x) for x in ops.adam_hyper(10, 1e-6)])
    ctl[3] = 1.0                                           # apply; first stays 0: the fold adds
    forms = [('fold (acc += g)', 12, lambda: ops.grad_fold(acc, grad, ctl)),
             ('fold + sums of squares, one pass', 12, lambda: ops.grad_fold(acc, grad, ctl, partials=True)),
             ('sums of squares alone', 4, lambda: ops.grad_sumsq(grad)),
             ('finish (one workgroup)', 0, lambda: ops.grad_finish(n, ctl, 1.0, 1e-3)),
             ('Adam behind the record (clipped)', 28, lambda: ops.adam_step_ctl(p, grad, m, v, ctl)),
             ('Adam, gscale as an argument', 28, lambda: ops.adam_step(p, grad, m, v, 10, 1e-6)),
             ('RMSprop behind the record (clipped)', 20, lambda: ops.rmsprop_step_ctl(p, grad, v, ctl)),
             ('RMSprop, gscale as an argument', 20, lambda: ops.rmsprop_step(p, grad, v, 1e-6))]
    acc.mul_(0.0)
    side = torch.cuda.Stream()
    graphs = []
    for _, _, fn in forms:
        bench_support.timed(fn, 5)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()                                           # (the scratch of this stream exists before the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            for _ in range(reps):
                fn()
        graphs.append(graph)
    times, eager = [[] for _ in forms], [[] for _ in forms]
    for _ in range(rounds):
        for t, e, graph, (_, _, fn) in zip(times, eager, graphs, forms):
            acc.mul_(0.0)
            graph.replay()
            t.append(bench_support.timed(graph.replay, 1) / reps)
            e.append(bench_support.timed(fn, reps))
    torch.cuda.synchronize()
    out = []
    for t, e, (name, per, _) in zip(times, eager, forms):
        med = statistics.median(t)
        rate = per * n / (med * 1e-3) / 1e12
        out.append('%-38s %s%s | one by one from Python %.4f ms' % (name, fmt(t, 4), ' | %5.1f MB = %.2f TB/s = %3.0f %% of the %.1f TB/s copy rate'
                                                                    % (per * n / 1e6, rate, 100 * rate / copy_tbs, copy_tbs) if per else '',
                                                                    statistics.median(e)))
    return out


def step_models(names, shape):
    from dualpixelface_amd import load_option
    from dualpixelface_amd.plugin import STEREODPNET
    from dualpixelface_amd.recipe import fill_by_recipe, synthetic_batch
    B, H, W = shape
    batch = {k: v.cuda() for k, v in synthetic_batch(B, H, W, seed=7, mask_mode='bern').items()}
    models = []
    for name in names:
        opt = load_option()
        for k, v in CONFIGS[name].items():
            setattr(opt, k, v)
        model = STEREODPNET(opt)
        fill_by_recipe(model)
        model = model.cuda().train()
        for _ in range(8):                                  # state creation, warm-up steps, the graph capture; ends on a group boundary
            model.train_step(batch, None, lr=1e-6)
        models.append(model)
    return models, batch


def step_round(model, batch, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        model.train_step(batch, None, lr=1e-6)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def child(args):
    """One configuration in this process (the package comes from --root): a JSON line with its rounds."""
    models, batch = step_models([args.child], tuple(int(v) for v in args.step_shape.split(',')))
    print(json.dumps({'ms': [step_round(models[0], batch, args.step_reps) for _ in range(args.step_rounds)]}), flush=True)


def spawn(root, args):
    cmd = [sys.executable, os.path.abspath(__file__), '--child', 'off', '--root', root, '--step_shape', args.step_shape, '--step_reps',
           str(args.step_reps), '--step_rounds', str(args.step_rounds)]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=240, check=True).stdout.decode()
    return statistics.median(json.loads([l for l in out.splitlines() if l.startswith('{')][-1])['ms'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=3670492)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--step_shape', default='2,256,384')
    ap.add_argument('--step_reps', type=int, default=30)
    ap.add_argument('--step_rounds', type=int, default=5)
    ap.add_argument('--parent', default=None)
    ap.add_argument('--parent_rounds', type=int, default=3)
    ap.add_argument('--copy_tbs', type=float, default=5.9)
    ap.add_argument('--child', default=None)
    ap.add_argument('--root', default=ROOT)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'grad_ctl_timings.txt'))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    assert torch.cuda.is_available(), 'grad_ctl_bench needs an MI355X'
    if args.child:
        return child(args)
    import hashlib
    from dualpixelface_amd import _lib
    digest = hashlib.sha256(open(_lib.LIB_PATH, 'rb').read()).hexdigest()[:16]
    lines = ['Gradient accumulation and clipping: python tools/grad_ctl_bench.py --n %d --reps %d --rounds %d --step_shape %s --step_reps %d '
             '--step_rounds %d%s' % (args.n, args.reps, args.rounds, args.step_shape, args.step_reps, args.step_rounds,
                                     ' --parent <built parent checkout> --parent_rounds %d' % args.parent_rounds if args.parent else ''),
             'One MI355X (gfx950, %s), one process per table.  libdpf_hip.so sha256 %s.  torch %s.'
             % (torch.cuda.get_device_name(0), digest, torch.__version__),
             '', 'Kernels over an arena of %d floats, %d launches per captured graph, one replay between two events, forms alternating, median of %d rounds (min, max):'
             % (args.n, args.reps, args.rounds)]
    lines += kernel_lines(args.n, args.reps, args.rounds, args.copy_tbs)
    print('\n'.join(lines), flush=True)
    shape = tuple(int(v) for v in args.step_shape.split(','))
    names = ['off', 'clip', 'accum4', 'accum4_clip']
    models, batch = step_models(names, shape)
    times = {k: [] for k in names}
    for _ in range(args.step_rounds):
        for name, model in zip(names, models):
            times[name].append(step_round(model, batch, args.step_reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    more = ['', 'STEREODPNET train_step, synthetic batch %dx%dx%d, graph replays, %d calls per round, configurations alternating, median of %d rounds:'
            % (shape + (args.step_reps, args.step_rounds))]
    for k, label in (('off', 'knobs off'), ('clip', 'gradient_clip_val 1.0'), ('accum4', 'accumulate_grad_batches 4, per micro-step'),
                     ('accum4_clip', 'accumulate_grad_batches 4 + clip 1.0, per micro-step')):
        more.append('%-56s %s' % (label, fmt(times[k], 4)))
    more += ['(b) clipping on - off: %+.4f ms = %+.2f %% of the step' % (med['clip'] - med['off'], 100 * (med['clip'] - med['off']) / med['off']),
             '(c) N = 4 - N = 1 per micro-step: %+.4f ms = %+.2f %%' % (med['accum4'] - med['off'], 100 * (med['accum4'] - med['off']) / med['off'])]
    print('\n'.join(more), flush=True)
    lines += more
    del models
    torch.cuda.empty_cache()
    if args.parent:
        ours, theirs = [], []
        for _ in range(args.parent_rounds):
            theirs.append(spawn(args.parent, args))
            ours.append(spawn(ROOT, args))
        mo, mt = statistics.median(ours), statistics.median(theirs)
        lines += ['', '(a) knobs off, fresh processes alternating (each the median of %d rounds of %d replays): parent commit %s | this build %s'
                  % (args.step_rounds, args.step_reps, fmt(theirs, 4), fmt(ours, 4)),
                  '    this build - parent: %+.4f ms = %+.2f %%; the parent\'s own run-to-run spread (max - min): %.4f ms = %.2f %%'
                  % (mo - mt, 100 * (mo - mt) / mt, max(theirs) - min(theirs), 100 * (max(theirs) - min(theirs)) / mt)]
    else:
        lines += ['', '(a) knobs off against the parent commit: not measured (no --parent)']
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
