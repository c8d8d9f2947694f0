#!/usr/bin/env python3
"""Timing of the DPNet plugin and of the kernel families it adds, on one MI355X.

    python tools/dpnet_bench.py [--steps 20] [--warmup 5] [--repeats 5] [--no-graph] [--skip-model] [--out profiles/dpnet_bench.json]

Method: warm-up launches first, HIP events around a batch of launches, a device synchronisation before the events are read; every
figure is the median of ``--repeats`` such measurements and is reported with their min / max (the run-to-run spread a ratio has to beat).
  * model: train samples/s of DPNET.train_step at 2 x 1024 x 1536 (the reference config's batch) and 4 x 512 x 768, as a HIP graph and
    with --no-graph semantics (eager launches);
  * kernels: ms per launch and GB/s of algorithmic bytes for max-pool forward / backward, the general depthwise window and the 7x7
    convolution forward / data gradient / weight gradient at DPNet's largest shapes, each beside the same operator of torch-ROCm
    (F.max_pool2d, F.conv2d(groups=C), F.conv2d 7x7) timed in the same process.  ratio = torch ms / this build's ms (> 1: faster).
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

import bench_support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = 'cuda'


def median_min_max(fn, warmup, iters, repeats):
    """-> (median, min, max) ms per call."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    vals = sorted(bench_support.timed(fn, iters) for _ in range(repeats))
    return vals[len(vals) // 2], vals[0], vals[-1]


def row(name, mine, ref, nbytes):
    r = {'name': name, 'ms': mine[0], 'ms_min': mine[1], 'ms_max': mine[2], 'gbps': nbytes / mine[0] * 1e-6,
         'torch_ms': ref[0], 'torch_ms_min': ref[1], 'torch_ms_max': ref[2], 'ratio_torch_over_ours': ref[0] / mine[0]}
    print(json.dumps(r))
    return r


def kernel_rows(args):
    from dualpixelface_amd import ops
    rows = []
    t = lambda f: median_min_max(f, args.warmup, args.steps, args.repeats)
    g = torch.Generator(device=DEV).manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    # max-pool: Encoder2's pool of the raw input (k7 s2 p1) and the largest encoder skip (11 channels, k3 s1, 512 x 768)
    for name, shape, (k, s, p) in (('maxpool k7s2p1 2x6x1024x1536', (2, 6, 1024, 1536), (7, 2, 1)),
                                   ('maxpool k3s1p0 2x11x512x768', (2, 11, 512, 768), (3, 1, 0)),
                                   ('maxpool k3s2p0 2x32x510x766', (2, 32, 510, 766), (3, 2, 0))):
        x = rn(*shape).requires_grad_()
        y = ops.max_pool2d(x, k, s, p)
        go = torch.randn_like(y)
        yr = F.max_pool2d(x, k, s, p)
        rows.append(row(name + ' fwd', t(lambda: ops.max_pool2d(x.detach(), k, s, p)), t(lambda: F.max_pool2d(x.detach(), k, s, p)),
                        4.0 * x.numel() + 8.0 * y.numel()))
        rows.append(row(name + ' bwd', t(lambda: torch.autograd.grad(y, x, go, retain_graph=True)),
                        t(lambda: torch.autograd.grad(yr, x, go, retain_graph=True)), 8.0 * y.numel() + 4.0 * x.numel()))
    # depthwise, general window: skip_layer1 (11 channels, k3 pad 3, 510 x 766) and a decoder k1 pad 1
    for name, shape, (k, p) in (('depthwise k3p3 2x11x510x766', (2, 11, 510, 766), (3, 3)), ('depthwise k3p0 2x16x516x772', (2, 16, 516, 772), (3, 0)),
                                ('depthwise k1p1 2x16x514x770', (2, 16, 514, 770), (1, 1))):
        C = shape[1]
        x, w = rn(*shape).requires_grad_(), rn(C, 1, k, k).requires_grad_()
        y, yr = ops.depthwise_conv2d(x, w, p), F.conv2d(x, w, None, 1, p, 1, C)
        go = torch.randn_like(y)
        rows.append(row(name + ' fwd', t(lambda: ops.depthwise_conv2d(x.detach(), w.detach(), p)),
                        t(lambda: F.conv2d(x.detach(), w.detach(), None, 1, p, 1, C)), 4.0 * (x.numel() + y.numel())))
        rows.append(row(name + ' dgrad+wgrad', t(lambda: torch.autograd.grad(y, (x, w), go, retain_graph=True)),
                        t(lambda: torch.autograd.grad(yr, (x, w), go, retain_graph=True)), 4.0 * (3 * y.numel() + 2 * x.numel())))
    # 7x7: the stem (6 -> 8, stride 2) and the two largest heads
    for name, shape, K, (s, p) in (('conv7x7 stem 6->8 s2 2x1024x1536', (2, 6, 1024, 1536), 8, (2, 1)),
                                   ('conv7x7 head1 8->1 2x1028x1540', (2, 8, 1028, 1540), 1, (1, 1)),
                                   ('conv7x7 head2 32->1 2x516x772', (2, 32, 516, 772), 1, (1, 1))):
        C = shape[1]
        x, w = rn(*shape).requires_grad_(), (rn(K, C, 7, 7) * 0.05).requires_grad_()
        y, yr = ops.conv2d(x, w, None, s, p), F.conv2d(x, w, None, s, p)
        go = torch.randn_like(y)
        rows.append(row(name + ' fwd', t(lambda: ops.conv2d(x.detach(), w.detach(), None, s, p)), t(lambda: F.conv2d(x.detach(), w.detach(), None, s, p)),
                        4.0 * (x.numel() + y.numel())))
        rows.append(row(name + ' dgrad', t(lambda: torch.autograd.grad(y, x, go, retain_graph=True)),
                        t(lambda: torch.autograd.grad(yr, x, go, retain_graph=True)), 4.0 * (x.numel() + y.numel())))
        rows.append(row(name + ' wgrad', t(lambda: torch.autograd.grad(y, w, go, retain_graph=True)),
                        t(lambda: torch.autograd.grad(yr, w, go, retain_graph=True)), 4.0 * (x.numel() + y.numel())))
    return rows


def model_rows(args):
    from dualpixelface_amd import load_option
    from dualpixelface_amd.plugin import DPNET
    from dualpixelface_amd.recipe import fill_by_recipe, synthetic_batch
    rows = []
    for B, H, W in ((2, 1024, 1536), (4, 512, 768)):
        for graph in ((False,) if args.no_graph else (True, False)):
            os.environ['DPF_STEP_GRAPH'] = '1' if graph else '0'
            opt = load_option('train_faceDP_dpnet')
            model = DPNET(opt)
            fill_by_recipe(model)
            model.to(DEV).train()
            batch = {k: v.to(DEV) for k, v in synthetic_batch(B, H, W, seed=1, mask_mode='bern').items()}
            ms = median_min_max(lambda: model.train_step(batch, None, lr=1e-4), max(args.warmup, 4), args.steps, args.repeats)
            r = {'name': 'DPNET train_step %dx%dx%d %s' % (B, H, W, 'graph' if graph else 'eager'), 'ms': ms[0], 'ms_min': ms[1], 'ms_max': ms[2],
                 'samples_per_s': B / ms[0] * 1e3}
            print(json.dumps(r))
            rows.append(r)
            del model
    os.environ.pop('DPF_STEP_GRAPH', None)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--no-graph', action='store_true')
    ap.add_argument('--skip-model', action='store_true')
    ap.add_argument('--skip-kernels', action='store_true')
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    out = {'device': torch.cuda.get_device_name(0), 'steps': args.steps, 'warmup': args.warmup, 'repeats': args.repeats}
    if not args.skip_kernels:
        out['kernels'] = kernel_rows(args)
    if not args.skip_model:
        out['model'] = model_rows(args)
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
