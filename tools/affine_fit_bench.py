#!/usr/bin/env python3
"""The fitted ('least_square') disparity conversion: ops.affine_fit alone, with the loss forward + backward behind it, against the same number of
reweighting steps written in torch on the GPU, and the DPNet train step with and without it.

    python tools/affine_fit_bench.py [--shapes 4,1,1024,1536:4,5,1024,1536] [--reps 20] [--rounds 3] [--step_shape 2,256,384]
                                     [--step_reps 10] [--out profiles/affine_fit_timings.txt]

Inputs: depth uniform in [700, 1500] with 15 % zeros, pred = a / depth + b + noise per head; "clean" has noise 0.05, "heavy" noise 0.3 and
20 % of the pixels moved by uniform [-15, 15].  "fit" is one ops.affine_fit call with the default cap and tolerance (1 + max_iters pass /
fold launch pairs and a closing pair, whatever the data); "fit+loss" adds ops.depth_loss(target_ab=...) forward and backward.  "torch" runs
as many reweighting steps as the slowest sample of the hip fit used, as fp64 tensor expressions on the same device (boolean-mask indexing
once, then sums), without a stopping test.  Each side is warmed up, then `reps` calls are timed between two events on one stream; the sides
alternate for `rounds` rounds and the median is reported with min and max.  A hip call is about a hundred short launches enqueued from
Python, so its time is an upper bound of the device time.  Bandwidth: a pass reads head 0 and idepth once (8 bytes per pixel) and a stopped
sample's passes read nothing, so the algorithmic traffic is 8 bytes x sum over the samples of (2 + iterations used) x H W, over the fit time.
The train step is plugin.DPNET.train_step under train_faceDP_dpnet on one synthetic batch as it comes ('given': the batch's abvalue and
disparity) and on the same batch without 'abvalue' and 'disp' (fitted), alternating.  Needs a GPU; there is no CPU fallback.
"""
import argparse
import os
import statistics
import sys
import time

import torch

import bench_support
from bench_support import fmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

A0, B0 = -26996.49, 63.0
WEIGHTS = [1.0, 0.7, 0.5, 0.4, 0.3]


def fields(B, n, H, W, sigma, frac, seed):
    g = torch.Generator().manual_seed(seed)
    depth = (torch.rand(B, H, W, generator=g) * 800.0 + 700.0) * (torch.rand(B, H, W, generator=g) >= 0.15).float()
    idepth = torch.where(depth > 0, 1.0 / torch.where(depth > 0, depth, torch.ones_like(depth)), torch.zeros_like(depth))
    pred = A0 * idepth.unsqueeze(1) + B0 + sigma * torch.randn(B, n, H, W, generator=g)
    pred = pred + (torch.rand(B, n, H, W, generator=g) < frac).float() * (torch.rand(B, n, H, W, generator=g) * 30.0 - 15.0)
    return pred.cuda(), idepth.cuda(), depth.cuda()


def torch_fit(pred, idepth, steps, f=0.1):
    out = []
    for i in range(pred.shape[0]):
        x, y = idepth[i].reshape(-1), pred[i, 0].reshape(-1)
        keep = x > 0
        x, y = x[keep].double(), y[keep].double()
        w = torch.ones_like(x)
        for it in range(steps + 1):
            if it:
                w = torch.rsqrt(1.0 + ((A * x + B - y) / f) ** 2)
            sw, sx, sy, sxx, sxy = w.sum(), (w * x).sum(), (w * y).sum(), (w * x * x).sum(), (w * x * y).sum()
            det = sw * sxx - sx * sx
            A, B = (sw * sxy - sx * sy) / det, (sxx * sy - sx * sxy) / det
        out.append(torch.stack([B, A]))
    return torch.stack(out).float()


def step_times(shape, reps, rounds):
    from dualpixelface_amd import load_option
    from dualpixelface_amd.plugin import DPNET
    from dualpixelface_amd.recipe import fill_by_recipe, synthetic_batch
    B, H, W = shape
    batch = {k: v.cuda() for k, v in synthetic_batch(B, H, W, seed=7, mask_mode='bern').items()}
    bare = {k: v for k, v in batch.items() if k not in ('abvalue', 'disp')}
    models = []
    for b in (batch, bare):
        model = DPNET(load_option('train_faceDP_dpnet'))
        fill_by_recipe(model)
        model = model.cuda().train()
        for _ in range(4):                                  # warm-up steps and the graph capture
            model.train_step(b, None, lr=1e-4)
        models.append((model, b))
    times = [[], []]
    for _ in range(rounds):
        for t, (model, b) in zip(times, models):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                model.train_step(b, None, lr=1e-4)
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3 / reps)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='4,1,1024,1536:4,5,1024,1536')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--step_shape', default='2,256,384')
    ap.add_argument('--step_reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'affine_fit_timings.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'affine_fit_bench needs an MI355X'
    from dualpixelface_amd import ops
    lines = ['Robust affine fit: python tools/affine_fit_bench.py --shapes %s --reps %d --rounds %d --step_shape %s --step_reps %d'
             % (args.shapes, args.reps, args.rounds, args.step_shape, args.step_reps),
             'One MI355X (gfx950), one process.  max_iters %d, tol %g, f_scale %g.  %d calls between two events on one stream, sides alternating,'
             % (ops.AFFINE_FIT_MAX_ITERS, ops.AFFINE_FIT_TOL, ops.AFFINE_FIT_F_SCALE, args.reps),
             'median of %d rounds (min, max).  "torch" = the same number of reweighting steps as fp64 tensor expressions on the device.' % args.rounds, '']
    for shape in args.shapes.split(':'):
        B, n, H, W = (int(v) for v in shape.split(','))
        for name, sigma, frac in (('clean', 0.05, 0.0), ('heavy', 0.3, 0.2)):
            pred, idepth, depth = fields(B, n, H, W, sigma, frac, 3)
            pred.requires_grad_()
            weights = WEIGHTS[:n]
            ab, info = ops.affine_fit(pred, idepth, return_info=True)
            iters = [int(v) for v in info[:, 2].cpu()]
            steps = max(iters)

            def fit():
                return ops.affine_fit(pred, idepth)

            def fit_loss():
                loss = ops.depth_loss(pred, depth, None, None, weights, 'smoothL1', 'identity', 0.0, target_ab=ops.affine_fit(pred, idepth))
                return torch.autograd.grad(loss, pred)[0]

            def ref():
                return torch_fit(pred.detach(), idepth, steps)

            diff = float((ref() - ab).abs().div(ab.abs()).max())
            tf, tl, tr = bench_support.rounds_of((fit, fit_loss, ref), args.reps, args.rounds, warm=2)
            traffic = 8.0 * H * W * sum(2 + i for i in iters)
            mf = statistics.median(tf)
            lines.append('%-14s %-5s iterations %s | fit %s | fit+loss fwd+bwd %s | torch %d steps %s | torch / fit %.1fx | %.1f MB per fit = '
                         '%.3f TB/s | ab rel diff to torch %.1e'
                         % ('%dx%dx%dx%d' % (B, n, H, W), name, iters, fmt(tf), fmt(tl), steps, fmt(tr), statistics.median(tr) / mf, traffic / 1e6,
                            traffic / (mf * 1e-3) / 1e12, diff))
            print(lines[-1], flush=True)
    sb = tuple(int(v) for v in args.step_shape.split(','))
    tg, tl = step_times(sb, args.step_reps, args.rounds)
    mg, ml = statistics.median(tg), statistics.median(tl)
    lines += ['', 'DPNet train_step, synthetic batch %dx%dx%d, %d steps per round, wall clock around a synchronised run of graph replays:' % (sb + (args.step_reps,)),
              "train_faceDP_dpnet, batch with 'abvalue' (given)    %s" % fmt(tg), "train_faceDP_dpnet, batch without 'abvalue' (fitted) %s" % fmt(tl),
              'difference of the medians %.3f ms = %.1f %% of the given-conversion step' % (ml - mg, 100.0 * (ml - mg) / mg)]
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
