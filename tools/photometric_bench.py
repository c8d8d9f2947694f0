#!/usr/bin/env python3
"""Photometric and smoothness losses (loss_type 'photometric' / 'smoothness', csrc/photometric.hip): shift agreement, kernel timings,
share of the train step.

    python tools/photometric_bench.py --agreement [--config train_faceDP_dpnet_photometric] [--loader]
    python tools/photometric_bench.py [--reps 100] [--rounds 3] [--out profiles/photometric_timings.txt]
    python tools/photometric_bench.py --step [--config train_faceDP_dpnet_photometric] [--root DIR]

--agreement  prints the mean photometric term under the disparity the batch brings (pred = batch['disp']) for shift in
             {(0, +-1), (0, +-2), (+-1, 0), (+-2, 0)}, and under zero displacement: the shift whose term is the smallest, and clearly
             below the zero-displacement one, is the one the data was recorded with.  The batch is the first of the config's training
             loader with --loader (needs the dataset), else a synthetic pair built with ref(y) = tgt(y - 2 d), so the synthetic answer
             only proves the tool.
(default)    forward and backward of ops.photometric_loss and ops.smoothness_loss at 4x1x1024x1536 and 2x5x256x384 (DPNet's five heads):
             each warmed up, `reps` calls between two events on one stream, median of `rounds` rounds with min and max, against the
             algorithmic bytes at the 6.29 TB/s copy rate.  Then the captured DPNet step at 2x256x384 with the shipped photometric
             config on a batch of the two views against train_faceDP_dpnet on the full batch, alternating.  A call is enqueued from
             Python launch by launch, so its time is an upper bound of the device time.
--step       one line: the median time of the captured DPNet train step at 2x256x384 under --config, package imported from --root (so
             the same script times another checkout of the project).
Needs a GPU; there is no CPU fallback.
"""
import argparse
import math
import os
import statistics
import sys

import torch

import bench_support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = [1.0, 0.75294, 0.18824, 0.047059, 0.011765]
COPY_TBS = 6.29
SHIFTS = [(0.0, 1.0), (0.0, -1.0), (0.0, 2.0), (0.0, -2.0), (1.0, 0.0), (-1.0, 0.0), (2.0, 0.0), (-2.0, 0.0)]


def synthetic_pair(B, n, H, W, seed=3, device='cuda'):
    """A smooth target view, a disparity field d of up to 1.5 px, the reference view ref(y) = tgt(y - 2 d) (grid_sample, bilinear), an
    elliptical mask, and per head d plus a ripple of 0.1 px as the prediction.  Images are normalised as the data path normalises them."""
    from dualpixelface_amd.facedp import IMAGENET_MEAN, IMAGENET_STD
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    tgt = torch.stack([torch.stack([0.5 + 0.25 * torch.sin(xs / (11.0 + 3 * c) + b) * torch.cos(ys / (7.0 + 2 * c)) + 0.15 * torch.sin((xs + ys) / 23.0)
                                    for c in range(3)]) for b in range(B)])
    d = torch.stack([1.5 * torch.sin(xs / (60.0 + 7 * b)) * torch.cos(ys / 45.0) for b in range(B)])
    gy = (ys[None] - 2.0 * d) / (H - 1) * 2 - 1
    gx = (xs[None] / (W - 1) * 2 - 1).expand(B, H, W)
    ref = torch.nn.functional.grid_sample(tgt, torch.stack([gx, gy], -1), mode='bilinear', padding_mode='border', align_corners=True)
    mean, std = torch.tensor(IMAGENET_MEAN, dtype=torch.float64).view(1, 3, 1, 1), torch.tensor(IMAGENET_STD, dtype=torch.float64).view(1, 3, 1, 1)
    mask = ((((xs + 0.5) / W - 0.5) / 0.45) ** 2 + (((ys + 0.5) / H - 0.5) / 0.45) ** 2 <= 1.0).float().expand(B, H, W).contiguous()
    pred = torch.stack([d + 0.1 * torch.sin(xs / (7.0 + h)) * torch.cos(ys / (9.0 + h)) for h in range(n)], 1)
    out = dict(ref=((ref - mean) / std).float(), tgt=((tgt - mean) / std).float(), disp=d.float(), mask=mask, pred=pred.float())
    return {k: v.contiguous().to(device) for k, v in out.items()}


def agreement(args):
    from dualpixelface_amd import load_option, ops, photometric
    opt = load_option(args.config)
    s = photometric.settings(opt)
    if args.loader:
        from dualpixelface_amd.plugin import DPNET
        sys.path.insert(0, ROOT)
        os.chdir(ROOT)
        batch = next(iter(DPNET(opt).train_dataloader()))
        batch = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}
        what = 'the first training batch of %s' % args.config
        ref, tgt = (batch['right'], batch['left']) if opt.dataset.flip_lr else (batch['left'], batch['right'])     # as the loss takes them
    else:
        batch, what = synthetic_pair(2, 1, 256, 384), 'a synthetic pair with ref(y) = tgt(y - 2 d)'
        ref, tgt = batch['ref'], batch['tgt']
    disp = batch['disp'][:, None].contiguous().float()
    print('photometric agreement on %s (alpha %g, eps %g; configured shift %s)' % (what, s.alpha, s.charbonnier_eps, list(s.shift)))

    def term(pred, shift):
        loss, _, counted = ops.photometric_loss(pred, ref, tgt, mask=batch.get('mask'), shift=shift, alpha=s.alpha, eps=s.charbonnier_eps,
                                                return_warped=True)
        return float(loss), int(counted.sum()), counted.numel()

    rows = [('zero displacement', term(torch.zeros_like(disp), (0.0, 1.0)))] + [('shift (%+g, %+g)' % sh, term(disp, sh)) for sh in SHIFTS]
    best = min(rows[1:], key=lambda r: r[1][0] if r[1][1] else math.inf)
    for name, (loss, cnt, total) in rows:
        print('  %-18s mean term %.6f over %d of %d pixels%s' % (name, loss, cnt, total, '   <- smallest' if name == best[0] else ''))


def _row(tag, shape, times, nbytes, extra=''):
    m = statistics.median(times)
    floor = nbytes / (COPY_TBS * 1e12) * 1e3
    return ('%dx%dx%dx%d  %-22s %.4f ms (min %.4f, max %.4f) | %.1f MB -> %.2f TB/s, %.4f ms at %.2f TB/s = %.0f %% of the time%s'
            % (*shape, tag, m, min(times), max(times), nbytes / 1e6, nbytes / (m * 1e-3) / 1e12, floor, COPY_TBS, 100.0 * floor / m, extra))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--agreement', action='store_true')
    ap.add_argument('--config', default='train_faceDP_dpnet_photometric')
    ap.add_argument('--loader', action='store_true')
    ap.add_argument('--step', action='store_true')
    ap.add_argument('--root', default=ROOT)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'photometric_timings.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'photometric_bench needs an MI355X'
    if args.step:
        sys.path.insert(0, os.path.abspath(args.root))
        fn = bench_support.captured_dpnet_step(args.config, 256, 384, 'photometric' in args.config)
        return bench_support.step_line('config %s' % args.config, fn, args.reps, args.rounds, args.root)
    sys.path.insert(0, ROOT)
    if args.agreement:
        return agreement(args)
    from dualpixelface_amd import ops
    lines = ['Photometric and smoothness losses: python tools/photometric_bench.py --reps %d --rounds %d' % (args.reps, args.rounds),
             'One MI355X (gfx950), one process.  ops.photometric_loss (csrc/photometric.hip: 3 launches forward, 1 backward) and',
             'ops.smoothness_loss (3 + 1) on a synthetic pair, disp target, shift (0, -2), elliptical mask; %d calls between two events on one' % args.reps,
             'stream, median of %d rounds (min, max); enqueued from Python launch by launch, so an upper bound of the device time.' % args.rounds,
             'Algorithmic bytes per sample plane of H W floats: photometric forward 6 (both images) + 2 (luminance planes written) + n (pred,',
             'mask, both luminance planes = 4 n); backward n (those 4 and d pred = 5 n); smoothness forward 3 + 1 + 3 n, backward 4 n.', '']
    for B, n, H, W in ((4, 1, 1024, 1536), (2, 5, 256, 384)):
        sc = synthetic_pair(B, n, H, W)
        pred = sc['pred'].requires_grad_()
        weights = WEIGHTS[:n] if n > 1 else [1.0]
        plane = 4.0 * B * H * W
        ops_ = (('photometric', lambda: ops.photometric_loss(pred, sc['ref'], sc['tgt'], mask=sc['mask'], head_weights=weights),
                 plane * (8 + 4 * n), plane * 5 * n),
                ('smoothness', lambda: ops.smoothness_loss(pred, sc['ref'], mask=sc['mask'], head_weights=weights), plane * (4 + 3 * n), plane * 4 * n))
        for name, fwd, fbytes, bbytes in ops_:
            loss = fwd()
            bwd = lambda: torch.autograd.grad(loss, pred, retain_graph=True)[0]                    # noqa: E731
            grad = bwd()
            assert math.isfinite(float(loss)) and bool(torch.isfinite(grad).all())
            for fn in (fwd, bwd):
                bench_support.timed(fn, 5)
            tf, tb = [], []
            for _ in range(args.rounds):
                tf.append(bench_support.timed(fwd, args.reps))
                tb.append(bench_support.timed(bwd, args.reps))
            lines.append(_row(name + ' forward', (B, n, H, W), tf, fbytes, ' | loss %.6f' % float(loss)))
            lines.append(_row(name + ' backward', (B, n, H, W), tb, bbytes, ' | max |d pred| %.3e' % float(grad.abs().max())))
    lines += ['', 'Captured DPNet train step at 2x256x384 (synthetic batch, fp32): train_faceDP_dpnet (loss_type [smoothL1], the full batch) against',
              'train_faceDP_dpnet_photometric (loss_type [photometric, smoothness], lambdas 1.0, 0.1, a batch of the two views only),',
              '%d replays between two events, alternating, %d rounds:' % (args.reps, args.rounds)]
    plain = bench_support.captured_dpnet_step('train_faceDP_dpnet', 256, 384)
    ours = bench_support.captured_dpnet_step('train_faceDP_dpnet_photometric', 256, 384, views_only=True)
    tp, to = [], []
    for _ in range(args.rounds):
        tp.append(bench_support.timed(plain, args.reps))
        to.append(bench_support.timed(ours, args.reps))
    mp, mo = statistics.median(tp), statistics.median(to)
    lines.append('smoothL1 %.4f ms (min %.4f, max %.4f) | photometric + smoothness %.4f ms (min %.4f, max %.4f) | %+.4f ms = %+.2f %% of the step'
                 % (mp, min(tp), max(tp), mo, min(to), max(to), mo - mp, 100.0 * (mo - mp) / mp))
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
