#!/usr/bin/env python3
"""Depth-target loss bank: forward + backward of ops.depth_loss against the same expressions written in torch on the GPU.

    python tools/loss_bank_bench.py [--shape 4,3,1024,1536] [--reps 200] [--rounds 3] [--out profiles/loss_bank_timings.txt]

Two cases, masked: silog (identity transform) and smooth-L1 on the 'idepth' target.  "torch" is the reference's formula
(src/loss/depth/silog.py:45-48, smoothL1.py:41-42: boolean-mask indexing per head, then mean) under autograd on the same device.  Each side is
warmed up, then `reps` forward + backward calls are timed between two events on one stream; the sides alternate for `rounds` rounds and the
median round is reported with min and max.  A call of the hip side is three short launches enqueued from Python, so its time is an upper
bound of the device time (the host's enqueue cost is not measured apart).  Bandwidth is the algorithmic traffic of csrc/loss_bank.hip -- forward reads the n prediction
planes, the target and the mask once, backward reads them again and writes n planes -- over the measured time, against the 8 TB/s HBM
peak of the MI355X.  Needs a GPU; there is no CPU fallback.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

import bench_support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
WEIGHTS = [1.0, 0.7, 0.5, 0.4, 0.3, 0.2, 0.1, 0.05]
VARIANCE_FOCUS = 0.85


def torch_loss(kind, pred, target, mask, weights):
    sel = mask > 0
    gt = target[sel]
    if kind == 'silog':
        dist = [weights[i] * (torch.log(pred[:, i][sel]) - torch.log(gt)) for i in range(pred.shape[1])]
        return sum(torch.sqrt((d ** 2).mean() - VARIANCE_FOCUS * (d.mean() ** 2)) * 10.0 for d in dist)
    return sum(weights[i] * F.smooth_l1_loss(pred[:, i][sel], gt) for i in range(pred.shape[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='4,3,1024,1536')
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'loss_bank_timings.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'loss_bank_bench needs an MI355X'
    from dualpixelface_amd import ops
    B, n, H, W = (int(v) for v in args.shape.split(','))
    g = torch.Generator().manual_seed(3)
    u = lambda lo, hi, *shape: (torch.rand(*shape, generator=g) * (hi - lo) + lo).cuda()
    target, mask = u(0.5, 2.5, B, H, W), (torch.rand(B, H, W, generator=g) < 0.6).float().cuda()
    weights = WEIGHTS[:n]
    plane = 4.0 * B * H * W
    nbytes = (n + 2) * plane + (2 * n + 2) * plane             # forward reads n + target + mask; backward reads the same, writes n
    lines = ['Depth-target loss bank: python tools/loss_bank_bench.py --shape %s --reps %d --rounds %d' % (args.shape, args.reps, args.rounds),
             'One MI355X (gfx950), one process.  pred [%d, %d, %d, %d] fp32, Bernoulli(0.6) mask, no conf; forward + backward per call, %d calls'
             % (B, n, H, W, args.reps),
             'between two events on one stream, sides alternating, median of %d rounds (min, max).  "hip" = ops.depth_loss (csrc/loss_bank.hip),' % args.rounds,
             '"torch" = the reference\'s formula under autograd on the same device.  Bandwidth: %.1f MB of algorithmic traffic per call' % (nbytes / 1e6),
             '(forward reads n + 2 planes, backward reads n + 2 and writes n) over the hip time, against the %.0f TB/s HBM peak.' % (HBM_PEAK / 1e12), '']
    for name, kind in (('silog', 'silog'), ('smoothL1 idepth', 'smoothL1')):
        pred = u(0.5, 2.5, B, n, H, W).requires_grad_()

        def hip():
            loss = ops.depth_loss(pred, target, mask, None, weights, kind, 'identity', VARIANCE_FOCUS)
            return loss, torch.autograd.grad(loss, pred)[0]

        def ref():
            loss = torch_loss(kind, pred, target, mask, weights)
            return loss, torch.autograd.grad(loss, pred)[0]

        (lh, gh), (lr, gr) = hip(), ref()
        loss_rel = abs(float(lh.detach()) - float(lr.detach())) / abs(float(lr.detach()))
        grad_rel = float((gh - gr).abs().max() / gr.abs().max())
        for fn in (hip, ref):
            bench_support.timed(fn, 10)
        th, tr = [], []
        for _ in range(args.rounds):
            th.append(bench_support.timed(hip, args.reps))
            tr.append(bench_support.timed(ref, args.reps))
        mh, mr = statistics.median(th), statistics.median(tr)
        bw = nbytes / (mh * 1e-3)
        lines.append('%-16s hip %.4f ms (min %.4f, max %.4f) | torch %.4f ms (min %.4f, max %.4f) | torch / hip %.1fx | hip %.2f TB/s = %.0f %% of HBM peak'
                     ' | loss rel diff %.1e, grad max diff / max %.1e'
                     % (name, mh, min(th), max(th), mr, min(tr), max(tr), mr / mh, bw / 1e12, 100.0 * bw / HBM_PEAK, loss_rel, grad_rel))
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
