#!/usr/bin/env python3
"""The kernels on the heads' hypothesis distribution (csrc/head_confidence.hip, csrc/unimodal.hip): device time of ops.head_confidence with
all planes and with one, of ops.confidence_curve, of ops.unimodal_loss forward and backward, of the same five confidence quantities formed
in torch from the probability volume of ops.softargmin_heads in the same run, each against its algorithmic traffic at the copy rate, and
the StereoDPNet evaluation forward with the confidence block on against off.

    python tools/head_dist_bench.py [--shapes 1,1024,1536:4,1024,1536] [--heads 3] [--reps 10] [--rounds 5] [--forward_shape 1,1024,1536]
                                    [--out profiles/head_dist_timings.txt]

Logits: n tensors [B, 1, 8, H / 4, W / 4] of 2 x standard normal draws, the shipped hypotheses (32, 0.5 px apart), align_corners.  A call is
warmed up, then `reps` calls are captured into one graph and replayed between two events, median of `rounds` rounds (min, max): the device
time of a call.  The unimodal loss runs through autograd, so it is timed eagerly instead -- `reps` calls enqueued from Python between two
events, forward alone and forward + backward alternating, the backward their difference: an upper bound that includes the host.
Algorithmic bytes: the kernel reads the logits (B n 8 h w floats) and writes the planes asked for (B n H W each); the curve reads conf,
pred, target and mask (4 floats a pixel); the unimodal forward reads the logits, target and mask and writes the log-sum plane, the backward
reads those and writes the logit gradients; the torch formulation reads the probability volume (B n 32 H W floats) once per reduction it
takes -- six: max, entropy, mean, variance and the two window sums -- and the temporaries it writes are not counted.  Shares are of the
6.29 TB/s copy rate of profiles/README.md.  Needs a GPU; there is no CPU fallback.
"""
import argparse
import math
import os
import statistics
import sys

import torch

import bench_support
from bench_support import fmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12
D, L, SCALE = 8, 32, 4
TORCH_PASSES = 6


def torch_planes(prob, d, window):
    """peak, entropy, mass, spread, modal and the argmax from prob [B, n, L, H, W]; d [1, 1, L, 1, 1]."""
    idx = torch.arange(L, device=prob.device).view(1, 1, L, 1, 1)
    peak, lstar = prob.max(2)
    entropy = (1 + torch.xlogy(prob, prob).sum(2) / math.log(L)).clamp(0, 1)
    mu = (prob * d).sum(2)
    spread = (prob * (d - mu.unsqueeze(2)) ** 2).sum(2).sqrt()
    inside = ((idx - lstar.unsqueeze(2)).abs() <= window).to(prob.dtype)
    M = (prob * inside).sum(2)
    modal = (prob * inside * d).sum(2) / M
    return peak, entropy, M.clamp(max=1), spread, modal, lstar


def share(nbytes, ms):
    return '%.1f MB algorithmic = %.3f TB/s = %.1f %% of the copy rate' % (nbytes / 1e6, nbytes / (ms * 1e-3) / 1e12,
                                                                          100.0 * nbytes / (ms * 1e-3) / COPY_RATE)


def forward_times(shape, reps, rounds):
    """The StereoDPNet evaluation forward with the confidence block off and on (entropy, modal, a threshold), alternating."""
    from dualpixelface_amd import load_option
    from dualpixelface_amd.config import Option
    from dualpixelface_amd.plugin import STEREODPNET
    from dualpixelface_amd.recipe import fill_by_recipe, synthetic_batch
    B, H, W = shape
    model = STEREODPNET(load_option('eval_faceDP'))
    fill_by_recipe(model)
    model = model.cuda().eval()
    batch = {k: v.cuda() for k, v in synthetic_batch(B, H, W, seed=7).items()}

    def run(block):
        def fn():
            model.option.confidence = Option(dict(block))
            with torch.no_grad():
                model.forward(batch)
        return fn
    return bench_support.rounds_of((run(dict(enabled=False)), run(dict(enabled=True, estimator='modal', threshold=0.5))), reps, rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='1,1024,1536:4,1024,1536')
    ap.add_argument('--heads', type=int, default=3)
    ap.add_argument('--window', type=int, default=1)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--forward_shape', default='1,1024,1536')
    ap.add_argument('--forward_reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'head_dist_timings.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'head_dist_bench needs an MI355X'
    from dualpixelface_amd import ops
    from tests.unimodal_cpu import shipped_disp
    n, disp = args.heads, shipped_disp()
    lines = ['Head distribution kernels: python tools/head_dist_bench.py --shapes %s --heads %d --window %d --reps %d --rounds %d --forward_shape %s '
             '--forward_reps %d' % (args.shapes, n, args.window, args.reps, args.rounds, args.forward_shape, args.forward_reps),
             'One MI355X (gfx950), one process.  %d heads, 8 levels -> 32 hypotheses, align_corners (the fast path).' % n, '',
             'Time, median of %d rounds (min, max).  "graph replay": %d calls captured into one graph and replayed between two events, per call '
             '-- the device time.' % (args.rounds, args.reps),
             '"eager": calls enqueued from Python between two events, an upper bound that includes the host.']
    for shape in args.shapes.split(':'):
        B, H, W = (int(v) for v in shape.split(','))
        h, w = H // SCALE, W // SCALE
        tag = '%dx%dx%dx%d' % (B, n, H, W)
        g = torch.Generator(device='cuda').manual_seed(5)
        ks = [2.0 * torch.randn(B, 1, D, h, w, device='cuda', generator=g) for _ in range(n)]
        target = torch.rand(B, H, W, device='cuda', generator=g) * 20.0 - 6.0
        mask = (torch.rand(B, H, W, device='cuda', generator=g) < 0.8).float()
        plane, logit_bytes = 4.0 * B * n * H * W, 4.0 * B * n * D * h * w

        # the confidence planes
        every = lambda: ops.head_confidence(ks, disp, window=args.window)                                  # noqa: E731
        one = lambda: ops.head_confidence(ks, disp, window=args.window, want=('entropy',))                 # noqa: E731
        t_all, t_one = bench_support.replayed(every, args.reps, args.rounds), bench_support.replayed(one, args.reps, args.rounds)
        m_all, m_one = statistics.median(t_all), statistics.median(t_one)
        lines.append('%-16s head_confidence, 6 planes, graph replay %s | %s' % (tag, fmt(t_all), share(logit_bytes + 6 * plane, m_all)))
        lines.append('%-16s head_confidence, 1 plane,  graph replay %s | %s' % (tag, fmt(t_one), share(logit_bytes + plane, m_one)))
        print('\n'.join(lines[-2:]), flush=True)

        # the same five quantities in torch from the probability volume (formed once, outside the timed window)
        _, pred, prob = ops.softargmin_heads(ks, disp, SCALE, True)
        d = torch.tensor(disp, device='cuda').view(1, 1, L, 1, 1)
        got, want = every(), torch_planes(prob, d, args.window)
        # (torch takes the peak from the rounded probabilities, the kernel from the logits: where the two largest are an ulp apart they may
        # name different hypotheses, and the window sums then differ by construction; those pixels are counted, not compared)
        same = got['lstar'] == want[5]
        agree = ', '.join('%s %.1e' % (k, float((got[k] - v).abs()[same].max())) for k, v in zip(('peak', 'entropy', 'mass', 'spread', 'modal'), want))
        agree += ' where the peak index agrees (it differs at %d of %d pixels)' % (int((~same).sum()), same.numel())
        del want, same
        tor = lambda: torch_planes(prob, d, args.window)                                                   # noqa: E731
        t_tor = bench_support.replayed(tor, 2, args.rounds)
        m_tor = statistics.median(t_tor)
        lines.append('%-16s torch on the probability volume, graph replay %s | %s | torch / hip (5 planes against 6) %.1fx | max |hip - torch|: %s'
                     % (tag, fmt(t_tor, 2), share(TORCH_PASSES * 4.0 * B * n * L * H * W, m_tor), m_tor / m_all, agree))
        print(lines[-1], flush=True)
        del prob

        # the curve
        table = torch.zeros(16, 2, dtype=torch.float64, device='cuda')
        curve = lambda: ops.confidence_curve(got['entropy'][:, 0], pred[:, 0], target, mask=mask, bins=16, into=table)    # noqa: E731
        t_curve = bench_support.replayed(curve, args.reps, args.rounds)
        lines.append('%-16s confidence_curve, head 0, 16 bins, graph replay %s | %s' % ('%dx%dx%d' % (B, H, W), fmt(t_curve),
                                                                                       share(16.0 * B * H * W, statistics.median(t_curve))))
        print(lines[-1], flush=True)

        # the unimodal loss, through autograd
        leaves = [k.clone().requires_grad_(True) for k in ks]
        weights = tuple([1.0, 0.7, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5][:n])

        def fwd():
            with torch.no_grad():
                ops.unimodal_loss(leaves, disp, target, mask=mask, head_weights=weights)

        def both():
            for k in leaves:
                k.grad = None
            ops.unimodal_loss(leaves, disp, target, mask=mask, head_weights=weights).backward()
        t_f, t_fb = bench_support.rounds_of((fwd, both), args.reps, args.rounds)
        m_f, m_b = statistics.median(t_f), statistics.median(t_fb) - statistics.median(t_f)
        fwd_bytes = logit_bytes + 8.0 * B * H * W + plane
        bwd_bytes = 2 * logit_bytes + 8.0 * B * H * W + plane
        lines.append('%-16s unimodal_loss forward, eager %s | %s' % (tag, fmt(t_f), share(fwd_bytes, m_f)))
        lines.append('%-16s unimodal_loss forward + backward, eager %s | backward (the difference of the medians) %.3f ms | %s'
                     % (tag, fmt(t_fb), m_b, share(bwd_bytes, m_b)))
        print('\n'.join(lines[-2:]), flush=True)
        del leaves, got, pred
        torch.cuda.empty_cache()

    fs = tuple(int(v) for v in args.forward_shape.split(','))
    lines += ['', 'STEREODPNET evaluation forward (eval_faceDP), synthetic batch %dx%dx%d, %d forwards between two events, the block off and on '
              '(entropy, modal, threshold 0.5) alternating,' % (fs + (args.forward_reps,)), 'median of %d rounds:' % args.rounds]
    try:
        t_off, t_on = forward_times(fs, args.forward_reps, args.rounds)
        m_off, m_on = statistics.median(t_off), statistics.median(t_on)
        lines.append('block off      %s' % fmt(t_off))
        lines.append('block on       %s | on - off %.3f ms = %.2f %% of the forward' % (fmt(t_on), m_on - m_off, 100 * (m_on - m_off) / m_off))
    except Exception as e:                                   # (the forward at this size may not fit: the share is then not measured)
        lines.append('not measured: %s: %s' % (type(e).__name__, str(e).splitlines()[0][:200]))
    lines += ['', 'Not measured: kernel times from a profiler trace (the figures above are event times of captured or enqueued calls); the '
              'general path (any geometry but 8 -> 32 with align_corners);', 'the unimodal backward on its own (it is the difference of two eager '
              'medians); the measures on face data (threshold, window and measure are untuned starting values).']
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
