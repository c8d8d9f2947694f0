#!/usr/bin/env python3
"""Normal-guided refinement (csrc/normal_refine.hip): device time of the call, the same conjugate-gradient iteration written in torch on
the GPU in the same run, the algorithmic traffic of an iteration against the copy rate, and the share of an evaluation forward.

    python tools/normal_refine_bench.py [--shapes 1,1024,1536:4,1024,1536] [--iterations 16,32,64] [--reps 10] [--rounds 5]
                                        [--forward_shape 1,1024,1536] [--out profiles/normal_refine_timings.txt]

Scene: tests/normal_refine_cpu.scene (a bumpy tilted surface around 800 mm with depth steps, Bernoulli(0.8) mask, 'disp' target, 0.3 mm depth
noise, the clean surface's normals).  ops.normal_refine is warmed up, then timed two ways for `rounds` rounds, median (min, max): `reps`
calls captured into one graph and replayed between two events (the device time of a call), and `reps` eager calls between two events
(enqueued from Python: an upper bound that includes the host).  "torch" is the solver alone -- the iteration of include/dpf_hip.h as
elementwise tensor operations, shifts by padding and slicing, fp64 sums, alpha and beta kept on the device -- on the system the numpy
restatement assembles on the host (tests/normal_refine_cpu.system: edge flags, b, 1 / D), so its time leaves out the setup and the output
pass that the hip call includes.  Traffic of one iteration: the stencil pass reads r, 1 / D, p and the flag byte and writes p and q (21
bytes a pixel, the halo's second read not counted), the update pass reads p, q, 1 / D, delta, r and writes delta, r (28): 49 bytes a pixel,
over the time an added iteration costs, (t(most iterations) - t(fewest)) / their difference, against the 6.29 TB/s copy rate of
profiles/README.md.  Needs a GPU; there is no CPU fallback.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

import bench_support
from bench_support import fmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12
BYTES_PER_PIXEL_ITERATION = 49.0
LAM, RATIO, MIN_COS = 0.1, 0.01, 0.1


def _shift(t, dy, dx):
    """t at (y + dy, x + dx), zero outside."""
    H, W = t.shape[-2:]
    return torch.nn.functional.pad(t, (1, 1, 1, 1))[..., 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def torch_pcg(T, iterations):
    """The solver of include/dpf_hip.h on the uploaded system T (left, right, up, down, b, invD) -> delta.  Nothing is read on the host."""
    zero = torch.zeros((), device=T['b'].device)
    zero64 = zero.double()

    def A(v):
        d = torch.where(T['left'], v - _shift(v, 0, -1), zero)
        d = d + torch.where(T['right'], v - _shift(v, 0, 1), zero)
        d = d + torch.where(T['up'], v - _shift(v, -1, 0), zero)
        d = d + torch.where(T['down'], v - _shift(v, 1, 0), zero)
        return LAM * v + d

    def total(a, b):
        return (a.double() * b.double()).sum((1, 2))

    r = T['b'].clone()
    delta = torch.zeros_like(r)
    s = r * T['invD']
    p = s.clone()
    rho = total(r, s)
    for _ in range(iterations):
        q = A(p)
        sigma = total(p, q)
        alpha = torch.where((sigma > 0) & (rho > 0), rho / sigma, zero64).float().view(-1, 1, 1)
        delta = delta + alpha * p
        r = r - alpha * q
        s = r * T['invD']
        rho_new = total(r, s)
        beta = torch.where(rho > 0, rho_new / rho, zero64).float().view(-1, 1, 1)
        p = s + beta * p
        rho = rho_new
    return delta


def operands(B, H, W, seed=3):
    """The scene on the device and its system as the numpy restatement assembles it (fp32), uploaded for the torch side."""
    from tests import normal_refine_cpu as nr
    sc = nr.scene(B, H, W, seed)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    sy = nr.system(np.ascontiguousarray(sc['pred'][:, 0]), 'disp', sc['ab'], sc['K'], sc['mask'], sc['normal'], max_edge_ratio=RATIO,
                   min_cos=MIN_COS, lam=LAM, dt=np.float32)
    T = {k: dev(sy[k]) for k in ('left', 'right', 'up', 'down', 'b', 'invD', 'z', 'valid')}
    return dev(sc['pred']), dev(sc['K']), dev(sc['ab']), dev(sc['mask']), dev(sc['normal']), T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='1,1024,1536:4,1024,1536')
    ap.add_argument('--iterations', default='16,32,64')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--forward_shape', default='1,1024,1536')
    ap.add_argument('--forward_reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'normal_refine_timings.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'normal_refine_bench needs an MI355X'
    from dualpixelface_amd import ops
    from reconstruct_bench import forward_time                     # the evaluation forward, timed as that tool times it
    its = [int(v) for v in args.iterations.split(',')]
    lines = ['Normal-guided refinement: python tools/normal_refine_bench.py --shapes %s --iterations %s --reps %d --rounds %d --forward_shape %s '
             '--forward_reps %d' % (args.shapes, args.iterations, args.reps, args.rounds, args.forward_shape, args.forward_reps),
             'One MI355X (gfx950), one process.  target type disp, near 0, no far limit, max_edge_ratio %g, min_cos %g, lambda %g, mask given.'
             % (RATIO, MIN_COS, LAM), '',
             'Time, median of %d rounds (min, max).  "graph replay": %d calls captured into one graph and replayed between two events, per call -- '
             'the device time; the planes' % (args.rounds, args.reps),
             'repeat, so they come from the caches, not from HBM (7 fp32 planes and a byte plane of workspace: 46 MB at 1x1024x1536, 182 MB at 4x).  '
             '"eager": calls enqueued from Python',
             'between two events, hip and torch alternating -- an upper bound that includes the host.  torch: the iteration alone, on the system '
             'the restatement assembled on the host.']
    at_shape = {}
    for shape in args.shapes.split(':'):
        B, H, W = (int(v) for v in shape.split(','))
        pred, K, ab, mask, normal, T = operands(B, H, W)
        tag = '%dx%dx%d' % (B, H, W)
        px = float(B * H * W)
        medians = {}
        for it in its:
            hip = lambda it=it: ops.normal_refine(pred, K, normal, ab=ab, mask=mask, max_edge_ratio=RATIO, min_cos=MIN_COS, lam=LAM, iterations=it)
            tor = lambda it=it: torch_pcg(T, it)
            out, stats = ops.normal_refine(pred, K, normal, ab=ab, mask=mask, max_edge_ratio=RATIO, min_cos=MIN_COS, lam=LAM, iterations=it,
                                           stats=True)
            z = ab[:, 1].view(B, 1, 1) / (out[:, 0] - ab[:, 0].view(B, 1, 1))
            delta = torch.where(T['valid'], torch.log(z.double() / T['z'].double()), torch.zeros((), device=z.device, dtype=torch.float64))
            agree = float((delta - tor().double()).abs().max())
            tr = bench_support.replayed(hip, args.reps, args.rounds)
            th, tt = bench_support.rounds_of((hip, tor), max(1, args.reps // 2), args.rounds)
            ttr = bench_support.replayed(tor, 2, args.rounds)
            medians[it] = statistics.median(tr)
            row = stats[0].cpu().tolist()
            lines.append('%-11s %3d iterations  hip, graph replay %s | hip, eager %s | torch solver, graph replay %s | torch solver, eager %s | '
                         'torch / hip replay %.1fx | rho %.2e -> %.2e (sample 0), max |delta hip - delta torch| %.1e'
                         % (tag, it, fmt(tr), fmt(th), fmt(ttr), fmt(tt), statistics.median(ttr) / medians[it], row[2], row[-1], agree))
            print(lines[-1], flush=True)
        lo, hi = min(its), max(its)
        if hi > lo:
            per = (medians[hi] - medians[lo]) / (hi - lo)
            traffic = BYTES_PER_PIXEL_ITERATION * px
            lines.append('%-11s one more iteration costs %.4f ms (4 launches) | %.1f MB algorithmic = %.3f TB/s = %.1f %% of the copy rate | '
                         'setup, folds and output pass (the intercept): %.3f ms | %d valid pixels, %d edges (sample 0)'
                         % (tag, per, traffic / 1e6, traffic / (per * 1e-3) / 1e12, 100.0 * traffic / (per * 1e-3) / COPY_RATE,
                            medians[lo] - per * lo, row[0], row[1]))
            print(lines[-1], flush=True)
        at_shape[(B, H, W)] = dict(medians)
    fs = tuple(int(v) for v in args.forward_shape.split(','))
    lines += ['', 'STEREODPNET evaluation forward (eval_faceDP, the block off), synthetic batch %dx%dx%d, %d forwards between two events, median of '
              '%d rounds:' % (fs + (args.forward_reps, args.rounds))]
    try:
        t0 = forward_time(fs, args.forward_reps, args.rounds)
        m0 = statistics.median(t0)
        lines.append('forward        %s' % fmt(t0))
        for it, m in sorted(at_shape.get(fs, {}).items()):
            lines.append('the call at that shape, %d iterations, graph replay: %.3f ms = %.2f %% of the forward' % (it, m, 100 * m / m0))
    except Exception as e:                                   # (the forward at this size may not fit: the share is then not measured)
        lines.append('not measured: %s: %s' % (type(e).__name__, str(e).splitlines()[0][:200]))
    lines += ['', 'Not measured: kernel times from a profiler trace (the figures above are event times of captured calls); HBM-resident planes '
              '(the repeated planes stay in the caches); a torch setup pass', '(the torch side is the solver alone); the refinement on face '
              'data (lambda, iterations and min_cos are untuned starting values); a fused single-launch iteration or a multigrid preconditioner '
              '(DESIGN.md section 11).']
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
