#!/usr/bin/env python3
"""The shading block (csrc/shading.hip): device time of the fit and of the apply pass, the same quantities written in torch on the GPU in
the same run, and a StereoDPNet evaluation forward with the block off and on.

    python tools/shading_bench.py [--shapes 1,1024,1536:4,1024,1536] [--iterations 0,3] [--reps 10] [--rounds 5]
                                  [--forward_shape 1,1024,1536] [--out profiles/shading_timings.txt]

Scene: dualpixelface_amd/synthetic_shading.py (the shaded ellipsoid, texture albedo, 5 % outliers, stored gamma-encoded and normalised),
one scene repeated over the batch.  ops.shading_fit and ops.shading_apply (relighting on) are warmed up, then timed two ways for `rounds`
rounds, median (min, max): `reps` calls captured into one graph and replayed between two events (the device time of a call), and `reps`
eager calls between two events (enqueued from Python: an upper bound that includes the host).  "torch" is the fit alone for scale -- the
rows Z as an [N, 16] fp64 tensor built once outside the timing, then per pass the weights, an einsum Gram, torch.linalg.cholesky and
cholesky_solve, all on the device -- so its time leaves out the decoding of the view and the normals that the hip call includes.
Needs a GPU; there is no CPU fallback.
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

F_SCALE, RIDGE = 0.05, 1e-6


def torch_rows(view, normal, mask, gamma=2.2):
    """Z [B, H W, 16] fp64 of a batch, 0 at the pixels that are not counted (the definitions of include/dpf_hip.h in tensor operations)."""
    from dualpixelface_amd.facedp import IMAGENET_MEAN, IMAGENET_STD
    from dualpixelface_amd.synthetic_shading import Y_CONSTANTS
    mean = torch.tensor(IMAGENET_MEAN, device=view.device).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=view.device).view(1, 3, 1, 1)
    v = (view * std + mean).clamp(0, 1)
    I = v.pow(gamma).double()
    n = normal.double()
    length = n.pow(2).sum(1, keepdim=True).sqrt()
    counted = (mask > 0) & (length[:, 0] > 0.5) & ((v >= 0.02) & (v <= 0.98)).all(1)
    x, y, z = (n / length.clamp_min(1e-30)).unbind(1)
    c0, c1, c2, c3, c4 = Y_CONSTANTS
    Y = [torch.full_like(x, c0), c1 * y, c1 * z, c1 * x, c2 * x * y, c2 * y * z, c3 * (3 * z * z - 1), c2 * x * z, c4 * (x * x - y * y)]
    Z = torch.stack(Y + list(I.unbind(1)) + [torch.ones_like(x)] + [torch.zeros_like(x)] * 3, dim=-1)
    return (Z * counted.unsqueeze(-1)).flatten(1, 2)


def torch_fit(Z, iterations):
    """The iteratively reweighted fit on the rows Z [B, N, 16] -> L [B, 3, 9] fp64.  Nothing is read on the host."""
    ridge = torch.diag(torch.tensor([0.0] + [1.0] * 8, dtype=torch.float64, device=Z.device))
    w = torch.ones(Z.shape[:2], dtype=torch.float64, device=Z.device)
    L = None
    for p in range(iterations + 1):
        if p > 0:
            r = Z[..., 9:12] - Z[..., :9] @ L.transpose(1, 2)
            w = 1.0 / torch.sqrt(1.0 + r.pow(2).mean(-1) / (F_SCALE * F_SCALE))
        G = torch.einsum('bni,bnj->bij', Z * w.unsqueeze(-1), Z)
        A = G[:, :9, :9] + RIDGE * G[:, 12, 12].view(-1, 1, 1) * ridge
        L = torch.cholesky_solve(G[:, :9, 9:12], torch.linalg.cholesky(A)).transpose(1, 2)
    return L


def operands(B, H, W):
    from dualpixelface_amd import synthetic_shading as syn
    s = syn.scene(H, W, albedo='texture', outliers=0.05, gamma=2.2, seed=3)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))).cuda()
    return dev(s['view']), dev(s['normal']), dev(s['mask'])


def forward_time(shape, reps, rounds, block):
    from dualpixelface_amd import load_option
    from dualpixelface_amd.config import Option
    from dualpixelface_amd.plugin import STEREODPNET
    from dualpixelface_amd.recipe import fill_by_recipe, synthetic_batch
    B, H, W = shape
    opt = load_option('eval_faceDP')
    if block is not None:
        opt.shading = Option(dict(block))
    model = STEREODPNET(opt)
    fill_by_recipe(model)
    model = model.cuda().eval()
    batch = {k: v.cuda() for k, v in synthetic_batch(B, H, W, seed=7).items()}

    def fn():
        with torch.no_grad():
            model.forward(batch)
    return bench_support.rounds_of((fn,), reps, rounds)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='1,1024,1536:4,1024,1536')
    ap.add_argument('--iterations', default='0,3')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--forward_shape', default='1,1024,1536')
    ap.add_argument('--forward_reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'shading_timings.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'shading_bench needs an MI355X'
    from dualpixelface_amd import ops
    its = [int(v) for v in args.iterations.split(',')]
    lines = ['Shading block: python tools/shading_bench.py --shapes %s --iterations %s --reps %d --rounds %d --forward_shape %s --forward_reps %d'
             % (args.shapes, args.iterations, args.reps, args.rounds, args.forward_shape, args.forward_reps),
             'One MI355X (gfx950), one process.  order 2, gamma 2.2, limits [0.02, 0.98], f_scale %g, ridge %g, mask given; the shaded ellipsoid '
             'with a texture albedo and 5 %% outliers.' % (F_SCALE, RIDGE), '',
             'Time, median of %d rounds (min, max).  "graph replay": %d calls captured into one graph and replayed between two events, per call -- '
             'the device time; the planes repeat, so they' % (args.rounds, args.reps),
             'come from the caches, not from HBM.  "eager": calls enqueued from Python between two events -- an upper bound that includes the host.  '
             'torch: the fit alone (weights, einsum Gram,', 'torch.linalg.cholesky) on rows built outside the timing.']
    for shape in args.shapes.split(':'):
        B, H, W = (int(v) for v in shape.split(','))
        view, normal, mask = operands(B, H, W)
        Z = torch_rows(view, normal, mask)
        tag = '%dx%dx%d' % (B, H, W)
        rows, per_block = ops.shading_rows(H, W)
        for it in its:
            hip = lambda it=it: ops.shading_fit(view, normal, mask, iterations=it, f_scale=F_SCALE, ridge=RIDGE)
            tor = lambda it=it: torch_fit(Z, it)
            light, stats = hip()
            agree = float((light.double() - tor()).abs().max())
            tr = bench_support.replayed(hip, args.reps, args.rounds)
            th, tt = bench_support.rounds_of((hip, tor), max(1, args.reps // 2), args.rounds)
            row = stats[0].cpu().tolist()
            lines.append('%-11s fit, %d reweighted passes (%d launches)  hip, graph replay %s | hip, eager %s | torch fit, eager %s | torch / hip '
                         'replay %.1fx | %d counted pixels, sum w %.0f, RMS %.4f -> %.4f (sample 0, red), max |light hip - L torch| %.1e'
                         % (tag, it, 2 * (it + 1), fmt(tr), fmt(th), fmt(tt), statistics.median(tt) / statistics.median(tr), row[0], row[3], row[4],
                            row[7], agree))
            print(lines[-1], flush=True)
        light, stats = ops.shading_fit(view, normal, mask)
        app = lambda: ops.shading_apply(view, normal, light, mask=mask, stats=stats, relight=True, rotate_deg=(0, 30, 0))
        ta = bench_support.replayed(app, args.reps, args.rounds)
        te = bench_support.rounds_of((app,), max(1, args.reps // 2), args.rounds)[0]
        traffic = B * H * W * (7 * 4 + 9 * 4 + 1)
        lines.append('%-11s apply with relighting (1 launch)  hip, graph replay %s | hip, eager %s | reads 7 and writes 9 fp32 planes and a byte plane: '
                     '%.1f MB algorithmic = %.2f TB/s at the replay time | %d partial rows of %d pixels per sample'
                     % (tag, fmt(ta), fmt(te), traffic / 1e6, traffic / (statistics.median(ta) * 1e-3) / 1e12, rows, per_block))
        print(lines[-1], flush=True)
    fs = tuple(int(v) for v in args.forward_shape.split(','))
    lines += ['', 'STEREODPNET evaluation forward (eval_faceDP), synthetic batch %dx%dx%d, %d forwards between two events, median of %d rounds:'
              % (fs + (args.forward_reps, args.rounds))]
    try:
        t0 = forward_time(fs, args.forward_reps, args.rounds, None)
        t1 = forward_time(fs, args.forward_reps, args.rounds, dict(enabled=True, relight=dict(enabled=True, rotate_deg=[0, 30, 0])))
        lines.append('block off      %s' % fmt(t0))
        lines.append('block on       %s  (+ %.3f ms = %.2f %% of the forward; predicted normals, 3 reweighted passes, relighting)'
                     % (fmt(t1), statistics.median(t1) - statistics.median(t0),
                        100 * (statistics.median(t1) - statistics.median(t0)) / statistics.median(t0)))
    except Exception as e:                                   # (the forward at this size may not fit: the share is then not measured)
        lines.append('not measured: %s: %s' % (type(e).__name__, str(e).splitlines()[0][:200]))
    lines += ['', 'Not measured: kernel times from a profiler trace (the figures above are event times of captured calls); HBM-resident planes (the '
              'repeated planes stay in the caches);', 'the split of a pass between the Gram kernel and the solve; the fit on face data (gamma, '
              'f_scale, ridge and the value limits are untuned starting values).']
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
