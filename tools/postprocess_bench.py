#!/usr/bin/env python3
"""The post_process filters (csrc/postprocess.hip): accuracy against the fp64 restatement on the test cases, time against the same
arithmetic written in torch on the GPU, achieved bandwidth, and the share of an evaluation forward.

    python tools/postprocess_bench.py [--shapes 1,1,1024,1536:4,1,1024,1536] [--reps 50] [--rounds 5] [--forward_shape 1,1024,1536]
                                      [--out profiles/postprocess_timings.txt] [--calls_only N]

Accuracy: the cases of tests/test_gpu_postprocess.py, max |q - q64| against the bar 2 x (error of the fp32 restatement) + 1e-6, and the
hard-statistics case (p + 200) against 2 x (error of the fp32 restatement on the unshifted input) + 2 ulp(200).
Time: ops.guided_filter (radius 8, eps 1e-3: three launches) and ops.joint_bilateral_filter (radius 5, sigma 3.0 / 0.1: one launch), each
warmed up, then timed two ways for `rounds` rounds, median (min, max): `reps` calls captured into one graph and replayed between two
events (the device time of a call), and `reps` eager calls between two events with the hip and torch sides alternating (enqueued from
Python: an upper bound that includes the host).  "torch" is the guided filter as F.avg_pool2d with
count_include_pad=False on raw moments (about twenty launches) and the bilateral filter as F.unfold of the zero-padded planes
((2 r + 1)^2 times the image) with the out-of-image taps masked.  Bandwidth (guided): the algorithmic traffic -- luminance 16 bytes per
pixel and sample, each of the two passes 16 bytes per pixel and head -- over the time, against the 6.29 TB/s copy rate of profiles/README.md.
Share: plugin.STEREODPNET evaluation forward at `forward_shape` on a synthetic batch with the switch off and on, alternating.
Needs a GPU; there is no CPU fallback.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

import bench_support
from bench_support import fmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12
G_R, G_EPS, B_R, B_SS, B_SC = 8, 1e-3, 5, 3.0, 0.1


def torch_luma(guide):
    from dualpixelface_amd.facedp import IMAGENET_MEAN, IMAGENET_STD
    return sum(w * (guide[:, c:c + 1] * IMAGENET_STD[c] + IMAGENET_MEAN[c]) for c, w in enumerate((0.299, 0.587, 0.114)))


def torch_guided(p, guide, r, eps):
    I = torch_luma(guide)
    mean = lambda x: F.avg_pool2d(x, 2 * r + 1, stride=1, padding=r, count_include_pad=False)
    mI, mp = mean(I), mean(p)
    a = (mean(I * p) - mI * mp) / (mean(I * I) - mI * mI + eps)
    b = mp - a * mI
    return mean(a) * I + mean(b)


def torch_bilateral(p, guide, r, ss, sc):
    I = torch_luma(guide)
    B, n, H, W = p.shape
    k = 2 * r + 1
    d = torch.arange(-r, r + 1, device=p.device, dtype=torch.float32)
    ws = torch.exp(-(d[:, None] ** 2 + d[None, :] ** 2) / (2 * ss * ss)).reshape(1, k * k, 1)
    inside = F.unfold(torch.ones(1, 1, H, W, device=p.device), k, padding=r)
    w = ws * inside * torch.exp(-(F.unfold(I, k, padding=r) - I.reshape(B, 1, H * W)) ** 2 / (2 * sc * sc))
    den = w.sum(1)
    return torch.stack([(w * F.unfold(p[:, h:h + 1], k, padding=r)).sum(1) / den for h in range(n)], 1).reshape(B, n, H, W)


def accuracy_lines():
    from tests import postprocess_cpu as pc
    lines = ['Accuracy, max |q - q64| over every element against the bar 2 x (error of the fp32 restatement against fp64) + 1e-6:']
    for kind, cases in (('guided', pc.GUIDED), ('bilateral', pc.BILATERAL)):
        for case in cases:
            p, guide, q64, bar = pc.case(kind, case)
            q = pc.run_filter(kind, pc.on_device(p, case[5]), guide.cuda(), case[4])
            lines.append('  %-9s %-26s kernel %.3e   bar %.3e' % (kind, pc.case_id(case), float((q.cpu().double() - q64).abs().max()), bar))
    B, n, H, W, r, eps = 1, 2, 70, 300, 8, 1e-4
    p, guide = pc.scene(B, n, H, W, seed=7, constant_left=True)
    base = float((pc.guided_filter_fp32(p, guide, r, eps).double() - pc.guided_filter(p, guide, r, eps)).abs().max())
    q64 = pc.guided_filter(p + 200.0, guide, r, eps)
    naive = float((pc.guided_filter_fp32(p + 200.0, guide, r, eps).double() - q64).abs().max())
    from dualpixelface_amd import ops
    err = float((ops.guided_filter((p + 200.0).cuda(), guide.cuda(), r, eps).cpu().double() - q64).abs().max())
    lines.append('  guided, hard statistics (p + 200, eps 1e-4, 1x2x70x300, guide constant left of column 100): kernel %.3e   bar %.3e '
                 '(= 2 x %.3e on the unshifted input + 2 ulp(200))   the fp32 restatement on the shifted input %.3e'
                 % (err, 2 * base + 2 * pc.ULP200, base, naive))
    return lines


def forward_share(shape, reps, rounds):
    from dualpixelface_amd import load_option
    from dualpixelface_amd.plugin import STEREODPNET
    from dualpixelface_amd.recipe import fill_by_recipe, synthetic_batch
    B, H, W = shape
    model = STEREODPNET(load_option('eval_faceDP_guided'))
    fill_by_recipe(model)
    model = model.cuda().eval()
    batch = {k: v.cuda() for k, v in synthetic_batch(B, H, W, seed=7).items()}
    block = model.option.post_process

    def run(guided, bilateral):
        def fn():
            block.use_guided, block.use_bilateral = guided, bilateral
            with torch.no_grad():
                model.forward(batch)
        return fn
    times = bench_support.rounds_of((run(False, False), run(True, False), run(False, True)), reps, rounds)
    # the filters alone on this forward's own prediction and guide, as device time
    from dualpixelface_amd import ops
    run(False, False)()
    with torch.no_grad():
        raw = model.forward(batch)['pred_depth'].contiguous()
    guide = model._views(batch)[0]
    alone = (bench_support.replayed(lambda: ops.guided_filter(raw, guide, G_R, G_EPS), 20, rounds),
             bench_support.replayed(lambda: ops.joint_bilateral_filter(raw, guide, B_R, B_SS, B_SC), 20, rounds))
    return times, alone, tuple(raw.shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='1,1,1024,1536:4,1,1024,1536')
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--forward_shape', default='1,1024,1536')
    ap.add_argument('--forward_reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'postprocess_timings.txt'))
    ap.add_argument('--calls_only', type=int, default=0, help='N guided and N bilateral calls per shape and nothing else: the run to put under '
                    'rocprofv3 --kernel-trace (profiles/postprocess_kernel_trace.txt)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'postprocess_bench needs an MI355X'
    from dualpixelface_amd import ops
    from tests import postprocess_cpu as pc
    if args.calls_only:
        for shape in args.shapes.split(':'):
            B, n, H, W = (int(v) for v in shape.split(','))
            p, guide = (t.cuda() for t in pc.scene(B, n, H, W, seed=3))
            for _ in range(args.calls_only):
                ops.guided_filter(p, guide, G_R, G_EPS)
                ops.joint_bilateral_filter(p, guide, B_R, B_SS, B_SC)
            torch.cuda.synchronize()
        return
    lines = ['Post-processing filters: python tools/postprocess_bench.py --shapes %s --reps %d --rounds %d --forward_shape %s --forward_reps %d'
             % (args.shapes, args.reps, args.rounds, args.forward_shape, args.forward_reps),
             'One MI355X (gfx950), one process.  guided: radius %d, eps %g; bilateral: radius %d, sigma_space %g, sigma_color %g.'
             % (G_R, G_EPS, B_R, B_SS, B_SC), '']
    lines += accuracy_lines()
    lines += ['', 'Time, median of %d rounds (min, max).  "graph replay": %d calls captured into one graph and replayed between two events, per call '
              '-- the device time; the inputs' % (args.rounds, args.reps),
              'repeat, so at 1x1x1024x1536 (6 MB a plane) they come from the caches, not from HBM.  "eager calls": %d calls enqueued from Python '
              'between two events, hip and torch' % args.reps,
              'alternating -- an upper bound that includes the host (bilateral and its torch side: a fifth of the calls).']
    for shape in args.shapes.split(':'):
        B, n, H, W = (int(v) for v in shape.split(','))
        p, guide = pc.scene(B, n, H, W, seed=3)
        p, guide = p.cuda(), guide.cuda()
        tag = '%dx%dx%dx%d' % (B, n, H, W)
        guided = lambda: ops.guided_filter(p, guide, G_R, G_EPS)
        tg, tt = bench_support.rounds_of((guided, lambda: torch_guided(p, guide, G_R, G_EPS)), args.reps, args.rounds)
        tr = bench_support.replayed(guided, args.reps, args.rounds)
        diff = float((guided() - torch_guided(p, guide, G_R, G_EPS)).abs().max())
        traffic = 16.0 * B * H * W + 32.0 * B * n * H * W
        mg = statistics.median(tr)
        lines.append('%-14s guided    hip, graph replay %s | hip, eager calls %s | torch avg_pool2d %s | torch / hip replay %.1fx | %.1f MB '
                     'algorithmic = %.3f TB/s = %.1f %% of the copy rate | max diff to torch %.1e'
                     % (tag, fmt(tr), fmt(tg), fmt(tt), statistics.median(tt) / mg, traffic / 1e6, traffic / (mg * 1e-3) / 1e12,
                        100.0 * traffic / (mg * 1e-3) / COPY_RATE, diff))
        print(lines[-1], flush=True)
        bilateral = lambda: ops.joint_bilateral_filter(p, guide, B_R, B_SS, B_SC)
        tr = bench_support.replayed(bilateral, args.reps, args.rounds)
        try:
            tb, tu = bench_support.rounds_of((bilateral, lambda: torch_bilateral(p, guide, B_R, B_SS, B_SC)), max(1, args.reps // 5), args.rounds)
            diff = float((bilateral() - torch_bilateral(p, guide, B_R, B_SS, B_SC)).abs().max())
            lines.append('%-14s bilateral hip, graph replay %s | hip, eager calls %s | torch unfold (%d x the image) %s | torch / hip replay '
                         '%.1fx | max diff to torch %.1e'
                         % (tag, fmt(tr), fmt(tb), (2 * B_R + 1) ** 2, fmt(tu), statistics.median(tu) / statistics.median(tr), diff))
        except torch.cuda.OutOfMemoryError:
            lines.append('%-14s bilateral hip, graph replay %s | torch unfold: out of memory at this size, not measured' % (tag, fmt(tr)))
        print(lines[-1], flush=True)
    fs = tuple(int(v) for v in args.forward_shape.split(','))
    lines += ['', 'STEREODPNET evaluation forward (eval_faceDP_guided), synthetic batch %dx%dx%d, %d forwards between two events, median of %d rounds:'
              % (fs + (args.forward_reps, args.rounds))]
    try:
        (t0, t1, t2), (ag, ab), pshape = forward_share(fs, args.forward_reps, args.rounds)
        m0, m1, m2 = (statistics.median(t) for t in (t0, t1, t2))
        lines += ['switches off   %s' % fmt(t0),
                  'use_guided     %s   difference of the medians %.3f ms = %.2f %% of the forward' % (fmt(t1), m1 - m0, 100 * (m1 - m0) / m0),
                  'use_bilateral  %s   difference of the medians %.3f ms = %.2f %% of the forward' % (fmt(t2), m2 - m0, 100 * (m2 - m0) / m0),
                  'the filters alone on that forward\'s pred_depth %s, graph replay: guided %s = %.2f %% of the forward; bilateral %s = %.2f %%'
                  % ('x'.join(str(v) for v in pshape), fmt(ag), 100 * statistics.median(ag) / m0, fmt(ab), 100 * statistics.median(ab) / m0)]
    except Exception as e:                                   # (the forward at this size may not fit: the share is then not measured)
        lines.append('not measured: %s: %s' % (type(e).__name__, str(e).splitlines()[0][:200]))
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
