#!/usr/bin/env python3
"""The refocus block (csrc/refocus.hip): device time of the plan and of the render, the same render written in torch on the GPU at a size
where its unfold fits, and a StereoDPNet evaluation forward with the block off and on.

    python tools/refocus_bench.py [--shapes 1,1024,1536:4,1024,1536] [--radii 8,16,32] [--reps 5] [--rounds 5]
                                  [--torch_shape 1,128,192] [--forward_shape 1,1024,1536] [--out profiles/refocus_timings.txt]

Scenes: the textures of dualpixelface_amd/synthetic_refocus.py, one scene repeated over the batch.  "full": every pixel at r = max_radius
(the worst case: every tile walks the whole window).  "portrait": a near plane over the middle third of the width, in focus (r = 0), the
far plane around it at r = max_radius -- the tiles further than max_radius from the far plane walk a window of one tap.  The plan and
the render are warmed up, then `reps` calls are captured into one graph and replayed between two events, median of `rounds` rounds
(min, max): the device time of a call.  Needs a GPU; there is no CPU fallback.
"""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

import bench_support
from bench_support import fmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def operands(B, H, W, kind):
    """(view, disparity, mask) on the device, and the focus settings under which `kind` is what the docstring says."""
    from dualpixelface_amd import synthetic_refocus as syn
    s = syn.scene(H, W, box=(0, H, W // 3, W - W // 3), d_near=1.0, d_far=-100.0, seed=3)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))).cuda()
    if kind == 'full':
        return dev(s['view']), dev(np.ones((H, W), np.float32)), None, dict(focus='value', focus_value=-100.0)
    return dev(s['view']), dev(s['disparity']), dev(s['mask']), dict(focus='mask_mean')


def calls(view, disp, mask, radius, focus):
    """(plan, render, outputs): the two C calls of ops.refocus as closures over one set of buffers."""
    from dualpixelface_amd import ops
    B, _, H, W = view.shape
    L = ops.lib()
    nbytes = L.call('dpf_refocus_workspace_bytes', B, H, W)
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=view.device)
    out = {'refocused': torch.empty_like(view), 'defocus': torch.empty_like(disp), 'refocus_stats': torch.empty(B, 8, dtype=torch.float64, device=view.device)}
    norm = ops._normalizer_floats()
    p = ops._ptr

    def plan():
        L.call('dpf_refocus_plan', p(disp), H * W, 0, None, p(mask), B, H, W, ops.REFOCUS_FOCUS[focus['focus']], 0, 0, float(focus.get('focus_value', 0.0)),
               4.0, radius, 0, p(ws), nbytes, p(out['defocus']), p(out['refocus_stats']), ops._stream())

    def render():
        L.call('dpf_refocus_render', p(view), 1, norm, p(out['defocus']), p(out['refocus_stats']), B, H, W, radius, 2.2, 1.0, p(ws), nbytes,
               p(out['refocused']), ops._stream())
    return plan, render, out


def torch_render(view, disp, defocus, radius, gamma=2.2):
    """The render in tensor operations: unfold of the (2 radius + 1)^2 window over linear RGB, r and d (near sign +1, every d finite)."""
    import torch.nn.functional as F
    from dualpixelface_amd.facedp import IMAGENET_MEAN, IMAGENET_STD
    B, _, H, W = view.shape
    k = 2 * radius + 1
    mean = torch.tensor(IMAGENET_MEAN, device=view.device).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=view.device).view(1, 3, 1, 1)
    lin = (view * std + mean).clamp(0, 1).pow(gamma)
    r = defocus.abs().unsqueeze(1)
    win = lambda x, fill: F.unfold(F.pad(x, (radius,) * 4, value=fill), k).view(B, x.shape[1], k * k, H, W)
    rq, dq, Lq = win(r, -1.0), win(disp.unsqueeze(1), 0.0), win(lin, 0.0)
    off = torch.arange(-radius, radius + 1, device=view.device, dtype=torch.float32)
    dist = (off.view(-1, 1) ** 2 + off.view(1, -1) ** 2).sqrt().view(1, 1, k * k, 1, 1)
    reff = torch.where(dq < disp.view(B, 1, 1, H, W), torch.minimum(rq, r.unsqueeze(2)), rq)
    w = (reff + 1 - dist).clamp(0, 1) / (math.pi * reff * reff).clamp_min(1)
    return ((w * Lq).sum(2) / w.sum(2)).pow(1 / gamma).clamp(0, 1)


def forward_time(shape, reps, rounds, block):
    from dualpixelface_amd import load_option
    from dualpixelface_amd.config import Option
    from dualpixelface_amd.plugin import STEREODPNET
    from dualpixelface_amd.recipe import fill_by_recipe, synthetic_batch
    B, H, W = shape
    opt = load_option('eval_faceDP')
    if block is not None:
        opt.refocus = Option(dict(block))
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
    ap.add_argument('--radii', default='8,16,32')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--torch_shape', default='1,128,192')
    ap.add_argument('--torch_radius', type=int, default=8)
    ap.add_argument('--forward_shape', default='1,1024,1536')
    ap.add_argument('--forward_reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'refocus_timings.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'refocus_bench needs an MI355X'
    radii = [int(v) for v in args.radii.split(',')]
    lines = ['Refocus block: python tools/refocus_bench.py --shapes %s --radii %s --reps %d --rounds %d --torch_shape %s --torch_radius %d '
             '--forward_shape %s --forward_reps %d' % (args.shapes, args.radii, args.reps, args.rounds, args.torch_shape, args.torch_radius,
                                                      args.forward_shape, args.forward_reps),
             'One MI355X (gfx950), one process.  aperture 4, gamma 2.2, gain 1.  "full": every pixel at r = max_radius.  "portrait": the middle '
             'third of the width in focus, the rest at r = max_radius.', '',
             'Device time, median of %d rounds (min, max): %d calls captured into one graph and replayed between two events, per call; the '
             'planes repeat, so they come from the caches, not from HBM.' % (args.rounds, args.reps),
             'Taps per second are counted against the worst case B H W (2 R + 1)^2, whatever the tiles actually walked.']
    for shape in args.shapes.split(':'):
        B, H, W = (int(v) for v in shape.split(','))
        for radius in radii:
            full = None
            for kind in ('full', 'portrait'):
                view, disp, mask, focus = operands(B, H, W, kind)
                plan, render, out = calls(view, disp, mask, radius, focus)
                plan(), render()
                tp = bench_support.replayed(plan, args.reps, args.rounds)
                tr = bench_support.replayed(render, args.reps, args.rounds)
                taps = B * H * W * (2 * radius + 1) ** 2
                med = statistics.median(tr)
                full = med if kind == 'full' else full
                c = out['defocus']
                lines.append('%-11s R %2d %-8s plan (4 launches) %s | render (1 launch) %s | %.2f G taps worst case = %.2f T taps/s%s | '
                             'share of pixels at r = R %.2f, at r = 0 %.2f'
                             % ('%dx%dx%d' % (B, H, W), radius, kind, fmt(tp), fmt(tr), taps / 1e9, taps / (med * 1e-3) / 1e12,
                                '' if kind == 'full' else ' | full / portrait %.2fx' % (full / med),
                                float((c.abs() == radius).float().mean()), float((c == 0).float().mean())))
                print(lines[-1], flush=True)
    B, H, W = (int(v) for v in args.torch_shape.split(','))
    view, disp, mask, focus = operands(B, H, W, 'portrait')
    plan, render, out = calls(view, disp, mask, args.torch_radius, focus)
    plan(), render()
    tor = lambda: torch_render(view, disp, out['defocus'], args.torch_radius)
    agree = float((tor() - out['refocused']).abs().max())
    tr = bench_support.replayed(render, args.reps, args.rounds)
    tt = bench_support.rounds_of((tor,), args.reps, args.rounds)[0]
    lines += ['', 'For scale, the same render in torch (unfold of the window over five planes, eager) at %dx%dx%d, R %d, portrait: hip, graph replay %s | '
              'torch, eager %s | torch / hip %.0fx | max |hip - torch| %.1e' % (B, H, W, args.torch_radius, fmt(tr), fmt(tt),
                                                                               statistics.median(tt) / statistics.median(tr), agree)]
    print(lines[-1], flush=True)
    fs = tuple(int(v) for v in args.forward_shape.split(','))
    lines += ['', 'STEREODPNET evaluation forward (eval_faceDP), synthetic batch %dx%dx%d, %d forwards between two events, median of %d rounds:'
              % (fs + (args.forward_reps, args.rounds))]
    try:
        t0 = forward_time(fs, args.forward_reps, args.rounds, None)
        t1 = forward_time(fs, args.forward_reps, args.rounds, dict(enabled=True))
        lines.append('block off      %s' % fmt(t0))
        lines.append('block on       %s  (+ %.3f ms = %.2f %% of the forward; the defaults: mask_mean focus, aperture 4, max_radius 16)'
                     % (fmt(t1), statistics.median(t1) - statistics.median(t0), 100 * (statistics.median(t1) - statistics.median(t0)) / statistics.median(t0)))
    except Exception as e:                                   # (the forward at this size may not fit: the share is then not measured)
        lines.append('not measured: %s: %s' % (type(e).__name__, str(e).splitlines()[0][:200]))
    lines += ['', 'Not measured: the forward with the block off against a build of the parent commit in alternating processes (with the block off '
              'the forward makes no call it did not make before, which the tests assert on its keys and bits);', 'kernel times from a profiler '
              'trace; HBM-resident planes; occupancy and LDS bank conflict counters of the render; other tile shapes or more than one receiver per lane.']
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
