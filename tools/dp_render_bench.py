#!/usr/bin/env python3
"""The dual-pixel renderer (csrc/dp_render.hip, ops.dp_render): device time of the plan and of the two-view render beside ops.refocus's
one-view render at the same radii, the agreement of the photometric term with the rendering's shift, and whether DPNet learns from
rendered batches.

    python tools/dp_render_bench.py [--shapes 1,1024,1536:4,1024,1536] [--radii 8,16,32] [--reps 5] [--rounds 5] [--out profiles/dp_render_timings.txt]
    python tools/dp_render_bench.py --agreement [--config train_faceDP_dpnet_photometric]
    python tools/dp_render_bench.py --learn N [--config train_faceDP_dpnet_rendered] [--lr 1e-4]

(default)    Scenes.  "full": every pixel at r = max_radius (the worst case: every tile walks the whole window).  "face": the face scene
             of dualpixelface_amd/synthetic_dp.py under the block's defaults (d in [-1.5, 2], r up to 4.2: a window of 11 x 11 at most,
             whatever max_radius allows).  The plan and the render are warmed up, then `reps` calls are captured into one graph and
             replayed between two events, median of `rounds` rounds (min, max): the device time of a call.  The comparison is
             dpf_refocus_render on a frame at r = max_radius everywhere (the "full" scene of tools/refocus_bench.py), measured in this
             process right after the dual-pixel render of the same shape and radius; the ratio is the cost of the second view.
--agreement  the mean photometric term at the true d (pred = batch['disp']) on a rendered 2 x 64 x 96 face batch for shift in
             {(0, +-1), (0, +-2), (+-1, 0), (+-2, 0)} and under zero displacement, as tools/photometric_bench.py --agreement prints it.
--learn N    DPNet under --config (the dp_render block switched on over it, so the label-free train_faceDP_dpnet_photometric works too) trained for N steps at 2 x 64 x 96, a fresh rendered batch per step, lr = --lr or the config's init_lr; prints
             the mean |pred - disp| over the mask on 4 held-out scenes before and after.  A measurement, not a test.

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


def operands(B, H, W, kind, radius):
    """(image, disparity) on the device: one scene repeated over the batch."""
    from dualpixelface_amd import ops, synthetic_dp
    s = synthetic_dp.face_scene(H, W, seed=3)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))).cuda()     # noqa: E731
    if kind == 'full':
        d = np.full((H, W), (radius + 1.0) / ops.dp_render_radius_scale(ops.DP_RENDER_SHIFT), np.float32)
        return dev(s['center']), dev(d)
    return dev(s['center']), dev(s['disp'])


def calls(image, disp, radius):
    """(plan, render, outputs): the two C calls of ops.dp_render as closures over one set of buffers."""
    from dualpixelface_amd import ops
    B, _, H, W = image.shape
    L = ops.lib()
    nbytes = L.call('dpf_dp_render_workspace_bytes', B, H, W)
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=image.device)
    out = {'reference': torch.empty_like(image), 'target': torch.empty_like(image), 'radius': torch.empty_like(disp),
           'dp_stats': torch.empty(B, ops.DP_RENDER_STATS, dtype=torch.float64, device=image.device)}
    norm, p = ops._normalizer_floats(), ops._ptr
    sx, sy = ops.DP_RENDER_SHIFT
    rho = ops.dp_render_radius_scale(ops.DP_RENDER_SHIFT)

    def plan():
        L.call('dpf_dp_render_plan', p(disp), B, H, W, rho, radius, p(ws), nbytes, p(out['radius']), p(out['dp_stats']), ops._stream())

    def render():
        L.call('dpf_dp_render', p(image), 1, norm, p(disp), p(out['radius']), B, H, W, sx, sy, radius, 1, 2.2, 1, p(ws), nbytes, p(out['reference']),
               p(out['target']), ops._stream())
    return plan, render, out


def refocus_render(image, radius):
    """dpf_refocus_render on a frame at r = max_radius everywhere, planned once -> the render call as a closure."""
    from dualpixelface_amd import ops
    B, _, H, W = image.shape
    L = ops.lib()
    disp = torch.ones(B, H, W, device=image.device)
    nbytes = L.call('dpf_refocus_workspace_bytes', B, H, W)
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=image.device)
    defocus, stats, out = torch.empty_like(disp), torch.empty(B, 8, dtype=torch.float64, device=image.device), torch.empty_like(image)
    norm, p = ops._normalizer_floats(), ops._ptr
    L.call('dpf_refocus_plan', p(disp), H * W, 0, None, None, B, H, W, ops.REFOCUS_FOCUS['value'], 0, 0, -100.0, 4.0, radius, 0, p(ws), nbytes,
           p(defocus), p(stats), ops._stream())

    def render():
        L.call('dpf_refocus_render', p(image), 1, norm, p(defocus), p(stats), B, H, W, radius, 2.2, 1.0, p(ws), nbytes, p(out), ops._stream())
    render()
    assert float(defocus.abs().min()) == radius
    return render, (ws, defocus, stats, out)


def timings(args):
    radii = [int(v) for v in args.radii.split(',')]
    lines = ['Dual-pixel renderer: python tools/dp_render_bench.py --shapes %s --radii %s --reps %d --rounds %d' % (args.shapes, args.radii, args.reps, args.rounds),
             'One MI355X (gfx950), one process.  shift (0, -2), rho = (3 pi / 8) |shift|, gamma 2.2, normalised in and out.  "full": every pixel at '
             'r = max_radius.  "face": the face scene, d in [-1.5, 2] (r <= 4.2).', '',
             'Device time, median of %d rounds (min, max): %d calls captured into one graph and replayed between two events, per call; the '
             'planes repeat, so they come from the caches, not from HBM.' % (args.rounds, args.reps),
             'refocus: dpf_refocus_render (one view) on a frame at r = max_radius everywhere, same shape and radius, measured in this process '
             'right after.  Taps per second are counted against the worst case B H W (2 R + 1)^2.']
    for shape in args.shapes.split(':'):
        B, H, W = (int(v) for v in shape.split(','))
        for radius in radii:
            for kind in ('full', 'face'):
                image, disp = operands(B, H, W, kind, radius)
                plan, render, out = calls(image, disp, radius)
                plan(), render()
                tp = bench_support.replayed(plan, args.reps, args.rounds)
                tr = bench_support.replayed(render, args.reps, args.rounds)
                med = statistics.median(tr)
                taps = B * H * W * (2 * radius + 1) ** 2
                tail = ''
                if kind == 'full':
                    one, keep = refocus_render(image, radius)
                    t1 = bench_support.replayed(one, args.reps, args.rounds)
                    tail = ' | refocus render (1 view) %s | two views / one view %.2fx' % (fmt(t1), med / statistics.median(t1))
                c = out['radius']
                lines.append('%-11s R %2d %-5s plan (2 launches) %s | render (1 launch, 2 views) %s | %.2f G taps worst case = %.2f T taps/s | '
                             'largest r %.2f%s' % ('%dx%dx%d' % (B, H, W), radius, kind, fmt(tp), fmt(tr), taps / 1e9, taps / (med * 1e-3) / 1e12,
                                                  float(c.abs().max()), tail))
                print(lines[-1], flush=True)
    lines += ['', 'Not measured: kernel times from a profiler trace; HBM-resident planes; occupancy and LDS bank conflict counters; other tile shapes, '
              'more than one receiver per lane, or one launch per view; the loader against worker processes.']
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)
    print('written to', args.out)


def rendered_option(config):
    """The config with its dp_render block switched on (added with the defaults where the config has none)."""
    from dualpixelface_amd import dp_render, load_option
    from dualpixelface_amd.config import Option
    opt = load_option(config)
    opt.dp_render = Option(dict(dp_render.settings(opt)._asdict(), enabled=True, shift=None))
    return opt


CANDIDATES = ((0.0, 1.0), (0.0, -1.0), (0.0, 2.0), (0.0, -2.0), (1.0, 0.0), (-1.0, 0.0), (2.0, 0.0), (-2.0, 0.0))


def agreement(args):
    from dualpixelface_amd import dp_render, load_option, ops, photometric, synthetic_dp
    from dualpixelface_amd.core import reference_key
    opt = rendered_option(args.config)
    s, ph = dp_render.settings(opt), photometric.settings(opt)
    batch = synthetic_dp.rendered_batch(2, 64, 96, seed=3, option=opt)
    key = reference_key(opt)
    ref, tgt = batch[key], batch['left' if key == 'right' else 'right']
    pred = batch['disp'].unsqueeze(1).contiguous()
    print('photometric agreement on a rendered 2x64x96 face batch (%s: rendered under shift %s, d in %s; alpha %g, eps %g)'
          % (args.config, list(s.shift), list(s.d_range), ph.alpha, ph.charbonnier_eps))
    term = lambda p, shift: float(ops.photometric_loss(p, ref, tgt, shift=shift, alpha=ph.alpha, eps=ph.charbonnier_eps))     # noqa: E731
    rows = [('shift (%+g, %+g)' % c, term(pred, c)) for c in CANDIDATES] + [('zero displacement', term(torch.zeros_like(pred), s.shift))]
    rows += [('shift (%+g, %+g) at %.1f d' % (s.shift + (k,)), term((pred * k).contiguous(), s.shift)) for k in (0.5, 1.5)]
    for name, v in rows:
        print('  %-28s mean term %.5f' % (name, v))
    nine = sorted(rows[:9], key=lambda r: r[1])
    print('smallest: %s; next smallest / smallest %.2f' % (nine[0][0], nine[1][1] / nine[0][1]))


def learn(args):
    from dualpixelface_amd import dp_render, load_option, synthetic_dp
    from dualpixelface_amd.plugin import DPNET
    from dualpixelface_amd.recipe import fill_by_recipe
    opt = rendered_option(args.config)
    model = DPNET(opt)
    fill_by_recipe(model)
    model.to('cuda')
    held = synthetic_dp.rendered_batch(4, 64, 96, seed=900001, option=opt)

    def error():
        model.eval()
        with torch.no_grad():
            pred = model.forward(dict(held))['pred_depth']
        pred = pred[:, 0] if pred.dim() == 4 else pred
        m = held['mask'] > 0
        return float((pred - held['disp']).abs()[m].mean()), float((pred - held['disp']).abs().mean())
    before = error()
    lr = float(args.lr if args.lr is not None else opt.init_lr)
    static, losses = None, []
    for step in range(args.learn):
        batch = synthetic_dp.rendered_batch(2, 64, 96, seed=step, option=opt)
        if static is None:
            static = {k: v.clone() for k, v in batch.items()}
        for k in static:
            static[k].copy_(batch[k])
        losses.append(model.train_step(static, None, lr=lr)['final_loss'])
    losses = [float(v) for v in losses]
    after = error()
    k = max(1, len(losses) // 10)
    print('dpnet (%s) at 2x64x96 on rendered batches, %d steps, lr %g: final_loss first %d steps %.4f, last %d steps %.4f'
          % (args.config, args.learn, lr, k, statistics.mean(losses[:k]), k, statistics.mean(losses[-k:])))
    print('mean |pred - disp| on 4 held-out scenes, over the mask: before %.4f, after %.4f; over every pixel: before %.4f, after %.4f  '
          '(d spans %s; predicting the mean of d over the mask would leave %.4f)'
          % (before[0], after[0], before[1], after[1], list(dp_render.settings(opt).d_range),
             float((held['disp'] - held['disp'][held['mask'] > 0].mean()).abs()[held['mask'] > 0].mean())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='1,1024,1536:4,1024,1536')
    ap.add_argument('--radii', default='8,16,32')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dp_render_timings.txt'))
    ap.add_argument('--agreement', action='store_true')
    ap.add_argument('--learn', type=int, default=0)
    ap.add_argument('--config', default=None)
    ap.add_argument('--lr', type=float, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'dp_render_bench needs an MI355X'
    if args.agreement:
        args.config = args.config or 'train_faceDP_dpnet_photometric'
        return agreement(args)
    if args.learn:
        args.config = args.config or 'train_faceDP_dpnet_rendered'
        return learn(args)
    timings(args)


if __name__ == '__main__':
    main()
