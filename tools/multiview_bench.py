#!/usr/bin/env python3
"""Multi-view photometric loss (loss_type 'multiview', csrc/multiview.hip): convention agreement, kernel timings, share of the train step.

    python tools/multiview_bench.py --agreement [--config train_faceDP_dpnet_multiview] [--loader]
    python tools/multiview_bench.py [--reps 100] [--rounds 3] [--out profiles/multiview_timings.txt]
    python tools/multiview_bench.py --step [--config train_faceDP_dpnet_multiview] [--root DIR]
    python tools/multiview_bench.py --occlusion [--reps 100] [--rounds 3] [--out profiles/multiview_occlusion_timings.txt]

--agreement  prints the mean term under the depth the batch brings (pred = batch['depth'], target type 'depth') for the pose matrices as
             stored and inverted (P and Ps both), and for the depth in its units, x1e-3 and x1e3: the combination whose term is the
             smallest, and clearly below the others, is the one the data was recorded with.  The batch is the first of the config's
             training loader with --loader (needs the dataset), else the synthetic plane scene, whose answer (as stored, x1) only proves
             the tool.
(default)    forward and backward of ops.multiview_loss at 4x1x1024x1536 with S = 3 neighbours of 1280x1920 and at 2x5x256x384 (DPNet's
             five heads), beside ops.photometric_loss at the same shapes (the same window work without the projective gather and with one
             view): each warmed up, `reps` calls between two events on one stream, median of `rounds` rounds with min and max.  Then the
             captured DPNet step at 2x256x384 with the shipped multiview config on the synthetic multi-view batch against
             train_faceDP_dpnet on the plain synthetic batch, alternating.  A call is enqueued from Python launch by launch, so its time
             is an upper bound of the device time.
--step       one line: the median time of the captured DPNet train step at 2x256x384 under --config, package imported from --root (so
             the same script times another checkout of the project; a config without use_multi steps on the plain synthetic batch).
--occlusion  the occlusion modes (reduce 'min', visibility 'zbuffer', both) against the plain call at the two shapes above in one process,
             the sides alternating; the z-buffer pre-pass (dpf_multiview_zbuffer: fill + splat) on its own; the captured DPNet step under
             train_faceDP_dpnet_multiview_occlusion against train_faceDP_dpnet_multiview, alternating; and on the occluder scene
             (synthetic_multiview.occluder_sample) at the true depth the loss of every mode with the share of pixels each view sees and
             wins.
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
DEFAULT_OUT = os.path.join(ROOT, 'profiles', 'multiview_timings.txt')


def captured_step(config, H, W):
    """DPNET under `config` stepped until the step is captured -> a callable that replays it.  Under use_multi the batch is the
    synthetic multi-view one without its label maps, else recipe.synthetic_batch."""
    from dualpixelface_amd import load_option
    from dualpixelface_amd.plugin import DPNET
    from dualpixelface_amd.recipe import fill_by_recipe, synthetic_batch
    opt = load_option(config)
    model = DPNET(opt)
    fill_by_recipe(model)
    model.to('cuda').train()
    if getattr(opt, 'use_multi', False):
        from dualpixelface_amd import multiview
        from dualpixelface_amd.synthetic_multiview import synthetic_multiview_batch
        batch = synthetic_multiview_batch(2, H, W, views=multiview.settings(opt).select_view, seed=7, device='cuda')
        batch = {k: v for k, v in batch.items() if k not in ('disp', 'depth', 'idepth', 'normal')}
    else:
        batch = {k: v.cuda() for k, v in synthetic_batch(2, H, W, seed=7, mask_mode='bern').items()}
    for _ in range(5):                                             # two warm-up steps, the capture, two replays
        model.train_step(batch, None, lr=1e-4)
    assert model._graph_state.get('graph') is not None, 'the step was not captured'
    return lambda: model.train_step(batch, None, lr=1e-4)


def scene(B, n, H, W, views, device='cuda'):
    """The synthetic plane scene with every head predicting the true depth plus a ripple of 0.5 %."""
    from dualpixelface_amd.synthetic_multiview import synthetic_multiview_batch
    b = synthetic_multiview_batch(B, H, W, views=views, seed=3, device=device)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=device), torch.arange(W, dtype=torch.float32, device=device), indexing='ij')
    b['pred'] = torch.stack([b['depth'] * (1 + 0.005 * torch.sin(xs / (7.0 + h)) * torch.cos(ys / (9.0 + h))) for h in range(n)], 1).contiguous()
    Hs, Ws = b['centers'].shape[2:]
    b['src'] = b['centers'].view(B, views, 3, Hs, Ws)
    return b


def agreement(args):
    from dualpixelface_amd import load_option, multiview, ops
    opt = load_option(args.config)
    s = multiview.settings(opt)
    if args.loader:
        from dualpixelface_amd.plugin import DPNET
        sys.path.insert(0, ROOT)
        os.chdir(ROOT)
        batch = next(iter(DPNET(opt).train_dataloader()))
        batch = {k: (v.cuda().float() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch.items()}
        what = 'the first training batch of %s' % args.config
    else:
        batch, what = scene(2, 1, 256, 384, s.select_view), 'the synthetic plane scene'
    S = s.select_view
    B, _, Hs, Ws = batch['centers'].shape
    src = batch['centers'][:, :3 * S].view(B, S, 3, Hs, Ws)
    depth = batch['depth'][:, None].contiguous()
    print('multiview agreement on %s (select_view %d, weight_ssim %g, alpha %g, scale %g)' % (what, S, s.weight_ssim, s.alpha, s.scale))

    def term(P, Ps, unit):
        loss, _, counted, _, _, _ = ops.multiview_loss(depth * unit, batch['center'], src, batch['K'], P, batch['Ks'][:, :S], Ps, mask=batch.get('mask'),
                                                       target_type='depth', weight_ssim=s.weight_ssim, alpha=s.alpha, scale=s.scale,
                                                       min_depth=s.min_depth, return_warped=True)
        return float(loss), int(counted.sum()), counted.numel()

    P, Ps = batch['P'], batch['Ps'][:, :S].contiguous()
    inverted = lambda m: torch.linalg.inv(m.cpu().double()).float().to(m.device)                   # noqa: E731
    rows = [('P %s, depth x%g' % (name, unit), term(p, ps, unit))
            for name, p, ps in (('as stored', P, Ps), ('inverted', inverted(P), inverted(Ps))) for unit in (1.0, 1e-3, 1e3)]
    best = min(rows, key=lambda r: r[1][0] if r[1][1] else math.inf)
    for name, (loss, cnt, total) in rows:
        print('  %-28s mean term %.6f over %d of %d pixels%s' % (name, loss, cnt, total, '   <- smallest' if name == best[0] else ''))


OCC_MODES = (('min', dict(reduce='min')), ('zbuffer', dict(visibility='zbuffer')), ('min + zbuffer', dict(reduce='min', visibility='zbuffer')))


def occlusion(args):
    from dualpixelface_amd import ops
    from dualpixelface_amd._lib import lib
    from dualpixelface_amd.synthetic_multiview import occluder_sample
    lines = ['Multi-view loss, occlusion handling: python tools/multiview_bench.py --occlusion --reps %d --rounds %d' % (args.reps, args.rounds),
             'One MI355X (gfx950), one process.  ops.multiview_loss on the synthetic plane scene with S = 3 neighbours whose images are 1.25 x',
             'the target\'s, target type depth, cell 2, tolerance 0.01: the plain call (mean / none) and the three occlusion modes, %d calls' % args.reps,
             'between two events on one stream, the sides alternating, median of %d rounds (min, max); enqueued from Python launch by' % args.rounds,
             'launch, so an upper bound of the device time.  zbuffer pre-pass: dpf_multiview_zbuffer alone (fill + splat, two launches).', '']
    for B, n, H, W in ((4, 1, 1024, 1536), (2, 5, 256, 384)):
        sc = scene(B, n, H, W, 3)
        pred = sc['pred'].requires_grad_()
        weights = WEIGHTS[:n] if n > 1 else [1.0]
        call = lambda kw: ops.multiview_loss(pred, sc['center'], sc['src'], sc['K'], sc['P'], sc['Ks'], sc['Ps'], mask=sc['mask'],   # noqa: E731
                                             head_weights=weights, target_type='depth', **kw)
        names, sides, notes = [], [], []
        for name, kw in (('mean / none', {}),) + OCC_MODES:
            fwd = lambda kw=kw: call(kw)                                                            # noqa: E731
            loss = fwd()
            bwd = lambda loss=loss: torch.autograd.grad(loss, pred, retain_graph=True)[0]           # noqa: E731
            grad = bwd()
            assert math.isfinite(float(loss)) and bool(torch.isfinite(grad).all())
            names += [name + ' forward', name + ' backward']
            sides += [fwd, bwd]
            notes += [' | loss %.6f' % float(loss), ' | max |d pred| %.3e' % float(grad.abs().max())]
        S, Hs, Ws = sc['src'].shape[1], sc['src'].shape[3], sc['src'].shape[4]
        rig = ops.multiview_rig(sc['K'], sc['P'], sc['Ks'], sc['Ps'])
        zbuf = torch.empty((B, n, S, -(-Hs // 2), -(-Ws // 2)), dtype=torch.float32, device='cuda')
        held = (pred.detach().contiguous(), sc['mask'].contiguous())
        names.append('zbuffer pre-pass')
        sides.append(lambda: lib().call('dpf_multiview_zbuffer', ops._ptr(held[0]), ops._ptr(rig), None, ops._ptr(held[1]), B, n, S, H, W, Hs, Ws,
                                        ops.TARGET_TYPES['depth'], 1e-3, 2, ops._ptr(zbuf), ops._stream()))
        sides[-1]()
        notes.append(' | %d of %d cells hit' % (int(torch.isfinite(zbuf).sum()), zbuf.numel()))
        for name, t, note in zip(names, bench_support.rounds_of(sides, args.reps, args.rounds, warm=5), notes):
            lines.append(_row(name, (B, n, H, W), t, note))
        lines.append('')
    lines += ['Captured DPNet train step at 2x256x384 (fp32) on the synthetic multi-view batch without its label maps:',
              'train_faceDP_dpnet_multiview (mean / none) against train_faceDP_dpnet_multiview_occlusion (min + zbuffer), %d replays between' % args.reps,
              'two events, alternating, %d rounds:' % args.rounds]
    tp, to = bench_support.rounds_of((captured_step('train_faceDP_dpnet_multiview', 256, 384),
                                      captured_step('train_faceDP_dpnet_multiview_occlusion', 256, 384)), args.reps, args.rounds)
    mp, mo = statistics.median(tp), statistics.median(to)
    lines.append('mean / none %s | min + zbuffer %s | %+.4f ms = %+.2f %% of the step'
                 % (bench_support.fmt(tp, 4), bench_support.fmt(to, 4), mo - mp, 100.0 * (mo - mp) / mp))
    s = occluder_sample(48, 64, 2)
    dev = lambda k: s[k][None].cuda()                                                              # noqa: E731
    Hs, Ws = s['centers'].shape[1:]
    src = dev('centers').view(1, 2, 3, Hs, Ws)
    pred = dev('depth')[:, None].contiguous()
    lines += ['', 'The occluder scene (48x64, two opposed views) at the true depth, cell 2, tolerance 0.01; closed form: view 0 sees %.1f %% of the'
              % (100.0 * s['visible'][0].mean()), 'target\'s pixels, view 1 %.1f %%:' % (100.0 * s['visible'][1].mean())]
    for name, kw in (('mean / none', {}),) + OCC_MODES:
        out = ops.multiview_loss(pred, dev('center'), src, dev('K'), dev('P'), dev('Ks'), dev('Ps'), target_type='depth', return_warped=True, **kw)
        row = '%-14s loss %.6e | counted per view %s' % (name, float(out[0]), out[2].sum(dim=(0, 1, 3, 4)).tolist())
        if kw:
            row += ' | seen per view %s %%' % ['%.1f' % v for v in (100.0 * out[6].float().mean(dim=(0, 1, 3, 4))).tolist()]
        if 'reduce' in kw:
            row += ' | selected per view %s %%, none %.1f %%' % (['%.1f' % (100.0 * float((out[7] == v).float().mean())) for v in range(2)],
                                                               100.0 * float((out[7] == 255).float().mean()))
        lines.append(row)
    text = '\n'.join(lines) + '\n'
    print(text)
    out = args.out if args.out != DEFAULT_OUT else os.path.join(ROOT, 'profiles', 'multiview_occlusion_timings.txt')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        f.write(text)


def _row(tag, shape, times, extra=''):
    return '%-16s %-22s %s%s' % ('x'.join(str(v) for v in shape), tag, bench_support.fmt(times, 4), extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--agreement', action='store_true')
    ap.add_argument('--config', default='train_faceDP_dpnet_multiview')
    ap.add_argument('--loader', action='store_true')
    ap.add_argument('--step', action='store_true')
    ap.add_argument('--root', default=ROOT)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--occlusion', action='store_true')
    ap.add_argument('--out', default=DEFAULT_OUT)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'multiview_bench needs an MI355X'
    if args.step:
        sys.path.insert(0, os.path.abspath(args.root))
        return bench_support.step_line('config %s' % args.config, captured_step(args.config, 256, 384), args.reps, args.rounds, args.root)
    sys.path.insert(0, ROOT)
    if args.agreement:
        return agreement(args)
    if args.occlusion:
        return occlusion(args)
    from dualpixelface_amd import ops
    lines = ['Multi-view photometric loss: python tools/multiview_bench.py --reps %d --rounds %d' % (args.reps, args.rounds),
             'One MI355X (gfx950), one process.  ops.multiview_loss (csrc/multiview.hip: rig + 3 launches forward, 1 backward) on the synthetic',
             'plane scene with S = 3 neighbours whose images are 1.25 x the target\'s, target type depth, beside ops.photometric_loss',
             '(csrc/photometric.hip, 3 + 1 launches, one view) on the target image and the first neighbour\'s crop; %d calls between two' % args.reps,
             'events on one stream, median of %d rounds (min, max); enqueued from Python launch by launch, so an upper bound of the' % args.rounds,
             'device time.', '']
    for B, n, H, W in ((4, 1, 1024, 1536), (2, 5, 256, 384)):
        sc = scene(B, n, H, W, 3)
        pred = sc['pred'].requires_grad_()
        weights = WEIGHTS[:n] if n > 1 else [1.0]
        crop = sc['src'][:, 0, :, :H, :W].contiguous()
        flat = (pred.detach() * 0 + 0.5).requires_grad_()
        ops_ = (('multiview S=3', pred, lambda: ops.multiview_loss(pred, sc['center'], sc['src'], sc['K'], sc['P'], sc['Ks'], sc['Ps'],
                                                                   mask=sc['mask'], head_weights=weights, target_type='depth')),
                ('photometric', flat, lambda: ops.photometric_loss(flat, sc['center'], crop, mask=sc['mask'], head_weights=weights)))
        for name, leaf, fwd in ops_:
            loss = fwd()
            bwd = lambda: torch.autograd.grad(loss, leaf, retain_graph=True)[0]                    # noqa: E731
            grad = bwd()
            assert math.isfinite(float(loss)) and bool(torch.isfinite(grad).all())
            tf, tb = bench_support.rounds_of((fwd, bwd), args.reps, args.rounds, warm=5)
            lines.append(_row(name + ' forward', (B, n, H, W), tf, ' | loss %.6f' % float(loss)))
            lines.append(_row(name + ' backward', (B, n, H, W), tb, ' | max |d pred| %.3e' % float(grad.abs().max())))
    lines += ['', 'Captured DPNet train step at 2x256x384 (fp32): train_faceDP_dpnet (loss_type [smoothL1], the plain synthetic batch) against',
              'train_faceDP_dpnet_multiview (loss_type [multiview], the synthetic multi-view batch without its',
              'label maps), %d replays between two events, alternating, %d rounds:' % (args.reps, args.rounds)]
    tp, to = bench_support.rounds_of((captured_step('train_faceDP_dpnet', 256, 384), captured_step('train_faceDP_dpnet_multiview', 256, 384)),
                                     args.reps, args.rounds)
    mp, mo = statistics.median(tp), statistics.median(to)
    lines.append('smoothL1 %s | multiview %s | %+.4f ms = %+.2f %% of the step'
                 % (bench_support.fmt(tp, 4), bench_support.fmt(to, 4), mo - mp, 100.0 * (mo - mp) / mp))
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
