#!/usr/bin/env python3
"""Geometric-normal loss (loss_type 'normal_geo', csrc/normal_geo.hip): frame agreement, kernel timings, share of the train step.

    python tools/normal_geo_bench.py --agreement [--config train_faceDP_dpnet_normal_geo] [--loader]
    python tools/normal_geo_bench.py [--reps 100] [--rounds 3] [--out profiles/normal_geo_timings.txt]
    python tools/normal_geo_bench.py --step [--losses smoothL1,normal_geo] [--root DIR]

--agreement  prints the mean cosine between the normals of batch['depth'] ITSELF and batch['normal'] under the config's normal_geo
             settings: near +1 when towards_camera / target_signs match the frame the normals are stored in, near -1 or 0 when they do
             not.  The batch is the first of the config's training loader with --loader (needs the dataset), else a synthetic smooth
             surface whose normals are its own, so the synthetic answer only proves the tool.
(default)    forward + backward of ops.normal_geo_loss at 4x1x1024x1536 and 2x5x256x384 against the same definition written as torch
             expressions on the device, under autograd: each side warmed up, `reps` calls between two events on one stream, the sides
             alternating for `rounds` rounds, median with min and max.  Then the captured DPNet step at 2x256x384 with and without the
             loss, alternating, three rounds.  A hip call is enqueued from Python launch by launch, so its time is an upper bound of the
             device time.
--step       one line: the median time of the captured DPNet train step at 2x256x384 with the given loss_type, package imported from
             --root (so the same script times another checkout of the project).
Needs a GPU; there is no CPU fallback.
"""
import argparse
import os
import statistics
import sys

import torch

import bench_support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = [1.0, 0.75294, 0.18824, 0.047059, 0.011765]


def _shift(z, dy, dx):
    """z [..., H, W] at (y + dy, x + dx), 0 outside the image."""
    out = torch.zeros_like(z)
    H, W = z.shape[-2:]
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    out[..., yd, xd] = z[..., ys, xs]
    return out


def torch_loss(pred, depth, normal, K, ab, mask, weights, target_type='disp', ratio=0.01, s=1, towards=True, signs=(1, 1, 1)):
    """The definition of DESIGN.md section 7 as torch expressions on the device (fp32, no attention to the association order)."""
    B, n, H, W = pred.shape
    inv = torch.linalg.inv(K.double()).float()
    ys, xs = torch.meshgrid(torch.arange(H, device=pred.device, dtype=torch.float32), torch.arange(W, device=pred.device, dtype=torch.float32),
                            indexing='ij')

    def rays(dy, dx):
        return inv[:, :, 0, None, None] * (xs + dx) + inv[:, :, 1, None, None] * (ys + dy) + inv[:, :, 2, None, None]

    r0, rr, rd = rays(0, 0), rays(0, s), rays(s, 0)
    g = normal * torch.tensor(signs, dtype=torch.float32, device=pred.device).view(1, 3, 1, 1)
    glen = g.norm(dim=1)
    base = torch.isfinite(depth) & (depth > 0)
    if mask is not None:
        base = base & (mask > 0)
    zero = torch.zeros((), device=pred.device)
    loss = 0.0
    for h in range(n):
        with torch.no_grad():
            zr = pred[:, h] if target_type == 'depth' else ab[:, 1, None, None] / (pred[:, h] - ab[:, 0, None, None])
            usable = base & torch.isfinite(zr) & (zr > 0)
            zt = torch.where(usable, depth, zero)

            def conn(a, b):
                return (a > 0) & (b > 0) & ((a - b).abs() <= ratio * torch.minimum(a, b))
            cl, cr = conn(_shift(zt, 0, -s), zt), conn(zt, _shift(zt, 0, s))
            cu, cd = conn(_shift(zt, -s, 0), zt), conn(zt, _shift(zt, s, 0))
        safe = torch.where(usable, pred[:, h], torch.ones((), device=pred.device) + (0 if target_type == 'depth' else ab[:, 0, None, None]))
        z = torch.where(usable, safe if target_type == 'depth' else ab[:, 1, None, None] / (safe - ab[:, 0, None, None]), zero)

        def step(col, cm, cp, zm, zq, rq):
            zfrom, zto = torch.where(cm, zm, z), torch.where(cp, zq, z)
            delta = torch.where(cm & cp, 2.0 * s, 1.0 * s)
            rto = torch.where(cp[:, None], rq, r0)
            return (zto - zfrom)[:, None] * rto + (zfrom * delta)[:, None] * inv[:, :, col, None, None]

        drow = step(0, cl, cr, _shift(z, 0, -s), _shift(z, 0, s), rr)
        dcol = step(1, cu, cd, _shift(z, -s, 0), _shift(z, s, 0), rd)
        c = torch.cross(drow, dcol, dim=1)
        with torch.no_grad():
            length = c.norm(dim=1)
            counted = usable & (cl | cr) & (cu | cd) & (length > 0) & torch.isfinite(length) & (glen > 1e-6) & torch.isfinite(glen)
            dot = (c * (z[:, None] * r0)).sum(1)
            sigma = torch.where((dot > 0) if towards else (dot < 0), -1.0, 1.0)
        c = torch.where(counted[:, None], c, torch.ones((), device=pred.device))
        nn = sigma[:, None] * c / c.norm(dim=1, keepdim=True)
        gh = torch.where(counted[:, None], g, torch.ones((), device=pred.device))
        gh = gh / gh.norm(dim=1, keepdim=True)
        term = 1 - (nn * gh).sum(1).clamp(-1, 1)
        cnt = counted.sum()
        loss = loss + weights[h] * torch.where(cnt > 0, torch.where(counted, term, zero).sum() / cnt.clamp(min=1), zero)
    return loss


def synthetic_surface(B, n, H, W, seed=3, device='cuda'):
    """A smooth surface around 800 mm in front of an f = 2500 px camera, with 0.2 % ripples in every head's prediction, a Bernoulli(0.8) mask
    and target normals that are the surface's own geometric normals (ops.depth_normals of the target depth)."""
    from dualpixelface_amd import ops
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    depth = torch.stack([800.0 + 30.0 * torch.sin(xs / (40.0 + 5 * b)) * torch.cos(ys / 55.0) + 0.02 * xs for b in range(B)])
    ab = torch.tensor([[-4.5, 41000.0]]).repeat(B, 1)
    ripple = torch.stack([1.0 + 0.002 * torch.sin(xs / (7.0 + h)) * torch.cos(ys / (9.0 + h)) for h in range(n)])
    zp = depth[:, None] * ripple[None]
    pred = (ab[:, 0, None, None, None].double() + ab[:, 1, None, None, None].double() / zp).float()
    K = torch.tensor([[2500.0, 0.0, W / 2.0], [0.0, 2500.0, H / 2.0], [0.0, 0.0, 1.0]]).repeat(B, 1, 1)
    mask = (torch.rand(B, H, W, generator=g) < 0.8).float()
    out = {k: v.to(device) for k, v in dict(pred=pred, depth=depth.float(), ab=ab, K=K, mask=mask).items()}
    out['normal'] = ops.depth_normals(out['depth'], out['K'], target_type='depth')[0]
    return out


def agreement(args):
    from dualpixelface_amd import load_option, normal_geo, ops
    opt = load_option(args.config)
    s = normal_geo.settings(opt)
    if args.loader:
        from dualpixelface_amd.plugin import DPNET
        sys.path.insert(0, ROOT)
        os.chdir(ROOT)
        batch = next(iter(DPNET(opt).train_dataloader()))
        batch = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}
        depth, normal, K, mask, what = batch['depth'], batch['normal'], batch['K'], batch.get('mask'), 'the first training batch of %s' % args.config
    else:
        sc = synthetic_surface(2, 1, 256, 384)
        depth, normal, K, mask, what = sc['depth'], sc['normal'], sc['K'], sc['mask'], 'a synthetic surface with its own normals'
    loss, _, counted = ops.normal_geo_loss(depth[:, None].contiguous(), depth, normal, K, mask=mask, target_type='depth',
                                           max_edge_ratio=s.max_edge_ratio, step=s.step, towards_camera=s.towards_camera,
                                           target_signs=s.target_signs, return_normals=True)
    print('normal_geo agreement on %s: mean cosine %.6f over %d of %d pixels (settings %s)'
          % (what, 1.0 - float(loss), int(counted.sum()), counted.numel(), dict(s._asdict())))


def _step_with(losses):
    lambdas = [1.0] + [0.1] * (len(losses) - 1)
    return bench_support.captured_dpnet_step('train_faceDP_dpnet', 256, 384, loss_type=list(losses), lambdas=lambdas)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--agreement', action='store_true')
    ap.add_argument('--config', default='train_faceDP_dpnet_normal_geo')
    ap.add_argument('--loader', action='store_true')
    ap.add_argument('--step', action='store_true')
    ap.add_argument('--losses', default='smoothL1,normal_geo')
    ap.add_argument('--root', default=ROOT)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'normal_geo_timings.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'normal_geo_bench needs an MI355X'
    if args.step:
        sys.path.insert(0, os.path.abspath(args.root))
        return bench_support.step_line('loss_type %s' % args.losses, _step_with(args.losses.split(',')), args.reps, args.rounds, args.root)
    sys.path.insert(0, ROOT)
    if args.agreement:
        return agreement(args)
    from dualpixelface_amd import ops
    lines = ['Geometric-normal loss: python tools/normal_geo_bench.py --reps %d --rounds %d' % (args.reps, args.rounds),
             'One MI355X (gfx950), one process.  Forward + backward per call (ops.normal_geo_loss, csrc/normal_geo.hip: 2 + 1 launches) on a',
             'synthetic smooth surface, disp target, Bernoulli(0.8) mask, step 1; %d calls between two events on one stream, sides alternating,' % args.reps,
             'median of %d rounds (min, max).  "torch" = the same definition as torch expressions under autograd on the same device.' % args.rounds,
             'Traffic: forward reads n + 5 planes per sample (pred, depth, mask, 3 normal), backward reads them again and writes n.', '']
    for B, n, H, W in ((4, 1, 1024, 1536), (2, 5, 256, 384)):
        sc = synthetic_surface(B, n, H, W)
        pred = sc['pred'].requires_grad_()
        weights = WEIGHTS[:n] if n > 1 else [1.0]

        def hip():
            loss = ops.normal_geo_loss(pred, sc['depth'], sc['normal'], sc['K'], ab=sc['ab'], mask=sc['mask'], head_weights=weights)
            return loss, torch.autograd.grad(loss, pred)[0]

        def ref():
            loss = torch_loss(pred, sc['depth'], sc['normal'], sc['K'], sc['ab'], sc['mask'], weights)
            return loss, torch.autograd.grad(loss, pred)[0]

        (lh, gh), (lr, gr) = hip(), ref()
        loss_rel = abs(float(lh.detach()) - float(lr.detach())) / abs(float(lr.detach()))
        grad_rel = float((gh - gr).abs().max() / gr.abs().max())
        for fn in (hip, ref):
            bench_support.timed(fn, 5)
        th, tr = [], []
        for _ in range(args.rounds):
            th.append(bench_support.timed(hip, args.reps))
            tr.append(bench_support.timed(ref, max(args.reps // 10, 3)))
        mh, mr = statistics.median(th), statistics.median(tr)
        nbytes = 4.0 * B * H * W * ((n + 5) + (2 * n + 5))
        lines.append('%dx%dx%dx%d  hip %.4f ms (min %.4f, max %.4f) | torch %.3f ms (min %.3f, max %.3f) | torch / hip %.0fx | %.1f MB -> %.2f TB/s'
                     ' | loss %.6f, rel diff to torch %.1e, grad max diff / max %.1e'
                     % (B, n, H, W, mh, min(th), max(th), mr, min(tr), max(tr), mr / mh, nbytes / 1e6, nbytes / (mh * 1e-3) / 1e12,
                        float(lh.detach()), loss_rel, grad_rel))
    lines += ['', 'Captured DPNet train step at 2x256x384 (synthetic batch, fp32), loss_type [smoothL1] against [smoothL1, normal_geo] (lambdas 1.0, 0.1),',
              '%d replays between two events, alternating, %d rounds:' % (args.reps, args.rounds)]
    plain, both = _step_with(['smoothL1']), _step_with(['smoothL1', 'normal_geo'])
    tp, tb = [], []
    for _ in range(args.rounds):
        tp.append(bench_support.timed(plain, args.reps))
        tb.append(bench_support.timed(both, args.reps))
    mp, mb = statistics.median(tp), statistics.median(tb)
    lines.append('smoothL1 %.4f ms (min %.4f, max %.4f) | smoothL1 + normal_geo %.4f ms (min %.4f, max %.4f) | + %.4f ms = %.2f %% of the step'
                 % (mp, min(tp), max(tp), mb, min(tb), max(tb), mb - mp, 100.0 * (mb - mp) / mp))
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
