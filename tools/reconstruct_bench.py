#!/usr/bin/env python3
"""The surface operators (csrc/reconstruct.hip): time against the same definitions written in torch on the GPU in the same run, achieved
bandwidth on the algorithmic bytes, and the share of an evaluation forward.

    python tools/reconstruct_bench.py [--shapes 1,1024,1536:4,1024,1536] [--stride 2] [--reps 50] [--rounds 5] [--forward_shape 1,1024,1536]
                                      [--out profiles/reconstruct_timings.txt]

Scene: tests/reconstruct_cpu.scene (a bumpy tilted surface with depth steps, Bernoulli(0.8) mask, 'disp' target).  Each of ops.backproject,
ops.depth_normals, ops.depth_mesh and the three in a row is warmed up, then timed two ways for `rounds` rounds, median (min, max): `reps`
calls captured into one graph and replayed between two events (the device time of a call), and `reps` eager calls between two events with
the hip and torch sides alternating (enqueued from Python: an upper bound that includes the host).  "torch" is the same arithmetic as
elementwise tensor operations, shifts by slicing and, for the mesh, cumsum and boolean indexing (which reads the host, so it is timed eagerly
only).  Bandwidth: the algorithmic traffic -- backproject and depth_normals read pred and mask (8 bytes a pixel) and write 13; depth_mesh
reads pred, mask, the normal map and the view at its nodes (32 bytes a node) and writes 27 bytes a vertex and 12 a face -- over the replayed
time, against the 6.29 TB/s copy rate of profiles/README.md.  Share: plugin.STEREODPNET evaluation forward at `forward_shape` on a synthetic
batch with the block off, against the replayed time of the three operators at that shape.  Needs a GPU; there is no CPU fallback.
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
RATIO = 0.01


def torch_scene(pred, K, ab, mask):
    """(z [B, H, W], 0 where invalid; rays [B, 3, H, W]; Kinv [B, 3, 3]) as the kernels define them, near 0 and no far limit."""
    B, H, W = pred.shape
    inv = torch.linalg.inv(K.double()).float()
    z = ab[:, 1].view(B, 1, 1) / (pred - ab[:, 0].view(B, 1, 1))
    z = torch.where(torch.isfinite(z), z, torch.zeros_like(z))
    z = torch.where((z > 0) & (mask > 0), z, torch.zeros_like(z))
    y, x = torch.meshgrid(torch.arange(H, device=pred.device, dtype=torch.float32), torch.arange(W, device=pred.device, dtype=torch.float32),
                          indexing='ij')
    rays = (inv[:, :, 0].view(B, 3, 1, 1) * x + inv[:, :, 1].view(B, 3, 1, 1) * y) + inv[:, :, 2].view(B, 3, 1, 1)
    return z, rays, inv


def torch_backproject(pred, K, ab, mask):
    z, rays, _ = torch_scene(pred, K, ab, mask)
    return z.unsqueeze(1) * rays, (z > 0).to(torch.uint8)


def _connected(zp, zq):
    return (zp > 0) & (zq > 0) & ((zp - zq).abs() <= RATIO * torch.minimum(zp, zq))


def _shift(t, dy, dx):
    """t at (y + dy, x + dx), zero outside."""
    return torch.roll(torch.nn.functional.pad(t, (1, 1, 1, 1)), shifts=(-dy, -dx), dims=(-2, -1))[..., 1:-1, 1:-1]


def torch_normals(pred, K, ab, mask):
    z, rays, inv = torch_scene(pred, K, ab, mask)
    B = z.shape[0]
    steps = []
    for col, (dy, dx) in enumerate(((0, 1), (1, 0))):
        zm, zp = _shift(z, -dy, -dx), _shift(z, dy, dx)
        rp = rays + inv[:, :, col].view(B, 3, 1, 1)                  # the ray one pixel on (what the kernel evaluates at x + 1 / y + 1)
        cm, cp = _connected(zm, z), _connected(z, zp)
        zfrom, zto = torch.where(cm, zm, z), torch.where(cp, zp, z)
        delta = torch.where(cm & cp, 2.0, 1.0)
        d = (zto - zfrom).unsqueeze(1) * torch.where(cp.unsqueeze(1), rp, rays) + (zfrom * delta).unsqueeze(1) * inv[:, :, col].view(B, 3, 1, 1)
        steps.append((d, cm | cp))
    (dr, hr), (dc, hc) = steps
    n = torch.cross(dr, dc, dim=1)
    length = n.norm(dim=1)
    ok = (z > 0) & hr & hc & (length > 0)
    n = n / length.unsqueeze(1)
    flip = (n * z.unsqueeze(1) * rays).sum(1) > 0
    n = torch.where(flip.unsqueeze(1), -n, n)
    return torch.where(ok.unsqueeze(1), n, torch.zeros_like(n)), ok.to(torch.uint8)


def torch_mesh(pred, K, ab, mask, nmap, view, stride):
    """Per sample (vertices, normals, colours, faces) by cumsum and boolean indexing."""
    from dualpixelface_amd.facedp import IMAGENET_MEAN, IMAGENET_STD
    z, rays, _ = torch_scene(pred, K, ab, mask)
    zn, rn = z[:, ::stride, ::stride], rays[:, :, ::stride, ::stride]
    P = zn.unsqueeze(1) * rn
    std, mean = (torch.tensor(v, device=pred.device).view(1, 3, 1, 1) for v in (IMAGENET_STD, IMAGENET_MEAN))
    col = torch.clamp(torch.round(255.0 * (view[:, :, ::stride, ::stride] * std + mean)), 0, 255).to(torch.uint8)
    nn = nmap[:, :, ::stride, ::stride]
    out = []
    for b in range(z.shape[0]):
        valid = zn[b] > 0
        vidx = (torch.cumsum(valid.flatten().to(torch.int32), 0) - 1).view_as(valid).to(torch.int32)
        za, zb, zc, zd = zn[b, :-1, :-1], zn[b, :-1, 1:], zn[b, 1:, :-1], zn[b, 1:, 1:]
        ia, ib, ic, id_ = vidx[:-1, :-1], vidx[:-1, 1:], vidx[1:, :-1], vidx[1:, 1:]
        bc = _connected(zb, zc)
        t0, t1 = bc & _connected(za, zc) & _connected(zb, za), bc & _connected(zc, zd) & _connected(zd, zb)
        tris = torch.stack([torch.stack([ia, ic, ib], -1), torch.stack([ib, ic, id_], -1)], 2).view(-1, 3)
        faces = tris[torch.stack([t0, t1], 2).flatten()]
        sel = valid.flatten()
        out.append((P[b].flatten(1).t()[sel], nn[b].flatten(1).t()[sel], col[b].flatten(1).t()[sel], faces))
    return out


def operands(B, H, W, seed=3):
    from tests import reconstruct_cpu as rc
    sc = rc.scene(B, H, W, seed)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return dev(sc['pred']), dev(sc['K']), dev(sc['ab']), dev(sc['mask']), dev(sc['view'])


def forward_time(shape, reps, rounds):
    from dualpixelface_amd import load_option
    from dualpixelface_amd.plugin import STEREODPNET
    from dualpixelface_amd.recipe import fill_by_recipe, synthetic_batch
    B, H, W = shape
    model = STEREODPNET(load_option('eval_faceDP'))
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
    ap.add_argument('--stride', type=int, default=2)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--forward_shape', default='1,1024,1536')
    ap.add_argument('--forward_reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'reconstruct_timings.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'reconstruct_bench needs an MI355X'
    from dualpixelface_amd import ops
    lines = ['Surface operators: python tools/reconstruct_bench.py --shapes %s --stride %d --reps %d --rounds %d --forward_shape %s --forward_reps %d'
             % (args.shapes, args.stride, args.reps, args.rounds, args.forward_shape, args.forward_reps),
             'One MI355X (gfx950), one process.  target type disp, near 0, no far limit, max_edge_ratio %g, mask and view given; the mesh at stride '
             '%d and, for comparison, 1.' % (RATIO, args.stride), '',
             'Time, median of %d rounds (min, max).  "graph replay": %d calls captured into one graph and replayed between two events, per call -- '
             'the device time; the inputs' % (args.rounds, args.reps),
             'repeat, so at 1x1024x1536 (6 MB a plane) they come from the caches, not from HBM.  "eager": %d calls enqueued from Python between two '
             'events, hip and torch alternating' % args.reps,
             '-- an upper bound that includes the host (the torch mesh reads the host for its boolean indexing: a fifth of the calls).']
    together = {}
    for shape in args.shapes.split(':'):
        B, H, W = (int(v) for v in shape.split(','))
        pred, K, ab, mask, view = operands(B, H, W)
        tag = '%dx%dx%d' % (B, H, W)
        kw = dict(ab=ab, mask=mask, max_edge_ratio=RATIO)
        nmap = ops.depth_normals(pred, K, **kw)[0]
        hip_bp = lambda: ops.backproject(pred, K, ab=ab, mask=mask)
        hip_n = lambda: ops.depth_normals(pred, K, **kw)
        meshes = {s: (lambda s=s: ops.depth_mesh(pred, K, nmap, view=view, stride=s, **kw)) for s in sorted({1, args.stride})}

        def hip_all():
            ops.backproject(pred, K, ab=ab, mask=mask)
            n = ops.depth_normals(pred, K, **kw)[0]
            ops.depth_mesh(pred, K, n, view=view, stride=args.stride, **kw)

        def torch_all():
            torch_backproject(pred, K, ab, mask)
            n = torch_normals(pred, K, ab, mask)[0]
            torch_mesh(pred, K, ab, mask, n, view, args.stride)

        # the torch side computes what the kernels compute (the tests hold the kernels to the numpy restatement, bit for bit)
        P, V = hip_bp()
        tP, tV = torch_backproject(pred, K, ab, mask)
        N, NV = hip_n()
        tN, tNV = torch_normals(pred, K, ab, mask)
        agree = 'valid differs at %d pixels, max |dP| %.1e; normal_valid differs at %d, max |dn| where both %.1e' % (
            int((V != tV).sum()), float((P - tP).abs().max()), int((NV != tNV).sum()),
            float(((N - tN).abs().amax(1))[(NV > 0) & (tNV > 0)].max()))
        px = float(B * H * W)
        rows = [('backproject', hip_bp, lambda: torch_backproject(pred, K, ab, mask), 21.0 * px, args.reps),
                ('depth_normals', hip_n, lambda: torch_normals(pred, K, ab, mask), 21.0 * px, args.reps)]
        for s, fn in meshes.items():
            counts = fn()[4].cpu().tolist()
            nodes = B * (-(-H // s)) * (-(-W // s))
            traffic = 32.0 * nodes + sum(27.0 * nv + 12.0 * nf for nv, nf in counts)
            rows.append(('depth_mesh s=%d' % s, fn, lambda s=s: torch_mesh(pred, K, ab, mask, nmap, view, s), traffic, max(1, args.reps // 5)))
            lines.append('%-11s mesh at stride %d: %s (vertices, faces) of %d nodes' % (tag, s, counts, nodes // B))
        rows.append(('all three s=%d' % args.stride, hip_all, torch_all, 0.0, max(1, args.reps // 5)))
        lines.append('%-11s hip against torch on this scene: %s' % (tag, agree))
        for name, hip, tor, traffic, reps in rows:
            tr = bench_support.replayed(hip, args.reps, args.rounds)
            th, tt = bench_support.rounds_of((hip, tor), reps, args.rounds)
            m = statistics.median(tr)
            bw = '' if not traffic else ' | %.1f MB algorithmic = %.3f TB/s = %.1f %% of the copy rate' % (
                traffic / 1e6, traffic / (m * 1e-3) / 1e12, 100.0 * traffic / (m * 1e-3) / COPY_RATE)
            lines.append('%-11s %-16s hip, graph replay %s | hip, eager %s | torch, eager %s | torch / hip replay %.1fx%s'
                         % (tag, name, fmt(tr), fmt(th), fmt(tt), statistics.median(tt) / m, bw))
            print(lines[-1], flush=True)
            if name.startswith('all three'):
                together[(B, H, W)] = m
    fs = tuple(int(v) for v in args.forward_shape.split(','))
    lines += ['', 'STEREODPNET evaluation forward (eval_faceDP, the block off), synthetic batch %dx%dx%d, %d forwards between two events, median of '
              '%d rounds:' % (fs + (args.forward_reps, args.rounds))]
    try:
        t0 = forward_time(fs, args.forward_reps, args.rounds)
        m0 = statistics.median(t0)
        lines.append('forward        %s' % fmt(t0))
        if fs in together:
            lines.append('the three operators at that shape, graph replay: %.3f ms = %.3f %% of the forward' % (together[fs], 100 * together[fs] / m0))
    except Exception as e:                                   # (the forward at this size may not fit: the share is then not measured)
        lines.append('not measured: %s: %s' % (type(e).__name__, str(e).splitlines()[0][:200]))
    lines += ['', 'Not measured: kernel times from a profiler trace (the figures above are event times of captured calls); HBM-resident inputs at '
              '1x1024x1536 (the repeated inputs stay in the caches);', 'the evaluation forward with the block on (it is the forward above plus the '
              'operators); PLY writing (host numpy and the file system); other strides than the two above.']
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
