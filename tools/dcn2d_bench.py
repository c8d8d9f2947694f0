"""Stand-alone timing of the 2-D deformable-conv kernels (csrc/dcn2d.hip over csrc/dcn_gather.hip), by default B=4, C=K=64, 256x384,
3x3, padding kernel // 2.

    python tools/dcn2d_bench.py [fwd|all] [C ...] [--shape B,H,W] [--k K] [--kernel KH[,KW]] [--group G] [--deformable-group DG]
                                [--modulated] [--via-3d] [--reps N]

--modulated adds the mask operand (DCN v2).  --via-3d times the same PLAIN problem through the 3-D entry points
(ops.deform_conv_forward_raw / deform_conv_backward_raw) on a depth-1 volume with a [K, C/G, 1, kh, kw] weight and zero depth offsets --
the only way a tree without the 2-D kernels computes it; the offset repack that route needs per call is not timed.
The first call is dropped as warm-up; min and median of the rest."""
import argparse, sys, time, torch
sys.path.insert(0, '.')
from dualpixelface_amd import ops
ap = argparse.ArgumentParser()
ap.add_argument('mode', nargs='?', default='all', choices=['fwd', 'all'])
ap.add_argument('channels', nargs='*', type=int)
ap.add_argument('--shape', default='4,256,384')
ap.add_argument('--k', type=int, default=64)
ap.add_argument('--kernel', default='3')
ap.add_argument('--group', type=int, default=1)
ap.add_argument('--deformable-group', type=int, default=1)
ap.add_argument('--modulated', action='store_true')
ap.add_argument('--via-3d', action='store_true')
ap.add_argument('--reps', type=int, default=6)
a = ap.parse_args()
if a.reps < 2:
    ap.error('--reps must be at least 2: the first call is dropped as warm-up')
if a.via_3d and a.modulated:
    ap.error('--via-3d: the 3-D entry points carry no mask')
dev = 'cuda'
mode, G, DG, K = a.mode, a.group, a.deformable_group, a.k
B, H, W = [int(v) for v in a.shape.split(',')]
ks = [int(v) for v in a.kernel.split(',')]
kh, kw = ks if len(ks) == 2 else (ks[0], ks[0])
T = kh * kw
s2, p2, d2 = (1, 1), (kh // 2, kw // 2), (1, 1)
Ho, Wo = H + 2 * p2[0] - kh + 1, W + 2 * p2[1] - kw + 1
for C in (a.channels or [64]):
    torch.manual_seed(0)
    x = torch.randn(B, C, H, W, device=dev)
    off = torch.randn(B, DG * 2 * T, Ho, Wo, device=dev) * 0.75
    mask = torch.sigmoid(torch.randn(B, DG * T, Ho, Wo, device=dev)) if a.modulated else None
    w = torch.randn(K, C // G, kh, kw, device=dev) * 0.05
    b = torch.zeros(K, device=dev)
    go = torch.randn(B, K, Ho, Wo, device=dev)
    if a.via_3d:
        x3, w3, go3 = x.unsqueeze(2).contiguous(), w.unsqueeze(2).contiguous(), go.unsqueeze(2).contiguous()
        off3 = torch.zeros(B, DG, T, 3, 1, Ho, Wo, device=dev)
        off3[:, :, :, 1:, 0] = off.reshape(B, DG, T, 2, Ho, Wo)
        off3 = off3.reshape(B, DG * 3 * T, 1, Ho, Wo)
        s3, p3, d3 = (1,) + s2, (0,) + p2, (1,) + d2
        fwd = lambda: ops.deform_conv_forward_raw(x3, w3, b, off3, s3, p3, d3, G, DG)
        bwd = lambda: ops.deform_conv_backward_raw(x3, w3, b, off3, go3, s3, p3, d3, G, DG)
    else:
        fwd = lambda: ops.deform_conv2d_forward_raw(x, w, b, off, mask, s2, p2, d2, G, DG)
        bwd = lambda: ops.deform_conv2d_backward_raw(x, w, b, off, mask, go, s2, p2, d2, G, DG)
    tf, tb = [], []
    for it in range(a.reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        y = fwd()
        torch.cuda.synchronize(); t1 = time.perf_counter()
        if mode == 'all':
            g = bwd()
        torch.cuda.synchronize(); t2 = time.perf_counter()
        tf.append((t1 - t0) * 1e3); tb.append((t2 - t1) * 1e3)
    med = lambda v: sorted(v[1:])[(len(v) - 1) // 2]
    print('C=%d K=%d %dx%dx%d %dx%d group=%d deformable_group=%d %s%s  fwd min %.2f med %.2f ms%s' % (
        C, K, B, H, W, kh, kw, G, DG, 'modulated' if a.modulated else 'plain', ' (via the 3-D entry, depth 1)' if a.via_3d else '',
        min(tf[1:]), med(tf), '   bwd(all) min %.2f med %.2f ms' % (min(tb[1:]), med(tb)) if mode == 'all' else ''))
