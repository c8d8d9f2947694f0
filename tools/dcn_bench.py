"""Stand-alone timing of the deformable-conv kernels, by default at the StereoDPNet shapes (B=4, 4x256x384 voxels, C = 35 and 64, K = 64).

    python tools/dcn_bench.py [fwd|all] [C ...] [--group G] [--deformable-group DG] [--shape B,D,H,W] [--k K] [--compat] [--reps N]

--group / --deformable-group: weight [K, C/G, 3, 3, 3], offset [B, DG*81, ...].  --compat times the drop-in module dcn_compat (the one surface
that takes every grouping on every revision of this tree) instead of the raw C-ABI wrappers of ops."""
import argparse, sys, time, torch
sys.path.insert(0, '.')
from dualpixelface_amd import ops
ap = argparse.ArgumentParser()
ap.add_argument('mode', nargs='?', default='all', choices=['fwd', 'all'])
ap.add_argument('channels', nargs='*', type=int)
ap.add_argument('--group', type=int, default=1)
ap.add_argument('--deformable-group', type=int, default=1)
ap.add_argument('--shape', default='4,4,256,384')
ap.add_argument('--k', type=int, default=64)
ap.add_argument('--compat', action='store_true')
ap.add_argument('--reps', type=int, default=6)
a = ap.parse_args()
if a.reps < 2:
    ap.error('--reps must be at least 2: the first call is dropped as warm-up')
dev = 'cuda'
mode, G, DG, K = a.mode, a.group, a.deformable_group, a.k
B, D, H, W = [int(v) for v in a.shape.split(',')]
sel = a.channels or [35, 64]
one = (1, 1, 1)
ints = (3, 3, 3) + one * 3 + (G, DG, 64)
if a.compat:
    import dualpixelface_amd.dcn_compat as DCN
    fwd = lambda x, w, b, off: DCN.deform_conv_forward(x, w, b, off, *ints)
    bwd = lambda x, w, b, off, go: DCN.deform_conv_backward(x, w, b, off, go, *ints)
else:
    fwd = lambda x, w, b, off: ops.deform_conv_forward_raw(x, w, b, off, one, one, one, G, DG)
    bwd = lambda x, w, b, off, go: ops.deform_conv_backward_raw(x, w, b, off, go, one, one, one, G, DG)
for C in sel:
    sig = 1.3 if C == 35 else 0.75
    torch.manual_seed(0)
    x = torch.randn(B, C, D, H, W, device=dev)
    off = torch.randn(B, DG * 81, D, H, W, device=dev) * sig
    w = torch.randn(K, C // G, 3, 3, 3, device=dev) * 0.05
    b = torch.zeros(K, device=dev)
    go = torch.randn(B, K, D, H, W, device=dev)
    tf, tb = [], []
    for it in range(a.reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        y = fwd(x, w, b, off)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        if mode == 'all':
            g = bwd(x, w, b, off, go)
        torch.cuda.synchronize(); t2 = time.perf_counter()
        tf.append((t1 - t0) * 1e3); tb.append((t2 - t1) * 1e3)
    med = lambda v: sorted(v[1:])[(len(v) - 1) // 2]
    print('C=%d K=%d %dx%dx%dx%d group=%d deformable_group=%d%s sigma=%.2f  fwd min %.2f med %.2f ms   bwd(all) min %.2f med %.2f ms' % (
        C, K, B, D, H, W, G, DG, ' (dcn_compat)' if a.compat else '', sig, min(tf[1:]), med(tf), min(tb[1:]), med(tb)))
