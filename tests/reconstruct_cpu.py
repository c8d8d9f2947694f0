"""The definitions of csrc/reconstruct.hip restated in numpy (test infrastructure): every function takes ``dt``,
np.float32 for the evaluation operation by operation in the kernels' order, np.float64 for the same expressions in double precision over the
same fp32 inputs (Kinv unrounded).  Also the scenes the tests draw, the distance of every comparison from its threshold, and a PLY reader.
"""
import numpy as np

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)           # the data path's Normalizer (facedp.IMAGENET_MEAN / _STD)
TARGET_TYPES = ('disp', 'idepth', 'depth')


# ---- definitions
def kinv(K):
    """K [B, 3, 3] float32 -> (adjugate / det in fp64 [B, 3, 3], regular [B])."""
    m = K.astype(np.float64).reshape(-1, 9).T
    c00, c01, c02 = m[4] * m[8] - m[5] * m[7], m[5] * m[6] - m[3] * m[8], m[3] * m[7] - m[4] * m[6]
    det = (m[0] * c00 + m[1] * c01) + m[2] * c02
    adj = np.stack([c00, m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                    c01, m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                    c02, m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]])
    ok = np.isfinite(det) & (np.abs(det) >= 1e-30)
    with np.errstate(all='ignore'):
        inv = np.where(ok, adj / det, 0.0)
    return inv.T.reshape(-1, 3, 3), ok


def raw_depth(pred, target_type, ab, dt):
    """z before the validity test: a / (pred - b) or pred, non-finite -> 0."""
    p = pred.astype(dt)
    with np.errstate(all='ignore'):
        if target_type == 'depth':
            z = p.copy()
        else:
            b, a = ab[:, 0].astype(dt)[:, None, None], ab[:, 1].astype(dt)[:, None, None]
            z = a / (p - b)
    z[~np.isfinite(z)] = 0
    return z


def scene_depth(pred, target_type, ab, K, mask, near, far, dt):
    """-> (z [B, H, W] in dt, 0 where invalid; Kinv [B, 3, 3] in dt).  The limits are the fp32 values the kernels receive."""
    inv, ok = kinv(K)
    z = raw_depth(pred, target_type, ab, dt)
    near, far = dt(np.float32(near)), dt(np.float32(np.inf if far is None else far))
    valid = ok[:, None, None] & (z > near) & (z < far)
    if mask is not None:
        with np.errstate(invalid='ignore'):
            valid &= mask > 0
    return np.where(valid, z, dt(0)), inv.astype(dt)


def rays(inv, H, W, dt, ys=None, xs=None):
    """r [B, 3, h, w] = (Kinv[k][0] x + Kinv[k][1] y) + Kinv[k][2] at the pixels ys x xs (default: all)."""
    ys = np.arange(H) if ys is None else ys
    xs = np.arange(W) if xs is None else xs
    yf, xf = ys.astype(dt)[None, None, :, None], xs.astype(dt)[None, None, None, :]
    i = inv[:, :, :, None, None]
    return (i[:, :, 0] * xf + i[:, :, 1] * yf) + i[:, :, 2]


def backproject(pred, target_type, ab, K, mask, near=0.0, far=None, dt=np.float32):
    z, inv = scene_depth(pred, target_type, ab, K, mask, near, far, dt)
    B, H, W = z.shape
    return z[:, None] * rays(inv, H, W, dt), (z > 0).astype(np.uint8)


def connected(zp, zq, ratio, dt):
    return (zp > 0) & (zq > 0) & (np.abs(zp - zq) <= dt(np.float32(ratio)) * np.minimum(zp, zq))


def _step(inv, col, zm, zc, zp, rc, rp, ratio, dt):
    """The step along one axis for every pixel: (d [B, 3, H, W], has [B, H, W])."""
    cm, cp = connected(zm, zc, ratio, dt), connected(zc, zp, ratio, dt)
    zfrom, zto = np.where(cm, zm, zc), np.where(cp, zp, zc)
    delta = np.where(cm & cp, dt(2), dt(1))
    dz, t = zto - zfrom, zfrom * delta
    rq = np.where(cp[:, None], rp, rc)
    d = dz[:, None] * rq + t[:, None] * inv[:, :, col][:, :, None, None]
    return d, cm | cp


def _shift(z, dy, dx):
    """z at (y + dy, x + dx), 0 outside the image."""
    out = np.zeros_like(z)
    H, W = z.shape[-2:]
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    out[..., yd, xd] = z[..., ys, xs]
    return out


def depth_normals(pred, target_type, ab, K, mask, near=0.0, far=None, max_edge_ratio=0.01, towards_camera=True, dt=np.float32):
    z, inv = scene_depth(pred, target_type, ab, K, mask, near, far, dt)
    B, H, W = z.shape
    rc = rays(inv, H, W, dt)
    rr = rays(inv, H, W, dt, xs=np.arange(W) + 1)
    rd = rays(inv, H, W, dt, ys=np.arange(H) + 1)
    drow, hrow = _step(inv, 0, _shift(z, 0, -1), z, _shift(z, 0, 1), rc, rr, max_edge_ratio, dt)
    dcol, hcol = _step(inv, 1, _shift(z, -1, 0), z, _shift(z, 1, 0), rc, rd, max_edge_ratio, dt)
    cx = drow[:, 1] * dcol[:, 2] - drow[:, 2] * dcol[:, 1]
    cy = drow[:, 2] * dcol[:, 0] - drow[:, 0] * dcol[:, 2]
    cz = drow[:, 0] * dcol[:, 1] - drow[:, 1] * dcol[:, 0]
    with np.errstate(all='ignore'):
        length = np.sqrt((cx * cx + cy * cy) + cz * cz)
        ok = (z > 0) & hrow & hcol & (length > 0) & np.isfinite(length)
        n = np.stack([cx, cy, cz], 1) / length[:, None]
        dot = (n[:, 0] * (z * rc[:, 0]) + n[:, 1] * (z * rc[:, 1])) + n[:, 2] * (z * rc[:, 2])
        flip = dot > 0 if towards_camera else dot < 0
    n = np.where(flip[:, None], -n, n)
    n = np.where(ok[:, None], n, dt(0))
    return n.astype(dt), ok.astype(np.uint8)


def colours(view, dt=np.float32):
    """clamp(round(255 (v std + mean)), 0, 255) as uint8, [B, 3, ...] -> the same shape."""
    shape = (1, 3) + (1,) * (view.ndim - 2)
    std, mean = np.asarray(STD, np.float32).astype(dt).reshape(shape), np.asarray(MEAN, np.float32).astype(dt).reshape(shape)
    c = np.rint(dt(255) * (view.astype(dt) * std + mean))
    c = np.where(np.isnan(c), 0, c)
    return np.minimum(np.maximum(c, 0), 255).astype(np.uint8)


def depth_mesh(pred, target_type, ab, K, mask, normal_map, view, stride=1, near=0.0, far=None, max_edge_ratio=0.01, towards_camera=True,
               dt=np.float32):
    """-> per sample (vertices [V, 3] dt, normals [V, 3], colours [V, 3] uint8, faces [F, 3] int32)."""
    z, inv = scene_depth(pred, target_type, ab, K, mask, near, far, dt)
    B, H, W = z.shape
    ys, xs = np.arange(0, H, stride), np.arange(0, W, stride)
    zn = z[:, ::stride, ::stride]
    Hs, Ws = zn.shape[1:]
    P = zn[:, None] * rays(inv, H, W, dt, ys, xs)
    out = []
    for b in range(B):
        valid = zn[b] > 0
        vidx = (np.cumsum(valid.ravel()) - 1).reshape(Hs, Ws)
        sel = valid.ravel()
        vertices = P[b].reshape(3, -1).T[sel]
        normals = normal_map[b][:, ::stride, ::stride].reshape(3, -1).T[sel]
        if view is None:
            cols = np.full((int(sel.sum()), 3), 255, np.uint8)
        else:
            cols = colours(view[b:b + 1, :, ::stride, ::stride], dt)[0].reshape(3, -1).T[sel]
        za, zb, zc, zd = zn[b, :-1, :-1], zn[b, :-1, 1:], zn[b, 1:, :-1], zn[b, 1:, 1:]
        ia, ib, ic, id_ = vidx[:-1, :-1], vidx[:-1, 1:], vidx[1:, :-1], vidx[1:, 1:]
        bc = connected(zb, zc, max_edge_ratio, dt)
        t0 = bc & connected(za, zc, max_edge_ratio, dt) & connected(zb, za, max_edge_ratio, dt)
        t1 = bc & connected(zc, zd, max_edge_ratio, dt) & connected(zd, zb, max_edge_ratio, dt)
        tri0 = np.stack([ia, ic, ib] if towards_camera else [ia, ib, ic], -1)
        tri1 = np.stack([ib, ic, id_] if towards_camera else [ib, id_, ic], -1)
        tris = np.stack([tri0, tri1], 2).reshape(-1, 3)                       # quads row-major, T0 before T1
        flags = np.stack([t0, t1], 2).reshape(-1)
        out.append((vertices.astype(dt), normals, cols, tris[flags].astype(np.int32)))
    return out


# ---- how far the comparisons of a scene sit from their thresholds (fp64)
def margins(pred, target_type, ab, K, mask, near=0.0, far=None, max_edge_ratio=0.01, strides=(1,)):
    """The smallest relative distance, in the fp64 restatement, between a compared quantity and its threshold: z against near and far over
    the pixels with a finite z, |z_p - z_q| against max_edge_ratio min(z_p, z_q) over every pair of valid neighbours the kernels compare
    (row, column and the b-c diagonal, at every stride of `strides`).  The integer outputs of fp32 and fp64 agree when this is well above
    the fp32 rounding of z (6e-8 relative per operation)."""
    dt = np.float64
    zraw = raw_depth(pred, target_type, ab, dt)
    worst = np.inf
    live = zraw != 0
    for lim in (np.float32(near), np.float32(np.inf if far is None else far)):
        if np.isfinite(lim) and live.any():
            worst = min(worst, float(np.min(np.abs(zraw[live] - dt(lim)) / max(abs(float(lim)), 1.0))))
    z, _ = scene_depth(pred, target_type, ab, K, mask, near, far, dt)
    for s in strides:
        zn = z[:, ::s, ::s]
        for zp, zq in ((zn[:, :, :-1], zn[:, :, 1:]), (zn[:, :-1], zn[:, 1:]), (zn[:, :-1, 1:], zn[:, 1:, :-1])):
            both = (zp > 0) & (zq > 0)
            if both.any():
                thr = dt(np.float32(max_edge_ratio)) * np.minimum(zp, zq)[both]
                worst = min(worst, float(np.min(np.abs(np.abs(zp - zq)[both] - thr) / thr)))
    return worst


def colour_margin(view):
    """The smallest distance of 255 (v std + mean) from a rounding tie or a clamp edge's tie, in fp64."""
    t = 255.0 * (view.astype(np.float64) * np.asarray(STD, np.float32).astype(np.float64).reshape(1, 3, 1, 1)
                 + np.asarray(MEAN, np.float32).astype(np.float64).reshape(1, 3, 1, 1))
    return float(np.min(np.abs(t - np.floor(t) - 0.5)))


# ---- scenes
def camera(B, H, W, rng, f=None):
    K = np.zeros((B, 3, 3), np.float32)
    for b in range(B):
        fx = f if f is not None else 1200.0 + 800.0 * rng.rand()
        K[b] = [[fx, 0.3 * rng.rand(), W / 2.0 + rng.rand()], [0.0, fx * (1.0 + 0.02 * rng.rand()), H / 2.0 + rng.rand()], [0.0, 0.0, 1.0]]
    return K


def scene(B, H, W, seed, target_type='disp', ratio=0.01, masked=True, bad=True, singular=None):
    """A face-like surface around 800 mm: a tilted plane with smooth bumps, cut by depth steps of 0.6, 1.7 (columns) and 0.8, 2.5 (rows)
    times `ratio`, a Bernoulli(0.8) mask, a few NaN / zero / negative / infinite predictions, and optionally one singular K.
    -> dict(pred [B, H, W] f32, ab [B, 2] f32 = [b, a], K, mask or None, view [B, 3, H, W] f32, z [B, H, W] f64 the surface drawn)."""
    rng = np.random.RandomState(seed)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    z = np.zeros((B, H, W))
    for b in range(B):
        gx, gy = (rng.rand(2) - 0.5) * 2.0 * np.minimum(0.35, 40.0 / np.array([W, H]))
        zb = 800.0 + 40.0 * (rng.rand() - 0.5) + gx * x + gy * y + 2.0 * np.sin(x / 5.0 + 6.0 * rng.rand()) * np.cos(y / 7.0 + 6.0 * rng.rand())
        for axis, factors in ((x, (0.6, 1.7)), (y, (0.8, 2.5))):
            n = W if axis is x else H
            for k, fac in enumerate(factors):
                zb = zb * np.where(axis >= int(n * (k + 1) / 3.0 + rng.randint(0, 2)), 1.0 + fac * ratio, 1.0)
        z[b] = zb
    ab = np.stack([-5.0 + rng.rand(B), 40000.0 * (1.0 + 0.1 * rng.rand(B))], 1).astype(np.float32)
    if target_type == 'depth':
        pred = z.astype(np.float32)
    else:
        pred = (ab[:, 0].astype(np.float64)[:, None, None] + ab[:, 1].astype(np.float64)[:, None, None] / z).astype(np.float32)
    if bad and H * W >= 12:
        junk = [np.nan, np.inf, -np.inf] + ([0.0, -3.0, -800.0] if target_type == 'depth' else [-1e4, -40.0])
        for b in range(B):
            for k, v in enumerate(junk):
                pred[b, rng.randint(H), rng.randint(W)] = v
            if target_type != 'depth':
                pred[b, rng.randint(H), rng.randint(W)] = ab[b, 0]           # pred - b = 0: a / 0
    mask = None
    if masked:
        mask = (rng.rand(B, H, W) < 0.8).astype(np.float32)
        if H * W >= 12:
            mask[0, rng.randint(H), rng.randint(W)] = -1.0
            mask[0, rng.randint(H), rng.randint(W)] = np.nan
            mask[0, rng.randint(H), rng.randint(W)] = 0.25
    K = camera(B, H, W, rng)
    if singular is not None:
        K[singular, 1] = 2.0 * K[singular, 0]
    # colours: 255 (v std + mean) over [-25, 280] (both clamps), moved off the rounding ties
    t = rng.rand(B, 3, H, W) * 305.0 - 25.0
    frac = t - np.floor(t)
    t = np.where(np.abs(frac - 0.5) < 0.02, t + 0.1, t)
    view = ((t / 255.0 - np.asarray(MEAN).reshape(1, 3, 1, 1)) / np.asarray(STD).reshape(1, 3, 1, 1)).astype(np.float32)
    return dict(pred=pred, ab=ab, K=K, mask=mask, view=view, z=z, target_type=target_type)


def gap_limit(sc, lo, hi):
    """A depth limit inside [lo, hi] in the middle of the widest gap between the scene's depths there (fp64), so that no pixel sits on it."""
    z = np.sort(raw_depth(sc['pred'], sc['target_type'], sc['ab'], np.float64).ravel())
    z = np.concatenate([[lo], z[(z > lo) & (z < hi)], [hi]])
    k = int(np.argmax(np.diff(z)))
    return float(np.float32(0.5 * (z[k] + z[k + 1])))


def tilted_plane(H=24, W=40, f=5000.0, z0=800.0, slope=(0.35, -0.2)):
    """The plane n . P = d at z0 mm in front of a camera with focal length f px, tilted by `slope` (dz/dX, dz/dY), as a depth-target scene
    whose depth is the fp32 rounding of the exact one.  -> (scene dict, unit normal facing the camera)."""
    K = np.array([[[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]]], np.float32)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    rx, ry = (x - W / 2.0) / f, (y - H / 2.0) / f
    # z = z0 + sx X + sy Y with X = z rx, Y = z ry  ->  z = z0 / (1 - sx rx - sy ry)
    z = z0 / (1.0 - slope[0] * rx - slope[1] * ry)
    n = np.array([slope[0], slope[1], -1.0])
    n /= np.linalg.norm(n)
    sc = dict(pred=z[None].astype(np.float32), ab=None, K=K, mask=None, view=None, z=z[None], target_type='depth')
    return sc, n


def angle(a, b):
    """The angle between the vectors a, b [..., 3] in fp64 (atan2 form: exact for small angles)."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), np.sum(a * b, -1))


# ---- PLY reader (tests only)
def read_ply(path):
    """-> dict(header=str, vertices, normals, colours, faces, nbytes): the files reconstruct.write_ply writes."""
    raw = open(path, 'rb').read()
    end = raw.index(b'end_header\n') + len(b'end_header\n')
    header = raw[:end].decode('ascii')
    lines = header.split('\n')
    assert lines[0] == 'ply' and lines[1] == 'format binary_little_endian 1.0', lines[:2]
    nv = int([ln for ln in lines if ln.startswith('element vertex')][0].split()[-1])
    nf = int([ln for ln in lines if ln.startswith('element face')][0].split()[-1])
    vdt = np.dtype([('p', '<f4', 3), ('n', '<f4', 3), ('c', 'u1', 3)])
    fdt = np.dtype([('k', 'u1'), ('i', '<i4', 3)])
    assert vdt.itemsize == 27 and fdt.itemsize == 13
    assert len(raw) == end + nv * 27 + nf * 13, (len(raw), end, nv, nf)
    v = np.frombuffer(raw, vdt, nv, end)
    f = np.frombuffer(raw, fdt, nf, end + nv * 27)
    assert nf == 0 or bool((f['k'] == 3).all())
    return dict(header=header, vertices=v['p'].copy(), normals=v['n'].copy(), colours=v['c'].copy(), faces=f['i'].copy(), nbytes=len(raw))


# ---- the cases of tests/test_gpu_reconstruct.py: (B, H, W, target type, masked, finite far, index of a singular K or None, strides, seed)
CASES = [
    (1, 5, 7, 'disp', True, False, None, (1, 2, 4, 8), 11),
    (2, 17, 33, 'idepth', True, True, 1, (1, 2, 4, 8), 12),
    (3, 40, 77, 'depth', True, False, None, (1, 2, 4, 8), 13),
    (3, 40, 77, 'disp', False, True, 2, (1, 8), 14),
    (1, 16, 32, 'disp', True, False, None, (2, 4, 8), 15),            # multiples of every stride
    (1, 1, 9, 'depth', False, False, None, (1, 2), 16),               # one row / one column: no quad, no normal
    (1, 9, 1, 'disp', False, False, None, (1, 4), 17),
    (2, 2, 9, 'depth', True, False, None, (1, 2), 18),                # two rows / two columns: one row of quads at stride 1
    (1, 9, 2, 'idepth', False, False, None, (1, 2), 19),
    (1, 384, 700, 'disp', True, False, None, (1, 2), 20),             # 263 workgroups of 1024 nodes at stride 1: more than the scan's 256 threads
]


def case_id(case):
    return '%dx%dx%d-%s%s%s%s' % (case[0], case[1], case[2], case[3], '' if case[4] else '-nomask', '-far' if case[5] else '',
                                  '' if case[6] is None else '-singular%d' % case[6])


_cache = {}


def case(c):
    """The scene of a case with its depth limits and both restatements, computed once: dict(sc, near, far, ratio, P32, P64, valid, n32, n64,
    nvalid, mesh32[stride], mesh64[stride], margin).  Nothing in it may be changed by a test."""
    if c in _cache:
        return _cache[c]
    B, H, W, tt, masked, finite_far, singular, strides, seed = c
    sc = scene(B, H, W, seed, target_type=tt, masked=masked, singular=singular)
    near, far, ratio = 0.0, None, 0.01
    if finite_far:
        far = gap_limit(sc, 835.0, 860.0)
        near = gap_limit(sc, 765.0, 785.0)
    args = (sc['pred'], tt, sc['ab'], sc['K'], sc['mask'])
    out = dict(sc=sc, near=near, far=far, ratio=ratio, strides=strides)
    out['P32'], out['valid'] = backproject(*args, near=near, far=far, dt=np.float32)
    out['P64'], valid64 = backproject(*args, near=near, far=far, dt=np.float64)
    out['n32'], out['nvalid'] = depth_normals(*args, near=near, far=far, max_edge_ratio=ratio, dt=np.float32)
    out['n64'], nvalid64 = depth_normals(*args, near=near, far=far, max_edge_ratio=ratio, dt=np.float64)
    out['mesh32'] = {s: depth_mesh(*args, out['n32'], sc['view'], stride=s, near=near, far=far, max_edge_ratio=ratio, dt=np.float32)
                     for s in strides}
    out['mesh64'] = {s: depth_mesh(*args, out['n32'], sc['view'], stride=s, near=near, far=far, max_edge_ratio=ratio, dt=np.float64)
                     for s in strides}
    out['margin'] = margins(*args, near=near, far=far, max_edge_ratio=ratio, strides=strides)
    out['agree'] = bool(np.array_equal(out['valid'], valid64) and np.array_equal(out['nvalid'], nvalid64) and all(
        np.array_equal(a[3], b[3]) and len(a[0]) == len(b[0]) for s in strides for a, b in zip(out['mesh32'][s], out['mesh64'][s])))
    _cache[c] = out
    return out
