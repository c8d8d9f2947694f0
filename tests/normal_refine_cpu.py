"""The definition of csrc/normal_refine.hip restated in numpy (test infrastructure): ``dt`` is np.float32 for the
evaluation operation by operation in the kernels' order, np.float64 for the same expressions in double precision over the same fp32 inputs
(Kinv unrounded, alpha and beta unrounded).  The sums are fp64 in both.  Depth, validity, rays and connected are tests/reconstruct_cpu.py's.
Also the scenes the tests draw and the distance of every comparison from its threshold.
"""
import numpy as np

from tests import reconstruct_cpu as rc


# ---- definitions
def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _normal_step(n, rp, rq, k, min_cos, at_q, dt):
    """The log-depth step the normals n [B, 3, H, W] predict along the edge p -> q -> (g [B, H, W], usable)."""
    with np.errstate(all='ignore'):
        length = np.sqrt(_dot(n, n))
        ok = np.isfinite(length) & (length > dt(np.float32(1e-6)))
        dp, dq = _dot(n, rp), _dot(n, rq)
        ok &= ((dp > 0) & (dq > 0)) | ((dp < 0) & (dq < 0))
        lp, lq = np.sqrt(_dot(rp, rp)), np.sqrt(_dot(rq, rq))
        t = dt(np.float32(min_cos)) * length
        ok &= (np.abs(dp) >= t * lp) & (np.abs(dq) >= t * lq)
        nk = _dot(n, k)
        v = np.log1p(-(nk / dq)) if at_q else -np.log1p(nk / dp)
        ok &= np.isfinite(v)
    return np.where(ok, v, dt(0)), ok


def _edges(z, n, inv, axis, ratio, min_cos, dt):
    """The edge from every pixel p to q, its right (axis 0) or lower (axis 1) neighbour -> (has [B, H, W], e, 0 where there is none)."""
    B, H, W = z.shape
    dy, dx = (0, 1) if axis == 0 else (1, 0)
    zq, nq = rc._shift(z, dy, dx), rc._shift(n, dy, dx)
    rp = rc.rays(inv, H, W, dt)
    rq = rc.rays(inv, H, W, dt, ys=np.arange(H) + dy, xs=np.arange(W) + dx)
    k = inv[:, :, axis][:, :, None, None]
    gp, up = _normal_step(n, rp, rq, k, min_cos, False, dt)
    gq, uq = _normal_step(nq, rp, rq, k, min_cos, True, dt)
    has = rc.connected(z, zq, ratio, dt) & (up | uq)
    g = np.where(up & uq, (gp + gq) * dt(0.5), np.where(up, gp, gq))
    with np.errstate(all='ignore'):
        e = g - np.log1p((zq - z) / z)
    return has, np.where(has, e, dt(0)).astype(dt)


def system(pred, target_type, ab, K, mask, normal, near=0.0, far=None, max_edge_ratio=0.01, min_cos=0.1, lam=0.1, normal_signs=(1, 1, 1),
           dt=np.float32):
    """-> dict(z, valid, right, down (the edge flags of every pixel), left, up (the same edges seen from their other end), b, invD, lam)."""
    z, inv = rc.scene_depth(pred, target_type, ab, K, mask, near, far, dt)
    n = normal.astype(dt) * np.asarray(normal_signs, np.float32).astype(dt).reshape(1, 3, 1, 1)
    right, e_r = _edges(z, n, inv, 0, max_edge_ratio, min_cos, dt)
    down, e_d = _edges(z, n, inv, 1, max_edge_ratio, min_cos, dt)
    left, e_l, up, e_u = rc._shift(right, 0, -1), rc._shift(e_r, 0, -1), rc._shift(down, -1, 0), rc._shift(e_d, -1, 0)
    b = (((dt(0) + e_l) - e_r) + e_u) - e_d                      # (an absent edge carries e = 0)
    lam = dt(np.float32(lam))
    deg = left.astype(np.int32) + right + up + down
    valid = z > 0
    with np.errstate(all='ignore'):
        invD = np.where(valid, dt(1) / (lam + deg.astype(dt)), dt(0))
    return dict(z=z, valid=valid, right=right, down=down, left=left, up=up, b=b.astype(dt), invD=invD.astype(dt), lam=lam)


def apply_A(sy, v):
    """(A v)_p = lam v_p + the sum over the edges at p, left, right, up, down, of (v_p - v_neighbour)."""
    dt = v.dtype.type
    d = np.zeros_like(v)
    for has, dy, dx in ((sy['left'], 0, -1), (sy['right'], 0, 1), (sy['up'], -1, 0), (sy['down'], 1, 0)):
        d = d + np.where(has, v - rc._shift(v, dy, dx), dt(0))
    return sy['lam'] * v + d


def _sum(a, b):
    return np.sum(a.astype(np.float64) * b.astype(np.float64), axis=(1, 2))


def pcg(sy, iterations, dt=np.float32):
    """-> (delta [B, H, W] in dt, rho [B, iterations + 1] fp64)."""
    cast = (lambda v: v.astype(np.float32)) if dt is np.float32 else (lambda v: v)
    r = sy['b'].copy()
    delta = np.zeros_like(r)
    s = r * sy['invD']
    p = s.copy()
    rho = _sum(r, s)
    rhos = [rho]
    for _ in range(iterations):
        q = apply_A(sy, p)
        sigma = _sum(p, q)
        with np.errstate(all='ignore'):
            alpha = cast(np.where((sigma > 0) & (rho > 0), rho / sigma, 0.0))[:, None, None]
        delta = delta + alpha * p
        r = r - alpha * q
        s = r * sy['invD']
        rho_new = _sum(r, s)
        with np.errstate(all='ignore'):
            beta = cast(np.where(rho > 0, rho_new / rho, 0.0))[:, None, None]
        p = s + beta * p
        rho = rho_new
        rhos.append(rho)
    return delta, np.stack(rhos, 1)


def normal_refine(pred, target_type, ab, K, mask, normal, near=0.0, far=None, max_edge_ratio=0.01, min_cos=0.1, lam=0.1, iterations=32,
                  normal_signs=(1, 1, 1), dt=np.float32):
    """-> dict(out [B, H, W] in dt: the refined plane, pred where invalid; delta; z, the input depth; stats [B, 3 + iterations]; sy)."""
    sy = system(pred, target_type, ab, K, mask, normal, near, far, max_edge_ratio, min_cos, lam, normal_signs, dt)
    delta, rhos = pcg(sy, iterations, dt)
    z2 = sy['z'] * np.exp(delta)
    with np.errstate(all='ignore'):
        if target_type == 'depth':
            out = z2
        else:
            out = ab[:, 1].astype(dt)[:, None, None] / z2 + ab[:, 0].astype(dt)[:, None, None]
    out = np.where(sy['valid'], out, pred.astype(dt))
    counts = np.stack([sy['valid'].sum((1, 2)), sy['right'].sum((1, 2)) + sy['down'].sum((1, 2))], 1).astype(np.float64)
    return dict(out=out, delta=delta, z=sy['z'], stats=np.concatenate([counts, rhos], 1), sy=sy)


def dense(sy, b):
    """The dense fp64 A and right-hand side of sample b over its valid pixels -> (A [n, n], rhs [n], the valid mask)."""
    valid = sy['valid'][b]
    H, W = valid.shape
    idx = -np.ones((H, W), np.int64)
    idx[valid] = np.arange(int(valid.sum()))
    A = np.diag(np.full(int(valid.sum()), float(sy['lam'])))
    for has, dy, dx in ((sy['right'][b], 0, 1), (sy['down'][b], 1, 0)):
        for y, x in zip(*np.nonzero(has)):
            i, j = idx[y, x], idx[y + dy, x + dx]
            A[i, i] += 1.0
            A[j, j] += 1.0
            A[i, j] -= 1.0
            A[j, i] -= 1.0
    return A, sy['b'][b][valid].astype(np.float64), valid


def recovered_delta(out, pred, target_type, ab, valid):
    """log(depth of out / depth of pred) in fp64 over the valid pixels, 0 elsewhere: how the tests read delta off a refined plane."""
    with np.errstate(all='ignore'):
        zo, zi = rc.raw_depth(out, target_type, ab, np.float64), rc.raw_depth(pred, target_type, ab, np.float64)
        return np.where(valid, np.log(zo / zi), 0.0)


# ---- how far the normal comparisons of a scene sit from their thresholds (fp64)
def normal_margin(K, normal, H, W, min_cos=0.1, normal_signs=(1, 1, 1)):
    """The smallest relative distance between |n . r| / (|n| |r|) and min_cos over every finite normal and the three rays it can be tested
    against (its own pixel's, the right neighbour's and the lower one's, as the normal of p; the left and upper ones, as the normal of q),
    and between |n| and 1e-6.  Where the cosine passes, the sign test is at least min_cos from its own threshold."""
    dt = np.float64
    inv, regular = rc.kinv(K)
    n = normal.astype(dt) * np.asarray(normal_signs, dt).reshape(1, 3, 1, 1)
    with np.errstate(all='ignore'):
        length = np.sqrt(_dot(n, n))
    live = np.isfinite(length) & regular[:, None, None]                     # (a sample with a singular K tests no normal)
    worst = float(np.min(np.abs(length[live] - 1e-6) / 1e-6)) if live.any() else np.inf
    live &= length > 1e-6
    for dy, dx in ((0, 0), (0, 1), (1, 0), (0, -1), (-1, 0)):
        r = rc.rays(inv, H, W, dt, ys=np.arange(H) + dy, xs=np.arange(W) + dx)
        with np.errstate(all='ignore'):
            c = np.abs(_dot(n, r)) / (length * np.sqrt(_dot(r, r)))
        if live.any():
            worst = min(worst, float(np.min(np.abs(c[live] - min_cos) / min_cos)))
    return worst


# ---- scenes
def noisy_sphere(H=24, W=40, seed=0, f=5000.0, z0=800.0, radius=60.0, noise=0.3):
    """A sphere whose nearest point lies z0 mm in front of a camera with focal length f px, as a depth-target scene: exact unit normals
    (facing the camera), the exact depth in fp64 and a prediction with Gaussian depth noise.  -> (scene dict, normal [1, 3, H, W] f32,
    z_true [1, H, W] f64)."""
    rng = np.random.RandomState(seed)
    K = np.array([[[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]]], np.float32)
    inv, _ = rc.kinv(K)
    r = rc.rays(inv, H, W, np.float64)[0]                                   # [3, H, W], r_z = 1
    c = np.array([0.0, 0.0, z0 + radius]).reshape(3, 1, 1)
    rr, rc_ = (r * r).sum(0), (r * c).sum(0)
    t = (rc_ - np.sqrt(rc_ * rc_ - rr * (float((c * c).sum()) - radius * radius))) / rr      # the near intersection of the ray t r
    P = t * r
    n = (P - c) / radius
    z = P[2]
    pred = (z + noise * rng.randn(H, W)).astype(np.float32)
    sc = dict(pred=pred[None], ab=None, K=K, mask=None, view=None, z=z[None], target_type='depth')
    return sc, n[None].astype(np.float32), z[None]


def plane(H=24, W=40):
    """rc.tilted_plane with its own normal at every pixel -> (scene dict, normal [1, 3, H, W] f32)."""
    sc, n = rc.tilted_plane(H, W)
    return sc, np.broadcast_to(n.astype(np.float32).reshape(1, 3, 1, 1), (1, 3, H, W)).copy()


def scene(B, H, W, seed, target_type='disp', masked=True, singular=None, empty=None, heads=1, noise=0.3):
    """rc.scene (a face-like surface around 800 mm with depth steps that cut edges, a mask with holes, junk predictions, optionally a
    singular K) with Gaussian depth noise on the prediction, the fp64 geometric normals of the clean surface as the normal map -- 0 where
    the surface has none -- and, among the valid pixels, an isolated one (its four neighbours masked out), normals set to 0, NaN, inf,
    grazing (perpendicular to the pixel's ray), and normals of length 3 and 0.01.  empty: a sample whose mask is 0 everywhere.  heads > 1:
    the prediction is [B, heads, H, W], the other heads filled with other values.
    -> dict(pred [B, heads, H, W], ab, K, mask, normal [B, 3, H, W] f32, target_type)."""
    sc = rc.scene(B, H, W, seed, target_type=target_type, masked=masked, singular=singular)
    rng = np.random.RandomState(seed + 1000)
    K_regular = rc.camera(B, H, W, np.random.RandomState(seed + 2000)) if singular is not None else sc['K']
    normal, _ = rc.depth_normals(sc['pred'], target_type, sc['ab'], K_regular, None, dt=np.float64)
    normal = normal.astype(np.float32)
    zn = sc['z'] + noise * rng.randn(B, H, W)
    if target_type == 'depth':
        clean, noisy = sc['z'].astype(np.float32), zn.astype(np.float32)
    else:
        b64, a64 = sc['ab'][:, 0].astype(np.float64)[:, None, None], sc['ab'][:, 1].astype(np.float64)[:, None, None]
        clean, noisy = (b64 + a64 / sc['z']).astype(np.float32), (b64 + a64 / zn).astype(np.float32)
    pred = np.where(sc['pred'] == clean, noisy, sc['pred'])                 # (the junk predictions stay)
    mask = sc['mask']
    if H >= 5 and W >= 7:
        inv, _ = rc.kinv(K_regular)
        rays = rc.rays(inv, H, W, np.float64)
        for b in range(B):
            y, x = 2, 3                                                     # an isolated valid pixel
            if mask is not None:
                mask[b, y - 1:y + 2, x - 1:x + 2] = 0.0
                mask[b, y, x] = 1.0
            picks = rng.permutation(H * W)[:7]
            for k, o in enumerate(picks):
                py, px = divmod(int(o), W)
                r = rays[b, :, py, px]
                graze = np.cross(r, [0.0, 1.0, 0.0])
                n = normal[b, :, py, px]
                normal[b, :, py, px] = ([0.0, 0.0, 0.0], [np.nan, 0.0, -1.0], [0.0, np.inf, -1.0], graze / np.linalg.norm(graze), 3.0 * n, 0.01 * n,
                                        [0.0, 0.0, 0.0])[k]
    if empty is not None:
        if mask is None:
            mask = np.ones((B, H, W), np.float32)
        mask[empty] = 0.0
    if heads > 1:
        pred = np.stack([pred] + [pred * np.float32(1.0 + 0.1 * h) for h in range(1, heads)], 1)
    else:
        pred = pred[:, None]
    return dict(pred=np.ascontiguousarray(pred), ab=sc['ab'], K=sc['K'], mask=mask, normal=normal, target_type=target_type)


# ---- the cases of tests/test_gpu_normal_refine.py: (B, H, W, target type, masked, singular K, empty sample, heads, seed)
CASES = [
    (1, 5, 7, 'depth', False, None, None, 1, 31),                # smaller than any tile
    (2, 19, 70, 'disp', True, None, None, 3, 32),                # ragged tiles on both axes, two systems, batch stride 3 H W
    (1, 33, 65, 'idepth', True, None, None, 1, 33),              # one past the tile multiples
    (3, 19, 70, 'depth', True, 2, 0, 1, 34),                     # an all-invalid sample, a live one, a singular K
]
LAM, ITERATIONS, MIN_COS, RATIO = 0.1, 32, 0.1, 0.01


def case_id(c):
    return '%dx%dx%d-%s%s%s%s%s' % (c[0], c[1], c[2], c[3], '' if c[4] else '-nomask', '' if c[5] is None else '-singular%d' % c[5],
                                    '' if c[6] is None else '-empty%d' % c[6], '' if c[7] == 1 else '-heads%d' % c[7])


_cache = {}


def case(c):
    """The scene of a case with both restatements, computed once: dict(sc, r32, r64, d32, d64 (delta as the tests recover it from the
    refined plane, and the fp64 delta itself), margin, agree).  Nothing in it may be changed by a test."""
    if c in _cache:
        return _cache[c]
    B, H, W, tt, masked, singular, empty, heads, seed = c
    sc = scene(B, H, W, seed, target_type=tt, masked=masked, singular=singular, empty=empty, heads=heads)
    plane0 = np.ascontiguousarray(sc['pred'][:, 0])
    args = (plane0, tt, sc['ab'], sc['K'], sc['mask'], sc['normal'])
    kw = dict(max_edge_ratio=RATIO, min_cos=MIN_COS, lam=LAM, iterations=ITERATIONS)
    r32, r64 = normal_refine(*args, dt=np.float32, **kw), normal_refine(*args, dt=np.float64, **kw)
    out = dict(sc=sc, r32=r32, r64=r64)
    out['d32'] = recovered_delta(r32['out'], plane0, tt, sc['ab'], r64['sy']['valid'])
    out['d64'] = r64['delta']
    out['margin'] = min(rc.margins(plane0, tt, sc['ab'], sc['K'], sc['mask'], max_edge_ratio=RATIO),
                        normal_margin(sc['K'], sc['normal'], H, W, MIN_COS))
    out['agree'] = all(np.array_equal(r32['sy'][k], r64['sy'][k]) for k in ('valid', 'right', 'down'))
    _cache[c] = out
    return out
