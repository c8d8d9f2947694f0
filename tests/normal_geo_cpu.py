"""The geometric-normal loss of csrc/normal_geo.hip restated twice (test infrastructure):

  * ``forward`` in numpy at a given dtype, on tests/reconstruct_cpu.py's kinv / rays / connected: np.float32 evaluates operation by
    operation in the kernels' order (normals and counted pixels compare exactly), np.float64 the same expressions in double precision
    over the same fp32 inputs (Kinv unrounded);
  * ``torch_loss`` in torch at a given dtype, which takes every discrete decision (usable, connected, the choice of step, the
    orientation sign, counted) from the fp32 numpy restatement and leaves the derivative to torch.autograd.  In fp64 its gradient is the
    reference for the hand-derived backward kernel, and it shares nothing with that derivation; in fp32 it measures what fp32 costs.

Also the scenes the tests draw and the distance of every comparison from its threshold.
"""
import numpy as np
import torch

from tests import reconstruct_cpu as rc


def _decisions(pred_h, depth, K, ab, mask, target_type, ratio, step, dt):
    """usable pixels, their predicted and target depths (0 elsewhere) and the four connectivities of every pixel, in dt."""
    inv, ok = rc.kinv(K)
    zraw = rc.raw_depth(pred_h, target_type, ab, dt)
    zt = depth.astype(dt)
    with np.errstate(invalid='ignore'):
        usable = ok[:, None, None] & (zraw > 0) & np.isfinite(zt) & (zt > 0)
        if mask is not None:
            usable &= mask > 0
    zp, ztu = np.where(usable, zraw, dt(0)), np.where(usable, zt, dt(0))
    s = step
    with np.errstate(all='ignore'):
        cl = rc.connected(rc._shift(ztu, 0, -s), ztu, ratio, dt)
        cr = rc.connected(ztu, rc._shift(ztu, 0, s), ratio, dt)
        cu = rc.connected(rc._shift(ztu, -s, 0), ztu, ratio, dt)
        cd = rc.connected(ztu, rc._shift(ztu, s, 0), ratio, dt)
    return dict(inv=inv, usable=usable, zp=zp, zt=ztu, cl=cl, cr=cr, cu=cu, cd=cd)


def _step(inv, col, cm, cp, zm, zc, zq, rc_, rq, s, dt):
    zfrom, zto = np.where(cm, zm, zc), np.where(cp, zq, zc)
    delta = np.where(cm & cp, dt(2 * s), dt(s))
    dz, t = zto - zfrom, zfrom * delta
    rto = np.where(cp[:, None], rq, rc_)
    return dz[:, None] * rto + t[:, None] * inv[:, :, col][:, :, None, None]


def forward(pred, depth, normal, K, ab=None, mask=None, head_weights=(1.0,), target_type='disp', max_edge_ratio=0.01, step=1,
            towards_camera=True, target_signs=(1, 1, 1), dt=np.float32):
    """-> dict(loss float, normal [B, n, 3, H, W] dt, counted [B, n, H, W] uint8, sigma [B, n, H, W] (+1 / -1), cos [B, n, H, W],
    count [n], sums [n], dec: the per-head decisions).  Sums are taken in fp64 over the dt terms, as the kernels do."""
    B, n, H, W = pred.shape
    s = step
    normals, counted, sigmas, coss, decs, counts, sums = [], [], [], [], [], [], []
    sg = np.asarray(target_signs, np.float32).astype(dt).reshape(1, 3, 1, 1)
    with np.errstate(all='ignore'):
        g = sg * normal.astype(dt)
        glen = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        gok = (glen > dt(np.float32(1e-6))) & np.isfinite(glen)
        gh = g / glen[:, None]
    loss = 0.0
    for h in range(n):
        d = _decisions(pred[:, h], depth, K, ab, mask, target_type, max_edge_ratio, s, dt)
        inv = d['inv'].astype(dt)
        z = d['zp']
        r0 = rc.rays(inv, H, W, dt)
        rr = rc.rays(inv, H, W, dt, xs=np.arange(W) + s)
        rd = rc.rays(inv, H, W, dt, ys=np.arange(H) + s)
        with np.errstate(all='ignore'):
            drow = _step(inv, 0, d['cl'], d['cr'], rc._shift(z, 0, -s), z, rc._shift(z, 0, s), r0, rr, s, dt)
            dcol = _step(inv, 1, d['cu'], d['cd'], rc._shift(z, -s, 0), z, rc._shift(z, s, 0), r0, rd, s, dt)
            cx = drow[:, 1] * dcol[:, 2] - drow[:, 2] * dcol[:, 1]
            cy = drow[:, 2] * dcol[:, 0] - drow[:, 0] * dcol[:, 2]
            cz = drow[:, 0] * dcol[:, 1] - drow[:, 1] * dcol[:, 0]
            length = np.sqrt((cx * cx + cy * cy) + cz * cz)
            ok = d['usable'] & (d['cl'] | d['cr']) & (d['cu'] | d['cd']) & (length > 0) & np.isfinite(length) & gok
            nn = np.stack([cx, cy, cz], 1) / length[:, None]
            dot = (nn[:, 0] * (z * r0[:, 0]) + nn[:, 1] * (z * r0[:, 1])) + nn[:, 2] * (z * r0[:, 2])
            flip = dot > 0 if towards_camera else dot < 0
            nn = np.where(flip[:, None], -nn, nn)
            cos = (nn[:, 0] * gh[:, 0] + nn[:, 1] * gh[:, 1]) + nn[:, 2] * gh[:, 2]
            term = dt(1) - np.minimum(np.maximum(cos, dt(-1)), dt(1))
        nn = np.where(ok[:, None], nn, dt(0))
        cnt = float(ok.sum())
        tot = float(np.where(ok, term, dt(0)).astype(np.float64).sum())
        if cnt > 0:
            loss += float(np.float32(head_weights[h])) * (tot / cnt)
        d.update(length=length, dot=dot, P=z[:, None] * r0)
        normals.append(nn.astype(dt)), counted.append(ok.astype(np.uint8)), sigmas.append(np.where(flip, -1, 1)), coss.append(cos)
        decs.append(d), counts.append(cnt), sums.append(tot)
    if dt is np.float32:
        loss = float(np.float32(loss))                             # the kernels hand the loss back as an fp32 scalar
    return dict(loss=loss, normal=np.stack(normals, 1), counted=np.stack(counted, 1), sigma=np.stack(sigmas, 1), cos=np.stack(coss, 1),
                count=counts, sums=sums, dec=decs, glen=glen)


def _tshift(z, dy, dx):
    """z [..., H, W] at (y + dy, x + dx), 0 outside the image (torch)."""
    out = torch.zeros_like(z)
    H, W = z.shape[-2:]
    if abs(dy) >= H or abs(dx) >= W:
        return out
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    out[..., yd, xd] = z[..., ys, xs]
    return out


def torch_loss(pred, ref, normal, K, ab=None, head_weights=(1.0,), target_type='disp', step=1, target_signs=(1, 1, 1),
               dtype=torch.float64):
    """The loss as torch expressions in `dtype` over pred (a torch tensor [B, n, H, W] of that dtype; give it requires_grad for the
    gradient), with the discrete decisions of ``ref`` = forward(..., dt=np.float32).  fp32 uses Kinv rounded to fp32 once and the
    kernels' association order; the sums are taken in fp64 either way."""
    B, n, H, W = pred.shape
    s = step
    dt = np.float32 if dtype == torch.float32 else np.float64
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a))                                         # noqa: E731
    sg = T(np.asarray(target_signs, np.float32).astype(dt).reshape(1, 3, 1, 1))
    g = sg * T(normal.astype(dt))
    glen = torch.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
    loss = torch.zeros((), dtype=torch.float64)
    for h in range(n):
        d = ref['dec'][h]
        counted = T(ref['counted'][:, h].astype(bool))
        usable = T(d['usable'])
        inv_np = d['inv'].astype(dt)
        inv = T(inv_np)
        if target_type == 'depth':
            z = torch.where(usable, pred[:, h], torch.zeros((), dtype=dtype))
        else:
            b, a = T(ab[:, 0].astype(dt))[:, None, None], T(ab[:, 1].astype(dt))[:, None, None]
            z = torch.where(usable, a / (torch.where(usable, pred[:, h], b + 1) - b), torch.zeros((), dtype=dtype))
        r0 = T(rc.rays(inv_np, H, W, dt))
        rr = T(rc.rays(inv_np, H, W, dt, xs=np.arange(W) + s))
        rd = T(rc.rays(inv_np, H, W, dt, ys=np.arange(H) + s))

        def stepv(col, cm, cp, zm, zq, rq):
            cm, cp = T(cm), T(cp)
            zfrom, zto = torch.where(cm, zm, z), torch.where(cp, zq, z)
            delta = torch.where(cm & cp, torch.tensor(2.0 * s, dtype=dtype), torch.tensor(1.0 * s, dtype=dtype))
            dz, t = zto - zfrom, zfrom * delta
            rto = torch.where(cp[:, None], rq, r0)
            return dz[:, None] * rto + t[:, None] * inv[:, :, col][:, :, None, None]

        drow = stepv(0, d['cl'], d['cr'], _tshift(z, 0, -s), _tshift(z, 0, s), rr)
        dcol = stepv(1, d['cu'], d['cd'], _tshift(z, -s, 0), _tshift(z, s, 0), rd)
        cx = drow[:, 1] * dcol[:, 2] - drow[:, 2] * dcol[:, 1]
        cy = drow[:, 2] * dcol[:, 0] - drow[:, 0] * dcol[:, 2]
        cz = drow[:, 0] * dcol[:, 1] - drow[:, 1] * dcol[:, 0]
        one = torch.ones((), dtype=dtype)
        cx, cy, cz = torch.where(counted, cx, one), torch.where(counted, cy, one), torch.where(counted, cz, one)
        length = torch.sqrt((cx * cx + cy * cy) + cz * cz)
        sigma = T(ref['sigma'][:, h].astype(dt))
        n0, n1, n2 = sigma * (cx / length), sigma * (cy / length), sigma * (cz / length)
        gl = torch.where(counted, glen, one)
        gh = torch.where(counted[:, None], g, one) / gl[:, None]
        cos = (n0 * gh[:, 0] + n1 * gh[:, 1]) + n2 * gh[:, 2]
        term = 1 - torch.clamp(cos, -1, 1)
        cnt = float(ref['count'][h])
        if cnt > 0:
            loss = loss + float(np.float32(head_weights[h])) * (torch.where(counted, term, torch.zeros((), dtype=dtype)).double().sum() / cnt)
    return loss


def loss_and_grad(case, ref, dtype):
    """(loss float, d loss / d pred as a float64 numpy array) of torch_loss in `dtype` on a case of ``cases``."""
    p = torch.tensor(case['pred'].astype(np.float32 if dtype == torch.float32 else np.float64), requires_grad=True)
    loss = torch_loss(p, ref, case['normal'], case['K'], case['ab'], case['head_weights'], case['target_type'], case['step'],
                      case['target_signs'], dtype)
    if loss.requires_grad:
        loss.backward()
        grad = p.grad.double().numpy()
    else:                                                          # nothing counted: the loss is the constant 0
        grad = np.zeros(p.shape)
    value = float(loss.detach())
    return (float(np.float32(value)) if dtype == torch.float32 else value), grad


# ---- how far the comparisons of a scene sit from their thresholds (fp64)
def margins(case):
    """The smallest relative distance, in the fp64 restatement, of a compared quantity from its threshold: |z_t(p) - z_t(q)| against
    max_edge_ratio min over every pair of usable pixels `step` apart, z_p and z_t against 0, |g| against 1e-6, and over the counted
    pixels the orientation dot against 0 (relative to |P|) and |cos| against the clamp's 1."""
    dt = np.float64
    r = forward(case['pred'], case['depth'], case['normal'], case['K'], case['ab'], case['mask'], case['head_weights'], case['target_type'],
                case['ratio'], case['step'], case['towards_camera'], case['target_signs'], dt=dt)
    s, worst = case['step'], np.inf
    zt = case['depth'].astype(dt)
    live = np.isfinite(zt) & (zt != 0)
    if live.any():
        worst = min(worst, float(np.abs(zt[live]).min()))
    gl = r['glen'][np.isfinite(r['glen'])]
    if gl.size:
        worst = min(worst, float(np.min(np.abs(gl - 1e-6) / 1e-6)))
    for h in range(case['pred'].shape[1]):
        d = r['dec'][h]
        zraw = rc.raw_depth(case['pred'][:, h], case['target_type'], case['ab'], dt)
        if (zraw != 0).any():
            worst = min(worst, float(np.abs(zraw[zraw != 0]).min()))
        z = d['zt']
        for zp, zq in ((z[:, :, :-s], z[:, :, s:]), (z[:, :-s], z[:, s:])):
            both = (zp > 0) & (zq > 0)
            if both.any():
                thr = dt(np.float32(case['ratio'])) * np.minimum(zp, zq)[both]
                worst = min(worst, float(np.min(np.abs(np.abs(zp - zq)[both] - thr) / thr)))
        on = r['counted'][:, h].astype(bool)
        if on.any():
            plen = np.sqrt((d['P'] ** 2).sum(1))
            worst = min(worst, float(np.min(np.abs(d['dot'][on]) / plen[on])))
            worst = min(worst, float(np.min(np.abs(1.0 - np.abs(r['cos'][:, h][on])))))
    return worst


# ---- scenes
def make_case(B, n, H, W, seed, target_type='disp', masked=True, bad=True, singular=None, step=1, towards_camera=True,
              target_signs=(1, 1, 1), ratio=0.01, off_clamp=False):
    """A case of the loss on reconstruct_cpu.scene's surface (a tilted, bumpy plane around 800 mm cut by depth steps): the target depth is
    the fp32 surface (with `bad` a few zero / NaN / negative / infinite pixels), every head predicts it times a smooth ripple of 0.3 % plus
    0.03 mm of noise (with `bad` the scene's NaN / Inf / out-of-range predictions on top), and the target normals are the surface's own,
    perturbed by about 0.3 rad and rescaled to lengths in [0.5, 2) (with `bad` a few zero and one NaN vector).  off_clamp: for a case
    of so many pixels that under every seed some target normal comes within margins()' 1e-4 of a predicted one (|cos| against the clamp's
    1): those few target normals are tilted by a further 0.3 rad or so, until none does."""
    sc = rc.scene(B, H, W, seed, target_type=target_type, ratio=ratio, masked=masked, bad=bad, singular=singular)
    rng = np.random.RandomState(seed + 1000)
    z, ab = sc['z'], sc['ab']
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    a64, b64 = ab[:, 1].astype(np.float64)[:, None, None], ab[:, 0].astype(np.float64)[:, None, None]
    clean = z.astype(np.float32) if target_type == 'depth' else (b64 + a64 / z).astype(np.float32)
    with np.errstate(invalid='ignore'):
        junk = ~(sc['pred'] == clean)
    pred = np.zeros((B, n, H, W), np.float32)
    for h in range(n):
        ripple = 1.0 + 0.003 * np.sin(x / 3.0 + 6.0 * rng.rand()) * np.cos(y / 4.0 + 6.0 * rng.rand())
        zh = z * ripple[None] + 0.03 * rng.randn(B, H, W)
        ph = zh.astype(np.float32) if target_type == 'depth' else (b64 + a64 / zh).astype(np.float32)
        pred[:, h] = np.where(junk, sc['pred'], ph)
    depth = z.astype(np.float32)
    n64, _ = rc.depth_normals(depth, 'depth', None, sc['K'], None, towards_camera=towards_camera, dt=np.float64)
    signs = np.asarray(target_signs, np.float64).reshape(1, 3, 1, 1)
    fallback = np.array([0.0, 0.0, -1.0 if towards_camera else 1.0]).reshape(1, 3, 1, 1)
    base = np.where((n64 ** 2).sum(1, keepdims=True) > 0, n64, fallback)
    g = base + 0.2 * rng.randn(B, 3, H, W)
    g = g / np.sqrt((g ** 2).sum(1, keepdims=True)) * (0.5 + 1.5 * rng.rand(B, 1, H, W))
    normal = (signs * g).astype(np.float32)
    if bad and H * W >= 12:
        for b in range(B):
            for v in (0.0, np.nan, -5.0, np.inf):
                depth[b, rng.randint(H), rng.randint(W)] = v
            normal[b, :, rng.randint(H), rng.randint(W)] = 0.0
            normal[b, :, rng.randint(H), rng.randint(W)] = 0.0
        normal[0, 1, rng.randint(H), rng.randint(W)] = np.nan
    weights = (1.0,) if n == 1 else tuple([1.0, 0.75294, 0.18824, 0.047059, 0.011765][:n])
    for _ in range(8 if off_clamp else 0):
        r = forward(pred, depth, normal, sc['K'], None if target_type == 'depth' else ab, sc['mask'], weights, target_type, ratio, step,
                    towards_camera, tuple(target_signs), dt=np.float64)
        near = (r['counted'].astype(bool) & (1.0 - np.abs(r['cos']) < 1e-3)).any(1)
        if not near.any():
            break
        b, yy, xx = np.nonzero(near)
        normal[b, 0, yy, xx] += np.float32(0.3) * np.sqrt((normal[b, :, yy, xx] ** 2).sum(-1))
    return dict(pred=pred, depth=depth, normal=normal, K=sc['K'], ab=None if target_type == 'depth' else ab, mask=sc['mask'],
                head_weights=weights, target_type=target_type, ratio=ratio, step=step, towards_camera=towards_camera,
                target_signs=tuple(target_signs), singular=singular)


# the cases of tests/test_gpu_normal_geo.py: name -> make_case arguments.  Seeds are chosen so that margins() >= 1e-4
# (tests/test_normal_geo_host.py checks that on the CPU); the 95 000 counted pixels of the last case need off_clamp for that.
CASES = {
    'tiny-5x7-disp': dict(B=1, n=1, H=5, W=7, seed=31, target_type='disp', masked=False, bad=False),
    'heads-19x70-idepth-singular1': dict(B=2, n=3, H=19, W=70, seed=76, target_type='idepth', masked=True, bad=True, singular=1),
    'holes-40x33-disp': dict(B=1, n=1, H=40, W=33, seed=32, target_type='disp', masked=True, bad=True),
    'step2-24x40-depth': dict(B=1, n=1, H=24, W=40, seed=32, target_type='depth', masked=False, bad=True, step=2),
    'step4-24x40-depth-away': dict(B=1, n=1, H=24, W=40, seed=31, target_type='depth', masked=True, bad=False, step=4, towards_camera=False,
                                   target_signs=(1, -1, -1)),
    # 9 x 16 tiles x 2 samples = 288 partial rows per head: the fold's r += 256 loop runs twice in some threads
    'rows288-65x500-disp': dict(B=2, n=2, H=65, W=500, seed=33, target_type='disp', masked=True, bad=True, off_clamp=True),
}

_cache = {}


def case(name):
    """A case with both numpy restatements, the torch losses and gradients in fp32 and fp64 and its margin, computed once:
    dict(case, r32, r64, loss32, grad32, loss64, grad64, margin).  Nothing in it may be changed by a test."""
    if name in _cache:
        return _cache[name]
    c = make_case(**CASES[name])
    args = (c['pred'], c['depth'], c['normal'], c['K'], c['ab'], c['mask'], c['head_weights'], c['target_type'], c['ratio'], c['step'],
            c['towards_camera'], c['target_signs'])
    out = dict(case=c, r32=forward(*args, dt=np.float32), r64=forward(*args, dt=np.float64))
    out['loss32'], out['grad32'] = loss_and_grad(c, out['r32'], torch.float32)
    out['loss64'], out['grad64'] = loss_and_grad(c, out['r32'], torch.float64)
    out['margin'] = margins(c)
    out['agree'] = bool(np.array_equal(out['r32']['counted'], out['r64']['counted']) and np.array_equal(out['r32']['sigma'] * out['r32']['counted'],
                                                                                                       out['r64']['sigma'] * out['r64']['counted']))
    _cache[name] = out
    return out


def plane_case(theta=0.0):
    """reconstruct_cpu.tilted_plane as a case of the loss: the prediction IS the target depth (the fp32 rounding of the exact plane) and
    the target normal is the plane's analytic normal turned by `theta` radians about an axis in the plane, so the loss is 1 - cos(theta)
    up to what the fp32 depth costs.  -> (case, 1 - cos(theta))"""
    sc, n_true = rc.tilted_plane()
    H, W = sc['pred'].shape[1:]
    t = np.cross(n_true, [0.0, 1.0, 0.0])
    t /= np.linalg.norm(t)
    g = np.cos(theta) * n_true + np.sin(theta) * t
    normal = np.broadcast_to(g.reshape(1, 3, 1, 1), (1, 3, H, W)).astype(np.float32)
    c = dict(pred=sc['pred'][:, None].copy(), depth=sc['pred'].copy(), normal=normal, K=sc['K'], ab=None, mask=None, head_weights=(1.0,),
             target_type='depth', ratio=0.01, step=1, towards_camera=True, target_signs=(1, 1, 1), singular=None)
    return c, 1.0 - float(np.cos(theta))


def run(c, dt=np.float32):
    """forward() on a case dict."""
    return forward(c['pred'], c['depth'], c['normal'], c['K'], c['ab'], c['mask'], c['head_weights'], c['target_type'], c['ratio'], c['step'],
                   c['towards_camera'], c['target_signs'], dt=dt)
