"""The photometric and smoothness losses of csrc/photometric.hip restated twice (test infrastructure):

  * ``forward`` / ``smooth_forward`` in numpy at a given dtype: np.float32 evaluates operation by operation in the kernels' order (the
    warped values and the counted map compare exactly), np.float64 the same expressions in double precision over the same fp32 inputs;
  * ``torch_loss`` / ``smooth_torch_loss`` in torch at a given dtype, which take every discrete decision (warpable, the tap indices of
    the bilinear sample, counted, usable pairs) from the fp32 numpy restatement and leave the derivative to torch.autograd.  In fp64 the
    gradient is the reference for the hand-derived backward kernels and shares nothing with that derivation; in fp32 it measures what
    fp32 costs.

The fp32 operation order, the one the kernels follow:

    Y     = (0.299 * (x0 * std0 + mean0) + 0.587 * (x1 * std1 + mean1)) + 0.114 * (x2 * std2 + mean2)
    D     = pred, or a / pred + b for target type 'depth'
    sx    = float(x) + shift_x * D;  sy = float(y) + shift_y * D
    x0    = floor(sx); fx = sx - x0; x1 = min(x0 + 1, W - 1); likewise y
    top   = v00 + fx * (v01 - v00); bot = v10 + fx * (v11 - v10); J = top + fy * (bot - top)
    sums  i = I - c, j = J - c with c = I at the centre (the variances are then differences of small numbers); sI, sJ, sII, sJJ, sIJ start
          at 0 and take the nine pixels in row-major order, s = s + value, the products i * i, j * j, i * j
    mu_I  = c + m_I, m_I = sI / 9, likewise J; var_I = sII / 9 - m_I * m_I; var_J likewise; cov = sIJ / 9 - m_I * m_J
    SSIM  = (((2 * mu_I) * mu_J + C1) * (2 * cov + C2)) / (((mu_I * mu_I + mu_J * mu_J) + C1) * ((var_I + var_J) + C2))
    term  = alpha * clamp((1 - SSIM) / 2, 0, 1) + (1 - alpha) * sqrt(d * d + eps * eps), d = J - I at the centre
    pair  sqrt(d * d + eps * eps) * exp(-(gamma * |Y_q - Y_p|)), d = pred_q - pred_p

Sums over pixels are taken in fp64 over the terms.  Also the scenes the tests draw: smooth images and a smooth displacement field, so that
the bilinear derivative means something.
"""
import numpy as np
import torch

MEAN = (0.485, 0.456, 0.406)            # the data path's Normalizer (dualpixelface_amd.facedp.IMAGENET_MEAN / _STD; the host tests
STD = (0.229, 0.224, 0.225)             # check that they are these)
C1, C2 = 0.01 ** 2, 0.03 ** 2


def luma(img, dt=np.float32):
    """Y [B, H, W] of a normalised image [B, 3, H, W] (fp32 data) in dt."""
    m, s = [dt(np.float32(v)) for v in MEAN], [dt(np.float32(v)) for v in STD]
    x = img.astype(dt)
    r, g, b = x[:, 0] * s[0] + m[0], x[:, 1] * s[1] + m[1], x[:, 2] * s[2] + m[2]
    return (dt(np.float32(0.299)) * r + dt(np.float32(0.587)) * g) + dt(np.float32(0.114)) * b


def _box(parts, H, W):
    """the nine shifted interior views [B, H - 2, W - 2] of X [B, H, W], row-major"""
    return [parts[:, 1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def _warp(pred_h, ytgt, ab, mask, target_type, shift, dt):
    """One head: warpable [B, H, W], J (0 where not warpable), and the taps (y0, y1, x0, x1 int arrays, clipped where not warpable)."""
    B, H, W = pred_h.shape
    p = pred_h.astype(dt)
    with np.errstate(all='ignore'):
        ok = np.isfinite(p)
        if mask is not None:
            ok &= mask > 0
        D = p
        if target_type == 'depth':
            ok &= p > 0
            b, a = ab[:, 0].astype(dt)[:, None, None], ab[:, 1].astype(dt)[:, None, None]
            D = a / p + b
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
        sx = xs.astype(dt)[None] + dt(np.float32(shift[0])) * D
        sy = ys.astype(dt)[None] + dt(np.float32(shift[1])) * D
        ok &= (sx >= 0) & (sx <= dt(W - 1)) & (sy >= 0) & (sy <= dt(H - 1))
        sx, sy = np.where(ok, sx, dt(0)), np.where(ok, sy, dt(0))
        fx0, fy0 = np.floor(sx), np.floor(sy)
        fx, fy = sx - fx0, sy - fy0
        x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        bi = np.arange(B)[:, None, None]
        v00, v01, v10, v11 = ytgt[bi, y0, x0], ytgt[bi, y0, x1], ytgt[bi, y1, x0], ytgt[bi, y1, x1]
        top, bot = v00 + fx * (v01 - v00), v10 + fx * (v11 - v10)
        J = top + fy * (bot - top)
    return ok, np.where(ok, J, dt(0)), (y0, y1, x0, x1), (fx, fy)


def forward(pred, ref_rgb, tgt_rgb, ab=None, mask=None, head_weights=(1.0,), target_type='disp', shift=(0.0, -2.0), alpha=0.85, eps=1e-3,
            dt=np.float32):
    """-> dict(loss float, warped [B, n, H, W] dt, counted [B, n, H, W] uint8, warpable, taps, frac (per head), count [n], sums [n],
    clamped: counted pixels whose (1 - SSIM) / 2 lies outside [0, 1])."""
    B, n, H, W = pred.shape
    I, Yt = luma(ref_rgb, dt), luma(tgt_rgb, dt)
    al, ep, one, nine = dt(np.float32(alpha)), dt(np.float32(eps)), dt(1), dt(9)
    c1, c2 = dt(np.float32(C1)), dt(np.float32(C2))
    out = dict(warped=[], counted=[], warpable=[], taps=[], frac=[], count=[], sums=[], clamped=[])
    loss = 0.0
    for h in range(n):
        ok, J, taps, frac = _warp(pred[:, h], Yt, ab, mask, target_type, shift, dt)
        counted = np.zeros((B, H, W), bool)
        term = np.zeros((B, H, W), dt)
        clamped = np.zeros((B, H, W), bool)
        if H >= 3 and W >= 3:
            inner = np.ones((B, H - 2, W - 2), bool)
            for v in _box(ok, H, W):
                inner &= v
            c = I[:, 1:-1, 1:-1]
            sI = sJ = sII = sJJ = sIJ = np.zeros((B, H - 2, W - 2), dt)
            for i, j in zip(_box(I, H, W), _box(J, H, W)):
                i, j = i - c, j - c
                sI, sJ, sII, sJJ, sIJ = sI + i, sJ + j, sII + i * i, sJJ + j * j, sIJ + i * j
            mI, mJ = sI / nine, sJ / nine
            muI, muJ = c + mI, c + mJ
            vI, vJ, cov = sII / nine - mI * mI, sJJ / nine - mJ * mJ, sIJ / nine - mI * mJ
            with np.errstate(all='ignore'):
                ssim = (((dt(2) * muI) * muJ + c1) * (dt(2) * cov + c2)) / (((muI * muI + muJ * muJ) + c1) * ((vI + vJ) + c2))
                ds = (one - ssim) / dt(2)
                d = J[:, 1:-1, 1:-1] - I[:, 1:-1, 1:-1]
                t = al * np.minimum(np.maximum(ds, dt(0)), one) + (one - al) * np.sqrt(d * d + ep * ep)
            counted[:, 1:-1, 1:-1] = inner
            term[:, 1:-1, 1:-1] = np.where(inner, t, dt(0))
            clamped[:, 1:-1, 1:-1] = inner & ~((ds >= 0) & (ds <= 1))
        cnt, tot = float(counted.sum()), float(term.astype(np.float64).sum())
        if cnt > 0:
            loss += float(np.float32(head_weights[h])) * (tot / cnt)
        for key, val in zip(('warped', 'counted', 'warpable', 'taps', 'frac', 'count', 'sums', 'clamped'),
                            (J, counted.astype(np.uint8), ok, taps, frac, cnt, tot, clamped)):
            out[key].append(val)
    if dt is np.float32:
        loss = float(np.float32(loss))                             # the kernels hand the loss back as an fp32 scalar
    out['warped'], out['counted'] = np.stack(out['warped'], 1), np.stack(out['counted'], 1)
    out['loss'], out['Y_ref'], out['Y_tgt'] = loss, I, Yt
    return out


def _tluma(img, dtype):
    dt = np.float32 if dtype == torch.float32 else np.float64
    return torch.as_tensor(luma(img, dt))


def torch_loss(pred, ref, ref_rgb, tgt_rgb, ab=None, head_weights=(1.0,), target_type='disp', shift=(0.0, -2.0), alpha=0.85, eps=1e-3,
               dtype=torch.float64):
    """The loss as torch expressions in `dtype` over pred (a torch tensor [B, n, H, W] of that dtype), with the discrete decisions of
    ``ref`` = forward(..., dt=np.float32): warpable, the taps, counted.  The clamp is torch.clamp (it passes the gradient on [0, 1])."""
    B, n, H, W = pred.shape
    dt = np.float32 if dtype == torch.float32 else np.float64
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a))                                          # noqa: E731
    I, Yt = _tluma(ref_rgb, dtype), _tluma(tgt_rgb, dtype)
    al, ep = float(dt(np.float32(alpha))), float(dt(np.float32(eps)))
    c1, c2 = float(dt(np.float32(C1))), float(dt(np.float32(C2)))
    sx_, sy_ = float(np.float32(shift[0])), float(np.float32(shift[1]))
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing='ij')
    bi = torch.arange(B)[:, None, None]
    zero = torch.zeros((), dtype=dtype)
    loss = torch.zeros((), dtype=torch.float64)
    for h in range(n):
        ok, counted = T(ref['warpable'][h]), T(ref['counted'][:, h].astype(bool))
        y0, y1, x0, x1 = [T(t) for t in ref['taps'][h]]
        p = torch.where(ok, pred[:, h], torch.ones((), dtype=dtype))
        D = p
        if target_type == 'depth':
            b, a = T(ab[:, 0].astype(dt))[:, None, None], T(ab[:, 1].astype(dt))[:, None, None]
            D = a / p + b
        sx, sy = xs[None] + sx_ * D, ys[None] + sy_ * D
        fx, fy = sx - x0.to(dtype), sy - y0.to(dtype)
        v00, v01, v10, v11 = Yt[bi, y0, x0], Yt[bi, y0, x1], Yt[bi, y1, x0], Yt[bi, y1, x1]
        top, bot = v00 + fx * (v01 - v00), v10 + fx * (v11 - v10)
        J = torch.where(ok, top + fy * (bot - top), zero)
        if not (H >= 3 and W >= 3 and ref['count'][h] > 0):
            continue
        c = I[:, 1:-1, 1:-1]
        sI = sJ = sII = sJJ = sIJ = torch.zeros((B, H - 2, W - 2), dtype=dtype)
        for i, j in zip(_box(I, H, W), _box(J, H, W)):
            i, j = i - c, j - c
            sI, sJ, sII, sJJ, sIJ = sI + i, sJ + j, sII + i * i, sJJ + j * j, sIJ + i * j
        mI, mJ = sI / 9, sJ / 9
        muI, muJ = c + mI, c + mJ
        vI, vJ, cov = sII / 9 - mI * mI, sJJ / 9 - mJ * mJ, sIJ / 9 - mI * mJ
        ssim = (((2 * muI) * muJ + c1) * (2 * cov + c2)) / (((muI * muI + muJ * muJ) + c1) * ((vI + vJ) + c2))
        d = J[:, 1:-1, 1:-1] - I[:, 1:-1, 1:-1]
        t = al * torch.clamp((1 - ssim) / 2, 0, 1) + (1 - al) * torch.sqrt(d * d + ep * ep)
        tot = torch.where(counted[:, 1:-1, 1:-1], t, zero).double().sum()
        loss = loss + float(np.float32(head_weights[h])) * (tot / float(ref['count'][h]))
    return loss


# ---- smoothness
def _pairs(pred_h, mask):
    with np.errstate(invalid='ignore'):
        ok = np.isfinite(pred_h)
        if mask is not None:
            ok = ok & (mask > 0)
    return ok[:, :, :-1] & ok[:, :, 1:], ok[:, :-1] & ok[:, 1:]


def smooth_forward(pred, guide_rgb, mask=None, head_weights=(1.0,), gamma=10.0, eps=1e-3, dt=np.float32):
    """-> dict(loss, use_x [n][B, H, W - 1], use_y [n][B, H - 1, W], count_x, count_y, sum_x, sum_y)."""
    B, n, H, W = pred.shape
    Y = luma(guide_rgb, dt)
    ga, ep = dt(np.float32(gamma)), dt(np.float32(eps))
    out = dict(use_x=[], use_y=[], count_x=[], count_y=[], sum_x=[], sum_y=[])
    loss = 0.0
    for h in range(n):
        p = pred[:, h].astype(dt)
        ux, uy = _pairs(pred[:, h], mask)
        with np.errstate(all='ignore'):
            dx, dy = p[:, :, 1:] - p[:, :, :-1], p[:, 1:] - p[:, :-1]
            tx = np.sqrt(dx * dx + ep * ep) * np.exp(-(ga * np.abs(Y[:, :, 1:] - Y[:, :, :-1])))
            ty = np.sqrt(dy * dy + ep * ep) * np.exp(-(ga * np.abs(Y[:, 1:] - Y[:, :-1])))
        for key, u, t in (('x', ux, tx), ('y', uy, ty)):
            cnt, tot = float(u.sum()), float(np.where(u, t, dt(0)).astype(np.float64).sum())
            if cnt > 0:
                loss += float(np.float32(head_weights[h])) * (tot / cnt)
            out['use_' + key].append(u), out['count_' + key].append(cnt), out['sum_' + key].append(tot)
    out['loss'] = float(np.float32(loss)) if dt is np.float32 else loss
    return out


def smooth_torch_loss(pred, ref, guide_rgb, head_weights=(1.0,), gamma=10.0, eps=1e-3, dtype=torch.float64):
    """The smoothness loss in torch over pred [B, n, H, W] of `dtype`, the usable pairs taken from ``ref`` = smooth_forward(...)."""
    dt = np.float32 if dtype == torch.float32 else np.float64
    Y = _tluma(guide_rgb, dtype)
    ga, ep = float(dt(np.float32(gamma))), float(dt(np.float32(eps)))
    wx, wy = torch.exp(-(ga * (Y[:, :, 1:] - Y[:, :, :-1]).abs())), torch.exp(-(ga * (Y[:, 1:] - Y[:, :-1]).abs()))
    zero = torch.zeros((), dtype=dtype)
    loss = torch.zeros((), dtype=torch.float64)
    for h in range(pred.shape[1]):
        ux, uy = torch.as_tensor(ref['use_x'][h]), torch.as_tensor(ref['use_y'][h])
        p = pred[:, h]
        dx = torch.where(ux, p[:, :, 1:], zero) - torch.where(ux, p[:, :, :-1], zero)
        dy = torch.where(uy, p[:, 1:], zero) - torch.where(uy, p[:, :-1], zero)
        for u, d, w, cnt in ((ux, dx, wx, ref['count_x'][h]), (uy, dy, wy, ref['count_y'][h])):
            if cnt > 0:
                tot = torch.where(u, torch.sqrt(d * d + ep * ep) * w, zero).double().sum()
                loss = loss + float(np.float32(head_weights[h])) * (tot / float(cnt))
    return loss


def _grad(fn, pred, dtype):
    """(loss float, d loss / d pred float64 numpy) of fn(p) with p = pred in dtype; non-finite entries of pred are replaced by 0 for torch
    (the decisions already exclude them, and autograd would carry their NaN through a where)."""
    clean = np.where(np.isfinite(pred), pred, 0.0)
    p = torch.tensor(clean.astype(np.float32 if dtype == torch.float32 else np.float64), requires_grad=True)
    loss = fn(p)
    if loss.requires_grad:
        loss.backward()
        grad = p.grad.double().numpy()
    else:
        grad = np.zeros(p.shape)
    value = float(loss.detach())
    return (float(np.float32(value)) if dtype == torch.float32 else value), grad


# ---- scenes
def smooth_noise(rng, shape, H, W, cells=4):
    """Uniform noise in [0, 1) on a (cells + 1)^2 grid, upsampled bilinearly to H x W (fp64): a field whose slope is about cells / size."""
    g = rng.rand(*shape, cells + 1, cells + 1)
    y, x = np.linspace(0, cells, H), np.linspace(0, cells, W)
    y0, x0 = np.minimum(y.astype(int), cells - 1), np.minimum(x.astype(int), cells - 1)
    fy, fx = (y - y0)[:, None], (x - x0)[None, :]
    a, b = g[..., y0, :][..., :, x0], g[..., y0, :][..., :, x0 + 1]
    c, d = g[..., y0 + 1, :][..., :, x0], g[..., y0 + 1, :][..., :, x0 + 1]
    return (a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy


def normalise(rgb):
    """de-normalised RGB [B, 3, H, W] in [0, 1] -> the fp32 normalised image the data path hands out"""
    m, s = np.asarray(MEAN).reshape(1, 3, 1, 1), np.asarray(STD).reshape(1, 3, 1, 1)
    return ((rgb - m) / s).astype(np.float32)


def sample64(img, sx, sy):
    """img [B, C, H, W] sampled bilinearly at (sx, sy) [B, H, W], coordinates clipped to the image (fp64)."""
    B, C, H, W = img.shape
    sx, sy = np.clip(sx, 0, W - 1), np.clip(sy, 0, H - 1)
    x0, y0 = np.minimum(np.floor(sx).astype(int), W - 2), np.minimum(np.floor(sy).astype(int), H - 2)
    fx, fy = (sx - x0)[:, None], (sy - y0)[:, None]
    bi, ci = np.arange(B)[:, None, None, None], np.arange(C)[None, :, None, None]
    y0, x0 = y0[:, None], x0[:, None]
    top = img[bi, ci, y0, x0] * (1 - fx) + img[bi, ci, y0, x0 + 1] * fx
    bot = img[bi, ci, y0 + 1, x0] * (1 - fx) + img[bi, ci, y0 + 1, x0 + 1] * fx
    return top * (1 - fy) + bot * fy


def ellipse(B, H, W, semi=0.45):
    y, x = np.meshgrid((np.arange(H) + 0.5) / H - 0.5, (np.arange(W) + 0.5) / W - 0.5, indexing='ij')
    return np.broadcast_to((((x / semi) ** 2 + (y / semi) ** 2) <= 1.0).astype(np.float32), (B, H, W)).copy()


def make_case(B, n, H, W, seed, shift=(0.0, -2.0), target_type='disp', dmax=1.5, masked=True, bad=False, fractions=False):
    """A case: the target view is a smooth image, the reference view is the target warped by a smooth field D0 (|D0| <= dmax) plus a
    smooth change of brightness of up to 0.05, and every head predicts D0 plus a smooth error of up to 0.15 dmax.  masked: the ellipse of
    semi-axes 0.45; bad: NaN / Inf / 0 in pred under the mask and outside it.  fractions: D0 and the heads are drawn so that the
    fractional part of every sample coordinate along a shifted axis lies in [0.1, 0.9] (one axis shifted, |shift| D in (0.1, 0.9) - 1)."""
    rng = np.random.RandomState(seed)
    tgt = 0.1 + 0.8 * smooth_noise(rng, (B, 3), H, W, cells=5)
    if fractions:
        assert (shift[0] == 0) != (shift[1] == 0)
        s = shift[0] if shift[0] != 0 else shift[1]
        D0 = (-0.88 + 0.76 * smooth_noise(rng, (B,), H, W, cells=2)) / s
        heads = [(-0.88 + 0.76 * smooth_noise(rng, (B,), H, W, cells=2)) / s for _ in range(n)]
    else:
        D0 = dmax * (2 * smooth_noise(rng, (B,), H, W, cells=3) - 1)
        heads = [D0 + 0.15 * dmax * (2 * smooth_noise(rng, (B,), H, W, cells=3) - 1) for _ in range(n)]
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    ref = sample64(tgt, xs[None] + shift[0] * D0, ys[None] + shift[1] * D0) + 0.05 * (2 * smooth_noise(rng, (B, 1), H, W, cells=3) - 1)
    ab = None
    pred = np.stack(heads, 1)
    if target_type == 'depth':
        ab = np.tile(np.array([[-4.0, 2000.0]], np.float32), (B, 1))                # D = a / pred + b: pred = a / (D - b), about 500
        ab[:, 1] += np.arange(B, dtype=np.float32) * 100
        pred = ab[:, 1].astype(np.float64)[:, None, None, None] / (pred - ab[:, 0].astype(np.float64)[:, None, None, None])
    pred = pred.astype(np.float32)
    mask = ellipse(B, H, W) if masked else None
    if bad:
        on, off = np.argwhere(mask[0] > 0), np.argwhere(~(mask[0] > 0))
        for k, v in enumerate((np.nan, np.inf, 0.0, -np.inf)):
            y, x = on[rng.randint(len(on))]
            pred[k % B, k % n, y, x] = v
            y, x = off[rng.randint(len(off))]
            pred[(k + 1) % B, (k + 1) % n, y, x] = v
    weights = (1.0,) if n == 1 else tuple([1.0, 0.75294, 0.18824, 0.047059, 0.011765][:n])
    return dict(pred=pred, ref_rgb=normalise(ref), tgt_rgb=normalise(tgt), ab=ab, mask=mask, head_weights=weights, target_type=target_type,
                shift=tuple(float(v) for v in shift), alpha=0.85, eps=1e-3, gamma=10.0, D0=D0)


# the cases of tests/test_gpu_photometric.py: name -> make_case arguments (tests/test_photometric_host.py checks on the CPU that each
# counts at least a quarter of its pixels and fewer than all)
CASES = {
    'tiny-7x9': dict(B=1, n=1, H=7, W=9, seed=11, shift=(0.0, -2.0), masked=False, fractions=True),
    'multi-tile-19x70': dict(B=2, n=3, H=19, W=70, seed=12, shift=(0.0, -2.0), masked=True, bad=True),
    'horizontal': dict(B=2, n=3, H=19, W=70, seed=13, shift=(1.5, 0.0), masked=True),
    'diagonal-33x40': dict(B=1, n=2, H=33, W=40, seed=14, shift=(-1.0, 0.5), masked=False),
    'depth-type': dict(B=2, n=1, H=16, W=35, seed=15, shift=(0.0, -2.0), target_type='depth', masked=False),
    # 9 x 16 tiles x 2 samples = 288 partial rows per head: the fold's r += 256 loop runs twice in some threads
    'rows288-65x500': dict(B=2, n=2, H=65, W=500, seed=16, shift=(0.0, -2.0), masked=True, bad=True),
}

_cache = {}


def run(c, dt=np.float32, **over):
    c = dict(c, **over)
    return forward(c['pred'], c['ref_rgb'], c['tgt_rgb'], c['ab'], c['mask'], c['head_weights'], c['target_type'], c['shift'], c['alpha'],
                   c['eps'], dt=dt)


def run_smooth(c, dt=np.float32, **over):
    c = dict(c, **over)
    return smooth_forward(c['pred'], c['ref_rgb'], c['mask'], c['head_weights'], c['gamma'], c['eps'], dt=dt)


def loss_and_grad(c, r32, dtype):
    return _grad(lambda p: torch_loss(p, r32, c['ref_rgb'], c['tgt_rgb'], c['ab'], c['head_weights'], c['target_type'], c['shift'],
                                      c['alpha'], c['eps'], dtype), c['pred'], dtype)


def smooth_loss_and_grad(c, r32, dtype):
    return _grad(lambda p: smooth_torch_loss(p, r32, c['ref_rgb'], c['head_weights'], c['gamma'], c['eps'], dtype), c['pred'], dtype)


def case(name):
    """A case with both numpy restatements and the torch losses and gradients in fp32 and fp64, computed once: dict(case, r32, r64, loss32,
    grad32, loss64, grad64).  Nothing in it may be changed by a test."""
    if name not in _cache:
        c = make_case(**CASES[name])
        out = dict(case=c, r32=run(c), r64=run(c, np.float64))
        out['loss32'], out['grad32'] = loss_and_grad(c, out['r32'], torch.float32)
        out['loss64'], out['grad64'] = loss_and_grad(c, out['r32'], torch.float64)
        _cache[name] = out
    return _cache[name]


def smooth_case(name):
    """The smoothness loss on the same scene: dict(case, r32, r64, loss32, grad32, loss64, grad64)."""
    key = ('smooth', name)
    if key not in _cache:
        c = make_case(**CASES[name])
        out = dict(case=c, r32=run_smooth(c), r64=run_smooth(c, np.float64))
        out['loss32'], out['grad32'] = smooth_loss_and_grad(c, out['r32'], torch.float32)
        out['loss64'], out['grad64'] = smooth_loss_and_grad(c, out['r32'], torch.float64)
        _cache[key] = out
    return _cache[key]
