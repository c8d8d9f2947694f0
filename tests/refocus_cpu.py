"""The refocus block restated in numpy from its definition (include/dpf_hip.h), in fp64 or fp32 (``dtype=``): the
defocus disparity, the focus, the signed blur radius and the gather with scatter semantics.  Test infrastructure only; nothing here
touches the device or follows the kernel's loop structure -- the window is walked offset by offset over whole planes.

What is fp32 by definition stays fp32 under either dtype: d and c (stored planes, compared bit for bit), the ordering test on the stored d,
and the encoded value v = clamp(x std + mean, 0, 1) of the stored view."""
import numpy as np

from dualpixelface_amd.synthetic_refocus import IMAGENET_MEAN, IMAGENET_STD


def disparity(pred, ab=None, target_type='disp'):
    """The fp32 defocus disparity a / z + b of a map [H, W], ab = [b, a]: the map itself under 'disp' and 'idepth' (both are read as
    z = a / (pred - b)), a / pred + b under 'depth'."""
    x = np.asarray(pred, dtype=np.float32)
    if target_type != 'depth':
        return x
    b, a = np.float32(ab[0]), np.float32(ab[1])
    with np.errstate(all='ignore'):
        return (a / x + b).astype(np.float32)


def focus_pixel(point, H, W):
    """The pixel (x, y) nearest point = [u, v], fractions of width and height."""
    return min(W - 1, max(0, int(np.floor(point[0] * W)))), min(H - 1, max(0, int(np.floor(point[1] * H))))


def focus(d, mask=None, mode='mask_mean', point=(0.5, 0.5), value=0.0):
    """(d_f fp64, counted pixels, valid flag) of one sample's d [H, W]."""
    if mode == 'value':
        return float(value), 0, 1
    if mode == 'point':
        x, y = focus_pixel(point, *d.shape)
        v = d[y, x]
        return (float(v), 1, 1) if np.isfinite(v) else (0.0, 0, 0)
    on = np.isfinite(d) if mask is None else np.isfinite(d) & (np.asarray(mask) > 0)
    n = int(on.sum())
    return (float(d[on].astype(np.float64).sum() / n), n, 1) if n else (0.0, 0, 0)


def near_sign(sign='auto', ab=None):
    if sign != 'auto':
        return int(sign)
    return -1 if ab is not None and np.float32(ab[1]) < 0 else 1


def defocus(d, d_f, aperture=4.0, max_radius=16):
    """The signed blur radius c [H, W] in fp32, operation by operation: clamp(aperture (d - (float) d_f)); 0 where d is not finite."""
    d = np.asarray(d, dtype=np.float32)
    with np.errstate(all='ignore'):
        c = np.float32(aperture) * (d - np.float32(d_f))
        c = np.minimum(np.maximum(c, np.float32(-max_radius)), np.float32(max_radius))
    return np.where(np.isfinite(d), c, np.float32(0)).astype(np.float32)


def encoded(image, normalised=True):
    """v [3, H, W] fp32 in [0, 1]: the stored image de-normalised in fp32 (x std + mean) where it is the normalised view, and clamped."""
    x = np.asarray(image, dtype=np.float32)
    if normalised:
        mean, std = np.array(IMAGENET_MEAN, np.float32).reshape(3, 1, 1), np.array(IMAGENET_STD, np.float32).reshape(3, 1, 1)
        x = x * std + mean
    return np.minimum(np.maximum(x, np.float32(0)), np.float32(1))


def _shift(a, dy, dx, fill):
    """a[..., y + dy, x + dx] where that lies inside the plane, else fill."""
    H, W = a.shape[-2:]
    out = np.full_like(a, fill)
    if abs(dy) >= H or abs(dx) >= W:
        return out
    ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
    xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
    out[..., yd, xd] = a[..., ys, xs]
    return out


def render(image, d, c, sign=1, max_radius=16, gamma=2.2, gain=1.0, dtype=np.float64, normalised=True):
    """The refocused image [3, H, W] (dtype) of one sample from its d and c planes:
        O_c(p) = sum_q w(q, p) L_c(q) / sum_q w(q, p),  w = clamp(r_eff + 1 - |q - p|_2, 0, 1) / max(1, pi r_eff^2),
        r_eff = r(q), or min(r(q), r(p)) where q is behind p (sign (d(q) - d(p)) < 0),
    over the renderable q with |q - p|_inf <= max_radius; out = clamp(O^(1 / gamma) gain, 0, 1).  A pixel that is not renderable, or that
    receives from nobody but itself, keeps its encoded value."""
    t = np.dtype(dtype).type
    v = encoded(image, normalised)
    L = v.astype(dtype) if gamma == 1 else v.astype(dtype) ** t(gamma)
    d = np.asarray(d, dtype=np.float32)
    live = np.isfinite(d)
    key = np.where(live, d, np.float32(0)) * np.float32(sign)                # a source is behind a receiver iff its key is smaller
    r = np.abs(np.asarray(c, dtype=np.float32)).astype(dtype)
    one, pi = t(1), t(np.pi)
    W_other = np.zeros(d.shape, dtype)
    S = np.zeros(L.shape, dtype)
    R = int(max_radius)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if dy == 0 and dx == 0:
                continue
            lq = _shift(live, dy, dx, False)
            if not lq.any():
                continue
            rq, kq = _shift(r, dy, dx, t(0)), _shift(key, dy, dx, np.float32(0))
            reff = np.where(kq < key, np.minimum(rq, r), rq)
            dist = np.sqrt(t(dx * dx + dy * dy))
            w = np.clip(reff + one - dist, t(0), one) / np.maximum(one, pi * (reff * reff))
            w = np.where(lq, w, t(0))
            W_other += w
            S += w * _shift(L, dy, dx, t(0))
    w_self = one / np.maximum(one, pi * (r * r))
    O = (S + w_self * L) / (W_other + w_self)
    e = O if gamma == 1 else O ** (one / t(gamma))
    e = np.where(live & (W_other > 0), e, v.astype(dtype))
    return np.clip(e * t(gain), t(0), one)


def refocus(view, pred, mask=None, ab=None, target_type='disp', focus_mode='mask_mean', point=(0.5, 0.5), value=0.0, aperture=4.0, max_radius=16,
            sign='auto', gamma=2.2, gain=1.0, dtype=np.float64, normalised=True):
    """One sample end to end -> {'refocused' [3, H, W] dtype, 'defocus' [H, W] fp32, 'stats' [8] fp64}."""
    d = disparity(pred, ab, target_type)
    d_f, n, flag = focus(d, mask, focus_mode, point, value)
    c = defocus(d, d_f, aperture, max_radius)
    s = near_sign(sign, ab)
    out = render(view, d, c, s, max_radius, gamma, gain, dtype, normalised)
    return {'refocused': out, 'defocus': c, 'stats': np.array([d_f, n, flag, s, c.min(), c.max(), 0, 0], dtype=np.float64)}
