"""The confidence planes and the sparsification table of csrc/head_confidence.hip restated (test infrastructure):

  * ``planes(..., dtype=np.float32)``: numpy fp32, operation by operation in the kernel's order (numpy rounds every operation, as
    -ffp-contract=off does).  The upsample is tests/unimodal_cpu.py's.  `lstar` and the bad map compare exactly.
  * ``planes(..., dtype=np.float64)``: the same formulas in fp64 over the fp64 upsample of the same fp32 taps; the reference of the five
    planes.  The discrete decision l* is handed over from the fp32 run (`lstar=`), as the counted map is in tests/unimodal_cpu.py.
  * ``curve``: the table in fp64 with fp32 t, |pred - t| and bin, as the kernel takes them.

The order (per head and pixel, every sum over l ascending):

    x_l = u_l - mx, mx = fmax over l starting from -3.4e38 (a NaN is skipped);  e_l = exp(x_l);  S = sum e_l;  p_l = e_l / S
    l*  = the smallest l with u_l == mx, 0 where there is none
    peak = 1 / S;  Hent = log(S) - sum p_l x_l;  entropy = clamp(1 - Hent / log(float(L)), 0, 1)
    mu = sum p_l d_l;  var = sum p_l ((d_l - mu) (d_l - mu));  spread = sqrt(var)
    M = sum over |l - l*| <= r of p_l;  mass = min(M, 1);  modal = (sum over |l - l*| <= r of p_l d_l) / M
    bad = S, Hent, var or modal not finite: peak = entropy = mass = 0, spread = modal = NaN
"""
import numpy as np

from tests import unimodal_cpu as uc

F32 = np.float32
NAMES = ('peak', 'entropy', 'mass', 'spread', 'modal')


def upsample64(k, scale, align):
    """unimodal_cpu.upsample with the same fp32 taps and fractions, the products and sums in fp64."""
    B, _, D, h, w = k.shape
    q = k[:, 0].astype(np.float64)
    y0, y1, ly = uc.taps(scale * h, h, align)
    x0, x1, lx = uc.taps(scale * w, w, align)
    d0, d1, ld = uc.taps(scale * D, D, align)
    ly, lx, ld = [v.astype(np.float64) for v in (ly[None, None, :, None], lx[None, None, None, :], ld[None, :, None, None])]
    g = lambda ys, xs: q[:, :, ys][:, :, :, xs]                                                        # noqa: E731
    bl = (1 - ly) * ((1 - lx) * g(y0, x0) + lx * g(y0, x1)) + ly * ((1 - lx) * g(y1, x0) + lx * g(y1, x1))
    return (1 - ld) * bl[:, d0] + ld * bl[:, d1]


def _seq(parts, dtype):
    s = np.zeros(parts.shape[1:], dtype=dtype)
    for p in parts:
        s = (s + p).astype(dtype)
    return s


def head_planes(u, disp, r, dtype=F32, lstar=None):
    """The planes of one head from its upsampled logits u [B, L, H, W] (of `dtype`) -> dict of [B, H, W] arrays: NAMES, 'lstar' (int32),
    'bad' (bool), 'var', 'mu', 'S', 'gap' (the difference of the two largest u_l) and 'umax' (max |u_l|)."""
    T = dtype
    u = np.moveaxis(np.asarray(u, dtype=T), 1, 0)                                                      # [L, B, H, W]
    L = u.shape[0]
    d = np.asarray(disp, dtype=F32).astype(T)[:, None, None, None]
    with np.errstate(all='ignore'):
        mx = np.full(u.shape[1:], T(-3.4e38), dtype=T)
        for ul in u:
            mx = np.fmax(mx, ul)
        x = (u - mx).astype(T)
        e = np.exp(x).astype(T)
        S = _seq(e, T)
        hit = u == mx
        ls = np.where(hit.any(0), hit.argmax(0), 0).astype(np.int32) if lstar is None else np.asarray(lstar, dtype=np.int32)
        p = (e / S).astype(T)
        cross = _seq((p * x).astype(T), T)
        mu = _seq((p * d).astype(T), T)
        inside = np.abs(np.arange(L, dtype=np.int32)[:, None, None, None] - ls[None]) <= r
        M = _seq(np.where(inside, p, T(0)), T)
        N = _seq(np.where(inside, (p * d).astype(T), T(0)), T)
        dm = (d - mu).astype(T)
        var = _seq((p * (dm * dm).astype(T)).astype(T), T)
        Hent = (np.log(S).astype(T) - cross).astype(T)
        modal = (N / M).astype(T)
        bad = ~(np.isfinite(S) & np.isfinite(Hent) & np.isfinite(var) & np.isfinite(modal))
        ent = np.minimum(np.maximum((T(1) - (Hent / np.log(T(L)).astype(T)).astype(T)).astype(T), T(0)), T(1))
        srt = np.sort(np.where(np.isnan(u), T(-np.inf), u), axis=0)
        out = dict(peak=np.where(bad, T(0), (T(1) / S).astype(T)), entropy=np.where(bad, T(0), ent),
                   mass=np.where(bad, T(0), np.minimum(M, T(1))), spread=np.where(bad, T(np.nan), np.sqrt(var).astype(T)),
                   modal=np.where(bad, T(np.nan), modal), lstar=ls, bad=bad, var=var, mu=mu, S=S, gap=srt[-1] - srt[-2],
                   umax=np.abs(u).max(0))
    return out


def planes(logits, disp, scale=4, align=True, r=1, dtype=F32, lstar=None):
    """All heads -> dict of [B, n, H, W] arrays (head_planes).  lstar: [B, n, H, W] to take the peak index from."""
    heads = []
    for i, k in enumerate(logits):
        u = uc.upsample(k, scale, align) if dtype is F32 else upsample64(k, scale, align)
        heads.append(head_planes(u, disp, r, dtype, None if lstar is None else lstar[:, i]))
    return {key: np.stack([hd[key] for hd in heads], 1) for key in heads[0]}


def near_tie(p32):
    """The pixels the exact comparisons may leave out: the two largest fp32 u_l differ by more than 0 and less than 8 * 2^-24 * max |u|."""
    return (p32['gap'] > 0) & (p32['gap'] < 8 * 2.0 ** -24 * p32['umax'])


def curve(conf, pred, target, mask=None, ab=None, bins=16):
    """-> (table [bins, 2] float64 = (count, sum |pred - t|), counted [B, H, W] bool, err [B, H, W] fp32, bin [B, H, W] int)."""
    with np.errstate(all='ignore'):
        t = target.astype(F32)
        if ab is not None:
            b, a = ab[:, 0].astype(F32)[:, None, None], ab[:, 1].astype(F32)[:, None, None]
            t = (a / t + b).astype(F32)
        conf, pred = conf.astype(F32), pred.astype(F32)
        ok = np.isfinite(t) & np.isfinite(pred) & np.isfinite(conf)
        if mask is not None:
            ok &= mask > 0
        err = np.abs((pred - t).astype(F32))
        scaled = (conf * F32(bins)).astype(F32)
        which = np.where(np.isfinite(scaled), np.minimum(np.maximum(scaled, F32(0)), F32(bins - 1)), 0).astype(np.int64)
    table = np.zeros((bins, 2), dtype=np.float64)
    for k in range(bins):
        sel = ok & (which == k)
        table[k] = sel.sum(), err[sel].astype(np.float64).sum()
    return table, ok, err, which
