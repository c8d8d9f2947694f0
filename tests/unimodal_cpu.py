"""The unimodal loss of csrc/unimodal.hip restated three times (test infrastructure):

  * ``torch_loss(dtype=torch.float64)``: F.interpolate(mode='trilinear') + log_softmax + the softmax of -|d_l - t| / s, the derivative
    left to torch.autograd.  The reference of loss and gradient; it shares neither the index arithmetic nor the hand-derived backward
    with the kernels.  Only the discrete decision `counted` is taken from the fp32 restatement.
  * ``torch_loss(dtype=torch.float32)``: the same formulation in fp32, which measures what fp32 costs.
  * ``forward`` in numpy fp32, operation by operation in the kernels' order (numpy rounds every operation, as -ffp-contract=off does):
    the counted map compares exactly.

The fp32 operation order, the one the kernels follow (csrc/dpf_softargmin.h, csrc/unimodal.hip):

    ratio = float(in - 1) / float(out - 1) (0 for out = 1) and off = 0 under align_corners, else float(in) / float(out) and off = 0.5
    src   = ratio * (float(dst) + off) - off, at least 0;  i0 = min(int(src), in - 1);  i1 = i0 + (i0 < in - 1);  lam = src - float(i0)
    bl_d  = hy * (hx * q[y0, x0] + lx * q[y0, x1]) + ly * (hx * q[y1, x0] + lx * q[y1, x1]),  hy = 1 - ly, hx = 1 - lx
    u_l   = (1 - ld) * bl[d0] + ld * bl[d1]
    t     = target, or a / target + b
    mx    = max_l u_l;  S = sum over l in order of exp(u_l - mx);  lg = log(S);  lse = mx + lg
    m     = min_l |d_l - t|;  e_l = exp(-((|d_l - t| - m) / s));  Z = sum over l in order of e_l
    term  = lg - (sum over l in order of (e_l / Z) * (u_l - mx))
    expect = sum over l in order of (exp(u_l - mx) / S) * d_l

Sums over pixels are taken in fp64 over the terms; the loss is float32(sum_h double(w_h) * (sum_h / count_h)).  Also the cases the tests
draw.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32


def taps(out, inn, align):
    """ac_src of csrc/dpf_softargmin.h for every dst < out: (i0, i1, lam), in fp32."""
    dst = np.arange(out, dtype=F32)
    if align:
        ratio, off = (F32(inn - 1) / F32(out - 1) if out > 1 else F32(0)), F32(0)
    else:
        ratio, off = F32(inn) / F32(out), F32(0.5)
    src = ratio * (dst + off) - off
    src = np.where(src < 0, F32(0), src).astype(F32)
    i0 = np.minimum(src.astype(np.int32), inn - 1)
    i1 = i0 + (i0 < inn - 1)
    return i0, i1, (src - i0.astype(F32)).astype(F32)


def upsample(k, scale, align):
    """u [B, L, H, W] of the logits k [B, 1, D, h, w], fp32, in the kernels' order."""
    B, _, D, h, w = k.shape
    q = k[:, 0].astype(F32)
    y0, y1, ly = taps(scale * h, h, align)
    x0, x1, lx = taps(scale * w, w, align)
    d0, d1, ld = taps(scale * D, D, align)
    ly, lx, ld = ly[None, None, :, None], lx[None, None, None, :], ld[None, :, None, None]
    hy, hx = F32(1) - ly, F32(1) - lx
    g = lambda ys, xs: q[:, :, ys][:, :, :, xs]                                                        # noqa: E731
    bl = hy * (hx * g(y0, x0) + lx * g(y0, x1)) + ly * (hx * g(y1, x0) + lx * g(y1, x1))
    return ((F32(1) - ld) * bl[:, d0] + ld * bl[:, d1]).astype(F32)


def label(target, mask, ab, disp):
    """(t [B, H, W] fp32, counted [B, H, W] bool)"""
    with np.errstate(all='ignore'):
        t = target.astype(F32)
        if ab is not None:
            b, a = ab[:, 0].astype(F32)[:, None, None], ab[:, 1].astype(F32)[:, None, None]
            t = (a / t + b).astype(F32)
        ok = np.isfinite(t) & (t >= F32(disp[0])) & (t <= F32(disp[-1]))
        if mask is not None:
            ok &= mask > 0
    return t, ok


def _seq(parts):
    """s = s + part over the leading axis, in order, in fp32."""
    s = np.zeros(parts.shape[1:], dtype=F32)
    for p in parts:
        s = (s + p).astype(F32)
    return s


def forward(logits, disp, target, mask=None, ab=None, head_weights=(1.0,), scale=4, align=True, s=None):
    """The fp32 restatement -> dict(loss, counted [B, n, H, W] uint8, expect, lse, term [B, n, H, W] fp32 (term 0 where not counted),
    count per head)."""
    d = np.asarray(disp, dtype=F32)
    s = F32(d[1] - d[0]) if s is None else F32(s)
    t, ok = label(target, mask, ab, d)
    counted, expect, lses, terms, loss, counts = [], [], [], [], 0.0, []
    with np.errstate(all='ignore'):
        a = np.abs(d[:, None, None, None] - t[None]).astype(F32)                                       # [L, B, H, W]
        e = np.exp(-((a - a.min(0)) / s)).astype(F32)
        Z = _seq(e)
        P = (e / Z).astype(F32)
        for k, wh in zip(logits, head_weights):
            u = np.moveaxis(upsample(k, scale, align), 1, 0)                                           # [L, B, H, W]
            mx = u.max(0)
            ex = np.exp(u - mx).astype(F32)
            S = _seq(ex)
            lg = np.log(S).astype(F32)
            term = (lg - _seq(P * (u - mx))).astype(F32)
            term = np.where(ok, term, F32(0))
            cnt = int(ok.sum())
            if cnt:
                loss += float(F32(wh)) * (float(term.astype(np.float64).sum()) / cnt)
            counted.append(ok.astype(np.uint8)), lses.append((mx + lg).astype(F32)), terms.append(term), counts.append(cnt)
            expect.append(_seq((ex / S).astype(F32) * d[:, None, None, None]))
    stack = lambda xs: np.stack(xs, 1)                                                                 # noqa: E731
    return dict(loss=float(F32(loss)), counted=stack(counted), expect=stack(expect), lse=stack(lses), term=stack(terms), count=counts, t=t)


def torch_loss(logits, counted, disp, target, ab=None, head_weights=(1.0,), scale=4, align=True, s=None, dtype=torch.float64):
    """The loss as a torch scalar of `dtype` over the torch tensors `logits` (a list, [B, 1, D, h, w] of that dtype); counted [B, H, W]
    bool comes from the fp32 restatement."""
    d = torch.tensor(np.asarray(disp, dtype=F32).astype(np.float64)).to(dtype)
    s = float(F32(F32(disp[1]) - F32(disp[0]))) if s is None else float(F32(s))
    t = torch.tensor(np.asarray(target, dtype=F32)).to(dtype)
    if ab is not None:
        ab_t = torch.tensor(np.asarray(ab, dtype=F32)).to(dtype)
        t = ab_t[:, 1, None, None] / t + ab_t[:, 0, None, None]
    on = torch.tensor(counted)
    t = torch.where(on, t, torch.zeros_like(t))
    P = F.softmax(-(d[None, :, None, None] - t[:, None]).abs() / s, dim=1)
    total = 0
    for k, wh in zip(logits, head_weights):
        B, _, D, h, w = k.shape
        u = F.interpolate(k, size=(scale * D, scale * h, scale * w), mode='trilinear', align_corners=align)[:, 0]
        term = -(P * F.log_softmax(u, dim=1)).sum(1)
        if int(on.sum()):
            total = total + float(F32(wh)) * (term[on].sum() / int(on.sum()))
    return total


def loss_and_grad(c, counted, dtype):
    """-> (loss as a float, [d k_i] as fp64 numpy arrays) of the torch restatement at dtype."""
    ks = [torch.tensor(k.astype(np.float64)).to(dtype).requires_grad_(True) for k in c['logits']]
    loss = torch_loss(ks, counted, c['disp'], c['target'], c['ab'], c['head_weights'], c['scale'], c['align'], c['s'], dtype)
    if not torch.is_tensor(loss):
        return 0.0, [np.zeros(k.shape) for k in c['logits']]
    loss.backward()
    return float(loss.detach().double()), [k.grad.double().numpy() for k in ks]


def run(c, **over):
    c = dict(c, **over)
    return forward(c['logits'], c['disp'], c['target'], c['mask'], c['ab'], c['head_weights'], c['scale'], c['align'], c['s'])


def shipped_disp(L=32, mindisp=-4.0, maxdisp=12.0):
    """core.set_levels: the hypothesis values of the shipped geometry, 0.5 px apart."""
    return [i * ((maxdisp - mindisp) / float(L)) + mindisp for i in range(L)]


def ellipse(B, H, W, semi=0.45):
    ys, xs = np.mgrid[0:H, 0:W]
    return np.broadcast_to((((ys - (H - 1) / 2) / (semi * H)) ** 2 + ((xs - (W - 1) / 2) / (semi * W)) ** 2 <= 1.0), (B, H, W)).astype(F32)


def make_case(B, n, D, h, w, seed, scale=4, align=True, uneven=False, s=None, weights=None, mask='random', fitted=False, amp=2.0):
    """Logits of amplitude `amp`, a target uniform in [d_0 - R / 8, d_{L-1} + R / 8) (R the hypothesis range; about 80 % lies inside) and a
    mask that keeps about 80 % (random) or the inscribed ellipse (64 %), then one pixel each of NaN, +Inf, -Inf, far below d_0 and far
    above d_{L-1} inside the mask.  fitted: the target is handed over as the depth map a / (t - b) with target_ab = [b, a] per sample,
    and three more pixels get a depth of 0, a negative depth and NaN."""
    rng = np.random.RandomState(seed)
    L, H, W = scale * D, scale * h, scale * w
    disp = shipped_disp(L) if not uneven else list(np.cumsum(rng.uniform(0.25, 1.0, L)) - 3.0)
    disp = [float(F32(v)) for v in disp]
    logits = [(amp * rng.standard_normal((B, 1, D, h, w))).astype(F32) for _ in range(n)]
    R = disp[-1] - disp[0]
    t = rng.uniform(disp[0] - R / 8, disp[-1] + R / 8, (B, H, W)).astype(F32)
    m = None
    if mask == 'random':
        m = (rng.uniform(size=(B, H, W)) < 0.8).astype(F32)
    elif mask == 'ellipse':
        m = ellipse(B, H, W)
    inside = np.argwhere(np.ones((B, H, W), bool) if m is None else m > 0)
    picks = inside[rng.permutation(len(inside))[:8]]
    kinds = {}
    for (b, y, x), (kind, v) in zip(picks, (('nan', np.nan), ('inf', np.inf), ('inf', -np.inf), ('below', disp[0] - 50.0),
                                            ('above', disp[-1] + 50.0))):
        t[b, y, x] = v
        kinds[kind] = (b, y, x)
    ab = None
    if fitted:
        ab = np.stack([rng.uniform(-14.0, -13.0, B), rng.uniform(40.0, 60.0, B)], 1).astype(F32)       # [b, a]: t = a / depth + b
        with np.errstate(all='ignore'):
            t = (ab[:, 1, None, None] / (t - ab[:, 0, None, None])).astype(F32)                          # the depth map
        for (b, y, x), v in zip(picks[5:], (0.0, -1.0, np.nan)):
            t[b, y, x] = v
    weights = tuple(weights) if weights is not None else tuple([1.0, 0.7, 0.5][:n]) if n > 1 else (1.0,)
    return dict(logits=logits, disp=disp, target=t, mask=m, ab=ab, head_weights=weights, scale=scale, align=align, s=s, kinds=kinds)


# the cases of tests/test_gpu_unimodal.py (the table of its docstring), the first one also the finite-difference case of the host tests
CASES = {
    'one-tile': dict(B=1, n=1, D=8, h=2, w=3, seed=11),
    'multi-tile': dict(B=2, n=3, D=8, h=5, w=18, seed=12, mask='ellipse', weights=(1.0, 0.7, 0.5)),
    'general': dict(B=1, n=2, D=4, h=3, w=9, seed=13, uneven=True, s=0.8),
    'half-pixel': dict(B=1, n=2, D=8, h=3, w=10, seed=14, align=False),
    'thin': dict(B=1, n=1, D=8, h=1, w=9, seed=15),
    'fitted': dict(B=2, n=1, D=8, h=4, w=9, seed=16, fitted=True),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """{'case', 'r32' (the fp32 restatement), 'loss64', 'grad64', 'loss32', 'grad32' (the torch restatements)}: computed once per name and
    shared; nobody writes into it."""
    c = make_case(**CASES[name])
    r32 = run(c)
    on = r32['counted'][:, 0] > 0
    loss64, grad64 = loss_and_grad(c, on, torch.float64)
    loss32, grad32 = loss_and_grad(c, on, torch.float32)
    return dict(case=c, r32=r32, loss64=loss64, grad64=grad64, loss32=loss32, grad32=grad32)
