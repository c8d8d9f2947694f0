"""Occlusion handling of the multi-view loss (csrc/multiview.hip: visibility 'zbuffer', reduce 'min') restated (test infrastructure;
DESIGN.md section 7), on top of tests/multiview_cpu.py, which is imported unchanged:

  * ``forward`` in numpy fp32, operation by operation in the kernels' order, with every discrete decision spelled out: the z-buffer
    (per sample, head and view the smallest q_z splatted into each cell), visible (q_z <= zmin + tolerance * zmin of the pixel's own
    cell), seen = warpable and visible, counted (the window lies in the image and its nine pixels are seen), selected (the view of the
    smallest term among the views that count the pixel, the lowest view at a tie; 255 none).  These compare exactly with the kernels.
  * ``torch_loss`` in torch fp32 / fp64 with those decisions frozen (and, where asked, with a selection plane handed in: the kernel's
    own), the derivative left to torch.autograd.

    q_z   z * ((M6 x + M7 y) + M8) + t_z, as tests/multiview_cpu.py::warp forms it
    cell  (int(floor(v + 0.5)) // cell, int(floor(u + 0.5)) // cell), clamped to the Hc x Wc grid, Hc = ceil(Hs / cell)
    loss  reduce 'mean': multiview_cpu's, over the counted maps above;  reduce 'min': sum_h w_h (sum of the selected terms / count_h),
          count_h the pixels some view counts

Also the cases the tests draw and the occluder scene (dualpixelface_amd/synthetic_multiview.py) as a case.
"""
import numpy as np
import torch

from dualpixelface_amd import synthetic_multiview as scene
from tests import multiview_cpu as mc
from tests import photometric_cpu as pc

NONE = 255
MODES = {'min': dict(reduce='min', visibility='none'), 'zbuffer': dict(reduce='mean', visibility='zbuffer'),
         'min-zbuffer': dict(reduce='min', visibility='zbuffer')}


def q_z(z, rg):
    """z [B, H, W] fp32, rg [B, 12] fp32 -> q_z [B, H, W] fp32, the expression of multiview_cpu.warp."""
    B, H, W = z.shape
    r = [rg[:, k].astype(np.float32)[:, None, None] for k in (6, 7, 8, 11)]
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    xf, yf = xs.astype(np.float32)[None], ys.astype(np.float32)[None]
    with np.errstate(all='ignore'):
        return z * ((r[0] * xf + r[1] * yf) + r[2]) + r[3]


def zbuffer(ok, qz, u, v, Hs, Ws, cell):
    """One head and one view: warpable [B, H, W], q_z, the sample points -> (zbuf [B, Hc, Wc] fp32, +inf where nothing landed; the
    cell indices (cy, cx) of every pixel)."""
    B = ok.shape[0]
    Hc, Wc = -(-Hs // cell), -(-Ws // cell)
    half = np.float32(0.5)
    cx = np.clip(np.floor(u + half).astype(np.int64) // cell, 0, Wc - 1)
    cy = np.clip(np.floor(v + half).astype(np.int64) // cell, 0, Hc - 1)
    zb = np.full((B, Hc, Wc), np.inf, np.float32)
    bi = np.broadcast_to(np.arange(B)[:, None, None], ok.shape)
    np.minimum.at(zb, (bi[ok], cy[ok], cx[ok]), qz[ok])
    return zb, (cy, cx)


def forward(c, reduce='mean', visibility='none', cell=2, tolerance=0.01, **over):
    """A case dict of tests/multiview_cpu.py -> what multiview_cpu.forward returns at fp32 (warpable stays the geometric flag; counted,
    count, sums, views follow 'seen'), and: seen [n][S], visible [B, n, S, H, W] uint8 (= seen), zbuffer [B, n, S, Hc, Wc] (None with
    visibility 'none'), terms [B, n, S, H, W] fp32 (0 where not counted), selected [B, n, H, W] uint8 and count_min [n] (reduce 'min')."""
    c = dict(c, **over)
    dt = np.float32
    pred, src = c['pred'], c['src_rgb']
    B, n, H, W = pred.shape
    S, Hs, Ws = src.shape[1], src.shape[3], src.shape[4]
    rg = mc.rig(c['K'], c['P'], c['Ks'], c['Ps'])
    I = pc.luma(c['tgt_rgb'], dt)
    Ys = pc.luma(src.reshape(B * S, 3, Hs, Ws), dt).reshape(B, S, Hs, Ws)
    wsd, one, tol = dt(np.float32(c['weight_ssim'])), dt(1), np.float32(tolerance)
    out = dict(usable=[], warpable=[], taps=[], count=[], sums=[], views=[], seen=[], count_min=[])
    warped = np.zeros((B, n, S, H, W), dt)
    terms = np.zeros((B, n, S, H, W), dt)
    counted = np.zeros((B, n, S, H, W), np.uint8)
    visible = np.zeros((B, n, S, H, W), np.uint8)
    xy = np.zeros((B, n, S, 2, H, W), dt)
    selected = np.full((B, n, H, W), NONE, np.uint8)
    zbuf = np.zeros((B, n, S, -(-Hs // cell), -(-Ws // cell)), dt) if visibility == 'zbuffer' else None
    loss = 0.0
    for h in range(n):
        usable, z = mc.depth_of(pred[:, h], c['ab'], c['mask'], c['target_type'], c['min_depth'], dt)
        rows = dict(warpable=[], taps=[], count=[], sums=[], seen=[])
        hsum, views = 0.0, 0
        best = np.zeros((B, H, W), dt)
        for v in range(S):
            ok, J, (u, vv), taps, _ = mc.warp(z, usable, rg[:, v], Ys[:, v], dt)
            seen = ok
            if visibility == 'zbuffer':
                qz = q_z(z, rg[:, v])
                zb, (cy, cx) = zbuffer(ok, qz, u, vv, Hs, Ws, cell)
                zmin = zb[np.arange(B)[:, None, None], cy, cx]
                with np.errstate(all='ignore'):
                    slack = tol * zmin
                    seen = ok & (qz <= zmin + slack)
                zbuf[:, h, v] = zb
            cnt_map = np.zeros((B, H, W), bool)
            term = np.zeros((B, H, W), dt)
            if H >= 3 and W >= 3:
                inner = np.ones((B, H - 2, W - 2), bool)
                for m in pc._box(seen, H, W):
                    inner &= m
                ds, _ = mc.ssim_term(I, J, dt)
                d = J[:, 1:-1, 1:-1] - I[:, 1:-1, 1:-1]
                with np.errstate(all='ignore'):
                    t = wsd * ds + (one - wsd) * mc.rho(d, c['alpha'], c['scale'], dt).astype(dt)
                cnt_map[:, 1:-1, 1:-1] = inner
                term[:, 1:-1, 1:-1] = np.where(inner, t, dt(0))
            cnt, tot = float(cnt_map.sum()), float(term.astype(np.float64).sum())
            if cnt > 0:
                hsum += tot / cnt
                views += 1
            take = cnt_map & ((selected[:, h] == NONE) | (term < best))          # strictly smaller: the lowest view wins a tie
            best = np.where(take, term, best)
            selected[:, h][take] = v
            warped[:, h, v], counted[:, h, v], xy[:, h, v, 0], xy[:, h, v, 1] = J, cnt_map, u, vv
            terms[:, h, v], visible[:, h, v] = term, seen
            for key, val in zip(('warpable', 'taps', 'count', 'sums', 'seen'), (ok, taps, cnt, tot, seen)):
                rows[key].append(val)
        cmin = float((selected[:, h] != NONE).sum())
        w = float(np.float32(c['head_weights'][h]))
        if reduce == 'min':
            if cmin > 0:
                loss += w * (float(best.astype(np.float64).sum()) / cmin)
        elif views > 0:
            loss += w * (hsum / views)
        out['usable'].append(usable), out['views'].append(views), out['count_min'].append(cmin)
        for key in rows:
            out[key].append(rows[key])
    out.update(loss=float(np.float32(loss)), rig=rg, Y_tgt=I, Y_src=Ys, warped=warped, counted=counted, xy=xy, visible=visible, zbuffer=zbuf,
               terms=terms, selected=selected, reduce=reduce)
    return out


def view_terms(pred, ref, c, dtype):
    """The term maps as torch expressions in `dtype` over pred [B, n, H, W], with the decisions of ``ref`` = forward(c, ...) (usable,
    warpable, the taps): a list [n][S] of [B, H - 2, W - 2] tensors, meaningful where ref['counted'] is set."""
    B, n, H, W = pred.shape
    dt = np.float32 if dtype == torch.float32 else np.float64
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a))                                          # noqa: E731
    src = c['src_rgb']
    S, Hs, Ws = src.shape[1], src.shape[3], src.shape[4]
    I = T(pc.luma(c['tgt_rgb'], dt))
    Ys = T(pc.luma(src.reshape(B * S, 3, Hs, Ws), dt).reshape(B, S, Hs, Ws))
    rg = T(ref['rig'].astype(dt))
    wsd = float(dt(np.float32(c['weight_ssim'])))
    c1, c2 = float(dt(np.float32(pc.C1))), float(dt(np.float32(pc.C2)))
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing='ij')
    bi = torch.arange(B)[:, None, None]
    zero, unit = torch.zeros((), dtype=dtype), torch.ones((), dtype=dtype)
    out = []
    for h in range(n):
        usable = T(ref['usable'][h])
        p = pred[:, h]
        if c['target_type'] == 'depth':
            z = torch.where(usable, p, unit)
        elif c['target_type'] == 'idepth':
            z = 1 / torch.where(usable, p, unit)
        else:
            b, a = T(c['ab'][:, 0].astype(dt))[:, None, None], T(c['ab'][:, 1].astype(dt))[:, None, None]
            z = a / torch.where(usable, p - b, unit)
        row = []
        for v in range(S):
            ok = T(ref['warpable'][h][v])
            y0, y1, x0, x1 = [T(t) for t in ref['taps'][h][v]]
            r = [rg[:, v, k][:, None, None] for k in range(12)]
            mx, my, mz = (r[0] * xs + r[1] * ys) + r[2], (r[3] * xs + r[4] * ys) + r[5], (r[6] * xs + r[7] * ys) + r[8]
            qx, qy, qz = z * mx + r[9], z * my + r[10], z * mz + r[11]
            qz = torch.where(ok, qz, unit)
            u, vv = qx / qz, qy / qz
            fx, fy = u - x0.to(dtype), vv - y0.to(dtype)
            Y = Ys[:, v]
            v00, v01, v10, v11 = Y[bi, y0, x0], Y[bi, y0, x1], Y[bi, y1, x0], Y[bi, y1, x1]
            top, bot = v00 + fx * (v01 - v00), v10 + fx * (v11 - v10)
            J = torch.where(ok, top + fy * (bot - top), zero)
            cc = I[:, 1:-1, 1:-1]
            sI = sJ = sII = sJJ = sIJ = torch.zeros((B, H - 2, W - 2), dtype=dtype)
            for i, j in zip(pc._box(I, H, W), pc._box(J, H, W)):
                i, j = i - cc, j - cc
                sI, sJ, sII, sJJ, sIJ = sI + i, sJ + j, sII + i * i, sJJ + j * j, sIJ + i * j
            mI, mJ = sI / 9, sJ / 9
            muI, muJ = cc + mI, cc + mJ
            vI, vJ, cov = sII / 9 - mI * mI, sJJ / 9 - mJ * mJ, sIJ / 9 - mI * mJ
            ssim = (((2 * muI) * muJ + c1) * (2 * cov + c2)) / (((muI * muI + muJ * muJ) + c1) * ((vI + vJ) + c2))
            d = J[:, 1:-1, 1:-1] - I[:, 1:-1, 1:-1]
            row.append(wsd * torch.clamp((1 - ssim) / 2, 0, 1) + (1 - wsd) * mc.rho(d, c['alpha'], c['scale'], dt, xp=torch))
        out.append(row)
    return out


def torch_loss(pred, ref, c, dtype=torch.float64, selected=None):
    """The loss in `dtype` with the decisions of ``ref`` frozen; reduce is ref['reduce'].  selected: a selection plane [B, n, H, W] uint8
    to use in place of ref['selected'] (the kernel's own; which pixels are selected at all must agree)."""
    B, n, H, W = pred.shape
    if H < 3 or W < 3:
        return torch.zeros((), dtype=torch.float64)
    S = c['src_rgb'].shape[1]
    terms = view_terms(pred, ref, c, dtype)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a))                                          # noqa: E731
    zero = torch.zeros((), dtype=dtype)
    sel = ref['selected'] if selected is None else selected
    loss = torch.zeros((), dtype=torch.float64)
    for h in range(n):
        w = float(np.float32(c['head_weights'][h]))
        if ref['reduce'] == 'min':
            if ref['count_min'][h] > 0:
                tot = torch.zeros((), dtype=torch.float64)
                for v in range(S):
                    tot = tot + torch.where(T(sel[:, h, 1:-1, 1:-1] == v), terms[h][v], zero).double().sum()
                loss = loss + w * (tot / ref['count_min'][h])
            continue
        hsum = torch.zeros((), dtype=torch.float64)
        for v in range(S):
            if ref['count'][h][v] > 0:
                tot = torch.where(T(ref['counted'][:, h, v, 1:-1, 1:-1].astype(bool)), terms[h][v], zero).double().sum()
                hsum = hsum + tot / ref['count'][h][v]
        if ref['views'][h] > 0:
            loss = loss + w * (hsum / ref['views'][h])
    return loss


def loss_and_grad(c, ref, dtype, selected=None):
    return pc._grad(lambda p: torch_loss(p, ref, c, dtype, selected), c['pred'], dtype)


def near_ties(c, ref):
    """Pixels whose two smallest fp64 terms, among the views that count them, differ by less than 4 fp32 ulps of the larger:
    [B, n, H, W] bool.  There the kernel's fp32 comparison may pick the other view."""
    B, n, H, W = c['pred'].shape
    S = c['src_rgb'].shape[1]
    out = np.zeros((B, n, H, W), bool)
    if S < 2 or H < 3 or W < 3:
        return out
    clean = np.where(np.isfinite(c['pred']), c['pred'], 0.0).astype(np.float64)
    with torch.no_grad():
        terms = view_terms(torch.tensor(clean), ref, c, torch.float64)
    for h in range(n):
        t = np.stack([terms[h][v].numpy() for v in range(S)], 1)                                   # [B, S, H - 2, W - 2]
        t = np.where(ref['counted'][:, h, :, 1:-1, 1:-1] > 0, t, np.inf)
        two = np.sort(t, axis=1)[:, :2]
        both = np.isfinite(two[:, 1])
        with np.errstate(invalid='ignore'):
            gap = np.where(both, two[:, 1] - two[:, 0], np.inf)
        ulp = np.spacing(np.where(both, two[:, 1], 1.0).astype(np.float32)).astype(np.float64)
        out[:, h, 1:-1, 1:-1] = gap < 4 * ulp
    return out


# ---- cases: the shapes at which the kernels can go wrong, each with its cell size and z-buffer tolerance.  The depth fields of
# multiview_cpu.make_case slope by 0.2 to 3 % per pixel, far more than a face does, so the tolerances are set case by case to leave a mix:
# between a third and two thirds of the pixels the plain loss counts stay counted (tests/test_multiview_occlusion_host.py checks it)
CASES = {
    'tiny-7x9': (dict(B=1, n=1, S=1, H=7, W=9, Hs=11, Ws=13, seed=21, target_type='depth'), dict(cell=1, tolerance=0.01)),
    'multi-tile-19x70': (dict(B=2, n=3, S=2, H=19, W=70, Hs=40, Ws=90, seed=22, target_type='disp', masked=True, bad=True),
                         dict(cell=2, tolerance=0.03)),
    # multi-tile in both axes; Hs and Ws are no multiples of the cell
    'rows-65x500': (dict(B=2, n=2, S=2, H=65, W=500, Hs=81, Ws=563, seed=26, target_type='depth', masked=True, bad=True),
                    dict(cell=4, tolerance=0.02)),
    'one-behind-33x40': (dict(B=1, n=2, S=3, H=33, W=40, Hs=30, Ws=37, seed=24, target_type='idepth', alpha=-2.0, behind=(2,)),
                         dict(cell=2, tolerance=0.015)),
}

_cache = {}


def case(name, mode):
    """A case under MODES[mode] with the fp32 restatement, the torch losses and gradients in fp32 and fp64 and the near-tie map,
    computed once: dict(case, kw, r32, loss32, grad32, loss64, grad64, ties).  Nothing in it may be changed by a test."""
    key = (name, mode)
    if key not in _cache:
        args, occ = CASES[name]
        c = mc.make_case(**args)
        kw = dict(MODES[mode], **occ)
        r32 = forward(c, **kw)
        out = dict(case=c, kw=kw, r32=r32, ties=near_ties(c, r32))
        out['loss32'], out['grad32'] = loss_and_grad(c, r32, torch.float32)
        out['loss64'], out['grad64'] = loss_and_grad(c, r32, torch.float64)
        _cache[key] = out
    return _cache[key]


# ---- the occluder scene
def occluder_case(H=48, W=64, views=2, offset=0.0, n=1, target_type='depth'):
    """The occluder scene as a case dict, every head predicting the true depth times (1 + offset); 'closed' holds the closed-form
    maps: on_occluder [H, W], visible [S, H, W], edge [S, H, W]."""
    s = scene.occluder_sample(H, W, views)
    Hs, Ws = s['centers'].shape[1:]
    z = np.repeat(s['depth'].numpy().astype(np.float64)[None, None], n, 1) * (1.0 + offset)
    ab = s['abvalue'].numpy()[None] if target_type == 'disp' else None
    N = lambda k: s[k].numpy()[None]                                                               # noqa: E731
    return dict(pred=mc.pred_of(z, target_type, ab), tgt_rgb=N('center'), src_rgb=s['centers'].numpy().reshape(1, views, 3, Hs, Ws),
                K=N('K'), P=N('P'), Ks=N('Ks'), Ps=N('Ps'), ab=ab, mask=None, head_weights=(1.0, 0.5)[:n], target_type=target_type,
                weight_ssim=0.8, alpha=1.0, scale=0.1, min_depth=1e-3, z=z,
                closed=dict(on_occluder=s['on_occluder'], visible=s['visible'], edge=s['edge']))


def closed_form_loss(c, dtype=torch.float64):
    """The loss of the occluder case under CLOSED-FORM visibility, reduce 'mean': seen = warpable and closed-form visible -> (loss,
    the decisions).  The floor the kernels' z-buffer is measured against."""
    r = forward(c)
    vis = c['closed']['visible']
    B, n, H, W = c['pred'].shape
    S = vis.shape[0]
    for h in range(n):
        r['views'][h] = 0
        for v in range(S):
            seen = r['warpable'][h][v] & vis[v][None]
            inner = np.ones((B, H - 2, W - 2), bool)
            for m in pc._box(seen, H, W):
                inner &= m
            r['counted'][:, h, v] = 0
            r['counted'][:, h, v, 1:-1, 1:-1] = inner
            r['count'][h][v] = float(inner.sum())
            r['views'][h] += int(inner.any())
    clean = torch.tensor(c['pred'].astype(np.float32 if dtype == torch.float32 else np.float64))
    with torch.no_grad():
        return float(torch_loss(clean, r, c, dtype)), r
