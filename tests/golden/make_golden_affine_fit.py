#!/usr/bin/env python3
"""Golden vectors for the 'least_square' branch of the depth losses: runs the REFERENCE's regress_affine / depth2disp
(src/utils/geometry.py) and its SMOOTHL1Loss / SILOGLoss with dp_conversion='least_square' on the CPU (scipy) and stores inputs, the fitted
abvalue, loss values and pred.grad as float32.  Build container only:
    python tests/golden/make_golden_affine_fit.py

B, H, W = 2, 24, 40.  Two scenes: 'z' has depth uniform in [700, 1500] with about 15 % zeros (idepth 0 there: not valid for the fit, target
-100 for the loss) and a Bernoulli(0.6) mask that is independent of the zeros; 'p' has no zeros, so that every target is positive (silog).
pred = a * idepth + b + noise per head with (a, b) near (-26996, 63), at three noise levels: 'clean' (sigma 0.05), 'outlier10' (10 % of the
pixels moved by uniform [-15, 15]) and 'heavy' (sigma 0.3, 20 % moved).  'pred_inv' is the reciprocal of such a field (target_type 'depth').

Per scene and level: the reference's ab [B, 2] float32 and ref_dd [B], the distance in disparity units between that ab and the fp64
restatement of the fit run to convergence (tests/affine_fit_cpu.py) -- the reference's own distance from the minimiser, which sets the
fit bars of the tests.  Per case: ab, loss, grad.  B = 1 cases without a mask are the reference classes' own output; masked and B = 2
cases are the reference's expressions composed here with the [B, H, W] target (regress_affine -> depth2disp -> squeeze ->
F.smooth_l1_loss / the silog lines), because the classes cannot run there (IndexError) or average a [B, B, H, W] cross product.
"""
import os
import sys
import types
import warnings

import numpy as np
import torch
import torch.nn.functional as F

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
B, H, W = 2, 24, 40
LOSS_WEIGHT = [1.0, 0.7, 0.5]
VARIANCE_FOCUS = 0.85
LEVELS = {'clean': (0.05, 0.0), 'outlier10': (0.05, 0.10), 'heavy': (0.3, 0.20)}
AB = [(-26996.49, 63.0), (-25510.2, 61.4)]                   # (a, b) per sample


def option(n):
    return types.SimpleNamespace(model=types.SimpleNamespace(variance_focus=VARIANCE_FOCUS, loss_weight=LOSS_WEIGHT[:n]),
                                 dataset=types.SimpleNamespace(dp_conversion='least_square'))


def main():
    warnings.simplefilter('ignore')
    sys.path.insert(0, REF)
    from src.loss.depth.silog import SILOGLoss
    from src.loss.depth.smoothL1 import SMOOTHL1Loss
    from src.utils.geometry import regress_affine, depth2disp, inverse_depth
    from tests import affine_fit_cpu as af
    bank = {'silog': SILOGLoss, 'smoothL1': SMOOTHL1Loss}
    g = torch.Generator().manual_seed(43)
    u = lambda lo, hi, *shape: torch.rand(*shape, generator=g) * (hi - lo) + lo
    out, t = {}, {}

    def keep(key, v):
        t[key] = v.float()
        out[key] = t[key].numpy()

    for scene in ('z', 'p'):
        depth = u(700.0, 1500.0, B, H, W)
        if scene == 'z':
            depth = depth * (torch.rand(B, H, W, generator=g) >= 0.15).float()
        keep(scene + '::depth', depth)
        keep(scene + '::idepth', inverse_depth(depth.unsqueeze(1))[:, 0])
        keep(scene + '::mask', (torch.rand(B, H, W, generator=g) < 0.6).float())
        for level, (sigma, frac) in LEVELS.items():
            if scene == 'p' and level != 'outlier10':
                continue
            a = torch.tensor([v[0] for v in AB]).view(B, 1, 1, 1)
            b = torch.tensor([v[1] for v in AB]).view(B, 1, 1, 1)
            pred = a * t[scene + '::idepth'].unsqueeze(1) + b + sigma * torch.randn(B, 3, H, W, generator=g)
            moved = (torch.rand(B, 3, H, W, generator=g) < frac).float()
            pred = pred + moved * u(-15.0, 15.0, B, 3, H, W)
            keep('%s::%s::pred' % (scene, level), pred)
            ab = regress_affine(t['%s::%s::pred' % (scene, level)][:, 0:1], t[scene + '::idepth'].unsqueeze(1))
            keep('%s::%s::ab' % (scene, level), ab)
            conv, _ = af.converged(t['%s::%s::pred' % (scene, level)], t[scene + '::idepth'])
            ref_dd = [af.dd(out['%s::%s::ab' % (scene, level)][i], conv[i], out[scene + '::idepth'][i]) for i in range(B)]
            out['%s::%s::ref_dd' % (scene, level)] = np.asarray(ref_dd, dtype=np.float64)
            print('%s %-10s ab %s  ref_dd %s' % (scene, level, out['%s::%s::ab' % (scene, level)].tolist(), ref_dd))
    keep('z::outlier10::pred_inv', 1.0 / t['z::outlier10::pred'])

    # (kind, target_type, n, scene, level, masked, b1)
    cases = [('smoothL1', tt, n, 'z', 'outlier10', False, True) for tt in ('disp', 'idepth', 'depth') for n in (1, 3)]
    cases += [('silog', 'disp', n, 'p', 'outlier10', False, True) for n in (1, 3)]
    cases += [('smoothL1', 'disp', 3, 'z', level, True, False) for level in LEVELS]
    cases += [('smoothL1', 'idepth', 1, 'z', 'outlier10', True, False), ('smoothL1', 'depth', 3, 'z', 'outlier10', True, False),
              ('smoothL1', 'disp', 3, 'z', 'heavy', False, False), ('silog', 'disp', 3, 'p', 'outlier10', True, False),
              ('silog', 'idepth', 1, 'p', 'outlier10', False, False)]
    names = []
    for kind, tt, n, scene, level, masked, b1 in cases:
        name = '%s_%s_n%d_%s_%s%s%s' % (kind, tt, n, scene, level, '_mask' if masked else '', '_b1' if b1 else '')
        sl = slice(0, 1) if b1 else slice(None)
        field = 'pred_inv' if tt == 'depth' else 'pred'
        pred = t['%s::%s::%s' % (scene, level, field)][sl, :n].clone().requires_grad_()
        batch = {'idepth': t[scene + '::idepth'][sl], 'depth': t[scene + '::depth'][sl]}
        if masked:
            batch['mask'] = t[scene + '::mask'][sl]
        if b1 and not masked:
            res = bank[kind](option(n)).forward({'pred_depth': pred}, batch, tt)           # the reference class itself
            loss, ab = res['loss'], res['abvalue']
        else:
            weights = [1.0] if n == 1 else LOSS_WEIGHT[:n]
            ab = regress_affine(pred[:, 0:1], batch['idepth'].unsqueeze(1))
            gt = depth2disp(batch['depth'].unsqueeze(1), ab).squeeze(1)                     # the squeeze the classes lack
            pred_ = inverse_depth(pred) if (tt == 'depth' and kind == 'smoothL1') else pred
            sel = batch['mask'] > 0 if masked else torch.ones_like(gt, dtype=torch.bool)
            if kind == 'smoothL1':
                loss = sum(weights[i] * F.smooth_l1_loss(pred_[:, i][sel], gt[sel]) for i in range(n))
            else:
                dist = [weights[i] * (torch.log(pred_[:, i][sel]) - torch.log(gt[sel])) for i in range(n)]
                loss = sum(torch.sqrt((d ** 2).mean() - VARIANCE_FOCUS * (d.mean() ** 2)) * 10.0 for d in dist)
        loss.backward()
        assert ab.dtype == torch.float32 and tuple(ab.shape) == (pred.shape[0], 2)
        assert torch.isfinite(loss) and bool(torch.isfinite(pred.grad).all()), name
        out[name + '::ab'] = ab.detach().numpy().astype(np.float32)
        out[name + '::loss'] = loss.detach().numpy().astype(np.float32)
        out[name + '::grad'] = pred.grad.numpy().astype(np.float32)
        conv, _ = af.converged(pred, batch['idepth'])
        out[name + '::ref_dd'] = np.asarray(af.dd(out[name + '::ab'], conv, batch['idepth'].numpy()), dtype=np.float64)
        names.append('%s %s %s %d %s %s %d %d' % (name, kind, tt, n, scene, level, int(masked), int(b1)))
        print('%-44s loss %.7g  max |grad| %.3e  ref_dd %.3e' % (name, float(loss), float(pred.grad.abs().max()), float(out[name + '::ref_dd'])))
    out['cases'] = np.asarray(names)
    out['loss_weight'] = np.asarray(LOSS_WEIGHT, dtype=np.float32)
    out['variance_focus'] = np.asarray(VARIANCE_FOCUS, dtype=np.float32)
    path = os.path.join(HERE, 'affine_fit.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
