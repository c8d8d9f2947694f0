#!/usr/bin/env python3
"""Golden vectors for the depth-target loss bank: runs the REFERENCE's own SILOGLoss / SMOOTHL1Loss (src/loss/depth/{silog,smoothL1}.py,
which pull in src.utils.geometry only) on the CPU and stores inputs, loss values and pred.grad as float32.  Build container only:
    python tests/golden/make_golden_loss_bank.py

Cases, B = 2, H = 24, W = 40:  {silog, smoothL1} x {disp, idepth, depth} x n in {1, 3} with a Bernoulli(0.6) mask, one mask-less silog case
with conf, one masked smoothL1 'idepth' case with conf.  Predictions and the disp / idepth targets are uniform in [0.5, 2.5]; depth, and the
prediction of the silog 'depth' case, uniform in [700, 1500]; conf uniform in [0.1, 1].  The batch arrays and the two prediction fields are
stored once and shared by the cases (a case with n heads uses the first n channels); every case stores its own loss and gradient.
"""
import os
import sys
import types
import warnings

import numpy as np
import torch

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
B, H, W = 2, 24, 40
LOSS_WEIGHT = [1.0, 0.7, 0.5]
VARIANCE_FOCUS = 0.85


def option(n):
    return types.SimpleNamespace(model=types.SimpleNamespace(variance_focus=VARIANCE_FOCUS, loss_weight=LOSS_WEIGHT[:n]),
                                 dataset=types.SimpleNamespace(dp_conversion='given'))


def case_name(kind, target_type, n, tag=''):
    return '%s_%s_n%d%s' % (kind, target_type, n, tag)


def main():
    warnings.simplefilter('ignore')
    sys.path.insert(0, REF)
    from src.loss.depth.silog import SILOGLoss
    from src.loss.depth.smoothL1 import SMOOTHL1Loss
    bank = {'silog': SILOGLoss, 'smoothL1': SMOOTHL1Loss}
    g = torch.Generator().manual_seed(41)
    u = lambda lo, hi, *shape: torch.rand(*shape, generator=g) * (hi - lo) + lo
    shared = {'disp': u(0.5, 2.5, B, H, W), 'idepth': u(0.5, 2.5, B, H, W), 'depth': u(700.0, 1500.0, B, H, W),
              'mask': (torch.rand(B, H, W, generator=g) < 0.6).float(), 'conf': u(0.1, 1.0, B, H, W),
              'pred_unit': u(0.5, 2.5, B, 3, H, W), 'pred_far': u(700.0, 1500.0, B, 3, H, W), 'abvalue': torch.tensor([[32.98, -26996.49]] * B)}
    assert all(float(v.abs().min()) > 0 for k, v in shared.items() if k != 'mask')
    out = {k: v.numpy().astype(np.float32) for k, v in shared.items()}
    out['loss_weight'] = np.asarray(LOSS_WEIGHT, dtype=np.float32)
    out['variance_focus'] = np.asarray(VARIANCE_FOCUS, dtype=np.float32)
    cases = [(kind, tt, n, True, False, '') for kind in ('silog', 'smoothL1') for tt in ('disp', 'idepth', 'depth') for n in (1, 3)]
    cases += [('silog', 'idepth', 3, False, True, '_conf_nomask'), ('smoothL1', 'idepth', 3, True, True, '_conf')]
    names = []
    for kind, tt, n, masked, with_conf, tag in cases:
        far = kind == 'silog' and tt == 'depth'
        pred = shared['pred_far' if far else 'pred_unit'][:, :n].clone().requires_grad_()
        batch = {k: shared[k] for k in ('disp', 'idepth', 'depth', 'abvalue')}
        if masked:
            batch['mask'] = shared['mask']
        if with_conf:
            batch['conf'] = shared['conf']
        res = bank[kind](option(n)).forward({'pred_depth': pred}, batch, tt)
        res['loss'].backward()
        name = case_name(kind, tt, n, tag)
        assert torch.isfinite(res['loss']) and bool(torch.isfinite(pred.grad).all()), name
        out[name + '::loss'] = res['loss'].detach().numpy().astype(np.float32)
        out[name + '::grad'] = pred.grad.numpy().astype(np.float32)
        names.append('%s %s %s %d %d %d' % (name, kind, tt, n, int(masked), int(with_conf)))
        print('%-32s loss %.7g  max |grad| %.3e' % (name, float(res['loss']), float(pred.grad.abs().max())))
    out['cases'] = np.asarray(names)
    path = os.path.join(HERE, 'loss_bank.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
