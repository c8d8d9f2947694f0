"""fp64 numpy restatement of the robust affine fit (dualpixelface_amd/csrc/affine_fit.hip) and of the loss bank's 'least_square' branch on
top of tests/loss_bank_cpu.py: the yardstick of test_affine_fit_host.py and test_gpu_affine_fit.py.

Per sample: x = idepth, y = pred[:, 0], valid iff x > 0; minimise sum f^2 * 2 (sqrt(1 + (r / f)^2) - 1), r = A x + B - y (scipy's soft_l1 with
f_scale = f, src/utils/geometry.py:102-103) by iteratively reweighted least squares from the ordinary least-squares line."""
import numpy as np
import torch

from tests import loss_bank_cpu as lb

F_SCALE, MAX_ITERS, TOL = 0.1, 48, 1e-7         # the defaults of ops.affine_fit (DESIGN section 7 has the probe behind them)
DET_MIN = 1e-30                                  # metrics._weighted_affine_fit's rule


def _solve(w, x, y):
    sw, sx, sy = w.sum(), (w * x).sum(), (w * y).sum()
    sxx, sxy = ((w * x) * x).sum(), ((w * x) * y).sum()
    det = sw * sxx - sx * sx
    if not abs(det) >= DET_MIN:                  # (a NaN determinant is degenerate too)
        return 0.0, (float(sy / sw) if sw > 0 else 0.0)
    return float((sw * sxy - sx * sy) / det), float((sxx * sy - sx * sxy) / det)


def _weights(A, B, x, y, f):
    s = np.sqrt(1.0 + (((A * x + B) - y) / f) ** 2)
    return 1.0 / s, float((f * f) * (2.0 * (s - 1.0)).sum())


def fit_sample(x, y, f_scale=F_SCALE, max_iters=MAX_ITERS, tol=TOL):
    """x, y: flat arrays -> dict A, B, iters, count, objective (at the result), objective0 (at the least-squares start) and `trace`, the
    objective at every iterate from the start to the result."""
    x, y = np.asarray(x, dtype=np.float64).ravel(), np.asarray(y, dtype=np.float64).ravel()
    keep = x > 0                                 # False for NaN
    x, y = x[keep], y[keep]
    xmax = float(x.max()) if x.size else 0.0
    A, B = _solve(np.ones_like(x), x, y)
    iters, trace = 0, []
    if x.size:
        for p in range(1, max_iters + 1):
            w, obj = _weights(A, B, x, y, f_scale)
            trace.append(obj)
            A2, B2 = _solve(w, x, y)
            step = abs(A2 - A) * xmax + abs(B2 - B)
            A, B, iters = A2, B2, p
            if step < tol:
                break
    trace.append(_weights(A, B, x, y, f_scale)[1])
    return {'A': A, 'B': B, 'iters': iters, 'count': int(x.size), 'objective': trace[-1], 'objective0': trace[0], 'trace': trace}


def affine_fit(pred, idepth, f_scale=F_SCALE, max_iters=MAX_ITERS, tol=TOL):
    """pred [B, n, H, W], idepth [B, H, W] -> (ab float64 [B, 2] in the project's order [b, a] = [B_offset, A_slope], list of fit_sample dicts)."""
    p, x = pred.detach().cpu().double().numpy(), idepth.detach().cpu().double().numpy()
    info = [fit_sample(x[i], p[i, 0], f_scale, max_iters, tol) for i in range(p.shape[0])]
    return np.asarray([[r['B'], r['A']] for r in info], dtype=np.float64).reshape(-1, 2), info


def converged(pred, idepth, f_scale=F_SCALE):
    """The fit run far past every stopping rule used elsewhere: the minimiser the fit bars are measured from."""
    return affine_fit(pred, idepth, f_scale, 2000, 1e-13)


def dd(ab1, ab2, x):
    """max over valid pixels |dA x + dB| per sample, max over the samples: the distance between two fits in disparity units."""
    ab1, ab2 = np.asarray(ab1, dtype=np.float64).reshape(-1, 2), np.asarray(ab2, dtype=np.float64).reshape(-1, 2)
    x = np.asarray(x, dtype=np.float64).reshape(ab1.shape[0], -1)
    worst = 0.0
    for i in range(ab1.shape[0]):
        xi = x[i][x[i] > 0]
        if xi.size:
            worst = max(worst, float(np.abs((ab1[i, 1] - ab2[i, 1]) * xi + (ab1[i, 0] - ab2[i, 0])).max()))
    return worst


def depth2disp(depth, ab):
    """fp32 a / depth + b, divide then add, non-finite -> -100 (src/utils/geometry.py:64-69); ab [B, 2] = [b, a]."""
    ab = torch.as_tensor(np.asarray(ab)).float() if not torch.is_tensor(ab) else ab.detach().cpu().float()
    d = depth.detach().cpu().float()
    g = ab[:, 1].view(-1, 1, 1) / d + ab[:, 0].view(-1, 1, 1)
    return torch.where(torch.isfinite(g), g, torch.full_like(g, -100.0))


def branch_call(kind, target_type, pred, batch, head_weights, variance_focus, ab):
    """The 'least_square' branch of losses.SMOOTHL1Loss / SILOGLoss at a given ab (no gradient through it) -> (loss, d loss / d pred), fp64."""
    assert target_type in ('disp', 'idepth', 'depth')
    if kind == 'silog' and target_type == 'depth':              # silog.py:35-37: prediction and target are both overwritten
        target, transform = batch['depth'], 'identity'
    else:
        target = depth2disp(batch['depth'], ab)
        transform = 'reciprocal' if (kind == 'smoothL1' and target_type == 'depth') else 'identity'
    return lb.depth_loss(pred, target, batch.get('mask'), batch.get('conf'), head_weights, kind, transform, variance_focus)


class Fixture(object):
    """tests/golden/affine_fit.npz (tests/golden/make_golden_affine_fit.py): scenes 'z' (about 15 % zero depths) and 'p' (none), noise
    levels per scene, and per case the reference's ab, loss and gradient."""

    def __init__(self, golden_dir):
        self.g = np.load(golden_dir + '/affine_fit.npz')
        self.loss_weight = [float(v) for v in self.g['loss_weight']]
        self.variance_focus = float(self.g['variance_focus'])
        self.fits = sorted(k[:-len('::ref_dd')] for k in self.g.files if k.endswith('::ref_dd') and k.count('::') == 2)   # 'scene::level'
        self.cases = []
        for row in self.g['cases']:
            name, kind, tt, n, scene, level, masked, b1 = str(row).split(' ')
            self.cases.append((name, kind, tt, int(n), scene, level, bool(int(masked)), bool(int(b1))))
        # the reference's own distance from the minimiser, the largest over every fit stored: what the fit bars are multiples of
        self.ref_dd = float(max(self.g[k].max() for k in self.g.files if k.endswith('::ref_dd')))

    def t(self, key, device='cpu'):
        return torch.from_numpy(self.g[key]).to(device)

    def fields(self, fit, device='cpu'):
        """fit 'scene::level' -> pred [B, 3, H, W], idepth [B, H, W] and the reference's ab [B, 2] float32."""
        return self.t(fit + '::pred', device), self.t(fit.split('::')[0] + '::idepth', device), self.t(fit + '::ab', device)

    def inputs(self, case, device='cpu'):
        """-> pred [B or 1, n, H, W], the batch (no 'abvalue', no 'disp') and the reference's ab for this case."""
        name, kind, tt, n, scene, level, masked, b1 = case
        pred = self.t('%s::%s::%s' % (scene, level, 'pred_inv' if tt == 'depth' else 'pred'), device)
        sl = slice(0, 1) if b1 else slice(None)
        batch = {'idepth': self.t(scene + '::idepth', device)[sl].contiguous(), 'depth': self.t(scene + '::depth', device)[sl].contiguous()}
        if masked:
            batch['mask'] = self.t(scene + '::mask', device)[sl].contiguous()
        return pred[sl, :n].contiguous(), batch, self.t(name + '::ab', device)

    def head_weights(self, n):
        return [1.0] if n == 1 else self.loss_weight[:n]

    def expected(self, case):
        return torch.from_numpy(self.g[case[0] + '::loss']), torch.from_numpy(self.g[case[0] + '::grad'])
