"""fp64 torch restatement of the depth-target loss bank (dualpixelface_amd/csrc/loss_bank.hip), the yardstick of test_loss_bank_host.py
and test_gpu_loss_bank.py.  Inputs are taken as given (float32 values widened to float64), everything after that is float64 on the CPU."""
import numpy as np
import torch

B, H, W = 2, 24, 40                      # the fixture's shape (tests/golden/make_golden_loss_bank.py)


def depth_loss(pred, target, mask=None, conf=None, head_weights=(1.0,), kind='smoothL1', transform='identity', variance_focus=0.0):
    """-> (loss, d loss / d pred), float64.  pred [B, n, H, W]; target / mask / conf [B, H, W] or None."""
    p = pred.detach().cpu().double().requires_grad_()
    g = target.detach().cpu().double()
    n = p.shape[1]
    assert len(head_weights) == n
    w = [float(np.float32(x)) for x in head_weights]             # the kernels take the weights and variance_focus as fp32
    vf = float(np.float32(variance_focus))
    if transform == 'reciprocal':
        kept = torch.isfinite(1.0 / p.detach().float())          # the fp32 quotient decides, as on the device
        pt = torch.where(kept, 1.0 / torch.where(kept, p, torch.ones_like(p)), torch.zeros_like(p))     # replaced: value 0, gradient 0
    else:
        assert transform == 'identity'
        pt = p
    if conf is not None:
        c = conf.detach().cpu().double()
        pt, g = pt * c.unsqueeze(1), g * c
    sel = mask.detach().cpu() > 0 if mask is not None else torch.ones_like(g, dtype=torch.bool)
    loss = 0.0
    for k in range(n):
        a, b = pt[:, k][sel], g[sel]                             # a pixel under the mask never enters a sum
        if kind == 'silog':
            d = w[k] * (torch.log(a) - torch.log(b))
            loss = loss + 10.0 * torch.sqrt((d ** 2).mean() - vf * d.mean() ** 2)
        else:
            assert kind == 'smoothL1'
            x = a - b
            loss = loss + w[k] * torch.where(x.abs() < 1.0, 0.5 * x * x, x.abs() - 0.5).mean()
    if loss.requires_grad and bool(sel.any()):
        grad, = torch.autograd.grad(loss, p)
    else:
        grad = torch.zeros_like(p)
    return loss.detach(), grad


def hook_call(kind, target_type, pred, batch, head_weights, variance_focus):
    """The target rules of losses.SMOOTHL1Loss / SILOGLoss (the reference's, smoothL1.py:27-33 and silog.py:28-37) over depth_loss."""
    assert target_type in ('disp', 'idepth', 'depth')
    if kind == 'silog':
        target, transform = batch[target_type], 'identity'
    else:
        target = batch['disp'] if target_type == 'disp' else batch['idepth']
        transform = 'reciprocal' if target_type == 'depth' else 'identity'
    return depth_loss(pred, target, batch.get('mask'), batch.get('conf'), head_weights, kind, transform, variance_focus)


class Fixture(object):
    """tests/golden/loss_bank.npz: shared batch arrays and prediction fields, per case the reference's loss and gradient."""

    def __init__(self, golden_dir):
        self.g = np.load(golden_dir + '/loss_bank.npz')
        self.loss_weight = [float(x) for x in self.g['loss_weight']]
        self.variance_focus = float(self.g['variance_focus'])
        self.cases = []
        for row in self.g['cases']:
            name, kind, tt, n, masked, with_conf = str(row).split(' ')
            self.cases.append((name, kind, tt, int(n), bool(int(masked)), bool(int(with_conf))))

    def inputs(self, case, device='cpu'):
        name, kind, tt, n, masked, with_conf = case
        t = lambda k: torch.from_numpy(self.g[k]).to(device)
        pred = t('pred_far' if (kind == 'silog' and tt == 'depth') else 'pred_unit')[:, :n].contiguous()
        batch = {k: t(k) for k in ('disp', 'idepth', 'depth', 'abvalue')}
        if masked:
            batch['mask'] = t('mask')
        if with_conf:
            batch['conf'] = t('conf')
        return pred, batch

    def head_weights(self, n):
        return [1.0] if n == 1 else self.loss_weight[:n]

    def expected(self, case):
        return torch.from_numpy(self.g[case[0] + '::loss']), torch.from_numpy(self.g[case[0] + '::grad'])
