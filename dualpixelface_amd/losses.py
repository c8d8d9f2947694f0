"""Loss hooks with the reference's contract (src/loss/loss_selector.py:7-42) over the fused HIP loss kernel.

``loss_selector(option).forward(results, batch)`` -> ``{'<name>_loss': ..., 'abvalue': ..., 'final_loss': ...}``.
Class names follow the reference's lookup rule ``<NAME.upper()>Loss`` (loss_selector.py:25).
"""
import torch

from . import ops


TARGET_TYPES = ('disp', 'depth', 'idepth')


_NO_LEAST_SQUARE = "dp_conversion='least_square' (scipy lsq_linear on the host; broken in the reference for masked batches) is not built"


def _given_only(option):
    if option.dataset.dp_conversion != 'given':
        # (the reference's own 'least_square' branch cannot run on a batch with a mask -- which every FaceDP batch has: its target is
        # [B, 1, H, W] (smoothL1.py:29-30) and is then indexed with the [B, H, W] mask (smoothL1.py:38): IndexError)
        raise NotImplementedError(_NO_LEAST_SQUARE)


def _abvalue(batch):
    if 'abvalue' not in batch:                  # smoothL1.py:28, silog.py:29: such a batch takes the 'least_square' branch
        raise NotImplementedError(_NO_LEAST_SQUARE)
    return batch['abvalue']


class _DepthLoss(object):
    """What the two depth losses share: the 'given' conversion only, and one weight per prediction head (smoothL1.py:22, silog.py:23)."""

    def __init__(self, option):
        _given_only(option)
        self.weights = list(option.model.loss_weight)

    def head_weights(self, n):
        return [1.0] if n == 1 else self.weights[:n]


class SMOOTHL1Loss(_DepthLoss):
    """Masked smooth-L1 over the prediction heads (src/loss/depth/smoothL1.py:15-49, 'given' conversion)."""

    def forward(self, preds, batch, target_type='disp'):
        assert target_type in TARGET_TYPES
        pd = preds['pred_depth']
        if target_type != 'disp':
            # smoothL1.py:27,33: the prediction against batch['idepth'], inverted first when it is a depth; conf is fused (csrc/loss_bank.hip)
            loss = ops.depth_loss(pd, batch['idepth'], batch.get('mask'), batch.get('conf'), self.head_weights(pd.shape[1]), 'smoothL1',
                                  'reciprocal' if target_type == 'depth' else 'identity')
            return {'loss': loss, 'abvalue': _abvalue(batch)}
        gt = batch['disp']
        if batch.get('conf') is not None:
            # confidence-weighted variant (smoothL1.py:33-36): both sides of the difference are multiplied by the per-pixel confidence.  No
            # loader of the reference emits 'conf', so this is two elementwise products in front of the fused loss kernel, not a kernel of its own
            pd, gt = pd * batch['conf'].unsqueeze(1), gt * batch['conf']
        mask = batch['mask'] if 'mask' in batch else torch.ones_like(batch['disp'])
        out = ops.stereo_losses(pd, None, gt, None, mask, self.head_weights(pd.shape[1]), 1.0, 0.0)
        return {'loss': out[0], 'abvalue': batch['abvalue']}


class SILOGLoss(_DepthLoss):
    """Masked scale-invariant log loss over the prediction heads (src/loss/depth/silog.py:16-52, 'given' conversion)."""

    def __init__(self, option):
        super(SILOGLoss, self).__init__(option)
        self.variance_focus = option.model.variance_focus

    def forward(self, preds, batch, target_type='disp'):
        assert target_type in TARGET_TYPES
        pd = preds['pred_depth']
        abvalue = _abvalue(batch)
        # silog.py:28-37: prediction and target are both overwritten for 'depth', so no target type inverts the prediction here
        loss = ops.depth_loss(pd, batch[target_type], batch.get('mask'), batch.get('conf'), self.head_weights(pd.shape[1]), 'silog',
                              'identity', self.variance_focus)
        return {'loss': loss, 'abvalue': abvalue}


class COSINELoss(object):
    """Masked per-channel "cosine" loss (src/loss/normal/cosine.py:35-53)."""

    def __init__(self, option):
        self.weights = list(option.model.loss_weight)

    def forward(self, preds, batch, target_type=None):
        pn = preds['pred_normal']
        if pn.shape[1] != 1:
            raise NotImplementedError('one normal prediction per sample (mainmodel.py:95)')
        mask = batch['mask'] if 'mask' in batch else torch.ones_like(batch['normal'][:, 0])
        out = ops.stereo_losses(None, pn[:, 0], None, batch['normal'], mask, [], 0.0, 1.0)
        return {'loss': out[1]}


_BANK = {'smoothL1': SMOOTHL1Loss, 'silog': SILOGLoss, 'cosine': COSINELoss}


class loss_selector(object):
    def __init__(self, option):
        assert len(option.model.loss_type) == len(option.model.lambdas)
        self.loss_func, self.loss_name, self.lambda_ = [], [], []
        for name, lam in zip(option.model.loss_type, option.model.lambdas):
            if name not in _BANK:
                raise NotImplementedError('wrong loss type : %s' % name)
            self.loss_func.append(_BANK[name](option))
            self.loss_name.append(name)
            self.lambda_.append(lam)

    def forward(self, results, batch, target_type='disp'):
        # shipped configuration (stereodpnet/config.json:2,4): one fused reduction pass for both losses
        if target_type == 'disp' and self.loss_name == ['smoothL1', 'cosine'] and results.get('pred_normal') is not None and 'mask' in batch and batch.get('conf') is None:
            pd, pn = results['pred_depth'], results['pred_normal']
            out = ops.stereo_losses(pd, pn[:, 0], batch['disp'], batch['normal'], batch['mask'],
                                    self.loss_func[0].head_weights(pd.shape[1]), self.lambda_[0], self.lambda_[1])
            return {'smoothL1_loss': out[0], 'abvalue': batch['abvalue'], 'cosine_loss': out[1], 'final_loss': out[2]}
        result, total = {}, []
        for name, lam, fn in zip(self.loss_name, self.lambda_, self.loss_func):
            out = fn.forward(results, batch, target_type)
            result[name + '_loss'] = out['loss']
            if 'abvalue' in out:
                result['abvalue'] = out['abvalue']
            total.append(lam * out['loss'])
        result['final_loss'] = sum(total)
        return result
