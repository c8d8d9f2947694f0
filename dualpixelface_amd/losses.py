"""Loss hooks with the reference's contract (src/loss/loss_selector.py:7-42) over the fused HIP loss kernel.

``loss_selector(option).forward(results, batch)`` -> ``{'<name>_loss': ..., 'abvalue': ..., 'final_loss': ...}``.
Class names follow the reference's lookup rule ``<NAME.upper()>Loss`` (loss_selector.py:25).
"""
import torch

from . import multiview, multiview_occlusion, normal_geo, ops, photometric, unimodal
from .core import reference_key


TARGET_TYPES = ('disp', 'depth', 'idepth')


def takes_least_square(batch):
    """smoothL1.py:28, silog.py:29: a batch that brings no (a, b) has its disparity conversion fitted (the reference's 'least_square'
    branch).  The other way into that branch, dataset.dp_conversion == 'least_square' over a batch that does bring one, stays refused."""
    return 'abvalue' not in batch


def conversion(preds, batch):
    """THE (a, b) rule of every loss, as a function of no arguments that a loss calls where it needs the conversion: batch['abvalue'],
    else the fitted one (src/utils/geometry.py::regress_affine on the device, ops.affine_fit): [b, a] per sample between head 0 of the
    raw prediction and batch['idepth'], whatever the target type; detached, as the reference fits under no_grad.  The fit is enqueued
    at the first call and kept: loss_selector.forward hands one such function to all its losses, so a step fits once."""
    kept = []

    def ab():
        if not takes_least_square(batch):
            return batch['abvalue']
        if not kept:
            missing = [k for k in ('idepth', 'depth') if k not in batch]
            if missing:
                raise NotImplementedError("a batch without 'abvalue' takes the 'least_square' disparity conversion, which needs batch[%s]"
                                          % "] and batch[".join(repr(k) for k in missing))
            kept.append(ops.affine_fit(preds['pred_depth'], batch['idepth']))
        return kept[0]
    return ab


class _HeadWeights(object):
    """What every loss over the heads of pred_depth shares: one weight per prediction head (smoothL1.py:22, silog.py:23)."""

    def __init__(self, option):
        self.weights = list(option.model.loss_weight)

    def head_weights(self, n):
        return [1.0] if n == 1 else self.weights[:n]


class _DepthLoss(_HeadWeights):
    """What the losses that read a label share: the dp_conversion they refuse."""

    def __init__(self, option):
        super(_DepthLoss, self).__init__(option)
        if option.dataset.dp_conversion != 'given':
            # the fit itself is built and every batch without 'abvalue' takes it; ignoring an 'abvalue' the batch does bring is not switched on
            raise NotImplementedError("dp_conversion=%r is not built as a dataset setting (a batch without 'abvalue' takes the 'least_square' "
                                      "fit under 'given')" % (option.dataset.dp_conversion,))


class SMOOTHL1Loss(_DepthLoss):
    """Masked smooth-L1 over the prediction heads (src/loss/depth/smoothL1.py:15-49)."""

    def forward(self, preds, batch, target_type='disp', ab_of=None):
        assert target_type in TARGET_TYPES
        pd = preds['pred_depth']
        transform = 'reciprocal' if target_type == 'depth' else 'identity'          # smoothL1.py:27
        if takes_least_square(batch):
            # smoothL1.py:29-30 with the [B, H, W] target the class lacks: depth2disp(batch['depth'], ab) is formed inside the loss kernels
            ab = (ab_of or conversion(preds, batch))()
            loss = ops.depth_loss(pd, batch['depth'], batch.get('mask'), batch.get('conf'), self.head_weights(pd.shape[1]), 'smoothL1',
                                  transform, target_ab=ab)
            return {'loss': loss, 'abvalue': ab}
        if target_type != 'disp':
            # smoothL1.py:27,33: the prediction against batch['idepth'], inverted first when it is a depth; conf is fused (csrc/loss_bank.hip)
            loss = ops.depth_loss(pd, batch['idepth'], batch.get('mask'), batch.get('conf'), self.head_weights(pd.shape[1]), 'smoothL1',
                                  transform)
            return {'loss': loss, 'abvalue': batch['abvalue']}
        gt = batch['disp']
        if batch.get('conf') is not None:
            # confidence-weighted variant (smoothL1.py:33-36): both sides of the difference are multiplied by the per-pixel confidence.  No
            # loader of the reference emits 'conf', so this is two elementwise products in front of the fused loss kernel, not a kernel of its own
            pd, gt = pd * batch['conf'].unsqueeze(1), gt * batch['conf']
        mask = batch['mask'] if 'mask' in batch else torch.ones_like(batch['disp'])
        out = ops.stereo_losses(pd, None, gt, None, mask, self.head_weights(pd.shape[1]), 1.0, 0.0)
        return {'loss': out[0], 'abvalue': batch['abvalue']}


class SILOGLoss(_DepthLoss):
    """Masked scale-invariant log loss over the prediction heads (src/loss/depth/silog.py:16-52)."""

    def __init__(self, option):
        super(SILOGLoss, self).__init__(option)
        self.variance_focus = option.model.variance_focus

    def forward(self, preds, batch, target_type='disp', ab_of=None):
        assert target_type in TARGET_TYPES
        pd = preds['pred_depth']
        fitted = takes_least_square(batch)
        abvalue = (ab_of or conversion(preds, batch))()
        if fitted and target_type != 'depth':
            # silog.py:30-31 with the [B, H, W] target; a non-positive a / depth + b gives NaN as in the reference (no clamp)
            loss = ops.depth_loss(pd, batch['depth'], batch.get('mask'), batch.get('conf'), self.head_weights(pd.shape[1]), 'silog',
                                  'identity', self.variance_focus, target_ab=abvalue)
            return {'loss': loss, 'abvalue': abvalue}
        # silog.py:28-37: prediction and target are both overwritten for 'depth', so no target type inverts the prediction here (and under
        # the fitted conversion only the returned abvalue is the fit's)
        loss = ops.depth_loss(pd, batch[target_type], batch.get('mask'), batch.get('conf'), self.head_weights(pd.shape[1]), 'silog',
                              'identity', self.variance_focus)
        return {'loss': loss, 'abvalue': abvalue}


class COSINELoss(object):
    """Masked per-channel "cosine" loss (src/loss/normal/cosine.py:35-53)."""

    def __init__(self, option):
        self.weights = list(option.model.loss_weight)

    def forward(self, preds, batch, target_type=None, ab_of=None):
        pn = preds['pred_normal']
        if pn.shape[1] != 1:
            raise NotImplementedError('one normal prediction per sample (mainmodel.py:95)')
        mask = batch['mask'] if 'mask' in batch else torch.ones_like(batch['normal'][:, 0])
        out = ops.stereo_losses(None, pn[:, 0], None, batch['normal'], mask, [], 0.0, 1.0)
        return {'loss': out[1]}


class NORMAL_GEOLoss(_DepthLoss):
    """The geometric-normal loss (not in the reference; DESIGN.md section 11, csrc/normal_geo.hip): the normals of the depth every head of
    pred_depth predicts against batch['normal'], the gradient going back into pred_depth.  Settings: the model config block normal_geo
    (normal_geo.settings).  The conversion is the depth losses': batch['abvalue'], else the fit."""

    def __init__(self, option):
        super(NORMAL_GEOLoss, self).__init__(option)
        self.settings = normal_geo.settings(option)

    def forward(self, preds, batch, target_type='disp', ab_of=None):
        assert target_type in TARGET_TYPES
        for key in ('K', 'depth', 'normal'):
            if key not in batch:
                raise NotImplementedError("the 'normal_geo' loss needs batch[%r], which is missing from the batch" % key)
        pd = preds['pred_depth']
        out, ab = {}, None
        if target_type != 'depth':
            ab = out['abvalue'] = (ab_of or conversion(preds, batch))()
        elif 'abvalue' in batch:
            out['abvalue'] = batch['abvalue']              # (a depth prediction needs no conversion; handed on as the depth losses do)
        s = self.settings
        out['loss'] = ops.normal_geo_loss(pd, batch['depth'], batch['normal'], batch['K'], ab=ab, mask=batch.get('mask'),
                                          head_weights=self.head_weights(pd.shape[1]), target_type=target_type,
                                          max_edge_ratio=s.max_edge_ratio, step=s.step, towards_camera=s.towards_camera,
                                          target_signs=s.target_signs)
        return out


class _LabelFreeLoss(_HeadWeights):
    """What the two label-free losses share (not in the reference; DESIGN.md section 11, csrc/photometric.hip): the settings of the model
    config block photometric (photometric.settings), one weight per prediction head, and the two views, swapped under dataset.flip_lr
    as the training branch of core._views swaps them.  Neither reads a label, so neither refuses a dp_conversion."""
    name = None

    def __init__(self, option):
        super(_LabelFreeLoss, self).__init__(option)
        self.settings = photometric.settings(option)
        self.reference = reference_key(option)

    def views(self, batch):
        """(reference view, target view)"""
        for key in ('left', 'right'):
            if key not in batch:
                raise NotImplementedError("the %r loss needs batch[%r], which is missing from the batch" % (self.name, key))
        return batch[self.reference], batch['left' if self.reference == 'right' else 'right']


class PHOTOMETRICLoss(_LabelFreeLoss):
    """The photometric loss: the target view warped by the displacement every head of pred_depth predicts against the reference view.
    (a, b) is needed for target_type 'depth' only: batch['abvalue'], else the fit, as in NORMAL_GEOLoss."""
    name = 'photometric'

    def forward(self, preds, batch, target_type='disp', ab_of=None):
        assert target_type in TARGET_TYPES
        ref, tgt = self.views(batch)
        pd = preds['pred_depth']
        out, ab = {}, None
        if target_type == 'depth':
            ab = out['abvalue'] = (ab_of or conversion(preds, batch))()
        s = self.settings
        out['loss'] = ops.photometric_loss(pd, ref, tgt, ab=ab, mask=batch.get('mask'), head_weights=self.head_weights(pd.shape[1]),
                                           target_type=target_type, shift=s.shift, alpha=s.alpha, eps=s.charbonnier_eps)
        return out


class SMOOTHNESSLoss(_LabelFreeLoss):
    """The edge-aware smoothness of every head of pred_depth under the luminance of the reference view."""
    name = 'smoothness'

    def forward(self, preds, batch, target_type='disp', ab_of=None):
        assert target_type in TARGET_TYPES
        ref, _ = self.views(batch)
        pd = preds['pred_depth']
        s = self.settings
        return {'loss': ops.smoothness_loss(pd, ref, mask=batch.get('mask'), head_weights=self.head_weights(pd.shape[1]),
                                            gamma=s.smooth_gamma, eps=s.charbonnier_eps)}


class UNIMODALLoss(_DepthLoss):
    """The unimodal loss (not in the reference; DESIGN.md section 11, csrc/unimodal.hip): the cross-entropy between the hypothesis
    distribution of every disparity head and a Laplace distribution centred on the label, the gradient going into the heads' logits.
    It reads the private record results['_heads'] the models with a hypothesis volume at the output resolution leave (stereodpnet,
    psmnet, nnet), not pred_depth.  Settings: the model config block unimodal (unimodal.settings).  The target rule is SMOOTHL1Loss's:
    batch['disp'], or under the fitted conversion batch['depth'] with the shared (a, b)."""
    MODELS = ('stereodpnet', 'psmnet', 'nnet')
    WHY_NOT = {'dpnet': 'it regresses its output and has no hypothesis volume',
               'stereonet': 'its volume is at low resolution and in other units than the prediction'}

    def __init__(self, option):
        super(UNIMODALLoss, self).__init__(option)
        model = getattr(option, 'model_name', None)
        if model not in self.MODELS:
            raise NotImplementedError("the 'unimodal' loss is not built for the model %r%s (it needs the disparity hypotheses of %s)"
                                      % (model, ': ' + self.WHY_NOT[model] if model in self.WHY_NOT else '', ', '.join(self.MODELS)))
        self.settings = unimodal.settings(option)

    def forward(self, preds, batch, target_type='disp', ab_of=None):
        if target_type != 'disp':
            raise NotImplementedError("the 'unimodal' loss needs target_type 'disp', got %r: the hypotheses are disparities" % (target_type,))
        heads = preds.get('_heads')
        if heads is None:
            raise NotImplementedError("the 'unimodal' loss needs results['_heads'], which this network does not leave")
        common = dict(head_weights=self.head_weights(len(heads['logits'])), scale=heads['scale'], align_corners=heads['align_corners'],
                      laplace_scale=self.settings.laplace_scale)
        if takes_least_square(batch):
            ab = (ab_of or conversion(preds, batch))()
            loss = ops.unimodal_loss(heads['logits'], heads['disp_values'], batch['depth'], batch.get('mask'), target_ab=ab, **common)
            return {'loss': loss, 'abvalue': ab}
        loss = ops.unimodal_loss(heads['logits'], heads['disp_values'], batch['disp'], batch.get('mask'), **common)
        return {'loss': loss, 'abvalue': batch['abvalue']}


class MULTIVIEWLoss(_HeadWeights):
    """The multi-view photometric loss (csrc/multiview.hip; it stands where the reference has
    src/loss/depth/folded.py, which cannot run): batch['centers'], the centre images of the neighbouring cameras, warped into the target
    view through the depth every head of pred_depth predicts, batch['K'] / batch['P'] and batch['Ks'] / batch['Ps'], against
    batch['center'].  Settings: the model config block multiview (multiview.settings); the first select_view views are used.  It reads
    calibration but no label map, so it refuses no dp_conversion.  (a, b) is needed for target_type 'disp' only: batch['abvalue'], else
    the fit, as in PHOTOMETRICLoss.  batch['conf'] is not read.  Occlusion handling (per-pixel minimum over the views, visibility from a
    z-buffer of the prediction) is the block multiview_occlusion (multiview_occlusion.settings), off by default: .occlusion."""
    name = 'multiview'
    KEYS = ('center', 'centers', 'K', 'P', 'Ks', 'Ps')

    def __init__(self, option):
        super(MULTIVIEWLoss, self).__init__(option)
        self.settings = multiview.settings(option)
        self.occlusion = multiview_occlusion.settings(option)

    def forward(self, preds, batch, target_type='disp', ab_of=None):
        assert target_type in TARGET_TYPES
        missing = [key for key in self.KEYS if key not in batch]
        if missing:
            raise NotImplementedError("the 'multiview' loss needs batch[%s], which %s missing from the batch (the FaceDP loader produces "
                                      "them under use_multi with use_center_img and multi_view.use_center_img)"
                                      % ("] and batch[".join(repr(k) for k in missing), 'is' if len(missing) == 1 else 'are'))
        s = self.settings
        pd, centers, Ks, Ps = preds['pred_depth'], batch['centers'], batch['Ks'], batch['Ps']
        views = min(centers.shape[1] // 3, Ks.shape[1], Ps.shape[1])
        if centers.dim() != 4 or centers.shape[1] % 3 or views < s.select_view:
            raise NotImplementedError("the 'multiview' loss is set to select_view = %d, but the batch carries %d views (centers %s, Ks %s, Ps %s)"
                                      % (s.select_view, views, tuple(centers.shape), tuple(Ks.shape), tuple(Ps.shape)))
        S = s.select_view
        src = centers[:, :3 * S].view(centers.shape[0], S, 3, centers.shape[2], centers.shape[3])
        out, ab = {}, None
        if target_type == 'disp':
            ab = out['abvalue'] = (ab_of or conversion(preds, batch))()
        elif 'abvalue' in batch:
            out['abvalue'] = batch['abvalue']
        f32 = lambda t: t if t.dtype == torch.float32 else t.to(torch.float32)                        # noqa: E731
        out['loss'] = ops.multiview_loss(pd, f32(batch['center']), f32(src), f32(batch['K']), f32(batch['P']), f32(Ks[:, :S]), f32(Ps[:, :S]),
                                         ab=None if ab is None else f32(ab), mask=batch.get('mask'),
                                         head_weights=self.head_weights(pd.shape[1]), target_type=target_type, weight_ssim=s.weight_ssim,
                                         alpha=s.alpha, scale=s.scale, min_depth=s.min_depth, **self.occlusion._asdict())
        return out


LABEL_FREE = ('photometric', 'smoothness', 'multiview')
_BANK = {'smoothL1': SMOOTHL1Loss, 'silog': SILOGLoss, 'cosine': COSINELoss, 'normal_geo': NORMAL_GEOLoss, 'photometric': PHOTOMETRICLoss,
         'smoothness': SMOOTHNESSLoss, 'unimodal': UNIMODALLoss, 'multiview': MULTIVIEWLoss}


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

    def least_square(self, batch):
        return takes_least_square(batch)

    def label_free(self):
        """Every configured loss is one of those that read no label map: a batch of only the views (and, for 'multiview', the rig's
        calibration) trains."""
        return bool(self.loss_name) and all(name in LABEL_FREE for name in self.loss_name)

    def forward(self, results, batch, target_type='disp'):
        # shipped configuration (stereodpnet/config.json:2,4): one fused reduction pass for both losses, against the disparity the batch brings
        if not self.least_square(batch) and target_type == 'disp' and self.loss_name == ['smoothL1', 'cosine'] and results.get('pred_normal') is not None and 'mask' in batch and batch.get('conf') is None:
            pd, pn = results['pred_depth'], results['pred_normal']
            out = ops.stereo_losses(pd, pn[:, 0], batch['disp'], batch['normal'], batch['mask'],
                                    self.loss_func[0].head_weights(pd.shape[1]), self.lambda_[0], self.lambda_[1])
            return {'smoothL1_loss': out[0], 'abvalue': batch['abvalue'], 'cosine_loss': out[1], 'final_loss': out[2]}
        result, total, ab_of = {}, [], conversion(results, batch)
        for name, lam, fn in zip(self.loss_name, self.lambda_, self.loss_func):
            out = fn.forward(results, batch, target_type, ab_of)
            result[name + '_loss'] = out['loss']
            if 'abvalue' in out:
                result['abvalue'] = out['abvalue']
            total.append(lam * out['loss'])
        result['final_loss'] = sum(total)
        return result
