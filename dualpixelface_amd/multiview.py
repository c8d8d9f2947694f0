"""The ``multiview`` block of a model configuration: the settings of the multi-view photometric loss (loss_type 'multiview',
losses.MULTIVIEWLoss, csrc/multiview.hip).

The loss warps the centre image of each neighbouring camera of the rig (batch['centers'], with batch['Ks'] and batch['Ps']; the FaceDP
loader produces them under ``use_multi``) into the target view through the predicted depth, batch['K'] and batch['P'], and compares the
result with batch['center'] by 3 x 3 SSIM and Barron's general robust loss.  It stands where the reference has
src/loss/depth/folded.py, which reads undefined names and cannot run; 'folded' itself stays refused.

Keys, all optional:

    select_view 3 (1 .. 8: the FIRST select_view views the batch carries are used; the reference's random draw per step is not built),
    weight_ssim 0.8 (in [0, 1]: the share of the SSIM term), alpha 1.0 (finite: the shape of the robust loss; 1 is Charbonnier, 2 is L2,
    0 is Cauchy, -2 is Geman-McClure; the limits at +-infinity are refused), scale 0.1 (> 0: its scale), image "center" (the batch
    image compared; "left" and "right" are refused by name: the loader produces no 'lefts' / 'rights' pairing that was checked),
    min_depth 1e-3 (> 0: a predicted depth below it is not usable)

Occlusion handling (per-pixel minimum over the views, visibility from a z-buffer of the prediction) has a block of its own,
``multiview_occlusion`` (dualpixelface_amd/multiview_occlusion.py), off by default.

A key missing from the block falls back to the top-level key of the same name in the model configuration (select_view, weight_ssim,
alpha, scale), so src/model/dpnet/config_multi.json's own keys mean what they say, and then to the default.

Nobody could check the conventions against FaceDP files: no dataset was at hand when this was written, so the direction of the pose
matrices (world to camera is assumed, as folded.py's comments say) and the units of the depth against the translations are unverified.
``tools/multiview_bench.py --agreement --loader`` prints the mean term under batch['depth'] for P as stored and P inverted, and for depth
units x1, x1e-3 and x1e3, so that a user who has the data can pick the minimum.  weight_ssim, alpha and scale are config_multi.json's.
"""
import collections

from .settings_block import Block

Settings = collections.namedtuple('Settings', ['select_view', 'weight_ssim', 'alpha', 'scale', 'image', 'min_depth'])
DEFAULTS = Settings(3, 0.8, 1.0, 0.1, 'center', 1e-3)
MAX_VIEWS = 8
FALLBACKS = ('select_view', 'weight_ssim', 'alpha', 'scale')


class _Block(Block):
    """Block whose missing keys fall back to the model configuration's top-level key of the same name (FALLBACKS)."""

    def __init__(self, model):
        super(_Block, self).__init__(model, 'multiview', 'multiview', DEFAULTS)
        self.model = model

    def get(self, key):
        missing = object()
        if self.block is not None:
            v = self.block.get(key, missing) if isinstance(self.block, dict) else getattr(self.block, key, missing)
            if v is not missing:
                return v
        if key in FALLBACKS and self.model is not None:
            v = self.model.get(key, missing) if isinstance(self.model, dict) else getattr(self.model, key, missing)
            if v is not missing:
                return v
        return getattr(self.defaults, key)


def settings(option):
    """The validated multiview record of an option object (config.Option, or anything whose ``model`` has a ``multiview`` attribute that
    is a dict, an attribute object or None).  A missing block or key takes the model's top-level key, then DEFAULTS; a malformed value
    raises ValueError naming its key."""
    block = _Block(getattr(option, 'model', None))
    select = block.integer('select_view', range(1, MAX_VIEWS + 1), 'an integer from 1 to %d' % MAX_VIEWS)
    wssim = block.number('weight_ssim', 'a number in [0, 1]', lambda v: 0 <= v <= 1)
    alpha = block.number('alpha', 'a finite number (the limits at +-infinity are not built)')
    scale = block.positive('scale')
    image = block.get('image')
    if image in ('left', 'right'):
        block.refuse('image', '"center" ("left" and "right" are not built: only the centre images of the neighbours are paired)', image)
    if image != 'center':
        block.refuse('image', '"center"', image)
    return Settings(select, wssim, alpha, scale, image, block.positive('min_depth'))
