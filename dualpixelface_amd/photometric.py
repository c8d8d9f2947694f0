"""The ``photometric`` block of a model configuration: the settings of the two label-free losses (loss_type 'photometric' and
'smoothness', losses.PHOTOMETRICLoss / SMOOTHNESSLoss, csrc/photometric.hip).

The photometric loss samples the luminance of the target view at (x + shift[0] D, y + shift[1] D), D the predicted displacement, and
compares it with the reference view (3 x 3 SSIM and a Charbonnier intensity term); the smoothness loss penalises first differences of
the prediction, less across luminance edges of the reference view.  Neither needs a label, so a batch of only 'left' and 'right' trains.

Keys, all optional:

    shift [0.0, -2.0] (x, y: two finite numbers, not both 0: the sample point moves by shift * D), alpha 0.85 (in [0, 1]: the share of
    the SSIM term), charbonnier_eps 1e-3 (> 0: the eps of sqrt(d^2 + eps^2) in both losses), smooth_gamma 10.0 (>= 0: the edge weight
    exp(-gamma |dY|))

The default shift is read off the reference's subpixel_shift: the reference view is sampled at row + d and the target at row - d
(src/module/asm/asm.py:21-36, src/model/stereodpnet/modules.py:187-188), hence ref(y) = tgt(y - 2 d), along rows.
Nobody could check this against FaceDP images: no dataset was at hand when this was written, and the axis, sign and scale per model
family are unverified.  ``tools/photometric_bench.py --agreement --loader`` prints the mean photometric term under batch['disp'] for
shift in {(0, +-1), (0, +-2), (+-1, 0), (+-2, 0)} and under zero displacement, so that a user who has the data can pick the minimum.
alpha, charbonnier_eps and smooth_gamma are conventional values, not tuned.
"""
import collections

from .settings_block import Block, is_number

Settings = collections.namedtuple('Settings', ['shift', 'alpha', 'charbonnier_eps', 'smooth_gamma'])
DEFAULTS = Settings((0.0, -2.0), 0.85, 1e-3, 10.0)


def settings(option):
    """The validated photometric record of an option object (config.Option, or anything whose ``model`` has a ``photometric`` attribute
    that is a dict, an attribute object or None).  A missing block or key takes DEFAULTS; a malformed value raises ValueError naming its
    key."""
    block = Block(getattr(option, 'model', None), 'photometric', 'photometric', DEFAULTS)
    shift = block.get('shift')
    if not isinstance(shift, (list, tuple)) or len(shift) != 2 or not all(is_number(v) for v in shift) or all(v == 0 for v in shift):
        block.refuse('shift', 'two finite numbers [x, y], not both 0', shift)
    alpha = block.number('alpha', 'a number in [0, 1]', lambda v: 0 <= v <= 1)
    eps = block.positive('charbonnier_eps')
    gamma = block.number('smooth_gamma', 'a finite number >= 0', lambda v: v >= 0)
    return Settings(tuple(float(v) for v in shift), alpha, eps, gamma)
