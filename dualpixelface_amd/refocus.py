"""The ``refocus`` block of the configuration: at evaluation time, render the view again with a shallow depth of field -- the application
dual-pixel depth was invented for (Garg et al., ICCV 2019, whose network is the `dpnet` model here).

An evaluation forward runs estimate -> filter -> fit -> refine -> surface -> shade.  With the block on it ends with a seventh step, refocus.
Under target_type "disp" the prediction is the signed defocus disparity d = a / z + b itself: zero on the sensor's focal plane and growing
with the blur circle, so a virtual aperture needs no calibration; under "depth" / "idepth" d = a / z + b with [b, a] from batch['abvalue']
or results['abvalue'] (the evaluation-time fit) -- an "idepth" map, which reconstruct reads as z = a / (map - b), is therefore d itself
and takes only its near sign from a.  Per sample a focus d_f is chosen on the device, every pixel gets the signed blur radius
c = clamp(aperture (d - d_f), -max_radius, max_radius), and every pixel spreads over its own disc of radius |c| -- except that a source
behind its receiver spreads no further than the receiver's own blur, which keeps a blurred background from bleeding over a sharp
foreground.  The definitions are in include/dpf_hip.h and DESIGN.md section 11, the kernels in csrc/refocus.hip.  It returns

    results['refocused']      [B, 3, H, W] fp32, encoded values in [0, 1] (not normalised)
    results['defocus']        [B, H, W] fp32, the signed c in pixels
    results['refocus_stats']  [B, 8] fp64 (ops.REFOCUS_STATS: d_f, counted pixels, valid flag, near sign used, min and max of c, then 0)

and changes no other key.

Keys, all optional:

    enabled false, source "view" ("view": the reference view; "relit": results['relit'] of shading.relight), focus "mask_mean"
    ("mask_mean": the mean of d over mask > 0 and finite; "point": the pixel nearest focus_point; "value": focus_value),
    focus_point [0.5, 0.5] (fractions of width and height), focus_value 0.0, aperture 4.0 (pixels of blur radius per pixel of disparity
    difference, >= 0), max_radius 16 (1 .. 32), near_sign "auto" ("auto" | 1 | -1: whether larger d is nearer; "auto": the sign of a where
    an abvalue is known, else +1), gamma 2.2, gain 1.0, use_mask true (the mask enters the focus only, never the rendering)

aperture, max_radius and gamma are conventional starting values; nobody has tuned them on face data, and the sign of a in FaceDP's files
is as unverified as the other conventions of that data set.  Out of scope: layered or ray-traced occlusion, bokeh shapes other than a
disc, highlight boosting, writing image files, any gradient, any model-side change.
"""
import collections

from . import ops
from .core import reference_key
from .settings_block import Block, is_number

Settings = collections.namedtuple('Settings', ['enabled', 'source', 'focus', 'focus_point', 'focus_value', 'aperture', 'max_radius', 'near_sign',
                                               'gamma', 'gain', 'use_mask'])
DEFAULTS = Settings(False, 'view', 'mask_mean', (0.5, 0.5), 0.0, 4.0, 16, 'auto', 2.2, 1.0, True)
SOURCES = ('view', 'relit')
RESULT_KEYS = ('refocused', 'defocus', 'refocus_stats')


def settings(option):
    """The validated refocus record of an option object (config.Option, or anything with a ``refocus`` attribute that is a dict, an
    attribute object or None).  A missing block is off; missing keys take DEFAULTS.  A malformed value raises ValueError naming its key,
    whether or not the block is enabled."""
    block = Block(option, 'refocus', 'refocus', DEFAULTS)
    source = block.get('source')
    if source not in SOURCES:
        block.refuse('source', 'one of %s' % ', '.join(repr(n) for n in SOURCES), source)
    focus = block.get('focus')
    if not isinstance(focus, str) or focus not in ops.REFOCUS_FOCUS:
        block.refuse('focus', 'one of %s' % ', '.join(repr(n) for n in ops.REFOCUS_FOCUS), focus)
    point = block.get('focus_point')
    if not isinstance(point, (list, tuple)) or len(point) != 2 or any(not is_number(v) or not 0 <= v <= 1 for v in point):
        block.refuse('focus_point', 'two numbers in [0, 1] (fractions of width and height)', point)
    value = block.number('focus_value')
    aperture = block.number('aperture', 'a finite number that is not negative', lambda v: v >= 0)
    radius = block.integer('max_radius', ops.REFOCUS_RADII, 'an integer from 1 to 32')
    sign = block.get('near_sign')
    if isinstance(sign, bool) or not (sign == 'auto' or (isinstance(sign, int) and sign in (1, -1))):
        block.refuse('near_sign', "'auto', 1 or -1", sign)
    gamma = block.positive('gamma')
    gain = block.number('gain', 'a finite number that is not negative', lambda v: v >= 0)
    return Settings(block.switch('enabled'), source, focus, tuple(float(v) for v in point), value, aperture, radius, sign, gamma, gain,
                    block.switch('use_mask'))


def active(option):
    """Whether option.refocus is switched on (validates the block like settings())."""
    return settings(option).enabled


def apply(option, results, batch, guide=None, training=False):
    """Attach the refocused view of an evaluation forward as option.refocus says and return `results`.  Block off, or `training`: `results`
    comes back untouched.  Otherwise RESULT_KEYS are added and no other key changes.  `guide` is the normalised view the prediction is
    aligned to (the plugin's reference view; else the batch's entry under core.reference_key).  A missing view, prediction, abvalue (for a
    'depth' / 'idepth' model) or relit image raises NotImplementedError naming what is missing and leaves `results` as it was."""
    s = settings(option)
    if training or not s.enabled:
        return results
    pred = results.get('pred_depth')
    if pred is None:
        raise NotImplementedError("refocus is switched on but the model returned no results['pred_depth'] to take the blur from")
    target_type = getattr(getattr(option, 'model', None), 'target_type', 'disp')
    ab = batch.get('abvalue')
    if ab is None:
        ab = results.get('abvalue')
    if ab is None and target_type != 'disp':
        raise NotImplementedError("refocus is switched on but neither batch['abvalue'] nor results['abvalue'] (the evaluation-time fit) "
                                  "says how a %r prediction converts to a defocus disparity" % (target_type,))
    if guide is None:
        key = reference_key(option)
        guide = batch.get(key)
        if guide is None:
            raise NotImplementedError("refocus is switched on but batch['%s'], the reference view, is missing from the batch" % key)
    source = None
    if s.source == 'relit':
        source = results.get('relit')
        if source is None:
            raise NotImplementedError("refocus.source is 'relit' but results['relit'] is missing: switch shading.relight.enabled (and "
                                      "shading.enabled) on")
    B, _, H, W = guide.shape
    mask = batch.get('mask') if s.use_mask else None
    if mask is not None:
        mask = mask.reshape(B, H, W)
    results.update(ops.refocus(guide, pred, mask=mask, ab=ab, target_type=target_type, source=source, focus=s.focus, focus_point=s.focus_point,
                               focus_value=s.focus_value, aperture=s.aperture, max_radius=s.max_radius, near_sign=s.near_sign,
                               gamma=s.gamma, gain=s.gain))
    return results
