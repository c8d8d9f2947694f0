"""The ``shading`` block of the configuration: at evaluation time, relate the image to the predicted normals -- fit low-order
spherical-harmonics lighting to the reference view, and return shading, relative albedo and the face under other light.

An evaluation forward runs estimate -> filter -> fit -> refine -> surface and treats the image only as a guide.  With the block on it
ends with a sixth step, shade: per sample the lighting L ([3][9], real spherical harmonics up to `order`) that best explains the linear
intensity of the reference view under a normal map, by iteratively reweighted least squares with a uniform-albedo model (the mean albedo
is absorbed into L, so the albedo returned is relative); the definitions are in include/dpf_hip.h and DESIGN.md section 11, the kernels in
csrc/shading.hip (the Gram matrix of a pass is formed on the fp64 matrix instruction).  It returns

    results['light']          [B, 3, 9] fp32
    results['shading']        [B, 3, H, W]   sum_k L_ck Y_k(n)
    results['albedo']         [B, 3, H, W]   intensity / max(shading, shade_floor), at most albedo_max
    results['shading_valid']  [B, H, W] uint8: mask > 0 and a usable normal
    results['shading_stats']  [B, 16] fp64 (ops.SHADING_STATS: counted pixels, valid flag, passes, sum of weights, RMS residuals of the
                              first and the last pass, the scale-invariant albedo error against batch['albedo'] or -1, pixels compared)
    results['relit']          with relight.enabled: [B, 3, H, W], encoded values in [0, 1] (not normalised)

and changes no other key.  How well a Lambertian model under the normals explains the image (stats 7..9) is a check of the normals that
needs no normal label; it is the same for every normal_signs, which only the relighting rotation depends on.

Keys, all optional:

    enabled false, normals "auto" ("auto": head 0 of results['pred_normal'] where the model has a normal head, else geometric;
    "predicted"; "geometric": results['normal_geo'] where reconstruct attached it, else ops.depth_normals of the final pred_depth under
    reconstruct's near / far / max_edge_ratio / towards_camera; "batch": batch['normal']), normal_signs [1, 1, 1], order 2 (1 | 2),
    gamma 2.2, min_value 0.02, max_value 0.98, iterations 3 (0 .. 8), f_scale 0.05, ridge 1e-6, min_pixels 72, shade_floor 0.05,
    albedo_max 4.0, use_mask true, report false,
    relight {enabled false, rotate_deg [0, 0, 0], coefficients null (or [3][9] numbers), gain 1.0}

gamma, f_scale, ridge and the value limits are conventional starting values; nobody has tuned them on face data.  The unit of FaceDP's
albedo files is unknown here, which is why the albedo error is scale-invariant.  Out of scope: a fit under a per-pixel albedo label, cast
shadows and specular models, writing image files, and any gradient.
"""
import collections

import torch

from . import ops, reconstruct
from .core import reference_key
from .settings_block import Block, is_number

Relight = collections.namedtuple('Relight', ['enabled', 'rotate_deg', 'coefficients', 'gain'])
Settings = collections.namedtuple('Settings', ['enabled', 'normals', 'normal_signs', 'order', 'gamma', 'min_value', 'max_value', 'iterations',
                                               'f_scale', 'ridge', 'min_pixels', 'shade_floor', 'albedo_max', 'use_mask', 'report', 'relight'])
RELIGHT_DEFAULTS = Relight(False, (0, 0, 0), None, 1.0)
DEFAULTS = Settings(False, 'auto', (1, 1, 1), 2, 2.2, 0.02, 0.98, 3, 0.05, 1e-6, 72, 0.05, 4.0, True, False, RELIGHT_DEFAULTS)
NORMAL_SOURCES = ('auto', 'predicted', 'geometric', 'batch')
RESULT_KEYS = ('light', 'shading', 'albedo', 'shading_valid', 'shading_stats', 'relit')
NO_NORMAL_HEAD = ('dpnet', 'psmnet', 'stereonet')
REPORT_ENTRIES = 8          # the device table of shading.report: sums of stats 7..9, their samples, sums of stats 10..12, their samples


def _relight(block):
    """The validated relight record inside the shading block."""
    holder = type('Holder', (object,), {'relight': block.get('relight')})
    if holder.relight is RELIGHT_DEFAULTS:
        return RELIGHT_DEFAULTS
    sub = Block(holder, 'relight', 'shading.relight', RELIGHT_DEFAULTS)
    deg = sub.get('rotate_deg')
    if not isinstance(deg, (list, tuple)) or len(deg) != 3 or any(not is_number(v) for v in deg):
        sub.refuse('rotate_deg', 'three finite numbers (degrees about x, y, z)', deg)
    coeff = sub.get('coefficients')
    if coeff is not None:
        if (not isinstance(coeff, (list, tuple)) or len(coeff) != 3
                or any(not isinstance(row, (list, tuple)) or len(row) != 9 or any(not is_number(v) for v in row) for row in coeff)):
            sub.refuse('coefficients', 'null or [3][9] finite numbers', coeff)
        coeff = tuple(tuple(float(v) for v in row) for row in coeff)
    gain = sub.number('gain', 'a finite number that is not negative', lambda v: v >= 0)
    return Relight(sub.switch('enabled'), tuple(float(v) for v in deg), coeff, gain)


def settings(option):
    """The validated shading record of an option object (config.Option, or anything with a ``shading`` attribute that is a dict, an
    attribute object or None).  A missing block is off; missing keys take DEFAULTS.  A malformed value raises ValueError naming its key,
    whether or not the block is enabled."""
    block = Block(option, 'shading', 'shading', DEFAULTS)
    normals = block.get('normals')
    if normals not in NORMAL_SOURCES:
        block.refuse('normals', 'one of %s' % ', '.join(repr(n) for n in NORMAL_SOURCES), normals)
    signs = block.get('normal_signs')
    if not isinstance(signs, (list, tuple)) or len(signs) != 3 or any(isinstance(v, bool) or v not in (1, -1) for v in signs):
        block.refuse('normal_signs', 'three values of 1 or -1', signs)
    order = block.integer('order', ops.SHADING_ORDERS, '1 or 2')
    gamma = block.positive('gamma')
    lo = block.number('min_value', 'a number in [0, 1)', lambda v: 0 <= v < 1)
    hi = block.number('max_value', 'a number in (min_value = %r, 1]' % (lo,), lambda v: lo < v <= 1)
    iterations = block.integer('iterations', range(0, ops.SHADING_MAX_ITERATIONS + 1), 'an integer from 0 to %d' % ops.SHADING_MAX_ITERATIONS)
    f_scale = block.positive('f_scale')
    ridge = block.number('ridge', 'a finite number that is not negative', lambda v: v >= 0)
    min_pixels = block.integer('min_pixels', range(1, 1 << 31), 'a positive integer')
    floor = block.positive('shade_floor')
    amax = block.positive('albedo_max')
    return Settings(block.switch('enabled'), normals, tuple(int(v) for v in signs), order, gamma, lo, hi, iterations, f_scale, ridge,
                    min_pixels, floor, amax, block.switch('use_mask'), block.switch('report'), _relight(block))


def active(option):
    """Whether option.shading is switched on (validates the block like settings())."""
    return settings(option).enabled


def check_model(option):
    """With the block on and normals "predicted", refuse by name a model that has no normal head."""
    s = settings(option)
    model = getattr(option, 'model_name', None)
    if s.enabled and s.normals == 'predicted' and model in NO_NORMAL_HEAD:
        raise NotImplementedError("shading.normals is 'predicted' but the model %r has no normal head; use 'auto', 'geometric' or 'batch'"
                                  % (model,))


def _geometric(option, results, batch):
    """The geometric normals of the final pred_depth: reconstruct's where it attached them, else computed under its settings."""
    if results.get('normal_geo') is not None:
        return results['normal_geo']
    r = reconstruct.settings(option)
    pred, K, ab, mask, target_type = reconstruct._scene(option, r, results, batch)
    return ops.depth_normals(pred, K, ab=ab, mask=mask, target_type=target_type, near=r.near, far=r.far, max_edge_ratio=r.max_edge_ratio,
                             towards_camera=r.towards_camera)[0]


def _normals(option, s, results, batch):
    """The [B, 3, H, W] map the block fits under, or NotImplementedError naming what is missing."""
    predicted = results.get('pred_normal')
    if s.normals == 'batch':
        normal = batch.get('normal')
        if normal is None:
            raise NotImplementedError("shading.normals is 'batch' but batch['normal'] is missing from the batch")
        return normal
    if s.normals == 'predicted' and predicted is None:
        raise NotImplementedError("shading.normals is 'predicted' but the model returned no results['pred_normal']")
    if s.normals != 'geometric' and predicted is not None:
        return predicted.detach()[:, 0] if predicted.dim() == 5 else predicted.detach()
    return _geometric(option, results, batch)


def apply(option, results, batch, guide=None, training=False):
    """Attach the shading of an evaluation forward as option.shading says and return `results`.  Block off, or `training`: `results` comes
    back untouched.  Otherwise RESULT_KEYS are added ('relit' only with relight.enabled) and no other key changes.  `guide` is the
    normalised view the prediction is aligned to (the plugin's reference view; else the batch's entry under core.reference_key).  A
    missing view or normal map raises NotImplementedError naming the key and leaves `results` as it was."""
    s = settings(option)
    if training or not s.enabled:
        return results
    check_model(option)
    if guide is None:
        key = reference_key(option)
        guide = batch.get(key)
        if guide is None:
            raise NotImplementedError("shading is switched on but batch['%s'], the reference view, is missing from the batch" % key)
    normal = _normals(option, s, results, batch)
    B, _, H, W = guide.shape
    mask = batch.get('mask') if s.use_mask else None
    if mask is not None:
        mask = mask.reshape(B, H, W)
    label = batch.get('albedo')
    common = dict(mask=mask, order=s.order, gamma=s.gamma, min_value=s.min_value, max_value=s.max_value, normal_signs=s.normal_signs)
    light, stats = ops.shading_fit(guide, normal, iterations=s.iterations, f_scale=s.f_scale, ridge=s.ridge, min_pixels=s.min_pixels, **common)
    planes = ops.shading_apply(guide, normal, light, stats=stats, albedo_label=label, shade_floor=s.shade_floor, albedo_max=s.albedo_max,
                               relight=s.relight.enabled, rotate_deg=s.relight.rotate_deg, coefficients=s.relight.coefficients,
                               gain=s.relight.gain, **common)
    results['light'], results['shading_stats'] = light, stats
    results.update(planes)
    return results


def new_table(device):
    return torch.zeros(REPORT_ENTRIES, dtype=torch.float64, device=device)


def accumulate(option, results, table):
    """shading.report: add one evaluated batch into `table` (None: a fresh one) and return it -- over the valid samples the sums of
    stats 7..9 (the final RMS residual per channel) and their number, over those that had an albedo label the sums of stats 10..12 and
    their number.  No host read."""
    s = settings(option)
    stats = None if results is None else results.get('shading_stats')
    if not (s.enabled and s.report) or stats is None:
        return table
    if table is None:
        table = new_table(stats.device)
    valid = (stats[:, 1] > 0).to(stats.dtype)
    labelled = valid * (stats[:, 13] > 0).to(stats.dtype)
    table[0:3] += (stats[:, 7:10] * valid[:, None]).sum(0)
    table[3] += valid.sum()
    table[4:7] += (stats[:, 10:13] * labelled[:, None]).sum(0)
    table[7] += labelled.sum()
    return table


def report_rows(table):
    """What the table says, from a host copy of it: {'samples', 'rms_residual' [3] or None, 'albedo_samples', 'albedo_error' [3] or None}."""
    t = [float(v) for v in table]
    return {'samples': t[3], 'rms_residual': [v / t[3] for v in t[0:3]] if t[3] > 0 else None,
            'albedo_samples': t[7], 'albedo_error': [v / t[7] for v in t[4:7]] if t[7] > 0 else None}
