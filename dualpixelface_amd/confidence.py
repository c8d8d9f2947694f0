"""The ``confidence`` block of the configuration: at evaluation time, say how far each pixel of the prediction can be trusted, and read the
hypothesis distribution of the disparity heads with a single-mode estimator.

The disparity heads form a softmax over 32 hypotheses per pixel and the prediction is its mean, the soft-argmin.  Where the distribution is
bimodal (hair against background) the mean lies between the modes: the flying pixels of a reconstructed mesh.  With the block on, an
evaluation forward recomputes the distribution of every pixel from the heads' low-resolution logits (csrc/head_confidence.hip through
ops.head_confidence; the definitions are in include/dpf_hip.h and DESIGN.md section 11; no [B, n, 32, H, W] volume is read) and returns

    results['pred_conf']               [B, n, H, W]  the chosen measure, in [0, 1]
    results['pred_spread']             [B, n, H, W]  the standard deviation of the distribution, in disparity units
    results['pred_depth']              with estimator "modal": the expectation over the window around the peak, for every head
    results['pred_depth_expectation']  with estimator "modal": the soft-argmin the network returned
    results['pred_conf_valid']         with a threshold: uint8 [B, H, W], head 0, pred_conf >= threshold
    results['conf_coverage']           with a threshold: [B], the share of the masked pixels (all pixels without a mask) that are valid

before post_process, so the order of an evaluation forward is estimate -> filter -> fit -> refine -> surface.  The models without a
hypothesis volume at the output resolution (dpnet, stereonet) are refused by name.

Keys, all optional:

    enabled false, measure "entropy" ("entropy": 1 - H(p) / log L; "peak": max_l p_l; "mass": the probability within `window`
    hypotheses of the peak), window 1 (0 .. 32), estimator "expectation" ("expectation" | "modal"), threshold null (or a number in
    [0, 1]), gate [] (any of "metrics", "reconstruct"; needs a threshold), report false, bins 16 (1 .. 64)

gate "metrics": the metric hooks of a validation step see the batch with its mask multiplied by pred_conf_valid (the valid map itself
where the batch has no mask); gate "reconstruct": the surface export and the PLY writer see that view (through reconstruct.use_mask).
batch['conf'], the dataset's own confidence, is a different thing and is not touched.  report: every validation step adds the
sparsification table of head 0 -- per confidence bin the pixel count and the sum of |pred - label| (ops.confidence_curve) -- into a
device table, which Trainer.validate reads once after the pass (curve_rows).

The threshold 0.5, window 1 and the measure "entropy" of config_/eval_faceDP_confidence.json are conventional starting values; nobody has
tuned them on face data.
"""
import collections

import torch

from . import ops
from .settings_block import Block

Settings = collections.namedtuple('Settings', ['enabled', 'measure', 'window', 'estimator', 'threshold', 'gate', 'report', 'bins'])
DEFAULTS = Settings(False, 'entropy', 1, 'expectation', None, (), False, 16)
MEASURES = ('entropy', 'peak', 'mass')
ESTIMATORS = ('expectation', 'modal')
GATES = ('metrics', 'reconstruct')
RESULT_KEYS = ('pred_conf', 'pred_spread', 'pred_depth_expectation', 'pred_conf_valid', 'conf_coverage')
MODELS = ('stereodpnet', 'psmnet', 'nnet')
WHY_NOT = {'dpnet': 'it regresses its output and has no hypothesis volume',
           'stereonet': 'its volume is at low resolution and in other units than the prediction'}


def settings(option):
    """The validated confidence record of an option object (config.Option, or anything with a ``confidence`` attribute that is a dict, an
    attribute object or None).  A missing block is off; missing keys take DEFAULTS.  A malformed value raises ValueError naming its key,
    whether or not the block is enabled."""
    block = Block(option, 'confidence', 'confidence', DEFAULTS)
    measure = block.get('measure')
    if measure not in MEASURES:
        block.refuse('measure', 'one of %s' % ', '.join(repr(m) for m in MEASURES), measure)
    window = block.integer('window', range(0, ops.CONFIDENCE_MAX_WINDOW + 1), 'an integer from 0 to %d' % ops.CONFIDENCE_MAX_WINDOW)
    estimator = block.get('estimator')
    if estimator not in ESTIMATORS:
        block.refuse('estimator', 'one of %s' % ', '.join(repr(e) for e in ESTIMATORS), estimator)
    threshold = block.get('threshold')
    if threshold is not None:
        threshold = block.number('threshold', 'null or a number in [0, 1]', lambda v: 0 <= v <= 1)
    gate = block.get('gate')
    if not isinstance(gate, (list, tuple)) or any(not isinstance(g, str) or g not in GATES for g in gate) or len(set(gate)) != len(gate):
        block.refuse('gate', 'a list of distinct names out of %s' % ', '.join(repr(g) for g in GATES), gate)
    if gate and threshold is None:
        block.refuse('gate', 'empty while confidence.threshold is null (a gate needs a threshold)', gate)
    bins = block.integer('bins', range(1, ops.CONFIDENCE_MAX_BINS + 1), 'an integer from 1 to %d' % ops.CONFIDENCE_MAX_BINS)
    return Settings(block.switch('enabled'), measure, window, estimator, threshold, tuple(gate), block.switch('report'), bins)


def active(option):
    """Whether option.confidence is switched on (validates the block like settings())."""
    return settings(option).enabled


def check_model(option):
    """With the block on, refuse by name a model that leaves no hypothesis distribution, the way the 'unimodal' loss does."""
    if not active(option):
        return
    model = getattr(option, 'model_name', None)
    if model not in MODELS:
        raise NotImplementedError("the confidence block is not built for the model %r%s (it needs the disparity hypotheses of %s)"
                                  % (model, ': ' + WHY_NOT[model] if model in WHY_NOT else '', ', '.join(MODELS)))


def apply(option, results, batch, training=False):
    """Attach the confidence planes of an evaluation forward as option.confidence says and return `results`.  Block off, or `training`:
    `results` comes back untouched.  Reads the private record results['_heads'] (the heads' logits and geometry); a network that leaves
    none raises NotImplementedError and `results` stays as it was."""
    s = settings(option)
    if training or not s.enabled:
        return results
    check_model(option)
    heads = results.get('_heads')
    if heads is None:
        raise NotImplementedError("confidence is switched on but the network left no results['_heads'], the logits of its disparity heads")
    want = (s.measure, 'spread') + (('modal',) if s.estimator == 'modal' else ())
    planes = ops.head_confidence(heads['logits'], heads['disp_values'], scale=heads['scale'], align_corners=heads['align_corners'],
                                 window=s.window, want=want)
    conf = planes[s.measure]
    results['pred_conf'], results['pred_spread'] = conf, planes['spread']
    if s.estimator == 'modal':
        results['pred_depth_expectation'], results['pred_depth'] = results['pred_depth'], planes['modal']
    if s.threshold is not None:
        valid = conf[:, 0] >= s.threshold
        mask = batch.get('mask')
        on = valid if mask is None else valid & (mask.reshape(valid.shape) > 0)
        total = float(valid[0].numel()) if mask is None else (mask.reshape(valid.shape) > 0).sum((1, 2)).double()
        results['pred_conf_valid'] = valid.to(torch.uint8)
        results['conf_coverage'] = on.sum((1, 2)).double() / total
    return results


def gated(option, results, batch, gate):
    """The batch the consumer `gate` ("metrics" or "reconstruct") is to see: `batch` itself unless the block is on, names that gate and
    the forward left results['pred_conf_valid']; then a shallow copy whose 'mask' is the batch's multiplied by the valid map, or the
    valid map itself (in the prediction's dtype) where the batch has none."""
    s = settings(option)
    valid = None if results is None else results.get('pred_conf_valid')
    if not s.enabled or gate not in s.gate or valid is None:
        return batch
    view = dict(batch)
    mask = batch.get('mask')
    if mask is None:
        view['mask'] = valid.to(results['pred_conf'].dtype)
    else:
        view['mask'] = mask * valid.to(mask.dtype).reshape(mask.shape)
    return view


def new_table(s, device):
    return torch.zeros((s.bins, 2), dtype=torch.float64, device=device)


def accumulate(option, results, batch, table, target_type='disp'):
    """Add the sparsification table of head 0 of one evaluated batch into `table` (None: a fresh one) and return it: pred_conf against
    |pred_depth - label|, the label batch['disp'], or batch['depth'] under [b, a] from the batch or the evaluation-time fit.  A batch
    without either label adds nothing.  No host read."""
    s = settings(option)
    if not (s.enabled and s.report) or results is None or results.get('pred_conf') is None:
        return table
    if target_type != 'disp':
        raise NotImplementedError("confidence.report needs target_type 'disp', got %r: the hypotheses are disparities" % (target_type,))
    pred, conf = results['pred_depth'], results['pred_conf']
    ab = None
    if 'disp' in batch:
        target = batch['disp']
    elif 'depth' in batch:
        target = batch['depth']
        ab = batch.get('abvalue')
        if ab is None:
            ab = results.get('abvalue')
        if ab is None:
            return table
    else:
        return table
    if table is None:
        table = new_table(s, conf.device)
    mask = batch.get('mask')
    B, H, W = conf.shape[0], conf.shape[-2], conf.shape[-1]
    return ops.confidence_curve(conf[:, 0], pred[:, 0], target.reshape(B, H, W), mask=None if mask is None else mask.reshape(B, H, W),
                                target_ab=ab, bins=s.bins, into=table)


def curve_rows(table):
    """What a sparsification table says, from a host copy of it ([bins][2] numbers): per bin edge k / bins the dict {'edge', 'coverage',
    'mean_error', 'count'} of the pixels whose confidence is at or above the edge -- their share of all counted pixels and their mean
    |pred - label| (None where there are none)."""
    table = [[float(c), float(e)] for c, e in table]
    bins, total = len(table), sum(c for c, _ in table)
    rows, count, err = [], 0.0, 0.0
    for k in range(bins - 1, -1, -1):
        count, err = count + table[k][0], err + table[k][1]
        rows.append({'edge': k / float(bins), 'coverage': count / total if total > 0 else 0.0,
                     'mean_error': err / count if count > 0 else None, 'count': count})
    return rows[::-1]
