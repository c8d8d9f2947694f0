"""The ``post_process`` block of the configuration: edge-aware filtering of the predicted disparity at evaluation time.

The reference's configs declare ``"post_process": {"use_bilateral": false, "use_guided": false}`` and nothing in the reference reads the
block (its src/utils/visualizer.py is empty), so the behaviour is defined here and in DESIGN.md section 11: with a switch on, every head of
``results['pred_depth']`` is filtered by csrc/postprocess.hip under the guidance of the luminance of the reference view -- the joint
bilateral filter first, then the guided filter, whichever are on -- and the unfiltered map stays as ``results['pred_depth_raw']``.

Parameter keys, all optional, beside the two switches:

    guided_radius 8, guided_eps 1e-3, bilateral_radius 5, bilateral_sigma_space 3.0, bilateral_sigma_color 0.1

These defaults are conventional starting values for a guide in [0, 1]; nobody has tuned them on face data.
"""
import collections

from . import ops
from .core import reference_key
from .settings_block import Block

Settings = collections.namedtuple('Settings', ['use_bilateral', 'use_guided', 'guided_radius', 'guided_eps', 'bilateral_radius',
                                               'bilateral_sigma_space', 'bilateral_sigma_color'])
DEFAULTS = Settings(False, False, 8, 1e-3, 5, 3.0, 0.1)
GUIDED_MAX_RADIUS, BILATERAL_MAX_RADIUS = 32, 16          # what csrc/postprocess.hip supports


def settings(option):
    """The validated post_process record of an option object (config.Option, or anything with a ``post_process`` attribute that is a
    dict, an attribute object or None).  A missing block means both switches off; missing parameter keys take DEFAULTS.  A malformed value
    raises ValueError naming its key, whether or not its filter is switched on."""
    block = Block(option, 'post_process', 'post_process', DEFAULTS)

    def radius(key, most):
        return block.integer(key, range(1, most + 1), 'an integer in [1, %d]' % most)

    def positive(key):
        return block.positive(key, 'a positive number')
    return Settings(block.switch('use_bilateral'), block.switch('use_guided'), radius('guided_radius', GUIDED_MAX_RADIUS),
                    positive('guided_eps'), radius('bilateral_radius', BILATERAL_MAX_RADIUS), positive('bilateral_sigma_space'),
                    positive('bilateral_sigma_color'))


def active(option):
    """Whether option.post_process switches a filter on (validates the block like settings())."""
    s = settings(option)
    return s.use_bilateral or s.use_guided


def _guide(option, results, batch, guide):
    pred = results.get('pred_depth')
    if pred is None:
        raise NotImplementedError("post_process is switched on but the model returned no results['pred_depth'] to filter")
    if guide is None:
        key = reference_key(option)
        guide = batch.get(key)
        name = "batch['%s']" % key
    else:
        name = 'the reference view'
    if guide is None:
        raise NotImplementedError('post_process is switched on but %s, the guide image, is missing from the batch' % name)
    if guide.dim() != 4 or guide.shape[1] != 3 or pred.dim() != 4 or tuple(guide.shape[2:]) != tuple(pred.shape[2:]) or \
            guide.shape[0] != pred.shape[0]:
        raise NotImplementedError('post_process is switched on but %s %s is not a [B, 3, H, W] guide for pred_depth %s'
                                  % (name, tuple(guide.shape), tuple(pred.shape)))
    return pred, guide


def apply(option, results, batch, guide=None):
    """Filter results['pred_depth'] as option.post_process says and return `results`.  Both switches off: `results` comes back untouched.
    Otherwise results['pred_depth_raw'] keeps the unfiltered map (detached) and results['pred_depth'] becomes the joint bilateral filter
    of it, then the guided filter of that, whichever are on.  The guide is the view the prediction is aligned to: `guide` when the
    caller passes it (the plugin passes the network's reference view), else batch['right'] when option.dataset.flip_lr is set and
    batch['left'] otherwise.  A missing prediction or guide raises NotImplementedError naming it."""
    s = settings(option)
    if not (s.use_bilateral or s.use_guided):
        return results
    pred, guide = _guide(option, results, batch, guide)
    out = pred.detach()
    results['pred_depth_raw'] = out
    if s.use_bilateral:
        out = ops.joint_bilateral_filter(out, guide, s.bilateral_radius, s.bilateral_sigma_space, s.bilateral_sigma_color)
    if s.use_guided:
        out = ops.guided_filter(out, guide, s.guided_radius, s.guided_eps)
    results['pred_depth'] = out
    return results
