"""The ``unimodal`` block of a model configuration: the settings of the unimodal loss (loss_type 'unimodal', losses.UNIMODALLoss,
csrc/unimodal.hip).  The loss is not in the reference.

Every other loss supervises the soft-argmin's expectation only; this one is the cross-entropy between the softmax over the disparity
hypotheses that the expectation is taken of and a Laplace distribution over the hypotheses centred on the label,
P_l ~ exp(-|d_l - t| / laplace_scale) (the zero-focal case of AcfNet's unimodal cost volume filtering).  It needs a model with a
hypothesis volume at the output resolution: stereodpnet, psmnet, nnet.

Keys, all optional:

    laplace_scale null (the hypothesis spacing d_1 - d_0: 0.5 px for the shipped geometry) or a positive finite number, in disparity
    units

The scale, and the weight 0.1 of src/model/stereodpnet/config_unimodal.json, are conventional starting values, not tuned.
"""
import collections

from .settings_block import Block

Settings = collections.namedtuple('Settings', ['laplace_scale'])
DEFAULTS = Settings(None)


def settings(option):
    """The validated unimodal record of an option object (config.Option, or anything whose ``model`` has a ``unimodal`` attribute that is
    a dict, an attribute object or None).  A missing block or key takes DEFAULTS; a malformed value raises ValueError naming its key."""
    block = Block(getattr(option, 'model', None), 'unimodal', 'unimodal', DEFAULTS)
    if block.get('laplace_scale') is None:
        return Settings(None)
    return Settings(block.positive('laplace_scale', 'null or a positive finite number'))
