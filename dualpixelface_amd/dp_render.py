"""The ``dp_render`` block of the configuration: the forward model of a dual-pixel sensor, used to turn an all-in-focus image and a signed
defocus disparity into the pair of half-aperture views the models train on (ops.dp_render, csrc/dp_render.hip; the definitions are in
include/dpf_hip.h and DESIGN.md section 11).

A scene point at defocus disparity d spreads over a blur disc of radius rho |d|.  One photodiode of a dual pixel looks through one half
of the aperture and so sees one half of that disc, the other photodiode the other half; the halves swap when d changes sign.  The
centroids of the two halves are 8 rho |d| / (3 pi) apart, and with the default rho = (3 pi / 8) |shift| that gap is |shift| |d|: the
displacement the photometric loss samples under the same ``shift`` and the disparity the networks regress (the half-disc model of
Punnappurath et al., ICCP 2020, and Abuolaim et al., ICCV 2021).  The reference view's point-spread function has its centroid at
-shift d / 2, the target view's at +shift d / 2, so the label d is aligned to the centre (all-in-focus) view, as a real sensor's depth is
to the sum image.  Below rho |d| = 0.5 the two views coincide (a dead zone: there is no sub-pixel area coverage), and up to rho |d| of
about 1 the gap falls short of shift d by up to a quarter of a pixel.

With the block on, ``main.py --synthetic N`` trains on rendered face scenes (dualpixelface_amd/synthetic_dp.py) in place of the noise
batch of recipe.synthetic_batch; nothing else reads it.

Keys, all optional:

    enabled false, shift null (null: the model's photometric.shift, which defaults to [0.0, -2.0]; else two finite numbers [x, y], not
    both 0), radius_scale null (null: (3 pi / 8) |shift|; else a finite number >= 0: pixels of blur radius per unit of |d|), max_radius 16
    (1 .. 32), near_sign 1 (1 | -1: whether larger d is nearer; the occlusion rule only), gamma 2.2 (the linearisation; 1: none),
    d_range [-1.5, 2.0] (the far and the near end of the synthetic scene's d, two finite numbers, low < high)

Out of scope: any gradient through the renderer, sensor noise, vignetting, point-spread functions other than a half disc, layered or
ray-traced occlusion, sub-pixel area coverage for rho |d| < 0.5, reading RGB-D files, tuning on face data.
"""
import collections

from . import ops, photometric
from .settings_block import Block, is_number

Settings = collections.namedtuple('Settings', ['enabled', 'shift', 'radius_scale', 'max_radius', 'near_sign', 'gamma', 'd_range'])
DEFAULTS = Settings(False, None, None, 16, 1, 2.2, (-1.5, 2.0))


def settings(option):
    """The validated dp_render record of an option object (config.Option, or anything with a ``dp_render`` attribute that is a dict, an
    attribute object or None).  A missing block is off; missing keys take DEFAULTS, and a null shift resolves to the model's
    photometric.shift.  A malformed value raises ValueError naming its key, whether or not the block is enabled."""
    block = Block(option, 'dp_render', 'dp_render', DEFAULTS)
    shift = block.get('shift')
    if shift is None:
        shift = photometric.settings(option).shift
    elif not isinstance(shift, (list, tuple)) or len(shift) != 2 or not all(is_number(v) for v in shift) or all(v == 0 for v in shift):
        block.refuse('shift', 'null or two finite numbers [x, y], not both 0', shift)
    scale = block.get('radius_scale')
    if scale is not None:
        scale = block.number('radius_scale', 'null or a finite number that is not negative', lambda v: v >= 0)
    radius = block.integer('max_radius', ops.DP_RENDER_RADII, 'an integer from 1 to 32')
    sign = block.integer('near_sign', (1, -1), '1 or -1')
    gamma = block.positive('gamma')
    d_range = block.get('d_range')
    if not isinstance(d_range, (list, tuple)) or len(d_range) != 2 or not all(is_number(v) for v in d_range) or not d_range[0] < d_range[1]:
        block.refuse('d_range', 'two finite numbers [low, high], low < high', d_range)
    return Settings(block.switch('enabled'), tuple(float(v) for v in shift), scale, radius, sign, gamma, tuple(float(v) for v in d_range))


def active(option):
    """Whether option.dp_render is switched on (validates the block like settings())."""
    return settings(option).enabled


def render(option, image, disparity, normalised=True, output='normalised'):
    """ops.dp_render under the block's settings (whether or not it is enabled)."""
    s = settings(option)
    return ops.dp_render(image, disparity, shift=s.shift, radius_scale=s.radius_scale, max_radius=s.max_radius, near_sign=s.near_sign,
                         gamma=s.gamma, normalised=normalised, output=output)
