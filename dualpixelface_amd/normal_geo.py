"""The ``normal_geo`` block of a model configuration: the settings of the geometric-normal loss (loss_type 'normal_geo',
losses.NORMAL_GEOLoss, csrc/normal_geo.hip).

The loss takes the normals of the PREDICTED depth (the stencil of csrc/reconstruct.hip, neighbours ``step`` pixels away), compares them
with batch['normal'] and sends the gradient into pred_depth, so every model with a depth head is supervised by the ground-truth normals.

Keys, all optional:

    max_edge_ratio 0.01 (> 0: two neighbours lie on one surface while their TARGET depths differ by at most this share of the smaller),
    step 1 (1, 2 or 4: the distance of the stencil's neighbours in pixels), towards_camera true (the normals of the depth are turned to
    face the camera, n . P <= 0; false: away from it), target_signs [1, 1, 1] (each +1 or -1: multiplied into batch['normal'])

Nobody could check the frame of the normals stored in FaceDP files: no dataset was at hand when this was written.  towards_camera and
target_signs exist so that a user who has the data can match the frame; ``tools/normal_geo_bench.py --agreement`` prints the mean cosine
between the normals of batch['depth'] itself and batch['normal'] under the current settings, which is near +1 when they match.
max_edge_ratio is a conventional value; nobody has tuned it on face data.
"""
import collections

from .settings_block import Block

Settings = collections.namedtuple('Settings', ['max_edge_ratio', 'step', 'towards_camera', 'target_signs'])
DEFAULTS = Settings(0.01, 1, True, (1, 1, 1))
STEPS = (1, 2, 4)


def settings(option):
    """The validated normal_geo record of an option object (config.Option, or anything whose ``model`` has a ``normal_geo`` attribute that
    is a dict, an attribute object or None).  A missing block or key takes DEFAULTS; a malformed value raises ValueError naming its key."""
    block = Block(getattr(option, 'model', None), 'normal_geo', 'normal_geo', DEFAULTS)
    ratio = block.positive('max_edge_ratio')
    step = block.integer('step', STEPS, '1, 2 or 4')
    towards = block.switch('towards_camera')
    signs = block.get('target_signs')
    if not isinstance(signs, (list, tuple)) or len(signs) != 3 or \
            any(isinstance(v, bool) or not isinstance(v, (int, float)) or v not in (1, -1) for v in signs):
        block.refuse('target_signs', 'three values of 1 or -1', signs)
    return Settings(ratio, step, towards, tuple(int(v) for v in signs))
