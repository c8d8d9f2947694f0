"""The ``multiview_occlusion`` block of a model configuration: occlusion handling for the multi-view photometric loss (loss_type
'multiview', losses.MULTIVIEWLoss, csrc/multiview.hip).  The ``multiview`` block keeps its six keys; these live
beside it, and with the defaults the loss is exactly the one it was.

Keys, all optional:

    reduce "mean" ("mean": the mean over the views that count a pixel of each view's mean term; "min": per pixel the smallest term over
    the views that count it, averaged over the pixels some view counts -- a pixel one neighbour cannot see is scored by one that can),
    visibility "none" ("zbuffer": a pixel is seen by a neighbour where no other usable pixel of the same prediction lands in the same
    cell of that neighbour's image at a smaller depth; what is not seen is not counted), cell 2 (1, 2 or 4: the side of a z-buffer cell
    in source pixels), tolerance 0.01 (finite, >= 0: a pixel is visible up to (1 + tolerance) x the cell's smallest depth)

cell 2 and tolerance 0.01 are conventional starting values; they were not tuned on face data.  The z-buffer is built from the prediction,
so it hides what the PREDICTED surface hides, and only usable pixels splat: an occluder under the mask hides nothing.
"""
import collections

from .settings_block import Block

Settings = collections.namedtuple('Settings', ['reduce', 'visibility', 'cell', 'tolerance'])
DEFAULTS = Settings('mean', 'none', 2, 0.01)
REDUCE = ('mean', 'min')
VISIBILITY = ('none', 'zbuffer')
CELLS = (1, 2, 4)


def settings(option):
    """The validated multiview_occlusion record of an option object (config.Option, or anything whose ``model`` has a
    ``multiview_occlusion`` attribute that is a dict, an attribute object or None).  A missing block or key takes DEFAULTS; a malformed
    value raises ValueError naming its key."""
    block = Block(getattr(option, 'model', None), 'multiview_occlusion', 'multiview_occlusion', DEFAULTS)
    reduce, visibility = block.get('reduce'), block.get('visibility')
    if not isinstance(reduce, str) or reduce not in REDUCE:
        block.refuse('reduce', '"mean" or "min"', reduce)
    if not isinstance(visibility, str) or visibility not in VISIBILITY:
        block.refuse('visibility', '"none" or "zbuffer" (visibility from a label map is not built)', visibility)
    cell = block.integer('cell', CELLS, '1, 2 or 4')
    tolerance = block.number('tolerance', 'a finite number >= 0', lambda v: v >= 0)
    return Settings(reduce, visibility, cell, tolerance)
