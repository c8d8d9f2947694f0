"""The ``normal_refine`` block of the configuration: at evaluation time, bring the predicted depth into agreement with a normal map.

The network predicts a depth map and a normal map and nothing in the reference brings the two together: the depth carries the soft-argmin's
sub-pixel noise, the normals the high-frequency shape.  With the block on, an evaluation forward solves, per sample, for the log-depth
correction that makes the depth steps between neighbouring pixels follow the normals (Nehab et al. 2005; the definition is in
include/dpf_hip.h and DESIGN.md section 11, the solver in csrc/normal_refine.hip) and returns

    results['pred_depth_unrefined']  the map as it came in (after post_process and the evaluation-time fit), detached
    results['pred_depth']            the same tensor with head 0 refined
    results['refine_stats']          float64 [B, 3 + iterations]: valid pixels, edges, rho_0 .. rho_iterations of the solver

so the metric hooks and the surface export (reconstruct) both see the refined map.

Keys, all optional:

    enabled false, lambda 0.1, iterations 32 (1 .. 256), max_edge_ratio 0.01, min_cos 0.1, normals "predicted" ("predicted": head 0 of
    results['pred_normal']; "batch": batch['normal'], the ground truth -- an upper bound for diagnosis), normal_signs [1, 1, 1],
    use_mask true, near 0.0, far null

lambda, iterations and min_cos are conventional starting values; nobody has tuned them on face data.  The frame of FaceDP's stored normals
is still unverified: normal_signs plays the role of normal_geo.target_signs, and ``tools/normal_geo_bench.py --agreement --loader`` is how a
user with the data finds the signs to set.
"""
import collections
import types

from . import ops
from .settings_block import Block

Settings = collections.namedtuple('Settings', ['enabled', 'lam', 'iterations', 'max_edge_ratio', 'min_cos', 'normals', 'normal_signs',
                                               'use_mask', 'near', 'far'])
DEFAULTS = Settings(False, 0.1, 32, 0.01, 0.1, 'predicted', (1, 1, 1), True, 0.0, None)
# the defaults under the keys of the block: 'lambda' is a key there and cannot be a field here
_KEY_DEFAULTS = types.SimpleNamespace(**{('lambda' if f == 'lam' else f): v for f, v in zip(Settings._fields, DEFAULTS)})
NORMAL_SOURCES = ('predicted', 'batch')
RESULT_KEYS = ('pred_depth_unrefined', 'refine_stats')


def settings(option):
    """The validated normal_refine record of an option object (config.Option, or anything with a ``normal_refine`` attribute that is a dict,
    an attribute object or None).  A missing block is off; missing keys take DEFAULTS.  A malformed value raises ValueError naming its key,
    whether or not the block is enabled."""
    block = Block(option, 'normal_refine', 'normal_refine', _KEY_DEFAULTS)
    lam = block.positive('lambda')
    iterations = block.integer('iterations', range(1, ops.NORMAL_REFINE_MAX_ITERATIONS + 1), 'an integer from 1 to %d'
                               % ops.NORMAL_REFINE_MAX_ITERATIONS)
    ratio = block.positive('max_edge_ratio')
    min_cos = block.number('min_cos', 'a number in [0, 1)', lambda v: 0 <= v < 1)
    normals = block.get('normals')
    if normals not in NORMAL_SOURCES:
        block.refuse('normals', 'one of %s' % ', '.join(repr(n) for n in NORMAL_SOURCES), normals)
    signs = block.get('normal_signs')
    if not isinstance(signs, (list, tuple)) or len(signs) != 3 or any(isinstance(v, bool) or v not in (1, -1) for v in signs):
        block.refuse('normal_signs', 'three values of 1 or -1', signs)
    near = block.number('near', 'a finite number that is not negative', lambda v: v >= 0)
    far = block.get('far')
    if far is not None:
        far = block.number('far', 'null or a finite number larger than near = %r' % (near,), lambda v: v > near)
    return Settings(block.switch('enabled'), lam, iterations, ratio, min_cos, normals, tuple(int(v) for v in signs), block.switch('use_mask'),
                    near, far)


def active(option):
    """Whether option.normal_refine is switched on (validates the block like settings())."""
    return settings(option).enabled


def _operands(option, s, results, batch):
    """(pred, K, normal, ab, mask, target_type) of an evaluation forward, or NotImplementedError naming what is missing."""
    pred = results.get('pred_depth')
    if pred is None:
        raise NotImplementedError("normal_refine is switched on but the model returned no results['pred_depth'] to refine")
    target_type = getattr(getattr(option, 'model', None), 'target_type', 'disp')
    K = batch.get('K')
    if K is None:
        raise NotImplementedError("normal_refine is switched on but batch['K'], the camera intrinsics, is missing from the batch")
    ab = batch.get('abvalue')
    if ab is None:
        ab = results.get('abvalue')
    if ab is None and target_type != 'depth':
        raise NotImplementedError("normal_refine is switched on but neither batch['abvalue'] nor results['abvalue'] (the evaluation-time "
                                  "fit) says how a %r prediction converts to depth" % (target_type,))
    if s.normals == 'predicted':
        normal = results.get('pred_normal')
        if normal is None:
            raise NotImplementedError("normal_refine.normals is 'predicted' but the model returned no results['pred_normal']; a model "
                                      "without a normal head can only be refined with normals 'batch'")
        normal = normal.detach()[:, 0] if normal.dim() == 5 else normal.detach()
    else:
        normal = batch.get('normal')
        if normal is None:
            raise NotImplementedError("normal_refine.normals is 'batch' but batch['normal'] is missing from the batch")
    mask = batch.get('mask') if s.use_mask else None
    return pred, K, normal, (None if target_type == 'depth' else ab), mask, target_type


def apply(option, results, batch, training=False):
    """Refine head 0 of results['pred_depth'] as option.normal_refine says and return `results`.  Block off, or `training`: `results` comes
    back untouched.  Otherwise results['pred_depth_unrefined'] keeps the input (detached), results['pred_depth'] becomes the refined
    tensor (the other heads copied) and results['refine_stats'] the solver's record; no other key changes.  abvalue comes from the batch,
    else from results (the evaluation-time ops.affine_fit).  A missing K, abvalue (for a 'disp' / 'idepth' model) or normal map raises
    NotImplementedError naming the key and leaves `results` as it was."""
    s = settings(option)
    if training or not s.enabled:
        return results
    pred, K, normal, ab, mask, target_type = _operands(option, s, results, batch)
    refined, stats = ops.normal_refine(pred, K, normal, ab=ab, mask=mask, target_type=target_type, near=s.near, far=s.far,
                                       max_edge_ratio=s.max_edge_ratio, min_cos=s.min_cos, lam=s.lam, iterations=s.iterations,
                                       normal_signs=s.normal_signs, stats=True)
    results['pred_depth_unrefined'], results['pred_depth'], results['refine_stats'] = pred.detach(), refined, stats
    return results
