"""The ``reconstruct`` block of the configuration: the camera-space surface of an evaluation forward, and its export as PLY files.

The reference stops at a disparity map and a normal map (its save_result_fig_depth call is commented out, its src/utils/visualizer.py is
empty), so the behaviour is defined here and in DESIGN.md section 11.  With the block on, an evaluation forward also returns

    results['points']            [B, 3, H, W]  z K^-1 [x, y, 1] of head 0 of results['pred_depth'] (the filtered map when post_process is on)
    results['points_valid']      [B, H, W]     uint8
    results['normal_geo']        [B, 3, H, W]  normals from the depth alone, so a model without a normal head has normals too
    results['normal_geo_valid']  [B, H, W]     uint8

all from csrc/reconstruct.hip, and with ``write_ply`` a test pass of the trainer writes one binary PLY mesh per sample (extract, write_ply).

Keys, all optional:

    enabled false, write_ply false (implies enabled), stride 1 (1, 2, 4 or 8: the mesh takes every stride-th pixel), near 0.0, far null,
    max_edge_ratio 0.01, use_mask true, normals "auto" ("auto" | "predicted" | "geometric": which normals the mesh vertices carry),
    towards_camera true, colour true

max_edge_ratio -- two neighbouring pixels belong to one surface while their depths differ by at most this share of the smaller one -- is a
conventional value; nobody has tuned it on face data.
"""
import collections
import os

from . import ops
from .core import reference_key
from .settings_block import Block

Settings = collections.namedtuple('Settings', ['enabled', 'write_ply', 'stride', 'near', 'far', 'max_edge_ratio', 'use_mask', 'normals',
                                               'towards_camera', 'colour'])
DEFAULTS = Settings(False, False, 1, 0.0, None, 0.01, True, 'auto', True, True)
NORMAL_SOURCES = ('auto', 'predicted', 'geometric')
RESULT_KEYS = ('points', 'points_valid', 'normal_geo', 'normal_geo_valid')


def settings(option):
    """The validated reconstruct record of an option object (config.Option, or anything with a ``reconstruct`` attribute that is a dict, an
    attribute object or None).  A missing block is off; missing keys take DEFAULTS; write_ply switches enabled on.  A malformed value raises
    ValueError naming its key, whether or not the block is enabled."""
    block = Block(option, 'reconstruct', 'reconstruct', DEFAULTS)
    write = block.switch('write_ply')
    stride = block.integer('stride', ops.MESH_STRIDES, '1, 2, 4 or 8')
    near = block.number('near')
    if near < 0:
        raise ValueError('reconstruct.near must not be negative, got %r' % (near,))
    far = block.get('far')
    if far is not None:
        far = block.number('far')
        if not far > near:
            block.refuse('far', 'null or larger than near = %r' % (near,), far)
    ratio = block.number('max_edge_ratio')
    if not ratio > 0:
        block.refuse('max_edge_ratio', 'positive', ratio)
    normals = block.get('normals')
    if normals not in NORMAL_SOURCES:
        block.refuse('normals', 'one of %s' % ', '.join(repr(n) for n in NORMAL_SOURCES), normals)
    return Settings(block.switch('enabled') or write, write, stride, near, far, ratio, block.switch('use_mask'), normals,
                    block.switch('towards_camera'), block.switch('colour'))


def active(option):
    """Whether option.reconstruct is switched on (validates the block like settings())."""
    return settings(option).enabled


def _scene(option, s, results, batch):
    """(pred, K, ab, mask, target_type) of an evaluation forward, or NotImplementedError naming what is missing."""
    pred = results.get('pred_depth')
    if pred is None:
        raise NotImplementedError("reconstruct is switched on but the model returned no results['pred_depth'] to place in space")
    target_type = getattr(getattr(option, 'model', None), 'target_type', 'disp')
    K = batch.get('K')
    if K is None:
        raise NotImplementedError("reconstruct is switched on but batch['K'], the camera intrinsics, is missing from the batch")
    ab = batch.get('abvalue')
    if ab is None:
        ab = results.get('abvalue')
    if ab is None and target_type != 'depth':
        raise NotImplementedError("reconstruct is switched on but neither batch['abvalue'] nor results['abvalue'] (the evaluation-time fit) "
                                  "says how a %r prediction converts to depth" % (target_type,))
    mask = batch.get('mask') if s.use_mask else None
    return pred, K, (None if target_type == 'depth' else ab), mask, target_type


def apply(option, results, batch, guide=None, training=False):
    """Attach the camera-space surface of results['pred_depth'] (head 0) as option.reconstruct says and return `results`.  Block off, or
    `training`: `results` comes back untouched.  Otherwise RESULT_KEYS are added and no other key changes.  abvalue comes from the batch,
    else from results (the evaluation-time ops.affine_fit); a missing K, or a missing abvalue for a 'disp' / 'idepth' model, raises
    NotImplementedError naming the key and leaves `results` as it was.  `guide` is unused here (extract colours the mesh with it)."""
    s = settings(option)
    if training or not s.enabled:
        return results
    pred, K, ab, mask, target_type = _scene(option, s, results, batch)
    if s.normals == 'predicted' and results.get('pred_normal') is None:
        raise NotImplementedError("reconstruct.normals is 'predicted' but the model returned no results['pred_normal']")
    points, valid = ops.backproject(pred, K, ab=ab, mask=mask, target_type=target_type, near=s.near, far=s.far)
    normal, nvalid = ops.depth_normals(pred, K, ab=ab, mask=mask, target_type=target_type, near=s.near, far=s.far,
                                       max_edge_ratio=s.max_edge_ratio, towards_camera=s.towards_camera)
    results['points'], results['points_valid'], results['normal_geo'], results['normal_geo_valid'] = points, valid, normal, nvalid
    return results


def _vertex_normals(s, results, scene):
    """The [B, 3, H, W] map the mesh vertices take their normals from: head 0 of results['pred_normal'] or the geometric normals (those
    apply() attached, else computed here)."""
    predicted = results.get('pred_normal')
    if s.normals == 'predicted' and predicted is None:
        raise NotImplementedError("reconstruct.normals is 'predicted' but the model returned no results['pred_normal']")
    if s.normals != 'geometric' and predicted is not None:
        return predicted.detach()[:, 0] if predicted.dim() == 5 else predicted.detach()
    if results.get('normal_geo') is not None:
        return results['normal_geo']
    pred, K, ab, mask, target_type = scene
    return ops.depth_normals(pred, K, ab=ab, mask=mask, target_type=target_type, near=s.near, far=s.far, max_edge_ratio=s.max_edge_ratio,
                             towards_camera=s.towards_camera)[0]


def extract(option, results, batch, guide=None):
    """The triangle mesh of every sample of an evaluation forward -> a list, one entry per sample, of numpy arrays
    (vertices [V, 3] float32, normals [V, 3] float32, colours [V, 3] uint8, faces [F, 3] int32).  ops.depth_mesh on the device, then ONE host
    copy of the counts before the buffers are trimmed.  The colours come from `guide`, the normalised view the prediction is aligned to
    (the plugin's reference view; else batch['right'] under option.dataset.flip_lr and batch['left'] otherwise), or are 255 with colour off."""
    s = settings(option)
    scene = _scene(option, s, results, batch)
    pred, K, ab, mask, target_type = scene
    view = None
    if s.colour:
        if guide is None:
            key = reference_key(option)
            guide = batch.get(key)
            if guide is None:
                raise NotImplementedError("reconstruct.colour is on but batch['%s'], the view the vertices take their colour from, is missing "
                                          "from the batch" % key)
        view = guide
    vertices, normals, colours, faces, counts = ops.depth_mesh(pred, K, _vertex_normals(s, results, scene), ab=ab, mask=mask, view=view,
                                                               target_type=target_type, stride=s.stride, near=s.near, far=s.far,
                                                               max_edge_ratio=s.max_edge_ratio, towards_camera=s.towards_camera)
    counts = counts.cpu().tolist()                            # the one host read
    out = []
    for b, (nv, nf) in enumerate(counts):
        out.append((vertices[b, :nv].cpu().numpy(), normals[b, :nv].cpu().numpy(), colours[b, :nv].cpu().numpy(), faces[b, :nf].cpu().numpy()))
    return out


def write_ply(path, vertices, normals, colours, faces):
    """One mesh as a binary_little_endian 1.0 PLY file: vertex properties x y z nx ny nz (float) and red green blue (uchar), faces as
    ``property list uchar int vertex_indices``.  Plain numpy."""
    import numpy as np
    vertices = np.ascontiguousarray(vertices, dtype='<f4').reshape(-1, 3)
    normals = np.ascontiguousarray(normals, dtype='<f4').reshape(-1, 3)
    colours = np.ascontiguousarray(colours, dtype=np.uint8).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype='<i4').reshape(-1, 3)
    if not len(vertices) == len(normals) == len(colours):
        raise ValueError('write_ply: %d vertices, %d normals, %d colours' % (len(vertices), len(normals), len(colours)))
    if len(faces) and (faces.min() < 0 or faces.max() >= len(vertices)):
        raise ValueError('write_ply: a face index lies outside the %d vertices' % len(vertices))
    header = ('ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n'
              'property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n'
              'element face %d\nproperty list uchar int vertex_indices\nend_header\n' % (len(vertices), len(faces)))
    vrec = np.empty(len(vertices), dtype=[('p', '<f4', 3), ('n', '<f4', 3), ('c', 'u1', 3)])
    vrec['p'], vrec['n'], vrec['c'] = vertices, normals, colours
    frec = np.empty(len(faces), dtype=[('k', 'u1'), ('i', '<i4', 3)])
    frec['k'], frec['i'] = 3, faces
    tmp = path + '.tmp'
    with open(tmp, 'wb') as fh:
        fh.write(header.encode('ascii'))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())
    os.replace(tmp, path)
    return path


def output_dir(option, workspace_path):
    """Where a test pass writes its meshes: <option.output_path, else workspace_path/output>/recon."""
    base = getattr(option, 'output_path', None) or os.path.join(str(workspace_path), 'output')
    return os.path.join(str(base), 'recon')


def write_batch(option, workspace_path, position, results, batch, guide=None):
    """Write the meshes of one evaluated batch as <output_dir>/<loader position>_<sample>.ply and return the paths.  Loader positions are
    unique across ranks (every rank evaluates its own positions), so no two ranks write the same file."""
    folder = output_dir(option, workspace_path)
    os.makedirs(folder, exist_ok=True)
    paths = []
    for b, mesh in enumerate(extract(option, results, batch, guide)):
        paths.append(write_ply(os.path.join(folder, '%d_%d.ply' % (position, b)), *mesh))
    return paths
