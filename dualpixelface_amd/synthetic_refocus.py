"""Two textured planes with everything known: the scene the refocus block's tests and tools/refocus_bench.py render.

A near plane (a rectangle, by default the middle half of the width from a quarter of the height down, like a portrait) covers part of a
far plane.  Both carry a seeded texture -- the far plane darker than the near one, so that light that bleeds across the edge shows -- and
the defocus disparity steps from d_far to d_near at the rectangle's edge (larger is nearer: near_sign +1).  A share `holes` of the pixels
(a seeded draw) has a NaN disparity.  Plain numpy; nothing here touches the device.
"""
import numpy as np

IMAGENET_MEAN = (0.485, 0.456, 0.406)       # the data path's Normalizer (dualpixelface_amd/facedp.py states the same numbers)
IMAGENET_STD = (0.229, 0.224, 0.225)


def default_box(H, W):
    """(y0, y1, x0, x1) of the near plane: rows [y0, y1), columns [x0, x1)."""
    return H // 4, H, W // 4, W - W // 4


def normalise(v):
    """Encoded values [3, H, W] in [0, 1] -> the float32 view the data path hands the models, (v - mean) / std."""
    mean, std = np.array(IMAGENET_MEAN).reshape(3, 1, 1), np.array(IMAGENET_STD).reshape(3, 1, 1)
    return ((np.asarray(v, dtype=np.float64) - mean) / std).astype(np.float32)


def scene(H, W, box=None, d_near=1.5, d_far=-2.0, holes=0.0, seed=0, constant=None):
    """One sample -> dict of
        'near' [H, W] bool, 'mask' [H, W] float32 (the near plane), 'box' (y0, y1, x0, x1),
        'encoded' [3, H, W] float64 in [0.05, 0.95]: the far plane's texture in [0.05, 0.45], the near plane's in [0.55, 0.95]
        (`constant`: that value everywhere instead),
        'view' [3, H, W] float32: encoded, normalised as the data path does,
        'disparity' [H, W] float32: d_near on the near plane, d_far elsewhere, NaN at the holes, 'hole' [H, W] bool."""
    y0, y1, x0, x1 = default_box(H, W) if box is None else box
    near = np.zeros((H, W), dtype=bool)
    near[y0:y1, x0:x1] = True
    rng = np.random.RandomState(seed)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    smooth = 0.5 + 0.25 * np.sin(xs * 0.41 + 0.3) * np.cos(ys * 0.29)
    tex = np.stack([0.5 * smooth + 0.5 * rng.rand(H, W) for _ in range(3)])                  # in [0.125, 0.875]
    enc = np.where(near[None], 0.55 + 0.4 * tex, 0.05 + 0.4 * tex)
    if constant is not None:
        enc = np.full((3, H, W), float(constant))
    hole = rng.rand(H, W) < holes
    d = np.where(near, d_near, d_far).astype(np.float32)
    d[hole] = np.nan
    return {'near': near, 'mask': near.astype(np.float32), 'box': (y0, y1, x0, x1), 'encoded': enc, 'view': normalise(enc), 'disparity': d,
            'hole': hole}


def batch(B, H, W, **kw):
    """B scenes with seeds seed, seed + 1, ... stacked: 'view' [B, 3, H, W], 'disparity', 'mask' [B, H, W] float32, 'near' [B, H, W] bool."""
    seed = kw.pop('seed', 0)
    ones = [scene(H, W, seed=seed + b, **kw) for b in range(B)]
    return {k: np.stack([s[k] for s in ones]) for k in ('view', 'disparity', 'mask', 'near')}
