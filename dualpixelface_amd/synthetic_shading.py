"""A shaded ellipsoid with everything known: the scene the shading block's tests and tools/shading_bench.py fit.

An ellipsoid fills the middle of the image and shows the camera its near half, so the normals cover a hemisphere (z > 0 towards the
camera, x to the right, y down; the frame is the scene's own -- the fit does not depend on it).  It is lit by LIGHT, second-order
spherical-harmonics coefficients under which the shading of that hemisphere is positive everywhere, and carries either a uniform albedo
or a smooth texture.  Outside the ellipsoid the normal is 0 and the mask is 0.  Plain numpy; nothing here touches the device.
"""
import numpy as np

Y_CONSTANTS = (0.282095, 0.488603, 1.092548, 0.315392, 0.546274)

# [3][9]: per channel an ambient term, a key light from the upper left front, and a little of the second band
LIGHT = np.array([[2.20, -0.30, 0.42, 0.25, 0.06, -0.05, 0.10, 0.08, 0.04],
                  [2.05, -0.26, 0.40, 0.22, 0.05, -0.04, 0.09, 0.07, 0.05],
                  [1.85, -0.22, 0.36, 0.18, 0.04, -0.06, 0.08, 0.05, 0.03]], dtype=np.float64)

IMAGENET_MEAN = (0.485, 0.456, 0.406)       # the data path's Normalizer (dualpixelface_amd/facedp.py states the same numbers)
IMAGENET_STD = (0.229, 0.224, 0.225)


def basis(n):
    """Y0 .. Y8 of unit normals n [..., 3] -> [..., 9], in n's dtype, operation by operation as include/dpf_hip.h writes them."""
    t = n.dtype.type
    c0, c1, c2, c3, c4 = (t(v) for v in Y_CONSTANTS)
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    return np.stack([np.full_like(x, c0), c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z), c3 * (t(3) * (z * z) - t(1)), c2 * (x * z),
                     c4 * (x * x - y * y)], axis=-1)


def hemisphere(H, W, fill=0.92):
    """(normal [3, H, W] float64, inside [H, W] bool) of the ellipsoid whose outline spans `fill` of the image in both directions."""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    u = (xs - (W - 1) / 2.0) / (fill * W / 2.0)
    v = (ys - (H - 1) / 2.0) / (fill * H / 2.0)
    r2 = u * u + v * v
    inside = r2 < 1.0
    z = np.sqrt(np.where(inside, 1.0 - r2, 0.0))
    n = np.stack([u, v, z]) * inside
    return n, inside


def texture(H, W):
    """A smooth albedo texture [3, H, W] in [0.55, 0.95]."""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    base = 0.75 + 0.1 * np.sin(xs * 0.37) * np.cos(ys * 0.23)
    return np.stack([base + 0.1 * np.sin(ys * 0.11 + c) for c in range(3)])


def scene(H, W, albedo='uniform', outliers=0.0, outlier_value=0.95, gamma=1.0, seed=0, light=LIGHT):
    """One sample -> dict of
        'normal' [3, H, W] float32, 'mask' [H, W] float32, 'inside' [H, W] bool,
        'albedo' [3, H, W] float64 (1 everywhere under 'uniform', texture() under 'texture'),
        'shading' [3, H, W] float64 (0 outside), 'intensity' [3, H, W] float64: albedo x shading, `outliers` of the inside pixels (a seeded
        draw) replaced by outlier_value in every channel, 'outlier' [H, W] bool,
        'view' [3, H, W] float32: intensity^(1 / gamma), normalised as the data path does ((v - mean) / std).
    The light is scaled so that no pixel leaves [0.02, 0.98]: every inside pixel is counted by the default limits."""
    n, inside = hemisphere(H, W)
    seen = np.moveaxis(n.astype(np.float32).astype(np.float64), 0, -1)        # the stored normals, renormalised as the fit reads them
    seen = seen / np.where(inside, np.sqrt((seen * seen).sum(-1)), 1.0)[..., None]
    S = np.einsum('ck,hwk->chw', np.asarray(light, dtype=np.float64), basis(seen)) * inside
    rho = np.ones((3, H, W)) if albedo == 'uniform' else texture(H, W)
    I = rho * S
    rng = np.random.RandomState(seed)
    out = (rng.rand(H, W) < outliers) & inside
    I = np.where(out[None], outlier_value, I)
    v = I if gamma == 1.0 else I ** (1.0 / gamma)
    mean, std = np.array(IMAGENET_MEAN).reshape(3, 1, 1), np.array(IMAGENET_STD).reshape(3, 1, 1)
    view = ((v - mean) / std).astype(np.float32)
    return {'normal': n.astype(np.float32), 'mask': inside.astype(np.float32), 'inside': inside, 'albedo': rho, 'shading': S,
            'intensity': I, 'outlier': out, 'view': view}


def batch(B, H, W, **kw):
    """B scenes with seeds seed, seed + 1, ... stacked: 'view' and 'normal' [B, 3, H, W], 'mask' [B, H, W], 'albedo' [B, 3, H, W] float32."""
    seed = kw.pop('seed', 0)
    ones = [scene(H, W, seed=seed + b, **kw) for b in range(B)]
    return {'view': np.stack([s['view'] for s in ones]), 'normal': np.stack([s['normal'] for s in ones]),
            'mask': np.stack([s['mask'] for s in ones]), 'albedo': np.stack([s['albedo'] for s in ones]).astype(np.float32)}
