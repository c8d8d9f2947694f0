"""Synthetic multi-view samples with the keys of the FaceDP loader under ``use_multi`` (dualpixelface_amd/facedp.py): a textured plane in
world space seen by a target camera and S neighbours, for smoke runs of the 'multiview' loss and for its tests when no FaceDP data is
on disk.  recipe.synthetic_batch is untouched: this module adds to its batch.

The scene is closed-form.  A camera is (K, P), P = [R | t; 0 0 0 1] world to camera.  The ray of pixel (x, y) is r = K^-1 [x, y, 1],
the plane is n . X = d, so the depth along the ray is z = (d + n . R^T t) / (n . R^T r), the world point X = R^T (z r - t), and the
colour is an analytic texture of X (three sinusoids per channel, low enough in frequency that a bilinear sample of the rendered raster is
close to the texture).  The target image and every neighbour image are rendered this way, so warping a neighbour by the TRUE depth of
the target reproduces the target image up to the bilinear interpolation of the raster.  Lambertian, no occlusion: a plane hides nothing.

Keys added: 'center' [3, H, W] and 'centers' [3 S, Hs, Ws] (normalised like the data path's images), 'P' [4, 4], 'Ks' [S, 3, 3],
'Ps' [S, 4, 4], and 'K', 'depth', 'idepth', 'disp', 'abvalue', 'mask' replaced by the scene's own, consistent with each other:
disp = a / depth + b.
"""
import numpy as np
import torch
import torch.utils.data as torch_data

from .facedp import IMAGENET_MEAN, IMAGENET_STD
from .recipe import synthetic_batch

AB = (-4.0, 8000.0)                     # [b, a]: disp = a / depth + b, depth about 800 -> disp about 6
PLANE_N, PLANE_D = (0.05, -0.08, 1.0), 800.0
WAVES = (((0.033, 0.012, 0.0), 0.3), ((-0.009, 0.039, 0.0), 1.1), ((0.021, -0.027, 0.0), 2.0))     # (wave vector, phase) per sinusoid


def rotation(rx, ry, rz):
    """R = Rz Ry Rx of three small angles (radians), fp64."""
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], np.float64)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], np.float64)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], np.float64)
    return Rz @ Ry @ Rx


def pose(angles, t):
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = rotation(*angles), t
    return P


def intrinsics(f, H, W):
    return np.array([[f, 0.0, (W - 1) / 2.0], [0.0, f, (H - 1) / 2.0], [0.0, 0.0, 1.0]], np.float64)


def texture(X):
    """RGB in [0.14, 0.86] of world points X [..., 3] -> [3, ...] (fp64)."""
    out = []
    for c in range(3):
        v = 0.5
        for k, (wave, phase) in enumerate(WAVES):
            v = v + 0.12 * np.sin(X @ np.asarray(wave) + phase + 0.7 * c * (k + 1))
        out.append(v)
    return np.stack(out, 0)


def render(K, P, H, W, plane=(PLANE_N, PLANE_D)):
    """The plane seen by the camera (K, P) (fp64 arrays) -> (rgb [3, H, W] de-normalised, depth [H, W]), fp64."""
    n, d = np.asarray(plane[0], np.float64), float(plane[1])
    R, t = P[:3, :3], P[:3, 3]
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    rays = np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(K).T              # [H, W, 3]
    z = (d + n @ (R.T @ t)) / (rays @ (R @ n))
    X = (z[..., None] * rays - t) @ R                                                     # R^T (z r - t), row vectors
    return texture(X), z


def normalise(rgb):
    m, s = np.asarray(IMAGENET_MEAN, np.float64).reshape(3, 1, 1), np.asarray(IMAGENET_STD, np.float64).reshape(3, 1, 1)
    return ((rgb - m) / s).astype(np.float32)


def rig(H, W, views, seed=0, source_size=None):
    """A target camera and `views` neighbours around it: focal length 4 W (in the thousands at FaceDP sizes), rotations of up to 0.01 rad,
    translations of tens of units at a depth of about 800, so a neighbour's parallax is a few pixels -> (K, P, Ks, Ps, (Hs, Ws)) fp64."""
    rng = np.random.RandomState((4000 + int(seed)) % 2 ** 32)
    Hs, Ws = source_size or (H + 2 * (H // 8), W + 2 * (W // 8))
    f = 4.0 * W
    K, P = intrinsics(f, H, W), pose(0.005 * rng.randn(3), 5.0 * rng.randn(3))
    Ks, Ps = [], []
    for v in range(views):
        Ks.append(intrinsics(f, Hs, Ws))
        step = pose(0.01 * rng.uniform(-1, 1, 3), np.array([20.0, 20.0, 5.0]) * rng.uniform(-1, 1, 3))
        Ps.append(step @ P)
    return K, P, np.stack(Ks), np.stack(Ps), (Hs, Ws)


def plane_sample(H, W, views=3, seed=0, source_size=None):
    """One sample of the plane scene as fp32 torch tensors: center, centers, K, P, Ks, Ps, depth, idepth, disp, abvalue, mask."""
    K, P, Ks, Ps, (Hs, Ws) = rig(H, W, views, seed, source_size)
    rgb, z = render(K, P, H, W)
    srcs = [render(Ks[v], Ps[v], Hs, Ws)[0] for v in range(views)]
    b, a = AB
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))                        # noqa: E731
    return {'center': T(normalise(rgb)), 'centers': T(np.concatenate([normalise(s) for s in srcs], 0)), 'K': T(K), 'P': T(P), 'Ks': T(Ks),
            'Ps': T(Ps), 'depth': T(z), 'idepth': T(z.max() / z), 'disp': T(a / z + b), 'abvalue': T(np.array([b, a])),
            'mask': torch.ones(H, W)}


def synthetic_multiview_batch(B, H, W, views=3, seed=0, device='cpu'):
    """recipe.synthetic_batch (the dual-pixel pair, the normals) with the plane scene's keys added or replaced."""
    batch = synthetic_batch(B, H, W, seed=seed)
    samples = [plane_sample(H, W, views, seed * 100003 + i) for i in range(B)]
    for key in samples[0]:
        batch[key] = torch.stack([s[key] for s in samples])
    return {k: v.to(device) for k, v in batch.items()}


class SyntheticMultiview(torch_data.Dataset):
    def __init__(self, length=16, height=256, width=384, views=3, seed=0):
        self.length, self.height, self.width, self.views, self.seed = int(length), int(height), int(width), int(views), int(seed)

    def __len__(self):
        return self.length

    def __getitem__(self, idx):
        batch = synthetic_multiview_batch(1, self.height, self.width, self.views, seed=self.seed * 100003 + int(idx))
        return {k: v[0] for k, v in batch.items()}


def synthetic_multiview_loader(length, height, width, batch_size, views=3, shuffle=False, seed=0, workers=0):
    return torch_data.DataLoader(SyntheticMultiview(length, height, width, views, seed), batch_size=batch_size, shuffle=shuffle,
                                 num_workers=workers, drop_last=False)
