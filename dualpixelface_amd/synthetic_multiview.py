"""Synthetic multi-view samples with the keys of the FaceDP loader under ``use_multi`` (dualpixelface_amd/facedp.py): a textured plane in
world space seen by a target camera and S neighbours, for smoke runs of the 'multiview' loss and for its tests when no FaceDP data is
on disk.  recipe.synthetic_batch is untouched: this module adds to its batch.

The scene is closed-form.  A camera is (K, P), P = [R | t; 0 0 0 1] world to camera.  The ray of pixel (x, y) is r = K^-1 [x, y, 1],
the plane is n . X = d, so the depth along the ray is z = (d + n . R^T t) / (n . R^T r), the world point X = R^T (z r - t), and the
colour is an analytic texture of X (three sinusoids per channel, low enough in frequency that a bilinear sample of the rendered raster is
close to the texture).  The target image and every neighbour image are rendered this way, so warping a neighbour by the TRUE depth of
the target reproduces the target image up to the bilinear interpolation of the raster.  Lambertian, no occlusion: a plane hides nothing.
The occluder scene below (occluder_sample) puts a rectangle in front of the plane, with closed-form visibility, for the occlusion modes.

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


# ---- the occluder scene: the plane, and in front of it a fronto-parallel textured rectangle (taller than every frame, and reaching beyond
# it on the right) that hides a band of the plane from a camera to its right.  Closed form as well: per ray the nearest hit.  Units are those of the plane scene.
OCCLUDER_Z = 400.0                       # the rectangle lies in the world plane Z = OCCLUDER_Z (the plane is at about 800)
OCCLUDER_Y = (-1.0e4, 1.0e4)
OCCLUDER_SHIFT = (37.0, -21.0, 0.0)      # its texture is the plane's read at X + OCCLUDER_SHIFT: its own phase


def occluder_x(W):
    """The rectangle's extent in world x: from two target pixels left of the image centre (at a focal length of 4 W) to beyond every
    frame on the right.  One silhouette edge lies in the frame: the windows within a few columns of a silhouette straddle the depth
    step, and at this size a second edge would put more than a tenth of the counted pixels there."""
    return (-2.0 * OCCLUDER_Z / (4.0 * W), 1.0e4)


def occluder_rig(H, W, views=2):
    """A target camera at the world origin (turned by a few milliradians) and neighbours to its sides in turn (+x, -x, then half as
    far), so that what one neighbour cannot see of the plane the opposite one can.  The baseline is 7 W / 8 units: at a focal length of
    4 W the rectangle's shadow on the plane is displaced by 4 W x (7 W / 8) / 800 = 7 W^2 / 1600 target pixels (18 at W = 64), and that is
    the width of the band of the plane the target sees and the neighbour does not.  The neighbours stay at the target's height: a
    rectangle that leaves the target's frame at the top cannot be splatted from the target's pixels where a raised neighbour would still
    see it.  The neighbours' images are wider than the target's by 3 W / 4 so that the samples land inside
    -> (K, P, Ks, Ps, (Hs, Ws)) fp64."""
    f = 4.0 * W
    Hs, Ws = H + 2 * (H // 8), W + 3 * (W // 4)
    K, P = intrinsics(f, H, W), pose((0.002, -0.003, 0.001), (0.0, 0.0, 0.0))
    Ks, Ps = [], []
    for v in range(views):
        side = (1.0 if v % 2 == 0 else -1.0) / (1 + v // 2)
        R = rotation(0.001 * (v + 1), -0.002 * side, 0.0015)
        centre = np.array([side * 0.875 * W, 0.0, 0.0])
        Pv = np.eye(4)
        Pv[:3, :3], Pv[:3, 3] = R, -R @ centre
        Ks.append(intrinsics(f, Hs, Ws))
        Ps.append(Pv)
    return K, P, np.stack(Ks), np.stack(Ps), (Hs, Ws)


def _occluder_hit(origin, direction, x_range):
    """Rays origin + l direction (direction [..., 3]) against the rectangle -> (hit, l)."""
    with np.errstate(divide='ignore', invalid='ignore'):
        lam = (OCCLUDER_Z - origin[2]) / direction[..., 2]
    X = origin + lam[..., None] * direction
    hit = (lam > 0) & (X[..., 0] >= x_range[0]) & (X[..., 0] <= x_range[1]) & (X[..., 1] >= OCCLUDER_Y[0]) & (X[..., 1] <= OCCLUDER_Y[1])
    return hit, lam


def render_occluder(K, P, H, W, x_range):
    """The occluder scene seen by the camera (K, P): per ray the nearer of the rectangle and the plane -> (rgb [3, H, W] de-normalised,
    depth [H, W], the world points [H, W, 3], on_occluder [H, W]), fp64."""
    rgb, z = render(K, P, H, W)
    R, t = P[:3, :3], P[:3, 3]
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    rays = np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(K).T
    hit, lam = _occluder_hit(-R.T @ t, rays @ R, x_range)               # (the camera depth along r = K^-1 [x, y, 1] is l itself)
    front = hit & (lam < z)
    z = np.where(front, lam, z)
    X = (z[..., None] * rays - t) @ R
    rgb = np.where(front[None], texture(X + np.asarray(OCCLUDER_SHIFT)), rgb)
    return rgb, z, X, front


def occluder_visibility(X, on_occluder, Ks, Ps, x_range):
    """Closed-form visibility of the world points X [H, W, 3] a target camera sees: the point is visible in view v iff the segment from
    camera v's centre to it misses the rectangle (a point ON the rectangle is visible: nothing lies in front of it) -> visible
    [S, H, W] bool, and edge [S, H, W]: the distance, in pixels of view v, from the point's projection to the outline of the
    rectangle's projection -- the occlusion boundary in that view."""
    corners = np.array([[x_range[0], OCCLUDER_Y[0], OCCLUDER_Z], [x_range[1], OCCLUDER_Y[0], OCCLUDER_Z],
                        [x_range[1], OCCLUDER_Y[1], OCCLUDER_Z], [x_range[0], OCCLUDER_Y[1], OCCLUDER_Z]])
    visible, edge = [], []
    for Kv, Pv in zip(Ks, Ps):
        R, t = Pv[:3, :3], Pv[:3, 3]
        centre = -R.T @ t
        hit, lam = _occluder_hit(centre, X - centre, x_range)
        visible.append(on_occluder | ~(hit & (lam < 1.0)))

        def project(Y):
            q = (Y @ R.T + t) @ Kv.T
            return q[..., :2] / q[..., 2:]
        p, c = project(X), project(corners)
        dist = np.full(X.shape[:2], np.inf)
        for k in range(4):
            a, b = c[k], c[(k + 1) % 4]
            w = np.clip(((p - a) @ (b - a)) / ((b - a) @ (b - a)), 0.0, 1.0)
            dist = np.minimum(dist, np.linalg.norm(p - (a + w[..., None] * (b - a)), axis=-1))
        edge.append(dist)
    return np.stack(visible), np.stack(edge)


def occluder_sample(H=48, W=64, views=2):
    """One sample of the occluder scene as fp32 torch tensors with the keys of plane_sample, and beside them (fp64 numpy) 'on_occluder'
    [H, W], 'visible' [S, H, W] and 'edge' [S, H, W] of occluder_visibility."""
    K, P, Ks, Ps, (Hs, Ws) = occluder_rig(H, W, views)
    xr = occluder_x(W)
    rgb, z, X, front = render_occluder(K, P, H, W, xr)
    srcs = [render_occluder(Ks[v], Ps[v], Hs, Ws, xr)[0] for v in range(views)]
    visible, edge = occluder_visibility(X, front, Ks, Ps, xr)
    b, a = AB
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))                        # noqa: E731
    return {'center': T(normalise(rgb)), 'centers': T(np.concatenate([normalise(s) for s in srcs], 0)), 'K': T(K), 'P': T(P), 'Ks': T(Ks),
            'Ps': T(Ps), 'depth': T(z), 'idepth': T(z.max() / z), 'disp': T(a / z + b), 'abvalue': T(np.array([b, a])),
            'mask': torch.ones(H, W), 'on_occluder': front, 'visible': visible, 'edge': edge}


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
