"""A synthetic face scene with everything known, and dual-pixel batches rendered from it on the device (ops.dp_render).

recipe.synthetic_batch draws 'left', 'right' and 'disp' independently: it exercises every kernel and teaches a network nothing.  Here a
batch is a scene -- a far plane with a smooth head-sized ellipsoidal bump and a smaller nose bump, a band-limited texture, the defocus
disparity d = a / z + b of its depth -- and the two half-aperture views the dual-pixel forward model makes of it
(dualpixelface_amd/dp_render.py), so 'disp' is the exact label of the pair.  The batch has the keys, shapes and dtypes of
recipe.synthetic_batch, plus 'center', the all-in-focus view the label is aligned to.  recipe.synthetic_batch is untouched.

The scene is plain numpy; rendering happens once per batch on the device, not in worker processes.
"""
import numpy as np
import torch

from . import dp_render
from .core import reference_key
from .synthetic_refocus import normalise

FOCAL = 5000.0                          # recipe.synthetic_batch's K
Z_FAR = 800.0                           # the far plane
HEAD_HEIGHT, NOSE_HEIGHT = 0.8, 0.25    # how far the head and the nose rise towards the camera, in widths of the head's half axis
WAVES = 32                              # cosines per texture component
MAX_FREQUENCY = 0.9                     # rad / pixel: white noise does not survive the blur, a band-limited texture does


def _bump(xs, ys, cx, cy, ax, ay, height):
    """height (1 - q)^2 inside the ellipse q = ((x - cx) / ax)^2 + ((y - cy) / ay)^2 < 1, zero outside -- C1 at the rim -- and its
    derivatives along x and y."""
    u, v = (xs - cx) / ax, (ys - cy) / ay
    q = u * u + v * v
    inside = q < 1.0
    g = np.where(inside, 1.0 - q, 0.0)
    return height * g * g, -4.0 * height * g * u / ax, -4.0 * height * g * v / ay, inside


def _texture(rng, xs, ys):
    """Encoded RGB [3, H, W] in [0.02, 0.98]: a shared sum of WAVES cosines plus a weaker one per channel, frequencies in
    [0.15, MAX_FREQUENCY] rad / pixel in seeded directions."""
    def waves():
        k = rng.uniform(0.15, MAX_FREQUENCY, WAVES)
        th, ph = rng.uniform(0.0, 2.0 * np.pi, WAVES), rng.uniform(0.0, 2.0 * np.pi, WAVES)
        s = np.zeros_like(xs)
        for i in range(WAVES):
            s += np.cos(k[i] * np.cos(th[i]) * xs + k[i] * np.sin(th[i]) * ys + ph[i])
        return s / np.sqrt(WAVES / 2.0)                                   # unit variance
    shared = waves()
    return np.clip(np.stack([0.5 + 0.2 * shared + 0.07 * waves() for _ in range(3)]), 0.02, 0.98)


def face_scene(H, W, seed=0, d_range=(-1.5, 2.0)):
    """One sample, fp64 unless said otherwise -> dict of
        'z' [H, W]: the depth; 'K' [3, 3]; 'abvalue' [2] = [b, a], solved so that d = a / z + b is d_range[0] on the far plane and
        d_range[1] at the nearest point (a > 0: larger d is nearer); 'disp' [H, W] float32: that d; 'normal' [3, H, W]: the analytic unit
        normals in camera space, towards the camera (n_z < 0); 'mask' [H, W] float32: the head; 'encoded' [3, H, W] in [0.02, 0.98]: the
        texture; 'center' [3, H, W] float32: encoded, normalised as the data path does."""
    rng = np.random.RandomState((7000 + int(seed)) % 2 ** 32)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    cx, cy = W * (0.5 + 0.06 * rng.uniform(-1, 1)), H * (0.5 + 0.06 * rng.uniform(-1, 1))
    ax, ay = W * 0.27 * (1 + 0.1 * rng.uniform(-1, 1)), H * 0.42 * (1 + 0.1 * rng.uniform(-1, 1))
    unit = ax * Z_FAR / FOCAL                                            # the head's half axis in the units of z
    head, hx, hy, inside = _bump(xs, ys, cx, cy, ax, ay, HEAD_HEIGHT * unit)
    nose, nx, ny, _ = _bump(xs, ys, cx, cy + 0.1 * ay, 0.22 * ax, 0.3 * ay, NOSE_HEIGHT * unit)
    z = Z_FAR - head - nose
    zx, zy = -(hx + nx), -(hy + ny)
    K = np.array([[FOCAL, 0.0, W / 2.0], [0.0, FOCAL, H / 2.0], [0.0, 0.0, 1.0]])
    # the surface P(x, y) = z K^-1 [x, y, 1]; its normal is the cross product of the two tangents, turned towards the camera
    rx, ry = (xs - K[0, 2]) / FOCAL, (ys - K[1, 2]) / FOCAL
    tx = np.stack([z / FOCAL + rx * zx, ry * zx, zx])
    ty = np.stack([rx * zy, z / FOCAL + ry * zy, zy])
    n = np.cross(ty, tx, axis=0)
    n = n / np.linalg.norm(n, axis=0, keepdims=True)
    n = np.where(n[2:3] > 0, -n, n)
    z_near = z.min()
    a = (d_range[1] - d_range[0]) / (1.0 / z_near - 1.0 / Z_FAR)
    b = d_range[0] - a / Z_FAR
    enc = _texture(rng, xs, ys)
    return {'z': z, 'K': K, 'abvalue': np.array([b, a]), 'disp': (a / z + b).astype(np.float32), 'normal': n,
            'mask': inside.astype(np.float32), 'encoded': enc, 'center': normalise(enc)}


def _scene_tensors(H, W, scene_seed, d_range):
    """face_scene as fp32 torch tensors [1, ...] on the CPU, under the keys of recipe.synthetic_batch (without the pair) plus 'center'."""
    s = face_scene(H, W, scene_seed, d_range)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))[None]                  # noqa: E731
    return {'center': T(s['center']), 'disp': T(s['disp']), 'depth': T(s['z']), 'idepth': T(s['z'].max() / s['z']), 'mask': T(s['mask']),
            'normal': T(s['normal']), 'K': T(s['K']), 'abvalue': T(s['abvalue'])}


def _rendered(scene_seeds, H, W, option, device):
    """The scenes of those seeds as one batch on `device`, with the pair rendered there."""
    s = dp_render.settings(option)
    ones = [_scene_tensors(H, W, seed, s.d_range) for seed in scene_seeds]
    scene = {k: torch.cat([o[k] for o in ones]).to(device) for k in ones[0]}
    out = dp_render.render(option, scene['center'], scene['disp'])
    ref = reference_key(option)
    pair = {ref: out['reference'], 'left' if ref == 'right' else 'right': out['target']}
    batch = {'left': pair['left'], 'right': pair['right']}
    batch.update((k, scene[k]) for k in ('disp', 'depth', 'idepth', 'mask', 'normal', 'K', 'abvalue', 'center'))
    return batch


def rendered_batch(B, H, W, seed=0, option=None, device='cuda'):
    """A batch of face scenes (seeds seed 100003 + 0, 1, ...) on `device` with its dual-pixel pair rendered there under option.dp_render
    (None: the defaults): exactly the keys, shapes and dtypes of recipe.synthetic_batch, plus 'center'.  The rendered reference view goes
    under core.reference_key(option), the target view under the other key."""
    return _rendered([seed * 100003 + i for i in range(B)], H, W, option, device)


class RenderedLoader(object):
    """Iterable of device-resident rendered batches, the way facedp.FaceDPBatcher hands them out: `length` scenes per epoch in batches of
    `batch_size` (the last one may be smaller), reshuffled per epoch by an own generator under `shuffle`.  A scene is a function of
    (seed, index), so an epoch repeats."""

    def __init__(self, length, height, width, batch_size, option=None, shuffle=False, seed=0, device='cuda', sampler=None):
        self.length, self.height, self.width, self.batch_size = int(length), int(height), int(width), int(batch_size)
        self.option, self.shuffle, self.seed, self.device, self.sampler, self.epoch = option, bool(shuffle), int(seed), device, sampler, 0
        self.dataset = range(self.length)                               # what a DistributedSampler needs: a length
        self.num_workers, self.pin_memory, self.collate_fn, self.drop_last = 0, False, None, False

    def with_sampler(self, sampler):
        return RenderedLoader(self.length, self.height, self.width, self.batch_size, self.option, self.shuffle, self.seed, self.device, sampler)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def _order(self):
        if self.sampler is not None:
            return list(iter(self.sampler))
        if not self.shuffle:
            return list(range(self.length))
        g = torch.Generator()
        g.manual_seed(self.seed + self.epoch)
        return torch.randperm(self.length, generator=g).tolist()

    def __len__(self):
        n = len(self.sampler) if self.sampler is not None else self.length
        return (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        order = self._order()
        for at in range(0, len(order), self.batch_size):
            yield _rendered([self.seed * 100003 + int(i) for i in order[at:at + self.batch_size]], self.height, self.width, self.option,
                            self.device)


def rendered_loader(length, height, width, batch_size, option=None, shuffle=False, seed=0, device='cuda'):
    return RenderedLoader(length, height, width, batch_size, option, shuffle, seed, device)
