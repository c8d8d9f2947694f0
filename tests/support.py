"""What the test files share, each stated once: the comparison rules (close, close_elem, within_bound, the ulp helpers), the seeded
inputs, the raw-ABI argument helpers and the model builders.  A plain module (``from tests import support``), no conftest: importing it
needs neither a GPU nor the built library, and everything that touches dualpixelface_amd is imported inside the function that uses it."""
import ctypes

import numpy as np
import torch

DEV = 'cuda'


def ops():
    from dualpixelface_amd import ops
    return ops


def tensor(a):
    """A numpy array as a device tensor; None passes through."""
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=DEV)


def rnd(*shape, seed=0, scale=1.0, dtype=torch.float32):
    """Seeded normal draws on the CPU.  float64 draws are not the widened float32 ones; scale 1.0 multiplies exactly."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=dtype) * scale


# ---- comparison rules
def close(a, b, tol=1e-4, name='', atol=None):
    """max |a - b| <= tol * max(max |b|, 1e-6), in fp64; with `atol` given the limit is atol itself."""
    a = torch.as_tensor(a).detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    scale = max(b.abs().max().item(), 1e-6)
    err = (a - b).abs().max().item()
    lim = atol if atol is not None else tol * scale
    print('%s: max err %.3e / scale %.3e = %.3e (limit %.3e)' % (name, err, scale, err / scale, lim))
    assert err <= lim, '%s: max err %.3e > %.3e (scale %.3e, rel %.3e)' % (name, err, lim, scale, err / scale)


def close_elem(a, b, name='', rtol=1e-4, atol=1e-5):
    """Element-wise bound (rtol 1e-4 / atol 1e-5) for operators without a long reduction: every element has to satisfy
    |a - b| <= atol * rms(b) + rtol * |b|  (rms(b) = 1 for unit-scale data, so small-magnitude elements are held to an absolute 1e-5 instead
    of disappearing under the tensor's maximum as in close())."""
    a = torch.as_tensor(a).detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    rms = max(b.pow(2).mean().sqrt().item(), 1e-30)
    excess = (a - b).abs() - (atol * rms + rtol * b.abs())
    worst = excess.max().item()
    print('%s: worst excess %.3e over atol %.0e x rms %.3e + rtol %.0e' % (name, worst, atol, rms, rtol))
    assert worst <= 0, '%s: %d of %d elements outside rtol %.0e / atol %.0e x rms %.3e (worst excess %.3e)' % (
        name, int((excess > 0).sum()), excess.numel(), rtol, atol, rms, worst)


def within_bound(got, ref, what, p_before=None):
    """The optimiser tests' bound around the fp64 `ref`, per element: 1e-4 * |ref| + 1e-5 * rms(ref), plus one fp32 ulp of `p_before`
    (2^-23 * |p_before|) where an update is compared; prints the worst excess (<= 0 passes)."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    rms = ref.pow(2).mean().sqrt().item()
    lim = 1e-4 * ref.abs() + 1e-5 * rms
    if p_before is not None:
        lim = lim + 2.0 ** -23 * p_before.detach().cpu().double().abs()
    excess = (got - ref).abs() - lim
    worst = excess.max().item()
    print('%s: worst excess %.3e (rms %.3e, %d of %d outside)' % (what, worst, rms, int((excess > 0).sum()), excess.numel()))
    assert worst <= 0, '%s: %d of %d elements outside the bound (worst excess %.3e, rms %.3e)' % (
        what, int((excess > 0).sum()), excess.numel(), worst, rms)


def bits(a):
    """The fp32 bit patterns of an array, for bitwise comparisons that tell -0.0 from 0.0 and one NaN from another."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ulp_of(v):
    """One fp32 ulp of the scalar v."""
    return float(np.spacing(np.float32(abs(v))))


def ulp_of_max(x):
    """One fp32 ulp of the largest magnitude in the array x; 0 for an empty one."""
    return float(np.spacing(np.float32(np.abs(x).max()))) if x.size else 0.0


# ---- arguments of the C ABI, for the tests that call it directly
def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def offset_ptr(t, nbytes):
    return ctypes.c_void_p(t.data_ptr() + nbytes)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- stand-ins around the operator layer
class TwoRankExchange(object):
    """Stands in for distributed.StatExchange on a one-GPU box: plays the other rank of a 2-rank SyncBatchNorm with plain torch math, so
    the local kernels + merge / phase-2 kernels can be checked against full-batch batch norm.  One tensor, or a list per argument for the
    branches of a norm_act_concat: the other rank's slices are packed as the operator packs its own ([2C+1] per branch in the gather,
    [3C+1] in the reduce).  log: every collective appends its name (a list of the caller's, to interleave them with other records)."""
    world_size = 2

    def __init__(self, x1, dz1, mean_g, invstd_g, log=None):
        listed = lambda v: list(v) if isinstance(v, (list, tuple)) else [v]
        self.branches = list(zip(listed(x1), listed(dz1), listed(mean_g), listed(invstd_g)))
        self.log = [] if log is None else log

    @staticmethod
    def _dims(x1):
        return [0] + list(range(2, x1.dim())), [1, -1] + [1] * (x1.dim() - 2), x1.numel() // x1.shape[1]

    def all_gather(self, packed):
        self.log.append('all_gather')
        parts = []
        for x1, _, _, _ in self.branches:
            dims, bshape, count1 = self._dims(x1)
            m1 = x1.mean(dims)
            M2 = ((x1 - m1.view(bshape)) ** 2).sum(dims)
            parts += [torch.stack([m1, M2], 1).reshape(-1), torch.tensor([float(count1)], device=packed.device)]
        other = torch.cat(parts)
        assert other.shape == packed.shape, (other.shape, packed.shape)
        return torch.stack([packed, other.to(packed.dtype)])

    def all_reduce_sum_(self, ws):
        self.log.append('all_reduce_sum_')
        off = 0
        for x1, dz1, mean_g, invstd_g in self.branches:
            dims, bshape, count1 = self._dims(x1)
            xh = (x1 - mean_g.view(bshape)) * invstd_g.view(bshape)
            C = x1.shape[1]
            v = ws[off:off + 3 * C].view(-1, 3)
            v[:, 0] += dz1.sum(dims)
            v[:, 1] += (dz1 * xh).sum(dims)
            ws[off + 3 * C] += float(count1)           # the other rank's element count rides in the slice's last slot
            off += 3 * C + 1
        assert off == ws.numel(), (off, ws.numel())
        return ws


class CallRecorder(object):
    """Stands around the ctypes library of dualpixelface_amd._lib: every dpf_* entry reached through it -- lib().call and the direct
    lib().cdll.NAME(...) alike -- leaves (name, args) in `calls` and then runs.  record_calls() puts one in place."""

    def __init__(self, cdll):
        self.cdll, self.calls = cdll, []

    def __getattr__(self, name):
        fn = getattr(self.cdll, name)
        if not name.startswith('dpf_'):
            return fn

        def recorded(*args):
            self.calls.append((name, args))
            return fn(*args)
        return recorded


def record_calls(monkeypatch):
    """A CallRecorder around the loaded library until the test ends."""
    L = ops().lib()
    rec = CallRecorder(L.cdll)
    monkeypatch.setattr(L, 'cdll', rec)
    return rec


# ---- options and models
def option(config=None, **over):
    """load_option(config, **over): the overrides are merged into the model block before the Option is built."""
    from dualpixelface_amd import load_option
    return load_option(config, **over) if config else load_option(**over)


def option_set(config=None, **attrs):
    """The loaded option with `attrs` set on it afterwards: top-level keys (optim, init_lr, epoch, ...), which option() cannot reach."""
    opt = option(config)
    for k, v in attrs.items():
        setattr(opt, k, v)
    return opt


def build(cls_name, opt, train=True):
    """The plugin class of that name over `opt`, weights by the recipe, on the device (a fresh module is in training mode anyway)."""
    from dualpixelface_amd import plugin as plugins
    from dualpixelface_amd.recipe import fill_by_recipe
    model = getattr(plugins, cls_name)(opt)
    fill_by_recipe(model)
    return model.to(DEV).train(train)


def dpnet(config='train_faceDP_dpnet', **model_over):
    return build('DPNET', option(config, **model_over))


def plugin(optim, cls='STEREODPNET', config=None, **kw):
    return build(cls, option_set(config, optim=optim, **kw))


def batch(B, H, W, seed, **kw):
    """recipe.synthetic_batch on the device."""
    from dualpixelface_amd.recipe import synthetic_batch
    return {k: v.to(DEV) for k, v in synthetic_batch(B, H, W, seed=seed, **kw).items()}


def named(model, flat):
    """A flat arena of the model as {parameter name: CPU copy of its slice}."""
    return {name: flat[off:off + numel].view(shape).detach().cpu().clone() for name, off, numel, shape in model._layout}


def loss_steps(model, batch, k, lr=1e-3, abvalue_only_if_given=False):
    """k train steps -> per step {name: float} of the '*_loss' results.  abvalue_only_if_given: a step may report 'abvalue' only where the
    batch brought one."""
    out = []
    for _ in range(k):
        res = model.train_step(batch, None, lr=lr)
        if abvalue_only_if_given:
            assert 'abvalue' not in res or 'abvalue' in batch
        out.append({key: float(v.detach()) for key, v in res.items() if key.endswith('_loss')})
    return out
