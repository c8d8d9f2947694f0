"""fp64 closed-form restatement of the normalisation + activation operator (dualpixelface_amd/csrc/norm_act.hip), the yardstick of
test_norm_act_host.py and test_gpu_norm_act.py.  Inputs are taken as given (float32 values widened to float64), everything after that is
float64 on the CPU, without autograd: the forward, the running-statistics update and every gradient are written out.

    y = act(norm(x) * w[c % wmod] + b[c % wmod] + res) + res2          x, res, res2, y: [N, C, S]

mode 0: no normalisation (w and b are not read)      mode 1: batch norm, batch statistics (training)
mode 2: batch norm, running statistics (eval)        mode 3: instance norm (one statistic per sample and channel; w, b per channel)
"""
import torch

ACT_NONE, ACT_RELU, ACT_PRELU, ACT_LEAKY, ACT_SIGMOID = 0, 1, 2, 3, 4          # ops.ACT_*
EPS, MOMENTUM = 1e-5, 0.1                                                       # ops.BN_EPS, ops.BN_MOMENTUM


def _d(t):
    return None if t is None else torch.as_tensor(t).detach().cpu().double()


def norm_act(x, weight=None, bias=None, slope=None, res=None, res2=None, running_mean=None, running_var=None, mode=0, act=ACT_NONE,
             slope_const=0.0, go=None):
    """-> dict of float64 tensors: y and z (the activation's argument); running_mean / running_var after the call (mode 1, else as
    given); and with the upstream gradient `go`: dx, dw, db (None in mode 0 or without the parameter), dslope (PReLU), dres, dres2 (None
    without the operand)."""
    x, weight, bias, slope, res, res2, go = [_d(t) for t in (x, weight, bias, slope, res, res2, go)]
    rm, rv = _d(running_mean), _d(running_var)
    shape = x.shape
    N, C = shape[0], shape[1]
    x = x.reshape(N, C, -1)
    flat = lambda t: None if t is None else t.reshape(N, C, -1)
    res, res2, go = flat(res), flat(res2), flat(go)
    dims = {1: (0, 2), 3: (2,)}.get(mode)                         # what one statistic averages over
    out = {}
    if mode == 0:
        xh, invstd, g, be = x, None, None, None
    else:
        if mode == 2:
            mean, var = rm.view(1, C, 1), rv.view(1, C, 1)
        else:
            mean = x.mean(dims, keepdim=True)
            var = ((x - mean) ** 2).mean(dims, keepdim=True)
            if mode == 1 and rm is not None:
                n = N * x.shape[2]
                rm = (1.0 - MOMENTUM) * rm + MOMENTUM * mean.reshape(C)
                rv = (1.0 - MOMENTUM) * rv + MOMENTUM * var.reshape(C) * (n / (n - 1.0) if n > 1 else 1.0)
        invstd = 1.0 / torch.sqrt(var + EPS)
        xh = (x - mean) * invstd
        g = weight.view(1, C, 1) if weight is not None else None
        be = bias.view(1, C, 1) if bias is not None else None
    z = xh
    if g is not None:
        z = z * g
    if be is not None:
        z = z + be
    if res is not None:
        z = z + res
    a = float(slope.reshape(-1)[0]) if act == ACT_PRELU else float(slope_const)
    if act == ACT_RELU:
        y, dact = z.clamp(min=0.0), (z > 0).double()
    elif act in (ACT_PRELU, ACT_LEAKY):
        pos = z > 0
        y, dact = torch.where(pos, z, z * a), torch.where(pos, torch.ones_like(z), torch.full_like(z, a))
    elif act == ACT_SIGMOID:
        y = torch.sigmoid(z)
        dact = y * (1.0 - y)
    else:
        assert act == ACT_NONE
        y, dact = z, None
    out['z'] = z.reshape(shape)                                   # the activation's argument
    out['y'] = (y + res2 if res2 is not None else y).reshape(shape)
    out['running_mean'], out['running_var'] = rm, rv
    if go is None:
        return out
    dz = go if dact is None else go * dact
    out['dres2'] = go.reshape(shape) if res2 is not None else None
    out['dres'] = dz.reshape(shape) if res is not None else None
    out['dslope'] = (go * z * (z <= 0)).sum().reshape(1) if act == ACT_PRELU else None
    if mode == 0:
        out['dx'], out['dw'], out['db'] = dz.reshape(shape), None, None
        return out
    out['db'] = dz.sum((0, 2)) if bias is not None else None
    out['dw'] = (dz * xh).sum((0, 2)) if weight is not None else None
    dxh = dz * g if g is not None else dz
    if mode == 2:
        dx = dxh * invstd
    else:
        dx = invstd * (dxh - dxh.mean(dims, keepdim=True) - xh * (dxh * xh).mean(dims, keepdim=True))
    out['dx'] = dx.reshape(shape)
    return out


def channel_errors(a, b):
    """-> (err, scale) per channel, float64 [C]: max |a - b| and max |b| over everything but dim 1 (a [C] vector: per element)."""
    a, b = _d(a), _d(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.dim() == 1:
        return (a - b).abs(), b.abs()
    C = a.shape[1]
    err = (a - b).abs().transpose(0, 1).reshape(C, -1).amax(1)
    return err, b.abs().transpose(0, 1).reshape(C, -1).amax(1)


def close_channels(a, b, tol, name='', bars=None):
    """test_gpu_ops.py::close's rule on every channel slice [:, c] of its own (on every element of a per-channel vector): a large
    channel cannot hide a wrong small one.  bars: a per-channel bound that replaces `tol` where it is the larger.  -> err / scale [C]."""
    err, scale = channel_errors(a, b)
    scale = scale.clamp(min=1e-6)
    bound = torch.full_like(err, tol)
    if bars is not None:
        bound = torch.maximum(bound, torch.as_tensor(bars, dtype=torch.float64))
    rel = err / scale
    print('%s: err / scale per channel, worst %.2e, worst over its bound %.2e: %s (bound %s)' % (
        name, rel.max().item(), (rel / bound).max().item(), ' '.join('%.2e' % v for v in rel.tolist()[:16]),
        ' '.join('%.1e' % v for v in bound.tolist()[:16])))
    bad = (rel > bound).nonzero().reshape(-1).tolist()
    assert not bad, '%s: channels %s outside the bound: err / scale %s vs %s' % (
        name, bad[:8], ['%.3e' % rel[c].item() for c in bad[:8]], ['%.1e' % bound[c].item() for c in bad[:8]])
    return rel
