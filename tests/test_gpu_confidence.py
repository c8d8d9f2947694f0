"""Confidence maps on the GPU (run with ``-m gpu``): csrc/head_confidence.hip through ops.head_confidence and ops.confidence_curve, and the
``confidence`` block through the StereoDPNet evaluation forward, against the restatements of tests/confidence_cpu.py.
The cases are the geometries of tests/unimodal_cpu.py (the table in tests/test_gpu_unimodal.py): the fast and the general path, partial
tiles, clamped rows, and the structural ties u_0 == u_1 of the half-pixel geometry; `fitted` serves the curve under target_ab.

Exact: `lstar` and the bad map equal the fp32 numpy restatement.  A pixel whose two largest fp32 u_l differ by more than 0 and less than
8 x 2^-24 x max |u| may be left out there and in the `mass` and `modal` comparisons (confidence_cpu.near_tie; at most 1 % of a case).

Bounded: each plane against the fp64 restatement within 2 x (the fp32 restatement's own worst deviation from fp64, computed here on the
same input) + the allowance of `_allowance` for the device's exp, log and sqrt.  Independently: the same planes formed in torch from the
probability volume of ops.softargmin_heads, held to that head's own bound (1e-5 of the largest value, tests/test_gpu_ops.py).
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import confidence_cpu as cc
from tests import support
from tests import unimodal_cpu as uc
from tests.support import DEV, bits, tensor

pytestmark = pytest.mark.gpu

GEOMETRIES = ['general', 'half-pixel', 'multi-tile', 'one-tile', 'thin']
U = 2.0 ** -24
FLOATS = cc.NAMES
ALL = FLOATS + ('lstar',)


def _call(c, window=1, want=ALL, logits=None):
    """ops.head_confidence on a case -> {name: numpy array}."""
    ks = [tensor(k) for k in (c['logits'] if logits is None else logits)]
    out = support.ops().head_confidence(ks, c['disp'], scale=c['scale'], align_corners=c['align'], window=window, want=want)
    B, n, H, W = ks[0].shape[0], len(ks), c['scale'] * ks[0].shape[3], c['scale'] * ks[0].shape[4]
    assert set(out) == set(want)
    for name, t in out.items():
        assert t.shape == (B, n, H, W) and t.dtype == (torch.int32 if name == 'lstar' else torch.float32) and not t.requires_grad, name
    return {name: t.cpu().numpy() for name, t in out.items()}


def _bad_of(got):
    bad = np.isnan(got['modal'])
    assert np.array_equal(bad, np.isnan(got['spread']))
    for name in ('peak', 'entropy', 'mass'):
        assert not got[name][bad].any(), name
    return bad


def _refs(name, window=1):
    c = uc.case(name)['case']
    r32 = cc.planes(c['logits'], c['disp'], c['scale'], c['align'], window)
    r64 = cc.planes(c['logits'], c['disp'], c['scale'], c['align'], window, np.float64, lstar=r32['lstar'])
    return c, r32, r64


def _allowance(c, r64):
    """What the device's exp, log and sqrt may add to each plane beyond the numpy restatement, which evaluates the same operations in the
    same order with numpy's own functions.  In units of u = 2^-24, as tests/test_gpu_unimodal.py derives its own:

      * one exponential against numpy's: (|x| + 12) u relative (the rounded product x log2(e), v_exp_f32 at 2 ulp, numpy at 4 ulp).
      * S = sum_l exp(x_l), x_l <= 0, one x_l = 0, so S >= 1: |dS| <= u (12 S + L / e) and dS / S <= A u with A = 12 + L / e.
      * p_l = e_l / S: |dp_l| <= eps p_l with eps = (R + 12 + A) u, R the spread of the head's logits (|x_l| <= R: the upsample is a
        convex combination of them).

    From these, with dmax = max |d_l| and range = d_{L-1} - d_0:

        peak    1 / S <= 1                                   A u
        mass    a sum of p_l, <= 1                           eps
        entropy Hent = log S - sum p_l x_l: dS / S, the two logarithms at 6 ulp = 12 u of log S <= log L, sum |dp_l| |x_l| <= eps R;
                divided by log L, and 12 u more for logf(L) against numpy's      (A u + eps R) / log L + 24 u
        modal   N / M with |dN| <= eps dmax M and |dM| <= eps M                  2 eps dmax
        var     sum p_l (d_l - mu)^2 with |dmu| <= eps dmax                      eps range (range + 2 dmax)
        spread  sqrt(var), both square roots correctly rounded (1 ulp = 2 u allowed): per pixel allowance(var) / (2 spread) + 2 u spread;
                where var is below allowance(var) the square root is ill-conditioned and var is compared instead."""
    L = len(c['disp'])
    d = np.asarray(c['disp'], dtype=np.float64)
    R = max(float(k.max()) - float(k.min()) for k in c['logits'])
    A = 12 + L / math.e
    eps = (R + 12 + A) * U
    dmax, rng = float(np.abs(d).max()), float(d[-1] - d[0])
    var = eps * rng * (rng + 2 * dmax)
    with np.errstate(all='ignore'):
        spread = var / (2 * r64['spread']) + 2 * U * r64['spread']
    return dict(peak=A * U, mass=eps, entropy=(A * U + eps * R) / math.log(L) + 24 * U, modal=2 * eps * dmax, var=var, spread=spread), R


# ---- 1. lstar and the bad map, exactly
@pytest.mark.parametrize('name', GEOMETRIES)
def test_lstar_and_the_bad_map_equal_the_fp32_restatement(name):
    c, r32, _ = _refs(name)
    got = _call(c)
    near = cc.near_tie(r32)
    tied = int((r32['gap'] == 0).sum())
    print('lstar %s: %d of %d pixels left out as near ties, %d exact ties, %d differ among the left-out' % (
        name, near.sum(), near.size, tied, (got['lstar'] != r32['lstar'])[near].sum()))
    assert near.sum() <= 0.01 * near.size
    assert np.array_equal(got['lstar'][~near], r32['lstar'][~near])
    assert np.array_equal(_bad_of(got), r32['bad']) and not r32['bad'].any()
    if name == 'half-pixel':
        # u_0 == u_1 at the low end (and u_{L-2} == u_{L-1} at the high one): the smaller index
        assert tied > 0 and np.isin(got['lstar'][r32['gap'] == 0], (0, len(c['disp']) - 2)).all() and (got['lstar'][r32['gap'] == 0] == 0).any()


# ---- 2. the five planes against fp64
@pytest.mark.parametrize('name', GEOMETRIES)
def test_the_planes_against_the_fp64_restatement(name):
    c, r32, r64 = _refs(name)
    got = _call(c)
    allow, R = _allowance(c, r64)
    keep = ~cc.near_tie(r32)
    for key in FLOATS:
        sel = keep if key in ('mass', 'modal') else np.ones_like(keep)
        if key == 'spread':
            small = r64['var'] < allow['var']
            gvar = got['spread'].astype(np.float64) ** 2                       # (exact in fp64: the device's var up to its square root's ulp)
            own = float(np.abs(r32['var'] - r64['var'])[small].max()) if small.any() else 0.0
            assert (np.abs(gvar - r64['var'])[small] <= 2 * own + 2 * allow['var']).all()
            sel = ~small
            print('planes %s: var compared instead of spread at %d pixels' % (name, small.sum()))
        own = float(np.abs(r32[key].astype(np.float64) - r64[key])[sel].max())
        err = np.abs(got[key].astype(np.float64) - r64[key])
        bar = 2 * own + (allow[key][sel] if key == 'spread' else allow[key])
        print('planes %s %s: max |device - fp64| %.3e, fp32 restatement %.3e, allowance %.3e (logit spread %.2f), bits equal to fp32 at %d of %d'
              % (name, key, err[sel].max(), own, np.max(bar) - 2 * own, R, (bits(got[key]) == bits(r32[key])).sum(), err.size))
        assert np.isfinite(got[key]).all() and (err[sel] <= bar).all(), key
    for key in ('peak', 'entropy', 'mass'):
        assert (got[key] >= 0).all() and (got[key] <= 1).all()
    assert (got['spread'] >= 0).all()


# ---- 3. the torch formulation on the probability volume
def _torch_planes(prob, disp, r):
    """[B, n, L, H, W] fp32 on the device -> the five planes, mu and lstar (the smallest index of the maximum), with 0 log 0 = 0."""
    L = prob.shape[2]
    d = torch.tensor(disp, dtype=torch.float32, device=prob.device).view(1, 1, L, 1, 1)
    idx = torch.arange(L, device=prob.device).view(1, 1, L, 1, 1)
    peak = prob.amax(2)
    lstar = torch.where(prob == peak.unsqueeze(2), idx, L).amin(2)
    entropy = (1 + torch.xlogy(prob, prob).sum(2) / math.log(L)).clamp(0, 1)
    mu = (prob * d).sum(2)
    var = (prob * (d - mu.unsqueeze(2)) ** 2).sum(2)
    inside = ((idx - lstar.unsqueeze(2)).abs() <= r).to(prob.dtype)
    M = (prob * inside).sum(2)
    modal = (prob * inside * d).sum(2) / M
    return dict(peak=peak, entropy=entropy, mass=M.clamp(max=1), spread=var.sqrt(), modal=modal, mu=mu, lstar=lstar)


@pytest.mark.parametrize('name', GEOMETRIES)
def test_the_planes_against_torch_on_the_probability_volume(name):
    c, r32, _ = _refs(name)
    ops = support.ops()
    ks = [tensor(k) for k in c['logits']]
    _, pred, prob = ops.softargmin_heads(ks, c['disp'], c['scale'], c['align'])
    want = {k: v.cpu().numpy() for k, v in _torch_planes(prob, c['disp'], 1).items()}
    got = _call(c)
    keep = ~cc.near_tie(r32)
    assert np.array_equal(got['lstar'][keep], want['lstar'][keep])
    for key in FLOATS:
        a, b = (got[key][keep], want[key][keep]) if key in ('mass', 'modal') else (got[key], want[key])
        support.close(a, b, 1e-5, '%s %s against torch on prob' % (name, key))
    whole = _call(c, window=32, want=('modal', 'mass'))                        # the whole distribution: modal is mu / M, M = 1 within rounding
    support.close(whole['modal'], pred.cpu().numpy(), 1e-5, '%s mu against the soft-argmin' % name)
    support.close(whole['modal'], want['mu'], 1e-5, '%s mu against torch on prob' % name)


# ---- 4. closed forms on the device
@pytest.mark.parametrize('r', [0, 1, 2, 32])
@pytest.mark.parametrize('name', ['general', 'half-pixel', 'multi-tile'])
def test_zero_logits_give_the_uniform_distribution(name, r):
    c = uc.case(name)['case']
    got = _call(c, window=r, logits=[np.zeros_like(k) for k in c['logits']])
    d = np.asarray(c['disp'], dtype=np.float32).astype(np.float64)
    L, k = len(d), min(r, len(d) - 1) + 1
    tol = 4 * L * U * np.abs(d).max()
    assert not got['lstar'].any() and (got['peak'] == np.float32(1) / np.float32(L)).all() and (got['entropy'] == 0).all()
    assert np.abs(got['mass'] - k / L).max() <= L * U
    assert np.abs(got['modal'] - d[:k].mean()).max() <= tol and np.abs(got['spread'] - d.std()).max() <= tol


@pytest.mark.parametrize('name', ['general', 'multi-tile'])
def test_peaked_logits_give_confident_finite_planes(name):
    """Logits scaled by 20.  Everything stays finite and inside [0, 1].  Where the two largest u_l are g >= 12 apart (from the fp32
    restatement), the rest of the distribution holds delta <= (L - 1) exp(-12) < 1.91e-4 (L <= 32), so
        peak    = 1 - delta                                             > 0.9998
        Hent   <= -log(1 - delta) + delta log((L - 1) / delta)          < 2.5e-3, entropy > 1 - 2.5e-3 / log 16 > 0.999
        var    <= delta range^2,  spread <= sqrt(1.91e-4) range         < 0.0139 range
        modal   lies within delta range of d_{l*}
    each with room for the fp32 rounding measured in test 2 (below 2e-6)."""
    c = uc.case(name)['case']
    logits = [k * np.float32(20) for k in c['logits']]
    got = _call(c, logits=logits)
    r32 = cc.planes(logits, c['disp'], c['scale'], c['align'], 1)
    for key in FLOATS:
        assert np.isfinite(got[key]).all(), key
    for key in ('peak', 'entropy', 'mass'):
        assert (got[key] >= 0).all() and (got[key] <= 1).all(), key
    assert (got['spread'] >= 0).all() and np.array_equal(got['lstar'], r32['lstar'])
    sure = r32['gap'] >= 12
    d = np.asarray(c['disp'], dtype=np.float32)
    rng = float(d[-1] - d[0])
    print('peaked %s: %d of %d pixels with a gap >= 12; there min peak %.6f, min entropy %.6f, max spread %.3e; median peak overall %.4f'
          % (name, sure.sum(), sure.size, got['peak'][sure].min(), got['entropy'][sure].min(), got['spread'][sure].max(), np.median(got['peak'])))
    assert sure.sum() >= 30
    assert (got['peak'][sure] > 0.9998).all() and (got['entropy'][sure] > 0.999).all() and (got['mass'][sure] >= got['peak'][sure]).all()
    assert (got['spread'][sure] < 0.0139 * rng).all() and (np.abs(got['modal'][sure] - d[got['lstar'][sure]]) <= 1.91e-4 * rng + 1e-5).all()


# ---- 5. bad pixels
@pytest.mark.parametrize('name', ['general', 'multi-tile'])
def test_non_finite_logits_make_bad_pixels_and_touch_nothing_else(name):
    c = uc.case(name)['case']
    clean = _call(c)
    logits = [k.copy() for k in c['logits']]
    D, h, w = logits[0].shape[2:]
    logits[0][0, 0, 1, 0, 0] = np.nan
    logits[0][0, 0, D - 1, h - 1, w - 1] = np.inf
    logits[-1][-1, 0, 2, h // 2, w // 2] = -np.inf
    r32 = cc.planes(logits, c['disp'], c['scale'], c['align'], 1)
    got = _call(c, logits=logits)
    bad = _bad_of(got)
    print('bad %s: %d of %d pixels' % (name, bad.sum(), bad.size))
    assert np.array_equal(bad, r32['bad']) and 0 < bad.sum() < bad.size
    assert np.array_equal(got['lstar'][~bad], clean['lstar'][~bad])
    for key in FLOATS:
        assert np.array_equal(bits(got[key])[~bad], bits(clean[key])[~bad]), key


# ---- 6. output handling
def _abi(c, **over):
    """The arguments of dpf_head_confidence for a case, all planes given -> (list, the tensors that keep them alive)."""
    from dualpixelface_amd import ops
    ks = [tensor(k) for k in c['logits']]
    B, _, D, h, w = ks[0].shape
    s = c['scale']
    planes = [torch.empty((B, len(ks), s * h, s * w), dtype=torch.float32, device=DEV) for _ in range(5)]
    planes.append(torch.empty((B, len(ks), s * h, s * w), dtype=torch.int32, device=DEV))
    a = dict(logits=ops._host_ptrs(ks), B=B, n=len(ks), D=D, h=h, w=w, L=s * D, H=s * h, W=s * w, align=int(c['align']),
             disp=ops._host_floats(c['disp']), window=1)
    a.update(over)
    return list(a.values()) + [support.ptr(t) for t in planes] + [support.stream()], (ks, planes)


def test_one_plane_alone_equals_that_plane_of_the_whole_call_and_calls_repeat():
    for name in ('multi-tile', 'general'):
        c = uc.case(name)['case']
        whole, again = _call(c), _call(c)
        for key in ALL:
            assert np.array_equal(bits(whole[key]) if key != 'lstar' else whole[key], bits(again[key]) if key != 'lstar' else again[key]), key
            alone = _call(c, want=(key,))
            assert list(alone) == [key]
            assert np.array_equal(alone[key].view(np.uint32), whole[key].view(np.uint32)), key
    from dualpixelface_amd._lib import DpfError
    c = uc.case('one-tile')['case']
    ks = [tensor(k) for k in c['logits']]
    ops = support.ops()
    for kw, match in ((dict(want=()), 'want'), (dict(want=('mu',)), 'want'), (dict(window=33), 'window'), (dict(window=-1), 'window'),
                      (dict(window=1.5), 'window'), (dict(scale=2), 'disp_values')):
        with pytest.raises(DpfError, match=match):
            ops.head_confidence(ks, c['disp'], **kw)
    with pytest.raises(DpfError, match='ascending'):
        ops.head_confidence(ks, c['disp'][::-1])
    with pytest.raises(DpfError, match='does not match'):
        ops.head_confidence(ks + [ks[0][..., :2]], c['disp'])
    assert isinstance(ops.head_confidence(ks, c['disp'], want='peak')['peak'], torch.Tensor)


def test_abi_refusals_launch_nothing():
    from dualpixelface_amd import ops
    from dualpixelface_amd._lib import lib
    c = uc.case('one-tile')['case']
    inv, uns = -1, -3
    fn = lib().cdll.dpf_head_confidence
    args, keep = _abi(c)
    for t in keep[1]:
        t.zero_()
    assert fn(*args) == 0
    torch.cuda.synchronize()
    assert all(bool(t.any()) for t in keep[1][:5])
    for t in keep[1]:
        t.fill_(7)

    def refused(code, planes=None, **over):
        a, k = _abi(c, **over)
        a[12:18] = [support.ptr(t) for t in keep[1]] if planes is None else planes
        assert fn(*a) == code, (over, planes)

    refused(inv, logits=None)
    refused(inv, disp=None)
    refused(inv, planes=[None] * 6)                                              # no output at all
    refused(inv, n=0)
    refused(inv, n=9)
    refused(inv, window=-1)
    refused(inv, window=33)
    for key in ('B', 'D', 'h', 'w', 'L', 'H', 'W'):
        refused(inv, **{key: 0})
    refused(inv, disp=ops._host_floats(c['disp'][::-1]))                         # not ascending
    refused(inv, disp=ops._host_floats([float('nan')] + list(c['disp'][1:])))
    refused(inv, logits=(ctypes.c_void_p * 1)(None))
    refused(uns, D=9, L=36)                                                      # D > 8
    refused(uns, D=16, L=64, H=4 * args[4], W=4 * args[5])                       # D > 8 and L > 32
    refused(uns, L=64)                                                           # L > 32
    refused(uns, D=1, L=1, H=args[4], W=args[5])                                 # L < 2
    refused(uns, L=28)                                                           # no multiple of D
    refused(uns, H=args[7] + 1)
    refused(uns, W=args[8] + 4)
    refused(uns, B=65536)                                                        # B n > 65535
    refused(uns, D=1, L=2, h=1 << 23, H=1 << 24, w=1, W=2)                       # beyond 65535 tiles of 8 rows
    refused(uns, D=1, L=2, h=1, H=2, w=1 << 24, W=1 << 25)                       # W > 2^24
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in keep[1])                            # nothing was launched
    for one in range(6):                                                         # any single plane is enough
        a, k = _abi(c)
        a[12:18] = [support.ptr(keep[1][i]) if i == one else None for i in range(6)]
        assert fn(*a) == 0
    q = lib().cdll.dpf_confidence_curve_workspace_bytes
    assert q(1, 8, 12, 16) == 1 * 16 * 2 * 8 and q(2, 64, 65, 64) == 2 * 3 * 64 * 2 * 8
    for shape in ((0, 8, 12, 16), (1, 0, 12, 16), (1, 8, 0, 16), (1, 8, 12, 0), (1, 8, 12, 65), (65536, 8, 12, 16), (1, 1 << 16, 1 << 15, 16)):
        assert q(*shape) == -1, shape


# ---- 7. the curve
def _curve_case(ab=True):
    ref = uc.case('fitted')
    c = ref['case']
    rng = np.random.RandomState(7)
    B, H, W = c['target'].shape
    conf = rng.uniform(0, 1, (B, 3, H, W)).astype(np.float32)
    pred = np.stack([ref['r32']['expect'][:, 0]] * 3, 1) + rng.uniform(-1, 1, (B, 3, H, W)).astype(np.float32)
    flat = np.argwhere(c['mask'] > 0)
    for (b, y, x), v in zip(flat[:5], (1.0, 0.0, np.nan, np.inf, 0.999999)):
        conf[b, 0, y, x] = v
    pred[tuple(flat[5])[0], 0, flat[5][1], flat[5][2]] = np.nan
    pred[tuple(flat[6])[0], 0, flat[6][1], flat[6][2]] = -np.inf
    target, tab = (c['target'], c['ab']) if ab else (ref['r32']['t'], None)
    return dict(conf=conf, pred=pred.astype(np.float32), target=target, mask=c['mask'], ab=tab, special=flat[:7])


def _curve(k, bins=16, into=None, head=0, copy=False, mask=True):
    ops = support.ops()
    conf, pred = tensor(k['conf'])[:, head], tensor(k['pred'])[:, head]
    if copy:
        conf, pred = conf.contiguous(), pred.contiguous()
    else:
        assert not conf.is_contiguous()
    out = ops.confidence_curve(conf, pred, tensor(k['target']), mask=tensor(k['mask']) if mask else None, target_ab=tensor(k['ab']), bins=bins,
                               into=into)
    assert out.shape == (bins, 2) and out.dtype == torch.float64 and (into is None or out is into)
    return out


def _check_curve(table, k, bins, head=0, mask=True):
    want, ok, err, which = cc.curve(k['conf'][:, head], k['pred'][:, head], k['target'], k['mask'] if mask else None, k['ab'], bins)
    got = table.cpu().numpy()
    assert np.array_equal(got[:, 0], want[:, 0]) and got[:, 0].sum() == ok.sum()
    tol = want[:, 0] * 2.0 ** -53 * want[:, 1] + U * want[:, 1]           # fp64 summation order; one fp32 rounding of each |pred - t|
    print('curve bins %d: %d pixels counted, max |sum - fp64| %.3e (limit %.3e)' % (bins, ok.sum(), np.abs(got[:, 1] - want[:, 1]).max(), tol.max()))
    assert (np.abs(got[:, 1] - want[:, 1]) <= tol).all()
    return want, ok, which


@pytest.mark.parametrize('ab', [True, False], ids=['target_ab', 'disp'])
@pytest.mark.parametrize('bins', [1, 16, 64])
def test_the_curve_against_the_fp64_restatement(bins, ab):
    k = _curve_case(ab)
    first = _curve(k, bins)
    want, ok, which = _check_curve(first, k, bins)
    assert torch.equal(first, _curve(k, bins))                                 # the same bits on every call
    assert torch.equal(first, _curve(k, bins, copy=True))                      # the strided head-0 view against a contiguous copy
    (b0, y0, x0), (b1, y1, x1) = k['special'][0], k['special'][1]
    assert which[b0, y0, x0] == bins - 1 and which[b1, y1, x1] == 0          # conf = 1.0 lands in the last bin
    for b, y, x in k['special'][2:4].tolist() + k['special'][5:7].tolist():    # non-finite conf or pred
        assert not ok[b, y, x]
    assert 0 < ok.sum() < (k['mask'] > 0).sum()
    if bins > 1:
        assert (want[:, 0] > 0).sum() > 1
    other = _curve(k, bins, head=2)                                            # another head of the same tensors
    _check_curve(other, k, bins, head=2)
    into = first.clone()
    summed = _curve(k, bins, into=into, head=2)                                # accumulate adds
    assert summed is into and torch.equal(summed, first + other)
    free = _curve(k, bins, mask=False)
    _check_curve(free, k, bins, mask=False)
    assert free[:, 0].sum() > first[:, 0].sum()


def test_the_curve_over_many_workgroups_and_its_refusals():
    """64 x 65 pixels per sample: three workgroups a sample, the last one partial, the rows folded across samples."""
    from dualpixelface_amd._lib import DpfError
    rng = np.random.RandomState(9)
    B, H, W = 2, 64, 65
    k = dict(conf=rng.uniform(0, 1, (B, 1, H, W)).astype(np.float32), pred=rng.standard_normal((B, 1, H, W)).astype(np.float32),
             target=rng.standard_normal((B, H, W)).astype(np.float32), mask=(rng.uniform(size=(B, H, W)) < 0.7).astype(np.float32), ab=None)
    ops = support.ops()
    conf, pred, target, mask = tensor(k['conf'])[:, 0], tensor(k['pred'])[:, 0], tensor(k['target']), tensor(k['mask'])
    table = ops.confidence_curve(conf, pred, target, mask=mask, bins=16)
    _check_curve(table, k, 16)
    assert torch.equal(table, ops.confidence_curve(conf, pred, target, mask=mask, bins=16))
    for kw, match in ((dict(bins=0), 'bins'), (dict(bins=65), 'bins'), (dict(bins=2.0), 'bins'),
                      (dict(into=torch.zeros(8, 2, dtype=torch.float64, device=DEV)), 'into'),
                      (dict(into=torch.zeros(16, 2, dtype=torch.float32, device=DEV)), 'dtype'),
                      (dict(mask=mask[:, :8]), 'mask'), (dict(target_ab=torch.zeros(B, 3, device=DEV)), 'target_ab')):
        with pytest.raises(DpfError, match=match):
            ops.confidence_curve(conf, pred, target, **dict(dict(mask=mask, bins=16), **kw))
    with pytest.raises(DpfError, match='pred'):
        ops.confidence_curve(conf, pred[:, :8], target)
    with pytest.raises(DpfError, match=r'\[B, H, W\]'):
        ops.confidence_curve(tensor(k['conf']), pred, target)


# ---- 8. the model
def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _rows(model, batch):
    """The metric rows one validation step logs -> {benchmark: row}."""
    for f in model.metric_model.metric_func:
        f.clear()
    model.validation_step(dict(batch), 0)
    rows = {n: f.get_value() for n, f in zip(model.metric_model.metric_name, model.metric_model.metric_func)}
    for f in model.metric_model.metric_func:
        f.clear()
    assert rows
    return rows


def _block(model, **block):
    from dualpixelface_amd.config import Option
    model.option.confidence = Option(dict(block))


def test_stereodpnet_evaluation_with_the_block_absent_disabled_and_enabled():
    from dualpixelface_amd import confidence, ops
    from dualpixelface_amd.config import Option
    opt = support.option('eval_faceDP')
    opt.reconstruct = Option(dict(enabled=True))
    model = support.build('STEREODPNET', opt)
    batch = support.batch(1, 32, 48, seed=9, mask_mode='bern')
    model.eval()
    with torch.no_grad(), ops.deterministic_mode():
        assert not hasattr(model.option, 'confidence')
        absent = model.forward(dict(batch))
        _block(model, enabled=False, estimator='modal', threshold=0.5, gate=['metrics', 'reconstruct'], report=True)
        off = model.forward(dict(batch))
        assert list(off) == list(absent) and not set(off) & set(confidence.RESULT_KEYS)
        for k in absent:
            assert absent[k] is None and off[k] is None or _same_bits(absent[k], off[k]), k
        rows_absent = _rows(model, batch)

        # enabled, every measure, the expectation kept: the measure against torch on the model's own probability volume
        prob = absent['prob_depth']
        heads = model.network(dict(batch))['_heads']
        for measure in confidence.MEASURES:
            _block(model, enabled=True, measure=measure, window=2)
            on = model.forward(dict(batch))
            assert set(on) == set(off) | {'pred_conf', 'pred_spread'} and '_heads' not in on
            for k in off:
                assert off[k] is None and on[k] is None or _same_bits(off[k], on[k]), k
            want = _torch_planes(prob, heads['disp_values'], 2)
            support.close(on['pred_conf'], want[measure], 1e-5, 'pred_conf %s against torch on prob_depth' % measure)
            support.close(on['pred_spread'], want['spread'], 1e-5, 'pred_spread against torch on prob_depth')
            assert on['pred_conf'].shape == off['pred_depth'].shape and float(on['pred_conf'].min()) >= 0 and float(on['pred_conf'].max()) <= 1

        # the modal estimator replaces pred_depth for every head and everything downstream sees it
        _block(model, enabled=True, estimator='modal')
        on = model.forward(dict(batch))
        assert set(on) == set(off) | {'pred_conf', 'pred_spread', 'pred_depth_expectation'}
        assert _same_bits(on['pred_depth_expectation'], off['pred_depth']) and not torch.equal(on['pred_depth'], off['pred_depth'])
        planes = ops.head_confidence(heads['logits'], heads['disp_values'], window=1, want=('modal', 'entropy'))
        assert _same_bits(on['pred_depth'], planes['modal']) and _same_bits(on['pred_conf'], planes['entropy'])
        points, pvalid = ops.backproject(on['pred_depth'], batch['K'], ab=batch['abvalue'], mask=batch['mask'])
        assert torch.equal(on['points'], points) and torch.equal(on['points_valid'], pvalid) and not torch.equal(points, off['points'])

        # the gates
        _block(model, enabled=True, threshold=0.0, gate=['metrics'])
        zero = model.forward(dict(batch))
        assert bool(zero['pred_conf_valid'].all()) and zero['pred_conf_valid'].dtype == torch.uint8 and zero['pred_conf_valid'].shape == (1, 32, 48)
        assert zero['conf_coverage'].shape == (1,) and float(zero['conf_coverage'][0]) == 1.0
        assert _rows(model, batch) == rows_absent                                # threshold 0 keeps every pixel: the ungated rows, bit for bit
        thr = float(on['pred_conf'][:, 0].median())
        _block(model, enabled=True, threshold=thr, gate=['metrics', 'reconstruct'])
        part = model.forward(dict(batch))
        valid = part['pred_conf_valid']
        assert torch.equal(valid, (part['pred_conf'][:, 0] >= thr).to(torch.uint8)) and 0 < int(valid.sum()) < valid.numel()
        cover = float(((valid > 0) & (batch['mask'] > 0)).sum()) / float((batch['mask'] > 0).sum())
        assert abs(float(part['conf_coverage'][0]) - cover) <= 1e-12 and 0 < cover < 1
        gated_rows = _rows(model, batch)
        _block(model, enabled=True, threshold=thr, gate=[])
        plain = model.forward(dict(batch))
        by_hand = dict(batch, mask=batch['mask'] * valid.to(batch['mask'].dtype))
        assert _rows(model, by_hand) == gated_rows and gated_rows != _rows(model, batch)
        # ... and the surface: points_valid is off exactly where the valid map is off
        assert torch.equal(part['points_valid'], plain['points_valid'] * valid) and not torch.equal(part['points_valid'], plain['points_valid'])
        assert _same_bits(part['points'][:, :, valid[0] > 0], plain['points'][:, :, valid[0] > 0])

        # with post_process on, the filter sees the modal map
        from dualpixelface_amd import postprocess
        model.option.post_process = Option(dict(use_bilateral=False, use_guided=True))
        assert postprocess.active(model.option)
        _block(model, enabled=False)
        filtered_expectation = model.forward(dict(batch))
        _block(model, enabled=True, estimator='modal')
        filtered = model.forward(dict(batch))
        res = {'pred_depth': planes['modal'].clone()}
        postprocess.apply(model.option, res, batch, guide=model._views(batch)[0])
        assert _same_bits(filtered['pred_depth'], res['pred_depth']) and not torch.equal(filtered['pred_depth'], filtered_expectation['pred_depth'])
        assert _same_bits(filtered['pred_depth_expectation'], off['pred_depth'])

    # training mode: nothing is estimated, whatever the block says
    with ops.deterministic_mode():
        model.option.post_process = Option(dict(use_bilateral=False, use_guided=False))
        model.train()
        res = model.forward(dict(batch))
    assert not set(res) & set(confidence.RESULT_KEYS) and res['pred_depth'].requires_grad


def test_the_report_accumulates_on_the_device_and_the_trainer_reads_it_once(tmp_path):
    from dualpixelface_amd import confidence, ops
    from dualpixelface_amd.config import Option
    from dualpixelface_amd.trainer import Trainer
    opt = support.option('eval_faceDP')
    opt.confidence = Option(dict(enabled=True, report=True, bins=8))
    model = support.build('STEREODPNET', opt)
    batches = [{k: v.cpu() for k, v in support.batch(1, 32, 48, seed=s, mask_mode='bern').items()} for s in (3, 4)]
    trainer = Trainer(opt, workspace_path=str(tmp_path), rank=0, world_size=1)
    with ops.deterministic_mode():
        rows = trainer.validate(model, batches)
        assert model.confidence_table is None and rows
        curve = trainer.confidence_curve
        want = torch.zeros(8, 2, dtype=torch.float64, device=DEV)
        model.eval()
        with torch.no_grad():
            for b in batches:
                b = {k: v.to(DEV) for k, v in b.items()}
                res = model.forward(dict(b))
                ops.confidence_curve(res['pred_conf'][:, 0], res['pred_depth'][:, 0], b['disp'], mask=b['mask'], bins=8, into=want)
        assert curve == confidence.curve_rows(want.tolist()) and len(curve) == 8
        assert curve[0]['coverage'] == 1.0 and curve[0]['count'] == sum(float((b['mask'] > 0).sum()) for b in batches)
        print('report: %s' % [(r['edge'], round(r['coverage'], 3), r['mean_error']) for r in curve])
        assert trainer.history[-1]['confidence_curve'] == curve
        # the report off: the trainer keeps no curve and the rows are the same
        opt.confidence = Option(dict(enabled=True, report=False))
        assert trainer.validate(model, batches) == rows and trainer.confidence_curve is None


@pytest.mark.parametrize('cls, config', [('DPNET', 'eval_faceDP_dpnet'), ('STEREONET', 'train_faceDP_stereonet')])
def test_models_without_hypotheses_are_refused_by_name(cls, config):
    from dualpixelface_amd import plugin as plugins
    from dualpixelface_amd.config import Option
    opt = support.option(config)
    opt.confidence = Option(dict(enabled=True))
    with pytest.raises(NotImplementedError, match='confidence.*%s' % opt.model_name):
        getattr(plugins, cls)(opt)
