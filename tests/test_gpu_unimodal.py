"""The unimodal loss on the GPU (run with ``-m gpu``): csrc/unimodal.hip through ops.unimodal_loss against the restatements of
tests/unimodal_cpu.py.  The cases, the smallest shapes at which the kernels can go wrong:

    one-tile    B 1, n 1, 8 -> 32, 2 x 3 -> 8 x 12     the fast geometry, a single partial tile
    multi-tile  B 2, n 3, 8 -> 32, 5 x 18 -> 20 x 72   3 x 3 tiles with a partial last row and column, cells shared by up to four tiles,
                                                       weights [1, .7, .5], elliptical mask, every left-out kind
    general     B 1, n 2, 4 -> 16, 3 x 9 -> 12 x 36    the general path, unevenly spaced hypotheses, an explicit laplace_scale
    half-pixel  B 1, n 2, 8 -> 32, 3 x 10 -> 12 x 40   align_corners=False (NNet)
    thin        B 1, n 1, 8 -> 32, 1 x 9 -> 4 x 36     ratio 0 along y, both taps on the one row
    fitted      B 2, n 1, 8 -> 32, 4 x 9 -> 16 x 36    target_ab, depths that are 0, negative and not finite

Exact: `counted` equals the fp32 numpy restatement bit for bit.  `expect` against ops.softargmin's pred on the same logits: both files
take the index arithmetic and the expression order from csrc/dpf_softargmin.h, but unimodal.hip is compiled with -ffp-contract=off and
softargmin.hip contracts products and sums into fused multiply-adds, so NO case is bit for bit and every case is held to the soft-argmin
test's own bound (tests/test_gpu_ops.py::test_softargmin: 1e-5 of the largest value).

Bounded: the loss against the fp64 restatement within 2 x (the fp32 numpy restatement's own deviation from fp64) + one fp32 ulp of the
value + the allowance of `_allowance`; each d k_i against the fp64 autograd gradient, element-wise, within 2 x (the largest deviation of
the fp32 autograd gradient from it) + 1e-6 of the largest gradient magnitude (the convention of tests/test_gpu_photometric.py).  The fp32
figures are computed here, on the same input, not fixed in advance.
"""
import math

import numpy as np
import pytest
import torch

from tests import support
from tests import unimodal_cpu as uc
from tests.support import DEV, bits, tensor

pytestmark = pytest.mark.gpu


def _call(c, gout=None, backward=True, **over):
    """The operator on a case dict (fields replaced by `over`) -> (loss as a float, counted, expect, [d k_i]) as numpy arrays."""
    c = dict(c, **over)
    ks = [tensor(k).requires_grad_(True) for k in c['logits']]
    loss, counted, expect = support.ops().unimodal_loss(ks, c['disp'], tensor(c['target']), mask=tensor(c['mask']), target_ab=tensor(c['ab']),
                                                        head_weights=c['head_weights'], scale=c['scale'], align_corners=c['align'],
                                                        laplace_scale=c['s'], return_extras=True)
    assert loss.shape == () and loss.dtype == torch.float32 and counted.dtype == torch.uint8 and expect.dtype == torch.float32
    grads = None
    if backward:
        (loss if gout is None else loss * gout).backward()
        grads = [k.grad.cpu().numpy() for k in ks]
    return float(loss.detach().double()), counted.cpu().numpy(), expect.cpu().numpy(), grads


def _allowance(c):
    """What the device's exp and log may add to the loss beyond the numpy restatement, which evaluates the same operations in the same
    order with numpy's own exp and log.  In units of u = 2^-24:

      * __expf(x) is v_exp_f32(x * log2(e)): the rounded product moves the exponent by at most |x| u relative, the instruction is held
        to 2 ulp = 4 u (csrc/softargmin.hip:75); numpy's float32 exp is taken at 4 ulp = 8 u.  Relative error of one exponential against
        numpy's: (|x| + 12) u.
      * S = sum_l exp(x_l) with x_l = u_l - mx <= 0 and one x_l = 0, so S >= 1: |dS| <= u (12 S + sum_l |x_l| exp(x_l)) <= u (12 S + L / e),
        and d log(S) <= dS / S <= u (12 + L / e).  logf (OCML, 1 ulp; taken at 2) against numpy's log (taken at 4 ulp): 6 ulp = 12 u of
        log(S) <= log(L).
      * P_l = e_l / Z, e_l = exp(-y_l), y_l >= 0 and one y_l = 0, so Z >= 1, the same way: sum_l |dP_l| <= 2 u (12 + L / e), which the term
        multiplies by |u_l - mx| <= R, the spread of the head's logits (the upsample is a convex combination of them).

    Per term u ((12 + L / e) (1 + 2 R) + 12 log(L)), times sum_h w_h for the loss: L + 1 exponentials and one logarithm per sum."""
    L, u = len(c['disp']), 2.0 ** -24
    R = max(float(k.max()) - float(k.min()) for k in c['logits'])
    return sum(abs(float(w)) for w in c['head_weights']) * u * ((12 + L / math.e) * (1 + 2 * R) + 12 * math.log(L)), R


def _grad_bar(ref):
    own = max(float(np.abs(a - b).max()) for a, b in zip(ref['grad32'], ref['grad64']))
    gmax = max(float(np.abs(g).max()) for g in ref['grad64'])
    return 2.0 * own + 1e-6 * gmax, own, gmax


# ---- 1. the forward, exactly
@pytest.mark.parametrize('name', sorted(uc.CASES))
def test_counted_equals_the_fp32_restatement_and_expect_is_the_soft_argmins_value(name):
    ref = uc.case(name)
    c = ref['case']
    loss, counted, expect, _ = _call(c, backward=False)
    assert np.array_equal(counted, ref['r32']['counted'])
    print('forward %s: %d of %d pixels counted, loss %.9g (fp32 restatement %.9g)' % (name, counted.sum(), counted.size, loss, ref['r32']['loss']))
    for h, k in enumerate(c['logits']):
        pred, _ = support.ops().softargmin(tensor(k), c['disp'], c['scale'], False, c['align'])
        support.close(expect[:, h], pred, 1e-5, 'expect %s head %d against ops.softargmin' % (name, h))
    support.close(expect, ref['r32']['expect'], 1e-5, 'expect %s against the fp32 restatement' % name)


# ---- 2. loss and gradient against fp64
@pytest.mark.parametrize('name', sorted(uc.CASES))
def test_loss_and_gradient_against_the_fp64_restatement(name):
    ref = uc.case(name)
    loss, counted, _, grads = _call(ref['case'])
    own_loss = abs(ref['r32']['loss'] - ref['loss64'])
    allow, R = _allowance(ref['case'])
    bar, own, gmax = _grad_bar(ref)
    err = max(float(np.abs(g.astype(np.float64) - g64).max()) for g, g64 in zip(grads, ref['grad64']))
    print('unimodal %s: loss %.9g, |loss - fp64| %.3e (bar 2 x %.3e + ulp %.3e + allowance %.3e at logit spread %.2f); max |d k - fp64 autograd| '
          '%.3e (bar %.3e = 2 x %.3e + 1e-6 x %.3e)' % (name, loss, abs(loss - ref['loss64']), own_loss, support.ulp_of(ref['loss64']), allow, R,
                                                       err, bar, own, gmax))
    assert abs(loss - ref['loss64']) <= 2.0 * own_loss + support.ulp_of(ref['loss64']) + allow
    for g, g64 in zip(grads, ref['grad64']):
        assert g.shape == g64.shape and np.isfinite(g).all()
        assert (np.abs(g.astype(np.float64) - g64) <= bar).all(), (err, bar)
        assert not g[g64 == 0].any()                                 # every element is written: exactly 0 where nothing reaches it
    assert counted.sum() < counted.size


# ---- 3. closed forms
@pytest.mark.parametrize('name', ['multi-tile', 'general', 'half-pixel'])
def test_zero_logits_give_sum_w_log_L(name):
    """exp(0 - 0) = 1 exactly and S = L exactly, the cross term is a sum of P_l * 0: what is left are logf(L), the product with w_h, the
    sum over the heads and the fp32 result, 4 x 2^-24 as in the host test."""
    c = uc.case(name)['case']
    loss, _, expect, grads = _call(c, logits=[np.zeros_like(k) for k in c['logits']])
    want = sum(float(np.float32(w)) for w in c['head_weights']) * math.log(len(c['disp']))
    print('zero logits %s: loss %.9g, sum w log L %.9g' % (name, loss, want))
    assert abs(loss - want) <= 4 * 2.0 ** -24 * want and all(np.isfinite(g).all() for g in grads)
    support.close(expect, np.full_like(expect, np.mean(np.asarray(c['disp'], dtype=np.float32).astype(np.float64))), 1e-5, 'uniform expectation')


def test_heads_whose_pixels_are_all_left_out_add_zero_and_get_a_zero_gradient():
    c = uc.case('multi-tile')['case']
    loss, counted, _, grads = _call(c, mask=np.zeros_like(c['mask']))
    assert loss == 0.0 and not counted.any() and all(np.isfinite(g).all() and not g.any() for g in grads)
    loss, counted, _, grads = _call(c, target=np.full_like(c['target'], np.nan))
    assert loss == 0.0 and not counted.any() and all(np.isfinite(g).all() and not g.any() for g in grads)


@pytest.mark.parametrize('name', sorted(uc.CASES))
def test_the_gradient_of_every_head_sums_to_zero(name):
    """sum_l (p_l - P_l) = 0 per pixel and the upsample's weights sum to 1: the fp64 gradient sums to 0 (the host test), so the kernel's
    sum is at most the number of elements times the element-wise bar of test 2."""
    ref = uc.case(name)
    bar, _, gmax = _grad_bar(ref)
    for g in _call(ref['case'])[3]:
        total = float(g.astype(np.float64).sum())
        print('%s: sum d k %.3e over %d elements (largest %.3e)' % (name, total, g.size, gmax))
        assert abs(total) <= g.size * bar


def test_a_quarter_of_the_loss_gives_the_bitwise_quarter_of_the_gradient():
    c = uc.case('multi-tile')['case']
    g1, gq = _call(c)[3], _call(c, gout=0.25)[3]
    for a, b in zip(g1, gq):
        assert np.array_equal(bits(a * np.float32(0.25)), bits(b)) and b.any()


def test_three_plain_gradient_steps_lower_the_loss():
    c = uc.case('multi-tile')['case']
    logits, losses = [k.copy() for k in c['logits']], []
    for _ in range(4):
        loss, _, _, grads = _call(c, logits=logits)
        losses.append(loss)
        logits = [(k - np.float32(20.0) * g).astype(np.float32) for k, g in zip(logits, grads)]
    print('plain gradient steps at rate 20:', losses)
    assert losses[0] > losses[1] > losses[2] > losses[3]


# ---- 4. what must not reach a sum
def test_junk_under_the_mask_and_non_finite_depth_change_no_bit():
    c = uc.case('multi-tile')['case']
    clean = _call(c)
    target = c['target'].copy()
    off = np.argwhere(~(c['mask'] > 0))
    assert len(off) >= 6
    for k, v in enumerate((np.nan, np.inf, -np.inf, 1e30, 0.25, -3.0)):          # the last two lie inside the hypotheses' range
        target[tuple(off[k])] = v
    junk = _call(c, target=target)
    assert junk[0] == clean[0] and np.array_equal(junk[1], clean[1]) and np.array_equal(bits(junk[2]), bits(clean[2]))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(junk[3], clean[3]))
    f = uc.case('fitted')['case']
    clean = _call(f)
    depth = f['target'].copy()
    bad = np.argwhere(~np.isfinite(uc.case('fitted')['r32']['t']))
    assert len(bad) >= 3
    for k, pos in enumerate(bad):                                    # NaN, a / 0 and a / -0: t stays non-finite whichever it was before
        depth[tuple(pos)] = (np.nan, 0.0, -0.0)[k % 3]
    assert not np.array_equal(bits(depth), bits(f['target']))
    junk = _call(f, target=depth)
    assert junk[0] == clean[0] and np.array_equal(junk[1], clean[1])
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(junk[3], clean[3]))


# ---- 5. the bits repeat
def _abi_args(c):
    ops = support.ops()
    ks = [tensor(k) for k in c['logits']]
    held = [tensor(c['target']), tensor(c['mask']), tensor(c['ab'])]
    B, _, D, h, w = c['logits'][0].shape
    sc, d = c['scale'], c['disp']
    s = d[1] - d[0] if c['s'] is None else c['s']
    args = [ops._host_ptrs(ks)] + [ops._ptr(t) for t in held] + [B, len(ks), D, h, w, sc * D, sc * h, sc * w, int(c['align']), ops._host_floats(d),
                                                               float(s), ops._host_floats(c['head_weights'])]
    return ks, held, args


def test_two_calls_return_the_same_bits_whatever_the_workspace_held():
    from dualpixelface_amd._lib import lib
    ops = support.ops()
    ref = uc.case('multi-tile')
    c = ref['case']
    ks, held, args = _abi_args(c)
    B, n, H, W = ref['r32']['counted'].shape
    nbytes = lib().call('dpf_unimodal_workspace_bytes', B, n, H, W)
    assert nbytes == n * B * 3 * 3 * 16
    outs = []
    for poison in (float('nan'), -3e30):
        ws = torch.full(((nbytes + 7) // 8,), poison, dtype=torch.float64, device=DEV)
        stats = torch.full((ops.UNIMODAL_STATS,), poison, dtype=torch.float64, device=DEV)
        logsum = torch.full((B, n, H, W), poison, dtype=torch.float32, device=DEV)
        out = torch.full((), poison, dtype=torch.float32, device=DEV)
        grads = [torch.full(k.shape, poison, dtype=torch.float32, device=DEV) for k in ks]
        gout = torch.ones((), dtype=torch.float32, device=DEV)
        lib().call('dpf_unimodal_forward', *args, ops._ptr(ws), nbytes, ops._ptr(logsum), ops._ptr(stats), ops._ptr(out), None, None,
                   ops._stream())
        ws.fill_(poison)                                             # the backward needs the plane and the stats, not the workspace
        lib().call('dpf_unimodal_backward', *args, ops._ptr(logsum), ops._ptr(stats), ops._ptr(gout), ops._host_ptrs(grads), ops._stream())
        outs.append((out.cpu().numpy(), stats.cpu().numpy(), [g.cpu().numpy() for g in grads], logsum.cpu().numpy()))
    (o1, s1, d1, l1), (o2, s2, d2, l2) = outs
    assert np.isfinite(o1) and all(np.isfinite(g).all() for g in d1) and np.isfinite(s1).all() and np.isfinite(l1).all()
    assert bits(o1) == bits(o2) and np.array_equal(s1, s2) and np.array_equal(bits(l1), bits(l2))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(d1, d2))
    loss, _, _, grads = _call(c)                                     # and the operator, with whatever the allocator hands it
    assert np.float32(loss) == o1 and all(np.array_equal(bits(a), bits(b)) for a, b in zip(grads, d1))
    assert s1[:3].tolist() == ref['r32']['count'] and not s1[3:8].any()


def test_a_backward_after_other_operators_and_under_either_deterministic_setting_gives_the_same_bits():
    ops = support.ops()
    c = uc.case('multi-tile')['case']
    plain = _call(c)
    with ops.deterministic_mode(True):
        det = _call(c)
    with ops.deterministic_mode(False):
        nondet = _call(c)
    for other in (det, nondet):
        assert other[0] == plain[0] and all(np.array_equal(bits(a), bits(b)) for a, b in zip(other[3], plain[3]))
    ks = [tensor(k).requires_grad_(True) for k in c['logits']]
    loss = ops.unimodal_loss(ks, c['disp'], tensor(c['target']), mask=tensor(c['mask']), head_weights=c['head_weights'])
    other = uc.case('half-pixel')['case']                            # the same operator on other data, the head itself, a loss that
    _call(other)                                                     # takes the shared scratch, and a sweep over what was freed
    pred = ops.softargmin(tensor(other['logits'][0]).requires_grad_(True), other['disp'], 4, True, False)[0]
    ops.depth_loss(pred.unsqueeze(1), tensor(other['target']).nan_to_num(0.0, 0.0, 0.0)).backward()
    for buf in ops._scratch.values():                                # (not the zero arenas: their slots are promised to be 0)
        buf.fill_(float('nan'))
    torch.full((1 << 20,), float('nan'), device=DEV)
    loss.backward()
    assert float(loss.detach().double()) == plain[0]
    assert all(np.array_equal(bits(k.grad.cpu().numpy()), bits(g)) for k, g in zip(ks, plain[3]))


def test_a_captured_call_replays_the_eager_bits():
    ops = support.ops()
    c = uc.case('multi-tile')['case']
    eager_loss, _, _, eager_grads = _call(c)
    ks = [tensor(k).requires_grad_(True) for k in c['logits']]
    fixed = [tensor(c['target']), tensor(c['mask'])]

    def run():
        loss = ops.unimodal_loss(ks, c['disp'], fixed[0], mask=fixed[1], head_weights=c['head_weights'])
        return (loss,) + torch.autograd.grad(loss, ks)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for _ in range(2):
        for t in outs:
            t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert float(outs[0].detach().double()) == eager_loss
        assert all(np.array_equal(bits(t.cpu().numpy()), bits(g)) for t, g in zip(outs[1:], eager_grads))


# ---- 6. refusals
def test_refusals_raise_and_launch_nothing():
    from dualpixelface_amd._lib import lib, DpfError
    ops = support.ops()
    c = uc.case('one-tile')['case']
    ks, held, args = _abi_args(c)
    q = lambda *a: lib().call('dpf_unimodal_workspace_bytes', *a)                                     # noqa: E731
    assert q(1, 1, 8, 12) == 16 and q(2, 3, 20, 72) == 2 * 3 * 9 * 16 and q(1, 1, 8, 32) == 16 and q(1, 1, 9, 33) == 4 * 16
    assert q(0, 1, 8, 12) == -1 and q(1, 9, 8, 12) == -1 and q(1, 0, 8, 12) == -1 and q(1, 1, 0, 12) == -1 and q(8192, 8, 8, 12) == -1
    assert q(1, 1, 8 * 65536, 12) == -1 and q(1, 1, 65536, 32768) == -1                              # the tile plan's limits
    ws = torch.zeros(2, dtype=torch.float64, device=DEV)
    stats = torch.full((ops.UNIMODAL_STATS,), 7.0, dtype=torch.float64, device=DEV)
    logsum = torch.full((1, 1, 8, 12), 7.0, dtype=torch.float32, device=DEV)
    out = torch.full((), 7.0, dtype=torch.float32, device=DEV)
    expect = torch.full((1, 1, 8, 12), 7.0, dtype=torch.float32, device=DEV)
    grad = torch.full((1, 1, 8, 2, 3), 7.0, dtype=torch.float32, device=DEV)
    tail = (ops._ptr(ws), 16, ops._ptr(logsum), ops._ptr(stats), ops._ptr(out), None, None, ops._stream())

    def refused(a, t, code, entry='dpf_unimodal_forward'):
        with pytest.raises(DpfError, match=code):
            lib().call(entry, *a, *t)

    a, inv, uns = list(args), 'DPF_ERR_INVALID_ARG', 'DPF_ERR_UNSUPPORTED'
    # args: 0 logits, 1 target, 2 mask, 3 ab, 4 B, 5 n, 6 D, 7 h, 8 w, 9 L, 10 H, 11 W, 12 align, 13 disp, 14 scale s, 15 weights
    refused(a[:5] + [0] + a[6:], tail, inv)                                                        # n = 0
    refused(a[:5] + [9] + a[6:], tail, inv)                                                        # n = 9
    refused(a[:6] + [9] + a[7:], tail, uns)                                                        # D = 9
    refused(a[:6] + [16, 2, 3, 64, 8, 12] + a[12:], tail, uns)                                     # D > 8 and L > 32
    refused(a[:9] + [36] + a[10:], tail, uns)                                                      # L = 36 > 32
    refused(a[:9] + [28] + a[10:], tail, uns)                                                      # L no multiple of D
    refused(a[:10] + [9] + a[11:], tail, uns)                                                      # H is not scale h
    for s in (0.0, -0.5, float('inf'), float('nan')):
        refused(a[:14] + [s] + a[15:], tail, inv)                                                  # the scale is not positive and finite
    d = list(c['disp'])
    for bad in (d[:5] + [d[4]] + d[6:], d[:5] + [d[3]] + d[6:], d[:5] + [float('nan')] + d[6:], d[::-1]):
        refused(a[:13] + [ops._host_floats(bad)] + a[14:], tail, inv)                              # hypotheses not strictly ascending
    refused([None] + a[1:], tail, inv)                                                             # a NULL operand
    refused(a[:1] + [None] + a[2:], tail, inv)
    refused(a[:13] + [None] + a[14:], tail, inv)
    refused(a, (ops._ptr(ws), 8) + tail[2:], inv)                                                  # workspace too small
    refused(a, (support.offset_ptr(ws, 4), 16) + tail[2:], inv)                                    # workspace misaligned
    refused(a, tail[:2] + (None,) + tail[3:], inv)                                                 # no plane
    refused(a, tail[:5] + (None, ops._ptr(expect)) + tail[7:], inv)                                # one of the optional pair
    refused(a[:4] + [70000] + a[5:], tail, uns)                                                    # the grid's limit: B n > 65535
    btail = (ops._ptr(logsum), ops._ptr(stats), ops._ptr(out), ops._host_ptrs([grad]), ops._stream())
    refused(a, btail[:2] + (None,) + btail[3:], inv, 'dpf_unimodal_backward')                      # no gout
    refused(a, btail[:3] + (None,) + btail[4:], inv, 'dpf_unimodal_backward')                      # no gradients
    refused(a[:14] + [0.0] + a[15:], btail, inv, 'dpf_unimodal_backward')
    refused(a[:9] + [28] + a[10:], btail, uns, 'dpf_unimodal_backward')
    torch.cuda.synchronize()
    for t in (out, logsum, stats, expect, grad):                                                   # a refusal launches nothing
        assert (t == 7.0).all()
    for over, what in ((dict(s=0.0), 'laplace_scale'), (dict(s=float('nan')), 'laplace_scale'), (dict(disp=d[::-1]), 'ascending'),
                       (dict(disp=d[:-1]), 'disp_values'), (dict(head_weights=(1.0, 0.5)), 'head weights'), (dict(scale=2.5), 'scale'),
                       (dict(target=c['target'][:, :-1]), 'target'), (dict(mask=c['mask'][:, :, :-1]), 'mask'),
                       (dict(ab=np.zeros((1, 3), np.float32)), 'target_ab')):
        with pytest.raises(DpfError, match=what):
            _call(c, backward=False, **over)
    with pytest.raises(DpfError, match='not supported'):
        _call(c, backward=False, logits=[np.zeros((1, 1, 8, 2, 3), np.float32)], scale=5, disp=list(range(40)))


# ---- 7. the whole step
def _first_gradient(model, batch):
    steps = support.loss_steps(model, batch, 1)
    return steps[0], model.flat_gradients(zero=False).clone()


def test_stereodpnet_with_the_new_config_graph_equals_eager(monkeypatch):
    ops = support.ops()
    batch = support.batch(2, 32, 48, seed=7, mask_mode='bern')
    with ops.deterministic_mode():
        monkeypatch.setenv('DPF_STEP_GRAPH', '0')
        b = support.build('STEREODPNET', support.option('train_faceDP_unimodal'))
        eager = support.loss_steps(b, batch, 4)
        monkeypatch.setenv('DPF_STEP_GRAPH', '1')
        a = support.build('STEREODPNET', support.option('train_faceDP_unimodal'))
        graphed = support.loss_steps(a, batch, 4)                     # two warm-up steps, the capture, one replay
        assert a._graph_state.get('graph') is not None and not a._graph_state.get('failed')
    assert graphed == eager, (graphed, eager)
    assert torch.equal(a.flat_parameters(), b.flat_parameters())
    for step in eager:
        assert set(step) == {'smoothL1_loss', 'cosine_loss', 'unimodal_loss', 'final_loss'} and all(np.isfinite(v) for v in step.values())
        assert step['unimodal_loss'] > 0
        f32 = lambda v: torch.tensor(v, dtype=torch.float32)                                          # noqa: E731
        want = float(f32(step['smoothL1_loss']) * 1.0 + f32(step['cosine_loss']) * 1.0 + f32(step['unimodal_loss']) * 0.1)
        assert step['final_loss'] == want, (step, want)
    assert eager[0] != eager[1]                                      # the step moves the weights


def test_the_new_config_changes_the_first_gradient_and_adds_one_key(monkeypatch):
    ops = support.ops()
    batch = support.batch(2, 32, 48, seed=7, mask_mode='bern')
    monkeypatch.setenv('DPF_STEP_GRAPH', '0')
    with ops.deterministic_mode():
        shipped, ours = support.build('STEREODPNET', support.option('train_faceDP')), support.build('STEREODPNET', support.option('train_faceDP_unimodal'))
        keys_shipped, keys_ours = set(shipped(batch)), set(ours(batch))
        first_shipped, ga = _first_gradient(shipped, batch)
        first, gb = _first_gradient(ours, batch)
    assert keys_ours == keys_shipped | {'unimodal_loss'} and 'unimodal_loss' not in keys_shipped and '_heads' not in keys_ours
    assert first['smoothL1_loss'] == first_shipped['smoothL1_loss'] and first['cosine_loss'] == first_shipped['cosine_loss']
    assert torch.isfinite(gb).all() and not torch.equal(ga, gb)
    ours.eval()
    with torch.no_grad():
        assert set(ours(batch)) == set(shipped.eval()(batch))       # evaluation: no loss hook, the private record is gone all the same


def test_a_batch_without_abvalue_takes_the_fitted_target(monkeypatch):
    """StereoDPNet with predict_normal still names the missing 'abvalue' (its normal head needs the conversion before any loss runs), so
    this is StereoDPNet with predict_normal false and loss_type [smoothL1, unimodal]."""
    monkeypatch.setenv('DPF_STEP_GRAPH', '0')
    batch = support.batch(2, 32, 48, seed=7, mask_mode='bern')
    given = support.build('STEREODPNET', support.option('train_faceDP_unimodal', predict_normal=False, loss_type=['smoothL1', 'unimodal'],
                                                       lambdas=[1.0, 0.1]))
    res = given(batch)
    assert torch.equal(res['abvalue'], batch['abvalue']) and float(res['unimodal_loss']) > 0
    fitted = {k: v for k, v in batch.items() if k not in ('abvalue', 'disp')}
    res = given(fitted)
    assert res['abvalue'].shape == (2, 2) and not torch.equal(res['abvalue'], batch['abvalue'])
    assert torch.equal(res['abvalue'], support.ops().affine_fit(res['pred_depth'], batch['idepth']))
    assert np.isfinite(float(res['unimodal_loss'])) and float(res['unimodal_loss']) > 0 and np.isfinite(float(res['final_loss']))
    res['final_loss'].backward()
    with_normal = support.build('STEREODPNET', support.option('train_faceDP_unimodal'))
    with pytest.raises(NotImplementedError, match='abvalue'):
        with_normal.train_step(fitted)


def _stack_gradients(model):
    return [(n, p.grad) for n, p in model.named_parameters() if n.startswith(('aggregation.', 'dres', 'classif')) and n.endswith('weight')]


@pytest.mark.parametrize('cls,config,seed', [('PSMNET', 'train_faceDP_psmnet', 7), ('NNET', 'train_faceDP_nnet', 11)])
def test_one_training_step_of_the_other_models_sends_the_gradient_into_the_aggregation_stack(cls, config, seed, monkeypatch):
    """The fixture size of tests/test_gpu_e2e.py's golden comparisons, 2 x 256 x 256.  First with 'unimodal' added to the model's shipped
    losses (weight 0.1): finite losses under every name, and the step runs.  Then with 'unimodal' as the ONLY loss: whatever reaches the
    aggregation stack's parameters is this loss's gradient."""
    monkeypatch.setenv('DPF_STEP_GRAPH', '0')
    batch = support.batch(2, 256, 256, seed=seed)
    shipped = support.option(config).model
    names, lambdas = list(shipped.loss_type) + ['unimodal'], list(shipped.lambdas) + [0.1]
    model = support.build(cls, support.option(config, loss_type=names, lambdas=lambdas))
    res = model.train_step(batch, None, lr=1e-4)
    assert set(k for k in res if k.endswith('_loss')) == {n + '_loss' for n in names} | {'final_loss'} and '_heads' not in res
    assert all(np.isfinite(float(res[k].detach())) for k in res if k.endswith('_loss')) and float(res['unimodal_loss'].detach()) > 0
    del model
    model = support.build(cls, support.option(config, loss_type=['unimodal'], lambdas=[1.0]))
    model.flat_gradients(zero=True)
    res = model(batch)
    assert set(k for k in res if k.endswith('_loss')) == {'unimodal_loss', 'final_loss'} and '_heads' not in res
    assert np.isfinite(float(res['final_loss'].detach())) and float(res['unimodal_loss'].detach()) > 0
    res['final_loss'].backward()
    stack = _stack_gradients(model)
    assert len(stack) >= 4
    for n, g in stack:
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, n
