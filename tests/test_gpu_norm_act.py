"""csrc/norm_act.hip on the GPU (run with ``-m gpu``) against the closed-form fp64 reference tests/norm_act_cpu.py: rows longer than one
chunk, ragged tails, the scalar path, every operand / output subset, the pre-zeroed arena after it wrapped, and inputs whose statistics
are hard in fp32.  x is passed as [N, C, S] so that S is free.  Sections 6 and 7 are about the operator layer above the kernels: the
multi-branch SyncBatchNorm exchange of norm_act_concat, and the C entries every path of the three normalisation nodes reaches.

Bars, the ones test_gpu_ops.py uses for these kernels: forward and running statistics 1e-5 of the scale, gradients 2e-4 -- applied per
channel (every [:, c] slice, every element of dw / db), so that one large channel cannot hide a wrong small one."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import norm_act_cpu as na
from tests import support
from tests.support import DEV, close, rnd
from tests.support import TwoRankExchange as _TwoRankExchange

pytestmark = pytest.mark.gpu

FWD, GRAD = 1e-5, 2e-4
GRADS = ('dx', 'dw', 'db', 'dslope', 'dres', 'dres2')


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _params(C, seed):
    """weight in [0.5, 1.5), bias ~ N(0, 1), running_var in [0.5, 1.5), running_mean in [0.05, 0.15): the test inputs have means >= 0, so
    0.9 * running_mean + 0.1 * mean does not cancel and the per-element bar on the updated running_mean stays a relative one."""
    w = torch.rand(C, generator=_gen(seed + 1)) + 0.5
    b = rnd(C, seed=seed + 2)
    rm = torch.rand(C, generator=_gen(seed + 3)) * 0.1 + 0.05
    rv = torch.rand(C, generator=_gen(seed + 4)) + 0.5
    return w, b, rm, rv


def _inputs(N, C, S, seed, wb=True, res=False, res2=False, slope=False):
    """fp32 CPU operands.  The upstream gradient has mean 0.5: the per-channel sums dw / db are then no pure cancellations, and the
    per-element bar on them is a statement about the kernel."""
    t = {'x': rnd(N, C, S, seed=seed) * 2 + 0.7, 'go': rnd(N, C, S, seed=seed + 5) + 0.5}
    w, b, t['rm'], t['rv'] = _params(C, seed)
    t['w'], t['b'] = (w, b) if wb else (None, None)
    t['res'] = rnd(N, C, S, seed=seed + 6) if res else None
    t['res2'] = rnd(N, C, S, seed=seed + 7) if res2 else None
    t['slope'] = torch.tensor([0.17]) if slope else None
    return t


def _reference(t, mode, act, slope_const=0.0):
    return na.norm_act(t['x'], t['w'], t['b'], t['slope'], t['res'], t['res2'], t['rm'], t['rv'], mode, act, slope_const, t['go'])


KINK = 1e-4


def _reference_off_the_kink(t, mode, act, slope_const=0.0):
    """_reference(); for ReLU / PReLU / LeakyReLU, x is first moved (by <= 4e-3, in place) wherever the activation's argument lies within
    KINK of 0.  The derivative jumps there, and fp32 cannot tell the side: among the 1.7e7 elements of the largest case a few arguments
    are below 1e-6, each of them a gradient off by the whole upstream value in any fp32 implementation, torch's included.  The weights
    are positive, so x moves the argument the way it is pushed; the statistics change by ~1e-10, and the returned reference is the one of
    the moved inputs, with every argument at least KINK from 0."""
    ref = _reference(t, mode, act, slope_const)
    if act not in (na.ACT_RELU, na.ACT_PRELU, na.ACT_LEAKY):
        return ref
    for _ in range(3):
        near = ref['z'].abs() < KINK
        if not bool(near.any()):
            return ref
        t['x'][near] += (4e-3 * torch.sign(ref['z'][near] + 1e-300)).float()
        ref = _reference(t, mode, act, slope_const)
    raise AssertionError('arguments within %g of the kink remain' % KINK)


@functools.lru_cache(maxsize=None)
def _norm_act_case(N, C, S, mode, act, wb=True, res=False, res2=False):
    """(operands, fp64 reference) of one case: built once, shared by the default-mode and the deterministic-mode run, never modified."""
    t = _inputs(N, C, S, 1000 * mode + 10 * act + S % 97, wb, res, res2, act == na.ACT_PRELU)
    return t, _reference_off_the_kink(t, mode, act, 0.1)


def _run_norm_act(ops, t, mode, act, slope_const=0.0, want=('x', 'w', 'b', 'slope', 'res', 'res2'), exchange=None, x=None, go=None, repeat=False):
    """ops.norm_act on the device copies of t; gradients for the operands named in `want` that exist.  -> dict like the reference's;
    repeat: a second backward of the same graph, under 'again'."""
    dev = {}
    for k in ('x', 'w', 'b', 'slope', 'res', 'res2'):
        v = t[k] if (k != 'x' or x is None) else x
        dev[k] = None if v is None else v.to(DEV).requires_grad_(k in want)
    rm, rv = t['rm'].to(DEV), t['rv'].to(DEV)
    norm_stats = (rm, rv) if mode in (1, 2) else (None, None)
    y = ops.norm_act(dev['x'], dev['w'], dev['b'], dev['slope'], dev['res'], dev['res2'], norm_stats[0], norm_stats[1], mode, act,
                     slope_const, exchange=exchange)
    got = {'y': y.detach(), 'running_mean': rm, 'running_var': rv}
    leaves = [(n, dev[k]) for n, k in zip(GRADS, ('x', 'w', 'b', 'slope', 'res', 'res2')) if dev[k] is not None and k in want]
    gdev = (t['go'] if go is None else go).to(DEV)
    grads = torch.autograd.grad(y, [v for _, v in leaves], gdev, retain_graph=repeat)
    got.update({n: g for (n, _), g in zip(leaves, grads)})
    if repeat:
        got['again'] = dict(zip([n for n, _ in leaves], torch.autograd.grad(y, [v for _, v in leaves], gdev)))
    torch.cuda.synchronize()
    return got


def _compare(got, ref, tag, bars=None, expect=None):
    """Per-channel bars on y, the running statistics and every gradient `got` holds; expect: the gradients it must hold.
    bars: {name: per-channel bound} that replaces the standing bar where it is larger.  -> {name: err / scale per channel}."""
    bars = bars or {}
    rel = {'y': na.close_channels(got['y'], ref['y'], FWD, tag + ' y', bars.get('y'))}
    for k in ('running_mean', 'running_var'):                  # updated by mode 1, left alone by every other
        rel[k] = na.close_channels(got[k], ref[k], FWD, tag + ' ' + k, bars.get(k))
    have = [n for n in GRADS if n in got]
    if expect is not None:
        assert have == [n for n in GRADS if n in expect], (tag, have, expect)
    for n in have:
        assert ref[n] is not None, (tag, n)
        rel[n] = na.close_channels(got[n], ref[n], GRAD, tag + ' ' + n, bars.get(n))
    return rel


def _same_bits(got, tag):
    for n, g in got['again'].items():
        assert torch.equal(g, got[n]), '%s: %s differs between two backwards in deterministic mode' % (tag, n)


# ---- 1. rows of more than one chunk
# mode 1 with res, res2 and PReLU: all three reduction slots (sum dz, sum dz * xhat, the slope sum) cross chunks
ROW_CASES = [(1, na.ACT_PRELU, S) for S in (4100, 4099, 8192, 12292)]
ROW_CASES += [(3, na.ACT_SIGMOID, S) for S in (4100, 4099)] + [(2, na.ACT_RELU, S) for S in (4100, 4099)]


@pytest.mark.parametrize('det', [False, True], ids=['default', 'deterministic'])
@pytest.mark.parametrize('mode,act,S', ROW_CASES)
def test_row_chunks(mode, act, S, det):
    """N = 2, C = 5.  S = 4100: 16-byte path, last chunk of 4 elements; 4099: scalar path, last chunk of 3; 8192: exactly two chunks;
    12292: three full chunks and a tail.  Forward, running statistics and every gradient per channel; in deterministic mode a second
    backward returns the same bits."""
    ops = support.ops()
    full = mode == 1
    t, ref = _norm_act_case(2, 5, S, mode, act, True, full, full)
    with ops.deterministic_mode(det):
        got = _run_norm_act(ops, t, mode, act, repeat=det)
    expect = ('dx', 'dw', 'db') + (('dslope', 'dres', 'dres2') if full else ())
    _compare(got, ref, 'mode %d S %d' % (mode, S), expect=expect)
    if det:
        _same_bits(got, 'mode %d S %d' % (mode, S))


def reduce_chunk(rows, S):
    """norm_act.hip's reduce_chunk(): the row piece one workgroup of a reduction kernel takes (the apply kernels always take 4096)."""
    return min(max(((S * rows // 4096 + 1023) // 1024) * 1024, 4096), 65536)


@pytest.mark.parametrize('S', [131076, 131104])
def test_reduce_chunk_differs_from_apply_chunk(S):
    """N = 4, C = 32, ReLU, no residuals, default mode.  S = 131104 is the smallest S of this N * C at which reduce_chunk() leaves 4096: the
    reductions walk 5120-element pieces (25 full ones and a ragged one of 3104) while the apply kernels walk 4096-element ones (32 and a
    piece of 32).  S = 131076 still gives 4096 (the integer division S * rows / 4096 yields 4096, not 4097): 32 full pieces and one of 4,
    on rows 32 times as long as in test_row_chunks."""
    assert reduce_chunk(128, 131104) == 5120 and reduce_chunk(128, 131100) == 4096 and reduce_chunk(128, 131076) == 4096
    ops = support.ops()
    t, ref = _norm_act_case(4, 32, S, 1, na.ACT_RELU)
    got = _run_norm_act(ops, t, 1, na.ACT_RELU)
    _compare(got, ref, 'S %d' % S, expect=('dx', 'dw', 'db'))


# ---- 2. channel slices of a concatenation on long rows
@pytest.mark.parametrize('det', [False, True], ids=['default', 'deterministic'])
@pytest.mark.parametrize('S', [4100, 4099])
def test_norm_act_concat_long_rows(S, det):
    """norm_act_concat with branch widths (8, 5, 16), training and eval, against torch.cat of the per-branch reference: the slice base
    ((n * Ctot + c0 + c) - row) * S of the forward's y and the backward's dy, on rows of two chunks."""
    ops = support.ops()
    N, Cs = 2, (8, 5, 16)
    for mode in (1, 2):
        go = rnd(N, sum(Cs), S, seed=77) + 0.5
        ts, refs, c0 = [], [], 0
        for i, C in enumerate(Cs):
            t = _inputs(N, C, S, 300 + 10 * i)
            t['go'] = go[:, c0:c0 + C]
            ts.append(t)
            refs.append(_reference(t, mode, na.ACT_NONE))
            c0 += C
        xs, ws, bs = [[t[k].to(DEV).requires_grad_() for t in ts] for k in ('x', 'w', 'b')]
        rms, rvs = [[t[k].to(DEV) for t in ts] for k in ('rm', 'rv')]
        with ops.deterministic_mode(det):
            out = ops.norm_act_concat([(x, w, b, rm, rv, None) for x, w, b, rm, rv in zip(xs, ws, bs, rms, rvs)], mode)
            gg = torch.autograd.grad(out, xs + ws + bs, go.to(DEV))
        na.close_channels(out, torch.cat([r['y'] for r in refs], 1), FWD, 'concat y mode %d' % mode)
        for i in range(3):
            for k, g in (('dx', gg[i]), ('dw', gg[3 + i]), ('db', gg[6 + i])):
                na.close_channels(g, refs[i][k], GRAD, 'concat %s branch %d mode %d' % (k, i, mode))
            if mode == 1:
                na.close_channels(rms[i], refs[i]['running_mean'], FWD, 'concat running_mean branch %d' % i)
                na.close_channels(rvs[i], refs[i]['running_var'], FWD, 'concat running_var branch %d' % i)


# ---- 3. SyncBatchNorm on long rows
@pytest.mark.parametrize('det', [False, True], ids=['default', 'deterministic'])
def test_sync_batchnorm_long_rows(det):
    """The two-rank emulation of test_gpu_ops.py::test_sync_batchnorm_matches_full_batch at S = 4100: rank 0 holds 2 samples, the emulated
    rank 1 three more.  Local moments, the merge, phase 1 (local reductions) and phase 2 (dx with the device-side global count) on rows of
    two chunks, against batch norm over all 5 samples; dw / db are this rank's partial sums."""
    ops = support.ops()
    C, S = 6, 4100
    t = _inputs(5, C, S, 500)
    ref = _reference_off_the_kink(t, 1, na.ACT_RELU)
    x, go = t['x'].double(), t['go'].double()
    mean = x.mean((0, 2), keepdim=True)
    invstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean((0, 2), keepdim=True) + na.EPS)
    xh = (x - mean) * invstd
    dz = go * (xh * t['w'].double().view(1, C, 1) + t['b'].double().view(1, C, 1) > 0)
    ex = _TwoRankExchange(t['x'][2:].to(DEV), dz[2:].float().to(DEV), mean.reshape(C).float().to(DEV), invstd.reshape(C).float().to(DEV))
    with ops.deterministic_mode(det):
        got = _run_norm_act(ops, t, 1, na.ACT_RELU, exchange=ex, x=t['x'][:2].contiguous(), go=t['go'][:2].contiguous())
    local = dict(ref, y=ref['y'][:2], dx=ref['dx'][:2], dw=(dz * xh)[:2].sum((0, 2)), db=dz[:2].sum((0, 2)))
    _compare(got, local, 'syncbn', expect=('dx', 'dw', 'db'))


# ---- 4. operand and output subsets
SUBSETS = {
    # name: (mode, act, weight and bias, res, res2, operands that require a gradient)
    'res_only': (1, na.ACT_PRELU, True, True, False, ('x', 'w', 'b', 'slope', 'res')),
    'res2_only': (1, na.ACT_PRELU, True, False, True, ('x', 'w', 'b', 'slope', 'res2')),            # backward: RES = false
    'neither': (1, na.ACT_PRELU, True, False, False, ('x', 'w', 'b', 'slope')),
    'dres_without_dx': (1, na.ACT_PRELU, True, True, True, ('w', 'b', 'slope', 'res', 'res2')),
    'parameters_only': (1, na.ACT_PRELU, True, True, False, ('w', 'b', 'slope')),                   # the stand-alone finalize kernel
    'instance_norm_no_affine': (3, na.ACT_RELU, False, False, False, ('x',)),
    'prelu_no_norm': (0, na.ACT_PRELU, False, True, False, ('x', 'slope', 'res')),                  # reduction without statistics
    'prelu_no_norm_slope_only': (0, na.ACT_PRELU, False, False, False, ('slope',)),
    'leaky_no_norm': (0, na.ACT_LEAKY, False, False, True, ('x', 'res2')),
}


@pytest.mark.parametrize('det', [False, True], ids=['default', 'deterministic'])
@pytest.mark.parametrize('name', sorted(SUBSETS))
def test_operand_and_output_subsets(name, det):
    """S = 4100, N = 2, C = 5: the <ACT, RES> specialisations and the wanted-output branches that the training test (both residuals, every
    gradient) never takes.  Exactly the wanted gradients come back, each within the bars."""
    ops = support.ops()
    mode, act, wb, res, res2, want = SUBSETS[name]
    t, ref = _norm_act_case(2, 5, 4100, mode, act, wb, res, res2)
    with ops.deterministic_mode(det):
        got = _run_norm_act(ops, t, mode, act, 0.1, want=want, repeat=det)
    expect = [n for n, k in zip(GRADS, ('x', 'w', 'b', 'slope', 'res', 'res2')) if k in want]
    _compare(got, ref, name, expect=expect)
    if det:
        _same_bits(got, name)


def test_zero_slot_arena_wrap():
    """Mode 3 backwards with N = 4, C = 4096, S = 4: 3 * N * C = 49152 floats of the pre-zeroed 2^20-float arena per call, so 50 calls
    refill it twice after the first fill.  The reductions add into their slot without clearing it: every call's gradients must equal the
    first call's (whose dx is held to the reference), also right after a refill."""
    ops = support.ops()
    N, C, S = 4, 4096, 4
    # every row is a permutation of (-1.5, -0.5, 0.5, 1.5) * scale + offset: no row of four has a vanishing variance
    base = torch.tensor([-1.5, -0.5, 0.5, 1.5])
    perm = torch.argsort(torch.rand(N, C, S, generator=_gen(61)), dim=2)
    x = base[perm] * (torch.rand(N, C, 1, generator=_gen(62)) + 0.5) + rnd(N, C, 1, seed=63)
    w, b, _, _ = _params(C, 64)
    go = rnd(N, C, S, seed=65) + 0.5
    ref = na.norm_act(x, w, b, mode=3, act=na.ACT_SIGMOID, go=go)
    xg, wg, bg = [v.to(DEV).requires_grad_() for v in (x, w, b)]
    gdev = go.to(DEV)
    ops.reset_zero_arenas()
    arena = lambda: [st[1] for st in ops._zero_arena.values()]
    first, fills, before = None, 0, arena()
    for call in range(50):
        y = ops.norm_act(xg, wg, bg, mode=3, act=ops.ACT_SIGMOID)
        grads = torch.autograd.grad(y, (xg, wg, bg), gdev)
        after = arena()
        fills += any(a <= p for a, p in zip(after, before)) or len(after) != len(before)
        before = after
        if first is None:
            first = grads
            na.close_channels(y, ref['y'], FWD, 'call 0 y')
            na.close_channels(grads[0], ref['dx'], GRAD, 'call 0 dx')
            continue
        for g, g0, n in zip(grads, first, ('dx', 'dw', 'db')):
            err, scale = na.channel_errors(g, g0)
            bad = (err > GRAD * scale.clamp(min=1e-6)).nonzero().reshape(-1).tolist()
            assert not bad, 'call %d: %s of channels %s differs from the first call (arena fills so far: %d)' % (call, n, bad[:8], fills)
    assert fills >= 3, fills


# ---- 5. statistics that are hard in fp32
HARD_S = 8200
HARD = ['offset 1e2', 'offset 1e3', 'offset 1e4', '5 + 1e-3 N(0,1)', 'constant 37.25', 'x[0,c,0] = 8', 'x[0,c,0] = 64',
        'x[0,c,0] = 1000', '50 + N(0,1), x[0,c,0] = 0', '2 N(0,1) + 0.7']
TORCH_RELATIVE = 5            # channels 0 .. 4: fp32 itself limits the answer, the bar follows torch's own fp32 error
OUTLIERS = (5, 6, 7, 8)


@functools.lru_cache(maxsize=None)
def _hard_case():
    """-> (operands, fp64 reference, {name: 4 x torch's fp32 CPU batch_norm error / scale per channel, 0 where the standing bar alone
    holds}).  One property per channel, N = 2, S = 8200 (three chunks, ragged)."""
    N, C, S = 2, len(HARD), HARD_S
    t = _inputs(N, C, S, 700)
    x = rnd(N, C, S, seed=701)
    for c, off in ((0, 1e2), (1, 1e3), (2, 1e4)):
        x[:, c] += off
    x[:, 3] = 5.0 + 1e-3 * x[:, 3]
    x[:, 4] = 37.25
    for c, v in ((5, 8.0), (6, 64.0), (7, 1000.0)):
        x[0, c, 0] = v
    x[:, 8] += 50.0
    x[0, 8, 0] = 0.0
    x[:, 9] = 2.0 * x[:, 9] + 0.7
    t['x'] = x
    ref = _reference(t, 1, na.ACT_NONE)
    xt, wt, bt = [t[k].clone().requires_grad_() for k in ('x', 'w', 'b')]
    rm, rv = t['rm'].clone(), t['rv'].clone()
    yt = F.batch_norm(xt, rm, rv, wt, bt, True, 0.1, 1e-5)
    gt = torch.autograd.grad(yt, (xt, wt, bt), t['go'])
    bars = {}
    for n, v in (('y', yt), ('running_mean', rm), ('running_var', rv), ('dx', gt[0]), ('dw', gt[1]), ('db', gt[2])):
        err, scale = na.channel_errors(v, ref[n])
        bar = 4.0 * err / scale.clamp(min=1e-6)
        bar[TORCH_RELATIVE:] = 0.0
        bars[n] = bar
        print('torch fp32 %s err / scale per channel: %s' % (n, ' '.join('%.2e' % e for e in (err / scale.clamp(min=1e-6)).tolist())))
    return t, ref, bars


@pytest.mark.parametrize('det', [False, True], ids=['default', 'deterministic'])
def test_hard_statistics_batch_norm(det):
    """Mode 1, no activation (what F.batch_norm computes), one property per channel (HARD), fp64 reference on the same fp32 inputs.
    Channels 0 - 4 (common offsets, a tiny spread, a constant channel): the bar is the larger of the standing bar and 4 x the error of
    torch's fp32 CPU batch_norm on that channel.  Channels 5 - 8 (an atypical first element) and 9 (plain): the standing bar.

    Measured err / scale per channel (channels 0 .. 9), MI355X:
      y, shift K_c = x[0, c, 0] (before), default:        1.6e-7 1.1e-6 1.1e-4 3.6e-5 3.0e-4 | 3.2e-6 2.7e-4 3.8e-5 1.1e-5 | 9.1e-8
      y, shift K_c = x[0, c, 0] (before), deterministic:  2.3e-7 1.1e-6 1.1e-4 3.6e-5 3.0e-4 | 3.2e-6 1.2e-4 3.8e-5 1.1e-4 | 8.9e-8
        (channels 6, 7, 8 over the 1e-5 bar in both modes; the run stopped at y)
      y, shift = median of three (now), default:          2.3e-7 1.1e-6 1.1e-4 3.6e-5 3.0e-4 | 2.3e-7 4.6e-8 2.5e-8 2.6e-8 | 3.8e-8
      y, shift = median of three (now), deterministic:    2.3e-7 1.1e-6 1.1e-4 3.6e-5 3.0e-4 | 7.5e-8 1.4e-8 2.5e-8 2.6e-8 | 3.8e-8
      y, torch fp32 CPU:                                  2.3e-7 1.1e-6 1.1e-4 3.6e-5 7.1e-4 | 7.5e-8 1.4e-8 2.5e-8 2.6e-8 | 3.8e-8
      dx now, default:                                    2.5e-7 1.1e-5 1.6e-4 4.1e-6 8.2e-8 | 3.1e-7 1.9e-7 1.2e-7 5.7e-6 | 6.3e-8
      dx now, deterministic:                              2.5e-7 1.1e-5 1.6e-4 4.1e-6 8.2e-8 | 1.4e-7 1.5e-7 1.2e-7 5.7e-6 | 6.3e-8
      dx, torch fp32 CPU:                                 2.7e-7 1.1e-5 1.6e-4 4.1e-6 9.3e-8 | 1.4e-7 1.7e-7 1.4e-7 5.7e-6 | 8.2e-8
      dw now, default:                                    2.1e-5 2.6e-3 1.2e-2 1.5e-2 0      | 2.2e-5 2.0e-6 5.5e-7 8.0e-5 | 1.8e-6
      dw now, deterministic:                              2.1e-5 2.6e-3 1.2e-2 1.5e-2 0      | 6.3e-6 1.6e-6 4.3e-7 8.0e-5 | 2.2e-6
      dw, torch fp32 CPU:                                 2.1e-5 2.6e-3 1.2e-2 1.5e-2 0      | 7.1e-6 1.8e-6 3.2e-7 7.9e-5 | 3.2e-6
      running_mean, running_var, db now, both modes:      <= 1.6e-7 on every channel (torch: <= 2.4e-7)
    On the offset channels the kernels and torch meet the same fp32 limit (the mean, and bias - mean * scale, rounded to fp32)."""
    ops = support.ops()
    t, ref, bars = _hard_case()
    with ops.deterministic_mode(det):
        got = _run_norm_act(ops, t, 1, na.ACT_NONE, want=('x', 'w', 'b'), repeat=det)
    _compare(got, ref, 'hard', bars=bars, expect=('dx', 'dw', 'db'))
    if det:
        _same_bits(got, 'hard')


@pytest.mark.parametrize('det', [False, True], ids=['default', 'deterministic'])
def test_hard_statistics_instance_norm(det):
    """Mode 3 on the channels with an atypical first element (x[0, c, 0] = 8, 64, 1000 in N(0,1); 0 in 50 + N(0,1)): only sample 0's
    row holds the outlier, sample 1's is plain.  Standing bars.

    Measured err / scale per channel (x[0, c, 0] = 8, 64, 1000; 50 + N(0,1) with 0), MI355X:
      y before, default 4.9e-6 1.4e-4 1.5e-5 1.7e-5, deterministic 2.1e-6 1.4e-4 2.4e-4 1.7e-5 (three of four over the bar)
      y now,    default 1.6e-7 6.2e-8 5.0e-8 7.0e-8, deterministic 8.7e-8 5.3e-9 5.0e-8 4.5e-8
      now, both modes: dx <= 3.1e-6, dw <= 8.2e-5, db <= 6.1e-8"""
    ops = support.ops()
    t, _, _ = _hard_case()
    sl = slice(OUTLIERS[0], OUTLIERS[-1] + 1)
    sub = {k: None if v is None else (v[:, sl] if v.dim() == 3 else v[sl]).contiguous() for k, v in t.items()}
    ref = _reference(sub, 3, na.ACT_NONE)
    with ops.deterministic_mode(det):
        got = _run_norm_act(ops, sub, 3, na.ACT_NONE, want=('x', 'w', 'b'))
    _compare(got, ref, 'hard instance norm', expect=('dx', 'dw', 'db'))


def test_conv_epilogue_statistics_under_an_offset():
    """The statistics a convolution's epilogue produces (dpf_conv_forward_stats + dpf_bn_finalize_partials, fp64 from the first add) with
    a conv bias of 1e3, in the style of test_gpu_ops.py::test_conv_epilogue_batchnorm_statistics: normalised output and running statistics
    against the fp64 reference on the convolution's own fp32 output, bar per channel the larger of 1e-5 and 4 x torch's fp32 error.

    Measured on an MI355X over the 35 channels: y err / scale <= 2.0e-5, at most 0.27 of the channel's bar (torch's fp32 error on that
    channel is 1.8e-5: values near 1e3 in fp32 limit both); running_mean <= 5.1e-8, running_var <= 4.7e-8."""
    ops = support.ops()
    N, C, K, D, H, W, ks = 3, 12, 35, 1, 33, 68, (1, 3, 3)
    x = rnd(N, C, D, H, W, seed=70)
    w = rnd(K, C, *ks, seed=71) * 0.2
    b = rnd(K, seed=72) + 1e3
    gamma, beta = rnd(K, seed=73).abs() + 0.5, rnd(K, seed=74)
    prev = ops.FUSE_BN_STATS
    ops.FUSE_BN_STATS = True
    try:
        st = {}
        rm, rv = torch.zeros(K, device=DEV), torch.ones(K, device=DEV)
        y = ops.conv3d(x.to(DEV), w.to(DEV), b.to(DEV), 1, (0, 1, 1), 1, stats=st)
        assert st, 'the LDS-DMA kernel should have taken this shape'
        z = ops.norm_act(y, gamma.to(DEV), beta.to(DEV), None, None, None, rm, rv, 1, ops.ACT_RELU, stats=st)
        assert not st                                                   # consumed
    finally:
        ops.FUSE_BN_STATS = prev
    yc = y.cpu()
    assert (yc.mean((0, 2, 3, 4)) - 1e3).abs().max() < 10.0            # the offset reached the normalised tensor
    ref = na.norm_act(yc, gamma, beta, running_mean=torch.zeros(K), running_var=torch.ones(K), mode=1, act=na.ACT_RELU)
    rm_t, rv_t = torch.zeros(K), torch.ones(K)
    z_t = F.relu(F.batch_norm(yc, rm_t, rv_t, gamma, beta, True, 0.1, 1e-5))
    for name, a, v in (('y', z, z_t), ('running_mean', rm, rm_t), ('running_var', rv, rv_t)):
        err, scale = na.channel_errors(v, ref[name])
        na.close_channels(a, ref[name], FWD, 'conv epilogue ' + name, bars=4.0 * err / scale.clamp(min=1e-6))


# ---- 6. SyncBatchNorm over the branches of a concatenation
SYNC_CAT = (8, 5, 16)


@functools.lru_cache(maxsize=None)
def _sync_concat_case():
    """Branch widths (8, 5, 16), 5 samples of 12 x 20, operands as in test_gpu_ops.py::test_norm_act_concat_matches_separate_norm_and_cat.
    The reference is torch.cat of F.batch_norm over all 5 samples on the CPU with autograd.  Built once, never modified."""
    H, W = 12, 20
    xs = [rnd(5, C, H, W, seed=100 + i).requires_grad_() for i, C in enumerate(SYNC_CAT)]
    ws = [(rnd(C, seed=110 + i).abs() + 0.5).requires_grad_() for i, C in enumerate(SYNC_CAT)]
    bs = [rnd(C, seed=120 + i).requires_grad_() for i, C in enumerate(SYNC_CAT)]
    rms = [rnd(C, seed=130 + i) * 0.1 for i, C in enumerate(SYNC_CAT)]
    rvs = [rnd(C, seed=140 + i).abs() + 0.5 for i, C in enumerate(SYNC_CAT)]
    rms_r, rvs_r = [t.clone() for t in rms], [t.clone() for t in rvs]
    y = torch.cat([F.batch_norm(x, rm, rv, w, b, True, 0.1, 1e-5) for x, w, b, rm, rv in zip(xs, ws, bs, rms_r, rvs_r)], 1)
    go = rnd(*y.shape, seed=150)
    dxs = torch.autograd.grad(y, xs, go)
    case = {'x': [x.detach() for x in xs], 'w': [w.detach() for w in ws], 'b': [b.detach() for b in bs], 'rm': rms, 'rv': rvs, 'go': go,
            'y': y.detach(), 'dx': dxs, 'running_mean': rms_r, 'running_var': rvs_r, 'dz': [], 'mean': [], 'invstd': [], 'dw': [], 'db': []}
    c0 = 0
    for x, C in zip(case['x'], SYNC_CAT):
        dz = go[:, c0:c0 + C]                                          # no activation: dz is the upstream gradient's slice
        mean = x.mean((0, 2, 3))
        invstd = 1.0 / torch.sqrt(x.var((0, 2, 3), unbiased=False) + 1e-5)
        xh = (x - mean.view(1, C, 1, 1)) * invstd.view(1, C, 1, 1)
        case['dz'].append(dz)
        case['mean'].append(mean)
        case['invstd'].append(invstd)
        case['dw'].append((dz * xh)[:2].sum((0, 2, 3)))               # this rank's partial sums (DDP averages them afterwards)
        case['db'].append(dz[:2].sum((0, 2, 3)))
        c0 += C
    return case


@pytest.mark.parametrize('det', [False, True], ids=['default', 'deterministic'])
def test_sync_batchnorm_concat_matches_full_batch(det):
    """norm_act_concat, mode 1, no activation, with the two-rank emulation: rank 0 holds 2 samples, the emulated rank 1 three more.  Three
    unequal widths put the gather slices [2C+1] at offsets 0, 17, 28 and the reduce slices [3C+1] at 0, 25, 41, so a swapped offset or a
    wrong count slot shows.  Output, the six running statistics and dx of the local samples against batch norm over all 5 samples, dw / db
    against this rank's partial sums; bars of the two tests this combines (forward and running statistics 1e-5, gradients 2e-4), and
    the branches travel in ONE all-gather and ONE all-reduce."""
    ops = support.ops()
    t = _sync_concat_case()
    ex = _TwoRankExchange([x[2:].to(DEV) for x in t['x']], [dz[2:].to(DEV) for dz in t['dz']], [m.to(DEV) for m in t['mean']],
                          [s.to(DEV) for s in t['invstd']])
    xs, ws, bs = [[v[:2].to(DEV).requires_grad_() for v in t['x']]] + [[v.to(DEV).requires_grad_() for v in t[k]] for k in ('w', 'b')]
    rms, rvs = [[v.to(DEV) for v in t[k]] for k in ('rm', 'rv')]
    with ops.deterministic_mode(det):
        out = ops.norm_act_concat([(x, w, b, rm, rv, None) for x, w, b, rm, rv in zip(xs, ws, bs, rms, rvs)], 1, ops.ACT_NONE, exchange=ex)
        gg = torch.autograd.grad(out, xs + ws + bs, t['go'][:2].to(DEV))
    torch.cuda.synchronize()
    close(out, t['y'][:2], FWD, 'sync concat y')
    for i in range(3):
        close(rms[i], t['running_mean'][i], FWD, 'sync concat running_mean branch %d' % i)
        close(rvs[i], t['running_var'][i], FWD, 'sync concat running_var branch %d' % i)
        close(gg[i], t['dx'][i][:2], GRAD, 'sync concat dx branch %d' % i)
        close(gg[3 + i], t['dw'][i], GRAD, 'sync concat dw (local part) branch %d' % i)
        close(gg[6 + i], t['db'][i], GRAD, 'sync concat db (local part) branch %d' % i)
    assert ex.log == ['all_gather', 'all_reduce_sum_'], ex.log


# ---- 7. the launch protocol of every path
FWD_ENTRY, BWD_ENTRY = 'dpf_norm_act_forward', 'dpf_norm_act_backward'


def _entries(ops, rec):
    """What the recorder holds, as names: 'dpf_norm_act_backward <phase>' for the backward, the collective's name for an exchange; cleared."""
    phase = [n for _, n in ops.lib().protos[BWD_ENTRY][1]].index('phase')
    out = [c if isinstance(c, str) else (c[0] if c[0] != BWD_ENTRY else '%s %d' % (BWD_ENTRY, c[1][phase])) for c in rec.calls]
    del rec.calls[:]
    return out


def _protocol_single(ops, rec, mode, exchange):
    N, C, H, W = 2, 5, 6, 8
    x, w, b = [v.to(DEV).requires_grad_() for v in (rnd(N, C, H, W, seed=1) + 0.7, rnd(C, seed=2).abs() + 0.5, rnd(C, seed=3))]
    rm, rv = (torch.zeros(C, device=DEV), torch.ones(C, device=DEV)) if mode in (1, 2) else (None, None)
    ex = None
    if exchange:
        ex = _TwoRankExchange(rnd(3, C, H, W, seed=4).to(DEV), rnd(3, C, H, W, seed=5).to(DEV), torch.zeros(C, device=DEV),
                              torch.ones(C, device=DEV), log=rec.calls)
    if mode == 0:
        w = b = None
    del rec.calls[:]
    y = ops.norm_act(x, w, b, None, None, None, rm, rv, mode, ops.ACT_RELU, exchange=ex)
    fwd = _entries(ops, rec)
    torch.autograd.grad(y, [v for v in (x, w, b) if v is not None], torch.ones_like(y))
    return fwd, _entries(ops, rec)


def _protocol_concat(ops, rec, exchange):
    N, H, W = 2, 6, 8
    dev = lambda v: v.to(DEV).requires_grad_()
    br = [(dev(rnd(N, C, H, W, seed=10 + i)), dev(rnd(C, seed=20 + i).abs() + 0.5), dev(rnd(C, seed=30 + i)), torch.zeros(C, device=DEV),
           torch.ones(C, device=DEV), None) for i, C in enumerate(SYNC_CAT)]
    ex = None
    if exchange:
        ex = _TwoRankExchange([rnd(3, C, H, W, seed=40 + i).to(DEV) for i, C in enumerate(SYNC_CAT)],
                              [rnd(3, C, H, W, seed=50 + i).to(DEV) for i, C in enumerate(SYNC_CAT)],
                              [torch.zeros(C, device=DEV) for C in SYNC_CAT], [torch.ones(C, device=DEV) for C in SYNC_CAT], log=rec.calls)
    del rec.calls[:]
    y = ops.norm_act_concat(br, 1, ops.ACT_NONE, exchange=ex)
    fwd = _entries(ops, rec)
    torch.autograd.grad(y, [v for b in br for v in b[:3]], torch.ones_like(y))
    return fwd, _entries(ops, rec)


def _protocol_conv_bn_concat(ops, rec):
    N, C, H, W = 2, 8, 20, 36
    dev = lambda v: v.to(DEV).requires_grad_()
    x = dev(rnd(N, C, H, W, seed=200))
    br = [(dev(rnd(C, C, 3, 3, seed=201 + i) * 0.2), dev(rnd(C, seed=210 + i).abs() + 0.5), dev(rnd(C, seed=220 + i)),
           torch.zeros(C, device=DEV), torch.ones(C, device=DEV)) for i in range(3)]
    del rec.calls[:]
    y = ops.conv_bn_concat(x, br, (1, 3, 5), True)
    fwd = _entries(ops, rec)
    torch.autograd.grad(y, [x] + [v for b in br for v in b[:3]], torch.ones_like(y))
    return fwd, _entries(ops, rec)


# the dense convolutions ask the library for their workspace sizes before every launch: C entries too, so they are part of the record
_CONV = ['dpf_conv_workspace_floats', 'dpf_conv_stats_slab_doubles', 'dpf_conv_forward_stats']
_WGRAD = ['dpf_conv_wgrad_workspace_floats', 'dpf_conv_wgrad_ws']
_DGRAD = ['dpf_conv_workspace_floats', 'dpf_conv_transpose']
PROTOCOL = {
    # path: (run, entries of the forward, entries of the backward)
    'single mode 0': (lambda o, r: _protocol_single(o, r, 0, False), [FWD_ENTRY], [BWD_ENTRY + ' 3']),
    'single mode 1': (lambda o, r: _protocol_single(o, r, 1, False), ['dpf_bn_stats', FWD_ENTRY], [BWD_ENTRY + ' 3']),
    'single mode 2': (lambda o, r: _protocol_single(o, r, 2, False), ['dpf_bn_eval_stats', FWD_ENTRY], [BWD_ENTRY + ' 3']),
    'single mode 3': (lambda o, r: _protocol_single(o, r, 3, False), ['dpf_bn_stats', FWD_ENTRY], [BWD_ENTRY + ' 3']),
    'single mode 1 exchange': (lambda o, r: _protocol_single(o, r, 1, True),
                               ['dpf_bn_local_moments', 'all_gather', 'dpf_bn_merge_moments', FWD_ENTRY],
                               [BWD_ENTRY + ' 1', 'all_reduce_sum_', BWD_ENTRY + ' 2']),
    'concat': (lambda o, r: _protocol_concat(o, r, False), ['dpf_bn_stats', FWD_ENTRY] * 3, [BWD_ENTRY + ' 0'] * 3),
    'concat exchange': (lambda o, r: _protocol_concat(o, r, True),
                        ['dpf_bn_local_moments'] * 3 + ['all_gather'] + ['dpf_bn_merge_moments', FWD_ENTRY] * 3,
                        [BWD_ENTRY + ' 1'] * 3 + ['all_reduce_sum_'] + [BWD_ENTRY + ' 2'] * 3),
    'conv_bn_concat': (_protocol_conv_bn_concat, _CONV * 3 + ['dpf_bn_finalize_partials', FWD_ENTRY] * 3,
                       ([BWD_ENTRY + ' 0'] + _WGRAD + _DGRAD) * 3),
}


@pytest.mark.parametrize('path', sorted(PROTOCOL))
def test_launch_protocol(path, monkeypatch):
    """The C entries every path of the three normalisation nodes reaches (lib().call and the direct cdll route alike, recorded around the
    library object), with the backward's phase and the collectives of an exchange in their places: literals, read off a run."""
    ops = support.ops()
    rec = support.record_calls(monkeypatch)
    run, fwd, bwd = PROTOCOL[path]
    got = run(ops, rec)
    torch.cuda.synchronize()
    print('%s forward: %r' % (path, got[0]))
    print('%s backward: %r' % (path, got[1]))
    assert got[0] == fwd, (path, got[0])
    assert got[1] == bwd, (path, got[1])
