"""Gradient accumulation, global-norm clipping and norm tracking on the GPU (``-m gpu``), from the kernels of csrc/grad_ctl.hip to the trainer.

The yardstick is torch on the CPU in fp64: ``torch.nn.utils.clip_grad_norm_(params, c, norm_type=2, error_if_nonfinite=False)`` and the
optimisers ``selectors.optimizer_selector`` builds.  What is compared is the UPDATE of an optimiser step, delta = p_after - p_before, and
the state arenas, element by element, under the bound of tests/test_gpu_optim.py (restated here, derived there):

    |delta_hip - delta_64| <= 1e-4 * |delta_64| + 1e-5 * rms(delta_64) + 2^-23 * |p_before|        (state: the first two terms)

The accumulation arena is compared bitwise with the left-to-right fp32 sum, and the reported norm must lie within one float32 ulp of the
fp64 norm of that sum (it is an fp64 value rounded once).
"""
import os
import sys
import time

import numpy as np
import pytest
import torch

from tests import support
from tests.support import DEV

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATES = {'adam': ('m', 'v'), 'sgd': ('buf',), 'rmsprop': ('sq',)}
STATES_TORCH = {'adam': ('exp_avg', 'exp_avg_sq'), 'sgd': ('momentum_buffer',), 'rmsprop': ('square_avg',)}
LR = 1e-3


def one_ulp(norm32, norm64, what):
    """The float32 `norm32` within one float32 ulp of the fp64 `norm64`."""
    ulp = float(np.spacing(np.float32(norm64)))
    print('%s: reported %.9g, fp64 %.17g, off by %.3f ulp' % (what, norm32, norm64, abs(norm32 - norm64) / ulp if ulp else 0.0))
    assert abs(float(norm32) - norm64) <= ulp, (what, norm32, norm64, ulp)


class Reference(object):
    """torch.optim in fp64 over named CPU tensors, built by the project's optimizer_selector, behind torch's clip_grad_norm_.  Before a
    step the parameters are set to the fp32 values the HIP step started from; the optimiser's own state runs on in fp64."""

    def __init__(self, optim, shapes, lr):
        from dualpixelface_amd.selectors import optimizer_selector
        self.optim = optim
        self.params = {k: torch.nn.Parameter(torch.zeros(shape, dtype=torch.float64)) for k, shape in shapes.items()}
        self.opt = optimizer_selector(list(self.params.values()), support.option_set(optim=optim, init_lr=lr))

    def step(self, before, grads, clip, lr=None):
        """before: {name: fp32 tensor}; grads: {name: fp64 tensor or None (= no gradient)}; clip: max norm, 0 = none
        -> ({name: delta in fp64}, the total norm torch measured before clipping)."""
        if lr is not None:
            for group in self.opt.param_groups:
                group['lr'] = lr
        with torch.no_grad():
            for k, p in self.params.items():
                p.copy_(before[k].detach().cpu().double())
        for k, p in self.params.items():
            p.grad = None if grads[k] is None else grads[k].detach().cpu().double().clone()
        with_grad = [p for p in self.params.values() if p.grad is not None]
        total = torch.nn.utils.clip_grad_norm_(with_grad, clip if clip > 0 else float('inf'), norm_type=2, error_if_nonfinite=False)
        self.opt.step()
        return {k: p.detach() - before[k].detach().cpu().double() for k, p in self.params.items()}, float(total)

    def state(self, name, which):
        st = self.opt.state.get(self.params[name], {})
        return st[which] if which in st else torch.zeros_like(self.params[name])


def _gradient_zeros_from_3(n, seed):
    """magnitudes over six decades, both signs, every 7th element exactly 0"""
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (-6.0 * torch.rand(n, generator=g))
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -torch.ones(n), torch.ones(n))
    out = (mag * sign).float()
    out[3::7] = 0.0
    return out


# ------------------------------------------------------------------------------------------------------------------ 1. kernels
LENGTHS = [1, 63, 64, 257, 4099, 256 * 1024 + 5, 3670492]            # the last: StereoDPNet's arena


def _arena(n, off, values=None):
    t = torch.zeros(n + 8, device=DEV)[off:off + n]
    if values is not None:
        t.copy_(values)
    return t


def _launch(optim, p, g, states, ctl):
    from dualpixelface_amd import ops
    if optim == 'adam':
        ops.adam_step_ctl(p, g, states[0], states[1], ctl)
    elif optim == 'sgd':
        ops.sgd_step_ctl(p, g, states[0], ctl)
    else:
        ops.rmsprop_step_ctl(p, g, states[0], ctl)


def _launch_plain(optim, p, g, states, gscale):
    from dualpixelface_amd import ops
    if optim == 'adam':
        ops.adam_step(p, g, states[0], states[1], 1, LR, gscale=gscale)
    elif optim == 'sgd':
        ops.sgd_step(p, g, states[0], LR, gscale=gscale)
    else:
        ops.rmsprop_step(p, g, states[0], LR, gscale=gscale)


def _hyper(optim):
    from dualpixelface_amd import ops
    return [float(x) for x in ops.adam_hyper(1, LR)] if optim == 'adam' else [LR, 0.0]


def _run_fold_finish_step(optim, n, off, grads, p0, clip, gscale, apply=1.0):
    """Three folds into an accumulation arena (the third with the sums in its pass), finish, the optimiser behind the record: every arena
    `off` floats into its allocation -> (acc, ctl, p, states) on the CPU."""
    from dualpixelface_amd import ops
    acc, g, p = _arena(n, off), _arena(n, off), _arena(n, off, p0)
    acc.fill_(float('nan'))                                # the first fold must overwrite, not add
    states = [_arena(n, off) for _ in STATES[optim]]
    ctl = torch.zeros(ops.GRAD_CTL_FLOATS, device=DEV)
    ctl[:2] = torch.tensor(_hyper(optim))
    ctl[4:6] = -7.0                                        # finish must write these (or leave them under apply = 0)
    for k, gk in enumerate(grads):
        g.copy_(gk)
        last = k == len(grads) - 1
        ctl[2], ctl[3] = float(k == 0), apply if last else 0.0
        ops.grad_fold(acc, g, ctl, partials=True)
    ops.grad_finish(n, ctl, gscale, clip)
    _launch(optim, p, acc, states, ctl)
    torch.cuda.synchronize()
    return acc.cpu(), ctl.cpu(), p.cpu(), [s.cpu() for s in states]


def _same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip([a[0], a[1], a[2]] + a[3], [b[0], b[1], b[2]] + b[3]))


@pytest.mark.parametrize('n', LENGTHS)
@pytest.mark.parametrize('optim', ['adam', 'sgd', 'rmsprop'])
def test_kernels_against_torch(optim, n):
    from dualpixelface_amd import ops
    grads = [_gradient_zeros_from_3(n, 300 + k) for k in range(3)]
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(7))
    total = (grads[0] + grads[1]) + grads[2]               # fp32, left to right
    norm64 = float(total.double().pow(2).sum().sqrt())
    assert norm64 > 0
    lo, hi = 0.3 * norm64, 10.0 * norm64                   # below 0.5 * norm: clipping is active at gscale 1 and 0.5
    for gscale in (1.0, 0.5):
        base = _run_fold_finish_step(optim, n, 0, grads, p0, lo, gscale)
        acc, ctl, p, states = base
        what = '%s n %d gscale %g' % (optim, n, gscale)
        # the fold: bitwise the fp32 sum; aligned, offset and repeated runs: the same bits everywhere
        assert torch.equal(acc.view(torch.int32), total.view(torch.int32)), what
        assert _same(base, _run_fold_finish_step(optim, n, 0, grads, p0, lo, gscale)), what + ': two runs differ'
        assert _same(base, _run_fold_finish_step(optim, n, 1, grads, p0, lo, gscale)), what + ': aligned and offset arenas differ'
        # the norm, the multiplier, the clipped step
        one_ulp(float(ctl[ops.GRAD_CTL_NORM]), gscale * norm64, what + ' grad_norm')
        ref = Reference(optim, {'p': (n,)}, LR)
        d64, measured = ref.step({'p': p0}, {'p': total.double() * gscale}, lo)
        assert abs(measured - gscale * norm64) <= 1e-12 * norm64 and lo < measured
        coef = lo / (gscale * norm64 + 1e-6)
        assert abs(float(ctl[ops.GRAD_CTL_GMUL]) - gscale * coef) <= 2.0 ** -23 * gscale * coef, what
        support.within_bound(p.double() - p0.double(), d64['p'], what + ' clipped update', p_before=p0)
        for s, name in zip(states, STATES_TORCH[optim]):
            support.within_bound(s, ref.state('p', name), what + ' state ' + name)
    # c above the norm: coef is exactly 1 and the step is bitwise the unclipped entry point's on the same gradient
    acc, ctl, p, states = _run_fold_finish_step(optim, n, 0, grads, p0, hi, 0.5)
    assert float(ctl[ops.GRAD_CTL_GMUL]) == 0.5
    one_ulp(float(ctl[ops.GRAD_CTL_NORM]), 0.5 * norm64, '%s n %d unclipped grad_norm' % (optim, n))
    pp, gg, ss = p0.clone().to(DEV), total.to(DEV), [torch.zeros(n, device=DEV) for _ in STATES[optim]]
    _launch_plain(optim, pp, gg, ss, 0.5)
    torch.cuda.synchronize()
    assert torch.equal(p, pp.cpu()) and all(torch.equal(a, b.cpu()) for a, b in zip(states, ss)), (optim, n)
    assert not torch.equal(p, p0)
    # clipping off, tracking on: the same step, the norm still reported
    acc0, ctl0, p_0, states0 = _run_fold_finish_step(optim, n, 0, grads, p0, 0.0, 0.5)
    assert torch.equal(p_0, p) and torch.equal(ctl0[4:6], ctl[4:6])
    # apply = 0: the fold still happens, nothing else changes by a bit -- for aligned and offset arenas
    for off in (0, 1):
        acc, ctl, p, states = _run_fold_finish_step(optim, n, off, grads, p0, lo, 1.0, apply=0.0)
        assert torch.equal(acc.view(torch.int32), total.view(torch.int32))
        assert torch.equal(p.view(torch.int32), p0.view(torch.int32)) and all(int((s != 0).sum()) == 0 and not torch.signbit(s).any() for s in states)
        assert ctl[4:6].tolist() == [-7.0, -7.0]
    # one inf: the reported norm is not finite, as torch's is not (only the norm is compared)
    bad = [g.clone() for g in grads]
    bad[1][n // 2] = float('inf')
    for off in (0, 1):
        _, ctl, _, _ = _run_fold_finish_step(optim, n, off, bad, p0, lo, 1.0)
        want = torch.linalg.vector_norm(((bad[0] + bad[1]) + bad[2]).double(), 2)
        assert not torch.isfinite(want) and not np.isfinite(float(ctl[ops.GRAD_CTL_NORM]))
        assert float(ctl[ops.GRAD_CTL_NORM]) == float(want) or (np.isnan(float(ctl[ops.GRAD_CTL_NORM])) and torch.isnan(want))
    # an all-zero gradient: norm 0 and, under RMSprop, an untouched parameter arena
    if optim == 'rmsprop':
        zeros = [torch.zeros(n)] * 3
        for off in (0, 1):
            acc, ctl, p, states = _run_fold_finish_step(optim, n, off, zeros, p0, 1.0, 1.0)
            assert float(ctl[ops.GRAD_CTL_NORM]) == 0.0 and float(ctl[ops.GRAD_CTL_GMUL]) == 1.0
            assert torch.equal(p.view(torch.int32), p0.view(torch.int32)) and int((states[0] != 0).sum()) == 0


def test_stand_alone_sums_equal_the_fused_pass_and_refusals():
    """grad_sumsq over an arena gives the bits the fold's own pass gives (N = 1 and the data-parallel path use it); the C entries refuse
    null pointers, n <= 0 and a short workspace before launching."""
    import ctypes
    from dualpixelface_amd import ops
    from dualpixelface_amd._lib import DpfError, lib
    n = 256 * 1024 + 5
    g = _gradient_zeros_from_3(n, 11)
    want = float(g.double().pow(2).sum().sqrt())
    got = []
    for off in (0, 1):
        arena = _arena(n, off, g)
        ctl = torch.zeros(ops.GRAD_CTL_FLOATS, device=DEV)
        ctl[3] = 1.0
        ops.grad_sumsq(arena)
        ops.grad_finish(n, ctl, 1.0, 0.0)
        acc = _arena(n, off)
        ctl2 = torch.zeros(ops.GRAD_CTL_FLOATS, device=DEV)
        ctl2[2], ctl2[3] = 1.0, 1.0
        ops.grad_fold(acc, arena, ctl2, partials=True)
        ops.grad_finish(n, ctl2, 1.0, 0.0)
        torch.cuda.synchronize()
        got += [float(ctl[5]), float(ctl2[5])]
        assert float(ctl[4]) == 1.0
    assert len(set(got)) == 1, got
    one_ulp(got[0], want, 'stand-alone grad_norm')
    x, ctl = torch.zeros(64, device=DEV), torch.zeros(8, device=DEV)
    ws = torch.zeros(64, dtype=torch.float64, device=DEV)
    ptr, null, st = (lambda t: ctypes.c_void_p(t.data_ptr())), None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cdll = lib().cdll
    assert cdll.dpf_grad_ctl_workspace_bytes(0) == -1 and cdll.dpf_grad_ctl_workspace_bytes(64) == 8
    assert cdll.dpf_grad_ctl_workspace_bytes(3670492) == 8 * 897
    for rc in (cdll.dpf_grad_fold(null, ptr(x), 64, ptr(ctl), null, 0, st), cdll.dpf_grad_fold(ptr(x), null, 64, ptr(ctl), null, 0, st),
               cdll.dpf_grad_fold(ptr(x), ptr(x), 64, null, null, 0, st), cdll.dpf_grad_fold(ptr(x), ptr(x), 0, ptr(ctl), null, 0, st),
               cdll.dpf_grad_fold(ptr(x), ptr(x), 64, ptr(ctl), ptr(ws), 4, st),
               cdll.dpf_grad_sumsq(null, 64, ptr(ws), 512, st), cdll.dpf_grad_sumsq(ptr(x), 64, null, 512, st),
               cdll.dpf_grad_sumsq(ptr(x), -1, ptr(ws), 512, st), cdll.dpf_grad_sumsq(ptr(x), 64, ptr(ws), 7, st),
               cdll.dpf_grad_finish(null, 512, 64, 1.0, 0.0, ptr(ctl), st), cdll.dpf_grad_finish(ptr(ws), 512, 64, 1.0, 0.0, null, st),
               cdll.dpf_grad_finish(ptr(ws), 512, 0, 1.0, 0.0, ptr(ctl), st), cdll.dpf_grad_finish(ptr(ws), 512, 64, 1.0, -1.0, ptr(ctl), st),
               cdll.dpf_adam_step_ctl(ptr(x), ptr(x), ptr(x), ptr(x), 64, null, 0.9, 0.999, 1e-5, st),
               cdll.dpf_adam_step_ctl(ptr(x), ptr(x), ptr(x), ptr(x), 0, ptr(ctl), 0.9, 0.999, 1e-5, st),
               cdll.dpf_sgd_step_ctl(ptr(x), ptr(x), ptr(x), null, 64, null, 0.9, 2e-4, st),
               cdll.dpf_sgd_step_ctl(null, ptr(x), ptr(x), null, 64, ptr(ctl), 0.9, 2e-4, st),
               cdll.dpf_rmsprop_step_ctl(ptr(x), ptr(x), ptr(x), 64, null, 0.99, 1e-5, st),
               cdll.dpf_rmsprop_step_ctl(ptr(x), ptr(x), null, 64, ptr(ctl), 0.99, 1e-5, st)):
        assert rc == -1
    with pytest.raises(DpfError):
        ops.grad_fold(x, x, torch.zeros(4, device=DEV))
    torch.cuda.synchronize()
    assert int((x != 0).sum()) == 0


# ------------------------------------------------------------------------------------------------------------------ whole steps
def _batch(seed, B=2, H=32, W=48):
    from dualpixelface_amd.recipe import synthetic_batch
    return {k: v.to(DEV) for k, v in synthetic_batch(B, H, W, seed=seed, mask_mode='bern').items()}


def test_eager_groups_against_a_twin_by_hand():
    """STEREODPNET, Adam, N = 3, clipping below the first group's norm, deterministic mode: two full groups and a short one of a single
    batch, against a twin from the same seed that runs forward + backward per micro-batch, sums the .grads in fp32 in order, scales by
    1 / N, clips with torch in fp64 and steps torch's Adam in fp64 (the twin takes over the stepped parameters after each group, so that
    each group is compared on its own)."""
    from dualpixelface_amd import ops
    N, lr = 3, 1e-4
    with ops.deterministic_mode():
        model = support.plugin('adam', step_graph=False, accumulate_grad_batches=N, gradient_clip_val=1.0)
        twin = support.plugin('adam', step_graph=False)
        layout = model._layout
        pd = dict(twin.named_parameters())
        ref = Reference('adam', {name: shape for name, _, _, shape in layout}, lr)
        seen_norm = 0
        micro = 0
        for gi, size in enumerate((3, 3, 1)):
            batches = [_batch(80 + micro + k) for k in range(size)]
            # the twin: the group's gradient by hand
            total, had = None, set()
            for b in batches:
                for p in twin.parameters():
                    p.grad = None
                twin.forward(b)['final_loss'].backward()
                flat = torch.cat([(pd[name].grad if pd[name].grad is not None else torch.zeros_like(pd[name])).reshape(-1).float()
                                  for name, _, _, _ in layout])
                had |= {name for name, _, _, _ in layout if pd[name].grad is not None}
                total = flat.clone() if total is None else total + flat
            torch.cuda.synchronize()
            norm64 = float((total.double().cpu() / N).pow(2).sum().sqrt())
            if gi == 0:
                model.option.gradient_clip_val = 0.5 * norm64          # below the measured norm of the first group
            clip = model.option.gradient_clip_val
            # the model: the same micro-batches through train_step
            before = support.named(model, model.flat_parameters())
            for k, b in enumerate(batches):
                last = k == size - 1
                res = model.train_step(b, lr=lr, last_in_epoch=(last and size < N))
                micro += 1
                assert ('grad_norm' in res) == last, (gi, k, sorted(res))
                assert torch.isfinite(res['final_loss'])
            torch.cuda.synchronize()
            seen_norm += 1
            what = 'group %d' % gi
            assert torch.equal(model._adam['acc'].view(torch.int32), total.view(torch.int32)), what + ': accumulation arena'
            one_ulp(float(res['grad_norm']), norm64, what + ' grad_norm')
            grads = support.named(model, total.double() / N)
            d64, measured = ref.step(before, {k: (g if k in had else None) for k, g in grads.items()}, clip)
            assert abs(measured - norm64) <= 1e-9 * norm64
            if gi == 0:
                assert clip < measured
            after = support.named(model, model.flat_parameters())
            m, v = support.named(model, model._adam['m']), support.named(model, model._adam['v'])
            for name in before:
                support.within_bound(after[name].double() - before[name].double(), d64[name], '%s %s' % (what, name), p_before=before[name])
                support.within_bound(m[name], ref.state(name, 'exp_avg'), '%s m %s' % (what, name))
                support.within_bound(v[name], ref.state(name, 'exp_avg_sq'), '%s v %s' % (what, name))
            assert model._adam['step'] == gi + 1
            with torch.no_grad():
                twin.flat_parameters().copy_(model.flat_parameters())
        assert micro == 7 and model._adam['step'] == 3 and seen_norm == 3
        sa, sb = model.state_dict(), twin.state_dict()
        tracked = [k for k in sa if k.endswith('num_batches_tracked')]
        # (every micro-step counts: 7 per use of a layer in the forward pass -- the shared feature extractor runs twice)
        counts = {k: (int(sa[k]), int(sb[k])) for k in tracked}
        assert tracked and all(x == y and x >= 7 and x % 7 == 0 for x, y in counts.values()), sorted(set(counts.values()))
        assert min(x for x, _ in counts.values()) == 7
        stats = [k for k in sa if k.endswith(('running_mean', 'running_var'))]
        assert stats and all(torch.equal(sa[k], sb[k]) for k in stats)
        assert not getattr(model, '_graph_states', None)


def test_stereonet_sgd_parameter_without_gradient_is_left_alone_under_accumulation():
    """The live-mask path under accumulation: StereoNet's unused conv2 weight (no gradient in any micro-step) keeps its bits over two
    groups of N = 2, weight decay included, and its momentum buffer stays zero; a used weight moves."""
    name, used = 'feature_extraction.residual_blocks.0.conv2.0.weight', 'feature_extraction.residual_blocks.0.conv1.0.0.weight'
    model = support.plugin('sgd', 'STEREONET', 'train_faceDP_stereonet', accumulate_grad_batches=2, gradient_clip_val=1.0)
    pd = dict(model.named_parameters())
    before = {k: pd[k].detach().clone() for k in (name, used)}
    norms = []
    for i in range(4):
        res = model.train_step(_batch(13 + i, 2, 64, 96), None, lr=1e-4)
        assert torch.isfinite(res['final_loss']) and ('grad_norm' in res) == (i % 2 == 1)
        norms += [float(res['grad_norm'])] if 'grad_norm' in res else []
    torch.cuda.synchronize()
    assert len(norms) == 2 and all(np.isfinite(x) and x > 0 for x in norms)
    assert torch.equal(before[name], pd[name].detach())
    assert not torch.equal(before[used], pd[used].detach())
    off, numel = next((off, numel) for n, off, numel, _ in model._layout if n == name)
    assert int((model._optim['buf'][off:off + numel] != 0).sum()) == 0
    assert int(model._optim['live'][off:off + numel].sum()) == 0 and int(model._optim['live'].sum()) > 0
    assert model._adam is None


@pytest.mark.parametrize('optim', ['adam', 'rmsprop'])
def test_graph_replays_equal_an_eager_twin(optim):
    """N = 2, clipping on, deterministic mode: twelve micro-steps with step_graph on (state creation, two warm-ups, capture on the fourth,
    replays after) leave parameters, optimiser state and BatchNorm buffers bitwise as an eager twin's, with exactly one captured graph."""
    from dualpixelface_amd import ops
    clip = 0.05
    with ops.deterministic_mode():
        a = support.plugin(optim, step_graph=True, accumulate_grad_batches=2, gradient_clip_val=clip)
        b = support.plugin(optim, step_graph=False, accumulate_grad_batches=2, gradient_clip_val=clip)
        norms = []
        for i in range(12):
            batch, lr = _batch(60 + i), 1e-4 * 0.5 ** (i // 4)
            ra, rb = a.train_step(batch, lr=lr), b.train_step(batch, lr=lr)
            torch.cuda.synchronize()
            what = '%s call %d' % (optim, i)
            assert set(ra) == set(rb) and ('grad_norm' in ra) == (i % 2 == 1), (what, sorted(ra), sorted(rb))
            for k, v in rb.items():
                if torch.is_tensor(v):
                    assert torch.equal(ra[k], v), (what, k)
            norms += [float(ra['grad_norm'])] if 'grad_norm' in ra else []
            sta, stb = (optim_state(m, optim) for m in (a, b))
            assert torch.equal(a.flat_parameters(), b.flat_parameters()), what
            assert all(torch.equal(sta[k], stb[k]) for k in STATES[optim] + ('acc',)), what
            sa, sb = a.state_dict(), b.state_dict()
            diff = [k for k in sb if not torch.equal(sa[k], sb[k])]
            assert not diff, (what, diff[:8])
        assert len(norms) == 6 and all(np.isfinite(x) for x in norms) and max(norms) > clip, norms      # clipping was active
        if optim == 'adam':
            assert a._adam['step'] == b._adam['step'] == 6
        states = [(st['calls'], st['graph'] is not None, bool(st.get('failed'))) for st in a._graph_states]
        assert states == [(1, False, False), (11, True, False)], states
        assert not getattr(b, '_graph_states', None)


def optim_state(model, optim):
    return model._adam if optim == 'adam' else model._optim


def test_trainer_fit_groups_logs_and_checkpoints(tmp_path):
    """Trainer.fit over 7 synthetic batches at N = 3 for one epoch: 3 optimiser steps in the log, each with a finite grad_norm; the
    checkpoint loads into a fresh model and equals the trained one; with every knob at its default the same data logs 7 steps."""
    from dualpixelface_amd.synthetic_data import synthetic_loader
    from dualpixelface_amd.trainer import Trainer
    loader = synthetic_loader(14, 32, 48, batch_size=2, seed=3)
    kw = dict(epoch=1, scheduler='none', accumulate_grad_batches=3, gradient_clip_val=0.05)
    a = support.plugin('adam', **kw)
    ta = Trainer(a.option, str(tmp_path / 'a'), log_every=1, rank=0, world_size=1)
    ta.fit(a, loader, None)
    steps = [r for r in ta.history if 'step' in r]
    assert [r['step'] for r in steps] == [1, 2, 3] and ta.global_step == 3 and a._adam['step'] == 3
    assert all(np.isfinite(r['grad_norm']) and r['grad_norm'] > 0 and np.isfinite(r['final_loss']) for r in steps), steps
    ck = torch.load(ta.checkpoint_path(0), map_location='cpu', weights_only=False)
    assert set(ck['optimizer_states'][0]) == {'kind', 'step', 'm', 'v'} and ck['optimizer_states'][0]['step'] == 3
    b = support.plugin('adam', **kw)
    with torch.no_grad():
        b.flat_parameters().mul_(0.5)
    tb = Trainer(b.option, str(tmp_path / 'b'), rank=0, world_size=1)
    tb.load_checkpoint(b, ta.checkpoint_path(0))
    assert tb.epoch == 1 and tb.global_step == 3 and b._adam['step'] == 3
    sa, sb = a.state_dict(), b.state_dict()
    assert set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert torch.equal(a._adam['m'], b._adam['m']) and torch.equal(a._adam['v'], b._adam['v'])
    c = support.plugin('adam', epoch=1, scheduler='none')
    tc = Trainer(c.option, str(tmp_path / 'c'), log_every=1, rank=0, world_size=1)
    tc.fit(c, loader, None)
    steps = [r for r in tc.history if 'step' in r]
    assert [r['step'] for r in steps] == list(range(1, 8)) and all('grad_norm' not in r for r in steps) and c._adam['step'] == 7
    assert c._adam.get('acc') is None


# ------------------------------------------------------------------------------------------------------------------ 6. two ranks
# RCCL refuses two ranks on one device ("Duplicate GPU detected", as tests/test_gpu_distributed.py records), so the two ranks of the one
# test GPU talk over gloo, like test_two_ranks_on_one_gpu_sgd, and 'nccl' is run with the one rank it accepts there (below).
BACKEND = 'gloo'


def _rank_batch(rank, seed):
    from dualpixelface_amd.recipe import synthetic_batch
    full = synthetic_batch(4, 32, 48, seed=seed)
    return {k: v[2 * rank:2 * rank + 2].to(DEV) for k, v in full.items()}


def _accum_rank(rank, world, port, out_dir):
    """One of two ranks on the one GPU: two optimiser steps of N = 2 micro-steps with clipping; writes where it ended, the norms it
    reported and how often its reducer exchanged."""
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0')
    import torch.distributed as dist
    from dualpixelface_amd.distributed import broadcast_flat, init_from_env, make_reducer
    torch.cuda.set_device(0)
    init_from_env(BACKEND)
    try:
        model = support.plugin('adam', accumulate_grad_batches=2, gradient_clip_val=0.05)
        if rank == 1:                                      # broadcast must repair this
            with torch.no_grad():
                model.flat_parameters().mul_(1.5)
        broadcast_flat(model.flat_parameters(), 0)
        reducer = make_reducer(model)
        norms, calls = [], []
        for i in range(4):
            res = model.train_step(_rank_batch(rank, 11 + i), reducer, lr=1e-3)
            torch.cuda.synchronize()
            calls.append(reducer.collective_calls)
            assert ('grad_norm' in res) == (i % 2 == 1)
            norms += [float(res['grad_norm'])] if 'grad_norm' in res else []
        torch.save({'params': model.flat_parameters().detach().cpu().clone(), 'm': model._adam['m'].detach().cpu().clone(),
                    'acc': model._adam['acc'].detach().cpu().clone(), 'norms': norms, 'calls': calls,
                    'buckets': len(reducer.buckets), 'step': model._adam['step']}, os.path.join(out_dir, 'rank%d.pt' % rank))
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_accumulate_and_clip(tmp_path):
    """Both ranks end with bitwise equal parameters and equal grad_norm after 2 optimiser steps of N = 2; the reducer exchanged once per
    optimiser step (one all-reduce per bucket), not once per micro-step."""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    port = 39500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_accum_rank, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    deadline = time.time() + 300                           # each child under its own time limit; the first failure ends the test
    try:
        while any(p.is_alive() for p in procs):
            failed = [p for p in procs if not p.is_alive() and p.exitcode != 0]
            assert not failed, 'a rank failed (exit code %r)' % failed[0].exitcode
            assert time.time() < deadline, 'the ranks did not finish in time'
            time.sleep(0.5)
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
            p.join(30)
    assert [p.exitcode for p in procs] == [0, 0], [p.exitcode for p in procs]
    r0, r1 = (torch.load(str(tmp_path / ('rank%d.pt' % r)), weights_only=False) for r in range(2))
    assert torch.equal(r0['params'], r1['params']) and torch.equal(r0['m'], r1['m']) and torch.equal(r0['acc'], r1['acc'])
    assert r0['norms'] == r1['norms'] and len(r0['norms']) == 2 and all(np.isfinite(x) and x > 0 for x in r0['norms'])
    nb = r0['buckets']
    assert r0['calls'] == r1['calls'] == [0, nb, nb, 2 * nb], (r0['calls'], nb)
    assert r0['step'] == r1['step'] == 2


def _nccl_one_rank(port, out_dir):
    """One rank, backend 'nccl': the all-reduce of the ACCUMULATED arena goes through ProcessGroupNCCL (its own stream, work.wait() before
    the norm); a one-rank all-reduce(SUM) is the identity, so the run must equal a twin without a reducer bit for bit."""
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from dualpixelface_amd import ops
    from dualpixelface_amd.distributed import make_reducer
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', init_method='tcp://127.0.0.1:%d' % port, rank=0, world_size=1)
    try:
        with ops.deterministic_mode():
            kw = dict(step_graph=False, accumulate_grad_batches=2, gradient_clip_val=0.05)
            model, twin = support.plugin('adam', **kw), support.plugin('adam', **kw)
            reducer = make_reducer(model, force_collectives=True)
            assert reducer.collectives and reducer.world_size == 1
            calls, norms, same = [], [], []
            for i in range(4):
                batch = _batch(11 + i)
                ra, rb = model.train_step(batch, reducer, lr=1e-3), twin.train_step(batch, lr=1e-3)
                torch.cuda.synchronize()
                calls.append(reducer.collective_calls)
                same.append(set(ra) == set(rb) and torch.equal(model.flat_parameters(), twin.flat_parameters())
                            and torch.equal(model._adam['acc'], twin._adam['acc']) and torch.equal(model._adam['v'], twin._adam['v']))
                norms += [(float(ra['grad_norm']), float(rb['grad_norm']))] if 'grad_norm' in ra else []
            torch.save({'calls': calls, 'norms': norms, 'same': same, 'buckets': len(reducer.buckets), 'backend': dist.get_backend(),
                        'step': model._adam['step']}, os.path.join(out_dir, 'nccl.pt'))
    finally:
        dist.destroy_process_group()


def test_one_rank_nccl_exchanges_the_accumulated_arena_once_per_optimiser_step(tmp_path):
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    p = mp.get_context('spawn').Process(target=_nccl_one_rank, args=(port, str(tmp_path)))
    p.start()
    p.join(300)
    if p.is_alive():
        p.terminate()
        p.join(30)
    assert p.exitcode == 0, 'nccl worker failed (exit code %r)' % (p.exitcode,)
    out = torch.load(str(tmp_path / 'nccl.pt'), weights_only=False)
    nb = out['buckets']
    assert out['backend'] == 'nccl' and out['calls'] == [0, nb, nb, 2 * nb] and out['step'] == 2, out
    assert all(out['same']), out['same']
    assert len(out['norms']) == 2 and all(a == b and np.isfinite(a) and a > 0 for a, b in out['norms']), out['norms']
