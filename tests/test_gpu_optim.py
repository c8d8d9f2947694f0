"""The fused SGD and RMSprop steps on the GPU (``-m gpu``), from the kernels to the trainer.

The yardstick throughout is ``torch.optim`` on the CPU in fp64, constructed by ``selectors.optimizer_selector`` so that the
hyper-parameters under test are the ones the config key ``optim`` selects.  What is compared is the UPDATE of a step,
delta = p_after - p_before (at lr 1e-4 the whole update hides inside any relative tolerance on p itself), and the state arena:

    |delta_hip - delta_64| <= 1e-4 * |delta_64| + 1e-5 * rms(delta_64) + 2^-23 * |p_before|        (state: the first two terms)

The first two terms are the project's element-wise bound (close_elem of test_gpu_ops.py).  The third is derived:
storing p in fp32 costs up to half an ulp of p, and the bound allows one full ulp.  Measured on an MI355X over every check of this
file: the worst excess over the bound is negative everywhere (closest -4.5e-13 on an update, -2.0e-27 on a state arena), so the ulp
term stays at one ulp.
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
STATE = {'sgd': 'buf', 'rmsprop': 'sq'}
STATE_TORCH = {'sgd': 'momentum_buffer', 'rmsprop': 'square_avg'}


class Reference(object):
    """torch.optim in fp64 over named CPU tensors, built by the project's optimizer_selector.  Before a step the parameters are set to the
    fp32 values the HIP step started from; the optimiser's own state runs on in fp64."""

    def __init__(self, optim, shapes, lr):
        from dualpixelface_amd.selectors import optimizer_selector
        self.optim = optim
        self.params = {k: torch.nn.Parameter(torch.zeros(shape, dtype=torch.float64)) for k, shape in shapes.items()}
        self.opt = optimizer_selector(list(self.params.values()), support.option_set(optim=optim, init_lr=lr))

    def step(self, before, grads, lr=None):
        """before: {name: fp32 tensor}; grads: {name: tensor or None (= the parameter had no gradient)} -> {name: delta in fp64}."""
        if lr is not None:
            for group in self.opt.param_groups:
                group['lr'] = lr
        with torch.no_grad():
            for k, p in self.params.items():
                p.copy_(before[k].detach().cpu().double())
        for k, p in self.params.items():
            p.grad = None if grads[k] is None else grads[k].detach().cpu().double()
        self.opt.step()
        return {k: p.detach() - before[k].detach().cpu().double() for k, p in self.params.items()}

    def state(self, name):
        st = self.opt.state.get(self.params[name], {})
        return st[STATE_TORCH[self.optim]] if STATE_TORCH[self.optim] in st else torch.zeros_like(self.params[name])


def _gradient_zeros_from_0(n, seed):
    """magnitudes over six decades, both signs, every 7th element exactly 0"""
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (-6.0 * torch.rand(n, generator=g))
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -torch.ones(n), torch.ones(n))
    out = (mag * sign).float()
    out[::7] = 0.0
    return out


N = 10007
DEAD = ((1001, 1338), (9990, N))                           # ranges a mask takes out (the second one reaches into the scalar tail)


@pytest.mark.parametrize('gscale', [1.0, 0.125])
@pytest.mark.parametrize('lr', [1e-2, 1e-4])
@pytest.mark.parametrize('case', ['sgd', 'sgd_masked', 'rmsprop'])
def test_kernels_against_torch_optim(case, lr, gscale):
    """Four steps over an arena of odd length against torch.optim in fp64 fed grad * gscale, per step.  Under the mask the reference holds
    the dead ranges as parameters of their own without a gradient, and the HIP side must leave them -- parameter and buffer -- bitwise."""
    from dualpixelface_amd import ops
    optim = case.split('_')[0]
    cuts = sorted({0, N} | ({c for r in DEAD for c in r} if case == 'sgd_masked' else set()))
    segs = [(lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
    dead = set(DEAD) if case == 'sgd_masked' else set()
    ref = Reference(optim, {seg: (seg[1] - seg[0],) for seg in segs}, lr)
    p = torch.randn(N, generator=torch.Generator().manual_seed(7)).to(DEV)
    state = torch.zeros(N, device=DEV)
    live = None
    if dead:
        live = torch.ones(N, dtype=torch.uint8, device=DEV)
        for lo, hi in dead:
            live[lo:hi] = 0
    p0 = p.clone()
    for step in range(4):
        g = _gradient_zeros_from_0(N, 100 + step)
        before = p.clone()
        if optim == 'sgd':
            ops.sgd_step(p, g.to(DEV), state, lr, gscale=gscale, live=live)
        else:
            ops.rmsprop_step(p, g.to(DEV), state, lr, gscale=gscale)
        torch.cuda.synchronize()
        d64 = ref.step({seg: before[seg[0]:seg[1]] for seg in segs},
                       {seg: (None if seg in dead else g[seg[0]:seg[1]].double() * gscale) for seg in segs})
        what = '%s lr %g gscale %g step %d' % (case, lr, gscale, step)
        support.within_bound(p.double() - before.double(), torch.cat([d64[seg] for seg in segs]), what + ' update', p_before=before)
        support.within_bound(state, torch.cat([ref.state(seg) for seg in segs]), what + ' state')
    for lo, hi in dead:
        assert torch.equal(p[lo:hi], p0[lo:hi]) and int((state[lo:hi] != 0).sum()) == 0 and not torch.signbit(state[lo:hi]).any()
    assert not torch.equal(p[:1001], p0[:1001])


@pytest.mark.parametrize('optim', ['sgd', 'rmsprop'])
def test_device_lr_variant_and_unaligned_arenas_are_bitwise_the_same(optim):
    """The rate from device memory gives the same bits as the rate as an argument; so do arenas that start off a 16-byte boundary
    (a scalar head of three elements) and arenas that are never aligned together (everything one by one)."""
    from dualpixelface_amd import ops
    lr = 1e-2
    dead = DEAD if optim == 'sgd' else ()

    def run(device_lr, offsets):
        arenas = []
        for k, off in enumerate(offsets):                  # param, grad, state as views `off` floats into their allocations
            arenas.append(torch.zeros(N + 8, device=DEV)[off:off + N])
        p, g, state = arenas
        p.copy_(torch.randn(N, generator=torch.Generator().manual_seed(7)))
        live = None
        if dead:
            live = torch.ones(N, dtype=torch.uint8, device=DEV)
            for lo, hi in dead:
                live[lo:hi] = 0
        lr_dev = torch.full((1,), lr, dtype=torch.float32, device=DEV)
        for step in range(3):
            g.copy_(_gradient_zeros_from_0(N, 200 + step))
            if optim == 'sgd':
                if device_lr:
                    ops.sgd_step_lr(p, g, state, lr_dev, gscale=0.5, live=live)
                else:
                    ops.sgd_step(p, g, state, lr, gscale=0.5, live=live)
            elif device_lr:
                ops.rmsprop_step_lr(p, g, state, lr_dev, gscale=0.5)
            else:
                ops.rmsprop_step(p, g, state, lr, gscale=0.5)
        torch.cuda.synchronize()
        return p.clone(), state.clone()

    base = run(False, (0, 0, 0))
    assert int((base[1] != 0).sum()) > N // 2
    for device_lr, offsets in ((True, (0, 0, 0)), (False, (1, 1, 1)), (True, (1, 1, 1)), (False, (0, 1, 2)), (True, (2, 0, 3))):
        got = run(device_lr, offsets)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), (optim, device_lr, offsets)


def _without_gradient(model, batch):
    """Names of the parameters autograd leaves without a gradient on this batch -- asked of autograd itself, on a model of its own:
    every .grad cleared, one forward + backward, which .grad is still None."""
    for p in model.parameters():
        p.grad = None
    model(batch)['final_loss'].backward()
    torch.cuda.synchronize()
    return {name for name, _, _, _ in model._layout if dict(model.named_parameters())[name].grad is None}


def _golden_batch(golden_dir):
    g = np.load(golden_dir + '/e2e_train_32x48_b2.npz')
    return {k[3:]: torch.from_numpy(g[k]).to(DEV) for k in g.files if k.startswith('in_')}


@pytest.mark.parametrize('optim', ['sgd', 'rmsprop'])
def test_whole_eager_step_against_torch_optim(golden_dir, optim):
    """Three eager train steps of STEREODPNET on the golden batch.  The gradients each step used are read back from the arena and drive
    torch.optim in fp64 from the same parameters (no gradient where autograd gave none): every parameter tensor's update must meet the
    bound, which isolates the optimiser from the network's own gradient noise."""
    batch = _golden_batch(golden_dir)
    unused = _without_gradient(support.plugin(optim, step_graph=False), batch)
    model = support.plugin(optim, step_graph=False)
    lr = float(model.option.init_lr)
    ref = Reference(optim, {name: shape for name, _, _, shape in model._layout}, lr)
    for step in range(3):
        before = support.named(model, model.flat_parameters())
        res = model.train_step(batch)
        torch.cuda.synchronize()
        assert torch.isfinite(res['final_loss'])
        grads = support.named(model, model.flat_gradients(zero=False))
        after = support.named(model, model.flat_parameters())
        d64 = ref.step(before, {k: (None if k in unused else g) for k, g in grads.items()})
        for name in before:
            what = '%s step %d %s' % (optim, step, name)
            support.within_bound(after[name].double() - before[name].double(), d64[name], what, p_before=before[name])
        state = support.named(model, model._optim[STATE[optim]])
        for name in before:
            support.within_bound(state[name], ref.state(name), '%s step %d state %s' % (optim, step, name))
    assert model._adam is None and model._optim['kind'] == optim
    assert not getattr(model, '_graph_states', None)


@pytest.mark.parametrize('optim', ['sgd', 'rmsprop'])
def test_stereonet_parameter_without_gradient_is_left_alone(optim):
    """StereoNet's BasicBlock never applies conv2 (modules.py:19-27): its weight has no gradient, torch.optim skips it, and so must the
    fused step -- under SGD weight decay would otherwise shrink it every step."""
    from dualpixelface_amd.recipe import synthetic_batch
    name, used = 'feature_extraction.residual_blocks.0.conv2.0.weight', 'feature_extraction.residual_blocks.0.conv1.0.0.weight'
    batch = {k: v.to(DEV) for k, v in synthetic_batch(2, 64, 96, seed=13).items()}
    model = support.plugin(optim, 'STEREONET', 'train_faceDP_stereonet')
    assert name in _without_gradient(support.plugin(optim, 'STEREONET', 'train_faceDP_stereonet'), batch)
    pd = dict(model.named_parameters())
    before = {k: pd[k].detach().clone() for k in (name, used)}
    for _ in range(2):
        res = model.train_step(batch, None, lr=1e-4)
        assert torch.isfinite(res['final_loss'])
    torch.cuda.synchronize()
    assert torch.equal(before[name], pd[name].detach())
    assert not torch.equal(before[used], pd[used].detach())
    off, numel = next((off, numel) for n, off, numel, _ in model._layout if n == name)
    assert int((model._optim[STATE[optim]][off:off + numel] != 0).sum()) == 0
    assert model._adam is None


def _assert_optim_twins_equal(a, b, ra, rb, what, optim):
    """Graph-mode model `a` and eager twin `b` after the same call: results, parameters, optimiser state and every state_dict tensor, bitwise."""
    assert set(ra) == set(rb), (what, sorted(ra), sorted(rb))
    for k, v in rb.items():
        if torch.is_tensor(v):
            assert torch.equal(ra[k], v), (what, k)
    assert torch.equal(a.flat_parameters(), b.flat_parameters()), what
    assert a._adam is None and b._adam is None
    assert a._optim['kind'] == b._optim['kind'] == optim
    assert torch.equal(a._optim[STATE[optim]], b._optim[STATE[optim]]), what
    sa, sb = a.state_dict(), b.state_dict()
    assert set(sa) == set(sb), what
    diff = [k for k in sb if not torch.equal(sa[k], sb[k])]
    assert not diff, (what, diff[:8])


@pytest.mark.parametrize('optim', ['sgd', 'rmsprop'])
def test_graph_replays_equal_an_eager_twin(optim):
    """Deterministic mode: the first call creates the optimiser state, two warm-ups follow, the fourth call captures and replays, three
    more replay -- with the rate halved twice on the way, as StepLR does between epochs.  After every call the graph-mode model and
    its eager twin hold the same bits."""
    from dualpixelface_amd import ops
    from dualpixelface_amd.recipe import synthetic_batch
    lrs = [1e-4] * 4 + [5e-5, 2.5e-5, 2.5e-5]
    with ops.deterministic_mode():
        a, b = support.plugin(optim, step_graph=True), support.plugin(optim, step_graph=False)
        for i, lr in enumerate(lrs):
            batch = {k: v.to(DEV) for k, v in synthetic_batch(2, 32, 48, seed=60 + i, mask_mode='bern').items()}
            ra = a.train_step(batch, lr=lr)
            rb = b.train_step(batch, lr=lr)
            torch.cuda.synchronize()
            _assert_optim_twins_equal(a, b, ra, rb, '%s call %d' % (optim, i), optim)
            if i == 2:
                assert a._graph_state['graph'] is None
        states = [(st['calls'], st['graph'] is not None, bool(st.get('failed'))) for st in a._graph_states]
        assert states == [(1, False, False), (6, True, False)], states
        assert not getattr(b, '_graph_states', None)


def test_trainer_resume_under_sgd_and_refusal_under_adam(tmp_path):
    """optim = 'sgd' through Trainer.fit: three epochs uninterrupted against a second model resumed from the epoch-1 checkpoint (the
    criterion of test_gpu_trainer.py's Adam test); the checkpoint says flat_sgd; resuming it under optim = 'adam' is refused with
    nothing restored."""
    from dualpixelface_amd.synthetic_data import synthetic_loader
    from dualpixelface_amd.trainer import Trainer
    opt = support.option_set(optim='sgd', epoch=3, init_lr=1e-3, scheduler='explr')
    loader = synthetic_loader(4, 32, 48, batch_size=2, seed=3)
    a = support.plugin('sgd', epoch=3, init_lr=1e-3, scheduler='explr')
    ta = Trainer(opt, str(tmp_path / 'a'), rank=0, world_size=1)
    ta.fit(a, loader, None)
    assert ta.global_step == 6 and all(os.path.exists(ta.checkpoint_path(e)) for e in range(3))
    ck = torch.load(ta.checkpoint_path(1), map_location='cpu', weights_only=False)
    st = ck['optimizer_states'][0]
    assert st['kind'] == 'flat_sgd' and set(st) == {'kind', 'buf'}
    assert st['buf'].shape == (a.flat_parameters().numel(),) and float(st['buf'].abs().max()) > 0
    opt.load_model = ta.checkpoint_path(1)
    b = support.plugin('sgd', epoch=3, init_lr=1e-3, scheduler='explr')
    with torch.no_grad():
        b.flat_parameters().mul_(0.5)                      # the checkpoint must overwrite this
    tb = Trainer(opt, str(tmp_path / 'b'), rank=0, world_size=1)
    tb.fit(b, loader, None)
    assert tb.epoch == 3 and tb.global_step == 6
    pa, pb = a.flat_parameters().cpu(), b.flat_parameters().cpu()
    assert torch.isfinite(pa).all() and torch.isfinite(pb).all()
    diff = (pa - pb).abs()
    print('resume under sgd: fraction off by > 1e-5: %.3e, max %.3e' % ((diff > 1e-5).float().mean().item(), diff.max().item()))
    assert (diff > 1e-5).float().mean().item() <= 5e-3 and diff.max().item() <= 1.1e-3, ((diff > 1e-5).float().mean().item(), diff.max().item())
    assert a._adam is None and b._adam is None and b._optim['kind'] == 'sgd'
    sa, sb = a.state_dict(), b.state_dict()
    k = 'feature_extraction.firstconv.0.1.running_var'
    assert torch.allclose(sa[k].cpu(), sb[k].cpu(), rtol=1e-4)
    assert int(sa['feature_extraction.firstconv.0.1.num_batches_tracked']) == int(sb['feature_extraction.firstconv.0.1.num_batches_tracked'])
    # the same file under optim = 'adam'
    opt_adam = support.option_set(optim='adam', epoch=3, init_lr=1e-3, scheduler='explr')
    c = support.plugin('adam')
    with torch.no_grad():
        c.flat_parameters().mul_(0.5)
    before = {k: v.detach().clone() for k, v in c.state_dict().items()}
    tc = Trainer(opt_adam, str(tmp_path / 'c'), rank=0, world_size=1)
    with pytest.raises(ValueError, match='Nothing was restored'):
        tc.load_checkpoint(c, ta.checkpoint_path(1))
    after = c.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    assert c._adam is None and c._optim is None and tc.epoch == 0 and tc.global_step == 0


H, W = 32, 48


def _rank_batch(rank):
    from dualpixelface_amd.recipe import synthetic_batch
    full = synthetic_batch(4, H, W, seed=11)
    return {k: v[2 * rank:2 * rank + 2].to(DEV) for k, v in full.items()}


def _sgd_rank(rank, world, port, out_dir):
    """One of two ranks on the one GPU (gloo): two SGD steps; writes what each step started from, the summed gradient it used and
    where it ended."""
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0')
    import torch.distributed as dist
    from dualpixelface_amd.distributed import broadcast_flat, init_from_env, make_reducer
    torch.cuda.set_device(0)
    init_from_env('gloo')
    try:
        model = support.plugin('sgd')
        if rank == 1:                                      # broadcast must repair this
            with torch.no_grad():
                model.flat_parameters().mul_(1.5)
        broadcast_flat(model.flat_parameters(), 0)
        reducer = make_reducer(model)
        batch = _rank_batch(rank)
        steps = []
        for _ in range(2):
            before = model.flat_parameters().detach().cpu().clone()
            model.train_step(batch, reducer, lr=1e-3)
            torch.cuda.synchronize()
            steps.append({'before': before, 'grad_sum': model.flat_gradients(zero=False).detach().cpu().clone(),
                          'after': model.flat_parameters().detach().cpu().clone(), 'buf': model._optim['buf'].detach().cpu().clone()})
        torch.save(steps, os.path.join(out_dir, 'rank%d.pt' % rank))
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_sgd(tmp_path):
    """Parameters stay bitwise replicated over two SGD steps, and each step is torch.optim's on the summed gradient scaled by 1/2 (the
    scale the reducer hands to the kernel as gscale)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    port = 37500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_sgd_rank, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    deadline = time.time() + 600                           # each child under its own time limit; the first failure ends the test
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
    model = support.plugin('sgd')
    unused = _without_gradient(model, _rank_batch(0))
    ref = Reference('sgd', {name: shape for name, _, _, shape in model._layout}, 1e-3)
    for i, (s0, s1) in enumerate(zip(r0, r1)):
        assert torch.equal(s0['before'], s1['before']) and torch.equal(s0['grad_sum'], s1['grad_sum']), i
        assert torch.equal(s0['after'], s1['after']) and torch.equal(s0['buf'], s1['buf']), 'step %d: the ranks drifted apart' % i
        before, grads, after, buf = (support.named(model, s0[k]) for k in ('before', 'grad_sum', 'after', 'buf'))
        d64 = ref.step(before, {k: (None if k in unused else g.double() * 0.5) for k, g in grads.items()})
        for name in before:
            support.within_bound(after[name].double() - before[name].double(), d64[name], 'two ranks step %d %s' % (i, name), p_before=before[name])
            support.within_bound(buf[name], ref.state(name), 'two ranks step %d buf %s' % (i, name))
    assert not torch.equal(r0[0]['before'], r0[1]['after'])
