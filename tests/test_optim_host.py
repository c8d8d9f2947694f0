"""The config key ``optim`` (adam | sgd | rmsprop) on the host side: what ``configure_optimizers`` hands out, what a checkpoint records
for each kind, the refusal to resume state of another kind, and an unknown name failing before anything reaches the GPU."""
import pytest
import torch

from dualpixelface_amd.config import load_option
from dualpixelface_amd.trainer import Trainer

STATE = {'sgd': 'buf', 'rmsprop': 'sq'}


class _Toy(torch.nn.Module):
    """flat-arena stand-in with the attributes the trainer touches, keeping the state arena of the new optimiser kinds"""

    def __init__(self, kind):
        super().__init__()
        self.w = torch.nn.Parameter(torch.arange(6, dtype=torch.float32))
        self.register_buffer('running', torch.ones(3))
        self.kind = kind
        self._adam = None
        self._optim = None
        self.steps = []

    def flat_parameters(self):
        return self.w.data

    def train_step(self, batch, reducer=None, lr=None):
        if self.kind == 'adam':
            if self._adam is None:
                self._adam = {'m': torch.zeros(6), 'v': torch.zeros(6), 'step': 0}
            self._adam['step'] += 1
            state = self._adam['m']
        else:
            if self._optim is None:
                self._optim = {'kind': self.kind, STATE[self.kind]: torch.zeros(6)}
            state = self._optim[STATE[self.kind]]
        state += batch['x'].mean()
        self.w.data -= lr * 1000 * state
        self.steps.append(lr)
        return {'final_loss': batch['x'].mean()}


@pytest.mark.parametrize('kind', ['sgd', 'rmsprop'])
def test_checkpoint_kind_round_trip_and_refusal(tmp_path, kind):
    opt = load_option()
    opt.epoch, opt.scheduler, opt.optim = 3, 'explr', kind
    data = [{'x': torch.full((2, 1), float(i + 1))} for i in range(4)]
    m = _Toy(kind)
    tr = Trainer(opt, str(tmp_path), rank=0, world_size=1)
    tr.fit(m, data, None)
    assert m._adam is None and len(m.steps) == 12
    ck = torch.load(tr.checkpoint_path(1), weights_only=False)
    st = ck['optimizer_states'][0]
    assert st['kind'] == 'flat_' + kind and set(st) == {'kind', STATE[kind]} and st[STATE[kind]].shape == (6,)
    # resume from the epoch-1 checkpoint: weights, the state arena and the counters come back, epoch 2 runs and lands on the same numbers
    m2 = _Toy(kind)
    opt.load_model = tr.checkpoint_path(1)
    tr2 = Trainer(opt, str(tmp_path / 'resumed'), rank=0, world_size=1)
    tr2.fit(m2, data, None)
    assert tr2.epoch == 3 and tr2.global_step == 12 and m2.steps == [2.5e-5] * 4
    assert m2._optim['kind'] == kind and m2._adam is None
    assert torch.equal(m2.w.data, m.w.data) and torch.equal(m2._optim[STATE[kind]], m._optim[STATE[kind]])
    # state of another kind cannot continue the run, whichever way round: refused, and NOTHING is restored
    opt.load_model = None
    for other in [k for k in ('adam', 'sgd', 'rmsprop') if k != kind]:
        opt.optim = other
        fresh = _Toy(other)
        w_before = fresh.w.data.clone()
        tr3 = Trainer(opt, str(tmp_path / ('as_' + other)), rank=0, world_size=1)
        with pytest.raises(ValueError, match='Nothing was restored'):
            tr3.load_checkpoint(fresh, tr.checkpoint_path(1))
        assert torch.equal(fresh.w.data, w_before) and fresh._adam is None and fresh._optim is None
        assert tr3.epoch == 0 and tr3.global_step == 0
        tr3.load_checkpoint(fresh, tr.checkpoint_path(1), resume=False)            # the weights alone always load
        assert torch.equal(fresh.w.data, ck['state_dict']['w']) and fresh._adam is None and fresh._optim is None and tr3.epoch == 0


def test_adam_checkpoint_is_refused_under_another_optim(tmp_path):
    opt = load_option()
    opt.epoch, opt.scheduler = 1, 'none'
    assert opt.optim == 'adam'
    m = _Toy('adam')
    tr = Trainer(opt, str(tmp_path), rank=0, world_size=1)
    tr.fit(m, [{'x': torch.ones(2, 1)}], None)
    assert torch.load(tr.checkpoint_path(0), weights_only=False)['optimizer_states'][0]['kind'] == 'flat_adam'
    opt.optim = 'sgd'
    fresh = _Toy('sgd')
    w_before = fresh.w.data.clone()
    tr2 = Trainer(opt, str(tmp_path / 'sgd'), rank=0, world_size=1)
    with pytest.raises(ValueError, match='Nothing was restored'):
        tr2.load_checkpoint(fresh, tr.checkpoint_path(0))
    assert torch.equal(fresh.w.data, w_before) and fresh._adam is None and fresh._optim is None and tr2.epoch == 0
    opt.optim = 'adam'
    back = _Toy('adam')
    tr2.load_checkpoint(back, tr.checkpoint_path(0))
    assert back._adam['step'] == 1 and torch.equal(back._adam['m'], m._adam['m']) and tr2.epoch == 1


def test_checkpoint_before_the_first_step_names_the_kind(tmp_path):
    opt = load_option()
    opt.optim = 'rmsprop'
    tr = Trainer(opt, str(tmp_path), rank=0, world_size=1)
    path = tr.save_checkpoint(_Toy('rmsprop'))
    assert torch.load(path, weights_only=False)['optimizer_states'][0] == {'kind': 'flat_rmsprop', 'sq': None}
    m = _Toy('rmsprop')
    tr.load_checkpoint(m, path)
    assert m._optim is None


def _cpu_plugin(optim):
    from dualpixelface_amd.plugin import STEREODPNET
    opt = load_option()
    opt.optim = optim
    return STEREODPNET(opt)


def test_configure_optimizers_under_each_optim():
    expect = {'adam': (torch.optim.Adam, {'betas': (0.9, 0.999), 'eps': 1e-5, 'weight_decay': 0}),
              'sgd': (torch.optim.SGD, {'momentum': 0.9, 'weight_decay': 2e-4, 'dampening': 0, 'nesterov': False}),
              'rmsprop': (torch.optim.RMSprop, {'eps': 1e-5, 'alpha': 0.99, 'momentum': 0, 'centered': False, 'weight_decay': 0})}
    for optim, (cls, hyper) in expect.items():
        model = _cpu_plugin(optim)
        optimizers, schedulers = model.configure_optimizers()
        assert len(optimizers) == 1 and type(optimizers[0]) is cls, optim
        group = optimizers[0].param_groups[0]
        assert group['lr'] == float(model.option.init_lr)
        assert {k: group[k] for k in hyper} == hyper, (optim, group)
        assert len(group['params']) == len(list(model.parameters()))
        assert len(schedulers) == 1 and isinstance(schedulers[0], torch.optim.lr_scheduler.StepLR)
        assert model._adam is None and model._optim is None


def test_unknown_optim_raises_before_any_gpu_call():
    model = _cpu_plugin('lbfgs')
    with pytest.raises(NotImplementedError, match='optimizer is not defined'):
        model.configure_optimizers()
    # CPU tensors, and nothing of the step has run when the name is refused: no gradient arena, no optimiser state
    from dualpixelface_amd.recipe import synthetic_batch
    with pytest.raises(NotImplementedError, match='optimizer is not defined'):
        model.train_step(synthetic_batch(1, 32, 48, seed=1))
    assert model._flat_grad is None and model._adam is None and model._optim is None
