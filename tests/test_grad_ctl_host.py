"""Gradient accumulation, global-norm clipping and norm tracking on the host side: how the option keys and the shim's keyword arguments
are read and refused, the trainer's group arithmetic on a stub model, and the refusal of the knobs outside the gather scheme."""
import os
import sys

import pytest
import torch

from dualpixelface_amd import optim
from dualpixelface_amd.config import load_option
from dualpixelface_amd.trainer import Trainer

from tests import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_defaults_and_parsing():
    kn = optim.knobs(load_option())
    assert kn == (1, 0.0, False) and not kn.on and not kn.reports
    kn = optim.knobs(support.option_set(accumulate_grad_batches=4, gradient_clip_val=1, gradient_clip_algorithm='norm', track_grad_norm=-1))
    assert kn == (4, 1.0, False) and kn.on and kn.reports and isinstance(kn.clip, float)
    kn = optim.knobs(support.option_set(track_grad_norm=2))
    assert kn == (1, 0.0, True) and kn.on and kn.reports
    kn = optim.knobs(support.option_set(accumulate_grad_batches=3))
    assert kn.on and not kn.reports


def test_every_shipped_config_keeps_the_knobs_off_except_the_accumulation_one():
    names = sorted(f[:-5] for f in os.listdir(os.path.join(ROOT, 'config_')) if f.endswith('.json'))
    assert 'train_faceDP_accum' in names
    for name in names:
        opt = load_option(name)
        if name == 'train_faceDP_accum':
            assert optim.knobs(opt) == (4, 1.0, False) and opt.model_name == 'stereodpnet'
        else:
            assert not optim.knobs(opt).on, name


@pytest.mark.parametrize('bad', [{'4': 2}, 2.5, 0, -1, '2', True, None])
def test_accumulate_grad_batches_refusals(bad):
    from dualpixelface_amd.config import Option
    with pytest.raises(ValueError, match='accumulate_grad_batches'):
        optim.knobs(support.option_set(accumulate_grad_batches=bad))
    if isinstance(bad, dict):                              # the form a JSON config gives a dict
        with pytest.raises(ValueError, match='accumulate_grad_batches'):
            optim.knobs(support.option_set(accumulate_grad_batches=Option(bad)))


def test_clip_and_track_refusals():
    with pytest.raises(NotImplementedError, match="'value'"):
        optim.knobs(support.option_set(gradient_clip_val=0.5, gradient_clip_algorithm='value'))
    with pytest.raises(ValueError, match='gradient_clip_algorithm'):
        optim.knobs(support.option_set(gradient_clip_algorithm='max'))
    for bad in (-0.5, float('nan'), '1.0', None):
        with pytest.raises(ValueError, match='gradient_clip_val'):
            optim.knobs(support.option_set(gradient_clip_val=bad))
    for bad in (1, 'inf', float('inf'), 0, True):
        with pytest.raises(ValueError, match='track_grad_norm'):
            optim.knobs(support.option_set(track_grad_norm=bad))


def _cpu_batch():
    from dualpixelface_amd.recipe import synthetic_batch
    return synthetic_batch(1, 32, 48, seed=1)


def test_train_step_refuses_the_knobs_without_the_gather_scheme():
    """Refused before anything of the step runs (CPU tensors, no gradient arena, no optimiser state); the refusals of the option itself
    surface from train_step too."""
    from dualpixelface_amd.plugin import STEREODPNET
    for kw in ({'accumulate_grad_batches': 2}, {'gradient_clip_val': 1.0}, {'track_grad_norm': 2}):
        model = STEREODPNET(support.option_set(**kw))
        model.gather_grads = False
        with pytest.raises(NotImplementedError, match='gather'):
            model.train_step(_cpu_batch())
        assert model._flat_grad is None and model._adam is None and model._optim is None
    model = STEREODPNET(support.option_set(gradient_clip_val=1.0, gradient_clip_algorithm='value'))
    with pytest.raises(NotImplementedError, match="'value'"):
        model.train_step(_cpu_batch())
    model = STEREODPNET(support.option_set(accumulate_grad_batches={'0': 2}))
    with pytest.raises(ValueError, match='accumulate_grad_batches'):
        model.train_step(_cpu_batch())
    assert model._flat_grad is None and model._adam is None


class _Stub(torch.nn.Module):
    """The attributes the trainer touches; groups its micro-steps the way the plugins do and records what it was asked."""

    def __init__(self, option):
        super().__init__()
        self.option = option
        self.w = torch.nn.Parameter(torch.zeros(4))
        self._adam = None
        self._optim = None
        self.calls = []                                    # (batch number, last_in_epoch, whether the optimiser ran)
        self.pos = 0

    def flat_parameters(self):
        return self.w.data

    def train_step(self, batch, reducer=None, lr=None, last_in_epoch=False):
        kn = optim.knobs(self.option)
        apply = self.pos + 1 >= kn.accum or last_in_epoch
        self.pos = 0 if apply else self.pos + 1
        self.calls.append((int(batch['x'][0]), bool(last_in_epoch), apply))
        res = {'final_loss': batch['x'].float().mean()}
        if apply and kn.reports:
            res['grad_norm'] = torch.tensor(2.5)
        return res


def _batches(n):
    return [{'x': torch.full((2,), i + 1)} for i in range(n)]


def test_trainer_group_arithmetic(tmp_path):
    """7 batches at N = 3: optimiser steps after batches 3, 6 and 7 (the short group is ended by last_in_epoch), global_step == 3, the log
    holds one record per optimiser step with grad_norm, and a second epoch starts a fresh group."""
    opt = support.option_set(accumulate_grad_batches=3, gradient_clip_val=1.0, epoch=1, scheduler='none')
    m = _Stub(opt)
    tr = Trainer(opt, str(tmp_path), log_every=1, rank=0, world_size=1)
    tr.fit(m, _batches(7), None)
    assert [c[0] for c in m.calls if c[2]] == [3, 6, 7]
    assert [c[1] for c in m.calls] == [False] * 6 + [True]
    assert tr.global_step == 3 and tr.epoch == 1 and m.pos == 0
    steps = [r for r in tr.history if 'step' in r]
    assert [r['step'] for r in steps] == [1, 2, 3] and all(r['grad_norm'] == 2.5 for r in steps)
    assert [r['final_loss'] for r in steps] == [3.0, 6.0, 7.0]
    assert os.path.exists(tr.checkpoint_path(0))
    opt.epoch = 2
    tr.fit(m, _batches(7), None)
    assert tr.global_step == 6 and [c[0] for c in m.calls[7:] if c[2]] == [3, 6, 7]


def test_trainer_max_steps_and_log_every_count_optimiser_steps(tmp_path):
    opt = support.option_set(accumulate_grad_batches=2, epoch=5, scheduler='none')
    m = _Stub(opt)
    tr = Trainer(opt, str(tmp_path), log_every=2, max_steps=None, rank=0, world_size=1)
    tr.fit(m, _batches(8), None)
    assert tr.global_step == 20 and [r['step'] for r in tr.history if 'step' in r] == list(range(2, 21, 2))
    assert all('grad_norm' not in r for r in tr.history)
    m2 = _Stub(opt)
    tr2 = Trainer(opt, str(tmp_path / 'capped'), max_steps=3, rank=0, world_size=1)
    tr2.fit(m2, _batches(8), None)
    assert tr2.global_step == 3 and len(m2.calls) == 6 and m2.pos == 0


def test_trainer_with_the_knobs_off_calls_train_step_as_before(tmp_path):
    """No look-ahead, no keyword: a model whose train_step knows nothing of last_in_epoch trains as it did."""
    class Old(_Stub):
        def train_step(self, batch, reducer=None, lr=None):
            self.calls.append(int(batch['x'][0]))
            return {'final_loss': batch['x'].float().mean()}
    opt = support.option_set(epoch=1, scheduler='none')
    m = Old(opt)
    tr = Trainer(opt, str(tmp_path), log_every=1, rank=0, world_size=1)
    tr.fit(m, _batches(7), None)
    assert m.calls == list(range(1, 8)) and tr.global_step == 7
    assert [r['step'] for r in tr.history if 'step' in r] == list(range(1, 8))
    with pytest.raises(ValueError, match='accumulate_grad_batches'):
        Trainer(support.option_set(accumulate_grad_batches={'1': 2}), str(tmp_path), rank=0, world_size=1).fit(Old(opt), _batches(1), None)


def test_shim_hands_the_keywords_through(tmp_path, monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, 'compat'))
    for name in [n for n in sys.modules if n == 'pytorch_lightning' or n.startswith('pytorch_lightning.')]:
        monkeypatch.delitem(sys.modules, name)
    import pytorch_lightning as pl
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    opt = support.option_set(gradient_clip_val=5.0, epoch=1, scheduler='none', workspace_path=str(tmp_path))
    m = _Stub(opt)
    shim = pl.Trainer(max_epochs=1, accumulate_grad_batches=3, gradient_clip_val=0.25, track_grad_norm=2, log_every_n_steps=1)
    shim.fit(m, _batches(7), None)
    assert (opt.accumulate_grad_batches, opt.gradient_clip_val, opt.track_grad_norm) == (3, 0.25, 2)
    assert optim.knobs(opt) == (3, 0.25, True)
    assert shim.native.global_step == 3 and [c[0] for c in m.calls if c[2]] == [3, 6, 7]
    # what is not given leaves the option alone; what is given wrongly is refused by the same rules
    opt2 = support.option_set(gradient_clip_val=5.0, accumulate_grad_batches=2, epoch=1, scheduler='none', workspace_path=str(tmp_path / 'b'))
    pl.Trainer(max_epochs=1).fit(_Stub(opt2), _batches(2), None)
    assert optim.knobs(opt2) == (2, 5.0, False)
    with pytest.raises(NotImplementedError, match="'value'"):
        pl.Trainer(max_epochs=1, gradient_clip_val=0.5, gradient_clip_algorithm='value').fit(_Stub(opt2), _batches(2), None)
    with pytest.raises(ValueError, match='accumulate_grad_batches'):
        pl.Trainer(max_epochs=1, accumulate_grad_batches={4: 2}).fit(_Stub(opt2), _batches(2), None)
