"""The host code of a train step without a GPU: the optimiser record (dualpixelface_amd/optim.py) as the step and the checkpoints use it, the
graph states' LRU lookup, and the refusals of ``train_step`` that must fire before anything reaches the GPU."""
import types

import pytest
import torch

from dualpixelface_amd import optim

KINDS = sorted(optim.TABLE)


class _Flat(object):
    """The attributes the record touches: the option, the parameter arena and the two state attributes."""

    def __init__(self, kind):
        self.option = types.SimpleNamespace(optim=kind)
        self._params = torch.arange(6, dtype=torch.float32)
        self._adam = None
        self._optim = None

    def flat_parameters(self):
        return self._params


def _stepped(kind):
    model, rec = _Flat(kind), optim.TABLE[kind]
    setattr(model, rec.attr, rec.new_state([torch.full((6,), float(i + 1)) for i in range(len(rec.names))], 7))
    return model, rec


@pytest.mark.parametrize('kind', KINDS)
def test_checkpoint_round_trip_through_the_record(kind):
    model, rec = _stepped(kind)
    other = '_optim' if rec.attr == '_adam' else '_adam'
    saved = optim.to_checkpoint(model, model.option)
    assert saved['kind'] == 'flat_' + kind and set(saved) == {'kind'} | set(rec.names) | ({'step'} if kind == 'adam' else set())
    fresh = _Flat(kind)
    optim.from_checkpoint(fresh, saved)
    back = rec.state(fresh)
    assert getattr(fresh, other) is None and set(back) == set(rec.state(model))
    for name in rec.names:
        assert torch.equal(back[name], rec.state(model)[name]) and back[name] is not rec.state(model)[name]
    assert (back['step'] == 7 and 'kind' not in back) if kind == 'adam' else (back['kind'] == kind and 'step' not in back)
    assert rec.counter_of(fresh) == (7 if kind == 'adam' else None)
    # before the first step the record names the kind and carries None arenas; reading it back leaves the model without state
    first = optim.to_checkpoint(_Flat(kind), model.option)
    assert first == dict({'kind': 'flat_' + kind}, **dict({n: None for n in rec.names}, **({'step': 0} if kind == 'adam' else {})))
    untouched = _Flat(kind)
    optim.from_checkpoint(untouched, first)
    assert untouched._adam is None and untouched._optim is None


def test_a_model_that_only_exposes_adam_checkpoints_as_flat_adam():
    model = types.SimpleNamespace(_adam={'m': torch.ones(2), 'v': torch.zeros(2), 'step': 3})
    for kind in KINDS + ['lbfgs']:
        saved = optim.to_checkpoint(model, types.SimpleNamespace(optim=kind))
        assert saved['kind'] == 'flat_adam' and saved['step'] == 3 and torch.equal(saved['m'], torch.ones(2))
    holder = _Flat('rmsprop')
    holder._optim = {'kind': 'sgd', 'buf': torch.zeros(6)}
    with pytest.raises(ValueError, match="holds 'sgd' optimiser state while option.optim is 'rmsprop'"):
        optim.to_checkpoint(holder, holder.option)


@pytest.mark.parametrize('kind', KINDS)
def test_arena_list_and_key_component(kind):
    model, rec = _Flat(kind), optim.TABLE[kind]
    assert rec.arenas(model) == [] and rec.key(model) == (kind,)
    model, rec = _stepped(kind)
    st = rec.state(model)
    want = {'adam': ['m', 'v'], 'sgd': ['buf'], 'rmsprop': ['sq']}[kind]
    assert [id(t) for t in rec.arenas(model)] == [id(st[n]) for n in want]
    key = rec.key(model)
    assert key == rec.key(model) and key[0] == kind and len(key) == 1 + len(want)
    if kind == 'sgd':                                           # the liveness mask: None = all live = not an arena
        st['dead'], st['live'] = (), None
        assert rec.key(model) == key
        st['dead'], st['live'] = ((0, 2),), torch.ones(6, dtype=torch.uint8)
        assert [id(t) for t in rec.arenas(model)] == [id(st['buf']), id(st['live'])]
        key = rec.key(model)
        assert len(key) == 3
        want = want + ['live']
    st['step' if kind == 'adam' else 'dead'] = 9                # what is no arena does not move the key
    assert rec.key(model) == key
    for name in want:                                           # a new tensor in an arena's place does (the old one is still alive)
        old, st[name] = st[name], st[name].clone()
        assert rec.key(model) != key
        st[name] = old
        assert rec.key(model) == key


@pytest.fixture(scope='module')
def plugin_model():
    from dualpixelface_amd import load_option, plugin
    return plugin.STEREODPNET(load_option('train_faceDP'))


def test_graph_state_lookup_keeps_the_last_three_in_order_of_use(plugin_model):
    model = plugin_model
    assert getattr(model, '_graph_states', None) is None
    a = model._graph_lookup(('a',))
    assert a == {'key': ('a',), 'calls': 0, 'graph': None} and model._graph_states == [a] and model._graph_state is a
    a['calls'] = 5
    b, c = model._graph_lookup(('b',)), model._graph_lookup(('c',))
    assert [g['key'] for g in model._graph_states] == [('a',), ('b',), ('c',)] and model._graph_state is c
    hit = model._graph_lookup(('a',))                           # a hit moves to the end and keeps its counter
    assert hit is a and a['calls'] == 5 and model._graph_state is a
    assert [g['key'] for g in model._graph_states] == [('b',), ('c',), ('a',)]
    d = model._graph_lookup(('d',))                             # a fourth key drops the least recently used
    assert [g['key'] for g in model._graph_states] == [('c',), ('a',), ('d',)] and model._graph_state is d
    assert all(g is s for g, s in zip(model._graph_states, (c, a, d))) and b not in model._graph_states
    again = model._graph_lookup(('b',))                         # ... which starts over when it comes back
    assert again is not b and again['calls'] == 0 and [g['key'] for g in model._graph_states] == [('a',), ('d',), ('b',)]
    del model._graph_states, model._graph_state


@pytest.mark.parametrize('optim_name, gather, message', [
    ('lbfgs', True, 'optimizer is not defined, please check your optimizer configuration !'),
    ('sgd', False, "optim 'sgd' needs the gather scheme (model.gather_grads): gradients accumulated into arena views do not tell an unused "
                   "parameter, which SGD must skip, from a zero gradient")])
def test_train_step_refusals_fire_before_any_gpu_call(plugin_model, monkeypatch, optim_name, gather, message):
    from dualpixelface_amd.recipe import synthetic_batch
    model = plugin_model
    monkeypatch.setattr(model.option, 'optim', optim_name)
    monkeypatch.setattr(model, 'gather_grads', gather, raising=False)

    def no_cuda(*args, **kwargs):
        raise AssertionError('train_step touched CUDA before refusing')
    for name in ('current_stream', 'is_available', 'synchronize', 'is_current_stream_capturing'):
        monkeypatch.setattr(torch.cuda, name, no_cuda)
    with pytest.raises(NotImplementedError) as err:
        model.train_step(synthetic_batch(1, 32, 48, seed=1))
    assert str(err.value) == message
    assert model._flat_grad is None and model._adam is None and model._optim is None and getattr(model, '_graph_states', None) is None
