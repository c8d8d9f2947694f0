"""The model layer's shared base (dualpixelface_amd/core.py), host side (no GPU, no kernel library): every family keeps the reference's
state_dict contract and the flat-arena invariants, leaves the caller's option alone, and carries only the methods of its own network."""
import copy
import json
import os

import pytest
import torch

FAMILIES = {                     # plugin class -> (config, committed state_dict key list)
    'STEREODPNET': ('train_faceDP', 'state_dict_keys.json'),
    'PSMNET': ('train_faceDP_psmnet', 'psmnet_state_dict_keys.json'),
    'NNET': ('train_faceDP_nnet', 'nnet_state_dict_keys.json'),
    'STEREONET': ('train_faceDP_stereonet', 'stereonet_state_dict_keys.json'),
    'DPNET': ('train_faceDP_dpnet', 'dpnet_state_dict_keys.json'),
}
STEREODPNET_ONLY = ('_cost_volume', '_dpblock', '_deform', '_shift_tables')
family = pytest.mark.parametrize('name', sorted(FAMILIES))


def _build(name):
    from dualpixelface_amd import load_option, plugin
    return getattr(plugin, name)(load_option(FAMILIES[name][0]))


@family
def test_state_dict_keys_in_reference_order(name, golden_dir):
    keys = json.load(open(os.path.join(golden_dir, FAMILIES[name][1])))
    want = [k for k in keys if not k.endswith('.grid')]          # (registered by the first forward only)
    sd = _build(name).state_dict()
    assert list(sd) == want
    assert all(list(sd[k].shape) == keys[k] for k in want)


def _assert_arena(model):
    flat = model.flat_parameters()
    pd = dict(model.named_parameters())
    end = 0
    for pname, off, numel, shape in model._layout:               # the slices tile the arena: no gap, no overlap
        assert off == end and numel == int(torch.Size(shape).numel()) and numel > 0, pname
        end = off + numel
        p = pd[pname]
        assert p.requires_grad and tuple(p.shape) == tuple(shape) and p.is_contiguous(), pname
        assert p.data_ptr() == flat.data_ptr() + 4 * off, pname  # the parameter's storage IS its slice
        assert p.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr(), pname
    assert end == flat.numel() and flat.dtype == torch.float32
    assert {n for n, p in pd.items() if p.requires_grad} == {n for n, _, _, _ in model._layout}
    return pd


@family
def test_arena_invariants(name):
    model = _build(name)
    before = _assert_arena(model)
    values = model.flat_parameters().clone()
    assert model.float() is model                                # through _apply / _repack: a new arena ...
    after = _assert_arena(model)
    assert list(after) == list(before) and all(after[k] is before[k] for k in before)      # ... the same Parameter objects
    assert torch.equal(model.flat_parameters(), values)
    fg = model.flat_gradients()
    assert fg.shape == model.flat_parameters().shape and not fg.any()
    for pname, off, numel, shape in model._layout:
        g = after[pname].grad
        assert g.data_ptr() == fg.data_ptr() + 4 * off and tuple(g.shape) == tuple(shape), pname
        assert g.untyped_storage().data_ptr() == fg.untyped_storage().data_ptr(), pname
    assert model.flat_gradients(zero=False) is fg


@family
def test_constructor_leaves_the_option_alone(name):
    from dualpixelface_amd import load_option, plugin
    opt = load_option(FAMILIES[name][0])
    before = copy.deepcopy(vars(opt.model))
    getattr(plugin, name)(opt)
    assert vars(opt.model) == before


def test_each_family_carries_its_own_network_only():
    models = {name: _build(name) for name in FAMILIES}
    for name in ('DPNET', 'STEREONET', 'NNET'):
        for attr in STEREODPNET_ONLY + ('_hourglass', '_aggregate', '_tables'):
            assert not hasattr(models[name], attr), (name, attr)
    assert not hasattr(models['DPNET'], 'costrange') and not hasattr(models['DPNET'], 'disp_values')
    for name in ('PSMNET', 'STEREODPNET'):
        assert callable(models[name]._aggregate) and callable(models[name]._hourglass)
    for attr in STEREODPNET_ONLY:
        assert not hasattr(models['PSMNET'], attr), attr
        assert callable(getattr(models['STEREODPNET'], attr))
    assert models['STEREODPNET']._tables == {}
    # the disparity geometry: 4 hypotheses per cost level, StereoNet 2^k levels with one hypothesis each (stereonet/mainmodel.py:38-40)
    for name in ('STEREODPNET', 'PSMNET', 'NNET'):
        m = models[name]
        assert (m.mindisp, m.maxdisp, m.level) == (-4, 12, 8) and m.costrange == [0.5 * i - 1.0 for i in range(8)]
        assert m.disp_values == [0.5 * i - 4.0 for i in range(32)]
    m = models['STEREONET']
    assert m.level == 8 and m.costrange == [0.5 * i - 1.0 for i in range(8)] and m.disp_values == [2.0 * i - 4.0 for i in range(8)]


@family
def test_shape_constants_start_empty(name):
    model = _build(name)
    assert model._shape_constants() == []
    if name != 'STEREODPNET':                                   # (StereoDPNet's: the two-stream switch, below)
        assert model._capture_key() == ()


def test_shape_constants_are_the_lazily_built_tensors():
    import dualpixelface_amd.stereodpnet as sdn
    model = _build('STEREODPNET')
    tables, phase = model._shift_tables(8, 12, model.costrange[0], 'cpu')
    want = [t for t in tuple(tables) + tuple(phase or ()) if torch.is_tensor(t)]
    got = model._shape_constants()
    assert len(want) >= 6 and len(got) == len(want) and all(a is b for a, b in zip(got, want))
    assert model._capture_key() == (sdn.FEATURES_TWO_STREAMS,)
    model.float()                                               # a device / dtype move drops the tables (rebuilt where the model lives)
    assert model._tables == {} and model._shape_constants() == []
    nnet = _build('NNET')
    nnet._levels = torch.zeros(2, 8, 4, 6)
    got = nnet._shape_constants()
    assert len(got) == 1 and got[0] is nnet._levels


def test_stereodpnet_resumes_a_checkpoint_with_the_lazy_grid():
    src = _build('STEREODPNET')
    sd = dict(src.state_dict())
    grid = torch.arange(3 * 8 * 12, dtype=torch.float32).view(1, 3, 8, 12)
    sd['normal_estimator.grid'] = grid
    model = _build('STEREODPNET')
    assert 'normal_estimator.grid' not in model.state_dict()
    model.load_state_dict(sd, strict=True)
    got = model.state_dict()['normal_estimator.grid']
    assert torch.equal(got, grid) and not model.normal_estimator.grid.requires_grad
    assert model._P['normal_estimator.grid'] is model.normal_estimator.grid
    _assert_arena(model)


@pytest.mark.parametrize('name', sorted(set(FAMILIES) - {'STEREODPNET'}))
def test_other_families_still_refuse_that_key(name):
    model = _build(name)
    sd = dict(model.state_dict())
    sd['normal_estimator.grid'] = torch.zeros(1, 3, 8, 12)
    with pytest.raises((RuntimeError, KeyError)):
        model.load_state_dict(sd, strict=True)
