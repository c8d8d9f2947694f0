"""The geometric-normal loss on the host (no GPU): the loss bank entry, normal_geo.settings, the hook's refusals, the C ABI, the shipped
configs, and the proof of the oracle tests/test_gpu_normal_geo.py measures the kernels against (tests/normal_geo_cpu.py; DESIGN.md
section 7)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import normal_geo_cpu as ng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = (0.01, 1, True, (1, 1, 1))


class _Opt(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _settings(block):
    from dualpixelface_amd import normal_geo
    return normal_geo.settings(_Opt(model=_Opt(normal_geo=block)))


# ---- the loss bank
@pytest.mark.parametrize('loss_type,lambdas', [(['normal_geo'], [1.0]), (['smoothL1', 'normal_geo'], [1.0, 0.1])])
def test_loss_selector_accepts_normal_geo(loss_type, lambdas):
    from dualpixelface_amd import load_option, losses
    sel = losses.loss_selector(load_option('train_faceDP_dpnet', loss_type=loss_type, lambdas=lambdas))
    assert sel.loss_name == loss_type and sel.lambda_ == lambdas
    assert isinstance(sel.loss_func[-1], losses.NORMAL_GEOLoss) and losses._BANK['normal_geo'] is losses.NORMAL_GEOLoss
    assert tuple(sel.loss_func[-1].settings) == DEFAULTS
    assert sel.loss_func[-1].head_weights(1) == [1.0] and sel.loss_func[-1].head_weights(5)[1] == 0.75294


def test_folded_and_least_square_stay_refused():
    from dualpixelface_amd import load_option, losses
    with pytest.raises(NotImplementedError, match='wrong loss type : folded'):
        losses.loss_selector(load_option('train_faceDP_dpnet', loss_type=['normal_geo', 'folded'], lambdas=[1.0, 1.0]))
    opt = load_option('train_faceDP_dpnet', loss_type=['normal_geo'])
    opt.dataset.dp_conversion = 'least_square'
    with pytest.raises(NotImplementedError, match='least_square'):
        losses.loss_selector(opt)


def test_the_hook_names_a_missing_key_and_reaches_the_operator():
    from dualpixelface_amd import load_option, losses
    from dualpixelface_amd._lib import DpfError
    sel = losses.loss_selector(load_option('train_faceDP_dpnet', loss_type=['normal_geo']))
    B, H, W = 1, 4, 6
    full = {'K': torch.eye(3).unsqueeze(0), 'depth': torch.ones(B, H, W), 'normal': torch.ones(B, 3, H, W), 'abvalue': torch.ones(B, 2),
            'mask': torch.ones(B, H, W)}
    preds = {'pred_depth': torch.ones(B, 1, H, W)}
    for key in ('K', 'depth', 'normal'):
        batch = {k: v for k, v in full.items() if k != key}
        with pytest.raises(NotImplementedError, match=r"batch\['%s'\]" % key):
            sel.forward(preds, batch)
    with pytest.raises(DpfError, match='GPU tensors'):               # everything there: the operator refuses the CPU tensors
        sel.forward(preds, full)
    with pytest.raises(DpfError, match='GPU tensors'):               # a depth model needs no abvalue
        sel.forward(preds, {k: v for k, v in full.items() if k != 'abvalue'}, target_type='depth')
    # a disp model without abvalue takes the fit, which names what it needs
    with pytest.raises(NotImplementedError, match='idepth'):
        sel.forward(preds, {k: v for k, v in full.items() if k != 'abvalue'})


def test_operator_refuses_cpu_tensors_and_malformed_operands():
    from dualpixelface_amd import ops
    from dualpixelface_amd._lib import DpfError
    pred, depth, normal, K, ab = torch.zeros(1, 2, 8, 8), torch.ones(1, 8, 8), torch.ones(1, 3, 8, 8), torch.eye(3).unsqueeze(0), torch.ones(1, 2)
    with pytest.raises(DpfError, match='GPU tensors'):
        ops.normal_geo_loss(pred, depth, normal, K, ab=ab, head_weights=(1.0, 0.5))
    with pytest.raises(DpfError, match='target_type'):
        ops.normal_geo_loss(pred, depth, normal, K, ab=ab, target_type='inverse')
    import inspect
    assert str(inspect.signature(ops.normal_geo_loss)) == (
        "(pred, depth, normal, Kmat, ab=None, mask=None, head_weights=(1.0,), target_type='disp', max_edge_ratio=0.01, step=1, "
        "towards_camera=True, target_signs=(1, 1, 1), return_normals=False)")


# ---- settings
def test_settings_defaults_for_a_missing_block_and_missing_keys():
    from dualpixelface_amd import normal_geo
    assert tuple(normal_geo.settings(_Opt())) == DEFAULTS and tuple(normal_geo.settings(_Opt(model=_Opt()))) == DEFAULTS
    assert tuple(_settings(None)) == DEFAULTS and tuple(_settings({})) == DEFAULTS and tuple(normal_geo.DEFAULTS) == DEFAULTS
    assert normal_geo.Settings._fields == ('max_edge_ratio', 'step', 'towards_camera', 'target_signs')
    s = _settings({'step': 4, 'target_signs': [1, -1, -1], 'max_edge_ratio': 1})
    assert s.step == 4 and s.target_signs == (1, -1, -1) and s.max_edge_ratio == 1.0 and isinstance(s.max_edge_ratio, float)
    s = _settings(_Opt(towards_camera=False, step=2))                # an attribute block, as config.Option makes one
    assert s.towards_camera is False and s.step == 2 and s.max_edge_ratio == 0.01


@pytest.mark.parametrize('key,value', [
    ('max_edge_ratio', 0), ('max_edge_ratio', -0.01), ('max_edge_ratio', None), ('max_edge_ratio', '0.01'), ('max_edge_ratio', float('inf')),
    ('max_edge_ratio', float('nan')), ('max_edge_ratio', True),
    ('step', 3), ('step', 0), ('step', 8), ('step', 2.0), ('step', True), ('step', '2'), ('step', None),
    ('towards_camera', 1), ('towards_camera', 'true'), ('towards_camera', None),
    ('target_signs', [1, 1]), ('target_signs', [1, 1, 0]), ('target_signs', [1, 1, 2]), ('target_signs', 1), ('target_signs', None),
    ('target_signs', [1, 1, True]), ('target_signs', ['1', 1, 1]), ('target_signs', [1, 1, 1, 1]), ('target_signs', [1, -0.5, 1])])
def test_settings_names_the_malformed_key(key, value):
    with pytest.raises(ValueError, match=key):
        _settings({key: value})


def test_a_non_block_is_refused():
    for bad in (True, 3, 'on', [1]):
        with pytest.raises(ValueError, match='normal_geo'):
            _settings(bad)


# ---- configs
def test_configs_are_their_bases_with_the_loss_and_the_block_spelled_out():
    from dualpixelface_amd import load_option, normal_geo
    base = json.load(open(os.path.join(ROOT, 'src', 'model', 'dpnet', 'config.json')))
    ours = json.load(open(os.path.join(ROOT, 'src', 'model', 'dpnet', 'config_normal_geo.json')))
    block = ours.pop('normal_geo')
    assert set(block) == set(normal_geo.Settings._fields)
    assert block == {'max_edge_ratio': 0.01, 'step': 1, 'towards_camera': True, 'target_signs': [1, 1, 1]}
    assert ours.pop('loss_type') == ['smoothL1', 'normal_geo'] and ours.pop('lambdas') == [1.0, 0.1]
    assert base.pop('loss_type') == ['smoothL1'] and base.pop('lambdas') == [1.0] and ours == base
    top_base = json.load(open(os.path.join(ROOT, 'config_', 'train_faceDP_dpnet.json')))
    top = json.load(open(os.path.join(ROOT, 'config_', 'train_faceDP_dpnet_normal_geo.json')))
    assert top.pop('model_config') == 'config_normal_geo' and top_base.pop('model_config') == 'config' and top == top_base
    opt = load_option('train_faceDP_dpnet_normal_geo')
    assert opt.model_name == 'dpnet' and opt.model.loss_type == ['smoothL1', 'normal_geo'] and opt.model.lambdas == [1.0, 0.1]
    assert tuple(normal_geo.settings(opt)) == DEFAULTS
    for key in ('post_process', 'reconstruct', 'accumulate_grad_batches', 'gradient_clip_val', 'track_grad_norm'):
        assert key not in top, key
    # no other shipped configuration asks for the loss
    for name in sorted(f[:-5] for f in os.listdir(os.path.join(ROOT, 'config_')) if f.endswith('.json')):
        assert ('normal_geo' in load_option(name).model.loss_type) == (name == 'train_faceDP_dpnet_normal_geo'), name


# ---- C ABI
def test_header_declares_the_new_entry_points():
    from dualpixelface_amd import _lib
    protos = _lib.parse_header()
    assert protos['dpf_normal_geo_workspace_bytes'][0] is _lib._CTYPES['long long']
    assert [n for _, n in protos['dpf_normal_geo_workspace_bytes'][1]] == ['B', 'n', 'H', 'W']
    fwd = [n for _, n in protos['dpf_normal_geo_forward'][1]]
    bwd = [n for _, n in protos['dpf_normal_geo_backward'][1]]
    assert len(fwd) == 23 and len(bwd) == 20 and fwd[:16] == bwd[:16]
    assert fwd[16:] == ['ws', 'ws_bytes', 'stats', 'out', 'normal_out', 'counted_out', 'stream'] and bwd[16:] == ['stats', 'gout', 'dpred', 'stream']
    csrc = os.path.join(ROOT, 'dualpixelface_amd', 'csrc')
    make = open(os.path.join(csrc, 'Makefile')).read()
    assert '$(OBJDIR)/normal_geo.o: CXXFLAGS += -ffp-contract=off' in make and ' dpf_geometry.h' in make
    # one statement of the geometry: both kernel files take it from the shared header
    shared = open(os.path.join(csrc, 'dpf_geometry.h')).read()
    for name in ('struct Cam', 'void cam_setup(', 'void ray_of(', 'bool connected('):
        assert name in shared, name
        for f in ('reconstruct.hip', 'normal_geo.hip'):
            src = open(os.path.join(csrc, f)).read()
            assert name not in src and '#include "dpf_geometry.h"' in src, (name, f)


# ---- the oracle
def test_fp64_autograd_gradient_agrees_with_finite_differences():
    """The fp64 torch restatement against central differences of its own loss on the 5 x 7 scene, every element: with the discrete
    decisions held the loss is smooth, the difference quotient at h = 1e-6 (disparities are about 45) is off by h^2 f''' + 1e-16 / h, and
    1e-7 of the largest gradient covers both."""
    r = ng.case('tiny-5x7-disp')
    c = r['case']
    p0 = torch.tensor(c['pred'].astype(np.float64))

    def f(p):
        return float(ng.torch_loss(p, r['r32'], c['normal'], c['K'], c['ab'], c['head_weights'], c['target_type'], c['step'],
                                   c['target_signs'], torch.float64))
    g, h = r['grad64'], 1e-6
    assert g.shape == c['pred'].shape and np.abs(g).max() > 0 and np.count_nonzero(g) == g.size
    worst = 0.0
    for i in range(p0.numel()):
        e = torch.zeros(p0.numel(), dtype=torch.float64)
        e[i] = h
        fd = (f(p0 + e.view_as(p0)) - f(p0 - e.view_as(p0))) / (2 * h)
        worst = max(worst, abs(fd - g.ravel()[i]))
    assert worst <= 1e-7 * np.abs(g).max(), (worst, np.abs(g).max())


def test_both_restatements_of_the_loss_agree_in_fp64():
    """numpy and torch state the same loss: in fp64, with the same decisions, to rounding."""
    for name in ng.CASES:
        r = ng.case(name)
        assert r['agree'], name
        assert abs(r['loss64'] - r['r64']['loss']) <= 1e-12, (name, r['loss64'], r['r64']['loss'])
        assert abs(r['loss32'] - r['r32']['loss']) <= 1.2e-7 * max(r['loss64'], 1e-30), (name, r['loss32'], r['r32']['loss'])


@pytest.mark.parametrize('name', sorted(ng.CASES))
def test_gpu_cases_keep_their_comparisons_off_the_thresholds(name):
    """What tests/test_gpu_normal_geo.py compares exactly must not hang on a rounding: in fp64 no comparison of a case (connectivity,
    depth > 0, |g| > 1e-6, the orientation dot, the clamp) sits within 1e-4 relative of its threshold, and the fp32 and fp64 restatements
    take the same decisions."""
    r = ng.case(name)
    c = r['case']
    assert r['margin'] >= 1e-4 and r['agree']
    counted = r['r32']['counted']
    assert counted.sum() > 0
    if c['singular'] is not None:
        assert not counted[c['singular']].any() and not r['grad64'][c['singular']].any()
    if c['mask'] is not None or name.startswith('step'):
        assert counted.sum() < counted.size
    assert not np.isnan(r['grad64']).any() and not np.isnan(r['grad32']).any()


def test_the_cases_reach_every_branch_of_the_stencil():
    one_sided = no_step = central = 0
    for name in ng.CASES:
        for d in ng.case(name)['r32']['dec']:
            row_c, col_c = d['cl'] & d['cr'], d['cu'] & d['cd']
            central += int((row_c & col_c & d['usable']).sum())
            one_sided += int(((d['cl'] ^ d['cr']) & d['usable']).sum()) + int(((d['cu'] ^ d['cd']) & d['usable']).sum())
            no_step += int((~(d['cl'] | d['cr']) & d['usable']).sum())
    assert central > 1000 and one_sided > 100 and no_step > 0, (central, one_sided, no_step)
    # d_row x d_col points away from the camera on a surface that faces it: every counted normal is negated under towards_camera, none
    # in the case that turns them away
    for name in ng.CASES:
        r = ng.case(name)
        flipped = int((r['r32']['sigma'] * r['r32']['counted'] < 0).sum())
        assert flipped == (int(r['r32']['counted'].sum()) if r['case']['towards_camera'] else 0), name


def test_restatement_on_the_tilted_plane():
    """A prediction equal to the plane with the analytic normal as target: the loss is what the fp32 depth costs (the angles of
    tests/test_reconstruct_host.py, at most 5.4e-4 rad: 1 - cos <= 1.5e-7); turned by theta it is 1 - cos(theta) to about
    sin(theta) x that angle."""
    c, want = ng.plane_case(0.0)
    assert want == 0.0 and 0.0 <= ng.run(c, np.float64)['loss'] <= 1.5e-7 and 0.0 <= ng.run(c)['loss'] <= 1.5e-7
    assert ng.run(c)['count'] == [24.0 * 40.0]
    c, want = ng.plane_case(0.25)
    assert abs(ng.run(c, np.float64)['loss'] - want) <= np.sin(0.25) * 5.4e-4 and abs(ng.run(c)['loss'] - want) <= np.sin(0.25) * 5.4e-4


def test_zero_counted_pixels_give_zero():
    c = ng.make_case(**ng.CASES['tiny-5x7-disp'])
    c['mask'] = np.zeros((1, 5, 7), np.float32)
    r = ng.run(c)
    assert r['loss'] == 0.0 and r['count'] == [0.0] and not r['normal'].any()
    loss, grad = ng.loss_and_grad(c, r, torch.float64)
    assert loss == 0.0 and not grad.any()
