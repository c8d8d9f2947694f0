"""Confidence maps on the host (no GPU): confidence.settings and its refusals, the shipped config, the batch views of the gates, the
curve rows, the C ABI, and the proof of the restatements tests/test_gpu_confidence.py measures the kernels against
(tests/confidence_cpu.py) by closed forms.

The closed-form groups exercise tests/confidence_cpu.py alone and pass with or without the feature; every other test needs the feature."""
import json
import os

import numpy as np
import pytest
import torch

from tests import confidence_cpu as cc
from tests import unimodal_cpu as uc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U = 2.0 ** -24
GEOMETRIES = ['one-tile', 'multi-tile', 'general', 'half-pixel', 'thin']


class _Opt(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _settings(block):
    from dualpixelface_amd import confidence
    return confidence.settings(_Opt(confidence=block))


# ---- settings
def test_settings_defaults_and_overrides():
    from dualpixelface_amd import confidence
    want = (False, 'entropy', 1, 'expectation', None, (), False, 16)
    assert confidence.Settings._fields == ('enabled', 'measure', 'window', 'estimator', 'threshold', 'gate', 'report', 'bins')
    assert tuple(confidence.DEFAULTS) == want and tuple(confidence.settings(_Opt())) == want
    assert tuple(_settings(None)) == want and tuple(_settings({})) == want
    assert not confidence.active(_Opt()) and not confidence.active(_Opt(confidence={'enabled': False, 'measure': 'peak'}))
    s = _settings({'enabled': True, 'measure': 'mass', 'window': 0, 'estimator': 'modal', 'threshold': 1, 'gate': ['reconstruct', 'metrics'],
                   'report': True, 'bins': 64})
    assert tuple(s) == (True, 'mass', 0, 'modal', 1.0, ('reconstruct', 'metrics'), True, 64) and isinstance(s.threshold, float)
    assert _settings({'threshold': 0}).threshold == 0.0 and _settings({'window': 32, 'bins': 1})[2::5] == (32, 1)
    assert _settings(_Opt(enabled=True, measure='peak')).measure == 'peak'          # an attribute block, as config.Option makes one
    assert confidence.active(_Opt(confidence={'enabled': True}))


@pytest.mark.parametrize('key, value', [
    ('enabled', 1), ('enabled', 'yes'), ('enabled', None), ('report', 0), ('report', 'no'),
    ('measure', 'variance'), ('measure', None), ('measure', 3), ('estimator', 'argmax'), ('estimator', None),
    ('window', -1), ('window', 33), ('window', 1.0), ('window', True), ('window', '1'), ('window', None),
    ('threshold', -0.01), ('threshold', 1.01), ('threshold', float('nan')), ('threshold', float('inf')), ('threshold', '0.5'), ('threshold', True),
    ('gate', 'metrics'), ('gate', ['mesh']), ('gate', ['metrics', 'metrics']), ('gate', [1]), ('gate', None),
    ('bins', 0), ('bins', 65), ('bins', 16.0), ('bins', False), ('bins', None)])
def test_a_malformed_value_is_refused_by_key(key, value):
    block = {'threshold': 0.5} if key == 'gate' else {}
    with pytest.raises(ValueError, match=r'confidence\.%s must be ' % key):
        _settings(dict(block, **{key: value}))
    with pytest.raises(ValueError, match=r'confidence\.%s must be ' % key):
        _settings(dict(dict(block, enabled=True), **{key: value}))


def test_a_gate_needs_a_threshold_and_a_non_block_is_refused():
    for gate in (['metrics'], ['reconstruct'], ['metrics', 'reconstruct']):
        with pytest.raises(ValueError, match=r'confidence\.gate must be .*threshold'):
            _settings({'enabled': True, 'gate': gate})
        assert _settings({'gate': gate, 'threshold': 0.25}).gate == tuple(gate)
    assert _settings({'gate': []}).gate == ()
    for bad in (True, 3, 'on', [1]):
        with pytest.raises(ValueError, match='confidence'):
            _settings(bad)


def test_the_shipped_config_loads_and_differs_from_the_plain_one_by_the_block_only():
    from dualpixelface_amd import confidence, load_option
    ours = json.load(open(os.path.join(ROOT, 'config_', 'eval_faceDP_confidence.json')))
    block = ours.pop('confidence')
    assert ours == json.load(open(os.path.join(ROOT, 'config_', 'eval_faceDP.json')))
    assert block == {'enabled': True, 'measure': 'entropy', 'window': 1, 'estimator': 'modal', 'threshold': 0.5,
                     'gate': ['metrics', 'reconstruct'], 'report': True, 'bins': 16}
    assert set(block) == set(confidence.Settings._fields)
    opt = load_option('eval_faceDP_confidence')
    assert opt.model_name == 'stereodpnet'
    assert tuple(confidence.settings(opt)) == (True, 'entropy', 1, 'modal', 0.5, ('metrics', 'reconstruct'), True, 16)
    for name in sorted(os.listdir(os.path.join(ROOT, 'config_'))):
        if name.endswith('.json'):
            assert confidence.active(load_option(name[:-5])) == (name == 'eval_faceDP_confidence.json'), name


@pytest.mark.parametrize('config, model', [('train_faceDP_dpnet', 'dpnet'), ('train_faceDP_stereonet', 'stereonet')])
def test_models_without_hypotheses_are_refused_by_name(config, model):
    from dualpixelface_amd import confidence, load_option
    opt = load_option(config)
    confidence.check_model(opt)                                               # block absent: nothing to refuse
    opt.confidence = {'enabled': False}
    confidence.check_model(opt)
    opt.confidence = {'enabled': True}
    with pytest.raises(NotImplementedError, match='confidence.*%s' % model):
        confidence.check_model(opt)
    for name in ('train_faceDP', 'train_faceDP_psmnet', 'train_faceDP_nnet'):
        ok = load_option(name)
        ok.confidence = {'enabled': True}
        confidence.check_model(ok)


# ---- the parts that need no device
def test_apply_leaves_results_alone_when_off_or_training_and_needs_the_heads_when_on():
    from dualpixelface_amd import confidence
    res = {'pred_depth': torch.zeros(1, 1, 4, 4)}
    assert confidence.apply(_Opt(), res, {}) is res and list(res) == ['pred_depth']
    on = _Opt(confidence={'enabled': True}, model_name='stereodpnet')
    assert confidence.apply(on, res, {}, training=True) is res and list(res) == ['pred_depth']
    with pytest.raises(NotImplementedError, match="_heads"):
        confidence.apply(on, res, {})
    assert list(res) == ['pred_depth']


def test_the_gates_hand_out_a_view_and_leave_the_batch_and_its_own_conf_alone():
    from dualpixelface_amd import confidence
    valid = torch.tensor([[[1, 0], [1, 1]]], dtype=torch.uint8)
    res = {'pred_conf': torch.rand(1, 2, 2, 2), 'pred_conf_valid': valid}
    mask, own = torch.tensor([[[1.0, 1.0], [0.0, 1.0]]]), torch.rand(1, 2, 2)
    batch = {'mask': mask, 'conf': own, 'depth': torch.ones(1, 2, 2)}
    opt = _Opt(confidence={'enabled': True, 'threshold': 0.5, 'gate': ['metrics']})
    view = confidence.gated(opt, res, batch, 'metrics')
    assert view is not batch and batch['mask'] is mask and view['conf'] is own and view['depth'] is batch['depth']
    assert torch.equal(view['mask'], torch.tensor([[[1.0, 0.0], [0.0, 1.0]]])) and view['mask'].dtype == mask.dtype
    assert confidence.gated(opt, res, batch, 'reconstruct') is batch            # a gate that is not named
    assert confidence.gated(_Opt(), res, batch, 'metrics') is batch             # block absent
    assert confidence.gated(opt, {'pred_depth': None}, batch, 'metrics') is batch and confidence.gated(opt, None, batch, 'metrics') is batch
    free = confidence.gated(opt, res, {'depth': batch['depth']}, 'metrics')     # no mask: the valid map is the mask
    assert torch.equal(free['mask'], valid.float()) and free['mask'].dtype == res['pred_conf'].dtype
    four = confidence.gated(opt, res, {'mask': mask[:, None]}, 'metrics')       # the mask keeps its shape
    assert four['mask'].shape == (1, 1, 2, 2) and torch.equal(four['mask'][:, 0], view['mask'])


def test_curve_rows_are_cumulative_from_the_confident_end():
    from dualpixelface_amd import confidence
    rows = confidence.curve_rows([[2, 4.0], [0, 0.0], [1, 0.5], [1, 0.25]])
    assert [r['edge'] for r in rows] == [0.0, 0.25, 0.5, 0.75]
    assert [r['coverage'] for r in rows] == [1.0, 0.5, 0.5, 0.25] and [r['count'] for r in rows] == [4, 2, 2, 1]
    assert [r['mean_error'] for r in rows] == [4.75 / 4, 0.375, 0.375, 0.25]
    empty = confidence.curve_rows([[0, 0.0], [0, 0.0]])
    assert [r['coverage'] for r in empty] == [0.0, 0.0] and [r['mean_error'] for r in empty] == [None, None]


def test_ops_refuse_what_does_not_fit_before_any_launch():
    """(CPU tensors: THE operand check answers first, which is what this pins down; the shape refusals are in the GPU file.)"""
    from dualpixelface_amd import ops
    from dualpixelface_amd._lib import DpfError
    k = torch.zeros(1, 1, 8, 2, 3)
    with pytest.raises(DpfError, match='GPU tensors'):
        ops.head_confidence([k], uc.shipped_disp())
    with pytest.raises(DpfError, match='list of 1..8'):
        ops.head_confidence([], uc.shipped_disp())
    with pytest.raises(DpfError, match='list of 1..8'):
        ops.head_confidence(k, uc.shipped_disp())
    with pytest.raises(DpfError, match='GPU tensors'):
        ops.confidence_curve(torch.zeros(1, 2, 2), torch.zeros(1, 2, 2), torch.zeros(1, 2, 2))
    assert ops.CONFIDENCE_PLANES == ('peak', 'entropy', 'mass', 'spread', 'modal', 'lstar')


# ---- C ABI
def test_header_prototypes_match_the_binding():
    from dualpixelface_amd import _lib
    import ctypes
    protos = _lib.parse_header()
    ret, args = protos['dpf_head_confidence']
    assert ret is ctypes.c_int and [n for _, n in args] == [
        'logits_host', 'B', 'n', 'D', 'h', 'w', 'L', 'H', 'W', 'align_corners', 'disp_host', 'window', 'peak', 'entropy', 'mass', 'spread',
        'modal', 'lstar', 'stream']
    assert [t for t, _ in args] == [ctypes.c_void_p] + [ctypes.c_int] * 9 + [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 7
    uni = [n for _, n in protos['dpf_unimodal_forward'][1]]
    assert [n for _, n in args][1:11] == uni[4:14]                            # the geometry is named and ordered as the unimodal entry has it
    q = protos['dpf_confidence_curve_workspace_bytes']
    assert q[0] is ctypes.c_longlong and [n for _, n in q[1]] == ['B', 'H', 'W', 'bins']
    ret, args = protos['dpf_confidence_curve']
    assert ret is ctypes.c_int and [n for _, n in args] == [
        'conf', 'conf_batch_stride', 'pred', 'pred_batch_stride', 'target', 'mask', 'target_ab', 'B', 'H', 'W', 'bins', 'accumulate', 'ws',
        'ws_bytes', 'curve', 'stream']
    assert [t for t, _ in args] == [ctypes.c_void_p, ctypes.c_longlong] * 2 + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 5 + [
        ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p]
    make = open(os.path.join(ROOT, 'dualpixelface_amd', 'csrc', 'Makefile')).read()
    assert '$(OBJDIR)/head_confidence.o: CXXFLAGS += -ffp-contract=off' in make
    # one definition of the per-pixel work: both files take Pixel<FAST> from the header
    shared = open(os.path.join(ROOT, 'dualpixelface_amd', 'csrc', 'dpf_softargmin.h')).read()
    assert 'struct Pixel {' in shared and '#define UNI_FOR_L(' in shared
    for name in ('unimodal.hip', 'head_confidence.hip'):
        src = open(os.path.join(ROOT, 'dualpixelface_amd', 'csrc', name)).read()
        assert '#include "dpf_softargmin.h"' in src and 'struct Pixel' not in src and '#define UNI_FOR_L' not in src, name


# ---- the restatements against closed forms
def _zero_case(name):
    c = uc.case(name)['case']
    return c, [np.zeros_like(k) for k in c['logits']]


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('r', [0, 1, 2, 32])
@pytest.mark.parametrize('name', ['multi-tile', 'general', 'half-pixel'])
def test_zero_logits_give_the_uniform_distribution(name, r, dtype):
    c, zeros = _zero_case(name)
    d = np.asarray(c['disp'], dtype=F32).astype(np.float64)
    L, k = len(d), min(r, len(d) - 1) + 1
    p = cc.planes(zeros, c['disp'], c['scale'], c['align'], r, dtype)
    tol = 4 * L * U * np.abs(d).max()
    assert not p['bad'].any() and not p['lstar'].any()
    assert (p['peak'] == dtype(1) / dtype(L)).all() and (p['entropy'] == 0).all()
    assert np.abs(p['mass'] - k / L).max() <= L * U
    assert np.abs(p['modal'] - d[:k].mean()).max() <= tol
    assert np.abs(p['mu'] - d.mean()).max() <= tol and np.abs(p['spread'] - d.std()).max() <= tol


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('name', GEOMETRIES)
def test_the_window_settings_at_both_ends(name, dtype):
    c = uc.case(name)['case']
    d = np.asarray(c['disp'], dtype=F32).astype(dtype)
    L = len(d)
    wide = cc.planes(c['logits'], c['disp'], c['scale'], c['align'], L - 1, dtype)
    assert np.array_equal(wide['lstar'], cc.planes(c['logits'], c['disp'], c['scale'], c['align'], 32, dtype)['lstar'])
    assert not wide['bad'].any()
    assert np.abs(wide['mass'] - 1).max() <= L * U                                      # the whole distribution: 1 within rounding
    assert np.abs(wide['modal'] - wide['mu']).max() <= (L + 2) * U * np.abs(d).max()   # ... and its mean
    point = cc.planes(c['logits'], c['disp'], c['scale'], c['align'], 0, dtype)
    assert np.array_equal(point['mass'], point['peak'])                                  # e_{l*} is exactly 1
    assert np.abs(point['modal'] - d[point['lstar']]).max() <= 2 * U * np.abs(d).max()
    ends = int(((point['lstar'] == 0) | (point['lstar'] == L - 1)).sum())
    print('%s: l* at hypothesis 0 or L - 1 in %d of %d pixels' % (name, ends, point['lstar'].size))
    assert ends > 0                                                                      # the clipped window is exercised


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('name', ['multi-tile', 'general', 'half-pixel'])
def test_spatially_constant_logits_give_every_pixel_the_same_values(name, dtype):
    """The level values differ from the constant by the rounding of hx + lx and hy + ly only: a few units of 2^-24 of the logits, which
    the planes pass on at most (12 + L / e) fold (the allowance of tests/test_gpu_confidence.py)."""
    c = uc.case(name)['case']
    rng = np.random.RandomState(3)
    logits = []
    for k in c['logits']:
        levels = rng.permutation(k.shape[2]).astype(F32) * F32(0.75)                     # distinct, 0.75 apart: no tie anywhere
        logits.append(np.broadcast_to(levels[None, None, :, None, None], k.shape).copy())
    p = cc.planes(logits, c['disp'], c['scale'], c['align'], 1, dtype)
    L, dmax = len(c['disp']), float(np.abs(c['disp']).max())
    spread_of = lambda a: float((a.max(axis=(0, 2, 3)) - a.min(axis=(0, 2, 3))).max())     # noqa: E731  (per head)
    assert not p['bad'].any() and spread_of(p['lstar']) == 0
    eps = 64 * (12 + L / np.e) * U
    for key, scale in (('peak', 1.0), ('entropy', 1.0), ('mass', 1.0), ('spread', dmax), ('modal', dmax)):
        assert spread_of(p[key].astype(np.float64)) <= eps * scale, key


def test_the_near_ties_of_the_cases_stay_inside_the_cap():
    """What test 1 of the GPU file may leave out, counted under the fp32 restatement alone: at most 1 % of a case's pixels."""
    for name in GEOMETRIES:
        c = uc.case(name)['case']
        p = cc.planes(c['logits'], c['disp'], c['scale'], c['align'], 1)
        near = cc.near_tie(p)
        tied = p['gap'] == 0
        print('%s: %d near ties, exact ties per head %s of %d pixels' % (name, near.sum(), tied.sum(axis=(0, 2, 3)).tolist(), near[:, 0].size))
        assert near.sum() <= 0.01 * near.size
        assert (name == 'half-pixel') == bool(tied.any())                                  # the structural ties u_0 == u_1 of NNet's geometry


# ---- the curve restatement
@pytest.mark.parametrize('bins', [1, 16, 64])
def test_the_curve_holds_every_counted_pixel_once(bins):
    ref = uc.case('fitted')
    c = ref['case']
    rng = np.random.RandomState(5)
    conf = rng.uniform(0, 1, c['target'].shape).astype(F32)
    conf[0, 0, :4] = [1.0, 0.0, np.nan, np.inf]
    pred = ref['r32']['expect'][:, 0].copy()
    pred[1, 2, 3] = np.nan
    table, ok, err, which = cc.curve(conf, pred, c['target'], c['mask'], c['ab'], bins)
    assert table.shape == (bins, 2) and table[:, 0].sum() == ok.sum() and 0 < ok.sum() < ok.size
    assert abs(table[:, 1].sum() - err[ok].astype(np.float64).sum()) <= 1e-12 * table[:, 1].sum()
    assert which[0, 0, 0] == bins - 1 and which[0, 0, 1] == 0 and not ok[0, 0, 2] and not ok[0, 0, 3] and not ok[1, 2, 3]
    assert not ok[c['mask'] <= 0].any() and (which[ok] >= 0).all() and (which[ok] < bins).all()
