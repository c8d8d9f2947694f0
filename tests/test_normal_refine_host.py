"""The normal_refine block on the host (no GPU): the closed forms that tie the restatement of tests/normal_refine_cpu.py to the definition
it restates (include/dpf_hip.h), normal_refine.settings / apply, and the operator's refusals."""
import json
import os

import numpy as np
import pytest
import torch

from tests import normal_refine_cpu as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = (False, 0.1, 32, 0.01, 0.1, 'predicted', (1, 1, 1), True, 0.0, None)


class _Opt(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _mod():
    from dualpixelface_amd import normal_refine
    return normal_refine


def _rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b) ** 2)))


# ---- the restatement
def test_converged_restatement_equals_a_dense_solve():
    """19 x 70, two samples, a mask with holes, depth steps, defective normals: 256 iterations of the fp64 restatement against
    numpy.linalg.solve on the dense A, to 1e-10 in delta."""
    c = nr.CASES[1]
    assert c[:3] == (2, 19, 70)
    sc = nr.case(c)['sc']
    plane0 = np.ascontiguousarray(sc['pred'][:, 0])
    r = nr.normal_refine(plane0, c[3], sc['ab'], sc['K'], sc['mask'], sc['normal'], lam=nr.LAM, iterations=256, dt=np.float64)
    for b in range(2):
        A, rhs, valid = nr.dense(r['sy'], b)
        assert np.array_equal(A, A.T) and np.linalg.eigvalsh(A).min() >= 0.0999
        want = np.linalg.solve(A, rhs)
        err = float(np.abs(r['delta'][b][valid] - want).max())
        print('sample %d: %d unknowns, max |delta - dense solve| %.3e, max |delta| %.3e' % (b, len(rhs), err, np.abs(want).max()))
        assert err <= 1e-10 and np.abs(want).max() > 1e-4
        assert not r['delta'][b][~valid].any()


@pytest.mark.parametrize('dt', [np.float32, np.float64], ids=['fp32', 'fp64'])
def test_a_plane_with_its_own_normals_is_a_fixed_point(dt):
    """The fp32 depth of the plane is off by at most half an ulp, 2^-24 relative, so every mismatch is at most 2^-23 and delta, which only
    has to undo that rounding, stays below 2^-23; with the exact fp64 depth of the same plane as the input the mismatch itself vanishes."""
    sc, n = nr.plane()
    r = nr.normal_refine(sc['pred'], 'depth', None, sc['K'], None, n, dt=dt)
    worst = float(np.abs(r['delta']).max())
    print('plane, %s: max |delta| %.3e (bar 2^-23 = %.3e), rho_0 %.3e' % (dt.__name__, worst, 2.0 ** -23, r['stats'][0, 2]))
    assert r['stats'][0, :2].tolist() == [24 * 40, 23 * 40 + 24 * 39] and worst <= 2.0 ** -23
    inv = nr.rc.kinv(sc['K'])[0]
    right, e_r = nr._edges(sc['z'], n.astype(np.float64), inv, 0, 0.01, 0.1, np.float64)
    down, e_d = nr._edges(sc['z'], n.astype(np.float64), inv, 1, 0.01, 0.1, np.float64)
    assert right[:, :, :-1].all() and down[:, :-1].all() and not right[:, :, -1].any() and not down[:, -1].any()
    assert max(np.abs(e_r).max(), np.abs(e_d).max()) <= 1e-9           # (what is left is the fp32 rounding of the normal's components)


def test_noisy_sphere_is_smoothed_to_a_quarter_of_its_error():
    sc, n, z_true = nr.noisy_sphere(24, 40, seed=0)
    before = _rmse(sc['pred'], z_true)
    for dt in (np.float32, np.float64):
        r = nr.normal_refine(sc['pred'], 'depth', None, sc['K'], None, n, lam=0.1, iterations=32, dt=dt)
        after = _rmse(r['out'], z_true)
        print('noisy sphere, %s: RMSE %.4f mm -> %.4f mm (x %.3f), rho %.3e -> %.3e' % (dt.__name__, before, after, after / before,
                                                                                       r['stats'][0, 2], r['stats'][0, -1]))
        assert after <= 0.25 * before
    r64 = nr.normal_refine(sc['pred'], 'depth', None, sc['K'], None, n, iterations=256, dt=np.float64)
    r32 = nr.normal_refine(sc['pred'], 'depth', None, sc['K'], None, n, iterations=32, dt=np.float32)
    r64_32 = nr.normal_refine(sc['pred'], 'depth', None, sc['K'], None, n, iterations=32, dt=np.float64)
    print('32 iterations against the converged solution %.3e, fp32 against fp64 at 32 iterations %.3e'
          % (np.abs(r64_32['delta'] - r64['delta']).max(), np.abs(r32['delta'] - r64_32['delta']).max()))
    assert np.abs(r64_32['delta'] - r64['delta']).max() <= 1e-6 and np.abs(r32['delta'] - r64_32['delta']).max() <= 1e-6


def test_a_large_lambda_returns_the_input_and_the_sign_of_the_normals_is_immaterial():
    sc, n, _ = nr.noisy_sphere(24, 40, seed=0)
    for dt in (np.float32, np.float64):
        r = nr.normal_refine(sc['pred'], 'depth', None, sc['K'], None, n, lam=1e4, dt=dt)
        assert float(np.abs(r['out'] / sc['pred'].astype(dt) - 1).max()) <= 1e-6
        base = nr.normal_refine(sc['pred'], 'depth', None, sc['K'], None, n, dt=dt)
        flipped = nr.normal_refine(sc['pred'], 'depth', None, sc['K'], None, -n, dt=dt)
        by_sign = nr.normal_refine(sc['pred'], 'depth', None, sc['K'], None, n, normal_signs=(-1, -1, -1), dt=dt)
        assert np.array_equal(base['out'], flipped['out']) and np.array_equal(base['out'], by_sign['out'])
        assert np.array_equal(base['stats'], flipped['stats']) and np.abs(base['delta']).max() > 1e-5


def test_guards_return_zero_for_samples_without_a_system():
    """No valid pixel, no usable normal, and one isolated pixel: delta = 0 and the input comes back, never NaN."""
    sc, n, _ = nr.noisy_sphere(6, 9, seed=1)
    lone = np.zeros((1, 6, 9), np.float32)
    lone[0, 2, 3] = 1.0
    for mask, normal in ((np.zeros((1, 6, 9), np.float32), n), (None, np.zeros_like(n)), (None, np.full_like(n, np.nan)), (lone, n)):
        for dt in (np.float32, np.float64):
            r = nr.normal_refine(sc['pred'], 'depth', None, sc['K'], mask, normal, dt=dt)
            assert not r['delta'].any() and np.array_equal(r['out'], sc['pred'].astype(dt)) and not r['stats'][0, 1:].any()


@pytest.mark.parametrize('case', nr.CASES, ids=nr.case_id)
def test_gpu_cases_keep_their_comparisons_off_the_thresholds(case):
    ref = nr.case(case)
    print('%s: margin %.3e, stats %s' % (nr.case_id(case), ref['margin'], ref['r64']['stats'][:, :3].tolist()))
    assert ref['margin'] >= 1e-4 and ref['agree']
    assert np.isfinite(ref['r32']['delta']).all() and np.isfinite(ref['r64']['stats']).all()
    live = [b for b in range(case[0]) if b not in (case[5], case[6])]
    assert all(ref['r64']['stats'][b, 1] > 0 for b in live) and all(not ref['r64']['stats'][b].any() for b in (case[5], case[6]) if b is not None)


def test_gpu_cases_cover_what_a_tiled_stencil_can_get_wrong():
    shapes = [c[:3] for c in nr.CASES]
    assert (1, 5, 7) in shapes and (2, 19, 70) in shapes and (1, 33, 65) in shapes
    assert {c[3] for c in nr.CASES} == {'disp', 'idepth', 'depth'} and any(c[7] == 3 for c in nr.CASES)
    assert any(c[5] is not None for c in nr.CASES) and any(c[6] is not None for c in nr.CASES)
    ref = nr.case(nr.CASES[1])
    sy, sc = ref['r64']['sy'], ref['sc']
    assert sc['mask'] is not None and not sc['mask'][0].all()                                       # holes
    deg = sy['left'].astype(int) + sy['right'] + sy['up'] + sy['down']
    assert (sy['valid'][0] & (deg[0] == 0)).any() and sy['valid'][0, 2, 3] and deg[0, 2, 3] == 0     # an isolated valid pixel
    z = sy['z'][0]
    both = (z[:, :-1] > 0) & (z[:, 1:] > 0)
    assert (both & (np.abs(z[:, :-1] - z[:, 1:]) > 0.01 * np.minimum(z[:, :-1], z[:, 1:]))).any()   # a depth step that cuts edges
    n = sc['normal']
    assert np.isnan(n).any() and np.isinf(n).any() and (sy['valid'][:, None] & ~n.astype(bool).any(1, keepdims=True)).any()


# ---- settings
def test_settings_defaults_for_a_missing_block_and_missing_keys():
    m = _mod()
    assert tuple(m.settings(_Opt())) == DEFAULTS and tuple(m.settings(_Opt(normal_refine=None))) == DEFAULTS
    assert tuple(m.settings(_Opt(normal_refine={}))) == DEFAULTS and tuple(m.DEFAULTS) == DEFAULTS
    assert m.Settings._fields == ('enabled', 'lam', 'iterations', 'max_edge_ratio', 'min_cos', 'normals', 'normal_signs', 'use_mask', 'near',
                                  'far')
    s = m.settings(_Opt(normal_refine={'enabled': True, 'lambda': 2, 'iterations': 64, 'normal_signs': [1, -1, -1], 'far': 1200}))
    assert s.enabled and s.lam == 2.0 and s.iterations == 64 and s.normal_signs == (1, -1, -1) and s.far == 1200.0
    s = m.settings(_Opt(normal_refine=_Opt(normals='batch', min_cos=0, near=100)))                  # an attribute block
    assert not s.enabled and s.normals == 'batch' and s.min_cos == 0.0 and s.near == 100.0
    assert m.active(_Opt(normal_refine={'enabled': True})) and not m.active(_Opt()) and not m.active(_Opt(normal_refine={'iterations': 8}))


@pytest.mark.parametrize('key,value', [
    ('enabled', 1), ('enabled', 'true'), ('enabled', None), ('use_mask', 'yes'), ('use_mask', 0),
    ('lambda', 0), ('lambda', -0.1), ('lambda', None), ('lambda', '0.1'), ('lambda', float('inf')), ('lambda', float('nan')), ('lambda', True),
    ('iterations', 0), ('iterations', 257), ('iterations', 32.0), ('iterations', True), ('iterations', '32'), ('iterations', None),
    ('max_edge_ratio', 0), ('max_edge_ratio', -0.01), ('max_edge_ratio', None), ('max_edge_ratio', float('inf')),
    ('min_cos', 1), ('min_cos', -0.1), ('min_cos', None), ('min_cos', 'small'), ('min_cos', float('nan')),
    ('normals', 'auto'), ('normals', 'geometric'), ('normals', None), ('normals', True),
    ('normal_signs', [1, 1]), ('normal_signs', [1, 1, 0]), ('normal_signs', [1, 1, 2]), ('normal_signs', 1), ('normal_signs', None),
    ('normal_signs', [True, 1, 1]), ('normal_signs', '111'),
    ('near', -1.0), ('near', None), ('near', float('nan')), ('near', True), ('far', 0.0), ('far', -5), ('far', 'inf'), ('far', False)])
def test_settings_names_the_malformed_key(key, value):
    for enabled in (False, True):
        with pytest.raises(ValueError, match='normal_refine.' + key):
            _mod().settings(_Opt(normal_refine={'enabled': enabled, key: value} if key != 'enabled' else {key: value}))


def test_settings_far_must_exceed_near_and_a_non_block_is_refused():
    m = _mod()
    with pytest.raises(ValueError, match='far'):
        m.settings(_Opt(normal_refine={'near': 500.0, 'far': 500.0}))
    assert m.settings(_Opt(normal_refine={'near': 500.0, 'far': 500.5})).far == 500.5
    for bad in (True, 3, 'on', [1]):
        with pytest.raises(ValueError, match='normal_refine'):
            m.settings(_Opt(normal_refine=bad))


def test_refine_config_is_eval_faceDP_with_the_block_spelled_out_and_no_other_config_is_on():
    from dualpixelface_amd import load_option
    m = _mod()
    base = json.load(open(os.path.join(ROOT, 'config_', 'eval_faceDP.json')))
    ours = json.load(open(os.path.join(ROOT, 'config_', 'eval_faceDP_refine.json')))
    block = ours.pop('normal_refine')
    keys = [('lambda' if f == 'lam' else f) for f in m.Settings._fields]
    assert block == dict(zip(keys, DEFAULTS), enabled=True, normal_signs=[1, 1, 1]) and ours == base
    for name in sorted(f[:-5] for f in os.listdir(os.path.join(ROOT, 'config_')) if f.endswith('.json')):
        s = m.settings(load_option(name))
        assert tuple(s) == ((True,) + DEFAULTS[1:] if name == 'eval_faceDP_refine' else DEFAULTS), name


# ---- apply
def test_apply_off_or_training_returns_results_untouched():
    m = _mod()
    pred = torch.zeros(1, 1, 4, 4)
    results = {'pred_depth': pred}
    for opt, training in ((_Opt(), False), (_Opt(normal_refine={'enabled': False, 'iterations': 8}), False),
                          (_Opt(normal_refine={'enabled': True}), True)):
        out = m.apply(opt, results, {}, training=training)           # no K in the batch: nothing looks for one
        assert out is results and list(results) == ['pred_depth'] and results['pred_depth'] is pred


def test_apply_on_names_what_is_missing_and_leaves_results_alone():
    from dualpixelface_amd._lib import DpfError
    m = _mod()
    pred, pn = torch.zeros(1, 1, 4, 6), torch.zeros(1, 1, 3, 4, 6)
    K, ab = torch.eye(3).unsqueeze(0), torch.tensor([[1.0, 2.0]])
    on = {'enabled': True}

    def check(opt, results, batch, match, error=NotImplementedError):
        before = dict(results)
        with pytest.raises(error, match=match):
            m.apply(opt, results, batch)
        assert list(results) == list(before) and all(results[k] is before[k] for k in before)

    check(_Opt(normal_refine=on), {'pred_depth': pred, 'pred_normal': pn}, {'abvalue': ab}, r"batch\['K'\]")
    check(_Opt(normal_refine=on), {'pred_depth': pred, 'pred_normal': pn}, {'K': K}, 'abvalue')
    check(_Opt(normal_refine=on, model=_Opt(target_type='idepth')), {'pred_depth': pred, 'pred_normal': pn}, {'K': K}, 'abvalue')
    check(_Opt(normal_refine=on), {'pred_depth': None, 'pred_normal': pn}, {'K': K, 'abvalue': ab}, 'pred_depth')
    check(_Opt(normal_refine=on), {'pred_depth': pred}, {'K': K, 'abvalue': ab}, 'pred_normal')              # a model without a normal head
    check(_Opt(normal_refine=on), {'pred_depth': pred, 'pred_normal': None}, {'K': K, 'abvalue': ab, 'normal': pn[:, 0]}, 'pred_normal')
    check(_Opt(normal_refine=dict(on, normals='batch')), {'pred_depth': pred, 'pred_normal': pn}, {'K': K, 'abvalue': ab}, r"batch\['normal'\]")
    # everything there: the operator is reached, and refuses the CPU tensors (a depth model needs no abvalue; the fit stands in for it)
    check(_Opt(normal_refine=on), {'pred_depth': pred, 'pred_normal': pn}, {'K': K, 'abvalue': ab}, 'GPU tensors', DpfError)
    check(_Opt(normal_refine=on, model=_Opt(target_type='depth')), {'pred_depth': pred, 'pred_normal': pn}, {'K': K}, 'GPU tensors', DpfError)
    check(_Opt(normal_refine=dict(on, normals='batch')), {'pred_depth': pred, 'abvalue': ab}, {'K': K, 'normal': pn[:, 0]}, 'GPU tensors', DpfError)


# ---- the operator and the header
def test_ops_refuse_bad_operands_before_any_library_call(monkeypatch):
    from dualpixelface_amd import ops
    from dualpixelface_amd._lib import DpfError

    def no_library():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(ops, 'lib', no_library)
    pred, K, ab, n = torch.zeros(1, 2, 8, 8), torch.eye(3).unsqueeze(0), torch.ones(1, 2), torch.zeros(1, 3, 8, 8)
    with pytest.raises(DpfError, match='GPU tensors'):
        ops.normal_refine(pred, K, n, ab=ab)
    with pytest.raises(DpfError, match='target_type'):
        ops.normal_refine(pred, K, n, ab=ab, target_type='inverse')
    with pytest.raises(DpfError, match='needs ab'):
        ops.normal_refine(pred, K, n)
    for kw, match in ((dict(iterations=0), 'iterations'), (dict(iterations=257), 'iterations'), (dict(iterations=8.0), 'iterations must be an integer'),
                      (dict(lam=0.0), 'lam'), (dict(lam=float('inf')), 'lam'), (dict(lam=float('nan')), 'lam'), (dict(min_cos=1.0), 'min_cos'),
                      (dict(min_cos=-0.5), 'min_cos'), (dict(max_edge_ratio=0.0), 'max_edge_ratio'), (dict(normal_signs=(1, 1)), 'normal_signs'),
                      (dict(normal_signs=(1, 0, 1)), 'normal_signs')):
        with pytest.raises(DpfError, match=match):
            ops.normal_refine(pred, K, n, ab=ab, **kw)


def test_header_declares_the_new_entry_points():
    from dualpixelface_amd import _lib
    protos = _lib.parse_header()
    assert len(protos['dpf_normal_refine'][1]) == 23 and protos['dpf_normal_refine'][0] is _lib._CTYPES['int']
    assert protos['dpf_normal_refine_workspace_bytes'][0] is _lib._CTYPES['long long']
    assert [n for _, n in protos['dpf_normal_refine_workspace_bytes'][1]] == ['B', 'H', 'W']
    names = [n for _, n in protos['dpf_normal_refine'][1]]
    assert names[:8] == ['pred', 'pred_batch_stride', 'target_type', 'ab', 'Kmat', 'mask', 'normal', 'normal_signs_host']
    assert names[8:] == ['B', 'H', 'W', 'z_near', 'z_far', 'max_edge_ratio', 'min_cos', 'lambda', 'iterations', 'ws', 'ws_bytes', 'out',
                         'out_batch_stride', 'stats', 'stream']
    make = open(os.path.join(ROOT, 'dualpixelface_amd', 'csrc', 'Makefile')).read()
    assert '$(OBJDIR)/normal_refine.o: CXXFLAGS += -ffp-contract=off' in make
