"""The shading block without a GPU: its settings and refusals, the prototypes of its C ABI, and the numpy restatement of
tests/shading_cpu.py on the synthetic scene -- the known light is recovered, and the reweighted passes shed specular outliers.

Bars.  Recovery (ridge 0, no reweighting, gamma 1, exact fp64 intensities): max |L - L_true| <= cond(A) N 2^-53 max |L_true|, the
normal-equations bound with the Gram sums' own N 2^-53 relative perturbation; numpy gives 1.0e-11 at 37 x 53 and 3.0e-13 at 64 x 96 where
the bar is 3.2e-10 and 9.8e-10 (cond(A) = 1.0e3, asserted < 1e4).  Outliers: the bar is the issue's, a third of the plain fit's maximum shading error; numpy gives
0.0425 -> 0.0072 at 37 x 53 and 0.0396 -> 0.0051 at 64 x 96."""
import numpy as np
import pytest
import torch

from dualpixelface_amd import shading, synthetic_shading as syn
from dualpixelface_amd.config import Option
from tests import shading_cpu as sc

SIZES = ((37, 53), (64, 96))


def _option(block=None, model='stereodpnet'):
    return Option({'model_name': model, **({} if block is None else {'shading': block})})


def test_defaults_and_an_absent_block_is_off():
    assert shading.settings(Option({})) == shading.DEFAULTS and not shading.active(Option({}))
    assert shading.settings(_option({})) == shading.DEFAULTS
    d = shading.DEFAULTS
    assert (d.enabled, d.normals, d.normal_signs, d.order, d.gamma, d.min_value, d.max_value, d.iterations, d.f_scale, d.ridge, d.min_pixels,
            d.shade_floor, d.albedo_max, d.use_mask, d.report) == (False, 'auto', (1, 1, 1), 2, 2.2, 0.02, 0.98, 3, 0.05, 1e-6, 72, 0.05, 4.0,
                                                                    True, False)
    assert d.relight == shading.Relight(False, (0, 0, 0), None, 1.0)
    s = shading.settings(_option({'enabled': True, 'relight': {'enabled': True, 'rotate_deg': [0, 30, 0]}, 'normal_signs': [1, -1, 1]}))
    assert s.enabled and s.relight.enabled and s.relight.rotate_deg == (0.0, 30.0, 0.0) and s.normal_signs == (1, -1, 1)
    assert shading.RESULT_KEYS == ('light', 'shading', 'albedo', 'shading_valid', 'shading_stats', 'relit')


BAD = [('enabled', 1), ('normals', 'measured'), ('normal_signs', [1, 1]), ('normal_signs', [1, 0, 1]), ('normal_signs', [True, 1, 1]),
       ('order', 3), ('order', 2.0), ('gamma', 0), ('gamma', 'two'), ('min_value', -0.1), ('min_value', 1.0), ('max_value', 0.01),
       ('max_value', 1.5), ('iterations', 9), ('iterations', -1), ('iterations', 1.5), ('f_scale', 0), ('ridge', -1e-6),
       ('ridge', float('nan')), ('min_pixels', 0), ('min_pixels', 7.5), ('shade_floor', 0), ('albedo_max', -1), ('use_mask', 'yes'),
       ('report', 0), ('relight', 3)]


@pytest.mark.parametrize('key,value', BAD, ids=['%s=%r' % kv for kv in BAD])
def test_a_malformed_key_is_refused_by_name(key, value):
    with pytest.raises(ValueError, match=r'shading(\.%s)? must be ' % key if key == 'relight' else r'shading\.%s must be ' % key):
        shading.settings(_option({key: value}))              # refused whether or not the block is enabled


BAD_RELIGHT = [('enabled', 'on'), ('rotate_deg', [0, 30]), ('rotate_deg', [0, 'a', 0]), ('rotate_deg', 30), ('coefficients', [[1.0] * 9] * 2),
               ('coefficients', [[1.0] * 8] * 3), ('coefficients', [[float('inf')] * 9] * 3), ('gain', -1), ('gain', None)]


@pytest.mark.parametrize('key,value', BAD_RELIGHT, ids=['relight.%s=%r' % kv for kv in BAD_RELIGHT])
def test_a_malformed_relight_key_is_refused_by_name(key, value):
    with pytest.raises(ValueError, match=r'shading\.relight\.%s must be ' % key):
        shading.settings(_option({'relight': {key: value}}))


@pytest.mark.parametrize('model', shading.NO_NORMAL_HEAD)
def test_predicted_normals_are_refused_for_a_model_without_a_normal_head(model):
    assert model in ('dpnet', 'psmnet', 'stereonet')
    with pytest.raises(NotImplementedError, match=model):
        shading.check_model(_option({'enabled': True, 'normals': 'predicted'}, model))
    shading.check_model(_option({'enabled': False, 'normals': 'predicted'}, model))
    shading.check_model(_option({'enabled': True, 'normals': 'auto'}, model))
    shading.check_model(_option({'enabled': True, 'normals': 'predicted'}, 'stereodpnet'))
    shading.check_model(_option({'enabled': True, 'normals': 'predicted'}, 'nnet'))


def test_the_prototypes_are_in_the_header():
    from dualpixelface_amd._lib import parse_header
    protos = parse_header()
    assert [n for _, n in protos['dpf_shading_workspace_bytes'][1]] == ['B', 'H', 'W']
    fit = [n for _, n in protos['dpf_shading_fit'][1]]
    assert fit[:5] == ['view', 'normal', 'mask', 'norm_host', 'normal_signs_host'] and fit[-4:] == ['light', 'stats', 'gram_out', 'stream']
    app = [n for _, n in protos['dpf_shading_apply'][1]]
    assert app[-5:] == ['shading', 'albedo', 'valid', 'relit', 'stream'] and 'rotation_host' in app and 'albedo_label' in app


def test_the_relight_config_loads():
    from dualpixelface_amd import load_option
    s = shading.settings(load_option('eval_faceDP_relight'))
    assert s.enabled and s.relight.enabled and s.relight.rotate_deg == (0.0, 30.0, 0.0)
    assert not shading.active(load_option('eval_faceDP'))


@pytest.mark.parametrize('H,W', SIZES)
def test_the_restatement_recovers_the_known_light(H, W):
    s = syn.scene(H, W)
    px = sc.pixels(s['view'], s['normal'], s['mask'], gamma=1)
    assert np.array_equal(px['counted'], s['inside']) and np.array_equal(px['applicable'], s['inside'])
    shade = s['shading'][:, s['inside']]
    assert shade.min() > 0.3 and shade.max() < 0.98
    r = sc.fit(s['intensity'], px['nh'], px['counted'], iterations=0, ridge=0.0)
    N = int(r['stats'][0])
    err, bar = np.abs(r['light64'] - syn.LIGHT).max(), r['cond'] * N * 2.0 ** -53 * np.abs(syn.LIGHT).max()
    print('%d x %d: N %d, cond(A) %.3e, max |L - L_true| %.3e (bar %.3e), RMS %s' % (H, W, N, r['cond'], err, bar, r['stats'][4:7]))
    assert r['cond'] < 1e4 and r['stats'][1] == 1 and err <= bar
    assert (r['stats'][4:7] < 1e-6).all()
    # the stored float32 view brings the fp32 rounding of the values and nothing more
    r32 = sc.fit(px['I'], px['nh'], px['counted'], iterations=0, ridge=0.0)
    assert np.abs(r32['light64'] - syn.LIGHT).max() <= 1e-5


@pytest.mark.parametrize('H,W', SIZES)
def test_reweighting_sheds_the_specular_outliers(H, W):
    s = syn.scene(H, W, outliers=0.05, outlier_value=0.95)
    px = sc.pixels(s['view'], s['normal'], s['mask'], gamma=1)
    Y = syn.basis(px['nh'][s['inside']])
    errs = []
    for iterations in (0, 3):
        r = sc.fit(px['I'], px['nh'], px['counted'], iterations=iterations)
        errs.append(np.abs(Y @ r['light64'].T - Y @ syn.LIGHT.T).max())
    print('%d x %d, %d outliers: max shading error %.4f -> %.4f' % (H, W, s['outlier'].sum(), errs[0], errs[1]))
    assert 0.04 <= s['outlier'].sum() / s['inside'].sum() <= 0.06 and errs[1] < errs[0] / 3.0


def test_the_fit_does_not_depend_on_the_signs_and_a_small_sample_is_invalid():
    s = syn.scene(37, 53, albedo='texture')
    fits = []
    for signs in ((1, 1, 1), (1, -1, 1)):
        px = sc.pixels(s['view'], s['normal'], s['mask'], signs=signs, gamma=1)
        fits.append(sc.fit(px['I'], px['nh'], px['counted']))
    parity = np.array([1, -1, 1, 1, -1, -1, 1, 1, 1], np.float64)
    assert np.abs(fits[0]['light64'] - fits[1]['light64'] * parity).max() <= 1e-12
    tiny = syn.scene(5, 7)
    px = sc.pixels(tiny['view'], tiny['normal'], tiny['mask'], gamma=1)
    r = sc.fit(px['I'], px['nh'], px['counted'])
    assert r['stats'][0] == 23 and r['stats'][1] == 0 and not r['light'].any()


def test_the_report_table_adds_up():
    opt = _option({'enabled': True, 'report': True})
    stats = torch.zeros(3, 16, dtype=torch.float64)
    stats[:, 1] = torch.tensor([1.0, 0.0, 1.0])
    stats[:, 7:10] = torch.tensor([[0.1, 0.2, 0.3], [9.0, 9.0, 9.0], [0.3, 0.4, 0.5]])
    stats[:, 10:13] = torch.tensor([[0.01, 0.02, 0.03], [-1.0, -1.0, -1.0], [-1.0, -1.0, -1.0]])
    stats[:, 13] = torch.tensor([50.0, 0.0, 0.0])
    table = shading.accumulate(opt, {'shading_stats': stats}, None)
    table = shading.accumulate(opt, {'shading_stats': stats}, table)
    rows = shading.report_rows(table.tolist())
    assert rows['samples'] == 4 and rows['albedo_samples'] == 2
    assert np.allclose(rows['rms_residual'], [0.2, 0.3, 0.4]) and np.allclose(rows['albedo_error'], [0.01, 0.02, 0.03])
    assert shading.accumulate(_option({'enabled': True}), {'shading_stats': stats}, None) is None
    assert shading.report_rows(shading.new_table('cpu').tolist()) == {'samples': 0.0, 'rms_residual': None, 'albedo_samples': 0.0,
                                                                      'albedo_error': None}


def test_the_rotation_is_rz_ry_rx():
    from dualpixelface_amd import ops
    assert ops.shading_rotation((0, 0, 0)) == (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
    R = np.array(ops.shading_rotation((10, 30, -20))).reshape(3, 3)
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and np.isclose(np.linalg.det(R), 1.0)
    Ry = np.array(ops.shading_rotation((0, 90, 0))).reshape(3, 3)
    assert np.allclose(Ry @ [0, 0, 1], [1, 0, 0], atol=1e-15)                 # about y: z turns to x
    Rzx = np.array(ops.shading_rotation((90, 0, 90))).reshape(3, 3)
    assert np.allclose(Rzx @ [0, 1, 0], [0, 0, 1], atol=1e-15)                # Rx first (y -> z), then Rz leaves z alone
