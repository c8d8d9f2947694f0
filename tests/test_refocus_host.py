"""The refocus block without a GPU: its settings and refusals, the prototypes of its C ABI, what apply() does with the block off, and the
properties of the numpy restatement of tests/refocus_cpu.py on the two-plane scene of dualpixelface_amd/synthetic_refocus.py (near plane
at d = 1.5, far plane at d = -2, larger is nearer)."""
import numpy as np
import pytest

from dualpixelface_amd import refocus, synthetic_refocus as syn
from dualpixelface_amd.config import Option
from tests import refocus_cpu as rc

H, W = 29, 41
RADIUS = 6


def _option(block=None, **top):
    return Option(dict(top, **({} if block is None else {'refocus': block})))


def test_defaults_and_an_absent_block_is_off():
    assert refocus.settings(Option({})) == refocus.DEFAULTS and not refocus.active(Option({}))
    assert refocus.settings(_option({})) == refocus.DEFAULTS
    assert tuple(refocus.DEFAULTS) == (False, 'view', 'mask_mean', (0.5, 0.5), 0.0, 4.0, 16, 'auto', 2.2, 1.0, True)
    s = refocus.settings(_option({'enabled': True, 'focus': 'point', 'focus_point': [0.25, 1], 'near_sign': -1, 'max_radius': 32}))
    assert s.enabled and s.focus == 'point' and s.focus_point == (0.25, 1.0) and s.near_sign == -1 and s.max_radius == 32
    assert refocus.RESULT_KEYS == ('refocused', 'defocus', 'refocus_stats')


BAD = [('enabled', 1), ('source', 'albedo'), ('focus', 'nearest'), ('focus', 3), ('focus_point', [0.5]), ('focus_point', [0.5, 1.5]),
       ('focus_point', [0.5, 'a']), ('focus_value', float('inf')), ('focus_value', None), ('aperture', -1), ('aperture', 'wide'),
       ('max_radius', 0), ('max_radius', 33), ('max_radius', 8.0), ('near_sign', 0), ('near_sign', True), ('near_sign', 'far'),
       ('gamma', 0), ('gain', -0.5), ('use_mask', 'yes')]


@pytest.mark.parametrize('key,value', BAD, ids=['%s=%r' % kv for kv in BAD])
def test_a_malformed_key_is_refused_by_name(key, value):
    with pytest.raises(ValueError, match=r'refocus\.%s must be ' % key):
        refocus.settings(_option({key: value}))              # refused whether or not the block is enabled
    with pytest.raises(ValueError, match=r'refocus\.%s must be ' % key):
        refocus.active(_option({key: value, 'enabled': True} if key != 'enabled' else {key: value}))


def test_a_block_that_is_no_block_is_refused():
    with pytest.raises(ValueError, match='refocus must be a block'):
        refocus.settings(_option(3))


def test_the_prototypes_are_in_the_header():
    from dualpixelface_amd._lib import parse_header
    protos = parse_header()
    assert [n for _, n in protos['dpf_refocus_workspace_bytes'][1]] == ['B', 'H', 'W']
    plan = [n for _, n in protos['dpf_refocus_plan'][1]]
    assert plan == ['pred', 'pred_batch_stride', 'target_type', 'ab', 'mask', 'B', 'H', 'W', 'focus_mode', 'focus_x', 'focus_y', 'focus_value',
                    'aperture', 'max_radius', 'near_sign', 'ws', 'ws_bytes', 'defocus', 'stats', 'stream']
    render = [n for _, n in protos['dpf_refocus_render'][1]]
    assert render == ['image', 'normalised', 'norm_host', 'defocus', 'stats', 'B', 'H', 'W', 'max_radius', 'gamma', 'gain', 'ws', 'ws_bytes', 'out',
                      'stream']


def test_the_binding_states_the_kernel_constants():
    from dualpixelface_amd import ops
    assert ops.REFOCUS_STATS == 8 and ops.REFOCUS_FOCUS == {'mask_mean': 0, 'point': 1, 'value': 2}
    assert list(ops.REFOCUS_RADII) == list(range(1, 33)) and ops.REFOCUS_TILE == 16
    for point in ((0.5, 0.5), (0.0, 1.0), (0.999, 0.26)):
        assert ops.refocus_focus_pixel(point, 29, 41) == rc.focus_pixel(point, 29, 41)
    assert ops.refocus_focus_pixel((0.5, 1.0), 29, 41) == (20, 28)


class _NoLibrary(object):
    def __getattr__(self, name):
        raise AssertionError('the library was touched: %s' % name)


def test_apply_with_the_block_off_or_in_training_returns_the_results_untouched(monkeypatch):
    from dualpixelface_amd import ops
    monkeypatch.setattr(ops, 'lib', _NoLibrary())
    monkeypatch.setattr(ops, 'refocus', _NoLibrary())
    results = {'pred_depth': object()}
    before = dict(results)
    for opt, training in ((Option({}), False), (_option({'enabled': False, 'aperture': 9.0}), False), (_option({'enabled': True}), True)):
        assert refocus.apply(opt, results, {}, training=training) is results and results == before


def test_what_is_missing_is_refused_by_name(monkeypatch):
    from dualpixelface_amd import ops
    monkeypatch.setattr(ops, 'refocus', _NoLibrary())
    view = np.zeros((1, 3, 4, 4), np.float32)
    on = _option({'enabled': True, 'source': 'relit'})
    results = {'pred_depth': object()}
    with pytest.raises(NotImplementedError, match=r'shading\.relight\.enabled'):
        refocus.apply(on, results, {}, guide=view)
    assert list(results) == ['pred_depth']
    with pytest.raises(NotImplementedError, match='pred_depth'):
        refocus.apply(_option({'enabled': True}), {}, {}, guide=view)
    with pytest.raises(NotImplementedError, match='abvalue'):
        refocus.apply(_option({'enabled': True}, model=Option({'target_type': 'idepth'})), results, {}, guide=view)
    with pytest.raises(NotImplementedError, match='reference view'):
        refocus.apply(_option({'enabled': True}), results, {})


def test_the_refocus_config_loads():
    from dualpixelface_amd import load_option
    s = refocus.settings(load_option('eval_faceDP_refocus'))
    assert s.enabled and s == refocus.DEFAULTS._replace(enabled=True)
    assert not refocus.active(load_option('eval_faceDP'))


# ---- the restatement on the synthetic scene
def _scene(**kw):
    return syn.scene(H, W, seed=2, **kw)


def _render(s, d_f, sign=1, aperture=4.0, **kw):
    c = rc.defocus(s['disparity'], d_f, aperture, RADIUS)
    return rc.render(s['view'], s['disparity'], c, sign, RADIUS, **kw), c


def test_the_scene_is_what_it_says():
    s = _scene(holes=0.1)
    y0, y1, x0, x1 = s['box']
    assert s['near'].sum() == (y1 - y0) * (x1 - x0) and 0 < s['near'].sum() < H * W
    live = ~s['hole']
    assert 0.04 < s['hole'].mean() < 0.2 and np.isnan(s['disparity'][s['hole']]).all()
    assert (s['disparity'][live & s['near']] == 1.5).all() and (s['disparity'][live & ~s['near']] == -2.0).all()
    assert s['encoded'][:, s['near']].min() >= 0.55 and s['encoded'][:, ~s['near']].max() <= 0.45
    assert np.abs(rc.encoded(s['view']) - s['encoded']).max() < 1e-6
    assert rc.focus(s['disparity'], s['mask']) == (1.5, int((live & s['near']).sum()), 1)
    assert rc.focus(s['disparity'], s['mask'] * 0) == (0.0, 0, 0)
    assert rc.focus(s['disparity'], None, 'value', value=0.25) == (0.25, 0, 1)


def test_no_aperture_returns_the_clamped_view():
    s = _scene(holes=0.05)
    for dtype in (np.float64, np.float32):
        out, c = _render(s, 0.3, aperture=0.0, dtype=dtype)
        assert not c.any() and out.dtype == dtype and np.array_equal(out, rc.encoded(s['view']).astype(dtype))


def test_a_constant_image_stays_constant():
    s = _scene(constant=0.4)
    d = np.random.RandomState(5).randn(H, W).astype(np.float32) * 2
    out = rc.render(s['view'], d, rc.defocus(d, 0.1, 4.0, RADIUS), 1, RADIUS)
    v = rc.encoded(s['view']).astype(np.float64)
    assert np.ptp(rc.defocus(d, 0.1, 4.0, RADIUS)) > RADIUS and np.abs(out - v).max() <= 1e-12


def test_focus_on_the_near_plane_leaves_it_unchanged_and_focus_on_the_far_plane_lets_it_spill():
    s = _scene()
    v = rc.encoded(s['view']).astype(np.float64)
    near = s['near']
    out, c = _render(s, 1.5)                                            # near plane in focus, far plane at r = min(14, RADIUS)
    assert (c[near] == 0).all() and (np.abs(c[~near]) == RADIUS).all()
    assert np.array_equal(out[:, near], v[:, near])                     # the blurred background does not bleed over the sharp foreground
    assert (out[:, ~near] != v[:, ~near]).mean() > 0.9
    out, c = _render(s, -2.0)                                           # far plane in focus: the blurred near plane spreads over it
    assert (c[~near] == 0).all() and (c[near] == RADIUS).all()
    y0, y1, x0, x1 = s['box']
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    gap = np.hypot(np.maximum(np.maximum(y0 - ys, ys - (y1 - 1)), 0), np.maximum(np.maximum(x0 - xs, xs - (x1 - 1)), 0))
    band = ~near & (gap < RADIUS + 1)                                   # far pixels within the near plane's blur (r + 1) of its edge
    changed = (out != v).any(0)
    assert changed[band].all() and not changed[~near & ~band].any()
    assert (out[:, band] > v[:, band]).mean() > 0.95                    # what arrives is the brighter plane
    assert changed[near].mean() > 0.9


def test_flipping_the_near_sign_swaps_which_side_bleeds():
    s = _scene()
    v = rc.encoded(s['view']).astype(np.float64)
    near = s['near']
    for d_f, sharp in ((1.5, near), (-2.0, ~near)):
        keeps = {sign: np.array_equal(_render(s, d_f, sign)[0][:, sharp], v[:, sharp]) for sign in (1, -1)}
        # the sharp plane is kept exactly when it is the nearer one under that sign
        assert keeps == ({1: True, -1: False} if sharp is near else {1: False, -1: True}), (d_f, keeps)


def test_the_depth_targets_become_the_same_disparity():
    z = np.array([[0.5, 1.0, 2.0, 0.0]], np.float32)
    ab = (0.25, -3.0)
    with np.errstate(all='ignore'):
        want = (np.float32(-3.0) / z + np.float32(0.25)).astype(np.float32)
    assert np.array_equal(rc.disparity(z, ab, 'depth'), want) and not np.isfinite(want[0, 3])
    assert rc.disparity(want, ab, 'idepth') is want and rc.disparity(want, None, 'disp') is want
    assert rc.near_sign('auto', ab) == -1 and rc.near_sign('auto', None) == 1 and rc.near_sign(1, ab) == 1
    assert rc.defocus(want, 0.0, 4.0, 16)[0, 3] == 0
