"""Occlusion handling of the multi-view loss on the host (no GPU): multiview_occlusion.settings, the loss bank handing the record on, the
shipped configs, the occluder scene against its closed-form visibility, and the proof of the oracle tests/test_gpu_multiview_occlusion.py
measures the kernels against (tests/multiview_occ_cpu.py)."""
import numpy as np
import pytest
import torch

from tests import multiview_cpu as mc
from tests import multiview_occ_cpu as oc

DEFAULTS = ('mean', 'none', 2, 0.01)
MULTIVIEW_DEFAULTS = (3, 0.8, 1.0, 0.1, 'center', 1e-3)


class _Opt(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _settings(block, **top):
    from dualpixelface_amd import multiview_occlusion
    return multiview_occlusion.settings(_Opt(model=_Opt(multiview_occlusion=block, **top)))


# ---- settings
def test_settings_defaults_and_overrides():
    from dualpixelface_amd import multiview_occlusion as mo
    assert tuple(mo.settings(_Opt())) == DEFAULTS and tuple(mo.settings(_Opt(model=_Opt()))) == DEFAULTS
    assert tuple(_settings(None)) == DEFAULTS and tuple(_settings({})) == DEFAULTS and tuple(mo.DEFAULTS) == DEFAULTS
    assert mo.Settings._fields == ('reduce', 'visibility', 'cell', 'tolerance')
    s = _settings({'reduce': 'min', 'visibility': 'zbuffer', 'cell': 4, 'tolerance': 0})
    assert tuple(s) == ('min', 'zbuffer', 4, 0.0) and isinstance(s.tolerance, float) and isinstance(s.cell, int)
    s = _settings(_Opt(reduce='min', cell=1))                        # an attribute block, as config.Option makes one
    assert tuple(s) == ('min', 'none', 1, 0.01)
    # no top-level fallback: the model's own keys of the same names are not read
    assert tuple(_settings(None, reduce='min', cell=4, tolerance=0.5)) == DEFAULTS


@pytest.mark.parametrize('key,value', [
    ('reduce', 'max'), ('reduce', None), ('reduce', 1), ('reduce', True), ('reduce', ['min']),
    ('visibility', 'label'), ('visibility', 'depth'), ('visibility', None), ('visibility', True), ('visibility', 0),
    ('cell', 0), ('cell', 3), ('cell', 8), ('cell', 2.0), ('cell', True), ('cell', None), ('cell', '2'),
    ('tolerance', -0.01), ('tolerance', float('inf')), ('tolerance', float('nan')), ('tolerance', None), ('tolerance', '0.01'), ('tolerance', True),
])
def test_a_malformed_value_is_refused_by_key(key, value):
    with pytest.raises(ValueError, match=r'multiview_occlusion\.%s must be ' % key):
        _settings({key: value})


def test_a_non_block_is_refused_and_the_multiview_block_keeps_its_six_fields():
    from dualpixelface_amd import multiview
    for bad in (True, 3, 'on', [1]):
        with pytest.raises(ValueError, match='multiview_occlusion must be a block'):
            _settings(bad)
    assert multiview.Settings._fields == ('select_view', 'weight_ssim', 'alpha', 'scale', 'image', 'min_depth')
    assert tuple(multiview.DEFAULTS) == MULTIVIEW_DEFAULTS
    opt = _Opt(model=_Opt(multiview_occlusion={'reduce': 'min'}, multiview={'alpha': 0.0}))
    assert tuple(multiview.settings(opt)) == (3, 0.8, 0.0, 0.1, 'center', 1e-3)


# ---- the loss bank and the configs
def _sel(loss_type, config='train_faceDP_dpnet', **over):
    from dualpixelface_amd import load_option, losses
    return losses.loss_selector(load_option(config, loss_type=loss_type, lambdas=[1.0] * len(loss_type), **over))


def test_the_loss_bank_keeps_settings_and_hands_the_occlusion_record_to_the_operator(monkeypatch):
    from dualpixelface_amd import ops
    sel = _sel(['multiview'])
    assert tuple(sel.loss_func[0].settings) == MULTIVIEW_DEFAULTS and tuple(sel.loss_func[0].occlusion) == DEFAULTS and sel.label_free()
    occ = {'reduce': 'min', 'visibility': 'zbuffer', 'cell': 4, 'tolerance': 0.02}
    assert _sel(['multiview', 'smoothness'], multiview_occlusion=occ).label_free()
    sel = _sel(['multiview'], multiview_occlusion=occ)
    fn = sel.loss_func[0]
    assert tuple(fn.settings) == MULTIVIEW_DEFAULTS and tuple(fn.occlusion) == ('min', 'zbuffer', 4, 0.02) and sel.label_free()
    with pytest.raises(ValueError, match=r'multiview_occlusion\.cell'):
        _sel(['multiview'], multiview_occlusion={'cell': 3})
    seen = []
    monkeypatch.setattr(ops, 'multiview_loss', lambda *a, **k: seen.append(k) or torch.zeros(()))
    batch = {'center': torch.zeros(1, 3, 4, 6), 'centers': torch.zeros(1, 9, 5, 7), 'K': torch.eye(3)[None], 'P': torch.eye(4)[None],
             'Ks': torch.eye(3).repeat(1, 3, 1, 1), 'Ps': torch.eye(4).repeat(1, 3, 1, 1)}
    out = sel.forward({'pred_depth': torch.ones(1, 1, 4, 6)}, batch, target_type='depth')
    assert 'multiview_loss' in out and len(seen) == 1
    k = seen[0]
    assert (k['reduce'], k['visibility'], k['cell'], k['tolerance']) == ('min', 'zbuffer', 4, 0.02) and k['weight_ssim'] == 0.8
    _sel(['multiview']).forward({'pred_depth': torch.ones(1, 1, 4, 6)}, batch, target_type='depth')
    k = seen[1]
    assert (k['reduce'], k['visibility'], k['cell'], k['tolerance']) == DEFAULTS


def test_the_shipped_occlusion_config_loads_with_min_and_zbuffer():
    from dualpixelface_amd import load_option, losses, multiview, multiview_occlusion
    opt = load_option('train_faceDP_dpnet_multiview_occlusion')
    assert opt.model_name == 'dpnet' and opt.model_config == 'config_multiview_occlusion' and opt.use_multi and opt.use_center_img
    assert opt.model.loss_type == ['multiview'] and opt.model.lambdas == [1.0]
    assert tuple(multiview.settings(opt)) == MULTIVIEW_DEFAULTS
    assert tuple(multiview_occlusion.settings(opt)) == ('min', 'zbuffer', 2, 0.01)
    sel = losses.loss_selector(opt)
    assert sel.label_free() and tuple(sel.loss_func[0].occlusion) == ('min', 'zbuffer', 2, 0.01)
    assert tuple(multiview_occlusion.settings(load_option('train_faceDP_dpnet_multiview'))) == DEFAULTS


def test_operator_refuses_malformed_modes_before_it_looks_at_the_tensors():
    from dualpixelface_amd import ops
    from dualpixelface_amd._lib import DpfError
    pred, img, src = torch.zeros(1, 1, 4, 6), torch.zeros(1, 3, 4, 6), torch.zeros(1, 2, 3, 5, 7)
    args = (pred, img, src, torch.eye(3)[None], torch.eye(4)[None], torch.eye(3).repeat(1, 2, 1, 1), torch.eye(4).repeat(1, 2, 1, 1))
    for kw, what in ((dict(reduce='max'), 'reduce'), (dict(visibility='label'), 'visibility'), (dict(cell=3), 'cell'), (dict(cell=2.0), 'cell'),
                     (dict(tolerance=-1.0), 'tolerance'), (dict(tolerance=float('inf')), 'tolerance'), (dict(tolerance=float('nan')), 'tolerance'),
                     (dict(tolerance='0.1'), 'tolerance')):
        with pytest.raises(DpfError, match='multiview_loss: %s must be' % what):
            ops.multiview_loss(*args, target_type='depth', **kw)
    with pytest.raises(DpfError, match='GPU tensors'):
        ops.multiview_loss(*args, target_type='depth', reduce='min', visibility='zbuffer')


def test_c_abi_is_declared_with_the_plain_lead():
    from dualpixelface_amd._lib import parse_header
    protos = parse_header()
    for name in ('dpf_multiview_occ_workspace_bytes', 'dpf_multiview_zbuffer', 'dpf_multiview_occ_forward', 'dpf_multiview_occ_backward'):
        assert name in protos, name
    plain = [a for _, a in protos['dpf_multiview_forward'][1]]
    lead = plain[:plain.index('ws')]
    mode = ['reduce', 'visibility', 'cell', 'tolerance']
    fwd, bwd = [a for _, a in protos['dpf_multiview_occ_forward'][1]], [a for _, a in protos['dpf_multiview_occ_backward'][1]]
    assert fwd[:len(lead) + 4] == lead + mode and bwd[:len(lead) + 4] == lead + mode
    assert fwd[len(lead) + 4:] == ['ws', 'ws_bytes', 'luma', 'zbuffer', 'selected', 'stats', 'out', 'warped_out', 'counted_out', 'sample_xy_out',
                                   'visible_out', 'stream']
    assert bwd[len(lead) + 4:] == ['luma', 'zbuffer', 'selected', 'stats', 'gout', 'dpred', 'stream']
    assert [a for _, a in protos['dpf_multiview_occ_workspace_bytes'][1]] == ['B', 'n', 'S', 'H', 'W', 'reduce']


# ---- the occluder scene
def test_the_occluder_scene_hides_a_wide_band_from_one_view_that_the_other_sees():
    c = oc.occluder_case()
    cl = c['closed']
    assert c['pred'].shape == (1, 1, 48, 64) and c['src_rgb'].shape[1] == 2
    occ, hid0, hid1 = cl['on_occluder'], ~cl['visible'][0], ~cl['visible'][1]
    assert 0.3 * occ.size < occ.sum() < 0.7 * occ.size and not (hid0 & occ).any()
    width = hid0.sum(axis=1)
    print('occluder scene: %d of %d pixels on the rectangle, %d hidden from view 0 (band %d to %d pixels wide), %d from view 1, %d from both'
          % (occ.sum(), occ.size, hid0.sum(), width.min(), width.max(), hid1.sum(), (hid0 & hid1).sum()))
    assert width.min() >= 6                                          # the hidden band is at least 6 target pixels wide in every row
    assert (hid0 & ~hid1).sum() >= 0.9 * hid0.sum()                  # most of what view 0 cannot see view 1 can
    # the depth map is the nearer hit: the rectangle at OCCLUDER_Z, the plane at about 800
    z = c['z'][0, 0]
    assert np.abs(z[occ] - 400.0).max() < 3.0 and z[~occ].min() > 700.0


@pytest.mark.parametrize('cell', [1, 2])
def test_restated_visibility_equals_the_closed_form_outside_the_boundary_band(cell):
    """At the true depth the restated visible map (the z-buffer of the prediction, fp32) equals the closed-form visibility (segment
    against rectangle, fp64) at every warpable pixel farther than 2 cell + 2 source pixels from the outline of the rectangle in that
    view.  The band holds at most 40 % of the truly hidden pixels, so at least 60 % of them are tested: a condition of the rig."""
    c = oc.occluder_case()
    cl = c['closed']
    r = oc.forward(c, visibility='zbuffer', cell=cell, tolerance=0.01)
    for v in range(2):
        warpable = r['warpable'][0][v][0]
        got = r['visible'][0, 0, v] > 0
        want = cl['visible'][v] & warpable
        band = cl['edge'][v] <= 2 * cell + 2
        hidden = ~cl['visible'][v] & warpable
        share = (hidden & band).sum() / max(1, hidden.sum())
        print('cell %d view %d: %d warpable, %d truly hidden of which %.0f %% in the band, %d mismatches in the band, %d outside'
              % (cell, v, warpable.sum(), hidden.sum(), 100 * share, ((got != want) & band).sum(), ((got != want) & ~band).sum()))
        assert share <= 0.4
        assert np.array_equal(got[~band], want[~band])
    assert (~cl['visible'][0]).sum() > 500 and (r['visible'][0, 0, 0] == 0).sum() > 300


def test_visibility_brings_the_loss_at_the_true_depth_down_to_the_closed_form_floor():
    """Restated, not the kernels (tests/test_gpu_multiview_occlusion.py repeats the inequalities on the device): the floor is the fp64
    loss under closed-form visibility."""
    c = oc.occluder_case()
    floor, _ = oc.closed_form_loss(c)
    plain, vis, mn = oc.forward(c)['loss'], oc.forward(c, visibility='zbuffer')['loss'], oc.forward(c, reduce='min')['loss']
    print('occluder scene at the true depth: floor %.6e, mean / none %.6e, zbuffer %.6e, min %.6e' % (floor, plain, vis, mn))
    assert floor > 0 and plain > floor and vis <= 2 * floor and mn < plain
    # with nothing in front the z-buffer hides nothing: the plane scene counts what it counted
    p = mc.plane_case(H=24, W=40, views=2, seed=3)
    assert np.array_equal(oc.forward(p, visibility='zbuffer')['counted'], mc.forward(p)['counted'])


# ---- the oracle
@pytest.mark.parametrize('S', [1, 2])
def test_fp64_autograd_gradient_agrees_with_central_differences(S):
    """The fp64 torch restatement under 'min' + 'zbuffer' against central differences of its own loss, every element of the 7 x 9 case
    (and of the same shape with two views, where the minimum has something to choose), at h = 1e-5 of a depth near 10.  With the discrete
    decisions frozen the loss is smooth.  tests/test_multiview_host.py holds no such check for the plain loss, so the bar is that of the
    two-view sibling (tests/test_photometric_host.py: 6e-8 at a largest gradient of 0.038): 1.6e-6 of the largest gradient."""
    args, occ = oc.CASES['tiny-7x9']
    c = mc.make_case(**dict(args, S=S))
    kw = dict(oc.MODES['min-zbuffer'], **occ)
    ref = oc.forward(c, **kw)
    _, g = oc.loss_and_grad(c, ref, torch.float64)
    p0 = torch.tensor(c['pred'].astype(np.float64))
    f = lambda p: float(oc.torch_loss(p, ref, c, torch.float64))                                    # noqa: E731
    h, worst = 1e-5, 0.0
    for i in range(p0.numel()):
        e = torch.zeros(p0.numel(), dtype=torch.float64)
        e[i] = h
        fd = (f(p0 + e.view_as(p0)) - f(p0 - e.view_as(p0))) / (2 * h)
        worst = max(worst, abs(fd - g.ravel()[i]))
    bar = 1.6e-6 * np.abs(g).max()
    print('central differences, S = %d: worst %.3e against the bar %.3e, largest gradient %.3e' % (S, worst, bar, np.abs(g).max()))
    assert ref['count_min'][0] > 0 and np.abs(g).max() > 0 and worst <= bar


@pytest.mark.parametrize('name', sorted(oc.CASES))
@pytest.mark.parametrize('mode', sorted(oc.MODES))
def test_every_case_counts_pixels_in_every_mode_and_near_ties_are_rare(name, mode):
    """What the GPU tests lean on: under every mode a case counts pixels, under the z-buffer fewer than the plain loss but (the tiny case
    aside, where nothing collides) between a third and two thirds of them, near-ties of the selection are at most 1 % of the counted
    pixels, and the fp32 autograd gradient is close to the fp64 one."""
    ref = oc.case(name, mode)
    r32, c = ref['r32'], ref['case']
    plain = mc.forward(c)['counted']
    cnt = r32['counted']
    assert 0 < cnt.sum() <= plain.sum() and not (cnt & ~plain).any()
    if mode == 'min':
        assert np.array_equal(cnt, plain) and r32['zbuffer'] is None
    elif name != 'tiny-7x9':
        assert plain.sum() / 3 <= cnt.sum() <= 2 * plain.sum() / 3, (cnt.sum(), plain.sum())
    some = (r32['selected'] != oc.NONE)
    assert np.array_equal(some, cnt.max(axis=2) > 0) and sum(r32['count_min']) == some.sum()
    print('%s %s: counted %d of %d plain, near-ties %d of %d' % (name, mode, cnt.sum(), plain.sum(), ref['ties'].sum(), some.sum()))
    assert ref['ties'].sum() <= 0.01 * some.sum()
    assert np.isfinite(ref['grad64']).all() and np.abs(ref['grad64']).max() > 0
    assert np.abs(ref['grad32'] - ref['grad64']).max() <= 1e-3 * np.abs(ref['grad64']).max()
    assert abs(r32['loss'] - ref['loss64']) <= 1e-5 * abs(ref['loss64'])
    if name == 'one-behind-33x40':
        assert not cnt[:, :, 2].any() and not (r32['selected'] == 2).any()
