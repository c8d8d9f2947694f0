"""The multi-view photometric loss on the host (no GPU): multiview.settings, the loss bank entry beside the refused 'folded', label_free,
the hook's refusals, the shipped configs, the synthetic plane scene, and the proof of the oracle tests/test_gpu_multiview.py measures the
kernels against (tests/multiview_cpu.py) -- the restatement against records of the reference's own helpers
(tests/golden/multiview.npz, tests/golden/make_golden_multiview.py)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import multiview_cpu as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = (3, 0.8, 1.0, 0.1, 'center', 1e-3)


class _Opt(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _settings(block, **top):
    from dualpixelface_amd import multiview
    return multiview.settings(_Opt(model=_Opt(multiview=block, **top)))


# ---- settings
def test_settings_defaults_overrides_and_top_level_fallbacks():
    from dualpixelface_amd import multiview
    assert tuple(multiview.settings(_Opt())) == DEFAULTS and tuple(multiview.settings(_Opt(model=_Opt()))) == DEFAULTS
    assert tuple(_settings(None)) == DEFAULTS and tuple(_settings({})) == DEFAULTS and tuple(multiview.DEFAULTS) == DEFAULTS
    assert multiview.Settings._fields == ('select_view', 'weight_ssim', 'alpha', 'scale', 'image', 'min_depth')
    s = _settings({'select_view': 8, 'weight_ssim': 1, 'alpha': -2, 'scale': 2, 'min_depth': 0.5})
    assert tuple(s) == (8, 1.0, -2.0, 2.0, 'center', 0.5) and isinstance(s.weight_ssim, float) and isinstance(s.select_view, int)
    s = _settings(_Opt(alpha=0, scale=0.01))                          # an attribute block, as config.Option makes one
    assert s.alpha == 0.0 and s.scale == 0.01 and s.select_view == 3
    # config_multi.json's own top-level keys are read where the block has none, and the block wins
    s = _settings(None, select_view=2, weight_ssim=0.5, alpha=2.0, scale=0.3, min_depth=7.0, image='left')
    assert tuple(s) == (2, 0.5, 2.0, 0.3, 'center', 1e-3)            # (min_depth and image have no top-level fallback)
    s = _settings({'select_view': 4, 'alpha': 0.0}, select_view=2, weight_ssim=0.5, alpha=2.0)
    assert s.select_view == 4 and s.alpha == 0.0 and s.weight_ssim == 0.5


@pytest.mark.parametrize('key,value', [
    ('select_view', 0), ('select_view', 9), ('select_view', 2.0), ('select_view', True), ('select_view', None), ('select_view', '3'),
    ('weight_ssim', -0.1), ('weight_ssim', 1.5), ('weight_ssim', None), ('weight_ssim', '0.8'), ('weight_ssim', float('nan')), ('weight_ssim', True),
    ('alpha', float('inf')), ('alpha', -float('inf')), ('alpha', float('nan')), ('alpha', None), ('alpha', '1'), ('alpha', True),
    ('scale', 0), ('scale', -0.1), ('scale', float('inf')), ('scale', None), ('scale', '0.1'),
    ('image', 'left'), ('image', 'right'), ('image', 'centre'), ('image', None), ('image', 3),
    ('min_depth', 0), ('min_depth', -1), ('min_depth', float('nan')), ('min_depth', None),
])
def test_a_malformed_value_is_refused_by_key(key, value):
    with pytest.raises(ValueError, match=r'multiview\.%s' % key):
        _settings({key: value})


def test_a_malformed_top_level_fallback_is_refused_and_a_non_block_too():
    with pytest.raises(ValueError, match=r'multiview\.select_view'):
        _settings(None, select_view=12)
    with pytest.raises(ValueError, match=r'multiview\.image.*"left" and "right" are not built'):
        _settings({'image': 'left'})
    for bad in (True, 3, 'on', [1]):
        with pytest.raises(ValueError, match='multiview'):
            _settings(bad)


# ---- the loss bank
def _sel(loss_type, lambdas=None, config='train_faceDP_dpnet', **over):
    from dualpixelface_amd import load_option, losses
    return losses.loss_selector(load_option(config, loss_type=loss_type, lambdas=lambdas or [1.0] * len(loss_type), **over))


def test_bank_resolves_multiview_and_folded_stays_refused_beside_it():
    from dualpixelface_amd import losses
    assert losses._BANK['multiview'] is losses.MULTIVIEWLoss and 'folded' not in losses._BANK and 'multiview' in losses.LABEL_FREE
    sel = _sel(['multiview'])
    assert sel.loss_name == ['multiview'] and tuple(sel.loss_func[0].settings) == DEFAULTS
    assert sel.loss_func[0].head_weights(1) == [1.0] and sel.loss_func[0].head_weights(5)[1] == 0.75294
    with pytest.raises(NotImplementedError, match='wrong loss type : folded'):
        _sel(['multiview', 'folded'])
    with pytest.raises(NotImplementedError, match='wrong loss type : folded'):
        _sel(['folded'])
    sel = _sel(['multiview'], multiview={'select_view': 2, 'alpha': 0.0})
    assert sel.loss_func[0].settings.select_view == 2 and sel.loss_func[0].settings.alpha == 0.0


def test_label_free_holds_with_multiview_and_no_label_reading_loss():
    for names in (['multiview'], ['multiview', 'smoothness'], ['photometric', 'multiview', 'smoothness']):
        assert _sel(names).label_free(), names
    for names in (['multiview', 'smoothL1'], ['multiview', 'normal_geo'], ['cosine', 'multiview', 'smoothness']):
        assert not _sel(names).label_free(), names
    # it reads no label, so it refuses no dp_conversion
    from dualpixelface_amd import load_option, losses
    opt = load_option('train_faceDP_dpnet', loss_type=['multiview'], lambdas=[1.0])
    opt.dataset.dp_conversion = 'least_square'
    assert losses.loss_selector(opt).label_free()


def test_every_model_family_takes_the_entry():
    for config in ('train_faceDP', 'train_faceDP_dpnet', 'train_faceDP_psmnet', 'train_faceDP_nnet', 'train_faceDP_stereonet'):
        assert _sel(['multiview', 'smoothness'], [1.0, 0.1], config=config).loss_name == ['multiview', 'smoothness']


def _batch(B=1, H=4, W=6, S=3, Hs=5, Ws=7):
    return {'center': torch.zeros(B, 3, H, W), 'centers': torch.zeros(B, 3 * S, Hs, Ws), 'K': torch.eye(3).repeat(B, 1, 1),
            'P': torch.eye(4).repeat(B, 1, 1), 'Ks': torch.eye(3).repeat(B, S, 1, 1), 'Ps': torch.eye(4).repeat(B, S, 1, 1)}


def test_the_hook_names_every_missing_key_and_reaches_the_operator():
    from dualpixelface_amd._lib import DpfError
    full = _batch()
    preds = {'pred_depth': torch.ones(1, 1, 4, 6)}
    sel = _sel(['multiview'])
    for key in ('center', 'centers', 'K', 'P', 'Ks', 'Ps'):
        with pytest.raises(NotImplementedError, match=r"multiview.*batch\['%s'\]" % key):
            sel.forward(preds, {k: v for k, v in full.items() if k != key}, target_type='depth')
    with pytest.raises(NotImplementedError, match=r"batch\['K'\] and batch\['Ps'\]"):
        sel.forward(preds, {k: v for k, v in full.items() if k not in ('K', 'Ps')}, target_type='depth')
    with pytest.raises(DpfError, match='GPU tensors'):                # everything there: the operator refuses the CPU tensors
        sel.forward(preds, full, target_type='depth')
    with pytest.raises(DpfError, match='GPU tensors'):
        sel.forward(preds, full, target_type='idepth')
    # a disparity model needs the conversion: from the batch, else from the fit, which names what it needs
    with pytest.raises(NotImplementedError, match='idepth'):
        sel.forward(preds, full, target_type='disp')
    with pytest.raises(DpfError, match='GPU tensors'):
        sel.forward(preds, dict(full, abvalue=torch.ones(1, 2)), target_type='disp')


def test_the_hook_refuses_a_batch_with_fewer_views_than_select_view():
    preds = {'pred_depth': torch.ones(1, 1, 4, 6)}
    with pytest.raises(NotImplementedError, match='select_view = 3.*carries 2 views'):
        _sel(['multiview']).forward(preds, _batch(S=2), target_type='depth')
    short = _batch(S=3)
    short['Ps'] = short['Ps'][:, :1]
    with pytest.raises(NotImplementedError, match='select_view = 3.*carries 1 views'):
        _sel(['multiview']).forward(preds, short, target_type='depth')


def test_the_hook_hands_the_first_select_view_views_and_the_settings_on(monkeypatch):
    from dualpixelface_amd import ops
    seen = []
    monkeypatch.setattr(ops, 'multiview_loss', lambda pd, tgt, src, K, P, Ks, Ps, **k: seen.append((tgt, src, K, P, Ks, Ps, k)) or torch.zeros(()))
    batch = _batch(B=2, S=4)
    batch['centers'] = torch.arange(2 * 12 * 5 * 7, dtype=torch.float32).view(2, 12, 5, 7)
    batch['Ks'] = batch['Ks'].double()                                # the loader's host arrays may arrive in double precision
    batch['conf'] = torch.ones(2, 4, 6)                               # not read
    preds = {'pred_depth': torch.ones(2, 5, 4, 6)}
    out = _sel(['multiview'], multiview={'select_view': 2, 'alpha': 0.0}).forward(preds, batch, target_type='depth')
    assert set(out) == {'multiview_loss', 'final_loss'}
    tgt, src, K, P, Ks, Ps, k = seen[0]
    assert tgt is batch['center'] and tuple(src.shape) == (2, 2, 3, 5, 7) and torch.equal(src.reshape(2, 6, 5, 7), batch['centers'][:, :6])
    assert tuple(Ks.shape) == (2, 2, 3, 3) and Ks.dtype == torch.float32 and tuple(Ps.shape) == (2, 2, 4, 4) and K is batch['K']
    assert k['alpha'] == 0.0 and k['weight_ssim'] == 0.8 and k['scale'] == 0.1 and k['min_depth'] == 1e-3 and k['ab'] is None
    assert k['mask'] is None and k['target_type'] == 'depth' and k['head_weights'][:2] == [1.0, 0.75294] and 'conf' not in k
    out = _sel(['multiview']).forward(preds, dict(batch, abvalue=torch.ones(2, 2)), target_type='disp')
    assert seen[1][6]['ab'] is not None and 'abvalue' in out


def test_operator_refuses_cpu_tensors_and_malformed_operands():
    from dualpixelface_amd import ops
    from dualpixelface_amd._lib import DpfError
    b = _batch()
    pred = torch.zeros(1, 2, 4, 6)
    src = b['centers'].view(1, 3, 3, 5, 7)
    args = (pred, b['center'], src, b['K'], b['P'], b['Ks'], b['Ps'])
    with pytest.raises(DpfError, match='GPU tensors'):
        ops.multiview_loss(*args, head_weights=(1.0, 0.5), target_type='depth')
    with pytest.raises(DpfError, match='target_type'):
        ops.multiview_loss(*args, target_type='inverse')
    with pytest.raises(DpfError, match="'disp' needs ab"):
        ops.multiview_loss(*args, target_type='disp')
    with pytest.raises(DpfError, match='GPU tensors'):
        ops.multiview_rig(b['K'], b['P'], b['Ks'], b['Ps'])


# ---- configs
def test_the_shipped_configs_load_and_say_what_the_issue_sets():
    from dualpixelface_amd import load_option, losses, multiview
    opt = load_option('train_faceDP_dpnet_multiview')
    assert opt.model_name == 'dpnet' and opt.model_config == 'config_multiview' and opt.use_multi and opt.use_center_img
    assert opt.multi_view.use_center_img and opt.augmentation == ['crop_aug'] and not hasattr(opt, 'photo_aug')
    # ('smoothness' beside it is an override away, loss_type ['multiview', 'smoothness']: tests/test_photometric_host.py pins that no
    # shipped configuration but the photometric one names that loss)
    assert opt.model.loss_type == ['multiview'] and opt.model.lambdas == [1.0]
    assert tuple(multiview.settings(opt)) == DEFAULTS
    sel = losses.loss_selector(opt)
    assert sel.label_free() and sel.loss_name == ['multiview']
    # config_multi.json stays a settings file whose keys now mean what they say
    raw = json.load(open(os.path.join(ROOT, 'src', 'model', 'dpnet', 'config_multi.json')))
    assert 'multiview' not in raw and raw['select_view'] == 3
    s = multiview.settings(_Opt(model=_Opt(**raw)))
    assert (s.select_view, s.weight_ssim, s.alpha, s.scale) == (raw['select_view'], raw['weight_ssim'], raw['alpha'], raw['scale'])


def test_c_abi_is_declared_and_bound():
    from dualpixelface_amd._lib import parse_header
    protos = parse_header()
    for name in ('dpf_multiview_workspace_bytes', 'dpf_multiview_rig', 'dpf_multiview_forward', 'dpf_multiview_backward'):
        assert name in protos, name
    fwd, bwd = [a for _, a in protos['dpf_multiview_forward'][1]], [a for _, a in protos['dpf_multiview_backward'][1]]
    lead = fwd[:fwd.index('ws')]
    assert bwd[:len(lead)] == lead and fwd[-4:] == ['warped_out', 'counted_out', 'sample_xy_out', 'stream']
    assert bwd[len(lead):] == ['luma', 'stats', 'gout', 'dpred', 'stream']


# ---- the restatement against the reference's own helpers
@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'multiview.npz'))


def test_sample_coordinates_agree_with_the_reference_cam2pixel(golden):
    """The fp32 restatement (rig in fp64 rounded to fp32, then q = z m + t in fp32) against the recorded
    cam2pixel(pixel2cam(grid, K, depth), ...) of the reference, which inverts, multiplies and normalises in fp32 along another route.
    Measured when the fixture was made: max |du| 5.7e-6, max |dv| 2.9e-6 pixels over both views (the fp64 restatement is as far from the
    record, 4.3e-6 / 2.1e-6: most of it is the reference's own rounding).  Allowed: 4 x the larger = 2.3e-5 pixels.  Which points fall
    outside the 16 x 26 frame agrees exactly (41 of 240 in the second view, none in the first)."""
    g = golden
    rg = mc.rig(g['K'], g['P'], g['Ks'], g['Ps'])
    Hs, Ws = [int(v) for v in g['source_size']]
    assert np.abs(rg - mc.rig_plain(g['K'], g['P'], g['Ks'], g['Ps'])).max() <= 2.0 ** -23 * np.abs(rg).max()
    worst = 0.0
    for v in range(2):
        z = g['depth'].astype(np.float32)
        ok, _, (u, w), _, _ = mc.warp(z, np.ones(z.shape, bool), rg[:, v], np.zeros((1, Hs, Ws), np.float32), np.float32)
        outside = g['outside'][:, v]
        assert np.array_equal(ok, ~outside), (v, int(ok.sum()), int((~outside).sum()))
        du, dv = np.abs(u - g['coords'][:, v, 0])[ok].max(), np.abs(w - g['coords'][:, v, 1])[ok].max()
        print('view %d: %d points inside, max |du| %.3e, max |dv| %.3e pixels' % (v, ok.sum(), du, dv))
        worst = max(worst, du, dv)
    assert g['outside'][:, 1].sum() == 41 and not g['outside'][:, 0].any()
    assert worst <= 2.3e-5


def test_ssim_term_agrees_with_the_reference_ssim(golden):
    """The window of dpf_window.h (sums of the values less the centre's) against the reference's AvgPool2d form, which subtracts squared
    means of un-centred values in fp32.  Measured: max deviation 1.03e-5 of a term of up to 0.089 (the fp64 restatement deviates by the
    same 1.02e-5: it is the reference's cancellation).  Allowed: 4 x = 4.1e-5."""
    g = golden
    term, raw = mc.ssim_term(g['ssim_x'][:, 0], g['ssim_y'][:, 0], np.float32)
    err = np.abs(term - g['ssim_term'][:, 0]).max()
    print('SSIM term: max deviation %.3e, largest term %.3e' % (err, g['ssim_term'].max()))
    assert term.shape == (1, 10, 18) and g['ssim_term'].max() > 0.05 and err <= 4.1e-5


def test_rho_agrees_with_the_reference_charbonnier_at_the_four_alphas(golden):
    """Measured: relative deviation 7.1e-8 at alpha = -2 and alpha = 0, none at alpha = 1 and alpha = 2 (the same fp32 expressions).
    Allowed: 4 x 7.2e-8 = 2.9e-7 of the value."""
    g = golden
    assert g['alphas'].tolist() == [-2.0, 0.0, 1.0, 2.0] and g['scale'].item() == np.float32(0.1)
    for k, alpha in enumerate(g['alphas']):
        r = mc.rho(g['residual'], float(alpha), g['scale'].item(), np.float32)
        rel = (np.abs(r - g['rho'][k]) / np.maximum(np.abs(g['rho'][k]), 1e-30)).max()
        print('alpha %+.0f: max relative deviation %.3e, largest value %.4g' % (alpha, rel, g['rho'][k].max()))
        assert r.dtype == np.float32 and g['rho'][k].max() > 1.0 and rel <= 2.9e-7
    # the general form at alpha = 1 is the sqrt path's expression
    s = (g['residual'].astype(np.float64) / 0.1) ** 2
    assert np.allclose(mc.rho(g['residual'].astype(np.float64), 1.0, 0.1), np.sqrt(s + 1) - 1, rtol=1e-6, atol=0)


# ---- the plane scene and the cases
def test_the_plane_scene_warped_by_its_true_depth_reproduces_the_target_luminance():
    """In fp64 the warped luminance equals the target's up to the bilinear interpolation of the neighbour's raster: for a sinusoid of
    amplitude A whose phase advances by at most phi per pixel along each axis the error is at most A (phi_x^2 + phi_y^2) / 8; a pixel's
    footprint on the plane is at most 1.1 z_max / f units (the plane's tilt and the neighbour's turn stay below 10 %)."""
    from dualpixelface_amd import synthetic_multiview as scene
    c = mc.plane_case(H=24, W=40, views=2, seed=3)
    r = mc.forward(c, np.float64)
    foot = 1.1 * float(c['z'].max()) / float(c['Ks'][0, 0, 0, 0])
    bound = sum(0.12 * float(np.dot(w, w)) * foot ** 2 / 8 for w, _ in scene.WAVES)
    cnt = r['counted'][0, 0] > 0
    err = np.abs(r['warped'][0, 0] - r['Y_tgt'][0][None])[cnt].max()
    print('plane at the true depth: %d pixels counted, max |J - I| %.3e (interpolation bound %.3e), loss %.3e' % (cnt.sum(), err, bound, r['loss']))
    assert cnt.sum() >= cnt.size // 2 and err <= bound
    off = [mc.forward(mc.plane_case(H=24, W=40, views=2, seed=3, offset=o), np.float64) for o in (0.05, -0.05)]
    assert all(o['loss'] > 10 * r['loss'] for o in off), (r['loss'], [o['loss'] for o in off])
    # the three target types mean the same depth
    for tt in ('idepth', 'disp'):
        other = mc.forward(mc.plane_case(H=24, W=40, views=2, seed=3, target_type=tt), np.float64)
        assert abs(other['loss'] - r['loss']) <= 1e-3 * r['loss'] + 1e-9 and np.array_equal(other['counted'], r['counted'])


def test_the_synthetic_batch_has_the_loaders_keys_and_consistent_labels():
    from dualpixelface_amd.synthetic_multiview import AB, SyntheticMultiview, synthetic_multiview_batch
    b = synthetic_multiview_batch(2, 16, 24, views=3, seed=5)
    assert tuple(b['center'].shape) == (2, 3, 16, 24) and tuple(b['centers'].shape) == (2, 9, 20, 30)
    assert tuple(b['Ks'].shape) == (2, 3, 3, 3) and tuple(b['Ps'].shape) == (2, 3, 4, 4) and tuple(b['P'].shape) == (2, 4, 4)
    assert all(v.dtype == torch.float32 for v in b.values()) and {'left', 'right', 'normal', 'mask', 'abvalue', 'disp', 'idepth'} <= set(b)
    assert torch.allclose(b['disp'], AB[1] / b['depth'] + AB[0], rtol=1e-5) and (b['depth'] > 0).all()
    assert not torch.equal(b['center'][0], b['center'][1])
    one = SyntheticMultiview(4, 16, 24, views=2)[1]
    assert tuple(one['centers'].shape) == (6, 20, 30) and tuple(one['Ks'].shape) == (2, 3, 3)


@pytest.mark.parametrize('name', sorted(mc.CASES))
def test_every_case_counts_pixels_and_the_restatement_keeps_its_decisions_in_fp64(name):
    """What the GPU tests lean on: every case counts pixels in some view and fewer than all, the fp64 restatement takes the same discrete
    decisions as the fp32 one (no counted pixel is left out: 0 % of the 1 % allowed), and the fp32 autograd gradient is close to the fp64
    one."""
    ref = mc.case(name)
    r32, r64 = ref['r32'], ref['r64']
    cnt = r32['counted']
    assert 0 < cnt.sum() < cnt.size and np.array_equal(cnt, r64['counted'])
    assert abs(r32['loss'] - r64['loss']) <= 1e-5 * abs(r64['loss'])
    assert np.isfinite(ref['grad64']).all() and np.abs(ref['grad64']).max() > 0
    assert np.abs(ref['grad32'] - ref['grad64']).max() <= 1e-3 * np.abs(ref['grad64']).max()
    if name == 'one-view-behind':
        assert not cnt[:, :, 1].any() and r32['views'] == [1, 1]
    if name == 'rows288-65x500':
        assert cnt.shape[0] * (-(-65 // 8)) * (-(-500 // 32)) == 288
