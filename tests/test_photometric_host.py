"""The photometric and smoothness losses on the host (no GPU): photometric.settings, the loss bank entries, label_free, the hook's
refusals, the plugin's label-free branch on a stub network, the shipped configs, the C ABI, and the proof of the oracle
tests/test_gpu_photometric.py measures the kernels against (tests/photometric_cpu.py)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import photometric_cpu as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = ((0.0, -2.0), 0.85, 1e-3, 10.0)


class _Opt(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _settings(block):
    from dualpixelface_amd import photometric
    return photometric.settings(_Opt(model=_Opt(photometric=block)))


# ---- settings
def test_settings_defaults_and_overrides():
    from dualpixelface_amd import photometric
    assert tuple(photometric.settings(_Opt())) == DEFAULTS and tuple(photometric.settings(_Opt(model=_Opt()))) == DEFAULTS
    assert tuple(_settings(None)) == DEFAULTS and tuple(_settings({})) == DEFAULTS and tuple(photometric.DEFAULTS) == DEFAULTS
    assert photometric.Settings._fields == ('shift', 'alpha', 'charbonnier_eps', 'smooth_gamma')
    s = _settings({'shift': [1, 0], 'alpha': 1, 'smooth_gamma': 0})
    assert s.shift == (1.0, 0.0) and s.alpha == 1.0 and isinstance(s.alpha, float) and s.smooth_gamma == 0.0 and s.charbonnier_eps == 1e-3
    s = _settings(_Opt(alpha=0.5, charbonnier_eps=0.01))              # an attribute block, as config.Option makes one
    assert s.alpha == 0.5 and s.charbonnier_eps == 0.01 and s.shift == (0.0, -2.0)


@pytest.mark.parametrize('key,value', [
    ('shift', [0, 0]), ('shift', [0.0, 0.0]), ('shift', [1.0]), ('shift', [1, 2, 3]), ('shift', 2.0), ('shift', None), ('shift', [0, float('nan')]),
    ('shift', [float('inf'), 0]), ('shift', [True, 0]), ('shift', ['0', '-2']),
    ('alpha', -0.1), ('alpha', 1.5), ('alpha', None), ('alpha', '0.85'), ('alpha', float('nan')), ('alpha', True),
    ('charbonnier_eps', 0), ('charbonnier_eps', -1e-3), ('charbonnier_eps', None), ('charbonnier_eps', float('inf')), ('charbonnier_eps', '1e-3'),
    ('charbonnier_eps', float('nan')), ('charbonnier_eps', True),
    ('smooth_gamma', -1), ('smooth_gamma', None), ('smooth_gamma', float('inf')), ('smooth_gamma', float('nan')), ('smooth_gamma', '10'),
    ('smooth_gamma', False),
])
def test_a_malformed_value_is_refused_by_key(key, value):
    with pytest.raises(ValueError, match=r'photometric\.%s' % key):
        _settings({key: value})


def test_a_non_block_is_refused():
    for bad in (True, 3, 'on', [1]):
        with pytest.raises(ValueError, match='photometric'):
            _settings(bad)


# ---- the loss bank
def _sel(loss_type, lambdas=None, **over):
    from dualpixelface_amd import load_option, losses
    return losses.loss_selector(load_option('train_faceDP_dpnet', loss_type=loss_type, lambdas=lambdas or [1.0] * len(loss_type), **over))


def test_bank_resolves_both_names_and_label_free_holds_for_their_subsets_only():
    from dualpixelface_amd import losses
    assert losses._BANK['photometric'] is losses.PHOTOMETRICLoss and losses._BANK['smoothness'] is losses.SMOOTHNESSLoss
    for names in (['photometric'], ['smoothness'], ['photometric', 'smoothness'], ['smoothness', 'photometric']):
        sel = _sel(names)
        assert sel.loss_name == names and sel.label_free()
        assert all(tuple(f.settings) == DEFAULTS for f in sel.loss_func)
        assert sel.loss_func[0].head_weights(1) == [1.0] and sel.loss_func[0].head_weights(5)[1] == 0.75294
    for names in (['smoothL1'], ['smoothL1', 'photometric'], ['photometric', 'smoothness', 'normal_geo'], ['normal_geo', 'smoothness'], ['cosine']):
        assert not _sel(names).label_free(), names
    # the block reaches both entries
    sel = _sel(['photometric', 'smoothness'], photometric={'shift': [2.0, 0.0], 'smooth_gamma': 3.0})
    assert sel.loss_func[0].settings.shift == (2.0, 0.0) and sel.loss_func[1].settings.smooth_gamma == 3.0


def test_folded_stays_refused_next_to_them():
    with pytest.raises(NotImplementedError, match='wrong loss type : folded'):
        _sel(['photometric', 'smoothness', 'folded'])
    from dualpixelface_amd import load_option, losses
    opt = load_option('train_faceDP_dpnet', loss_type=['smoothL1', 'photometric'], lambdas=[1.0, 1.0])
    opt.dataset.dp_conversion = 'least_square'
    with pytest.raises(NotImplementedError, match='least_square'):
        losses.loss_selector(opt)


def test_the_hook_names_a_missing_view_and_reaches_the_operator():
    from dualpixelface_amd._lib import DpfError
    B, H, W = 1, 4, 6
    full = {'left': torch.zeros(B, 3, H, W), 'right': torch.zeros(B, 3, H, W)}
    preds = {'pred_depth': torch.ones(B, 1, H, W)}
    for name in ('photometric', 'smoothness'):
        sel = _sel([name])
        for key in ('left', 'right'):
            with pytest.raises(NotImplementedError, match=r"%s.*batch\['%s'\]" % (name, key)):
                sel.forward(preds, {k: v for k, v in full.items() if k != key})
        with pytest.raises(DpfError, match='GPU tensors'):           # everything there: the operator refuses the CPU tensors
            sel.forward(preds, full)
    # a depth model needs the conversion: from the batch, else from the fit, which names what it needs
    sel = _sel(['photometric'])
    with pytest.raises(NotImplementedError, match='idepth'):
        sel.forward(preds, full, target_type='depth')
    with pytest.raises(DpfError, match='GPU tensors'):
        sel.forward(preds, dict(full, abvalue=torch.ones(B, 2)), target_type='depth')


def test_the_hook_swaps_the_views_under_flip_lr(monkeypatch):
    from dualpixelface_amd import load_option, losses, ops
    seen = []
    monkeypatch.setattr(ops, 'photometric_loss', lambda pd, ref, tgt, **k: seen.append(('p', ref, tgt, k)) or torch.zeros(()))
    monkeypatch.setattr(ops, 'smoothness_loss', lambda pd, guide, **k: seen.append(('s', guide, None, k)) or torch.zeros(()))
    batch = {'left': torch.zeros(1, 3, 4, 6), 'right': torch.ones(1, 3, 4, 6)}
    preds = {'pred_depth': torch.ones(1, 1, 4, 6)}
    for flip in (False, True):
        opt = load_option('train_faceDP_dpnet', loss_type=['photometric', 'smoothness'], lambdas=[1.0, 0.1])
        opt.dataset.flip_lr = flip
        del seen[:]
        out = losses.loss_selector(opt).forward(preds, batch)
        assert set(out) == {'photometric_loss', 'smoothness_loss', 'final_loss'}
        ref, tgt = (batch['right'], batch['left']) if flip else (batch['left'], batch['right'])
        assert seen[0][0] == 'p' and seen[0][1] is ref and seen[0][2] is tgt and seen[1][0] == 's' and seen[1][1] is ref
        assert seen[0][3]['shift'] == (0.0, -2.0) and seen[0][3]['alpha'] == 0.85 and seen[0][3]['eps'] == 1e-3 and seen[0][3]['ab'] is None
        assert seen[1][3]['gamma'] == 10.0 and seen[1][3]['eps'] == 1e-3 and seen[0][3]['mask'] is None


def test_operators_refuse_cpu_tensors_and_malformed_operands():
    from dualpixelface_amd import ops
    from dualpixelface_amd._lib import DpfError
    pred, img = torch.zeros(1, 2, 8, 8), torch.zeros(1, 3, 8, 8)
    with pytest.raises(DpfError, match='GPU tensors'):
        ops.photometric_loss(pred, img, img, head_weights=(1.0, 0.5))
    with pytest.raises(DpfError, match='GPU tensors'):
        ops.smoothness_loss(pred, img, head_weights=(1.0, 0.5))
    with pytest.raises(DpfError, match='target_type'):
        ops.photometric_loss(pred, img, img, target_type='inverse')
    with pytest.raises(DpfError, match="'depth' needs ab"):
        ops.photometric_loss(pred, img, img, target_type='depth')
    import inspect
    assert str(inspect.signature(ops.photometric_loss)) == (
        "(pred, ref_rgb, tgt_rgb, ab=None, mask=None, head_weights=(1.0,), target_type='disp', shift=(0.0, -2.0), alpha=0.85, eps=0.001, "
        "return_warped=False)")
    assert str(inspect.signature(ops.smoothness_loss)) == "(pred, guide_rgb, mask=None, head_weights=(1.0,), gamma=10.0, eps=0.001)"


# ---- the plugin
def test_forward_in_training_reaches_the_loss_hook_for_a_batch_of_the_two_views(monkeypatch):
    from dualpixelface_amd import load_option
    from dualpixelface_amd.plugin import DPNET
    batch = {'left': torch.zeros(1, 3, 4, 6), 'right': torch.zeros(1, 3, 4, 6)}
    pred = torch.ones(1, 5, 4, 6)

    def build(loss_type, lambdas):
        model = DPNET(load_option('train_faceDP_dpnet', loss_type=loss_type, lambdas=lambdas))
        model.network = lambda b: {'pred_depth': pred, '_taps': None}                # the stub network
        calls = []
        monkeypatch.setattr(model.loss_model, 'forward',
                            lambda results, b, target_type='disp': calls.append((results['pred_depth'], b, target_type)) or {'final_loss': 1.0})
        return model, calls

    model, calls = build(['photometric', 'smoothness'], [1.0, 0.1])
    model.train()
    out = model._forward(batch)
    assert len(calls) == 1 and calls[0][0] is pred and calls[0][1] is batch and calls[0][2] == 'disp' and out['final_loss'] == 1.0
    model.eval()
    assert 'final_loss' not in model._forward(batch) and len(calls) == 1                # evaluation runs no loss hook
    # a loss that reads a label keeps the old rule: no label, no hook
    model, calls = build(['smoothL1', 'photometric'], [1.0, 1.0])
    model.train()
    assert 'final_loss' not in model._forward(batch) and not calls
    model._forward(dict(batch, disp=torch.zeros(1, 4, 6)))
    assert len(calls) == 1


# ---- configs
def test_configs_are_their_bases_with_the_losses_and_the_block_spelled_out():
    from dualpixelface_amd import load_option, photometric
    base = json.load(open(os.path.join(ROOT, 'src', 'model', 'dpnet', 'config.json')))
    ours = json.load(open(os.path.join(ROOT, 'src', 'model', 'dpnet', 'config_photometric.json')))
    block = ours.pop('photometric')
    assert block == {'shift': [0.0, -2.0], 'alpha': 0.85, 'charbonnier_eps': 1e-3, 'smooth_gamma': 10.0}
    assert set(block) == set(photometric.Settings._fields)
    assert ours.pop('loss_type') == ['photometric', 'smoothness'] and ours.pop('lambdas') == [1.0, 0.1]
    assert base.pop('loss_type') == ['smoothL1'] and base.pop('lambdas') == [1.0] and ours == base
    top_base = json.load(open(os.path.join(ROOT, 'config_', 'train_faceDP_dpnet.json')))
    top = json.load(open(os.path.join(ROOT, 'config_', 'train_faceDP_dpnet_photometric.json')))
    assert top.pop('model_config') == 'config_photometric' and top_base.pop('model_config') == 'config'
    assert top.pop('augmentation') == ['crop_aug'] and top_base.pop('augmentation') == ['crop_aug', 'photo_aug'] and top == top_base
    opt = load_option('train_faceDP_dpnet_photometric')
    assert opt.model_name == 'dpnet' and opt.model.loss_type == ['photometric', 'smoothness'] and opt.model.lambdas == [1.0, 0.1]
    assert tuple(photometric.settings(opt)) == DEFAULTS
    # no other shipped configuration names either loss
    for name in sorted(f[:-5] for f in os.listdir(os.path.join(ROOT, 'config_')) if f.endswith('.json')):
        names = load_option(name).model.loss_type
        assert ('photometric' in names or 'smoothness' in names) == (name == 'train_faceDP_dpnet_photometric'), name


# ---- C ABI
def test_header_declares_the_entry_points_and_forward_and_backward_share_their_leading_arguments():
    from dualpixelface_amd import _lib
    protos = _lib.parse_header()
    for name in ('dpf_photometric_workspace_bytes', 'dpf_smoothness_workspace_bytes'):
        assert protos[name][0] is _lib._CTYPES['long long'] and [n for _, n in protos[name][1]] == ['B', 'n', 'H', 'W']
    fwd = [n for _, n in protos['dpf_photometric_forward'][1]]
    bwd = [n for _, n in protos['dpf_photometric_backward'][1]]
    assert len(fwd) == 24 and len(bwd) == 21 and fwd[:16] == bwd[:16]
    assert fwd[:16] == ['pred', 'ref_rgb', 'tgt_rgb', 'ab', 'mask', 'B', 'n', 'H', 'W', 'target_type', 'shift_x', 'shift_y', 'alpha', 'eps',
                        'norm_host', 'head_weights_host']
    assert fwd[16:] == ['ws', 'ws_bytes', 'luma', 'stats', 'out', 'warped_out', 'counted_out', 'stream']
    assert bwd[16:] == ['luma', 'stats', 'gout', 'dpred', 'stream']
    fwd = [n for _, n in protos['dpf_smoothness_forward'][1]]
    bwd = [n for _, n in protos['dpf_smoothness_backward'][1]]
    assert fwd[:11] == bwd[:11] == ['pred', 'guide_rgb', 'mask', 'B', 'n', 'H', 'W', 'gamma', 'eps', 'norm_host', 'head_weights_host']
    assert fwd[11:] == ['ws', 'ws_bytes', 'luma', 'stats', 'out', 'stream'] and bwd[11:] == ['luma', 'stats', 'gout', 'dpred', 'stream']
    make = open(os.path.join(ROOT, 'dualpixelface_amd', 'csrc', 'Makefile')).read()
    assert '$(OBJDIR)/photometric.o: CXXFLAGS += -ffp-contract=off' in make


def test_the_restatement_uses_the_data_paths_normalizer():
    from dualpixelface_amd.facedp import IMAGENET_MEAN, IMAGENET_STD
    assert tuple(IMAGENET_MEAN) == pc.MEAN and tuple(IMAGENET_STD) == pc.STD


# ---- the oracle
def test_fp64_autograd_gradient_agrees_with_finite_differences():
    """The fp64 torch restatement against central differences of its own loss on tiny-7x9, every element, at h = 1e-6.  With the discrete
    decisions held the loss is smooth.  Truncation: h^2 f''' / 6, and f''' is largest in the intensity term, (1 - alpha) |dJ/dD|^3
    1.5 / eps^2 / count <= 0.15 * 1.6^3 * 1.5e6 / 28 = 3.3e4 (|dJ/dD| <= |shift| * the luminance range 0.8), so at most 5.5e-9.
    Rounding: a window's variance is a difference of numbers near 0.25 (error 1e-16) over at least C2 = 9e-4, so a term is off by at most
    0.425 * 1.2e-13 = 5e-14, and so is their mean: 5e-14 / h = 5e-8.  Both are covered by 6e-8; h = 1e-6 is where the two bounds meet
    ((3 * 5e-14 / 3.3e4)^(1/3) = 1.7e-6).  The largest gradient is 0.038, so the bar is 1.6e-6 of it."""
    r = pc.case('tiny-7x9')
    c = r['case']
    p0 = torch.tensor(c['pred'].astype(np.float64))

    def f(p):
        return float(pc.torch_loss(p, r['r32'], c['ref_rgb'], c['tgt_rgb'], c['ab'], c['head_weights'], c['target_type'], c['shift'],
                                   c['alpha'], c['eps'], torch.float64))
    g, h = r['grad64'], 1e-6
    assert g.shape == c['pred'].shape and np.abs(g).max() > 0.01 and r['r32']['count'] == [28.0]
    worst = 0.0
    for i in range(p0.numel()):
        e = torch.zeros(p0.numel(), dtype=torch.float64)
        e[i] = h
        fd = (f(p0 + e.view_as(p0)) - f(p0 - e.view_as(p0))) / (2 * h)
        worst = max(worst, abs(fd - g.ravel()[i]))
    print('finite differences: worst %.3e against the bar 6e-8, largest gradient %.3e' % (worst, np.abs(g).max()))
    assert worst <= 6e-8, (worst, np.abs(g).max())


def test_the_finite_difference_scene_keeps_its_samples_off_the_grid():
    """tiny-7x9: along the shifted axis the fractional part of every sample coordinate lies in [0.1, 0.9], so no sample sits on the kink of
    the bilinear interpolant and a step of 1e-6 crosses none; the other axis is not shifted at all."""
    c = pc.case('tiny-7x9')['case']
    assert c['shift'] == (0.0, -2.0)
    ys = np.arange(7, dtype=np.float64)[None, None, :, None]
    t = ys + c['shift'][1] * c['pred'].astype(np.float64)
    frac = t - np.floor(t)
    assert frac.min() >= 0.1 and frac.max() <= 0.9, (frac.min(), frac.max())
    assert np.abs(c['pred']).max() <= 0.6


def test_both_restatements_agree_and_each_case_counts_a_fair_share():
    """numpy and torch state the same loss: in fp64, with the same decisions, to rounding; every case counts at least a quarter of its
    pixels and fewer than all of them, fp32 and fp64 take the same decisions, and no counted pixel sits on an end of the clamp."""
    for name in pc.CASES:
        r = pc.case(name)
        counted = r['r32']['counted']
        assert 0.25 * counted.size <= counted.sum() < counted.size, (name, counted.mean())
        assert np.array_equal(counted, r['r64']['counted']), name
        assert not any(c.any() for c in r['r32']['clamped']) and not any(c.any() for c in r['r64']['clamped']), name
        assert abs(r['loss64'] - r['r64']['loss']) <= 1e-12, (name, r['loss64'], r['r64']['loss'])
        assert abs(r['loss32'] - r['r32']['loss']) <= 1.2e-7 * r['loss64'], (name, r['loss32'], r['r32']['loss'])
        assert np.isfinite(r['grad64']).all() and np.isfinite(r['grad32']).all() and (r['grad64'] == 0).any() and r['grad64'].any()
        s = pc.smooth_case(name)
        assert abs(s['loss64'] - s['r64']['loss']) <= 1e-12 * max(1.0, s['loss64']), (name, s['loss64'], s['r64']['loss'])
        assert np.isfinite(s['grad64']).all() and s['grad64'].any()
    bad = pc.case('multi-tile-19x70')['case']
    assert not np.isfinite(bad['pred']).all() and (bad['pred'] == 0).any() and bad['mask'] is not None
    assert pc.case('depth-type')['case']['ab'] is not None
