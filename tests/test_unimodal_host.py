"""The unimodal loss on the host (no GPU): unimodal.settings, the loss bank entry and its refusals, the private '_heads' record on a stub
network, the shipped configs, the C ABI, and the proof of the oracle tests/test_gpu_unimodal.py measures the kernels against
(tests/unimodal_cpu.py).

The last two groups ("the cases", "the oracle") exercise tests/unimodal_cpu.py alone: they prove the restatement and the drawn cases, need
nothing of the package and so pass with or without the feature.  Every other test here needs the feature."""
import inspect
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import unimodal_cpu as uc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Opt(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _settings(block):
    from dualpixelface_amd import unimodal
    return unimodal.settings(_Opt(model=_Opt(unimodal=block)))


# ---- settings
def test_settings_defaults_and_overrides():
    from dualpixelface_amd import unimodal
    assert tuple(unimodal.settings(_Opt())) == (None,) and tuple(unimodal.settings(_Opt(model=_Opt()))) == (None,)
    assert tuple(_settings(None)) == (None,) and tuple(_settings({})) == (None,) and tuple(unimodal.DEFAULTS) == (None,)
    assert unimodal.Settings._fields == ('laplace_scale',)
    assert _settings({'laplace_scale': None}).laplace_scale is None
    s = _settings({'laplace_scale': 1})
    assert s.laplace_scale == 1.0 and isinstance(s.laplace_scale, float)
    assert _settings(_Opt(laplace_scale=0.25)).laplace_scale == 0.25          # an attribute block, as config.Option makes one


@pytest.mark.parametrize('value', [0, 0.0, -0.5, float('inf'), float('nan'), '0.5', True, False, [0.5]])
def test_a_malformed_scale_is_refused_by_key(value):
    with pytest.raises(ValueError, match=r'unimodal\.laplace_scale'):
        _settings({'laplace_scale': value})


def test_a_non_block_is_refused():
    for bad in (True, 3, 'on', [1]):
        with pytest.raises(ValueError, match='unimodal'):
            _settings(bad)


# ---- the loss bank
def _sel(config, loss_type, **over):
    from dualpixelface_amd import load_option, losses
    return losses.loss_selector(load_option(config, loss_type=loss_type, lambdas=[1.0] * len(loss_type), **over))


@pytest.mark.parametrize('config', ['train_faceDP', 'train_faceDP_psmnet', 'train_faceDP_nnet'])
def test_the_selector_accepts_it_for_the_models_with_a_volume_at_the_output_resolution(config):
    from dualpixelface_amd import losses
    assert losses._BANK['unimodal'] is losses.UNIMODALLoss
    sel = _sel(config, ['smoothL1', 'unimodal'])
    assert sel.loss_name == ['smoothL1', 'unimodal'] and not sel.label_free()
    assert sel.loss_func[1].settings.laplace_scale is None
    assert _sel(config, ['unimodal'], unimodal={'laplace_scale': 0.75}).loss_func[0].settings.laplace_scale == 0.75
    with pytest.raises(ValueError, match=r'unimodal\.laplace_scale'):
        _sel(config, ['unimodal'], unimodal={'laplace_scale': 0})


@pytest.mark.parametrize('config,model', [('train_faceDP_dpnet', 'dpnet'), ('train_faceDP_stereonet', 'stereonet')])
def test_the_selector_refuses_it_by_model_name_where_there_is_no_such_volume(config, model):
    with pytest.raises(NotImplementedError, match="'unimodal'.*%s" % model):
        _sel(config, ['smoothL1', 'unimodal'])


def test_folded_and_least_square_stay_refused_next_to_it():
    with pytest.raises(NotImplementedError, match='wrong loss type : folded'):
        _sel('train_faceDP', ['unimodal', 'folded'])
    from dualpixelface_amd import load_option, losses
    opt = load_option('train_faceDP', loss_type=['unimodal'], lambdas=[1.0])
    opt.dataset.dp_conversion = 'least_square'
    with pytest.raises(NotImplementedError, match='least_square'):
        losses.loss_selector(opt)


def test_the_hook_takes_smooth_l1s_target_rule_and_refuses_other_target_types(monkeypatch):
    from dualpixelface_amd import losses, ops
    seen = []
    monkeypatch.setattr(ops, 'unimodal_loss', lambda *a, **k: seen.append((a, k)) or torch.zeros(()))
    monkeypatch.setattr(ops, 'affine_fit', lambda pred, idepth: 'fitted-ab')
    logits = [torch.zeros(1, 1, 8, 2, 3) for _ in range(3)]
    heads = {'logits': logits, 'disp_values': uc.shipped_disp(), 'scale': 4, 'align_corners': True}
    preds = {'pred_depth': torch.zeros(1, 3, 8, 12), '_heads': heads}
    batch = {'disp': 'DISP', 'depth': 'DEPTH', 'idepth': 'IDEPTH', 'mask': 'MASK', 'abvalue': 'AB'}
    fn = _sel('train_faceDP', ['unimodal'], unimodal={'laplace_scale': 0.75}).loss_func[0]
    out = fn.forward(preds, batch)
    (a, k), = seen
    assert a == (logits, heads['disp_values'], 'DISP', 'MASK') and out['abvalue'] == 'AB'
    assert k == dict(head_weights=[1.0, 0.7, 0.5], scale=4, align_corners=True, laplace_scale=0.75)
    del seen[:]
    fitted = {key: v for key, v in batch.items() if key != 'abvalue'}
    out = fn.forward(preds, fitted)                                           # no 'abvalue': the depth map and the fitted (a, b)
    (a, k), = seen
    assert a == (logits, heads['disp_values'], 'DEPTH', 'MASK') and k['target_ab'] == 'fitted-ab' and out['abvalue'] == 'fitted-ab'
    for target_type in ('depth', 'idepth'):
        with pytest.raises(NotImplementedError, match="'unimodal'.*'disp'.*%s" % target_type):
            fn.forward(preds, batch, target_type=target_type)
    with pytest.raises(NotImplementedError, match="_heads"):
        fn.forward({'pred_depth': preds['pred_depth']}, batch)


def test_the_operator_refuses_cpu_tensors_and_malformed_operands():
    from dualpixelface_amd import ops
    from dualpixelface_amd._lib import DpfError
    k, t, d = torch.zeros(1, 1, 8, 2, 3), torch.zeros(1, 8, 12), uc.shipped_disp()
    with pytest.raises(DpfError, match='GPU tensors'):
        ops.unimodal_loss([k], d, t)
    with pytest.raises(DpfError, match='list of 1..8'):
        ops.unimodal_loss([], d, t)
    with pytest.raises(DpfError, match='list of 1..8'):
        ops.unimodal_loss([k] * 9, d, t)
    with pytest.raises(DpfError, match='list of 1..8'):
        ops.unimodal_loss(k, d, t)
    assert str(inspect.signature(ops.unimodal_loss)) == (
        "(logits, disp_values, target, mask=None, target_ab=None, head_weights=(1.0,), scale=4, align_corners=True, laplace_scale=None, "
        "return_extras=False)")


# ---- the plugin
def test_forward_removes_the_private_record_after_the_hook_and_a_network_without_one_keeps_working(monkeypatch):
    from dualpixelface_amd import load_option
    from dualpixelface_amd.plugin import STEREODPNET
    batch = {'left': torch.zeros(1, 3, 8, 12), 'right': torch.zeros(1, 3, 8, 12), 'disp': torch.zeros(1, 8, 12)}
    pred, heads = torch.ones(1, 3, 8, 12), {'logits': []}
    model = STEREODPNET(load_option('train_faceDP_unimodal'))
    seen = []
    monkeypatch.setattr(model.loss_model, 'forward',
                        lambda results, b, target_type='disp': seen.append(results.get('_heads')) or {'final_loss': 1.0})
    for with_heads in (True, False):
        model.network = lambda b: dict({'pred_depth': pred, '_taps': None}, **({'_heads': heads} if with_heads else {}))     # the stub
        del seen[:]
        model.train()
        out = model._forward(batch)
        assert seen == [heads if with_heads else None] and set(out) == {'pred_depth', 'final_loss'}
        model.eval()
        assert set(model._forward(batch)) == {'pred_depth'} and len(seen) == 1


# ---- configs
def test_configs_are_their_bases_with_the_loss_and_the_block_spelled_out():
    from dualpixelface_amd import load_option, unimodal
    base = json.load(open(os.path.join(ROOT, 'src', 'model', 'stereodpnet', 'config.json')))
    ours = json.load(open(os.path.join(ROOT, 'src', 'model', 'stereodpnet', 'config_unimodal.json')))
    block = ours.pop('unimodal')
    assert block == {'laplace_scale': None} and set(block) == set(unimodal.Settings._fields)
    assert ours.pop('loss_type') == ['smoothL1', 'cosine', 'unimodal'] and ours.pop('lambdas') == [1.0, 1.0, 0.1]
    assert base.pop('loss_type') == ['smoothL1', 'cosine'] and base.pop('lambdas') == [1.0, 1.0] and ours == base
    top_base = json.load(open(os.path.join(ROOT, 'config_', 'train_faceDP.json')))
    top = json.load(open(os.path.join(ROOT, 'config_', 'train_faceDP_unimodal.json')))
    assert top.pop('model_config') == 'config_unimodal' and top_base.pop('model_config') == 'config' and top == top_base
    opt = load_option('train_faceDP_unimodal')
    assert opt.model_name == 'stereodpnet' and opt.model.loss_type == ['smoothL1', 'cosine', 'unimodal']
    assert tuple(unimodal.settings(opt)) == (None,)
    for name in sorted(f[:-5] for f in os.listdir(os.path.join(ROOT, 'config_')) if f.endswith('.json')):
        assert ('unimodal' in load_option(name).model.loss_type) == (name == 'train_faceDP_unimodal'), name


# ---- C ABI
def test_header_declares_the_entry_points_and_forward_and_backward_share_their_leading_arguments():
    from dualpixelface_amd import _lib
    protos = _lib.parse_header()
    q = protos['dpf_unimodal_workspace_bytes']
    assert q[0] is _lib._CTYPES['long long'] and [n for _, n in q[1]] == ['B', 'n', 'H', 'W']
    fwd = [n for _, n in protos['dpf_unimodal_forward'][1]]
    bwd = [n for _, n in protos['dpf_unimodal_backward'][1]]
    assert len(fwd) == 24 and len(bwd) == 21 and fwd[:16] == bwd[:16]
    assert fwd[:16] == ['logits_host', 'target', 'mask', 'target_ab', 'B', 'n', 'D', 'h', 'w', 'L', 'H', 'W', 'align_corners', 'disp_host',
                        'laplace_scale', 'head_weights_host']
    assert fwd[16:] == ['ws', 'ws_bytes', 'logsum', 'stats', 'out', 'counted_out', 'expect_out', 'stream']
    assert bwd[16:] == ['logsum', 'stats', 'gout', 'dlogits_host', 'stream']
    make = open(os.path.join(ROOT, 'dualpixelface_amd', 'csrc', 'Makefile')).read()
    assert '$(OBJDIR)/unimodal.o: CXXFLAGS += -ffp-contract=off' in make and ' dpf_softargmin.h' in make
    # one definition of the head's index arithmetic: both files take it from the header
    for name in ('softargmin.hip', 'unimodal.hip'):
        src = open(os.path.join(ROOT, 'dualpixelface_amd', 'csrc', name)).read()
        assert '#include "dpf_softargmin.h"' in src and 'void ac_src(' not in src and 'float head_ratio(' not in src, name


# ---- the cases
@pytest.mark.parametrize('name', sorted(uc.CASES))
def test_every_case_counts_between_a_quarter_and_nine_tenths_of_its_pixels(name):
    r = uc.case(name)
    c, counted = r['case'], r['r32']['counted']
    share = counted.mean()
    print('%s: %d of %d pixels counted' % (name, counted.sum(), counted.size))
    assert 0.25 <= share <= 0.90
    for h in range(counted.shape[1]):
        assert np.array_equal(counted[:, h], counted[:, 0])                   # the label decides, not the head
    if c['ab'] is None:
        t = c['target']
        for kind, (b, y, x) in c['kinds'].items():                            # each planted pixel lies inside the mask and is left out
            assert (c['mask'] is None or c['mask'][b, y, x] > 0) and not counted[b, 0, y, x], kind
        assert np.isnan(t[c['kinds']['nan']]) and np.isinf(t[c['kinds']['inf']])
        assert t[c['kinds']['below']] < c['disp'][0] and t[c['kinds']['above']] > c['disp'][-1]


def test_the_cases_leave_pixels_out_for_every_reason():
    multi = uc.case('multi-tile')['case']
    assert set(multi['kinds']) == {'nan', 'inf', 'below', 'above'} and (multi['mask'] == 0).any()
    t, on = uc.case('multi-tile')['r32']['t'], uc.case('multi-tile')['r32']['counted'][:, 0] > 0
    inside = multi['mask'] > 0
    assert (inside & ~on & (t < multi['disp'][0])).sum() > 1 and (inside & ~on & (t > multi['disp'][-1])).sum() > 1
    fitted = uc.case('fitted')
    depth = fitted['case']['target']
    assert (depth == 0).any() and (depth < 0).any() and np.isnan(depth).any() and not fitted['r32']['counted'][~np.isfinite(fitted['r32']['t'])[:, None]].any()
    assert uc.CASES['general']['uneven'] and len(set(np.round(np.diff(uc.case('general')['case']['disp']), 4))) > 8
    assert uc.case('thin')['case']['logits'][0].shape[3] == 1 and not uc.case('half-pixel')['case']['align']


# ---- the oracle
def test_fp64_autograd_gradient_agrees_with_central_differences():
    """The fp64 torch restatement against central differences of its own loss on 'one-tile', every element, at step h = 1e-4.  With
    `counted` held the loss is smooth in the logits: a mean over pixels of logsumexp(u) - sum_l P_l u_l, u linear in the logits with
    non-negative weights that sum to at most 1 per u_l, so a unit step of one logit moves every u_l by at most 1.  Truncation:
    h^2 |f'''| / 6, and the third directional derivative of logsumexp is the third cumulant of a variable in [0, 1], at most
    1 / (6 sqrt 3) < 0.1, times sum w.  Rounding: the loss is a mean of terms of magnitude up to the loss itself, each accurate to a few
    units of 2^-53 relative; 64 x 2^-53 x max(loss, 1) is taken for the error e of one evaluation, and the difference quotient has 2 e /
    (2 h).  The bar is the sum of the two; h = 1e-4 is near where they meet ((3 e / 0.1)^(1/3) = 6e-5 for a loss of 4)."""
    r = uc.case('one-tile')
    c, on = r['case'], r['r32']['counted'][:, 0] > 0
    (k0,) = [torch.tensor(k.astype(np.float64)) for k in c['logits']]
    f = lambda k: float(uc.torch_loss([k], on, c['disp'], c['target'], c['ab'], c['head_weights'], c['scale'], c['align'], c['s']))   # noqa: E731
    g, h = r['grad64'][0], 1e-4
    bar = h * h * 0.1 * sum(c['head_weights']) / 6 + 64 * 2.0 ** -53 * max(abs(r['loss64']), 1.0) / h
    worst = 0.0
    for i in range(k0.numel()):
        e = torch.zeros(k0.numel(), dtype=torch.float64)
        e[i] = h
        fd = (f(k0 + e.view_as(k0)) - f(k0 - e.view_as(k0))) / (2 * h)
        worst = max(worst, abs(fd - g.ravel()[i]))
    print('central differences: worst %.3e against the bar %.3e, largest gradient %.3e' % (worst, bar, np.abs(g).max()))
    assert worst <= bar and np.abs(g).max() > 1e4 * bar


@pytest.mark.parametrize('name', ['one-tile', 'general', 'half-pixel'])
def test_zero_logits_give_sum_w_log_L_whatever_the_target(name):
    r = uc.case(name)
    c = dict(r['case'], logits=[np.zeros_like(k) for k in r['case']['logits']])
    L = len(c['disp'])
    want = sum(float(np.float32(w)) for w in c['head_weights']) * math.log(L)
    got64, _ = uc.loss_and_grad(c, r['r32']['counted'][:, 0] > 0, torch.float64)
    got32 = uc.run(c)['loss']
    print('%s: zero logits %.9g (fp64) %.9g (fp32 restatement), sum w log %d = %.9g' % (name, got64, got32, L, want))
    assert abs(got64 - want) <= 1e-12 * want
    assert abs(got32 - want) <= 4 * 2.0 ** -24 * want          # log(float(L)) rounded, a product with w, the sum over heads, the fp32 result


@pytest.mark.parametrize('name', sorted(uc.CASES))
def test_the_gradient_of_every_head_sums_to_zero_and_the_restatements_agree(name):
    """sum_l (p_l - P_l) = 0 at every pixel and the upsample's weights sum to 1 over the cells, so d k_i sums to 0 up to rounding: some
    thousand fp64 terms of at most the largest |gradient| each."""
    r = uc.case(name)
    for g in r['grad64']:
        assert abs(g.sum()) <= g.size * 2.0 ** -52 * np.abs(g).max() and np.abs(g).max() > 0
    own = abs(r['r32']['loss'] - r['loss64'])
    print('%s: loss fp64 %.12g, fp32 torch off by %.3e, fp32 kernel order off by %.3e' % (name, r['loss64'], abs(r['loss32'] - r['loss64']), own))
    assert own <= 64 * 2.0 ** -24 * r['loss64'] and abs(r['loss32'] - r['loss64']) <= 64 * 2.0 ** -24 * r['loss64']
    # expect is the soft-argmin's value: inside the hypotheses' range
    ex = r['r32']['expect']
    assert (ex >= r['case']['disp'][0] - 1e-4).all() and (ex <= r['case']['disp'][-1] + 1e-4).all()
