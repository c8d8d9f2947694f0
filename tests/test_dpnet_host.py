"""DPNet plugin, host side (no GPU): the class resolves through every entry point, the configs load, the state_dict contract equals
the reference's 625 entries (tests/golden/make_golden_dpnet.py) and the shape arithmetic of the network holds."""
import json
import os
from runpy import run_path

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plugin_class_resolves():
    from dualpixelface_amd.plugin import DPNET
    assert run_path(os.path.join(ROOT, 'src', 'model', 'dpnet', 'mainmodel.py'))['DPNET'] is DPNET


@pytest.mark.parametrize('config,mode', [('train_faceDP_dpnet', 'train'), ('eval_faceDP_dpnet', 'test')])
def test_configs_load(config, mode):
    from dualpixelface_amd import load_option
    opt = load_option(config)
    assert opt.model_name == 'dpnet' and opt.mode == mode
    assert len(opt.model.loss_weight) == 5 and opt.model.loss_weight[0] == 1.0
    assert opt.model.metric_type == ['absolute_dp', 'affine_dp']
    assert opt.model.loss_type == ['smoothL1'] and opt.batch_size == 2


def test_state_dict_contract(golden_dir):
    from dualpixelface_amd import load_option
    from dualpixelface_amd.dpnet import build_dpnet_spec
    from dualpixelface_amd.plugin import DPNET
    keys = json.load(open(os.path.join(golden_dir, 'dpnet_state_dict_keys.json')))
    assert len(keys) == 625
    spec = build_dpnet_spec(load_option('train_faceDP_dpnet'))
    assert [(n, list(s)) for n, s, _, _ in spec.items] == [(k, v) for k, v in keys.items()]
    model = DPNET(load_option('train_faceDP_dpnet'))
    sd = model.state_dict()
    assert list(sd) == list(keys) and {k: list(v.shape) for k, v in sd.items()} == keys
    assert sum(p.numel() for p in model.parameters()) == 550766 == model.flat_parameters().numel()
    # initialisation (mainmodel.py:95-117): PReLU 0.05, BatchNorm 1 / 0, Xavier-uniform convolutions
    assert float(sd['prelu.weight']) == pytest.approx(0.05) and float(sd['enc_layer3_1.prelu.weight']) == pytest.approx(0.05)
    assert float(sd['conv_last_layer1.bn.weight']) == 1.0 and float(sd['conv_last_layer1.bn.bias']) == 0.0
    w = sd['enc_layer1_1.conv1.conv.weight']
    bound = (6.0 / (6 * 49 + 8 * 49)) ** 0.5
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.8 * bound


@pytest.mark.parametrize('hw', [(64, 96), (128, 192), (1024, 1536)])
def test_shape_arithmetic(hw):
    from dualpixelface_amd.dpnet import dpnet_shapes
    H, W = hw
    s = dpnet_shapes(H, W)
    for lvl, scale in ((5, 16), (4, 8), (3, 4), (2, 2), (1, 1)):
        assert s['head%d' % lvl] == (H // scale, W // scale) and s['out%d' % lvl] == (H, W)
    # mainmodel.py:162-177: x_layer1 = H/2 - 2, every further level (previous - 3) // 2 + 1 (+ padding), decoders 2x + the padded 1x1
    assert s['x_layer1'] == (H // 2 - 2, W // 2 - 2)
    assert s['x_layer2'] == ((s['x_layer1'][0] - 3) // 2 + 1, (s['x_layer1'][1] - 3) // 2 + 1)
    assert s['x_layer3'] == (H // 8, W // 8) and s['x_layer4'] == (H // 16, W // 16) and s['x_layer5'] == (H // 32, W // 32)
    assert s['y_layer5'] == (H // 16 + 4, W // 16 + 4) and s['y_layer4'] == (H // 8 + 6, W // 8 + 6)
    assert s['y_layer3'] == (H // 4 + 4, W // 4 + 4) and s['y_layer2'] == (H // 2 + 4, W // 2 + 4) and s['y_layer1'] == (H + 4, W + 4)


def test_reference_comment_shapes():
    """The sizes written next to DPNET.forward (mainmodel.py:162-177) belong to a 768 x 512 input."""
    from dualpixelface_amd.dpnet import dpnet_shapes
    s = dpnet_shapes(768, 512)
    assert s['y_layer5'] == (52, 36)                       # "torch.Size([1, 128, 52, 36])"
    assert (s['y_layer4'][0] - 2, s['y_layer4'][1] - 2) == (100, 68)
    assert (s['y_layer3'][0] - 2, s['y_layer3'][1] - 2) == (194, 130)
    assert (s['y_layer2'][0] - 2, s['y_layer2'][1] - 2) == (386, 258)


def test_sizes_that_do_not_fit_are_refused():
    from dualpixelface_amd.dpnet import dpnet_shapes
    with pytest.raises(ValueError):
        dpnet_shapes(70, 96)


def test_folded_loss_is_still_refused():
    from dualpixelface_amd import load_option
    from dualpixelface_amd.losses import loss_selector
    opt = load_option('train_faceDP_dpnet', loss_type=['folded'])
    with pytest.raises(NotImplementedError, match='wrong loss type'):
        loss_selector(opt)


def test_validation_hooks_are_noops():
    from dualpixelface_amd import load_option
    from dualpixelface_amd.plugin import DPNET
    model = DPNET(load_option('eval_faceDP_dpnet'))
    assert model.validation_step({}, 0) is None and model.validation_epoch_end([]) is None
