"""The DPNet plugin on the GPU (run with ``-m gpu``) against vectors produced by importing the reference's src/model/dpnet
(tests/golden/make_golden_dpnet.py): forward, loss, every stored gradient, running statistics, eval; the fused train step under every
optimiser with graph replay against an eager twin; one full-size step; the trainer entry point in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import support
from tests.support import DEV, close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_SPREAD = 4          # the project's multiple of the reference's own fp32 noise


def _model(config='train_faceDP_dpnet', **over):
    return support.build('DPNET', support.option_set(config, **over))


def test_dpnet_plugin_against_reference_golden(golden_dir):
    from dualpixelface_amd.recipe import fill_by_recipe, synthetic_batch
    g = np.load(golden_dir + '/dpnet_64x96_b2.npz')
    keys = json.load(open(golden_dir + '/dpnet_state_dict_keys.json'))
    model = _model()
    assert {k: list(v.shape) for k, v in model.state_dict().items()} == keys and list(model.state_dict()) == list(keys)
    batch = {k: v.to(DEV) for k, v in synthetic_batch(2, 64, 96, seed=13).items()}
    model.flat_gradients(zero=True)
    res = model(batch)

    def sampled(name, t):
        st = int(g['stride::' + name]) if 'stride::' + name in g.files else 1
        return t[..., ::st, ::st]

    for name in ('x_layer1', 'x_layer5', 'y_layer5', 'y_layer2'):
        close(sampled('tap::' + name, model.last_taps[name]), g['tap::' + name], 2e-4, 'dpnet ' + name)
    assert res['pred_depth'].shape == (2, 5, 64, 96)
    close(res['pred_depth'], g['train_pred_depth'], 2e-4, 'dpnet pred_depth')
    close(res['ref_feature'], g['train_ref_feature'], 2e-4, 'dpnet ref_feature')
    close(res['smoothL1_loss'], g['smoothL1_loss'], 1e-4, 'dpnet smoothL1')
    close(res['final_loss'], g['final_loss'], 1e-4, 'dpnet loss')
    res['final_loss'].backward()
    pd = dict(model.named_parameters())
    assert all(p.grad is not None for p in pd.values())            # every parameter receives a gradient
    checked, failed = 0, []
    for k in g.files:
        if not k.startswith('grad::'):
            continue
        ref = torch.from_numpy(g[k]).double()
        assert ref.norm() >= 1e-6
        mine = pd[k[6:]].grad.detach().cpu().double()
        rel = ((mine - ref).norm() / ref.norm()).item()
        bound = max(2e-2, K_SPREAD * float(g['noise::' + k[6:]]))
        print('%s: rel L2 %.3e (bound %.3e, reference fp32 noise %.3e)' % (k, rel, bound, float(g['noise::' + k[6:]])))
        checked += 1
        if not rel <= bound:
            failed.append((k, rel, bound))
    assert checked == 16 and not failed, failed
    sd = model.state_dict()
    for k in g.files:
        if k.startswith('post::'):
            close(sd[k[6:]], g[k], 1e-4, k)
    assert int(sd['enc_layer1_1.conv1.bn.num_batches_tracked']) == 1
    fill_by_recipe(model)
    model.eval()
    with torch.no_grad():
        ev = model(batch)
    close(sampled('eval_pred_depth', ev['pred_depth']), g['eval_pred_depth'], 5e-4, 'dpnet eval pred_depth')


@pytest.mark.parametrize('optim', ['adam', 'sgd', 'rmsprop'])
def test_train_step_graph_replay_equals_eager(optim, monkeypatch):
    from dualpixelface_amd import ops
    from dualpixelface_amd.recipe import synthetic_batch
    batch = {k: v.to(DEV) for k, v in synthetic_batch(2, 64, 96, seed=7, mask_mode='bern').items()}
    with ops.deterministic_mode():
        monkeypatch.setenv('DPF_STEP_GRAPH', '1')
        a = _model(optim=optim)
        before = a.flat_parameters().clone()
        la = [float(a.train_step(batch, None, lr=1e-3)['final_loss'].detach()) for _ in range(5)]      # two warm-up steps, the capture, two replays
        assert a._graph_state.get('graph') is not None and not a._graph_state.get('failed')
        monkeypatch.setenv('DPF_STEP_GRAPH', '0')
        b = _model(optim=optim)
        lb = [float(b.train_step(batch, None, lr=1e-3)['final_loss'].detach()) for _ in range(5)]
    assert all(np.isfinite(la)) and la == lb, (la, lb)
    assert float((a.flat_parameters() - before).abs().max()) > 0
    assert torch.equal(a.flat_parameters(), b.flat_parameters())
    sa, sb = a.state_dict(), b.state_dict()
    for k in ('enc_layer1_1.conv1.bn.running_mean', 'conv_last_layer3.bn.running_var', 'skip_layer2.bn.num_batches_tracked'):
        assert torch.equal(sa[k], sb[k]), k


def test_full_size_step_agrees_across_matrix_paths():
    """2 x 1024 x 1536, the reference config's batch: forward + backward complete, and the loss agrees with the same step on the fp32
    matrix instructions to the tolerance test_headline_config_whole_train_step holds the two paths to (1e-5)."""
    from dualpixelface_amd import ops
    from dualpixelface_amd.recipe import synthetic_batch
    batch = {k: v.to(DEV) for k, v in synthetic_batch(2, 1024, 1536, seed=2, mask_mode='bern').items()}
    prev = ops.f32_matrix_path()
    losses = {}
    try:
        for path in (prev, 0):
            ops.set_f32_matrix_path(path)
            model = _model()
            model.flat_gradients(zero=True)
            res = model(batch)
            assert res['pred_depth'].shape == (2, 5, 1024, 1536)
            res['final_loss'].backward()
            torch.cuda.synchronize()
            assert torch.isfinite(res['final_loss']) and bool(torch.isfinite(model.flat_gradients(zero=False)).all())
            losses[path] = float(res['final_loss'])
            del model, res
    finally:
        ops.set_f32_matrix_path(prev)
    print('full-size loss per path', losses)
    assert abs(losses[prev] - losses[0]) <= 1e-5 * abs(losses[0]), losses


def _main(*args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, 'main.py'] + list(args), cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def test_trainer_resume_and_eval(tmp_path, golden_dir):
    """main.py in a child process: train -> checkpoint (the reference's key names) -> resume lands where the uninterrupted run does; the
    eval config runs test_step with absolute_dp + affine_dp."""
    from dualpixelface_amd import load_option
    from dualpixelface_amd.synthetic_data import synthetic_loader
    from dualpixelface_amd.trainer import Trainer
    keys = json.load(open(golden_dir + '/dpnet_state_dict_keys.json'))
    _main('--config', 'train_faceDP_dpnet', '--workspace', 'pytest_dpnet', '--synthetic', '16', '--height', '64', '--width', '96', '--max_steps', '4')
    ws = os.path.join(ROOT, 'workspace', 'dpnet', 'pytest_dpnet')
    ck_path = os.path.join(ws, 'checkpoint_epoch=00.ckpt')
    ck = torch.load(ck_path, map_location='cpu', weights_only=False)
    assert list(ck['state_dict']) == list(keys)
    r = _main('--config', 'eval_faceDP_dpnet', '--workspace', 'pytest_dpnet_eval', '--synthetic', '4', '--height', '64', '--width', '96',
              '--load_model', ck_path)
    import ast
    rows = ast.literal_eval([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    assert set(rows) == {'absolute_dp', 'affine_dp'}

    def finite(v):
        return all(finite(x) for x in (v.values() if isinstance(v, dict) else v)) if isinstance(v, (dict, list, tuple)) else bool(np.isfinite(v))
    assert finite(rows), rows
    # resume == uninterrupted, in process (deterministic mode: the same bits)
    from dualpixelface_amd import ops
    with ops.deterministic_mode():
        opt = load_option('train_faceDP_dpnet')
        opt.epoch, opt.init_lr, opt.scheduler = 2, 1e-3, 'explr'
        loader = synthetic_loader(4, 64, 96, batch_size=2, seed=3)
        val = synthetic_loader(2, 64, 96, batch_size=1, seed=4)
        a = _model(epoch=2, init_lr=1e-3, scheduler='explr')
        ta = Trainer(a.option, str(tmp_path / 'a'), rank=0, world_size=1)
        ta.fit(a, loader, val)
        b = _model(epoch=2, init_lr=1e-3, scheduler='explr', load_model=ta.checkpoint_path(0))
        with torch.no_grad():
            b.flat_parameters().mul_(0.5)
        tb = Trainer(b.option, str(tmp_path / 'b'), rank=0, world_size=1)
        tb.fit(b, loader, None)
    assert tb.epoch == 2 and tb.global_step == ta.global_step == 4
    diff = (a.flat_parameters() - b.flat_parameters()).abs().max().item()
    assert diff <= 1e-6, diff
