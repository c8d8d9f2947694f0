"""GPU tests (``-m gpu``) of the ASM ablation switches: shift-mode subsets (M = 1, 2, 3 copies), the variance fetch and the PReLU gate --
operator level against fp64 torch restatements of src/module/asm/asm.py, end to end against the imported reference's own runs
(tests/golden/make_golden_asm.py: variants V1 ... V5 at 2 x 32 x 48).

Operator bounds.  cv_select: per element 16 x 2^-24 x (sum of the absolute values of the terms the element is a sum of, from the fp64
reference) -- the variance form `mean z^2 - (mean z)^2` cancels, so a bound relative to the result would be wrong.  Shift copies: the
fixture tolerance of tests/test_gpu_ops.py (5e-6 of the maximum); the adjoint through <A x, g> = <x, A^T g> to 1e-5.  Instance norm +
PReLU: the tolerances of the norm_act tests of tests/test_gpu_ops.py (1e-5 forward, 2e-4 gradients, of the maximum).
End-to-end tolerances are those of tests/test_gpu_e2e.py at this size; the gradient budget is K_SPREAD x the reference's own fp32-vs-fp64
distance per tensor (constants imported from there)."""
import functools
import itertools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import support
from tests.support import DEV, close, rnd
from tests.test_gpu_e2e import GRAD_FLOOR, K_SPREAD, build_model

pytestmark = pytest.mark.gpu
MODES = ('nearest', 'bilinear', 'phase')
SUBSETS = [s for s in itertools.product((False, True), repeat=3) if any(s)]
SUBSET_IDS = ['+'.join(m for m, on in zip(MODES, s) if on) for s in SUBSETS]
EPS = 2.0 ** -24


def _device_tables(h, w, delta, subset):
    from dualpixelface_amd.sampler_tables import build_phase_tables, build_shift_tables, is_fractional
    cpu = build_shift_tables(h, w, delta, *subset)
    phase = None
    if subset[2] and is_fractional(delta):
        phase = tuple(t.to(DEV) if torch.is_tensor(t) else t for t in build_phase_tables(h, w, delta))
    return cpu, tuple(t.to(DEV) for t in cpu), phase


def _adjoint_identity(ops, fea, out, tables, phase, seed, name):
    """<A x, g> = <x, A^T g>, inner products in fp64.  g = A x + noise: the left side is then |A x|^2 plus a fluctuation, never a sum
    that cancels to nothing (a relative bound on a cancelled sum would test the seed)."""
    fg = fea.detach().requires_grad_()
    y = ops.shift_triple(fg, tables, phase)
    g = (out.detach() + rnd(*out.shape, seed=seed).to(DEV)).contiguous()
    (gx,) = torch.autograd.grad(y, fg, g)
    lhs = (y.detach().double() * g.double()).sum().item()
    rhs = (fea.double() * gx.double()).sum().item()
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs), '%s: <Ax,g> %.9e vs <x,ATg> %.9e' % (name, lhs, rhs)
    (gx2,) = torch.autograd.grad(ops.shift_triple(fg, tables, phase), fg, g)          # gather adjoint: no atomics
    assert torch.equal(gx, gx2), name


@pytest.mark.parametrize('subset', SUBSETS, ids=SUBSET_IDS)
def test_shift_copies_forward_and_gather_adjoint(golden_dir, subset):
    """Every non-empty subset of the three modes: [B,C,M,h,w] with no dead slot, against the reference's own copies (six deltas, four of
    them fractional -- with `nearest` or `bilinear` off the fractional phase copy lands in slot 0 or 1 -- three shapes, both directions),
    then a random 10 x 13 map (a row tail below the 8-row block, w % 4 != 0: the scalar column path) against the fp64 table evaluation."""
    from dualpixelface_amd.sampler_tables import apply_tables_reference, is_fractional
    from oracle.stereodpnet import StereoDPNetOracle
    ops = support.ops()
    g = np.load(golden_dir + '/shift_fractional.npz')
    names = [m for m, on in zip(MODES, subset) if on]
    for ci in range(3):
        fea = torch.from_numpy(g['fea%d' % ci]).to(DEV)
        for di, delta in enumerate(g['deltas']):
            for direction, sign in (('forward', 1.0), ('backward', -1.0)):
                d = sign * float(delta)
                _, tables, phase = _device_tables(fea.shape[2], fea.shape[3], d, subset)
                out = ops.shift_triple(fea, tables, phase)
                assert out.shape == (fea.shape[0], fea.shape[1], len(names)) + tuple(fea.shape[2:])
                for j, nm in enumerate(names):
                    ref = torch.from_numpy(g['c%d_d%d_%s_%s' % (ci, di, direction, nm)]).double()
                    err = (out[:, :, j].cpu().double() - ref).abs().max().item()
                    assert err <= 5e-6 * ref.abs().max().item(), (nm, d, direction, err)
                if direction == 'forward':
                    _adjoint_identity(ops, fea, out, tables, phase, 100 + di, 'c%d d %s' % (ci, d))
    fea = rnd(2, 3, 10, 13, seed=71)
    for d in (1.0, -2.0, 0.5, -1.75):
        cpu, tables, phase = _device_tables(10, 13, d, subset)
        out = ops.shift_triple(fea.to(DEV), tables, phase)
        ref = apply_tables_reference(fea.double(), tuple(t.double() if t.is_floating_point() else t for t in cpu))
        if phase is not None:                                       # the fractional phase copy is not table-driven
            ref[:, :, -1] = StereoDPNetOracle.shift_triple(fea.double(), d)[2]
        err = (out.cpu().double() - ref).abs().max().item()
        assert err <= 5e-6 * ref.abs().max().item(), (d, err)
        _adjoint_identity(ops, fea.to(DEV), out, tables, phase, 7, 'random d %s' % d)


def _select_reference(x, s, go, mask, L, fetch):
    """asm.py:162-171 in fp64 with autograd on the CPU, broadcast to the levels of `mask`; and, per element of every output, the sum of
    the absolute values of its terms."""
    x = x.double().requires_grad_()
    s = s.double().requires_grad_()
    M = x.shape[2]
    z = x * F.softmax(s, dim=2)
    if fetch:
        avg = torch.mean(z, 2)
        out = torch.mean(z ** 2, 2) - avg ** 2
    else:
        out = torch.mean(z, 2)
    lv = torch.tensor([float((mask >> l) & 1) for l in range(L)], dtype=torch.float64).view(1, 1, L, 1, 1)
    vol = out.unsqueeze(2) * lv
    dx, ds = torch.autograd.grad(vol, (x, s), go.double())
    with torch.no_grad():
        p = F.softmax(s, dim=2)
        za = z.abs()
        mean_abs = za.sum(2) / M
        t_out = ((z ** 2).sum(2) / M + mean_abs ** 2) if fetch else mean_abs
        t_vol = t_out.unsqueeze(2) * lv
        G = (go.double().abs() * lv).sum(2, keepdim=True)                            # |terms| of the summed level gradient
        t_dz = G * 2.0 * (za + mean_abs.unsqueeze(2)) / M if fetch else (G / M).expand_as(z)
        t_dx = p * t_dz
        t_dp = x.abs() * t_dz
        t_ds = p * (t_dp + (p * t_dp).sum(2, keepdim=True))
    return vol.detach(), dx, ds, t_vol, t_dx, t_ds


def _within(a, ref, terms, name):
    err = (a.detach().cpu().double() - ref).abs()
    bound = 16.0 * EPS * terms
    worst = (err - bound).max().item()
    assert worst <= 0, '%s: %d of %d elements beyond 16 x 2^-24 x sum|terms| (worst excess %.3e, max err %.3e)' % (
        name, int((err > bound).sum()), err.numel(), worst, err.max().item())


@pytest.mark.parametrize('fetch', [False, True], ids=['mean', 'fetch'])
@pytest.mark.parametrize('M', [1, 2, 3])
def test_cv_select_copies_and_fetch(M, fetch):
    ops = support.ops()
    B, C, L, h = 2, 5, 8, 10
    for w, masks in ((13, (0xFF, 0x01, 0xA4)), (24, (0xA4,))):
        xs = [rnd(B, C, M, h, w, seed=80 + M + i) for i in range(2)]
        ss = [torch.sigmoid(rnd(B, C, M, h, w, seed=90 + M + i) * 2.0) for i in range(2)]        # the already activated mask
        go = rnd(B, 2 * C, L, h, w, seed=99)
        for mask in masks:
            refs = [_select_reference(xs[i], ss[i], go[:, i * C:(i + 1) * C], mask, L, fetch) for i in range(2)]
            tg = [t.to(DEV).requires_grad_() for t in (xs[0], ss[0], xs[1], ss[1])]
            vol = ops.cv_select(L, [mask], tg, fetch)
            assert vol.shape == (B, 2 * C, L, h, w)
            grads = torch.autograd.grad(vol, tg, go.to(DEV))
            for i in range(2):
                rv, rdx, rds, tv, tdx, tds = refs[i]
                name = 'M %d fetch %d w %d mask %#x half %d' % (M, fetch, w, mask, i)
                _within(vol[:, i * C:(i + 1) * C], rv, tv, name + ' vol')
                _within(grads[2 * i], rdx, tdx, name + ' dx')
                _within(grads[2 * i + 1], rds, tds, name + ' ds')
                if M == 1:
                    assert float(grads[2 * i + 1].abs().max()) == 0.0, name + ': one copy, softmax == 1: ds is exactly zero'
                    if fetch:
                        assert float(vol.abs().max()) == 0.0 and float(grads[2 * i].abs().max()) == 0.0, name + ': z^2 - z^2'
            unset = [l for l in range(L) if not (mask >> l) & 1]
            if unset:
                assert float(vol.detach()[:, :, unset].abs().max()) == 0.0


def test_instance_norm_prelu_gate():
    """The PReLU gate: instance norm (affine) + PReLU with ONE slope over [B,C,M,h,w]; the slope gradient sums over the whole tensor."""
    ops = support.ops()
    x = rnd(2, 4, 3, 6, 9, seed=60)
    w = torch.rand(4, generator=torch.Generator().manual_seed(61)) + 0.5
    b = rnd(4, seed=62)
    slope = torch.tensor([0.13])
    go = rnd(*x.shape, seed=63)
    xr, wr, br, sr = [t.double().requires_grad_() for t in (x, w, b, slope)]
    y_ref = F.prelu(F.instance_norm(xr, None, None, wr, br, True, 0.1, 1e-5), sr)
    gr = torch.autograd.grad(y_ref, (xr, wr, br, sr), go.double())
    xg, wg, bg, sg = [t.to(DEV).requires_grad_() for t in (x, w, b, slope)]
    y = ops.norm_act(xg, wg, bg, sg, mode=3, act=ops.ACT_PRELU)
    close(y, y_ref.detach(), 1e-5, 'in + prelu fwd')
    gg = torch.autograd.grad(y, (xg, wg, bg, sg), go.to(DEV))
    for a, r, nm in zip(gg, gr, ('dx', 'dw', 'db', 'dslope')):
        assert a.shape == r.shape
        close(a, r, 2e-4, 'in + prelu ' + nm)


def test_default_path_same_bits_through_new_and_old_entry_points(golden_dir):
    """M = 3 without fetch: dpf_shift_copies_* / dpf_cv_select_* return the bits the M = 3-only entry points they replaced returned.
    tests/golden/asm_default_path_bits.npz holds what those returned for these shapes and seeds, recorded on an MI355X from the library
    of commit 947c290 (the last one that had them)."""
    from dualpixelface_amd._lib import lib
    from dualpixelface_amd.ops import _ptr, _stream
    from dualpixelface_amd.sampler_tables import build_shift_tables
    rec = {k: torch.from_numpy(v).to(DEV) for k, v in np.load(golden_dir + '/asm_default_path_bits.npz').items()}
    B, C, h, w, L = 2, 5, 10, 13, 8
    iy, wy, ix, wx, iyi, ixi = (t.to(DEV) for t in build_shift_tables(h, w, -1.0))
    fea = rnd(B, C, h, w, seed=1).to(DEV)
    b_ = torch.empty(B, C, 3, h, w, device=DEV)
    lib().call('dpf_shift_copies_forward', _ptr(fea), _ptr(b_), _ptr(iy), _ptr(wy), _ptr(ix), _ptr(wx), B, C, 3, h, w, _stream())
    assert torch.equal(rec['shift_forward'], b_)
    g = rnd(B, C, 3, h, w, seed=2).to(DEV)
    db = torch.empty_like(fea)
    lib().call('dpf_shift_copies_backward_gather', _ptr(g), _ptr(db), _ptr(iyi), _ptr(wy), _ptr(ixi), _ptr(wx), B, C, 3, h, w, _stream())
    assert torch.equal(rec['shift_backward_gather'], db)
    x, s = rnd(B, C, 3, h, w, seed=3).to(DEV), torch.sigmoid(rnd(B, C, 3, h, w, seed=4)).to(DEV)
    vb = torch.zeros(B, 2 * C, L, h, w, device=DEV)
    lib().call('dpf_cv_select_forward', _ptr(x), _ptr(s), _ptr(vb), B, C, 3, h, w, 2 * C, L, C, 0xA5, 0, _stream())
    assert torch.equal(rec['cv_select_forward'], vb) and float(vb.abs().max()) > 0
    dv = rnd(B, 2 * C, L, h, w, seed=5).to(DEV)
    outs = [torch.empty_like(x) for _ in range(2)]
    lib().call('dpf_cv_select_backward', _ptr(x), _ptr(s), _ptr(dv), _ptr(outs[0]), _ptr(outs[1]), B, C, 3, h, w, 2 * C, L, C, 0xA5, 0,
               _stream())
    assert torch.equal(rec['cv_select_backward_dx'], outs[0]) and torch.equal(rec['cv_select_backward_ds'], outs[1])


# ------------------------------------------------------------------------------------------------ end to end against the reference
VARIANTS = ['v1_no_nearest', 'v2_phase_only', 'v3_relu_gate', 'v4_fetch', 'v5_no_nearest_relu_fetch_fix']
Q = 'cost_volume.attention_layer.mask_convs.1.'
GATE = 'cost_volume.attention_layer.activation.weight'


def _fixture(golden_dir, tag):
    from dualpixelface_amd.recipe import synthetic_batch
    g = np.load(golden_dir + '/e2e_asm_%s_32x48_b2.npz' % tag)
    over = json.loads(str(g['overrides']))
    if bool(g['fix_mode']):
        over['asm_grid_cache_compat'] = False
    B, H, W, seed = (int(v) for v in g['batch_args'])
    return g, over, synthetic_batch(B, H, W, seed=seed, mask_mode=str(g['mask_mode']), device=DEV)


@functools.lru_cache(maxsize=None)
def _step(golden_dir, tag):
    """ONE train step of the variant (forward, loss, backward, fused Adam step), shared by the checks below."""
    g, over, batch = _fixture(golden_dir, tag)
    model = build_model(True, **over)
    before = model.flat_parameters().clone()
    res = model.train_step(batch)
    taps = {k: v.detach().clone() for k, v in model.last_taps.items()}
    grads = {n: p.grad.detach().cpu().double() for n, p in model.named_parameters() if p.grad is not None}
    return g, model, {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in res.items()}, taps, grads, before


def _sampled(t, g, key, step, tol):
    s = g[key + '_s']
    assert tuple(t.shape) == tuple(int(v) for v in g[key + '_shape']), key
    lim = tol * float(g[key + '_max'])
    err = (t[:, :, :, ::2, ::step].cpu().double() - torch.from_numpy(s).double()).abs().max().item()
    assert err <= lim, '%s: max err %.3e > %.3e' % (key, err, lim)
    # the whole tensor through its fp64 checksums: a per-element error of `lim` moves sum and sum|.| by at most lim x numel
    t64 = t.double()
    cs = g[key + '_cs']
    assert abs(t64.sum().item() - cs[0]) <= lim * t.numel() and abs(t64.abs().sum().item() - cs[1]) <= lim * t.numel(), key


@pytest.mark.parametrize('tag', VARIANTS)
def test_variant_forward_losses_and_running_statistics(golden_dir, tag):
    g, model, res, taps, _, _ = _step(golden_dir, tag)
    _sampled(taps['volume'], g, 'volume', 3, 2e-4)
    _sampled(taps['out3'], g, 'out3', 2, 5e-4)
    close(res['pred_depth'], g['pred_depth'], None, 'pred_depth', atol=2e-3)
    close(res['pred_normal'], g['pred_normal'], None, 'pred_normal', atol=1e-3)
    for k in ('smoothL1_loss', 'cosine_loss', 'final_loss'):
        close(res[k], g[k], 1e-4, k)
    sd = model.state_dict()
    close(sd[Q + 'running_mean'], g['post::' + Q + 'running_mean'], 1e-4, 'attn rm')
    close(sd[Q + 'running_var'], g['post::' + Q + 'running_var'], 1e-4, 'attn rv')
    assert int(sd[Q + 'num_batches_tracked']) == 16 == int(g['post::' + Q + 'num_batches_tracked'])
    if bool(g['fix_mode']):
        assert not torch.equal(taps['volume'][:, :, 0], taps['volume'][:, :, 1])


@pytest.mark.parametrize('tag', VARIANTS)
def test_variant_gradients_within_the_references_own_noise(golden_dir, tag):
    g, _, _, _, grads, _ = _step(golden_dir, tag)
    names = [k[6:] for k in g.files if k.startswith('grad::')]
    assert len(names) >= 12 and ((GATE in names) == ('relu' in str(g['overrides'])))
    bad, zero = [], 0
    for n in names:
        ref = torch.from_numpy(g['grad::' + n]).double()
        mine = grads[n]
        if ref.norm().item() < 1e-6:                           # e.g. the mask convolutions behind a one-copy softmax (V2)
            zero += 1
            if not mine.norm().item() < 1e-6:
                bad.append((n, 'expected ~0', mine.norm().item()))
            continue
        noise = float(g['noise::' + n])
        rel = ((mine - ref).norm() / ref.norm()).item()
        budget = max(K_SPREAD * noise, GRAD_FLOOR)
        print('%s %s: rel L2 %.3e (budget %.3e, reference fp32 noise %.3e)' % (tag, n, rel, budget, noise))
        if rel > budget:
            bad.append((n, rel, budget))
    assert not bad, bad
    assert zero == (6 if tag == 'v2_phase_only' else 0), zero


def test_v5_deterministic_mode_two_steps_equal_bits(golden_dir):
    ops = support.ops()
    g, over, batch = _fixture(golden_dir, 'v5_no_nearest_relu_fetch_fix')
    runs = []
    with ops.deterministic_mode():
        for _ in range(2):
            model = build_model(True, **over)
            res = model.train_step(batch)
            runs.append((res['final_loss'].detach().clone(), model.last_taps['volume'].detach().clone(),
                         {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None},
                         model.flat_parameters().detach().clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    diff = [n for n in runs[0][2] if not torch.equal(runs[0][2][n], runs[1][2][n])]
    assert not diff, diff[:10]
    assert torch.equal(runs[0][3], runs[1][3])


def test_v3_gate_slope_trains_and_survives_a_checkpoint(golden_dir, tmp_path):
    from dualpixelface_amd import load_option
    from dualpixelface_amd.plugin import STEREODPNET
    from dualpixelface_amd.recipe import recipe_tensor
    from dualpixelface_amd.trainer import Trainer
    g, model, _, _, grads, before = _step(golden_dir, 'v3_relu_gate')
    sd = model.state_dict()
    start = recipe_tensor(GATE, sd[GATE].cpu())
    assert model.flat_parameters().numel() == 3670493 == before.numel()
    assert grads[GATE].abs().item() > 0
    moved = (sd[GATE].cpu() - start).item()
    # one Adam step (lr 1e-4) moves a parameter with a non-zero gradient by ~lr against the gradient's sign
    assert 0.5e-4 <= abs(moved) <= 1.5e-4 and moved * grads[GATE].item() < 0, (moved, grads[GATE].item())
    opt = load_option(asm_activation='relu')
    trainer = Trainer(opt, str(tmp_path), rank=0, world_size=1)
    path = trainer.save_checkpoint(model)
    other = STEREODPNET(opt).to(DEV)
    Trainer(opt, str(tmp_path), rank=0, world_size=1).load_checkpoint(other, path)
    assert torch.equal(other.state_dict()[GATE], sd[GATE]) and torch.equal(other.flat_parameters(), model.flat_parameters())
    assert other._adam['step'] == model._adam['step'] and torch.equal(other._adam['m'], model._adam['m'])
