"""The dual-pixel renderer on the GPU (run with ``-m gpu``): csrc/dp_render.hip through ops.dp_render, against the numpy restatement of
tests/dp_render_cpu.py, and the rendered batches of dualpixelface_amd/synthetic_dp.py through the photometric loss and a DPNet train step.

Shapes, those of tests/test_gpu_refocus.py (the two-plane scene of dualpixelface_amd/synthetic_refocus.py with a ripple on d, so that r
varies from pixel to pixel).  'tiny' 1 x 5 x 7 at max_radius 8: the window is larger than the image.  'ragged' 2 x 37 x 53 at 16 under the
diagonal shift (1, 1): partial tiles on both axes, NaN holes and a different d field per sample.  'wide' 1 x 70 x 131 at 32: rho |d|
beyond 32 on the far plane, so the clamp counts in the stats, and a halo wider than a tile.  'spill' 1 x 48 x 80 at 16: the far plane fills
the tile columns 0 and 1 exactly in focus (d = 0), the blurred NEAR plane starts at column 32 -- the sharp tiles receive from it, and a
window bound taken from the receivers' own radii would return them unchanged.

Bars.  radius and dp_stats: bit for bit against the fp32 restatement.  Both views: against the fp64 restatement evaluated on the device's
radius plane, within 2 x the fp32 restatement's own largest distance from the fp64 one + 2^-22; the test computes that bar and asserts it
is below 1e-4.  The identities (d = 0, the holes, the two swaps, a sample apart from its batch, repeats and replays): bit for bit.
Agreement: the photometric term at the true d under the rendering's own shift is the smallest of the nine candidates and at most 1 / 1.5
of the next.  Measured on an MI355X (largest |device - fp64| / bar, reference and target view): tiny 0.38 / 0.38 (gamma 1) and 0.31 / 0.30
(gamma 2.2), ragged 0.42 / 0.40 and 0.33 / 0.41 (the two samples), wide 0.45 / 0.41, spill 0.44 / 0.43; in absolute terms at most 1.26e-6
(spill, target), against bars between 8.7e-7 and 2.9e-6.  The constant image: 8.9e-8 (bars 3.6e-7 / 4.2e-7).  Agreement on the device
pair: 0.0053 at the true shift against 0.096 at the next smallest candidate, a ratio of 18.3."""
import functools

import numpy as np
import pytest
import torch

from dualpixelface_amd import synthetic_refocus as syn
from tests import dp_render_cpu as dc
from tests import support
from tests.support import DEV
from tests.dp_render_cpu import FACTOR, TRUE_SHIFT, check_agreement, nine_terms

pytestmark = pytest.mark.gpu

# name -> (B, H, W, max_radius, shift, scene settings per sample)
CASES = {
    'tiny': (1, 5, 7, 8, (0.0, -2.0), (dict(d_near=3.0, d_far=-2.0, holes=0.1, seed=1),)),
    'ragged': (2, 37, 53, 16, (1.0, 1.0), (dict(d_near=6.0, d_far=-4.0, holes=0.05, seed=2),
                                           dict(box=(0, 20, 30, 53), d_near=2.5, d_far=-8.0, holes=0.1, seed=3))),
    'wide': (1, 70, 131, 32, (0.0, -2.0), (dict(d_near=3.0, d_far=-15.0, holes=0.02, seed=4),)),
    'spill': (1, 48, 80, 16, (0.0, -2.0), (dict(box=(0, 48, 32, 80), d_near=5.0, d_far=0.0, seed=5),)),
}


@functools.lru_cache(maxsize=None)
def scene(name):
    """The batch of a case as numpy arrays; d carries a ripple of +-0.35 (on the near plane only in 'spill', whose far plane stays at 0)."""
    B, H, W, _, _, per = CASES[name]
    ones = [syn.scene(H, W, **kw) for kw in per]
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    ripple = (0.35 * np.sin(0.9 * xs + 0.4 * ys)).astype(np.float32)
    for s in ones:
        s['disparity'] = (s['disparity'] + ripple * (s['near'] if name == 'spill' else 1)).astype(np.float32)
    return {k: np.stack([s[k] for s in ones]) for k in ('view', 'disparity')}


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _render(name, **kw):
    b = scene(name)
    kw = dict(dict(max_radius=CASES[name][3], shift=CASES[name][4]), **kw)
    return support.ops().dp_render(support.tensor(b['view']), support.tensor(b['disparity']), **kw)


@functools.lru_cache(maxsize=None)
def device(name, gamma=2.2, near_sign=1):
    """ops.dp_render on a case -> numpy arrays (computed once, shared, never changed)."""
    return _np(_render(name, gamma=gamma, near_sign=near_sign))


@functools.lru_cache(maxsize=None)
def reference(name, gamma):
    """Per sample and view (the fp64 restatement on the device's radius plane, the bar 2 max |fp32 - fp64| + 2^-22)."""
    b, got = scene(name), device(name, gamma)
    _, _, _, R, shift, _ = CASES[name]
    out = []
    for s in range(CASES[name][0]):
        r64, r32 = (dc.render(b['view'][s], b['disparity'][s], got['radius'][s], shift, 1, R, gamma, dtype=t) for t in (np.float64, np.float32))
        out.append([(r64[v], 2.0 * float(np.abs(r32[v].astype(np.float64) - r64[v]).max()) + 2.0 ** -22) for v in range(2)])
    return out


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- 1. the plan
@pytest.mark.parametrize('name', ('tiny', 'ragged', 'wide'))
def test_radius_and_stats_bit_for_bit(name):
    B, H, W, R, shift, _ = CASES[name]
    b, got = scene(name), device(name)
    assert got['radius'].shape == (B, H, W) and got['radius'].dtype == np.float32
    assert got['dp_stats'].shape == (B, 8) and got['dp_stats'].dtype == np.float64
    assert got['reference'].shape == got['target'].shape == (B, 3, H, W) and got['reference'].dtype == got['target'].dtype == np.float32
    for s in range(B):
        d = b['disparity'][s]
        c, clamped = dc.radius(d, dc.radius_scale(shift), R)
        assert np.array_equal(support.bits(got['radius'][s]), support.bits(c)), (name, s)
        assert got['dp_stats'][s].tolist() == dc.stats(d, c, clamped).tolist()
        assert np.abs(c).max() > 2 and (c[~np.isfinite(d)] == 0).all() and not np.isfinite(d).all() and c.min() < 0 < c.max()
        assert (clamped.sum() > 100 and np.abs(c).max() == R) if name == 'wide' else not clamped.any()


# ---- 2. the render
@pytest.mark.parametrize('name,gamma', [('tiny', 1.0), ('tiny', 2.2), ('ragged', 2.2), ('wide', 2.2), ('spill', 1.0)])
def test_both_views_against_the_restatement(name, gamma):
    b, got = scene(name), device(name, gamma)
    for s, views in enumerate(reference(name, gamma)):
        hole = ~np.isfinite(b['disparity'][s])
        for key, (want, bar) in zip(('reference', 'target'), views):
            err = float(np.abs(got[key][s].astype(np.float64) - want).max())
            moved = float((got[key][s] != b['view'][s]).mean())
            print('%s %s sample %d gamma %.1f: max |dev - fp64| %.3e, bar %.3e (ratio %.3f), %.2f of the values moved'
                  % (key, name, s, gamma, err, bar, err / bar, moved))
            assert bar < 1e-4
            assert err <= bar
            assert moved > 0.3
            assert np.array_equal(support.bits(got[key][s][:, hole]), support.bits(b['view'][s][:, hole]))       # copied through
        assert not np.array_equal(got['reference'][s], got['target'][s])


def test_sharp_tiles_receive_from_the_blurred_near_plane_beside_them():
    b, got = scene('spill'), device('spill', 1.0)
    c, v = got['radius'][0], b['view'][0]
    assert not c[:, :32].any() and c[:, 32:].min() > 8                      # two tile columns exactly in focus, the near plane blurred
    reach = int(np.ceil(c[:, 32:].max()))
    for key in ('reference', 'target'):
        changed = (got[key][0] != v).any(0)
        assert changed[:, 32 - 4:32].all() and not changed[:, :32 - reach - 1].any() and 9 <= reach <= 13
    # under the other sign the near plane is behind the sharp one and may not spread over it
    other = device('spill', 1.0, -1)
    for key in ('reference', 'target'):
        assert np.array_equal(support.bits(other[key][0][:, :, :32]), support.bits(v[:, :, :32]))


def test_no_defocus_and_the_dead_zone_return_the_image():
    ops = support.ops()
    for name in ('tiny', 'ragged'):
        b = scene(name)
        view = support.tensor(b['view'])
        for d in (np.where(np.isfinite(b['disparity']), np.float32(0), b['disparity']), np.full_like(b['disparity'], 0.2)):
            for gamma in (1.0, 2.2):
                out = ops.dp_render(view, support.tensor(d), max_radius=CASES[name][3], shift=CASES[name][4], gamma=gamma)
                assert not bool(out['radius'].any()) and bool((out['dp_stats'][:, 1:] == 0).all())
                assert _same_bits(out['reference'], view) and _same_bits(out['target'], view)
    enc = support.tensor(dc.encoded(b['view']))                                # an encoded image in, an encoded image out
    out = ops.dp_render(enc, support.tensor(d), normalised=False, output='encoded')
    assert _same_bits(out['reference'], enc) and _same_bits(out['target'], enc)
    out = ops.dp_render(view, support.tensor(d), output='encoded')             # the other form: the clamped encoded value
    assert _same_bits(out['reference'], enc) and _same_bits(out['target'], enc)


@pytest.mark.parametrize('name', ('tiny', 'ragged', 'wide'))
def test_the_two_swaps_bit_for_bit(name):
    b = scene(name)
    shift = CASES[name][4]
    one = _render(name)
    neg = _render(name, shift=(-shift[0], -shift[1]))
    assert _same_bits(neg['reference'], one['target']) and _same_bits(neg['target'], one['reference']) and _same_bits(neg['radius'], one['radius'])
    flip = support.ops().dp_render(support.tensor(b['view']), support.tensor(-b['disparity']), max_radius=CASES[name][3], shift=shift, near_sign=-1)
    assert _same_bits(flip['reference'], one['target']) and _same_bits(flip['target'], one['reference'])
    assert _same_bits(flip['radius'], -one['radius'] + 0.0) and not _same_bits(one['reference'], one['target'])
    assert flip['dp_stats'][:, :2].tolist() == one['dp_stats'][:, :2].tolist()
    assert flip['dp_stats'][:, 2].tolist() == (-one['dp_stats'][:, 3]).tolist() and flip['dp_stats'][:, 3].tolist() == (-one['dp_stats'][:, 2]).tolist()


def test_a_sample_does_not_depend_on_its_batch():
    ops = support.ops()
    b = scene('ragged')
    both = _render('ragged')
    for s in range(2):
        alone = ops.dp_render(support.tensor(b['view'][s:s + 1]), support.tensor(b['disparity'][s:s + 1]), max_radius=16, shift=(1.0, 1.0))
        assert all(_same_bits(alone[k][0], both[k][s]) for k in both), s


def test_a_constant_image_stays_constant():
    H, W, R = 37, 53, 16
    view = syn.scene(H, W, constant=0.4)['view'][None]
    d = (np.random.RandomState(7).randn(1, H, W) * 3).astype(np.float32)
    d[0, 5, 5:9] = np.nan
    got = _np(support.ops().dp_render(support.tensor(view), support.tensor(d), max_radius=R, output='encoded'))
    v = dc.encoded(view[0]).astype(np.float64)
    r64, r32 = (dc.render(view[0], d[0], got['radius'][0], max_radius=R, dtype=t, output='encoded') for t in (np.float64, np.float32))
    for k, key in enumerate(('reference', 'target')):
        bar = 2.0 * float(np.abs(r32[k].astype(np.float64) - r64[k]).max()) + 2.0 ** -22
        err = float(np.abs(got[key][0].astype(np.float64) - v).max())
        print('constant image, %s: max |dev - v| %.3e, bar %.3e' % (key, err, bar))
        assert np.ptp(got['radius']) > R and np.abs(r64[k] - v).max() <= 1e-12 and bar < 1e-4 and err <= bar


# ---- 3. the same bits every time, eager or replayed
def test_repeats_bit_for_bit_whatever_the_workspace_holds():
    ops = support.ops()
    first = _render('wide')
    mine = [buf for key, buf in ops._scratch.items() if key[1] == 'dp_render']
    assert mine
    for fill in (float('nan'), 1e30):
        for buf in mine:
            buf.fill_(fill)
        again = _render('wide')
        assert all(_same_bits(first[k], again[k]) for k in first)


def test_calls_replay_from_a_graph():
    ops = support.ops()
    b = scene('ragged')
    d = {k: support.tensor(v) for k, v in b.items()}
    other = {'view': d['view'].flip(0).contiguous(), 'disparity': (d['disparity'] * 0.5).flip(0).contiguous()}

    def run(x):
        return ops.dp_render(x['view'], x['disparity'], shift=(1.0, 1.0))
    eager, want = run(d), run(other)
    assert not torch.equal(eager['reference'], want['reference'])
    st = {k: v.clone() for k, v in d.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                 # the side stream's scratch exists before the capture
        run(st)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):                    # one stream, no fork
        out = run(st)
    for src, w in ((other, want), (d, eager)):
        for k in st:
            st[k].copy_(src[k])
        graph.replay()
        torch.cuda.synchronize()
        assert all(_same_bits(out[k], w[k]) for k in out)


# ---- 4. refusals
def test_abi_refusals_launch_nothing():
    ops = support.ops()
    L = ops.lib()
    b = scene('tiny')
    view, disp = support.tensor(b['view']), support.tensor(b['disparity'])
    B, H, W = 1, 5, 7
    nbytes = L.call('dpf_dp_render_workspace_bytes', B, H, W)
    assert nbytes > 0 and nbytes % 8 == 0
    ws = torch.zeros(nbytes // 8 + 2, dtype=torch.float64, device=DEV)
    radius = torch.full((B, H, W), 7.0, device=DEV)
    stats = torch.full((B, 8), 7.0, dtype=torch.float64, device=DEV)
    ref, tgt = torch.full((B, 3, H, W), 7.0, device=DEV), torch.full((B, 3, H, W), 7.0, device=DEV)
    norm = ops._normalizer_floats()
    p, st = support.ptr, support.stream()
    rho = dc.radius_scale((0.0, -2.0))

    def plan(**kw):
        a = dict(disparity=p(disp), B=B, H=H, W=W, rho=rho, radius=8, ws=p(ws), nbytes=nbytes, out=p(radius), stats=p(stats))
        a.update(kw)
        return L.cdll.dpf_dp_render_plan(*a.values(), st)

    def render(**kw):
        a = dict(image=p(view), normalised=1, norm=norm, disparity=p(disp), c=p(radius), B=B, H=H, W=W, sx=0.0, sy=-2.0, radius=8, sign=1, gamma=2.2,
                 out_norm=1, ws=p(ws), nbytes=nbytes, ref=p(ref), tgt=p(tgt))
        a.update(kw)
        return L.cdll.dpf_dp_render(*a.values(), st)
    for kw in (dict(disparity=None), dict(out=None), dict(stats=None), dict(B=0), dict(H=0), dict(W=-1), dict(rho=-1.0), dict(rho=float('nan')),
               dict(rho=float('inf')), dict(radius=0), dict(radius=33), dict(ws=None), dict(nbytes=nbytes - 8), dict(ws=support.offset_ptr(ws, 4))):
        assert plan(**kw) == -1, kw
    for kw in (dict(image=None), dict(norm=None), dict(disparity=None), dict(c=None), dict(ref=None), dict(tgt=None), dict(B=0), dict(sx=0.0, sy=0.0),
               dict(sx=float('nan')), dict(sy=float('inf')), dict(radius=0), dict(radius=33), dict(sign=0), dict(sign=2), dict(gamma=0.0),
               dict(gamma=float('nan')), dict(ws=None), dict(nbytes=nbytes - 8), dict(ws=support.offset_ptr(ws, 4))):
        assert render(**kw) == -1, kw
    assert plan(B=65536) == -3 and render(B=65536) == -3
    q = L.cdll.dpf_dp_render_workspace_bytes
    for shape in ((0, 8, 12), (1, 0, 12), (1, 8, 0), (65536, 8, 12), (1, 1 << 16, 1 << 15)):
        assert q(*shape) == -1, shape
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in (radius, stats, ref, tgt)) and not bool(ws.any())
    assert plan() == 0 and render() == 0                               # and the same arguments, unbroken, run
    torch.cuda.synchronize()
    got = device('tiny')
    assert np.array_equal(support.bits(ref.cpu().numpy()), support.bits(got['reference']))
    assert np.array_equal(support.bits(tgt.cpu().numpy()), support.bits(got['target'])) and np.array_equal(stats.cpu().numpy(), got['dp_stats'])


def test_ops_refuse_what_does_not_fit():
    from dualpixelface_amd._lib import DpfError
    ops = support.ops()
    b = scene('tiny')
    view, disp = support.tensor(b['view']), support.tensor(b['disparity'])
    for kw, match in ((dict(max_radius=0), 'max_radius'), (dict(max_radius=33), 'max_radius'), (dict(max_radius=8.5), 'max_radius'),
                      (dict(max_radius=True), 'max_radius'), (dict(near_sign=0), 'near_sign'), (dict(near_sign='auto'), 'near_sign'),
                      (dict(shift=(0, 0)), 'shift'), (dict(shift=(1, float('nan'))), 'shift'), (dict(shift=3), 'shift'), (dict(output='linear'), 'output'),
                      (dict(radius_scale=-1.0), 'DPF_ERR_INVALID_ARG'), (dict(gamma=0.0), 'DPF_ERR_INVALID_ARG')):
        with pytest.raises(DpfError, match=match):
            ops.dp_render(view, disp, **kw)
    for bad_view, bad_disp, match in ((view[:, :2], disp, 'image'), (view, disp[:, :4], 'disparity'), (view, disp.unsqueeze(1), 'disparity'),
                                      (view.cpu(), disp, 'GPU'), (view, disp.half(), 'dtype'), (view.double(), disp, 'dtype')):
        with pytest.raises(DpfError, match=match):
            ops.dp_render(bad_view, bad_disp)
    got = ops.dp_render(view.clone().requires_grad_(), disp.clone().requires_grad_(), max_radius=8)
    want = _render('tiny')
    assert all(not got[k].requires_grad and _same_bits(got[k], want[k]) for k in want)


# ---- 5. what the pair is for
@functools.lru_cache(maxsize=None)
def face_batch():
    from dualpixelface_amd import synthetic_dp
    return synthetic_dp.rendered_batch(2, 64, 96, seed=3, device=DEV)


def test_the_rendered_batch_has_the_keys_of_the_noise_batch():
    from dualpixelface_amd import synthetic_dp
    from dualpixelface_amd.config import Option
    noise = support.batch(2, 64, 96, seed=3)
    batch = face_batch()
    assert list(batch) == list(noise) + ['center']
    for k in noise:
        assert batch[k].shape == noise[k].shape and batch[k].dtype == noise[k].dtype and batch[k].device == noise[k].device, k
    assert batch['center'].shape == (2, 3, 64, 96) and not torch.equal(batch['left'], batch['right'])
    assert float((batch['abvalue'][:, 1:2, None] / batch['depth'] + batch['abvalue'][:, 0:1, None] - batch['disp']).abs().max()) < 1e-3
    want = support.ops().dp_render(batch['center'], batch['disp'])
    assert _same_bits(batch['left'], want['reference']) and _same_bits(batch['right'], want['target'])
    flipped = synthetic_dp.rendered_batch(2, 64, 96, seed=3, option=Option({'dataset': Option({'flip_lr': True})}), device=DEV)
    assert _same_bits(flipped['right'], want['reference']) and _same_bits(flipped['left'], want['target'])
    loader = synthetic_dp.rendered_loader(3, 64, 96, 2, seed=3, device=DEV)
    got = list(loader)
    assert len(loader) == 2 and [g['left'].shape[0] for g in got] == [2, 1] and all(_same_bits(got[0][k], batch[k]) for k in batch)


def test_the_photometric_loss_prefers_the_true_shift_on_the_device_pair():
    ops = support.ops()
    batch = face_batch()
    ref, tgt, pred = batch['left'][:1], batch['right'][:1], batch['disp'][:1, None]

    def term(shift, scale):
        return float(ops.photometric_loss((pred * scale).contiguous(), ref, tgt, shift=shift))
    check_agreement(nine_terms(term), 'device pair, 64 x 96 face scene')
    for scale in (0.5, 1.5):
        assert term(TRUE_SHIFT, scale) > FACTOR * term(TRUE_SHIFT, 1.0)


def test_a_rendered_batch_feeds_a_captured_dpnet_train_step(monkeypatch):
    ops = support.ops()
    batch = face_batch()
    with ops.deterministic_mode():
        monkeypatch.setenv('DPF_STEP_GRAPH', '1')
        model = support.dpnet('train_faceDP_dpnet_rendered')
        steps = support.loss_steps(model, batch, 4)                   # two warm-up steps, the capture, one replay
        assert model._graph_state.get('graph') is not None and not model._graph_state.get('failed')
    assert all(np.isfinite(s['final_loss']) and s['final_loss'] > 0 for s in steps), steps
