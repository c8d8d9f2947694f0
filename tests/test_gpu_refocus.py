"""The refocus block on the GPU (run with ``-m gpu``): csrc/refocus.hip through ops.refocus, and the ``refocus`` block through the plugins'
evaluation forward, against the numpy restatement of tests/refocus_cpu.py on the two-plane scene of dualpixelface_amd/synthetic_refocus.py
(a ripple is added to d so that r varies from pixel to pixel).

Shapes.  1 x 5 x 7 at max_radius 8: the image is smaller than the window, so every clip path runs.  2 x 37 x 53 at 16: ragged, a different
plane, mask, focus and NaN holes per sample.  1 x 70 x 131 at 32: several tiles in both directions and a halo wider than a tile.
1 x 48 x 80 at 16 ('spill'): the far plane fills the tile columns 0 and 1 and is exactly in focus (r = 0 in every one of its pixels), the
blurred NEAR plane starts at column 32 -- the sharp tiles receive from it, and a window bound taken from the receivers' own radii would
return them unchanged.

Bars.  defocus and the stats of focus 'value' and 'point': bit for bit against the fp32 restatement.  'mask_mean': d_f within
N 2^-53 + 2^-24 relative of the fp64 mean.  refocused: against the fp64 restatement evaluated on the device's defocus plane, within
2 x the fp32 restatement's own largest distance from the fp64 one + 2^-22; the test computes that bar and asserts it is below 1e-4 (an
8-bit step is 3.9e-3).  Measured on an MI355X (largest |device - fp64| / bar):
tiny 0.33 (gamma 1) and 0.18 (gamma 2.2), ragged 0.10 and 0.10, wide 0.018 and 0.018, spill 0.16 and 0.13; in absolute terms at most
3.5e-7 (wide, gamma 1, where the bar is 1.9e-5), against bars between 4.4e-7 (tiny) and 1.9e-5.  The constant image: 2.1e-7 (bar 1.8e-6)
at gamma 1, 8.9e-8 (bar 8.9e-7) at gamma 2.2.  mask_mean: d_f equal to the fp64 mean to the last bit on both samples."""
import functools

import numpy as np
import pytest
import torch

from dualpixelface_amd import synthetic_refocus as syn
from tests import refocus_cpu as rc
from tests import support
from tests.support import DEV

pytestmark = pytest.mark.gpu

# name -> (B, H, W, max_radius, focus, scene settings per sample)
CASES = {
    'tiny': (1, 5, 7, 8, dict(focus='point', focus_point=(0.7, 0.2)), (dict(holes=0.1, seed=1),)),
    'ragged': (2, 37, 53, 16, dict(focus='mask_mean'), (dict(holes=0.05, seed=2), dict(box=(0, 20, 30, 53), d_near=0.8, d_far=-1.2, holes=0.1, seed=3))),
    'wide': (1, 70, 131, 32, dict(focus='value', focus_value=0.25), (dict(d_near=3.0, d_far=-7.4, holes=0.02, seed=4),)),
    'spill': (1, 48, 80, 16, dict(focus='value', focus_value=-1.0), (dict(box=(0, 48, 32, 80), d_near=1.5, d_far=-1.0, seed=5),)),
}
RENDERED = ('tiny', 'ragged', 'wide', 'spill')
GAMMAS = (1.0, 2.2)


@functools.lru_cache(maxsize=None)
def scene(name):
    """The batch of a case as numpy arrays; d carries a ripple of +-0.35 (on the near plane only in 'spill', whose far plane stays exact)."""
    B, H, W, _, _, per = CASES[name]
    ones = [syn.scene(H, W, **kw) for kw in per]
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    ripple = (0.35 * np.sin(0.9 * xs + 0.4 * ys)).astype(np.float32)
    for s in ones:
        s['disparity'] = (s['disparity'] + ripple * (s['near'] if name == 'spill' else 1)).astype(np.float32)
    return {k: np.stack([s[k] for s in ones]) for k in ('view', 'disparity', 'mask', 'near')}


def _dev(b):
    return {k: support.tensor(v) for k, v in b.items() if k != 'near'}


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def device(name, gamma=2.2, **kw):
    """ops.refocus on a case under its own focus -> numpy arrays (computed once, shared, never changed)."""
    d = _dev(scene(name))
    kw = dict(CASES[name][4], **kw)
    return _np(support.ops().refocus(d['view'], d['disparity'], mask=d['mask'], max_radius=CASES[name][3], gamma=gamma, **kw))


@functools.lru_cache(maxsize=None)
def reference(name, gamma):
    """Per sample (the fp64 restatement on the device's defocus plane, the bar 2 max |fp32 - fp64| + 2^-22)."""
    b, got = scene(name), device(name, gamma)
    out = []
    for s in range(CASES[name][0]):
        sign = int(got['refocus_stats'][s, 3])
        r64, r32 = (rc.render(b['view'][s], b['disparity'][s], got['defocus'][s], sign, CASES[name][3], gamma, dtype=t) for t in (np.float64, np.float32))
        out.append((r64, 2.0 * float(np.abs(r32.astype(np.float64) - r64).max()) + 2.0 ** -22))
    return out


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- 1. the plan: defocus and stats
@pytest.mark.parametrize('mode', ('value', 'point'))
@pytest.mark.parametrize('name', ('tiny', 'ragged', 'wide'))
def test_defocus_and_stats_bit_for_bit(name, mode):
    B, H, W, R = CASES[name][:4]
    b = scene(name)
    kw = dict(focus='value', focus_value=0.3) if mode == 'value' else dict(focus='point', focus_point=(0.7, 0.2))
    got = device(name, **kw)
    assert got['defocus'].shape == (B, H, W) and got['defocus'].dtype == np.float32 and got['refocus_stats'].shape == (B, 8)
    assert got['refocused'].shape == (B, 3, H, W) and got['refocus_stats'].dtype == np.float64
    for s in range(B):
        d_f, n, flag = rc.focus(b['disparity'][s], b['mask'][s], mode, (0.7, 0.2), 0.3)
        c = rc.defocus(b['disparity'][s], d_f, 4.0, R)
        assert flag == 1 and np.array_equal(support.bits(got['defocus'][s]), support.bits(c)), (name, s)
        assert got['refocus_stats'][s].tolist() == [d_f, n, flag, 1.0, float(c.min()), float(c.max()), 0.0, 0.0]
        assert np.abs(c).max() > 2 and (c[~np.isfinite(b['disparity'][s])] == 0).all() and not np.isfinite(b['disparity'][s]).all()


def test_a_point_on_a_hole_is_flagged():
    b = scene('ragged')
    ys, xs = np.nonzero(~np.isfinite(b['disparity'][1]))
    point = ((xs[0] + 0.5) / 53.0, (ys[0] + 0.5) / 37.0)
    got = device('ragged', focus='point', focus_point=point)
    finite0 = bool(np.isfinite(b['disparity'][0, ys[0], xs[0]]))
    assert got['refocus_stats'][1, :3].tolist() == [0.0, 0.0, 0.0] and got['refocus_stats'][0, 2] == float(finite0)
    assert np.array_equal(support.bits(got['defocus'][1]), support.bits(rc.defocus(b['disparity'][1], 0.0, 4.0, 16)))


def test_the_mask_mean_focus():
    b = scene('ragged')
    got = device('ragged')
    for s in range(2):
        d_f, n, flag = rc.focus(b['disparity'][s], b['mask'][s])
        err, bar = abs(got['refocus_stats'][s, 0] - d_f), (n * 2.0 ** -53 + 2.0 ** -24) * abs(d_f)
        print('mask_mean sample %d: N %d, d_f %.9f, |dev - np| %.3e (bar %.3e)' % (s, n, d_f, err, bar))
        assert 100 < n < 37 * 53 and err <= bar and got['refocus_stats'][s, 1:4].tolist() == [n, 1.0, 1.0]
        c = rc.defocus(b['disparity'][s], got['refocus_stats'][s, 0], 4.0, 16)       # from the device's own focus: bit for bit again
        assert np.array_equal(support.bits(got['defocus'][s]), support.bits(c))
        assert got['refocus_stats'][s, 4:6].tolist() == [float(c.min()), float(c.max())]
    d = _dev(b)
    d['mask'][1] = 0                                                                  # nothing counted: d_f = 0 and the flag is down
    none = _np(support.ops().refocus(d['view'], d['disparity'], mask=d['mask']))
    assert none['refocus_stats'][1, :3].tolist() == [0.0, 0.0, 0.0] and np.array_equal(none['refocus_stats'][0], got['refocus_stats'][0])
    assert np.array_equal(support.bits(none['refocused'][0]), support.bits(got['refocused'][0]))      # a sample does not depend on its batch
    every = _np(support.ops().refocus(d['view'], d['disparity']))                     # no mask: every finite pixel
    for s in range(2):
        d_f, n, _ = rc.focus(b['disparity'][s], None)
        assert every['refocus_stats'][s, 1] == n and abs(every['refocus_stats'][s, 0] - d_f) <= (n * 2.0 ** -53 + 2.0 ** -24) * abs(d_f)


def test_the_depth_targets_and_the_near_sign():
    ops = support.ops()
    b = scene('ragged')
    d = _dev(b)
    ab = np.array([[0.5, 2.0], [-0.25, -3.0]], np.float32)
    with np.errstate(all='ignore'):
        z = (ab[:, 1, None, None] / (b['disparity'] - ab[:, 0, None, None])).astype(np.float32)
    z[0, 3, 4] = 0.0                                                                  # a / 0: not finite, not renderable
    kw = dict(mask=d['mask'], ab=support.tensor(ab), focus='value', focus_value=0.1)
    depth = _np(ops.refocus(d['view'], support.tensor(z), target_type='depth', **kw))
    idepth = _np(ops.refocus(d['view'], d['disparity'], target_type='idepth', **kw))
    disp = _np(ops.refocus(d['view'], d['disparity'], **kw))
    plain = _np(ops.refocus(d['view'], d['disparity'], mask=d['mask'], focus='value', focus_value=0.1))
    for s in range(2):
        c = rc.defocus(rc.disparity(z[s], ab[s], 'depth'), 0.1, 4.0, 16)
        assert np.array_equal(support.bits(depth['defocus'][s]), support.bits(c)) and (s or c[3, 4] == 0)
        assert depth['refocus_stats'][s, 3] == idepth['refocus_stats'][s, 3] == disp['refocus_stats'][s, 3] == (1.0, -1.0)[s]
        assert plain['refocus_stats'][s, 3] == 1.0
    assert all(np.array_equal(support.bits(idepth[k]), support.bits(disp[k])) for k in ('refocused', 'defocus'))
    assert np.array_equal(support.bits(plain['refocused'][0]), support.bits(disp['refocused'][0]))
    forced = _np(ops.refocus(d['view'], d['disparity'], near_sign=-1, **kw))
    assert np.array_equal(support.bits(forced['refocused'][1]), support.bits(disp['refocused'][1]))
    assert not np.array_equal(forced['refocused'][0], disp['refocused'][0]) and forced['refocus_stats'][0, 3] == -1.0


# ---- 2. the render
@pytest.mark.parametrize('gamma', GAMMAS)
@pytest.mark.parametrize('name', RENDERED)
def test_refocused_against_the_restatement(name, gamma):
    b, got = scene(name), device(name, gamma)
    for s, (want, bar) in enumerate(reference(name, gamma)):
        v = rc.encoded(b['view'][s])
        err = float(np.abs(got['refocused'][s].astype(np.float64) - want).max())
        moved = float((got['refocused'][s] != v).mean())
        print('refocused %s sample %d gamma %.1f: max |dev - fp64| %.3e, bar %.3e (ratio %.3f), %.2f of the values moved'
              % (name, s, gamma, err, bar, err / bar, moved))
        assert bar < 1e-4
        assert err <= bar
        assert moved > 0.3 and got['refocused'][s].min() >= 0 and got['refocused'][s].max() <= 1
        hole = ~np.isfinite(b['disparity'][s])
        assert np.array_equal(support.bits(got['refocused'][s][:, hole]), support.bits(v[:, hole]))       # copied through


def test_sharp_tiles_receive_from_the_blurred_near_plane_beside_them():
    b, got = scene('spill'), device('spill', 1.0)
    c, out, v = got['defocus'][0], got['refocused'][0], rc.encoded(b['view'][0])
    assert not c[:, :32].any() and c[:, 32:].min() > 8                      # two tile columns exactly in focus, the near plane blurred
    assert got['refocus_stats'][0].tolist()[:4] == [-1.0, 0.0, 1.0, 1.0]
    reach = int(np.ceil(c[:, 32:].max()))
    changed = (out != v).any(0)
    assert changed[:, 32 - 8:32].all() and not changed[:, :32 - reach - 1].any() and 9 <= reach <= 12
    assert (out[:, :, 24:32] > v[:, :, 24:32]).all()                        # what arrives is the brighter plane
    want, bar = reference('spill', 1.0)[0]
    assert np.abs(out[:, :, :32].astype(np.float64) - want[:, :, :32]).max() <= bar
    # under the other sign the near plane is behind the sharp one and may not spread over it
    other = device('spill', 1.0, near_sign=-1)
    assert np.array_equal(support.bits(other['refocused'][0][:, :, :32]), support.bits(v[:, :, :32]))


def test_no_blur_returns_the_view():
    ops = support.ops()
    for name in ('tiny', 'ragged'):
        b, d = scene(name), _dev(scene(name))
        for gamma in GAMMAS:
            out = _np(ops.refocus(d['view'], d['disparity'], mask=d['mask'], aperture=0.0, max_radius=CASES[name][3], gamma=gamma))
            assert not out['defocus'].any() and (out['refocus_stats'][:, 4:6] == 0).all()
            for s in range(CASES[name][0]):
                ulps = np.abs(support.bits(out['refocused'][s]).astype(np.int64) - support.bits(rc.encoded(b['view'][s])).astype(np.int64))
                assert ulps.max() <= 1, (name, gamma, ulps.max())
    flat = torch.full_like(d['disparity'], 0.75)                              # a flat scene focused on itself
    out = ops.refocus(d['view'], flat, focus='point')
    assert not bool(out['defocus'].any()) and _same_bits(out['refocused'], support.tensor(rc.encoded(b['view'])))
    half = ops.refocus(d['view'], flat, focus='point', gain=0.5)['refocused']
    assert _same_bits(half, support.tensor(rc.encoded(b['view']) * np.float32(0.5)))


@pytest.mark.parametrize('gamma', GAMMAS)
def test_a_constant_image_stays_constant(gamma):
    ops = support.ops()
    H, W, R = 37, 53, 16
    view = syn.scene(H, W, constant=0.4)['view'][None]
    d = (np.random.RandomState(7).randn(1, H, W) * 2).astype(np.float32)
    d[0, 5, 5:9] = np.nan
    got = _np(ops.refocus(support.tensor(view), support.tensor(d), focus='value', focus_value=0.1, max_radius=R, gamma=gamma))
    c = got['defocus'][0]
    r64, r32 = (rc.render(view[0], d[0], c, 1, R, gamma, dtype=t) for t in (np.float64, np.float32))
    bar = 2.0 * float(np.abs(r32.astype(np.float64) - r64).max()) + 2.0 ** -22
    v = rc.encoded(view[0]).astype(np.float64)
    err = float(np.abs(got['refocused'][0].astype(np.float64) - v).max())
    print('constant image gamma %.1f: max |dev - v| %.3e, bar %.3e' % (gamma, err, bar))
    assert np.ptp(c) > R and np.abs(r64 - v).max() <= 1e-12 and bar < 1e-4 and err <= bar


# ---- 3. the same bits every time, eager or replayed
def test_repeats_bit_for_bit_whatever_the_workspace_holds():
    ops = support.ops()
    d = _dev(scene('wide'))
    kw = dict(mask=d['mask'], max_radius=32)
    first = ops.refocus(d['view'], d['disparity'], **kw)
    mine = [buf for key, buf in ops._scratch.items() if key[1] == 'refocus']
    assert mine
    for fill in (float('nan'), 1e30):
        for buf in mine:
            buf.fill_(fill)
        again = ops.refocus(d['view'], d['disparity'], **kw)
        assert all(_same_bits(first[k], again[k]) for k in first)


def test_calls_replay_from_a_graph():
    ops = support.ops()
    d, other = _dev(scene('ragged')), _dev(scene('ragged'))
    other['view'] = other['view'].flip(0).contiguous()
    other['disparity'] = (other['disparity'] * 0.5).flip(0).contiguous()

    def run(b):
        return ops.refocus(b['view'], b['disparity'], mask=b['mask'])
    eager, want = run(d), run(other)
    assert not torch.equal(eager['refocused'], want['refocused'])
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
    d = _dev(scene('tiny'))
    B, H, W = 1, 5, 7
    nbytes = L.call('dpf_refocus_workspace_bytes', B, H, W)
    assert nbytes > 0 and nbytes % 8 == 0
    ws = torch.zeros(nbytes // 8 + 2, dtype=torch.float64, device=DEV)
    defocus = torch.full((B, H, W), 7.0, device=DEV)
    stats = torch.full((B, 8), 7.0, dtype=torch.float64, device=DEV)
    out = torch.full((B, 3, H, W), 7.0, device=DEV)
    norm = ops._normalizer_floats()
    p, st = support.ptr, support.stream()

    def plan(**kw):
        a = dict(pred=p(d['disparity']), stride=H * W, target=0, ab=None, mask=p(d['mask']), B=B, H=H, W=W, mode=0, fx=3, fy=2, value=0.0, aperture=4.0,
                 radius=8, sign=0, ws=p(ws), nbytes=nbytes, defocus=p(defocus), stats=p(stats))
        a.update(kw)
        return L.cdll.dpf_refocus_plan(*a.values(), st)

    def render(**kw):
        a = dict(image=p(d['view']), normalised=1, norm=norm, defocus=p(defocus), stats=p(stats), B=B, H=H, W=W, radius=8, gamma=2.2, gain=1.0,
                 ws=p(ws), nbytes=nbytes, out=p(out))
        a.update(kw)
        return L.cdll.dpf_refocus_render(*a.values(), st)
    for kw in (dict(pred=None), dict(defocus=None), dict(stats=None), dict(B=0), dict(H=0), dict(W=-1), dict(stride=H * W - 1), dict(target=3), dict(target=-1),
               dict(target=1), dict(target=2), dict(mode=3), dict(mode=1, fx=W), dict(mode=1, fy=-1), dict(value=float('nan')), dict(aperture=-1.0),
               dict(aperture=float('inf')), dict(radius=0), dict(radius=33), dict(sign=2), dict(ws=None), dict(nbytes=nbytes - 8),
               dict(ws=support.offset_ptr(ws, 4))):
        assert plan(**kw) == -1, kw
    for kw in (dict(image=None), dict(norm=None), dict(defocus=None), dict(stats=None), dict(out=None), dict(B=0), dict(radius=0), dict(radius=33),
               dict(gamma=0.0), dict(gamma=float('nan')), dict(gain=-1.0), dict(ws=None), dict(nbytes=nbytes - 8), dict(ws=support.offset_ptr(ws, 4))):
        assert render(**kw) == -1, kw
    assert plan(B=65536) == -3 and render(B=65536) == -3
    q = L.cdll.dpf_refocus_workspace_bytes
    for shape in ((0, 8, 12), (1, 0, 12), (1, 8, 0), (65536, 8, 12), (1, 1 << 16, 1 << 15)):
        assert q(*shape) == -1, shape
    torch.cuda.synchronize()
    assert bool((defocus == 7).all()) and bool((stats == 7).all()) and bool((out == 7).all()) and not bool(ws.any())
    assert plan() == 0 and render() == 0                               # and the same arguments, unbroken, run
    torch.cuda.synchronize()
    got = device('tiny', focus='mask_mean')
    assert np.array_equal(support.bits(out.cpu().numpy()), support.bits(got['refocused']))
    assert np.array_equal(stats.cpu().numpy(), got['refocus_stats'])


def test_ops_refuse_what_does_not_fit():
    from dualpixelface_amd._lib import DpfError
    ops = support.ops()
    d = _dev(scene('tiny'))
    view, disp, mask = d['view'], d['disparity'], d['mask']
    for kw, match in ((dict(max_radius=0), 'max_radius'), (dict(max_radius=33), 'max_radius'), (dict(max_radius=8.5), 'max_radius'),
                      (dict(max_radius=True), 'max_radius'), (dict(focus='centre'), 'focus'), (dict(near_sign=0), 'near_sign'),
                      (dict(target_type='depth'), 'ab'), (dict(target_type='idepth'), 'ab'), (dict(target_type='range'), 'target_type'),
                      (dict(aperture=-1.0), 'DPF_ERR_INVALID_ARG'), (dict(gamma=0.0), 'DPF_ERR_INVALID_ARG'), (dict(gain=-1.0), 'DPF_ERR_INVALID_ARG'),
                      (dict(ab=torch.zeros(1, 3, device=DEV)), 'ab'), (dict(source=view[:, :2]), 'source'), (dict(mask=mask[:, :4]), 'mask'),
                      (dict(mask=mask.double()), 'dtype'), (dict(mask=mask.cpu()), 'GPU')):
        with pytest.raises(DpfError, match=match):
            ops.refocus(view, disp, **dict(dict(mask=mask), **kw))
    for bad_view, bad_disp, match in ((view[:, :2], disp, 'view'), (view, disp[:, :4], 'disparity'), (view, disp[0, 0], 'disparity'),
                                      (view.cpu(), disp, 'GPU'), (view, disp.half(), 'dtype'), (view.double(), disp, 'dtype')):
        with pytest.raises(DpfError, match=match):
            ops.refocus(bad_view, bad_disp)
    heads = torch.stack([disp, disp * 2, disp * 3], 1)                  # head 0 of [B, n, H, W], also as a slice of a wider tensor
    want = ops.refocus(view, disp, mask=mask, max_radius=8)
    for pred in (heads, heads[:, :1], disp.unsqueeze(1).requires_grad_()):
        got = ops.refocus(view.clone().requires_grad_(), pred, mask=mask, max_radius=8)
        assert all(_same_bits(got[k], want[k]) and not got[k].requires_grad for k in want)


# ---- 5. the whole model
def _model(cls_name, config, over=None, **blocks):
    from dualpixelface_amd.config import Option
    opt = support.option(config, **(over or {}))
    for name, block in blocks.items():
        setattr(opt, name, Option(dict(block)))
    return support.build(cls_name, opt)


def test_stereodpnet_evaluation_ends_with_the_refocused_view():
    from dualpixelface_amd import ops, refocus
    from dualpixelface_amd.config import Option
    model = _model('STEREODPNET', 'eval_faceDP')
    batch = support.batch(1, 64, 96, seed=9, mask_mode='bern')
    model.eval()
    with torch.no_grad(), ops.deterministic_mode():
        absent = model.forward(dict(batch))
        assert not hasattr(model.option, 'refocus')
        model.option.refocus = Option(dict(enabled=False, aperture=9.0))
        off = model.forward(dict(batch))
        assert list(off) == list(absent) and all(off[k] is None and absent[k] is None or _same_bits(off[k], absent[k]) for k in off)
        model.option.refocus = Option(dict(enabled=True, max_radius=8))
        on = model.forward(dict(batch))
        assert list(on) == list(off) + list(refocus.RESULT_KEYS)
        for k in off:
            assert off[k] is None and on[k] is None or _same_bits(off[k], on[k]), k
        view = model._views(batch)[0]
        want = ops.refocus(view, on['pred_depth'], mask=batch['mask'], ab=batch['abvalue'], max_radius=8)
        assert all(_same_bits(on[k], want[k]) for k in want)
        assert on['refocused'].shape == (1, 3, 64, 96) and on['defocus'].shape == (1, 64, 96) and on['refocus_stats'].shape == (1, 8)
        assert float(on['refocused'].min()) >= 0 and float(on['refocused'].max()) <= 1
        row = on['refocus_stats'][0].tolist()
        print('stereodpnet 1x64x96: stats %s' % row)
        assert row[1] == float((batch['mask'] > 0).sum()) and row[2] == 1 and row[3] == -1 and row[4] <= 0 <= row[5]    # the batch's a is negative
        model.option.refocus = Option(dict(enabled=True, source='relit'))
        with pytest.raises(NotImplementedError, match=r'shading\.relight\.enabled'):
            model.forward(dict(batch))
    with ops.deterministic_mode():                                # training mode: nothing is refocused, whatever the block says
        model.option.refocus = Option(dict(enabled=True))
        model.train()
        res = model.forward(dict(batch))
    assert not set(res) & set(refocus.RESULT_KEYS) and res['pred_depth'].requires_grad


def test_dpnet_under_idepth_takes_ab_from_the_fit():
    from dualpixelface_amd import ops
    model = _model('DPNET', 'eval_faceDP_dpnet', over=dict(target_type='idepth'), refocus=dict(enabled=True, max_radius=8, aperture=40.0))
    batch = support.batch(1, 64, 96, seed=9, mask_mode='bern')
    del batch['abvalue']
    model.eval()
    with torch.no_grad(), ops.deterministic_mode():
        assert model._target_type() == 'idepth'
        res = model.forward(dict(batch))
        fitted = res['abvalue']
        assert fitted.shape == (1, 2)
        want = ops.refocus(model._views(batch)[0], res['pred_depth'], mask=batch['mask'], ab=fitted, target_type='idepth', max_radius=8, aperture=40.0)
        assert all(_same_bits(res[k], want[k]) for k in want)
        assert float(res['refocus_stats'][0, 3]) == (-1.0 if float(fitted[0, 1]) < 0 else 1.0)
        missing = {k: v for k, v in batch.items() if k != 'idepth'}
        with pytest.raises(NotImplementedError, match='abvalue'):
            model.forward(missing)


def test_the_relit_view_is_what_gets_refocused():
    from dualpixelface_amd import ops
    from dualpixelface_amd import synthetic_shading
    from dualpixelface_amd.core import reference_key
    blocks = dict(shading=dict(enabled=True, normals='batch', relight=dict(enabled=True, rotate_deg=[0, 30, 0])),
                  refocus=dict(enabled=True, source='relit', max_radius=8))
    model = _model('STEREODPNET', 'eval_faceDP', **blocks)
    lit = synthetic_shading.batch(1, 64, 96, albedo='uniform', gamma=2.2, seed=5)      # a shaded ellipsoid the lighting fit explains
    batch = dict(support.batch(1, 64, 96, seed=9, mask_mode='bern'),
                 **{reference_key(model.option): support.tensor(lit['view']), 'normal': support.tensor(lit['normal']), 'mask': support.tensor(lit['mask'])})
    model.eval()
    with torch.no_grad(), ops.deterministic_mode():
        res = model.forward(dict(batch))
        view = model._views(batch)[0]
        assert float(res['shading_stats'][0, 1]) == 1 and not torch.equal(res['relit'], support.tensor(rc.encoded(lit['view'])))
        want = ops.refocus(view, res['pred_depth'], mask=batch['mask'], ab=batch['abvalue'], source=res['relit'], max_radius=8)
        plain = ops.refocus(view, res['pred_depth'], mask=batch['mask'], ab=batch['abvalue'], max_radius=8)
        assert all(_same_bits(res[k], want[k]) for k in want)
        assert _same_bits(plain['defocus'], want['defocus']) and not torch.equal(plain['refocused'], want['refocused'])
        sharp = ops.refocus(view, res['pred_depth'], source=res['relit'], aperture=0.0)['refocused']
        assert _same_bits(sharp, res['relit'].clamp(0, 1))


def test_main_evaluates_the_refocus_config():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, 'main.py', '--config', 'eval_faceDP_refocus', '--workspace', 'pytest_refocus', '--synthetic', '4', '--height',
                        '64', '--width', '96'], cwd=root, env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
