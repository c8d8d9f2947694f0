"""The shading block on the GPU (run with ``-m gpu``): csrc/shading.hip through ops.shading_fit and ops.shading_apply, and the ``shading``
block through the plugins' evaluation forward, against the numpy restatement of tests/shading_cpu.py on the scene of
dualpixelface_amd/synthetic_shading.py.

Shapes.  1 x 5 x 7: fewer pixels than one wave's strip of 64 and no multiple of 4 (min_pixels is lowered to 12 for its 23 pixels).
2 x 37 x 53: ragged, two partial rows per sample, a different mask per sample.  1 x 725 x 727: 527075 pixels are more than
ops.SHADING_MAX_ROWS x ops.SHADING_CHUNK = 512 x 1024, so a workgroup walks 1280 pixels instead of 1024 (five strips per wave instead of
four) and the sample leaves 412 partial rows -- more than the 256 threads of the fold, so a fold thread joins two rows (asserted below
from ops.shading_rows).

Bars.  Gram: every entry of the 13 x 13 block within 4 N 2^-53 sqrt(G_ii G_jj) of the restatement's (Cauchy-Schwarz with w <= 1, a factor
2 for each side's summation error), the padding exactly 0; on the clean scene without a ridge, where the residuals are the 1e-7 of the
stored fp32 values and the weights of the later passes do not feel the 1e-12 by which the two sides' L differ (with residuals e the weights
move by (e / f_scale^2) x 1e-12: under the default ridge e = 2e-5 and that is 1e-14, the size of the bound at N = 23).  light, iterations 0: within 2^-22 max |L_c|, given 8 cond(A) N 2^-53 < 2^-24 (asserted).
light, iterations 3: 4 ulp + 8 x the restatement's own spread between forward and reversed pixel order, in fp32 ulps of max |L_c|; that
spread is 0 ulp on every scene here (the fp64 difference is 1e-12 .. 3e-11, far below an fp32 ulp), so the bar is 4 ulp.  Planes at gamma 1:
bit for bit from the device's light.  Planes at gamma 2.2: shading and the map bit for bit, albedo and relit within POW_BAR ulp of the
restatement under fp64 pow rounded to fp32; measured on an MI355X: 2 ulp for both, so POW_BAR = 4 (below).  Also measured there: Gram at
most 0.059 of its bound; light of the plain fit within 5.3e-8 of max |L_c| (bar 2.4e-7); light of the reweighted fit within 0.50 ulp (bar
4); identity relight within 1 ulp on every applicable pixel (bar 2, share 1.0 against 0.9); rotation at most 0.018 of its bar."""
import functools

import numpy as np
import pytest
import torch

from dualpixelface_amd import synthetic_shading as syn
from tests import shading_cpu as sc
from tests import support
from tests.support import DEV

pytestmark = pytest.mark.gpu

# (B, H, W, min_pixels)
TINY, RAGGED, LARGE = (1, 5, 7, 12), (2, 37, 53, 72), (1, 725, 727, 72)
CASES = (TINY, RAGGED, LARGE)
# albedo and relit at gamma 2.2 against fp64 pow rounded to fp32: the largest distance measured on an MI355X was 2 ulp (albedo) and 2 ulp (relit);
# the bar is twice that and never above 16
POW_MEASURED = 2
POW_BAR = min(2 * POW_MEASURED, 16)
ROTATE = (10.0, 30.0, -20.0)


def case_id(c):
    return '%dx%dx%d' % c[:3]


@functools.lru_cache(maxsize=None)
def scene(case, kind='clean', gamma=1.0):
    """The batch of a case as numpy arrays: 'clean' (uniform albedo, every pixel explained) or 'rough' (texture and 5 % outliers).  Sample 1
    of a batch loses a seeded fifth of its mask."""
    B, H, W, _ = case
    kw = dict(albedo='uniform') if kind == 'clean' else dict(albedo='texture', outliers=0.05)
    b = syn.batch(B, H, W, gamma=gamma, seed=3, **kw)
    for s in range(1, B):
        b['mask'][s] *= np.random.RandomState(40 + s).rand(H, W) < 0.8
    return b


def _dev(b):
    return {k: support.tensor(v) for k, v in b.items()}


def _pixels(b, s, **kw):
    return sc.pixels(b['view'][s], b['normal'][s], b['mask'][s], **kw)


@functools.lru_cache(maxsize=None)
def reference(case, kind, iterations, reverse=False, ridge=1e-6):
    """The restatement's fit of every sample of a case at gamma 1 (computed once, shared, never changed)."""
    b = scene(case, kind)
    out = []
    for s in range(case[0]):
        px = _pixels(b, s, gamma=1)
        out.append(sc.fit(px['I'], px['nh'], px['counted'], iterations=iterations, min_pixels=case[3], reverse=reverse, ridge=ridge))
    return out


def _fit(case, kind='clean', gamma=1.0, **kw):
    d = _dev(scene(case, kind, gamma))
    kw.setdefault('min_pixels', case[3])
    return d, support.ops().shading_fit(d['view'], d['normal'], d['mask'], gamma=gamma, **kw)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_the_large_plane_is_past_both_thresholds():
    ops = support.ops()
    _, H, W, _ = LARGE
    rows, per_block = ops.shading_rows(H, W)
    assert H * W > ops.SHADING_MAX_ROWS * ops.SHADING_CHUNK and per_block > ops.SHADING_CHUNK and rows > ops.SHADING_FOLD, (rows, per_block)
    assert ops.shading_rows(5, 7) == (1, 256) and ops.shading_rows(37, 53) == (2, 1024)
    assert ops.lib().call('dpf_shading_workspace_bytes', 1, H, W) == (rows * 266 + 32) * 8


# ---- 1. the Gram matrix
@pytest.mark.parametrize('iterations', (0, 3))
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_gram_against_the_restatement(case, iterations):
    _, (light, stats, G) = _fit(case, iterations=iterations, ridge=0.0, gram=True)
    assert G.shape == (case[0], 16, 16) and G.dtype == torch.float64 and stats.shape == (case[0], 16) and light.shape == (case[0], 3, 9)
    G, stats = G.cpu().numpy(), stats.cpu().numpy()
    for s, ref in enumerate(reference(case, 'clean', iterations, ridge=0.0)):
        N = ref['stats'][0]
        want = ref['gram']
        diag = np.sqrt(np.abs(np.diag(want)))
        bound = 4.0 * N * 2.0 ** -53 * np.outer(diag, diag)
        err = np.abs(G[s] - want)
        worst = (err[:13, :13] / np.maximum(bound[:13, :13], 1e-300)).max()
        print('gram %s sample %d, %d passes: N %d, worst |G - G_np| / bound %.3f' % (case_id(case), s, iterations + 1, N, worst))
        assert stats[s, 0] == N and stats[s, 2] == iterations + 1
        assert (err[:13, :13] <= bound[:13, :13]).all()
        assert not G[s, 13:].any() and not G[s, :, 13:].any()                       # the padding rows and columns are exactly 0
        assert np.isclose(stats[s, 3], want[12, 12], rtol=1e-12) and G[s, 12, 12] == stats[s, 3]


# ---- 2. the light
@pytest.mark.parametrize('case', (TINY, RAGGED), ids=case_id)
def test_light_of_the_plain_fit(case):
    _, (light, stats) = _fit(case, iterations=0)
    light, stats = light.cpu().numpy(), stats.cpu().numpy()
    for s, ref in enumerate(reference(case, 'clean', 0)):
        N = ref['stats'][0]
        assert 8 * ref['cond'] * N * 2.0 ** -53 < 2.0 ** -24, (ref['cond'], N)
        scale = np.abs(ref['light64']).max(1, keepdims=True)
        err = (np.abs(light[s].astype(np.float64) - ref['light64']) / scale).max()
        print('light %s sample %d: cond %.3e, N %d, max |dev - np| / max |L_c| %.3e (bar 2^-22 = %.3e)' % (case_id(case), s, ref['cond'], N, err,
                                                                                                         2.0 ** -22))
        assert stats[s, 1] == 1 and err <= 2.0 ** -22
        assert np.allclose(stats[s, 4:10], ref['stats'][4:10], atol=1e-6)


@pytest.mark.parametrize('kind', ('clean', 'rough'))
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_light_of_the_reweighted_fit(case, kind):
    """The restatement's spread between forward and reversed pixel order is 0 fp32 ulp of max |L_c| on all six scenes (the fp64 difference
    is 8e-13 .. 3e-11), so the bar is 4 ulp."""
    _, (light, stats) = _fit(case, kind, iterations=3)
    light, stats = light.cpu().numpy(), stats.cpu().numpy()
    fwd, rev = reference(case, kind, 3), reference(case, kind, 3, True)
    for s in range(case[0]):
        for c in range(3):
            ulp = support.ulp_of(np.abs(fwd[s]['light64'][c]).max())
            spread = np.abs(fwd[s]['light'][c].astype(np.float64) - rev[s]['light'][c].astype(np.float64)).max() / ulp
            err = np.abs(light[s, c].astype(np.float64) - fwd[s]['light64'][c]).max() / ulp
            print('light %s %s sample %d channel %d: spread %.2f ulp, |dev - np| %.3f ulp (bar %.2f)' % (case_id(case), kind, s, c, spread, err,
                                                                                                      4 + 8 * spread))
            assert err <= 4 + 8 * spread
        assert stats[s, 1] == 1 and stats[s, 2] == 4
        assert np.allclose(stats[s, 3:10], fwd[s]['stats'][3:10], rtol=1e-6, atol=1e-6)
    if kind == 'rough' and case != TINY:                                                     # the weights did something
        assert stats[0, 3] < 0.99 * stats[0, 0] and (stats[0, 7:10] < stats[0, 4:7]).all()


# ---- 3. the planes
def _apply_both(case, kind, gamma, exact_pow=False, **kw):
    """(device planes, the restatement's from the device's light, the device's stats)"""
    ops = support.ops()
    d, (light, stats) = _fit(case, kind, gamma=gamma)
    got = ops.shading_apply(d['view'], d['normal'], light, mask=d['mask'], stats=stats, gamma=gamma, **kw)
    b = scene(case, kind, gamma)
    R = ops.shading_rotation(kw.get('rotate_deg', (0, 0, 0)))
    want = []
    for s in range(case[0]):
        px = _pixels(b, s, gamma=gamma, exact_pow=exact_pow, signs=kw.get('normal_signs', (1, 1, 1)))
        want.append(sc.apply32(light[s].cpu().numpy(), px, valid=bool(stats[s, 1] > 0), gamma=gamma, relight=kw.get('relight', False), R=R,
                               coefficients=kw.get('coefficients'), gain=kw.get('gain', 1.0), exact_pow=exact_pow))
    return {k: v.cpu().numpy() for k, v in got.items()}, want, stats.cpu().numpy()


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_planes_bit_for_bit_at_gamma_1(case):
    got, want, stats = _apply_both(case, 'rough', 1.0, relight=True, rotate_deg=ROTATE, gain=1.1)
    assert set(got) == {'shading', 'albedo', 'shading_valid', 'relit'} and got['shading_valid'].dtype == np.uint8
    for s in range(case[0]):
        assert stats[s, 1] == 1 and want[s]['shading_valid'].sum() > 0
        for k in ('shading', 'albedo', 'relit'):
            assert np.array_equal(support.bits(got[k][s]), support.bits(want[s][k])), (k, s)
        assert np.array_equal(got['shading_valid'][s], want[s]['shading_valid'])
    # replaced light: the relit view is lit by the coefficients, the other planes do not move
    coeff = (syn.LIGHT[:, ::-1] * 0.5).tolist()
    got2, want2, _ = _apply_both(case, 'rough', 1.0, relight=True, coefficients=coeff)
    for s in range(case[0]):
        assert np.array_equal(support.bits(got2['relit'][s]), support.bits(want2[s]['relit']))
        assert np.array_equal(support.bits(got2['albedo'][s]), support.bits(got['albedo'][s]))
    assert not np.array_equal(got2['relit'], got['relit'])


def test_planes_at_gamma_2_2():
    got, want, stats = _apply_both(RAGGED, 'rough', 2.2, exact_pow=True, relight=True, rotate_deg=ROTATE)
    for s in range(RAGGED[0]):
        live = want[s]['shading_valid'] > 0
        assert stats[s, 1] == 1 and np.array_equal(got['shading_valid'][s] > 0, live)
        assert np.array_equal(support.bits(got['shading'][s]), support.bits(want[s]['shading']))
        worst = {k: int(sc.ulps(got[k][s][:, live], want[s][k][:, live]).max()) for k in ('albedo', 'relit')}
        print('gamma 2.2 sample %d: largest distance to fp64 pow rounded to fp32: %s ulp (bar %d)' % (s, worst, POW_BAR))
        assert max(worst.values()) <= POW_BAR
        assert np.array_equal(support.bits(got['relit'][s][:, ~live]), support.bits(want[s]['relit'][:, ~live]))


# ---- 4. identity relight
def test_identity_relight_returns_the_view():
    got, want, _ = _apply_both(RAGGED, 'clean', 1.0, relight=True)
    b = scene(RAGGED, 'clean')
    for s in range(RAGGED[0]):
        px = _pixels(b, s, gamma=1)
        live = np.broadcast_to(px['applicable'], (3,) + px['applicable'].shape)
        ok = live & (got['shading'][s] > np.float32(0.05)) & (got['albedo'][s] < np.float32(4.0))
        share = ok.sum() / float(live.sum())
        worst = int(sc.ulps(got['relit'][s][ok], px['v'][ok]).max())
        print('identity relight sample %d: %.3f of the applicable pixels qualify, worst %d ulp' % (s, share, worst))
        assert share >= 0.9 and worst <= 2
        assert np.array_equal(support.bits(got['relit'][s][~live]), support.bits(px['v'][~live]))


# ---- 5. sign invariance
def test_the_fit_and_the_planes_do_not_depend_on_the_signs():
    ops = support.ops()
    d, (light, stats) = _fit(RAGGED, 'rough')
    _, (light2, stats2) = _fit(RAGGED, 'rough', normal_signs=(1, -1, 1))
    parity = torch.tensor(ops.SHADING_SIGN_PARITY, dtype=torch.float32, device=DEV)
    assert _same_bits(light, light2 * parity) and bool((light[:, :, 1] != 0).all())
    assert _same_bits(stats, stats2)
    a = ops.shading_apply(d['view'], d['normal'], light, mask=d['mask'], stats=stats)
    b = ops.shading_apply(d['view'], d['normal'], light2, mask=d['mask'], stats=stats2, normal_signs=(1, -1, 1))
    for k in ('shading', 'albedo', 'shading_valid'):
        assert _same_bits(a[k], b[k]), k


# ---- 6. rotation
def test_rotating_the_light_is_rotating_the_normals():
    """relit under rotate_deg against (a) the restatement that rotates in fp32 in the kernel's order, bit for bit (with the planes test
    above), and (b) the albedo times the shading that ops.shading_apply gives for normals rotated by R^T on the host and no rotation.  (b)
    cannot be bit for bit: the host rounds the rotated normal to fp32 and the kernel renormalises it, some 4 x 2^-24 in the normal, which
    the basis (gradient at most 2.2 per unit) and the nine products carry into at most 64 x 2^-24 x sum_k |L_ck| of shading."""
    ops = support.ops()
    rot = (0.0, 30.0, 0.0)
    got, want, _ = _apply_both(RAGGED, 'clean', 1.0, relight=True, rotate_deg=rot)
    d, (light, stats) = _fit(RAGGED, 'clean')
    R = np.array(ops.shading_rotation(rot)).reshape(3, 3)
    turned = np.einsum('ji,bjhw->bihw', R, scene(RAGGED, 'clean')['normal'].astype(np.float64)).astype(np.float32)
    other = ops.shading_apply(d['view'], support.tensor(turned), light, mask=d['mask'], stats=stats, gamma=1.0)
    for s in range(RAGGED[0]):
        assert np.array_equal(support.bits(got['relit'][s]), support.bits(want[s]['relit']))
        live = want[s]['shading_valid'] > 0
        albedo = got['albedo'][s].astype(np.float64)
        lin = np.clip(albedo * np.maximum(other['shading'][s].cpu().numpy().astype(np.float64), 0.0), 0.0, 1.0)
        bar = 64 * 2.0 ** -24 * np.abs(light[s].cpu().numpy().astype(np.float64)).sum(1).reshape(3, 1, 1) * albedo + 2.0 ** -23
        err = np.abs(got['relit'][s].astype(np.float64) - lin)
        print('rotation sample %d: worst |relit - albedo x shading(R^T n)| / bar %.3f' % (s, (err / bar)[:, live].max()))
        assert (err <= bar)[:, live].all()
        assert not np.array_equal(got['relit'][s][:, live], scene(RAGGED, 'clean')['view'][s][:, live])


# ---- 7. an invalid sample
def test_an_invalid_sample_is_flagged_and_leaves_the_others_alone():
    ops = support.ops()
    b = scene(RAGGED, 'rough')
    three = {k: np.stack([v[0], v[1], v[1]]) for k, v in b.items()}
    three['mask'][1] = 0
    d3, d2 = _dev(three), _dev(b)
    light3, stats3 = ops.shading_fit(d3['view'], d3['normal'], d3['mask'], gamma=1.0)
    light2, stats2 = ops.shading_fit(d2['view'], d2['normal'], d2['mask'], gamma=1.0)
    p3 = ops.shading_apply(d3['view'], d3['normal'], light3, mask=d3['mask'], stats=stats3, albedo_label=d3['albedo'], gamma=1.0, relight=True,
                           rotate_deg=ROTATE)
    p2 = ops.shading_apply(d2['view'], d2['normal'], light2, mask=d2['mask'], stats=stats2, albedo_label=d2['albedo'], gamma=1.0, relight=True,
                           rotate_deg=ROTATE)
    assert stats3[1, 0] == 0 and stats3[1, 1] == 0 and not bool(light3[1].any()) and bool((stats3[1, 10:13] == -1).all()) and stats3[1, 13] == 0
    v = sc.pixels(three['view'][1], three['normal'][1], three['mask'][1], gamma=1)['v']
    assert not bool(p3['shading'][1].any()) and not bool(p3['albedo'][1].any()) and not bool(p3['shading_valid'][1].any())
    assert np.array_equal(support.bits(p3['relit'][1].cpu().numpy()), support.bits(v))
    keep = torch.tensor([0, 2], device=DEV)
    assert _same_bits(light3[keep], light2) and _same_bits(stats3[keep], stats2) and bool((stats2[:, 1] == 1).all())
    for k in p2:
        assert _same_bits(p3[k][keep], p2[k]), k
    # a sample that is masked only in part but keeps fewer than min_pixels pixels is invalid too; so is one with a single normal
    few = {k: v[:1].copy() for k, v in b.items()}
    few['mask'][0] *= 0
    few['mask'][0, 17:20, 17:37] = 1                                                # 60 pixels in the middle of the ellipsoid
    df = _dev(few)
    _, st = ops.shading_fit(df['view'], df['normal'], df['mask'], gamma=1.0)
    assert st[0, 0] == 60 and st[0, 1] == 0
    flat = np.zeros_like(b['normal'][:1])
    flat[:, 2] = 1.0
    light, st = ops.shading_fit(d2['view'][:1], support.tensor(flat), d2['mask'][:1], gamma=1.0, ridge=0.0)
    assert st[0, 0] >= 72 and st[0, 1] == 0 and not bool(light.any())               # one normal and no ridge: the pivots vanish
    light, st = ops.shading_fit(d2['view'][:1], support.tensor(flat), d2['mask'][:1], gamma=1.0)
    assert st[0, 1] == 1 and bool(torch.isfinite(light).all())                      # the ridge holds the bands the normals do not span


def test_the_albedo_check():
    """The clean scene (uniform albedo, the label 1 everywhere) is fitted without a ridge: the error is then the 1e-7 of the fp32 planes.
    Under the default ridge of 1e-6 the fitted shading is off by 1e-4 and the error reads 2.9e-5."""
    ops = support.ops()
    for case, kind in ((RAGGED, 'rough'), (RAGGED, 'clean')):
        d, (light, stats) = _fit(case, kind, ridge=1e-6 if kind == 'rough' else 0.0)
        before = stats.clone()
        planes = ops.shading_apply(d['view'], d['normal'], light, mask=d['mask'], stats=stats, albedo_label=d['albedo'], gamma=1.0)
        b = scene(case, kind)
        st = stats.cpu().numpy()
        for s in range(case[0]):
            px = _pixels(b, s, gamma=1)
            want = sc.albedo_error(planes['albedo'][s].cpu().numpy(), b['albedo'][s], px['counted'])
            print('albedo check %s sample %d: %s against %s' % (kind, s, st[s, 10:14], want))
            assert st[s, 13] == want[3] == px['counted'].sum()
            if kind == 'clean':                                                     # 1 - x at x = 1: both sides are rounding noise below 1e-6
                assert (st[s, 10:13] >= 0).all() and (st[s, 10:13] < 1e-6).all() and (want[:3] < 1e-6).all()
            else:
                assert np.allclose(st[s, 10:13], want[:3], atol=1e-9) and (st[s, 10:13] > 1e-3).all()
        assert _same_bits(stats[:, :10], before[:, :10]) and bool((before[:, 10:13] == -1).all())
    one = ops.shading_apply(d['view'], d['normal'], light, mask=d['mask'], stats=before, albedo_label=d['albedo'][:, 0].contiguous(), gamma=1.0)
    assert torch.allclose(before[:, 10:14], stats[:, 10:14], atol=1e-9) and _same_bits(one['albedo'], planes['albedo'])


# ---- 8. the same bits every time, eager or replayed
def test_repeats_bit_for_bit_whatever_the_workspace_holds():
    ops = support.ops()
    d, first = _fit(LARGE, 'rough', gram=True)
    planes = ops.shading_apply(d['view'], d['normal'], first[0], mask=d['mask'], stats=first[1], relight=True, rotate_deg=ROTATE)
    mine = [buf for key, buf in ops._scratch.items() if key[1] == 'shading']
    assert mine
    for fill in (float('nan'), 1e30):
        for buf in mine:
            buf.fill_(fill)
        _, again = _fit(LARGE, 'rough', gram=True)
        assert all(_same_bits(a, b) for a, b in zip(first, again))
        for buf in mine:
            buf.fill_(fill)
        planes2 = ops.shading_apply(d['view'], d['normal'], again[0], mask=d['mask'], stats=again[1], relight=True, rotate_deg=ROTATE)
        assert all(_same_bits(planes[k], planes2[k]) for k in planes)


def test_calls_replay_from_a_graph():
    ops = support.ops()
    d = _dev(scene(RAGGED, 'rough'))
    other = _dev(scene(RAGGED, 'clean'))

    def run(view, normal, mask, label):
        light, stats = ops.shading_fit(view, normal, mask, gamma=1.0)
        return light, stats, ops.shading_apply(view, normal, light, mask=mask, stats=stats, albedo_label=label, gamma=1.0, relight=True,
                                               rotate_deg=ROTATE)
    eager = run(d['view'], d['normal'], d['mask'], d['albedo'])
    want = run(other['view'], other['normal'], other['mask'], other['albedo'])
    assert not torch.equal(eager[0], want[0])
    st = {k: v.clone() for k, v in d.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                 # the side stream's scratch exists before the capture
        run(st['view'], st['normal'], st['mask'], st['albedo'])
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):                    # one stream, no fork
        light, stats, planes = run(st['view'], st['normal'], st['mask'], st['albedo'])
    for src, w in ((other, want), (d, eager)):
        for k in st:
            st[k].copy_(src[k])
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(light, w[0]) and _same_bits(stats, w[1])
        assert all(_same_bits(planes[k], w[2][k]) for k in planes)


def test_ops_refuse_what_does_not_fit():
    from dualpixelface_amd._lib import DpfError
    ops = support.ops()
    d = _dev(scene(TINY))
    view, normal, mask = d['view'], d['normal'], d['mask']
    for kw, match in ((dict(order=3), 'order'), (dict(iterations=9), 'DPF_ERR_INVALID_ARG'), (dict(iterations=1.5), 'iterations'),
                      (dict(normal_signs=(1, 0, 1)), 'normal_signs'), (dict(gamma=0.0), 'DPF_ERR_INVALID_ARG'),
                      (dict(min_value=0.5, max_value=0.4), 'DPF_ERR_INVALID_ARG'), (dict(f_scale=0.0), 'DPF_ERR_INVALID_ARG'),
                      (dict(ridge=-1.0), 'DPF_ERR_INVALID_ARG'), (dict(min_pixels=0), 'DPF_ERR_INVALID_ARG')):
        with pytest.raises(DpfError, match=match):
            ops.shading_fit(view, normal, mask, **kw)
    with pytest.raises(DpfError, match='normal'):
        ops.shading_fit(view, normal[:, :, :4], mask)
    with pytest.raises(DpfError, match='mask'):
        ops.shading_fit(view, normal, mask[:, :4])
    with pytest.raises(DpfError, match='GPU'):
        ops.shading_fit(view.cpu(), normal, mask)
    light, stats = ops.shading_fit(view.requires_grad_(), normal, mask, min_pixels=12)
    assert not light.requires_grad and light.grad_fn is None
    for kw, match in ((dict(light=light[:, :2]), 'light'), (dict(stats=stats[:, :8].contiguous()), 'stats'), (dict(shade_floor=0.0), 'DPF_ERR_INVALID_ARG'),
                      (dict(albedo_max=0.0), 'DPF_ERR_INVALID_ARG'), (dict(gain=-1.0), 'DPF_ERR_INVALID_ARG'),
                      (dict(coefficients=[[0.0] * 9] * 2), 'coefficients'), (dict(albedo_label=view[:, :2]), 'albedo_label')):
        with pytest.raises(DpfError, match=match):
            ops.shading_apply(view, normal, **dict(dict(light=light, mask=mask, relight=True), **kw))
    q = ops.lib().cdll.dpf_shading_workspace_bytes
    for shape in ((0, 8, 12), (1, 0, 12), (1, 8, 0), (65536, 8, 12), (1, 1 << 16, 1 << 15)):
        assert q(*shape) == -1, shape


# ---- 9. the whole model
def _model(cls_name, config, **blocks):
    from dualpixelface_amd.config import Option
    opt = support.option(config)
    for name, block in blocks.items():
        setattr(opt, name, Option(dict(block)))
    return support.build(cls_name, opt)


def _scene_batch(option, batch, H, W):
    """The synthetic batch with the shaded ellipsoid as its reference view, normal map, mask and albedo label."""
    from dualpixelface_amd.core import reference_key
    s = _dev(syn.batch(1, H, W, albedo='uniform', gamma=2.2, seed=5))
    return dict(batch, **{reference_key(option): s['view'], 'normal': s['normal'], 'mask': s['mask'], 'albedo': s['albedo']})


def test_stereodpnet_evaluation_ends_with_the_shading():
    from dualpixelface_amd import ops, shading
    from dualpixelface_amd.config import Option
    model = _model('STEREODPNET', 'eval_faceDP')
    batch = support.batch(1, 64, 96, seed=9, mask_mode='bern')
    model.eval()
    with torch.no_grad(), ops.deterministic_mode():
        absent = model.forward(dict(batch))
        assert not hasattr(model.option, 'shading')
        model.option.shading = Option(dict(enabled=False, iterations=5))
        off = model.forward(dict(batch))
        assert list(off) == list(absent) and all(off[k] is None and absent[k] is None or _same_bits(off[k], absent[k]) for k in off)
        model.option.shading = Option(dict(enabled=True))
        on = model.forward(dict(batch))
        keys = set(shading.RESULT_KEYS) - {'relit'}
        assert set(on) == set(off) | keys and not set(off) & set(shading.RESULT_KEYS)
        model.option.shading = Option(dict(enabled=True, relight=dict(enabled=True, rotate_deg=[0, 30, 0])))
        lit = model.forward(dict(batch))
        assert set(lit) == set(off) | set(shading.RESULT_KEYS)
        for k in off:
            assert off[k] is None and lit[k] is None or _same_bits(off[k], lit[k]), k
        for k in keys:
            assert _same_bits(on[k], lit[k]), k
        view = model._views(batch)[0]
        light, stats = ops.shading_fit(view, lit['pred_normal'][:, 0], batch['mask'])
        planes = ops.shading_apply(view, lit['pred_normal'][:, 0], light, mask=batch['mask'], stats=stats, relight=True, rotate_deg=(0, 30, 0))
        assert _same_bits(lit['light'], light) and _same_bits(lit['shading_stats'], stats)
        assert all(_same_bits(lit[k], planes[k]) for k in planes)
        assert lit['shading'].shape == (1, 3, 64, 96) and lit['shading_valid'].dtype == torch.uint8 and lit['light'].shape == (1, 3, 9)
        assert float(lit['relit'].min()) >= 0 and float(lit['relit'].max()) <= 1 and bool((stats[:, 10:13] == -1).all())
        # the scene's true normals and its albedo label under a uniform albedo: the relative albedo matches the label up to scale
        # (without a ridge: the default 1e-6 moves the shading by 1e-4 and the error reads 2.8e-5; without it 1e-7 is the fp32 planes' own)
        model.option.shading = Option(dict(enabled=True, normals='batch', ridge=0.0))
        res = model.forward(_scene_batch(model.option, batch, 64, 96))
        row = res['shading_stats'][0].cpu().tolist()
        print('stereodpnet 1x64x96, true normals and a uniform albedo: stats %s' % row)
        assert row[1] == 1 and row[13] > 1000 and all(0 <= v <= 1e-6 for v in row[10:13])
        unlabelled = _scene_batch(model.option, batch, 64, 96)
        del unlabelled['albedo']
        assert bool((model.forward(unlabelled)['shading_stats'][:, 10:13] == -1).all())
        model.option.shading = Option(dict(enabled=True, normals='batch'))
        missing = {k: v for k, v in batch.items() if k != 'normal'}
        with pytest.raises(NotImplementedError, match='normal'):
            model.forward(missing)
    with ops.deterministic_mode():                                # training mode: nothing is shaded, whatever the block says
        model.train()
        res = model.forward(dict(batch))
    assert not set(res) & set(shading.RESULT_KEYS) and res['pred_depth'].requires_grad


def test_dpnet_shades_under_the_geometric_normals():
    from dualpixelface_amd import ops, plugin as plugins, shading
    from dualpixelface_amd.config import Option
    model = _model('DPNET', 'eval_faceDP_dpnet', shading=dict(enabled=True))
    batch = support.batch(1, 64, 96, seed=9, mask_mode='bern')
    model.eval()
    with torch.no_grad(), ops.deterministic_mode():
        res = model.forward(dict(batch))
        assert res.get('pred_normal') is None and 'normal_geo' not in res
        normal = ops.depth_normals(res['pred_depth'], batch['K'], ab=batch['abvalue'], mask=batch['mask'], target_type=model._target_type())[0]
        light, stats = ops.shading_fit(model._views(batch)[0], normal, batch['mask'])
        assert _same_bits(res['light'], light) and _same_bits(res['shading_stats'], stats)
        model.option.reconstruct = Option(dict(enabled=True))
        both = model.forward(dict(batch))
        assert _same_bits(both['normal_geo'], normal) and _same_bits(both['light'], light)
    opt = support.option('eval_faceDP_dpnet')
    opt.shading = Option(dict(enabled=True, normals='predicted'))
    with pytest.raises(NotImplementedError, match='dpnet'):
        plugins.DPNET(opt)


def test_the_report_accumulates_on_the_device_and_the_trainer_reads_it_once(tmp_path):
    from dualpixelface_amd import ops, shading
    from dualpixelface_amd.config import Option
    from dualpixelface_amd.trainer import Trainer
    opt = support.option('eval_faceDP')
    opt.shading = Option(dict(enabled=True, report=True, normals='batch', ridge=0.0))
    model = support.build('STEREODPNET', opt)
    batches = [{k: v.cpu() for k, v in _scene_batch(opt, support.batch(1, 64, 96, seed=s, mask_mode='bern'), 64, 96).items()} for s in (3, 4)]
    del batches[1]['albedo']
    trainer = Trainer(opt, workspace_path=str(tmp_path), rank=0, world_size=1)
    with ops.deterministic_mode():
        rows = trainer.validate(model, batches)
        assert model.shading_table is None
        report = trainer.shading_report
        print('report: %s' % (report,))
        assert report['samples'] == 2 and report['albedo_samples'] == 1 and all(0 <= v <= 1e-6 for v in report['albedo_error'])
        assert all(0 <= v < 1e-3 for v in report['rms_residual']) and trainer.history[-1]['shading_report'] == report
        opt.shading = Option(dict(enabled=True, report=False, normals='batch', ridge=0.0))
        assert trainer.validate(model, batches) == rows and trainer.shading_report is None


def test_main_evaluates_the_relight_config():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, 'main.py', '--config', 'eval_faceDP_relight', '--workspace', 'pytest_relight', '--synthetic', '4', '--height',
                        '64', '--width', '96'], cwd=root, env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'shading:' in r.stdout and 'rms_residual' in r.stdout, r.stdout[-2000:]
