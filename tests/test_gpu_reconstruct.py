"""The camera-space surface on the GPU (run with ``-m gpu``): csrc/reconstruct.hip through ops.backproject / depth_normals / depth_mesh, through
the plugins' evaluation forward and through the trainer's test pass, against the numpy restatement of tests/reconstruct_cpu.py.

Bars.  Integer outputs (valid, normal_valid, counts, faces, the order of the vertices) equal the fp32 restatement exactly, nothing
excluded; the scenes keep every comparison at least 1e-4 relative from its threshold in fp64 (asserted per case).  Points and vertices:
max |P - P64| <= 2 x (the fp32 restatement's own max deviation from fp64) + 2 ulp of the largest coordinate.  Normals: the angle to the fp64
restatement <= 2 x the fp32 restatement's worst angle + 1e-6 rad.  Colours: exact, the scenes keep 255 (v std + mean) 1e-3 from a tie.
Measured on an MI355X: DESIGN.md section 7.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import reconstruct_cpu as rc
from tests import support
from tests.support import DEV, ptr, stream

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH_CASES = [(c, s) for c in rc.CASES for s in c[7]]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _operands(ref):
    sc = ref['sc']
    pred = _dev(sc['pred']).unsqueeze(1)
    ab = None if sc['target_type'] == 'depth' else _dev(sc['ab'])
    kw = dict(ab=ab, mask=_dev(sc['mask']), target_type=sc['target_type'], near=ref['near'], far=ref['far'])
    return pred, _dev(sc['K']), kw


# ---- 1. against the restatement
@pytest.mark.parametrize('case', rc.CASES, ids=rc.case_id)
def test_backproject(case):
    ref = rc.case(case)
    assert ref['margin'] >= 1e-4 and ref['agree']
    pred, K, kw = _operands(ref)
    points, valid = support.ops().backproject(pred, K, **kw)
    assert points.dtype == torch.float32 and valid.dtype == torch.uint8 and points.shape == (case[0], 3, case[1], case[2])
    assert np.array_equal(valid.cpu().numpy(), ref['valid'])
    own = float(np.abs(ref['P32'] - ref['P64']).max())
    bar = 2.0 * own + 2.0 * support.ulp_of_max(ref['P64'])
    err = float(np.abs(points.cpu().numpy().astype(np.float64) - ref['P64']).max())
    bits = bool(np.array_equal(points.cpu().numpy(), ref['P32']))
    print('backproject %s: max |P - P64| %.3e (bar %.3e = 2 x %.3e + 2 ulp), equal to the fp32 restatement bit for bit: %s, valid %.2f'
          % (rc.case_id(case), err, bar, own, bits, ref['valid'].mean()))
    assert err <= bar
    assert not points.cpu().numpy()[np.broadcast_to(ref['valid'][:, None] == 0, points.shape)].any()      # 0 where invalid


@pytest.mark.parametrize('case', rc.CASES, ids=rc.case_id)
def test_depth_normals(case):
    ref = rc.case(case)
    pred, K, kw = _operands(ref)
    normal, nvalid = support.ops().depth_normals(pred, K, max_edge_ratio=ref['ratio'], **kw)
    assert normal.dtype == torch.float32 and nvalid.dtype == torch.uint8 and normal.shape == (case[0], 3, case[1], case[2])
    assert np.array_equal(nvalid.cpu().numpy(), ref['nvalid'])
    n = np.moveaxis(normal.cpu().numpy(), 1, -1)
    on = ref['nvalid'] > 0
    assert not n[~on].any()
    if on.any():
        n32, n64 = np.moveaxis(ref['n32'], 1, -1)[on], np.moveaxis(ref['n64'], 1, -1)[on]
        own = float(rc.angle(n32, n64).max())
        err = float(rc.angle(n[on], n64).max())
        print('depth_normals %s: worst angle to fp64 %.3e rad (bar 2 x %.3e + 1e-6), %d normals' % (rc.case_id(case), err, own, on.sum()))
        assert err <= 2.0 * own + 1e-6
        assert float(np.abs(np.linalg.norm(n[on].astype(np.float64), axis=-1) - 1.0).max()) <= 3e-7
    away, avalid = support.ops().depth_normals(pred, K, max_edge_ratio=ref['ratio'], towards_camera=False, **kw)
    assert torch.equal(avalid, nvalid) and torch.equal(away, -normal)


@pytest.mark.parametrize('case,stride', MESH_CASES, ids=lambda v: rc.case_id(v) if isinstance(v, tuple) else 's%d' % v)
def test_depth_mesh(case, stride):
    ref = rc.case(case)
    sc = ref['sc']
    B, H, W = case[:3]
    pred, K, kw = _operands(ref)
    nmap, view = _dev(ref['n32']), _dev(sc['view'])
    Hs, Ws = -(-H // stride), -(-W // stride)
    # buffers of this test's own, pre-filled: what lies past the counts must come back untouched
    out = (torch.full((B, Hs * Ws, 3), -7.0, device=DEV), torch.full((B, Hs * Ws, 3), -7.0, device=DEV),
           torch.full((B, Hs * Ws, 3), 7, dtype=torch.uint8, device=DEV),
           torch.full((B, 2 * (Hs - 1) * (Ws - 1), 3), -7, dtype=torch.int32, device=DEV), torch.full((B, 2), -7, dtype=torch.int32, device=DEV))
    got = support.ops().depth_mesh(pred, K, nmap, view=view, stride=stride, max_edge_ratio=ref['ratio'], out=out, **kw)
    assert all(g is o for g, o in zip(got, out))
    vertices, vnormals, vcolours, faces, counts = [t.cpu().numpy() for t in got]
    worst = 0.0
    for b, (v32, n32, c32, f32) in enumerate(ref['mesh32'][stride]):
        v64 = ref['mesh64'][stride][b][0]
        nv, nf = counts[b]
        assert (nv, nf) == (len(v32), len(f32)), (b, counts[b], len(v32), len(f32))
        assert np.array_equal(faces[b, :nf], f32)
        assert np.array_equal(vcolours[b, :nv], c32) and np.array_equal(vnormals[b, :nv], n32)
        bar = 2.0 * float(np.abs(v32.astype(np.float64) - v64).max() if nv else 0.0) + 2.0 * support.ulp_of_max(v64)
        err = float(np.abs(vertices[b, :nv].astype(np.float64) - v64).max()) if nv else 0.0
        worst = max(worst, err - bar)
        assert err <= bar, (b, err, bar)                             # (vertex k of the kernel is vertex k of the restatement: the order)
        assert (vertices[b, nv:] == -7.0).all() and (vnormals[b, nv:] == -7.0).all() and (vcolours[b, nv:] == 7).all()
        assert (faces[b, nf:] == -7).all()
    print('depth_mesh %s stride %d: counts %s, worst (error - bar) %.3e' % (rc.case_id(case), stride, counts.tolist(), worst))
    # the other winding: the last two indices of every face swapped, nothing else
    back = support.ops().depth_mesh(pred, K, nmap, view=None, stride=stride, max_edge_ratio=ref['ratio'], towards_camera=False, **kw)
    assert torch.equal(back[4], got[4])
    for b, (nv, nf) in enumerate(counts):
        assert torch.equal(back[3][b, :nf], got[3][b, :nf][:, [0, 2, 1]]) and torch.equal(back[0][b, :nv], got[0][b, :nv])
        assert bool((back[2][b, :nv] == 255).all())                  # no view: white


def test_tilted_plane_and_what_differencing_stored_points_would_cost():
    """800 mm, f = 5000 px, fp32 depth: the kernel's normals against the fp64 restatement on the same fp32 depth, within the bar of
    test_depth_normals; printed for information, the same normals from central differences of the stored fp32 points."""
    sc, n_true = rc.tilted_plane()
    pred, K = _dev(sc['pred']).unsqueeze(1), _dev(sc['K'])
    normal, nvalid = support.ops().depth_normals(pred, K, target_type='depth')
    points, _ = support.ops().backproject(pred, K, target_type='depth')
    assert bool(nvalid.all())
    n = np.moveaxis(normal.cpu().numpy(), 1, -1)
    n64, _ = rc.depth_normals(sc['pred'], 'depth', None, sc['K'], None, dt=np.float64)
    n32, _ = rc.depth_normals(sc['pred'], 'depth', None, sc['K'], None, dt=np.float32)
    n64, n32 = np.moveaxis(n64, 1, -1), np.moveaxis(n32, 1, -1)
    own, err = float(rc.angle(n32, n64).max()), float(rc.angle(n, n64).max())
    P = points.cpu().numpy()[0]                                      # fp32 differences of fp32 points, interior pixels
    dr, dc = P[:, 1:-1, 2:] - P[:, 1:-1, :-2], P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
    naive = np.cross(np.moveaxis(dr, 0, -1), np.moveaxis(dc, 0, -1))
    naive = -naive / np.linalg.norm(naive, axis=-1, keepdims=True)
    stored = float(rc.angle(naive, n64[0, 1:-1, 1:-1]).max())
    print('tilted plane: kernel to fp64 %.3e rad (bar 2 x %.3e + 1e-6); differencing stored fp32 points %.3e rad; the fp32 depth itself '
          'against the analytic normal %.3e rad' % (err, own, stored, float(rc.angle(n64, n_true).max())))
    assert err <= 2.0 * own + 1e-6


# ---- 2. the same bits every time
def test_repeats_bit_for_bit_whatever_the_workspace_holds():
    ops = support.ops()
    ref = rc.case(rc.CASES[2])
    pred, K, kw = _operands(ref)
    nmap, view = _dev(ref['n32']), _dev(ref['sc']['view'])

    def run():
        return ops.backproject(pred, K, **kw) + ops.depth_normals(pred, K, **kw) + ops.depth_mesh(pred, K, nmap, view=view, stride=2, **kw)

    first = run()
    mine = [buf for key, buf in ops._scratch.items() if key[1] == 'reconstruct']
    assert mine
    for fill in (float('nan'), 1e30):
        for buf in mine:
            buf.fill_(fill)
        again = run()
        counts = first[-1].cpu().tolist()
        for name, a, b in zip(('points', 'valid', 'normal', 'normal_valid'), first[:4], again[:4]):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), name
        assert torch.equal(first[-1], again[-1])
        for s, (nv, nf) in enumerate(counts):
            for a, b, k in zip(first[4:8], again[4:8], (nv, nv, nv, nf)):
                assert torch.equal(a[s, :k].contiguous().view(torch.uint8), b[s, :k].contiguous().view(torch.uint8))


def test_calls_replay_from_a_graph():
    ops = support.ops()
    ref = rc.case(rc.CASES[2])
    pred, K, kw = _operands(ref)
    nmap = _dev(ref['n32'])
    eager = ops.depth_mesh(pred, K, nmap, stride=1, **kw)
    sp = pred.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                 # the side stream's scratch exists before the capture
        ops.depth_mesh(sp, K, nmap, stride=1, **kw)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        points, valid = ops.backproject(sp, K, **kw)
        normal, nvalid = ops.depth_normals(sp, K, **kw)
        mesh = ops.depth_mesh(sp, K, nmap, stride=1, **kw)
    other = (pred * 1.01).contiguous()
    want = ops.backproject(other, K, **kw) + ops.depth_normals(other, K, **kw)
    want_mesh = ops.depth_mesh(other, K, nmap, stride=1, **kw)
    for source, w, wm in ((other, want, want_mesh), (pred, None, eager)):
        sp.copy_(source)
        graph.replay()
        torch.cuda.synchronize()
        if w is not None:
            assert torch.equal(points, w[0]) and torch.equal(valid, w[1]) and torch.equal(normal, w[2]) and torch.equal(nvalid, w[3])
        assert torch.equal(mesh[4], wm[4])
        for s, (nv, nf) in enumerate(wm[4].cpu().tolist()):
            assert torch.equal(mesh[0][s, :nv], wm[0][s, :nv]) and torch.equal(mesh[3][s, :nf], wm[3][s, :nf])


# ---- 3. refusals
def test_abi_refusals_launch_nothing():
    from dualpixelface_amd._lib import lib, DpfError
    B, H, W, s = 2, 9, 12, 2
    Hs, Ws = 5, 6
    pred = torch.full((B, H, W), 800.0, device=DEV)
    ab = torch.tensor([[0.0, 1.0]] * B, device=DEV)
    K = torch.eye(3, device=DEV).repeat(B, 1, 1).contiguous()
    mask = torch.ones(B, H, W, device=DEV)
    nmap = torch.zeros(B, 3, H, W, device=DEV)
    outs = dict(points=torch.full((B, 3, H, W), -7.0, device=DEV), valid=torch.full((B, H, W), 7, dtype=torch.uint8, device=DEV),
                normal=torch.full((B, 3, H, W), -7.0, device=DEV), nvalid=torch.full((B, H, W), 7, dtype=torch.uint8, device=DEV),
                vertices=torch.full((B, Hs * Ws, 3), -7.0, device=DEV), vnormals=torch.full((B, Hs * Ws, 3), -7.0, device=DEV),
                vcolours=torch.full((B, Hs * Ws, 3), 7, dtype=torch.uint8, device=DEV),
                faces=torch.full((B, 2 * (Hs - 1) * (Ws - 1), 3), -7, dtype=torch.int32, device=DEV),
                counts=torch.full((B, 2), -7, dtype=torch.int32, device=DEV))
    query = 'dpf_depth_mesh_workspace_bytes'
    nbytes = lib().call(query, B, H, W, s)
    assert nbytes == 4 * (4 * B * 1 + B * Hs * Ws) and nbytes % 8 == 0
    assert lib().call(query, 1, 5, 7, 1) == 4 * (4 + 35) + 4          # 156 -> 160: rounded up to 8 bytes
    for bad in ((0, H, W, s), (B, 0, W, s), (B, H, -1, s), (B, H, W, 0), (B, H, W, 3), (B, H, W, 16), (65536, H, W, s), (1, 65536, 32768, 1)):
        assert lib().call(query, *bad) == -1, bad
    ws = torch.full((nbytes // 4 + 2,), -7.0, device=DEV)
    norm = (ctypes.c_float * 6)(*(rc.MEAN + rc.STD))
    good = dict(pred=ptr(pred), pstride=H * W, tt=0, ab=ptr(ab), K=ptr(K), mask=ptr(mask), B=B, H=H, W=W, near=0.0, far=float('inf'),
                ratio=0.01, towards=1, nmap=ptr(nmap), view=None, norm=norm, stride=s, ws=ptr(ws), nbytes=nbytes,
                **{k: ptr(v) for k, v in outs.items()})

    def head(a):
        return (a['pred'], a['pstride'], a['tt'], a['ab'], a['K'], a['mask'])

    def backproject(a):
        lib().call('dpf_backproject', *head(a), a['B'], a['H'], a['W'], a['near'], a['far'], a['points'], a['valid'], stream())

    def normals(a):
        lib().call('dpf_depth_normals', *head(a), a['B'], a['H'], a['W'], a['near'], a['far'], a['ratio'], a['towards'], a['normal'],
                   a['nvalid'], stream())

    def mesh(a):
        lib().call('dpf_depth_mesh', *head(a), a['nmap'], a['view'], a['norm'], a['B'], a['H'], a['W'], a['stride'], a['near'], a['far'],
                   a['ratio'], a['towards'], a['ws'], a['nbytes'], a['vertices'], a['vnormals'], a['vcolours'], a['faces'], a['counts'],
                   stream())

    shared = [dict(pred=None), dict(K=None), dict(ab=None), dict(B=0), dict(H=0), dict(W=-3), dict(tt=3), dict(tt=-1), dict(pstride=H * W - 1),
              dict(near=-1.0), dict(near=float('nan')), dict(far=0.0), dict(far=float('nan')), dict(near=5.0, far=5.0)]
    invalid = {backproject: shared + [dict(points=None), dict(valid=None)],
               normals: shared + [dict(normal=None), dict(nvalid=None), dict(ratio=0.0), dict(ratio=-0.01), dict(ratio=float('nan'))],
               mesh: shared + [dict(nmap=None), dict(view=ptr(nmap), norm=None), dict(ws=None), dict(vertices=None), dict(vnormals=None),
                               dict(vcolours=None), dict(faces=None), dict(counts=None), dict(ratio=0.0), dict(stride=0), dict(stride=-2),
                               dict(nbytes=nbytes - 8), dict(ws=ctypes.c_void_p(ws.data_ptr() + 4))]}
    unsupported = {backproject: [dict(B=65536)], normals: [dict(B=65536)], mesh: [dict(B=65536), dict(stride=3), dict(stride=16)]}
    for table, code in ((invalid, 'DPF_ERR_INVALID_ARG'), (unsupported, 'DPF_ERR_UNSUPPORTED')):
        for fn, cases in table.items():
            for over in cases:
                with pytest.raises(DpfError, match=code):
                    fn(dict(good, **over))
    torch.cuda.synchronize()
    for name, t in outs.items():
        assert bool((t == (7 if t.dtype == torch.uint8 else -7)).all()), name
    assert bool((ws == -7.0).all())
    for fn in (backproject, normals, mesh):                           # and the arguments they were derived from do run
        fn(good)
    backproject(dict(good, tt=2, ab=None))                            # a depth target needs no ab
    torch.cuda.synchronize()
    assert bool(outs['valid'].all()) and bool(outs['nvalid'].all()) and outs['counts'].cpu().tolist() == [[Hs * Ws, 2 * (Hs - 1) * (Ws - 1)]] * B
    assert bool((outs['points'][:, 2] == 800.0).all())


def test_ops_refuse_what_does_not_fit():
    from dualpixelface_amd._lib import DpfError
    ops = support.ops()
    pred, K, ab = torch.ones(2, 1, 8, 12, device=DEV), torch.eye(3, device=DEV).repeat(2, 1, 1), torch.ones(2, 2, device=DEV)
    nmap = torch.zeros(2, 3, 8, 12, device=DEV)
    for kw in (dict(Kmat=K[:1]), dict(ab=ab[:1]), dict(mask=torch.ones(2, 8, 11, device=DEV)), dict(ab=None)):
        args = dict(dict(Kmat=K, ab=ab), **kw)
        with pytest.raises(DpfError, match='does not match|needs ab'):
            ops.backproject(pred, **args)
        with pytest.raises(DpfError, match='does not match|needs ab'):
            ops.depth_normals(pred, **args)
    with pytest.raises(DpfError, match='does not match'):
        ops.depth_mesh(pred, K, nmap[:, :, :4], ab=ab)
    with pytest.raises(DpfError, match='does not match'):
        ops.depth_mesh(pred, K, nmap, ab=ab, view=nmap[:, :2])
    with pytest.raises(DpfError, match='not supported'):
        ops.depth_mesh(pred, K, nmap, ab=ab, stride=3)
    with pytest.raises(DpfError, match='dtype'):
        ops.backproject(pred.double(), K, ab=ab)
    with pytest.raises(DpfError, match='DPF_ERR_INVALID_ARG'):
        ops.backproject(pred, K, ab=ab, near=3.0, far=2.0)
    points, _ = ops.backproject(pred.requires_grad_(), K, ab=ab)       # detached, not an autograd node
    assert not points.requires_grad and points.grad_fn is None
    wide = torch.ones(2, 3, 8, 12, device=DEV)                       # head 0 of a wider prediction is read through the batch stride
    wide[:, 1:] = float('nan')
    assert torch.equal(ops.backproject(wide, K, ab=ab)[0], points)


# ---- 4. the whole path
def _model_with_reconstruct(cls_name, config, **block):
    from dualpixelface_amd.config import Option
    opt = support.option(config)
    opt.reconstruct = Option(dict(block))
    return support.build(cls_name, opt)


def _rays(K, H, W):
    inv, _ = rc.kinv(K.cpu().numpy())
    return torch.from_numpy(rc.rays(inv.astype(np.float32), H, W, np.float32)).to(DEV)


def test_stereodpnet_evaluation_attaches_the_surface():
    from dualpixelface_amd import metrics, ops, reconstruct
    model = _model_with_reconstruct('STEREODPNET', 'eval_faceDP', enabled=False)
    batch = support.batch(1, 64, 96, seed=9, mask_mode='bern')
    model.eval()
    with torch.no_grad(), ops.deterministic_mode():
        off = model.forward(dict(batch))
        model.option.reconstruct.enabled = True
        on = model.forward(dict(batch))
        assert set(on) == set(off) | set(reconstruct.RESULT_KEYS) and not set(off) & set(reconstruct.RESULT_KEYS)
        for k in off:
            assert off[k] is None and on[k] is None or torch.equal(off[k], on[k]), k
        depth = metrics.disp2depth(on['pred_depth'][:, :1], batch['abvalue'])[:, 0]
        valid = on['points_valid'].bool()
        assert torch.equal(valid, (depth > 0) & (batch['mask'] > 0))
        want = torch.where(valid.unsqueeze(1), depth.unsqueeze(1) * _rays(batch['K'], 64, 96), torch.zeros(()).to(DEV))
        assert torch.equal(on['points'], want)
        print('stereodpnet: %d valid points, %d geometric normals of %d pixels' % (int(valid.sum()), int(on['normal_geo_valid'].sum()), 64 * 96))
        assert on['points'].shape == (1, 3, 64, 96) and on['normal_geo'].shape == (1, 3, 64, 96)
        # "auto": the mesh carries head 0 of the network's normals, "geometric" those of the depth
        (v, n, c, f), = reconstruct.extract(model.option, on, batch, guide=batch['left'])
        sel = valid[0].cpu().numpy()
        assert np.array_equal(n, np.moveaxis(on['pred_normal'][0, 0].cpu().numpy(), 0, -1)[sel]) and len(v) == sel.sum()
        model.option.reconstruct.normals = 'geometric'
        (_, n, _, _), = reconstruct.extract(model.option, on, batch, guide=batch['left'])
        assert np.array_equal(n, np.moveaxis(on['normal_geo'][0].cpu().numpy(), 0, -1)[sel])
        # both blocks on: the surface is the filtered map's
        model.option.post_process.use_guided = True
        both = model.forward(dict(batch))
        model.option.post_process.use_guided = False
        assert not torch.equal(both['pred_depth'], on['pred_depth']) and torch.equal(both['pred_depth_raw'], on['pred_depth'])
        points, pvalid = ops.backproject(both['pred_depth'], batch['K'], ab=batch['abvalue'], mask=batch['mask'])
        assert torch.equal(both['points'], points) and torch.equal(both['points_valid'], pvalid) and not torch.equal(points, on['points'])
    # training mode: nothing is attached, whatever the block says
    with ops.deterministic_mode():
        model.train()
        res = model.forward(dict(batch))
    assert not set(res) & set(reconstruct.RESULT_KEYS) and res['pred_depth'].requires_grad


def test_a_model_without_a_normal_head_gets_geometric_normals():
    from dualpixelface_amd import ops, reconstruct
    model = _model_with_reconstruct('DPNET', 'eval_faceDP_dpnet', enabled=True)
    batch = support.batch(1, 64, 96, seed=9, mask_mode='bern')
    model.eval()
    with torch.no_grad(), ops.deterministic_mode():
        res = model.forward(dict(batch))
        assert res.get('pred_normal') is None and set(reconstruct.RESULT_KEYS) <= set(res)
        normal, nvalid = ops.depth_normals(res['pred_depth'], batch['K'], ab=batch['abvalue'], mask=batch['mask'],
                                           target_type=model._target_type())
        assert torch.equal(res['normal_geo'], normal) and torch.equal(res['normal_geo_valid'], nvalid)
        (v, n, c, f), = reconstruct.extract(model.option, res, batch)
        sel = res['points_valid'][0].bool().cpu().numpy()
        assert np.array_equal(n, np.moveaxis(normal[0].cpu().numpy(), 0, -1)[sel])
        model.option.reconstruct.normals = 'predicted'
        with pytest.raises(NotImplementedError, match='pred_normal'):
            model.forward(dict(batch))
        model.option.reconstruct.normals = 'auto'
        # a batch without abvalue (this model builds no coordinate volume from it): placed with the evaluation-time fit
        fitted = model.forward({k: v for k, v in batch.items() if k != 'abvalue'})
        assert 'abvalue' in fitted and 'abvalue' not in res
        points, _ = ops.backproject(fitted['pred_depth'], batch['K'], ab=fitted['abvalue'], mask=batch['mask'], target_type=model._target_type())
        assert torch.equal(fitted['points'], points)
        with pytest.raises(NotImplementedError, match=r"batch\['K'\]"):
            model.forward({k: v for k, v in batch.items() if k != 'K'})


def test_trainer_test_pass_writes_one_ply_per_sample(tmp_path):
    from dualpixelface_amd import ops, reconstruct
    from dualpixelface_amd.synthetic_data import synthetic_loader
    from dualpixelface_amd.trainer import Trainer
    model = _model_with_reconstruct('STEREODPNET', 'eval_faceDP', write_ply=True, stride=2)
    model.option.mode = 'test'
    loader = synthetic_loader(3, 64, 96, 2, seed=4)                   # two batches: two samples, then one
    trainer = Trainer(model.option, str(tmp_path), rank=0, world_size=1)
    with ops.deterministic_mode():
        trainer.test(model, loader)
        folder = os.path.join(str(tmp_path), 'output', 'recon')
        assert sorted(os.listdir(folder)) == ['0_0.ply', '0_1.ply', '1_0.ply']
        assert sorted(trainer.written_meshes) == sorted(os.path.join(folder, n) for n in os.listdir(folder))
        model.eval()
        with torch.no_grad():
            for i, batch in enumerate(loader):
                batch = {k: v.to(DEV) for k, v in batch.items()}
                meshes = reconstruct.extract(model.option, model.forward(dict(batch)), batch, guide=model._views(batch)[0])
                for b, (v, n, c, f) in enumerate(meshes):
                    got = rc.read_ply(os.path.join(folder, '%d_%d.ply' % (i, b)))
                    assert np.array_equal(got['vertices'], v) and np.array_equal(got['normals'], n)
                    assert np.array_equal(got['colours'], c) and np.array_equal(got['faces'], f)
                    print('%d_%d.ply: %d vertices, %d faces, %d bytes' % (i, b, len(v), len(f), got['nbytes']))
                    assert len(v) <= 32 * 48 and (len(f) == 0 or f.max() < len(v))
        # validation (also during fit) and a test pass without write_ply write nothing
        for n in os.listdir(folder):
            os.remove(os.path.join(folder, n))
        trainer.validate(model, loader)
        model.option.reconstruct.write_ply = False
        trainer.test(model, loader)
        assert os.listdir(folder) == [] and trainer.written_meshes == []
        model.option.output_path = str(tmp_path / 'elsewhere')
        model.option.reconstruct.write_ply = True
        trainer.test(model, loader)
        assert len(os.listdir(os.path.join(str(tmp_path), 'elsewhere', 'recon'))) == 3 and os.listdir(folder) == []


def test_main_writes_the_meshes_of_the_mesh_config():
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, 'main.py', '--config', 'eval_faceDP_mesh', '--workspace', 'pytest_mesh', '--synthetic', '4', '--height', '64',
                        '--width', '96'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    folder = os.path.join(ROOT, 'workspace', 'stereodpnet', 'pytest_mesh', 'output', 'recon')
    names = sorted(os.listdir(folder))
    assert names == ['0_0.ply', '1_0.ply', '2_0.ply', '3_0.ply']
    for n in names:
        got = rc.read_ply(os.path.join(folder, n))
        assert len(got['vertices']) <= 32 * 48 and (len(got['faces']) == 0 or got['faces'].max() < len(got['vertices']))
