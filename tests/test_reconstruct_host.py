"""The reconstruct block on the host (no GPU): reconstruct.settings / apply / write_ply, the operators' refusals, and the closed forms that tie
the restatement of tests/reconstruct_cpu.py to the definitions it restates."""
import json
import os

import numpy as np
import pytest
import torch

from tests import reconstruct_cpu as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = (False, False, 1, 0.0, None, 0.01, True, 'auto', True, True)


class _Opt(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _rec():
    from dualpixelface_amd import reconstruct
    return reconstruct


# ---- settings
def test_settings_defaults_for_a_missing_block_and_missing_keys():
    rec = _rec()
    assert tuple(rec.settings(_Opt())) == DEFAULTS and tuple(rec.settings(_Opt(reconstruct=None))) == DEFAULTS
    assert tuple(rec.settings(_Opt(reconstruct={}))) == DEFAULTS and tuple(rec.DEFAULTS) == DEFAULTS
    assert rec.Settings._fields == ('enabled', 'write_ply', 'stride', 'near', 'far', 'max_edge_ratio', 'use_mask', 'normals', 'towards_camera',
                                    'colour')
    s = rec.settings(_Opt(reconstruct={'enabled': True, 'stride': 4, 'far': 1200}))
    assert s.enabled and not s.write_ply and s.stride == 4 and s.far == 1200.0 and isinstance(s.far, float) and s.near == 0.0
    s = rec.settings(_Opt(reconstruct=_Opt(write_ply=True, normals='geometric', near=100)))             # an attribute block
    assert s.enabled and s.write_ply and s.normals == 'geometric' and s.near == 100.0
    assert rec.active(_Opt(reconstruct={'write_ply': True})) and rec.active(_Opt(reconstruct={'enabled': True})) and not rec.active(_Opt())
    assert not rec.active(_Opt(reconstruct={'stride': 2}))


@pytest.mark.parametrize('key,value', [
    ('enabled', 1), ('enabled', 'true'), ('write_ply', 0), ('write_ply', None), ('use_mask', 'yes'), ('towards_camera', 1), ('colour', None),
    ('stride', 3), ('stride', 0), ('stride', 16), ('stride', 2.0), ('stride', True), ('stride', '2'),
    ('near', -1.0), ('near', None), ('near', 'close'), ('near', float('nan')), ('near', True), ('near', float('inf')),
    ('far', 0.0), ('far', -5), ('far', 'inf'), ('far', float('nan')), ('far', False),
    ('max_edge_ratio', 0), ('max_edge_ratio', -0.01), ('max_edge_ratio', None), ('max_edge_ratio', '0.01'), ('max_edge_ratio', float('inf')),
    ('normals', 'network'), ('normals', None), ('normals', True)])
def test_settings_names_the_malformed_key(key, value):
    with pytest.raises(ValueError, match=key):
        _rec().settings(_Opt(reconstruct={key: value}))


def test_settings_far_must_exceed_near_and_a_non_block_is_refused():
    rec = _rec()
    with pytest.raises(ValueError, match='far'):
        rec.settings(_Opt(reconstruct={'near': 500.0, 'far': 500.0}))
    assert rec.settings(_Opt(reconstruct={'near': 500.0, 'far': 500.5})).far == 500.5
    for bad in (True, 3, 'on', [1]):
        with pytest.raises(ValueError, match='reconstruct'):
            rec.settings(_Opt(reconstruct=bad))


# ---- configs
def test_mesh_config_is_eval_faceDP_with_the_block_spelled_out():
    base = json.load(open(os.path.join(ROOT, 'config_', 'eval_faceDP.json')))
    ours = json.load(open(os.path.join(ROOT, 'config_', 'eval_faceDP_mesh.json')))
    block = ours.pop('reconstruct')
    assert set(block) == set(_rec().Settings._fields)
    assert block == dict(zip(_rec().Settings._fields, DEFAULTS), enabled=True, write_ply=True, stride=2)
    assert 'reconstruct' not in base and ours == base
    assert ours['post_process'] == {'use_bilateral': False, 'use_guided': False}


def test_every_other_shipped_config_is_inactive():
    from dualpixelface_amd import load_option
    rec = _rec()
    names = sorted(f[:-5] for f in os.listdir(os.path.join(ROOT, 'config_')) if f.endswith('.json'))
    assert 'eval_faceDP_mesh' in names and 'eval_faceDP' in names and 'train_faceDP' in names
    for name in names:
        s = rec.settings(load_option(name))
        if name == 'eval_faceDP_mesh':
            assert tuple(s) == (True, True, 2) + DEFAULTS[3:]
        else:
            assert tuple(s) == DEFAULTS, name


# ---- apply
def test_apply_off_or_training_returns_results_untouched():
    rec = _rec()
    pred = torch.zeros(1, 1, 4, 4)
    results = {'pred_depth': pred}
    for opt, training in ((_Opt(), False), (_Opt(reconstruct={'enabled': False, 'stride': 2}), False),
                          (_Opt(reconstruct={'enabled': True}), True), (_Opt(reconstruct={'write_ply': True}), True)):
        out = rec.apply(opt, results, {}, training=training)         # no K in the batch: nothing looks for one
        assert out is results and list(results) == ['pred_depth'] and results['pred_depth'] is pred


def test_apply_on_names_what_is_missing_and_leaves_results_alone():
    rec = _rec()
    pred = torch.zeros(1, 1, 4, 6)
    K, ab = torch.eye(3).unsqueeze(0), torch.tensor([[1.0, 2.0]])
    on = {'enabled': True}

    def check(opt, results, batch, match):
        before = dict(results)
        with pytest.raises(NotImplementedError, match=match):
            rec.apply(opt, results, batch)
        assert list(results) == list(before) and all(results[k] is before[k] for k in before)

    check(_Opt(reconstruct=on), {'pred_depth': pred}, {'abvalue': ab}, r"batch\['K'\]")
    check(_Opt(reconstruct=on), {'pred_depth': pred}, {'K': K}, 'abvalue')
    check(_Opt(reconstruct=on, model=_Opt(target_type='idepth')), {'pred_depth': pred}, {'K': K}, 'abvalue')
    check(_Opt(reconstruct=on), {'pred_depth': None}, {'K': K, 'abvalue': ab}, 'pred_depth')
    check(_Opt(reconstruct=dict(on, normals='predicted')), {'pred_depth': pred}, {'K': K, 'abvalue': ab}, 'pred_normal')
    # everything there: the operator is reached, and refuses the CPU tensors (a depth model needs no abvalue)
    from dualpixelface_amd._lib import DpfError
    for opt, batch in ((_Opt(reconstruct=on), {'K': K, 'abvalue': ab}), (_Opt(reconstruct=on, model=_Opt(target_type='depth')), {'K': K})):
        results = {'pred_depth': pred}
        with pytest.raises(DpfError, match='GPU tensors'):
            rec.apply(opt, results, batch)
        assert list(results) == ['pred_depth']
    results = {'pred_depth': pred, 'abvalue': ab}                    # the evaluation-time fit stands in for batch['abvalue']
    with pytest.raises(DpfError, match='GPU tensors'):
        rec.apply(_Opt(reconstruct=on), results, {'K': K})


def test_ops_refuse_cpu_tensors_and_malformed_operands():
    from dualpixelface_amd import ops
    from dualpixelface_amd._lib import DpfError
    pred, K, ab = torch.zeros(1, 2, 8, 8), torch.eye(3).unsqueeze(0), torch.ones(1, 2)
    nmap = torch.zeros(1, 3, 8, 8)
    with pytest.raises(DpfError, match='GPU tensors'):
        ops.backproject(pred, K, ab=ab)
    with pytest.raises(DpfError, match='GPU tensors'):
        ops.depth_normals(pred, K, ab=ab)
    with pytest.raises(DpfError, match='GPU tensors'):
        ops.depth_mesh(pred, K, nmap, ab=ab)
    with pytest.raises(DpfError, match='target_type'):
        ops.backproject(pred, K, ab=ab, target_type='inverse')
    with pytest.raises(DpfError, match='stride must be an integer'):
        ops.depth_mesh(pred, K, nmap, ab=ab, stride=2.0)


def test_header_declares_the_new_entry_points():
    from dualpixelface_amd import _lib
    protos = _lib.parse_header()
    assert len(protos['dpf_backproject'][1]) == 14 and len(protos['dpf_depth_normals'][1]) == 16
    assert len(protos['dpf_depth_mesh'][1]) == 25 and protos['dpf_depth_mesh_workspace_bytes'][0] is _lib._CTYPES['long long']
    assert [n for _, n in protos['dpf_depth_mesh_workspace_bytes'][1]] == ['B', 'H', 'W', 'stride']
    make = open(os.path.join(ROOT, 'dualpixelface_amd', 'csrc', 'Makefile')).read()
    assert '$(OBJDIR)/reconstruct.o: CXXFLAGS += -ffp-contract=off' in make


# ---- PLY
def test_write_ply_round_trip(tmp_path):
    rec = _rec()
    rng = np.random.RandomState(0)
    V, F = 7, 5
    vertices, normals = rng.randn(V, 3).astype(np.float32), rng.randn(V, 3).astype(np.float32)
    colours = rng.randint(0, 256, (V, 3)).astype(np.uint8)
    faces = rng.randint(0, V, (F, 3)).astype(np.int32)
    path = rec.write_ply(str(tmp_path / 'a.ply'), vertices, normals, colours, faces)
    got = rc.read_ply(path)
    want = ('ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\n'
            'property float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nelement face 5\n'
            'property list uchar int vertex_indices\nend_header\n')
    assert got['header'] == want and got['nbytes'] == len(want) + V * 27 + F * 13
    assert np.array_equal(got['vertices'], vertices) and np.array_equal(got['normals'], normals)
    assert np.array_equal(got['colours'], colours) and np.array_equal(got['faces'], faces)
    raw = open(path, 'rb').read()                                    # the first face record: count byte 3, then three little-endian ints
    off = len(want) + V * 27
    assert raw[off] == 3 and np.array_equal(np.frombuffer(raw[off + 1:off + 13], '<i4'), faces[0])
    empty = rc.read_ply(rec.write_ply(str(tmp_path / 'b.ply'), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3))))
    assert empty['vertices'].shape == (0, 3) and empty['faces'].shape == (0, 3) and 'element vertex 0\n' in empty['header']
    with pytest.raises(ValueError, match='face index'):
        rec.write_ply(str(tmp_path / 'c.ply'), vertices, normals, colours, np.array([[0, 1, V]]))
    with pytest.raises(ValueError, match='normals'):
        rec.write_ply(str(tmp_path / 'c.ply'), vertices, normals[:3], colours, faces)
    assert sorted(os.listdir(str(tmp_path))) == ['a.ply', 'b.ply']


def test_output_dir_prefers_the_options_output_path():
    rec = _rec()
    assert rec.output_dir(_Opt(output_path='/x/out'), '/w') == os.path.join('/x/out', 'recon')
    assert rec.output_dir(_Opt(), '/w') == os.path.join('/w', 'output', 'recon')


# ---- the restatement against closed forms
def _flat(H, W, z=800.0, f=1500.0):
    K = np.array([[[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]]], np.float32)
    return np.full((1, H, W), z, np.float32), K


def test_restatement_kinv_inverts_k_and_flags_a_singular_one():
    rng = np.random.RandomState(3)
    K = rc.camera(3, 40, 60, rng)
    K[1, 1] = 2.0 * K[1, 0]
    inv, ok = rc.kinv(K)
    assert ok.tolist() == [True, False, True] and not inv[1].any()
    for b in (0, 2):
        assert np.abs(inv[b] @ K[b].astype(np.float64) - np.eye(3)).max() <= 1e-12


@pytest.mark.parametrize('dt', [np.float32, np.float64])
def test_restatement_fronto_parallel_plane(dt):
    pred, K = _flat(6, 9)
    for towards, nz in ((True, -1.0), (False, 1.0)):
        n, ok = rc.depth_normals(pred, 'depth', None, K, None, towards_camera=towards, dt=dt)
        assert n.dtype == dt and ok.all()
        assert np.abs(n - np.array([0.0, 0.0, nz]).reshape(1, 3, 1, 1)).max() <= (1e-6 if dt is np.float32 else 1e-12)
    P, valid = rc.backproject(pred, 'depth', None, K, None, dt=dt)
    assert valid.all() and np.all(P[:, 2] == 800.0)
    assert abs(float(P[0, 0, 0, 0]) - 800.0 * (0 - 4.5) / 1500.0) <= 1e-4 and abs(float(P[0, 1, 5, 0]) - 800.0 * (5 - 3.0) / 1500.0) <= 1e-4


def test_restatement_tilted_plane_gives_the_analytic_normal():
    """The step vector is the exact difference of two points of the surface, so on a plane both steps lie in it and the normal is the
    plane's, up to rounding: 1e-9 rad from an fp64 depth.  From the fp32 rounding of that depth: half an ulp of 800 mm (3.05e-5 mm) on each
    end of a step is 1.9e-4 rad per axis for the central step of 2 x 800 / 5000 = 0.32 mm and 3.8e-4 rad for the one-sided step of 0.16 mm
    that the border pixels take; both axes at once, sqrt(2) x 3.8e-4 = 5.4e-4 rad, which is the bar (2.7e-4 away from the border)."""
    sc, n_true = rc.tilted_plane()
    exact = sc['z']                                                  # float64: the restatement keeps it as it is
    n64, ok = rc.depth_normals(exact, 'depth', None, sc['K'], None, dt=np.float64)
    assert ok.all() and float(rc.angle(np.moveaxis(n64, 1, -1), n_true).max()) <= 1e-9
    assert float((n64[:, 2] < 0).all())
    n64r, _ = rc.depth_normals(sc['pred'], 'depth', None, sc['K'], None, dt=np.float64)
    n32, _ = rc.depth_normals(sc['pred'], 'depth', None, sc['K'], None, dt=np.float32)
    from_rounding = float(rc.angle(np.moveaxis(n64r, 1, -1), n_true).max())
    own = float(rc.angle(np.moveaxis(n32, 1, -1), np.moveaxis(n64r, 1, -1)).max())
    inner = float(rc.angle(np.moveaxis(n64r, 1, -1), n_true)[:, 1:-1, 1:-1].max())
    assert 1e-6 < from_rounding <= 5.4e-4 and inner <= 2.7e-4 and own <= 2e-6, (from_rounding, inner, own)
    away, _ = rc.depth_normals(exact, 'depth', None, sc['K'], None, towards_camera=False, dt=np.float64)
    assert np.abs(away + n64).max() == 0.0


def test_restatement_one_sided_steps_at_the_border_and_no_step_for_an_isolated_pixel():
    pred, K = _flat(5, 7)
    pred[0, 2, 3] = 900.0                                            # 12 % off its neighbours: connected to none
    n, ok = rc.depth_normals(pred, 'depth', None, K, None, dt=np.float64)
    assert not ok[0, 2, 3] and not n[0, :, 2, 3].any() and ok.sum() == 5 * 7 - 1
    # its four neighbours take the one-sided step away from it and still see the plane
    assert np.abs(n[0, :, 2, 2] - [0, 0, -1]).max() <= 1e-12 and np.abs(n[0, :, 1, 3] - [0, 0, -1]).max() <= 1e-12
    col = np.full((1, 5, 1), 800.0, np.float32)                     # one column: no row step anywhere
    n, ok = rc.depth_normals(col, 'depth', None, K, None, dt=np.float64)
    assert not ok.any() and not n.any()


def _mesh(pred, K, mask=None, stride=1, ratio=0.01, towards=True, dt=np.float64):
    nmap = np.zeros((pred.shape[0], 3) + pred.shape[1:], np.float32)
    nmap[:, 2] = -1.0
    return rc.depth_mesh(pred, 'depth', None, K, mask, nmap, None, stride=stride, max_edge_ratio=ratio, towards_camera=towards, dt=dt)


def test_restatement_full_grid_winding_and_order():
    pred, K = _flat(3, 4)
    (v, n, c, f), = _mesh(pred, K)
    assert v.shape == (12, 3) and f.shape == (12, 3) and (c == 255).all() and (n == [0, 0, -1]).all()
    assert f[0].tolist() == [0, 4, 1] and f[1].tolist() == [1, 4, 5] and f[2].tolist() == [1, 5, 2]      # quad 0: T0, T1; then quad 1
    face_n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert (face_n[:, 2] < 0).all()                                  # counter-clockwise seen from the camera: the front faces it
    (_, _, _, fb), = _mesh(pred, K, towards=False)
    assert np.array_equal(fb, f[:, [0, 2, 1]])


def test_restatement_one_invalid_pixel_removes_six_triangles_and_one_vertex():
    H, W = 6, 8
    pred, K = _flat(H, W)
    (v0, _, _, f0), = _mesh(pred, K)
    mask = np.ones((1, H, W), np.float32)
    mask[0, 2, 3] = 0.0
    (v1, _, _, f1), = _mesh(pred, K, mask=mask)
    k = 2 * W + 3
    assert len(v0) == H * W and len(f0) == 2 * (H - 1) * (W - 1) and len(v1) == H * W - 1 and len(f1) == len(f0) - 6
    assert (f0 == k).any(1).sum() == 6
    kept = f0[~(f0 == k).any(1)]
    assert np.array_equal(f1, kept - (kept > k))                     # the same faces in the same order, indices past the hole moved down
    assert np.array_equal(v1, np.delete(v0, k, 0))


def test_restatement_a_depth_step_cuts_the_mesh_along_it():
    H, W, c = 5, 9, 4
    pred, K = _flat(H, W)
    pred[..., c:] *= 1.0 + 0.011                                     # 1.1 % against a ratio of 1 %
    (v, _, _, f), = _mesh(pred, K)
    assert len(v) == H * W and len(f) == 2 * (H - 1) * (W - 2)
    left = (f % W) < c
    assert (left.all(1) | (~left).all(1)).all()                      # no triangle has a foot on both sides
    pred2, _ = _flat(H, W)
    pred2[..., c:] *= 1.0 + 0.009                                    # 0.9 %: one surface
    assert len(_mesh(pred2, K)[0][3]) == 2 * (H - 1) * (W - 1)
    n, ok = rc.depth_normals(pred, 'depth', None, K, None, dt=np.float64)
    assert ok.all() and np.abs(n - np.array([0, 0, -1.0]).reshape(1, 3, 1, 1)).max() <= 1e-12     # one-sided at the cut: the step is not seen


@pytest.mark.parametrize('H,W', [(6, 8), (7, 9), (1, 5), (2, 2)])
def test_restatement_stride_two_on_even_and_odd_sizes(H, W):
    pred, K = _flat(H, W)
    pred += np.arange(W, dtype=np.float32)[None, None, :] * 0.25
    (v, _, _, f), = _mesh(pred, K, stride=2)
    Hs, Ws = (H + 1) // 2, (W + 1) // 2
    P, _ = rc.backproject(pred, 'depth', None, K, None, dt=np.float64)
    assert len(v) == Hs * Ws and len(f) == 2 * (Hs - 1) * (Ws - 1)
    assert np.array_equal(v, np.moveaxis(P[0][:, ::2, ::2], 0, -1).reshape(-1, 3))
    assert f.size == 0 or f.max() == Hs * Ws - 1


def test_restatement_fp32_and_fp64_agree_where_the_margins_allow():
    sc = rc.scene(2, 17, 33, seed=3)
    args = (sc['pred'], 'disp', sc['ab'], sc['K'], sc['mask'])
    assert rc.margins(*args, strides=(1, 2)) >= 1e-4
    P32, v32 = rc.backproject(*args, dt=np.float32)
    P64, v64 = rc.backproject(*args, dt=np.float64)
    assert P32.dtype == np.float32 and P64.dtype == np.float64 and np.array_equal(v32, v64) and 0.5 < v32.mean() < 0.85
    assert 0.0 < np.abs(P32 - P64).max() <= 1e-3
    n32, o32 = rc.depth_normals(*args, dt=np.float32)
    n64, o64 = rc.depth_normals(*args, dt=np.float64)
    assert np.array_equal(o32, o64) and 0 < o32.sum() < v32.sum()
    for s in (1, 2):
        m32 = rc.depth_mesh(*args, n32, sc['view'], stride=s, dt=np.float32)
        m64 = rc.depth_mesh(*args, n32, sc['view'], stride=s, dt=np.float64)
        for a, b in zip(m32, m64):
            assert np.array_equal(a[3], b[3]) and np.array_equal(a[2], b[2]) and len(a[0]) == len(b[0]) and len(a[3]) > 0
    assert rc.colour_margin(sc['view']) >= 1e-3
    cols = rc.colours(sc['view'])
    assert cols.min() == 0 and cols.max() == 255


@pytest.mark.parametrize('case', rc.CASES, ids=rc.case_id)
def test_gpu_cases_keep_their_comparisons_off_the_thresholds(case):
    """What tests/test_gpu_reconstruct.py compares exactly must not hang on a rounding: in fp64 no comparison of a case sits within 1e-4
    relative of its threshold (the fp32 evaluation rounds z at the 1e-7 level), so both restatements give the same integers."""
    ref = rc.case(case)
    assert ref['margin'] >= 1e-4 and ref['agree'] and rc.colour_margin(ref['sc']['view']) >= 1e-3
    assert case[6] is None or not ref['valid'][case[6]].any()
    if case[1] * case[2] >= 35:
        assert 0 < ref['valid'].sum() < ref['valid'].size
