"""View coverage without a device: ivx_view_coverage_fwd is declared, bound and exported and rejects bad arguments before any launch;
ops.view_coverage raises its host errors; the numpy reference of tests/ref_view_coverage.py has the properties the definition promises; the
gate's arguments are validated and last_admitted behaves as specified on a session whose device calls are stubbed."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import ref_unproject as R
import ref_unproject_maps as RM
import ref_view_coverage as RC
from helpers import ROOT

NAME = 'ivx_view_coverage_fwd'


def test_entry_point_declared_bound_and_exported():
    from imvoxelnet_amd import _build, _lib
    header = open(os.path.join(ROOT, 'include', 'imvoxel.h')).read()
    declared = set(re.findall(r'\b(ivx_[a-z0-9_]+)\s*\(', header))
    L = _lib.lib()
    assert NAME in declared, f'{NAME} is not declared in include/imvoxel.h'
    assert NAME in _lib.EXPORTS and hasattr(L, NAME) and getattr(L, NAME).argtypes is not None and len(getattr(L, NAME).argtypes) == 11
    assert L.ivx_version() >= 501
    for src in ('model.cpp', 'api_common.cpp'):        # also compiled into the CPU restatement of the ABI, which does not define it
        assert NAME not in open(os.path.join(ROOT, 'imvoxelnet_amd', 'csrc', src)).read(), src
    assert 'view_coverage.hip' in [e[0] for e in _build.SOURCES]
    assert '-ffp-contract=off' in [e[1] for e in _build.SOURCES if e[0] == 'view_coverage.hip'][0]
    for k, v in (('IVX_STATE_NONE', 0), ('IVX_STATE_COUNT', 1), ('IVX_STATE_WSUM', 2), ('IVX_STATE_MASK', 3)):
        assert re.search(rf'#define {k} {v}\b', header), k
    assert (_lib.STATE_NONE, _lib.STATE_COUNT, _lib.STATE_WSUM, _lib.STATE_MASK) == (0, 1, 2, 3)


def _call(L, B=2, V=3, S=4, R=3, fhw=(6, 9), dims=(7, 6, 5), desc=True, lists=True, vs=64, row=128, first=None, maps=None, proj=192, origin=256, crop=320,
          state=384, kind=1, fresh_below=1.0, out=448):
    """The entry with dummy device pointers (never dereferenced: every call here is rejected before anything is launched)."""
    from imvoxelnet_amd import _lib
    d = _lib.BackprojectDesc(B, V, fhw[0], fhw[1], 0, *dims, (ctypes.c_float * 3)(0.25, 0.25, 0.25), 0, 0, 0, 0)
    l = _lib.LiftLists(S, R, vs, row, first)
    m = None if maps is None else ctypes.byref(_lib.LiftMaps(*maps))
    p = lambda a: None if a is None else ctypes.c_void_p(a)     # noqa: E731
    return getattr(L, NAME)(ctypes.byref(d) if desc else None, ctypes.byref(l) if lists else None, m, p(proj), p(origin), p(crop), p(state), kind,
                            fresh_below, p(out), None)


def test_argument_validation_without_gpu():
    """Every pre-launch rejection of the header's list: status -1 with a message that names the entry."""
    from imvoxelnet_amd import _lib
    L = _lib.lib()
    nan, inf = float('nan'), float('inf')
    cases = [dict(desc=False), dict(lists=False), dict(proj=None), dict(vs=None), dict(origin=None), dict(crop=None), dict(out=None)]
    cases += [dict(B=0), dict(B=-1), dict(V=0), dict(S=0), dict(S=-2), dict(R=0), dict(fhw=(0, 9)), dict(fhw=(6, -1)), dict(dims=(0, 6, 5)), dict(dims=(7, -6, 5)),
              dict(dims=(7, 6, 0))]
    cases += [dict(dims=(2048, 1024, 1024)), dict(dims=(1290, 1290, 1291)), dict(S=65536, fhw=(256, 128)), dict(B=1 << 24, V=256, R=1 << 24),
              dict(B=65536, R=65536), dict(V=257)]
    cases += [dict(R=1, row=None), dict(kind=4), dict(kind=-1), dict(state=None, kind=1), dict(state=None, kind=2), dict(state=None, kind=3), dict(state=384, kind=0)]
    cases += [dict(fresh_below=v) for v in (0.0, -1.0, nan, inf, -inf)]
    cases += [dict(first=512)]
    cases += [dict(maps=(None, 576, b, f)) for b, f in ((-0.5, 0.0), (0.0, -1.0), (nan, 0.0), (0.0, nan))]
    for kw in cases:
        assert _call(L, **kw) == -1 and NAME.encode() in L.ivx_last_error(), (kw, L.ivx_last_error())
    # what each rule says
    for kw, word in ((dict(proj=None), b'null'), (dict(desc=False), b'null'), (dict(lists=False), b'null'), (dict(V=0), b'non-positive'),
                     (dict(dims=(2048, 1024, 1024)), b'voxel grid too large'), (dict(S=65536, fhw=(256, 128)), b'pool too large'),
                     (dict(B=65536, R=65536), b'batch too large'), (dict(V=257), b'max 256'), (dict(R=1, row=None), b'no row list'), (dict(kind=4), b'state_kind'),
                     (dict(state=None, kind=1), b'contradict'), (dict(state=384, kind=0), b'contradict'), (dict(fresh_below=0.0), b'fresh_below'),
                     (dict(first=512), b'first'), (dict(maps=(None, 576, -0.5, 0.0)), b'gate')):
        assert _call(L, **kw) == -1 and word in L.ivx_last_error(), (kw, L.ivx_last_error())
    assert _call(L, B=1 << 24, V=256, R=1 << 24) == -1 and b'view list too large' in L.ivx_last_error()
    # a gate is read only with a depth map: a bad gate beside a weight map alone passes validation ... and is then stopped by the next rule we break
    assert _call(L, maps=(576, None, -1.0, nan), fresh_below=0.0) == -1 and b'fresh_below' in L.ivx_last_error()
    with pytest.raises(ValueError, match=NAME):
        _lib.check(_call(L, kind=7), NAME)


def _host_args(B=2, S=4, dims=(7, 6, 5), fhw=(6, 9)):
    return dict(proj_pool=torch.zeros(S, 3, 4), lists=[[0, 1], [2]][:B], rows=[1, 0][:B], new_origin=torch.zeros(B, 3), crop_hw=torch.zeros(B, 2, dtype=torch.int32),
                voxel_size=(0.25, 0.25, 0.25), n_voxels=dims, fhw=fhw)


def test_ops_raise_their_host_errors():
    """Host tensors throughout, so nothing can reach a launch: list, shape and value errors come first, and arguments that pass them stop at the
    first host tensor."""
    from imvoxelnet_amd import ops

    def op(**kw):
        return ops.view_coverage(**dict(_host_args(), **kw))

    with pytest.raises(TypeError, match='proj_pool must be a torch.Tensor'):
        op(proj_pool=np.zeros((4, 3, 4), np.float32))
    with pytest.raises(ValueError, match=r'\[S,3,4\]'):
        op(proj_pool=torch.zeros(4, 12))
    with pytest.raises(TypeError, match='lists must be a host list'):
        op(lists=torch.zeros(2, 2, dtype=torch.int32))
    with pytest.raises(TypeError, match='lists must be a host list'):
        op(lists=[])
    with pytest.raises(TypeError, match='integers'):
        op(lists=[[0, 1.0], [2]])
    with pytest.raises(ValueError, match=r'slots outside \[0, 4\) other than the padding -1: \[-2, 4\]'):
        op(lists=[[0, 4], [-2, -1]])
    with pytest.raises(ValueError, match='at most 256'):
        op(lists=[[0] * 257, [1]])
    with pytest.raises(ValueError, match='rows has 1 entries for 2 samples'):
        op(rows=[0])
    with pytest.raises(ValueError, match='distinct'):
        op(rows=[1, 1])
    with pytest.raises(ValueError, match='rows must be >= 0'):
        op(rows=[0, -1])
    with pytest.raises(ValueError, match=r'rows must be in \[0, 2\)'):
        op(rows=[0, 2], state=torch.zeros(2, 7, 6, 5, dtype=torch.int32))
    with pytest.raises(ValueError, match='positive'):
        op(n_voxels=(7, 0, 5))
    with pytest.raises(ValueError, match='fhw has 3 entries'):
        op(fhw=(6, 9, 1))
    with pytest.raises(TypeError, match='state must be None or a torch.Tensor'):
        op(state=np.zeros((2, 7, 6, 5), np.int32))
    with pytest.raises(TypeError, match='int32 .counts., float32 .weight sums. or uint8'):
        op(state=torch.zeros(2, 7, 6, 5, dtype=torch.int64))
    with pytest.raises(ValueError, match=r'state must be \[R,X,Y,Z\]'):
        op(state=torch.zeros(2, 7, 6, 4))
    for bad in (0, -1.0, float('nan'), float('inf'), True, '1', None):
        with pytest.raises(ValueError, match='fresh_below'):
            op(fresh_below=bad)
    with pytest.raises(ValueError, match='gate'):
        op(gate=(-1.0, 0.0))
    with pytest.raises(TypeError, match='gate'):
        op(gate=1.0)
    with pytest.raises(ValueError, match=r'depth must be \[S,FH,FW\] = \[4,6,9\]'):
        op(depth=torch.zeros(4, 6, 8))
    with pytest.raises(TypeError, match='pixel_weight must be None or a torch.Tensor'):
        op(pixel_weight=np.zeros((4, 6, 9), np.float32))
    with pytest.raises(ValueError, match=r'out must be an int32 tensor \[B,V,2\] = \[2,2,2\]'):
        op(out=torch.zeros(2, 3, 2, dtype=torch.int32))
    # everything host-checkable passed: the device check is last
    for kw in (dict(), dict(state=torch.zeros(3, 7, 6, 5)), dict(pixel_weight=torch.ones(4, 1, 6, 9), depth=torch.ones(4, 6, 9), gate=(0.5, float('inf')))):
        with pytest.raises(RuntimeError, match='proj_pool must be a device'):
            op(**kw)


# ------------------------------------------------------------------ the reference's properties
def _dyadic(kind, seed=3, with_maps=False):
    sc = R.dyadic_scene()
    N = int(np.prod(R.N_VOXELS))
    rng = np.random.default_rng(seed)
    state = {RC.NONE: None, RC.COUNT: rng.integers(0, 3, N).astype(np.int32), RC.WSUM: rng.choice([0.0, 0.5, 1.0, 1.5, np.nan], N).astype(np.float32),
             RC.MASK: rng.integers(0, 2, N).astype(np.uint8)}[kind]
    maps = dict(pixel_weight=RM.general_weight_map(), depth=RM.dyadic_depth(), gate=RM.GATE) if with_maps else {}
    return sc, state, maps


def _cov(sc, state, kind, fresh_below=1.0, **maps):
    return RC.coverage(sc['proj'], R.N_VOXELS, R.VOXEL_SIZE, sc['new_origin'], sc['crop'], (R.FH, R.FW), state, kind, fresh_below, **maps)


@pytest.mark.parametrize('with_maps', [False, True], ids=['plain', 'maps'])
@pytest.mark.parametrize('kind', [RC.NONE, RC.COUNT, RC.WSUM, RC.MASK], ids=['none', 'count', 'wsum', 'mask'])
def test_reference_bounds_and_monotonicity(kind, with_maps):
    sc, state, maps = _dyadic(kind, with_maps=with_maps)
    N = int(np.prod(R.N_VOXELS))
    c = _cov(sc, state, kind, **maps)
    assert c.dtype == np.int64 and c.shape == (3, 2)
    assert (0 <= c[:, 1]).all() and (c[:, 1] <= c[:, 0]).all() and (c[:, 0] <= N).all()
    if kind == RC.NONE:
        assert np.array_equal(c[:, 0], c[:, 1])
    else:
        assert (c[:, 1] < c[:, 0]).any() and (c[:, 1] > 0).any()
    prev = np.zeros(3, np.int64)
    for fb in (2.0 ** -20, 0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 3.0, 1e30):      # fresh is monotone in fresh_below, seen does not depend on it
        cc = _cov(sc, state, kind, fb, **maps)
        assert np.array_equal(cc[:, 0], c[:, 0]) and (cc[:, 1] >= prev).all(), fb
        prev = cc[:, 1]
    if not with_maps:                              # seen is the lift's validity rule, nothing else
        ok = R.valid_views(sc['xf'], sc['yf'], sc['d'], sc['hc'], sc['wc'])
        assert np.array_equal(c[:, 0], ok.sum(1)) and c[:, 0].tolist() == R.scene_classes(sc)['valid']
    else:
        plain = _cov(sc, state, kind)
        assert (c[:, 0] < plain[:, 0]).all() and (c[:, 0] > 0).all(), 'the maps drop some seen voxels and keep some'


def test_reference_ties_and_nan():
    """den == fresh_below is not fresh; a NaN evidence is fresh; a count converts to float before the comparison."""
    assert RC.fresh_of(np.array([0.0, 0.5, 1.0, 1.5, np.nan, -0.0, np.inf], np.float32), 1.0).tolist() == [True, True, False, False, True, True, False]
    assert RC.fresh_of(RC.den_of(np.array([0, 1, 2, 3], np.int32), RC.COUNT, 4), 2.0).tolist() == [True, True, False, False]
    assert RC.fresh_of(RC.den_of(np.array([0, 1, 7, 255], np.uint8), RC.MASK, 4), 1.0).tolist() == [True, False, False, False]
    assert RC.fresh_of(RC.den_of(None, RC.NONE, 3), 2.0 ** -100).all()
    sc = R.dyadic_scene()
    N = int(np.prod(R.N_VOXELS))
    seen = _cov(sc, None, RC.NONE)[:, 0]
    assert np.array_equal(_cov(sc, np.full(N, 0.75, np.float32), RC.WSUM, 0.75)[:, 1], np.zeros(3, np.int64)), 'equality is not fresh'
    assert np.array_equal(_cov(sc, np.full(N, np.nan, np.float32), RC.WSUM, 0.75)[:, 1], seen), 'NaN evidence is fresh'
    assert np.array_equal(_cov(sc, np.full(N, 0.75, np.float32), RC.WSUM, np.nextafter(np.float32(0.75), np.float32(1)))[:, 1], seen)


def test_reference_lists_rows_and_padding():
    sc, sc2 = R.dyadic_scene(R.NEW_ORIGIN, R.CROP), R.dyadic_scene(R.NEW_ORIGIN_2, R.CROP_2)
    N = int(np.prod(R.N_VOXELS))
    state = np.random.default_rng(1).integers(0, 3, (3, N)).astype(np.int32)
    lists, rows = [[2, -1, 0], [1], [-1, -1]], [2, 0, 1]
    out = RC.coverage_lists(sc['proj'], lists, rows, R.N_VOXELS, R.VOXEL_SIZE, [sc['new_origin'], sc2['new_origin'], sc['new_origin']],
                            [sc['crop'], sc2['crop'], sc['crop']], (R.FH, R.FW), state, RC.COUNT)
    assert out.shape == (3, 3, 2) and not out[0, 1].any() and not out[2].any() and not out[1, 1:].any()
    a = _cov(sc, state[2], RC.COUNT)
    b = RC.coverage(sc2['proj'], R.N_VOXELS, R.VOXEL_SIZE, sc2['new_origin'], sc2['crop'], (R.FH, R.FW), state[0], RC.COUNT)
    assert np.array_equal(out[0, 0], a[2]) and np.array_equal(out[0, 2], a[0]) and np.array_equal(out[1, 0], b[1])


# ------------------------------------------------------------------ the gate on the host
def test_min_novelty_and_fresh_below_are_validated():
    from imvoxelnet_amd import scene
    assert scene._check_novelty(None, None) == (None, 1.0) and scene._check_novelty(0.25, None) == (0.25, 1.0)
    assert scene._check_novelty(1, 0.5) == (1.0, 0.5) and scene._check_novelty(np.float32(0.5), np.float64(2)) == (0.5, 2.0)
    assert scene._check_novelty(None, 0.5, alone=True) == (None, 0.5)
    for bad in (0, 0.0, -0.1, 1.0001, 2, float('nan'), float('inf'), True, '0.5', [0.5]):
        with pytest.raises(ValueError, match='min_novelty'):
            scene._check_novelty(bad, None)
    for bad in (0, -1.0, float('nan'), float('inf'), True, '1'):
        with pytest.raises(ValueError, match='fresh_below'):
            scene._check_novelty(0.5, bad)
    with pytest.raises(ValueError, match='give min_novelty'):
        scene._check_novelty(None, 0.5)
    # the rule: seen > 0 and fresh / seen >= min_novelty, in Python floats; equality admits, nothing seen rejects
    assert scene.admitted(np.array([[10, 0], [10, 5], [0, 0], [3, 1], [7, 7]]), 0.5) == [False, True, False, False, True]
    assert scene.admitted([[3, 1]], 1 / 3) == [True] and scene.admitted([[210, 1]], 0.01) == [False] and scene.admitted([[100, 1]], 0.01) == [True]


VS = (0.16, 0.16, 0.2)
K4 = np.array([[90., 0, 63.5, 0], [0, 90., 47.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
META = dict(img_shape=(96, 128, 3), ori_shape=(96, 128, 3), lidar2img=dict(intrinsic=K4, origin=np.array([0.37, -1.21, .5], np.float32)))


class _OnDevice(torch.Tensor):
    """A host tensor that says it lives on the device: enough for the argument checks of an add whose launches are all stubbed."""
    is_cuda = True


def _stubbed_session(counts, **kw):
    """A SceneSession on a mock model whose device work is replaced by recorders: _coverage returns `counts`, _features and the lift record."""
    from imvoxelnet_amd import SceneSession
    log = types.SimpleNamespace(features=[], lifts=[], coverage=[])
    model = types.SimpleNamespace(head_2d=None, voxel_size=VS, n_voxels=(40, 40, 16), _prepared_device=torch.device('cpu'), _native=None,
                                  _camera_setup=lambda metas, stride, dev: (torch.zeros(1, len(metas[0]['lidar2img']['extrinsic']), 3, 4), torch.zeros(1, 3),
                                                                            torch.zeros(1, 2, dtype=torch.int32)),
                                  _compute_projection=lambda meta, stride: torch.zeros(len(meta['lidar2img']['extrinsic']), 3, 4))
    s = SceneSession(model, META, **kw)

    def coverage(E, maps, hw, meta, fresh_below, strided=True, dev=None):
        log.coverage.append((len(E), fresh_below))
        return np.asarray(counts[:len(E)], np.int64)

    def features(img):
        log.features.append(int(img.shape[0]))
        return torch.zeros(img.shape[0], 1, 24, 32, 8)

    def lift(p0, proj, origin, crop, E, hw, weights, emit, maps=(None, None)):
        log.lifts.append((int(p0.shape[0]), [float(e[0, 3]) for e in E], weights))
        s._grow(E, hw, stale=False)

    s._coverage, s._features, s._add_unbounded = coverage, features, lift
    return s, log


def _frames(V):
    img = torch.zeros(V, 3, 96, 128).as_subclass(_OnDevice)
    E = []
    for v in range(V):
        e = np.eye(4, dtype=np.float32)
        e[0, 3] = v
        E.append(e)
    return img, E


def test_last_admitted_on_a_stubbed_session():
    img, E = _frames(3)
    s, log = _stubbed_session([[10, 0], [10, 5], [0, 0]], decay=1.0)
    assert s.last_admitted is None
    assert s.add_views(img, E, weights=[1.0, 2.0, 3.0], min_novelty=0.5) is s
    assert s.last_admitted == [False, True, False] and log.coverage == [(3, 1.0)]
    assert log.features == [1] and log.lifts == [(1, [1.0], [2.0])] and s.n_views == 1, 'only the admitted view reached the trunk and the lift'
    assert len(s.meta['lidar2img']['extrinsic']) == 1 and s.meta['lidar2img']['extrinsic'][0][0, 3] == 1.0
    # every view rejected: no trunk, no lift, nothing changes, and the verdicts say so
    s.add_views(img[:2], E[:2], min_novelty=0.75, fresh_below=0.5)
    assert s.last_admitted == [False, False] and log.coverage[-1] == (2, 0.5) and log.features == [1] and len(log.lifts) == 1 and s.n_views == 1
    # every view admitted: the call goes through whole
    s.add_views(img[:2], E[:2], min_novelty=0.01)
    assert s.last_admitted == [False, True] and log.features == [1, 1]
    s2, log2 = _stubbed_session([[4, 4], [4, 2]])
    s2.add_views(img[:2], E[:2], min_novelty=0.5)
    assert s2.last_admitted == [True, True] and log2.features == [2] and log2.lifts == [(2, [0.0, 1.0], None)] and s2.n_views == 2
    # an ungated call asks for no coverage and leaves None
    s2.add_views(img[:1], E[:1])
    assert s2.last_admitted is None and len(log2.coverage) == 1 and log2.features == [2, 1] and s2.n_views == 3
    # bad gate arguments raise before anything happens
    for kw in (dict(min_novelty=0), dict(min_novelty=1.5), dict(fresh_below=0.5), dict(min_novelty=0.5, fresh_below=-1)):
        with pytest.raises(ValueError):
            s2.add_views(img[:1], E[:1], **kw)
    assert s2.last_admitted is None and log2.features == [2, 1] and s2.n_views == 3


def test_coverage_checks_its_arguments_on_the_host():
    from imvoxelnet_amd import SceneSession, SceneBatch
    model = types.SimpleNamespace(head_2d=None, voxel_size=VS, n_voxels=(40, 40, 16))
    _, E = _frames(2)
    s = SceneSession(model, META)
    with pytest.raises(ValueError, match='at least one'):
        s.coverage([])
    with pytest.raises(TypeError, match='float32'):
        s.coverage([np.eye(4)])
    with pytest.raises(ValueError, match='depth_gate'):
        s.coverage(E, depths=torch.zeros(2, 24, 32))
    with pytest.raises(ValueError, match=r'pixel_weights must be \[V,FH,FW\]'):
        s.coverage(E, pixel_weights=torch.zeros(3, 24, 32))
    with pytest.raises(ValueError, match='fresh_below'):
        s.coverage(E, fresh_below=0)
    with pytest.raises(ValueError, match='pad_shape'):
        s.coverage(E)                                   # no view yet and no pad_shape: the feature-map size is unknown
    with pytest.raises(ValueError, match='img_shape'):
        SceneSession(model, dict(lidar2img=META['lidar2img'])).coverage(E)
    s.close()
    with pytest.raises(RuntimeError, match='closed'):
        s.coverage(E)
    b = SceneBatch(model, [META] * 3)
    with pytest.raises(ValueError, match='one scene index per view'):
        b.coverage(E, [0])
    with pytest.raises(ValueError, match='unknown scene index'):
        b.coverage(E, [0, 3])
    with pytest.raises(ValueError, match='pad_shape'):
        b.coverage(E, [2, 0])
    assert b.last_admitted is None


def test_the_docs_speak_of_view_coverage():
    import imvoxelnet_amd as ia
    assert 'View coverage' in ia.scene.__doc__ and 'min_novelty' in ia.scene.__doc__
    assert 'view_coverage' in open(os.path.join(ROOT, 'DESIGN.md')).read() and 'view coverage' in open(os.path.join(ROOT, 'README.md')).read().lower()
    assert 'min_novelty' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
