"""Scene snapshots without a device: a SceneSnapshot built from arrays survives save / load field by field and byte by byte; load refuses what it
should not believe (a pickled object, a wrong format number, indices that are not ascending or out of range, a payload of the wrong width ...) with
a ValueError that names it; windowed and closed scenes refuse; an empty session and empty batch rows snapshot and restore with no launch; a
restore checks the model and the batch before anything changes."""
import os
import types

import numpy as np
import pytest
import torch

from helpers import ROOT

VS = (0.16, 0.16, 0.2)
K4 = np.array([[90., 0, 63.5, 0], [0, 90., 47.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
ORIGIN = np.array([0.37, -1.21, .5], np.float32)
META = dict(img_shape=(96, 128, 3), ori_shape=(96, 128, 3), lidar2img=dict(intrinsic=K4, origin=ORIGIN))
GRID, C = (4, 3, 5), 8


@pytest.fixture(autouse=True)
def _library_of_this_version():
    """Everything here, the reference included, states what library version 0.5.6 does: the library under test must be one."""
    from imvoxelnet_amd import _lib
    assert _lib.lib().ivx_version() >= 560, 'the loaded libimvoxel_hip.so predates the 0.5.6 entries'


def _mock_model(**kw):
    return types.SimpleNamespace(**dict(dict(head_2d=None, voxel_size=VS, n_voxels=GRID, neck=types.SimpleNamespace(out_channels=C), sampling='nearest',
                                             _prepared_device=None, storage_dtype=None), **kw))


def _snap(bf16=False, fading=True, **kw):
    from imvoxelnet_amd import SceneSnapshot
    rng = np.random.default_rng(3)
    index = np.array([0, 7, 8, 31, 59], np.int32)
    n = len(index)
    payload = rng.integers(0, 2 ** 16, (n, C)).astype(np.uint16) if bf16 else rng.integers(-2 ** 31, 2 ** 31, (n, C), dtype=np.int64).astype(np.int32).view(np.float32)
    E = np.stack([np.eye(4, dtype=np.float32) + np.float32(0.1 * i) for i in range(3)])
    frame = np.eye(4)
    frame[:3, 3] = (0.5, -0.25, 0.125)
    args = dict(index=index, payload=payload, count=rng.integers(0, 5, n).astype(np.int32), wsum=rng.uniform(0.1, 3, n).astype(np.float32) if fading else None,
                kind='fading' if fading else 'plain', decay=0.9 if fading else None, forget_below=0.25 if fading else 0.0, depth_gate=(0.5, float('inf')) if fading else None,
                grid=GRID, channels=C, voxel_size=VS, sampling='nearest', intrinsic=K4, origin=ORIGIN, extrinsics=E, img_shape=(96, 128, 3), ori_shape=(96, 128, 3),
                pad_shape=None, hw=(96, 128), n_views=3, scrolled=(1, 0, -2), frame=frame, box_type='DepthInstance3DBoxes')
    args.update(kw)
    return SceneSnapshot(args.pop('index'), args.pop('payload'), args.pop('count'), args.pop('wsum'), **args)


ARRAYS = ('index', 'payload', 'count', 'wsum', 'intrinsic', 'origin', 'extrinsics', 'frame')
FIELDS = ('kind', 'decay', 'forget_below', 'depth_gate', 'grid', 'channels', 'voxel_size', 'sampling', 'img_shape', 'ori_shape', 'pad_shape', 'hw', 'n_views', 'scrolled',
          'box_type', 'payload_dtype', 'version', 'format', 'n_seen', 'nbytes', 'seen_fraction')


def _equal(a, b):
    for k in ARRAYS:
        x, y = getattr(a, k), getattr(b, k)
        if (x is None) != (y is None) or (x is not None and (x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes())):
            return False
    return all(getattr(a, k) == getattr(b, k) and type(getattr(a, k)) is type(getattr(b, k)) for k in FIELDS)


@pytest.mark.parametrize('bf16,fading', [(False, True), (True, True), (False, False)])
def test_save_load_round_trip_field_by_field_and_byte_by_byte(tmp_path, bf16, fading):
    from imvoxelnet_amd import SceneSnapshot
    s = _snap(bf16, fading)
    assert s.payload_dtype == ('bfloat16' if bf16 else 'float32') and s.n_seen == 5 and s.seen_fraction == 5 / 60 and s.version >= 560 and s.format == 1
    assert s.nbytes == 5 * (4 + 4 + (4 if fading else 0) + C * (2 if bf16 else 4))
    path = str(tmp_path / 'scene.npz')
    assert s.save(path) == path
    t = SceneSnapshot.load(path)
    assert _equal(s, t) and t.payload.dtype == (np.uint16 if bf16 else np.float32)
    assert not any(isinstance(v, torch.Tensor) for v in vars(t).values()), 'host data only'
    with np.load(path, allow_pickle=False) as z:      # plain arrays only: the file opens without pickle
        assert 'index' in z.files and all(z[k].dtype != object for k in z.files)
    # an empty scene
    e = _snap(bf16, fading, index=np.zeros(0, np.int32), payload=np.zeros((0, C), np.uint16 if bf16 else np.float32), count=np.zeros(0, np.int32),
              wsum=np.zeros(0, np.float32) if fading else None, n_views=0, extrinsics=None, hw=None, img_shape=None, ori_shape=None)
    e.save(path)
    assert _equal(e, SceneSnapshot.load(path)) and e.n_seen == 0 and e.nbytes == 0 and e.seen_fraction == 0.0


def _saved(tmp_path, **change):
    """The arrays of a saved snapshot, changed, written back -> path."""
    path = str(tmp_path / 'a.npz')
    _snap().save(path)
    with np.load(path, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    for k, v in change.items():
        if v is None:
            d.pop(k)
        else:
            d[k] = v
    with open(path, 'wb') as f:
        np.savez(f, **d)
    return path


def test_load_refuses_what_it_should_not_believe(tmp_path):
    from imvoxelnet_amd import SceneSnapshot

    class Evil:
        def __reduce__(self):
            return (os.system, ('exit 1',))
    path = str(tmp_path / 'evil.npz')
    _snap().save(path)
    with np.load(path, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    d['box_type'] = np.array(Evil(), dtype=object)
    with open(path, 'wb') as f:
        np.savez(f, **d)
    with pytest.raises(ValueError, match='pickled object'):
        SceneSnapshot.load(path)
    rng = np.random.default_rng(0)
    for change, words in ((dict(format=np.asarray(2)), 'format 2'), (dict(format=np.asarray(0)), 'format 0'),
                          (dict(index=np.array([0, 8, 7, 31, 59], np.int32)), 'strictly ascending'), (dict(index=np.array([0, 7, 7, 31, 59], np.int32)), 'strictly ascending'),
                          (dict(index=np.array([0, 7, 8, 31, 60], np.int32)), r'inside \[0, 60\)'), (dict(index=np.array([-1, 7, 8, 31, 59], np.int32)), r'inside \[0, 60\)'),
                          (dict(index=np.array([0, 7, 8, 31, 59], np.int64)), 'index must be int32'),
                          (dict(payload=rng.random((5, C - 4)).astype(np.float32)), 'payload must be'), (dict(payload=rng.random((4, C)).astype(np.float32)), 'payload must be'),
                          (dict(payload=rng.random((5, C))), 'payload must be float32'), (dict(count=np.zeros(4, np.int32)), 'count must be'),
                          (dict(wsum=np.zeros(6, np.float32)), 'wsum must be'), (dict(wsum=None), 'weight sum per record'),
                          (dict(grid=np.array([4, 3])), 'grid'), (dict(grid=np.array([4, 3, 0])), 'grid'), (dict(channels=np.asarray(6)), 'channels'),
                          (dict(frame=np.full((4, 4), np.nan)), 'frame'), (dict(intrinsic=np.full((4, 4), np.inf, np.float32)), 'intrinsic'),
                          (dict(extrinsics=np.full((3, 4, 4), np.nan, np.float32)), 'extrinsics'), (dict(extrinsics=np.zeros((2, 4, 4), np.float32)), 'n_views'),
                          (dict(origin=np.array([0, np.nan, 0])), 'origin'), (dict(voxel_size=np.array([0.16, 0.0, 0.2])), 'voxel_size'),
                          (dict(kind=np.asarray('windowed')), 'kind'), (dict(decay=None), 'decay'), (dict(sampling=np.asarray('cubic')), 'sampling'),
                          (dict(hw=None), 'image size'), (dict(index=None), 'missing fields'), (dict(extra=np.zeros(3)), 'unknown fields'),
                          (dict(n_views=np.array([3, 3])), 'scalar')):
        with pytest.raises(ValueError, match=words):
            SceneSnapshot.load(_saved(tmp_path, **change))
    bare = str(tmp_path / 'bare.npz')
    with open(bare, 'wb') as f:
        import pickle
        pickle.dump({'index': [1, 2]}, f)
    with pytest.raises(ValueError, match='snapshot'):
        SceneSnapshot.load(bare)
    np.save(str(tmp_path / 'one.npy'), np.zeros(3))
    with pytest.raises(ValueError, match='not an .npz'):
        SceneSnapshot.load(str(tmp_path / 'one.npy'))
    # the same checks guard a snapshot built by hand
    with pytest.raises(ValueError, match='strictly ascending'):
        _snap(index=np.array([5, 4, 8, 31, 59], np.int32))
    with pytest.raises(ValueError, match='payload must be'):
        _snap(payload=np.zeros((5, 2 * C), np.float32))


def test_windowed_and_closed_scenes_refuse_and_an_empty_scene_launches_nothing(monkeypatch):
    from imvoxelnet_amd import SceneSession, SceneBatch, SceneSnapshot, ops
    calls = []
    monkeypatch.setattr(ops, 'volume_pack', lambda *a, **k: calls.append('pack'))
    monkeypatch.setattr(ops, 'volume_unpack_', lambda *a, **k: calls.append('unpack'))
    m = _mock_model()
    with pytest.raises(NotImplementedError, match='windowed session'):
        SceneSession(m, META, window=3).snapshot()
    for call in (lambda b: b.snapshot(0), lambda b: b.snapshot([0, 1]), lambda b: b.restore(0, _snap())):
        with pytest.raises(NotImplementedError, match='windowed batch'):
            call(SceneBatch(m, [META] * 2, window=2))
    s = SceneSession(m, META, decay=0.9)
    s.close()
    with pytest.raises(RuntimeError, match='closed'):
        s.snapshot()
    b = SceneBatch(m, [META] * 2)
    b.close()
    for call in (lambda: b.snapshot(0), lambda: b.restore(0, _snap(fading=False))):
        with pytest.raises(RuntimeError, match='closed'):
            call()
    for bad in (torch.float16, 'float32', None, np.float32):
        with pytest.raises(TypeError, match='dtype'):
            SceneSession(m, META).snapshot(bad)
    # an empty session of each kind, scrolled and warped: the record travels, nothing is launched
    for kw in (dict(), dict(decay=0.8, forget_below=0.5, depth_gate=(0.25, 1.0))):
        s = SceneSession(m, dict(META, box_type_3d=__import__('imvoxelnet_amd').DepthInstance3DBoxes), **kw)
        if kw:
            T = np.eye(4)
            T[:3, 3] = (0.1, 0.2, 0.3)
            s.warp(T)
        for dtype in (torch.float32, torch.bfloat16):
            snap = s.snapshot(dtype)
            assert isinstance(snap, SceneSnapshot) and snap.n_seen == 0 and snap.n_views == 0 and snap.nbytes == 0 and snap.kind == ('fading' if kw else 'plain')
            assert snap.grid == GRID and snap.channels == C and snap.voxel_size == VS and snap.decay == kw.get('decay') and snap.depth_gate == kw.get('depth_gate')
            assert snap.payload_dtype == ('float32' if dtype == torch.float32 else 'bfloat16') and (snap.wsum is None) == (not kw) and snap.box_type == 'DepthInstance3DBoxes'
            assert np.array_equal(snap.frame, s.frame) and np.array_equal(snap.intrinsic, K4) and np.array_equal(snap.origin, ORIGIN) and snap.hw is None
    assert not calls


def _restore_scene(m, snap, device=None):
    """ImVoxelNet.restore_scene on the stub model (the method needs nothing else of the class)."""
    from imvoxelnet_amd import ImVoxelNet
    return ImVoxelNet.restore_scene(m, snap, device)


def test_restore_checks_the_model_and_an_empty_snapshot_restores_with_no_launch(monkeypatch):
    from imvoxelnet_amd import SceneSession, SceneBatch, ops, DepthInstance3DBoxes
    calls = []
    monkeypatch.setattr(ops, 'volume_unpack_', lambda *a, **k: calls.append('unpack'))
    m = _mock_model()
    s = SceneSession(m, dict(META, box_type_3d=DepthInstance3DBoxes), decay=0.8, forget_below=0.5, depth_gate=(0.25, 1.0))
    T = np.eye(4)
    T[:3, 3] = (0.1, 0.2, 0.3)
    s.warp(T)
    s._scrolled = (2, 0, -1)
    snap = s.snapshot()
    r = _restore_scene(m, snap)
    assert isinstance(r, SceneSession) and r is not s and r._model is m and (r._decay, r._forget, r._gate, r._window) == (0.8, 0.5, (0.25, 1.0), None)
    assert r.n_views == 0 and r._sum is None and not r._stale and r._hw is None and r.scrolled == (2, 0, -1) and np.array_equal(r.frame, T)
    assert np.array_equal(r.meta['lidar2img']['intrinsic'], K4) and np.array_equal(r.meta['lidar2img']['origin'], ORIGIN) and r.meta['lidar2img']['extrinsic'] == []
    assert r.meta['img_shape'] == (96, 128, 3) and r.meta['box_type_3d'] is DepthInstance3DBoxes
    for other, words in ((_mock_model(n_voxels=(4, 3, 6)), 'grid'), (_mock_model(voxel_size=(0.16, 0.16, 0.25)), 'voxel size'),
                         (_mock_model(neck=types.SimpleNamespace(out_channels=16)), 'channels'), (_mock_model(sampling='bilinear'), 'rule')):
        with pytest.raises(ValueError, match=words):
            _restore_scene(other, snap)
    for bad in (None, META, s):
        with pytest.raises(TypeError, match='SceneSnapshot'):
            _restore_scene(m, bad)
    snap.index = np.array([3], np.int32)              # a snapshot spoiled after it was built is not believed either
    with pytest.raises(ValueError, match='payload must be'):
        _restore_scene(m, snap)
    # batches: the kind, the threshold and the gate must be the batch's; indices and lists are checked; nothing changes
    snap = s.snapshot()
    b = SceneBatch(m, [META] * 3, decay=0.9, forget_below=0.5, depth_gate=(0.25, 1.0))
    assert b.restore(1, snap) is b and b.restore([0, 2], [snap, snap]) is b and b.n_views == [0, 0, 0]
    assert b._scenes[1]._decay == 0.8 and b._scenes[1].scrolled == (2, 0, -1) and np.array_equal(b.frame(2), T) and b._cam == [None] * 3 and b._sum is None
    snaps = b.snapshot([2, 0])
    assert [x.scrolled for x in snaps] == [(2, 0, -1)] * 2 and snaps[0].decay == 0.8 and b.snapshot(1).n_seen == 0
    with pytest.raises(ValueError, match='plain snapshot into a fading batch'):
        b.restore(0, SceneSession(m, META).snapshot())
    with pytest.raises(ValueError, match='fading snapshot into a plain batch'):
        SceneBatch(m, [META] * 2).restore(0, snap)
    with pytest.raises(ValueError, match='forget_below'):
        SceneBatch(m, [META] * 2, decay=0.9, depth_gate=(0.25, 1.0)).restore(0, snap)
    with pytest.raises(ValueError, match='depth_gate'):
        SceneBatch(m, [META] * 2, decay=0.9, forget_below=0.5).restore(0, snap)
    for args in ((3, snap), (-1, snap), ([0, 0], [snap, snap]), ([0, 1], [snap]), ([], []), (True, snap), ([0, 1], snap)):
        with pytest.raises(ValueError):
            b.restore(*args)
    for arg in (3, [0, 0], [], True):
        with pytest.raises(ValueError):
            b.snapshot(arg)
    with pytest.raises(ValueError, match='grid'):
        SceneBatch(_mock_model(n_voxels=(4, 3, 6)), [META] * 2, decay=0.9, forget_below=0.5, depth_gate=(0.25, 1.0)).restore(0, snap)
    # a snapshot with views against the image size the batch already holds
    full = _snap(decay=0.8, forget_below=0.5, depth_gate=(0.25, 1.0))
    b._hw = (64, 128)
    b._scenes[0].n_views = 1
    before = (b.n_views, [r.scrolled for r in b._scenes])
    with pytest.raises(ValueError, match='image size'):
        b.restore(1, full)
    assert (b.n_views, [r.scrolled for r in b._scenes]) == before and not calls


def test_the_docs_speak_of_snapshots():
    import imvoxelnet_amd as ia
    doc = ia.scene.__doc__
    assert 'Scene snapshots' in doc and 'ivx_volume_pack_fwd' in doc and 'volume_unpack_' in doc
    out = doc[doc.index('Out of scope'):]
    for words in ('windowed scenes', 'merge taking a snapshot directly', 'turning a plain snapshot into a fading scene', 'beyond the bf16 mean',
                  'weights of\nthe restoring model'):
        assert words in out, words
    for d in (ia.SceneSnapshot.__doc__, ia.ImVoxelNet.restore_scene.__doc__):
        assert 'Out of scope' in d and 'windowed' in d
    header = open(os.path.join(ROOT, 'include', 'imvoxel.h')).read()
    for words in ('Order.', 'Untouched.', 'Round trip.', 'Checked data.'):
        assert words in header[header.index('(0.5.6) Ordered compaction'):header.index('int64_t ivx_volume_pack_scratch_bytes')], words
    assert 'volume_pack' in open(os.path.join(ROOT, 'DESIGN.md')).read() and 'scene snapshots' in open(os.path.join(ROOT, 'README.md')).read().lower()
    assert os.path.exists(os.path.join(ROOT, 'profiles', 'scene_snapshot.md')) and os.path.exists(os.path.join(ROOT, 'tools', 'scene_snapshot_bench.py'))
