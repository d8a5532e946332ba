"""Sliding-window scenes without a device: ivx_backproject_gather_fwd is declared / bound / exported and rejects bad arguments before any
launch; ops.backproject_gather_mean and the windowed SceneSession raise their pre-launch errors and leave the session as it was."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from helpers import ROOT

NAME = 'ivx_backproject_gather_fwd'


def test_entry_point_declared_bound_and_exported():
    from imvoxelnet_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'imvoxel.h')).read()
    assert NAME in set(re.findall(r'\b(ivx_[a-z0-9_]+)\s*\(', header)), f'{NAME} is not declared in include/imvoxel.h'
    L = _lib.lib()
    assert NAME in _lib.EXPORTS and hasattr(L, NAME) and getattr(L, NAME).argtypes is not None
    assert L.ivx_version() >= 460
    for src in ('model.cpp', 'api_common.cpp'):        # also compiled into the CPU restatement of the ABI, which does not define it
        assert NAME not in open(os.path.join(ROOT, 'imvoxelnet_amd', 'csrc', src)).read(), src


def test_gather_argument_validation_without_gpu():
    """Every invalid argument: status -1 with its message, nothing launched (the dummy pointers are never dereferenced)."""
    from imvoxelnet_amd import _lib
    L = _lib.lib()
    fn = getattr(L, NAME)
    p = ctypes.c_void_p(64)

    def call(S=3, desc=True, pool=p, ppool=p, slots=p, origin=p, crop=p, vol=p, valid=p, **kw):
        f = dict(B=1, V=2, FH=6, FW=8, C=8, X=4, Y=4, Z=2, feat_dtype=0, mode=0, sampling=0, first=0)
        f.update(kw)
        d = _lib.BackprojectDesc(f['B'], f['V'], f['FH'], f['FW'], f['C'], f['X'], f['Y'], f['Z'], (ctypes.c_float * 3)(.5, .5, .5), f['feat_dtype'],
                                 f['mode'], f['sampling'], f['first'])
        return fn(ctypes.byref(d) if desc else None, S, pool, ppool, slots, origin, crop, vol, valid, None)

    def err():
        return L.ivx_last_error()

    assert call(desc=False) == -1 and b'null descriptor' in err() and NAME.encode() in err()
    for ptr in ('pool', 'ppool', 'slots', 'origin', 'crop', 'vol', 'valid'):
        assert call(**{ptr: None}) == -1 and b'null argument' in err(), ptr
    for S in (0, -2):
        assert call(S=S) == -1 and b'slots' in err() and NAME.encode() in err()
    for bad in (dict(B=0), dict(V=0), dict(FH=-1), dict(FW=0), dict(C=0), dict(X=0), dict(Y=-1), dict(Z=-3)):
        assert call(**bad) == -1 and b'non-positive' in err(), bad
    for C in (6, 10, 1026):
        assert call(C=C) == -1 and b'C % 4' in err(), C
    assert call(C=1028) == -1 and b'too large (max 1024)' in err()
    for mode in (1, 2, 3, -1):                           # IVX_LIFT_SUM, IVX_LIFT_ACCUM, unknown
        assert call(mode=mode) == -1 and b'IVX_LIFT_MEAN only' in err(), mode
    for s in (2, -1):
        assert call(sampling=s) == -1 and b'sampling' in err(), s
    for dt in (2, 3, -1):                                # IVX_FP8 and unknown
        assert call(feat_dtype=dt) == -1 and b'feat_dtype' in err(), dt
    assert call(X=2048, Y=2048, Z=512) == -1 and b'voxel grid too large' in err()                # X*Y*Z = 2^31
    assert call(S=1 << 15, FH=256, FW=256) == -1 and b'feature pool too large' in err()          # S*FH*FW = 2^31
    assert call(B=65536) == -1 and b'batch too large' in err()
    with pytest.raises(ValueError, match=NAME):
        _lib.check(call(C=6), NAME)


def test_op_rejects_host_pools_bad_dtypes_and_bad_host_lists():
    from imvoxelnet_amd import ops
    pool, ppool = torch.zeros(3, 1, 4, 4, 8), torch.zeros(3, 3, 4)
    no, crop = torch.zeros(1, 3), torch.zeros(1, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='device'):
        ops.backproject_gather_mean(pool, ppool, [[0, 1]], no, crop, (1, 1, 1), (2, 2, 2))
    for dt in (torch.float16, torch.float64, torch.int32):
        with pytest.raises(TypeError, match='float32 or bfloat16'):
            ops.backproject_gather_mean(pool.to(dt), ppool, [[0, 1]], no, crop, (1, 1, 1), (2, 2, 2))
    with pytest.raises(ValueError, match='sampling'):
        ops.backproject_gather_mean(pool, ppool, [[0, 1]], no, crop, (1, 1, 1), (2, 2, 2), sampling='cubic')
    # a host list is checked against the pools' S before the pools' device: ValueError here, although the pools would be refused next
    for bad in ([[0, -1]], [[3, 1]], torch.tensor([[0, 3]], dtype=torch.int32), torch.tensor([[-1]])):
        with pytest.raises(ValueError, match=r'outside \[0, 3\)'):
            ops.backproject_gather_mean(pool, ppool, bad, no, crop, (1, 1, 1), (2, 2, 2))
    for bad in ([0, 1], [[0.5, 1.0]], [[]]):
        with pytest.raises(ValueError, match=r'\[B,V\]'):
            ops.backproject_gather_mean(pool, ppool, bad, no, crop, (1, 1, 1), (2, 2, 2))
    with pytest.raises(ValueError, match='proj_pool'):
        ops.backproject_gather_mean(pool, ppool[:2], [[0, 1]], no, crop, (1, 1, 1), (2, 2, 2))


# ------------------------------------------------------------------ the session's pre-launch errors
K = np.array([[90., 0, 63.5, 0], [0, 90., 47.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
META = dict(img_shape=(96, 128, 3), ori_shape=(96, 128, 3), lidar2img=dict(intrinsic=K, origin=np.array([0, 0, .5], np.float32)))
E4 = np.eye(4, dtype=np.float32)


def _mock_model(**kw):
    """What SceneSession touches before its first launch; any device work would fail on the missing attributes."""
    return types.SimpleNamespace(**dict(dict(head_2d=None), **kw))


def test_window_argument():
    from imvoxelnet_amd import SceneSession
    for bad in (0, -3):
        with pytest.raises(ValueError, match='window'):
            SceneSession(_mock_model(), META, window=bad)
    for bad in (2.0, '2', True, [2]):
        with pytest.raises(TypeError, match='window'):
            SceneSession(_mock_model(), META, window=bad)
    s = SceneSession(_mock_model(), META, window=np.int64(3))
    assert s._window == 3 and s.view_ids == [] and s.n_views == 0
    assert SceneSession(_mock_model(), META)._window is None


def test_open_scene_passes_the_window_on():
    import imvoxelnet_amd as ia
    from kitti_cfg import kitti_model_cfg, KITTI_TEST_CFG
    model = ia.build_detector(kitti_model_cfg(n_voxels=(24, 28, 12), in_ch=16, out_ch=32), test_cfg=KITTI_TEST_CFG)
    assert model.open_scene(META, window=2)._window == 2 and model.open_scene(META)._window is None
    with pytest.raises(ValueError, match='window'):
        model.open_scene(META, window=0)
    assert model._prepared_device is None


def _scene_with_views(window, ids_slots):
    """A windowed session as after adds that left these (id, slot) pairs, without any device work."""
    from imvoxelnet_amd import SceneSession
    s = SceneSession(_mock_model(), META, window=window)
    s._views = [(i, slot, E4 * (i + 1)) for i, slot in ids_slots]
    s.meta['lidar2img']['extrinsic'] = [v[2] for v in s._views]
    s.n_views, s._next_id, s._hw = len(s._views), max(i for i, _ in ids_slots) + 1, (96, 128)
    return s


def _snapshot(s):
    return list(s.view_ids), s.n_views, list(s.meta['lidar2img']['extrinsic']), {k: v for k, v in s.meta.items() if k != 'lidar2img'}, s._stale


def test_calls_that_raise_leave_the_windowed_session_as_it_was():
    s = _scene_with_views(3, [(4, 1), (5, 2), (7, 0)])
    before = _snapshot(s)
    assert before[0] == [4, 5, 7] and before[1] == 3
    img = torch.zeros(4, 3, 96, 128)
    with pytest.raises(ValueError, match='4 views in one call do not fit a window of 3'):       # stops before the host-tensor check
        s.add_views(img, [E4] * 4)
    with pytest.raises(ValueError, match='do not fit'):
        s.add_views_u8([np.zeros((48, 64, 3), np.uint8)] * 4, [E4] * 4, (128, 96))
    with pytest.raises(RuntimeError, match='device'):            # W views are accepted: stops at the host tensor, before any launch
        s.add_views(img[:3], [E4] * 3)
    with pytest.raises(ValueError, match='differs'):
        s.add_views(torch.zeros(1, 3, 96, 160), [E4])
    with pytest.raises(TypeError, match='float32'):
        s.add_views(img[:1], [E4.astype(np.float64)])
    for bad in ([6], [4, 9], 3, [-1]):
        with pytest.raises(KeyError, match='no view with id'):
            s.remove_views(bad)
    after = _snapshot(s)
    assert after[:2] == before[:2] and after[3:] == before[3:] and all(a is b for a, b in zip(after[2], before[2]))


def test_remove_views_bookkeeping_and_unbounded_sessions():
    from imvoxelnet_amd import SceneSession
    s = _scene_with_views(4, [(0, 0), (1, 1), (2, 2), (3, 3)])
    assert s.remove_views([1]) is s and s.view_ids == [0, 2, 3] and s.n_views == 3 and s._stale
    assert [float(e[0, 0]) for e in s.meta['lidar2img']['extrinsic']] == [1., 3., 4.]
    s.remove_views(np.int64(3))
    assert s.view_ids == [0, 2]
    s._stale = False
    s.remove_views([])
    assert s.view_ids == [0, 2] and not s._stale, 'an empty removal changes nothing'
    s.remove_views((0, 2))
    assert s.view_ids == [] and s.n_views == 0 and s.meta['lidar2img']['extrinsic'] == []
    with pytest.raises(RuntimeError, match='no views'):
        s.volume()
    s.reset()
    assert s._next_id == 0
    u = SceneSession(_mock_model(), META)
    u.n_views = 2
    assert u.view_ids == [0, 1]
    with pytest.raises(RuntimeError, match='window='):
        u.remove_views([0])
    assert u.n_views == 2


def test_calls_after_close():
    s = _scene_with_views(2, [(0, 0)])
    s.close()
    assert s._ring is None and s._pring is None and s._mean is None
    for call in (lambda: s.add_views(torch.zeros(1, 3, 96, 128), [E4]), lambda: s.remove_views([0]), s.detect, s.volume, s.reset,
                 lambda: s.add_views_u8([np.zeros((48, 64, 3), np.uint8)], [E4], (128, 96))):
        with pytest.raises(RuntimeError, match='closed'):
            call()
