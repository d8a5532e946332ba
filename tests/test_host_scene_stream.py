"""Streaming scenes without a device: the three C entry points are declared / bound / exported and reject bad arguments before any
launch; SceneSession raises its pre-launch errors."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from helpers import ROOT

NAMES = ('ivx_backproject_accum_fwd', 'ivx_backproject_accum_fwd_bf16', 'ivx_volume_mean_fwd')


def test_entry_points_declared_bound_and_exported():
    from imvoxelnet_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'imvoxel.h')).read()
    declared = set(re.findall(r'\b(ivx_[a-z0-9_]+)\s*\(', header))
    L = _lib.lib()
    for name in NAMES:
        assert name in declared, f'{name} is not declared in include/imvoxel.h'
        assert name in _lib.EXPORTS
        assert hasattr(L, name) and getattr(L, name).argtypes is not None
    for src in ('model.cpp', 'api_common.cpp'):        # also compiled into the CPU restatement of the ABI, which does not define them
        text = open(os.path.join(ROOT, 'imvoxelnet_amd', 'csrc', src)).read()
        assert not any(name in text for name in NAMES)


@pytest.mark.parametrize('name', NAMES[:2])
def test_accumulate_argument_validation_without_gpu(name):
    """Invalid arguments: status -1 with a message, nothing launched (the pointers are never dereferenced)."""
    from imvoxelnet_amd import _lib
    L = _lib.lib()
    fn = getattr(L, name)
    p = ctypes.c_void_p(64)
    vs = (ctypes.c_float * 3)(.5, .5, .5)

    def call(B=1, V=2, FH=6, FW=8, C=8, X=4, Y=4, Z=2, feat=p, vol_sum=p, count=p, mean=p, valid=p, first=1):
        return fn(feat, B, V, FH, FW, C, p, p, p, vs, X, Y, Z, vol_sum, count, first, mean, valid, None)

    assert call(C=6) == -1 and b'C % 4' in L.ivx_last_error() and name.encode() in L.ivx_last_error()
    assert call(vol_sum=None) == -1 and b'null' in L.ivx_last_error()
    assert call(count=None) == -1 and b'null' in L.ivx_last_error()
    assert call(feat=None) == -1 and b'null' in L.ivx_last_error()
    assert call(valid=None) == -1 and b'both' in L.ivx_last_error()
    assert call(mean=None) == -1 and b'both' in L.ivx_last_error()
    for bad in (dict(B=0), dict(V=0), dict(FH=-1), dict(C=0), dict(X=0), dict(Z=-3)):
        assert call(**bad) == -1 and b'non-positive' in L.ivx_last_error(), bad
    assert call(X=2048, Y=2048, Z=512) == -1 and b'too large' in L.ivx_last_error()
    assert call(C=1028) == -1 and b'too large' in L.ivx_last_error()
    with pytest.raises(ValueError):
        _lib.check(call(C=6), name)


def test_volume_mean_argument_validation_without_gpu():
    from imvoxelnet_amd import _lib
    L = _lib.lib()
    p, q = ctypes.c_void_p(64), ctypes.c_void_p(4096)
    fn = L.ivx_volume_mean_fwd
    assert fn(p, p, 16, 6, q, 0, p, None) == -1 and b'C % 4' in L.ivx_last_error()
    assert fn(None, p, 16, 8, q, 0, p, None) == -1 and b'null' in L.ivx_last_error()
    assert fn(p, None, 16, 8, q, 0, p, None) == -1 and b'null' in L.ivx_last_error()
    assert fn(p, p, 16, 8, None, 0, p, None) == -1 and b'null' in L.ivx_last_error()
    assert fn(p, p, 16, 8, q, 0, None, None) == -1 and b'null' in L.ivx_last_error()
    assert fn(p, p, 0, 8, q, 0, p, None) == -1 and b'bad dims' in L.ivx_last_error()
    assert fn(p, p, 16, 8, q, 2, p, None) == -1 and b'out_dtype' in L.ivx_last_error()          # IVX_FP8: not a volume type
    assert fn(p, p, 16, 8, p, 0, p, None) == -1 and b'in place' in L.ivx_last_error()


def test_ops_wrappers_reject_host_tensors_and_bad_pairs():
    from imvoxelnet_amd import ops
    t = torch.zeros(2, 1, 4, 4, 8)
    with pytest.raises(RuntimeError, match='device'):
        ops.backproject_accum_(t, torch.zeros(1, 2, 3, 4), torch.zeros(1, 3), torch.zeros(1, 2, dtype=torch.int32), (1, 1, 1),
                               torch.zeros(1, 2, 2, 2, 8), torch.zeros(1, 2, 2, 2, dtype=torch.int32), True)
    with pytest.raises(TypeError):
        ops.backproject_accum_(t.half(), None, None, None, (1, 1, 1), None, None, True)
    for pair in (dict(mean_out=torch.zeros(1, 2, 2, 2, 8)), dict(valid_out=torch.zeros(1, 2, 2, 2, dtype=torch.uint8))):
        with pytest.raises(ValueError, match='both'):          # mean_out and valid_out come both or neither: checked first
            ops.backproject_accum_(t, None, None, None, (1, 1, 1), None, None, True, **pair)
    with pytest.raises(RuntimeError, match='device'):
        ops.volume_mean(torch.zeros(1, 2, 2, 2, 8), torch.zeros(1, 2, 2, 2, dtype=torch.int32))


# ------------------------------------------------------------------ the session's pre-launch errors
K = np.array([[90., 0, 63.5, 0], [0, 90., 47.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
META = dict(img_shape=(96, 128, 3), ori_shape=(96, 128, 3), lidar2img=dict(intrinsic=K, origin=np.array([0, 0, .5], np.float32)))


def _mock_model(**kw):
    """What SceneSession touches before its first launch; any device work would fail on the missing attributes."""
    return types.SimpleNamespace(**dict(dict(head_2d=None), **kw))


def test_open_scene_on_an_unprepared_model_and_its_errors():
    import imvoxelnet_amd as ia
    from kitti_cfg import kitti_model_cfg, KITTI_TEST_CFG
    model = ia.build_detector(kitti_model_cfg(n_voxels=(24, 28, 12), in_ch=16, out_ch=32), test_cfg=KITTI_TEST_CFG)
    scene = model.open_scene(META)
    assert isinstance(scene, ia.SceneSession) and scene.n_views == 0 and model._prepared_device is None
    assert 'extrinsic' not in META['lidar2img'], 'the caller\'s meta must stay as it was'
    with pytest.raises(RuntimeError, match='no views'):
        scene.detect()
    with pytest.raises(RuntimeError, match='no views'):
        scene.volume()
    E = np.eye(4, dtype=np.float32)
    img = torch.zeros(2, 3, 96, 128)
    with pytest.raises(ValueError, match='1 extrinsics for 2 views'):
        scene.add_views(img, [E])
    with pytest.raises(TypeError, match='float32'):
        scene.add_views(img, [E, E.astype(np.float64)])
    with pytest.raises(ValueError, match='4x4'):
        scene.add_views(img, [E, E[:3]])
    with pytest.raises(TypeError, match='float32'):
        scene.add_views(img.double(), [E, E])
    with pytest.raises(ValueError, match=r'\[V,3,H,W\]'):
        scene.add_views(img[None], [E, E])
    with pytest.raises(RuntimeError, match='device'):          # everything valid: stops at the host tensor, before prepare() or any launch
        scene.add_views(img, [E, E])
    assert scene.n_views == 0 and model._prepared_device is None
    with pytest.raises(ValueError, match='2 extrinsics for 1 views'):
        scene.add_views_u8([np.zeros((48, 64, 3), np.uint8)], [E, E], (128, 96))
    before = dict(scene.meta)
    with pytest.raises(TypeError, match='float32'):            # a bad extrinsic stops add_views_u8 before the pipeline and the meta
        scene.add_views_u8([np.zeros((48, 64, 3), np.uint8)], [E.astype(np.float64)], (128, 96))
    assert set(scene.meta) == set(before) and all(scene.meta[k] is before[k] for k in before) and scene.meta['lidar2img']['extrinsic'] == []
    scene.close()
    for call in (lambda: scene.add_views(img, [E, E]), scene.detect, scene.volume, scene.reset,
                 lambda: scene.add_views_u8([np.zeros((48, 64, 3), np.uint8)], [E], (128, 96))):
        with pytest.raises(RuntimeError, match='closed'):
            call()


def test_scene_session_refuses_a_head_2d_and_bad_metas():
    from imvoxelnet_amd import SceneSession
    with pytest.raises(NotImplementedError, match='extrinsics from the image'):
        SceneSession(_mock_model(head_2d=object()), META)
    with pytest.raises(ValueError, match='lidar2img'):
        SceneSession(_mock_model(), dict(img_shape=(96, 128, 3)))
    with pytest.raises(TypeError, match='float32'):
        SceneSession(_mock_model(), dict(META, lidar2img=dict(intrinsic=K.astype(np.float64), origin=np.zeros(3, np.float32))))
    # shapes left to add_views_u8: add_views cannot work without them
    s = SceneSession(_mock_model(), dict(lidar2img=META['lidar2img']))
    with pytest.raises(ValueError, match='img_shape'):
        s.add_views(torch.zeros(1, 3, 96, 128), [np.eye(4, dtype=np.float32)])


def test_image_size_must_match_the_first_add():
    from imvoxelnet_amd import SceneSession
    s = SceneSession(_mock_model(), META)
    s._hw, s.n_views = (96, 128), 1                      # as after a first add of 96 x 128 views
    with pytest.raises(ValueError, match='differs'):
        s.add_views(torch.zeros(1, 3, 96, 160), [np.eye(4, dtype=np.float32)])
    s.reset()
    with pytest.raises(RuntimeError, match='device'):    # after reset() another size is a new scene: passes validation
        s.add_views(torch.zeros(1, 3, 96, 160), [np.eye(4, dtype=np.float32)])
