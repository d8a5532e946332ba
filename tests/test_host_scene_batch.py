"""Scene batches without a device: ivx_backproject_lists_fwd is declared / bound / exported and rejects bad arguments before any launch;
ops.backproject_lists_accum_ / _mean_ and SceneBatch (model.open_scenes) raise their pre-launch errors and leave the batch as it was."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from helpers import ROOT

NAME = 'ivx_backproject_lists_fwd'
MEAN, SUM, ACCUM = 0, 1, 2


def test_entry_point_declared_bound_and_exported():
    from imvoxelnet_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'imvoxel.h')).read()
    assert NAME in set(re.findall(r'\b(ivx_[a-z0-9_]+)\s*\(', header)), f'{NAME} is not declared in include/imvoxel.h'
    assert 'typedef struct ivx_lift_lists' in header
    L = _lib.lib()
    assert NAME in _lib.EXPORTS and hasattr(L, NAME) and getattr(L, NAME).argtypes is not None
    assert L.ivx_version() >= 470
    assert [f[0] for f in _lib.LiftLists._fields_] == ['S', 'R', 'view_slot', 'row', 'first']
    for src in ('model.cpp', 'api_common.cpp'):        # also compiled into the CPU restatement of the ABI, which does not define it
        assert NAME not in open(os.path.join(ROOT, 'imvoxelnet_amd', 'csrc', src)).read(), src


def test_lists_argument_validation_without_gpu():
    """Every invalid argument: status -1 with its message, nothing launched (the dummy pointers are never dereferenced)."""
    from imvoxelnet_amd import _lib
    L = _lib.lib()
    fn = getattr(L, NAME)
    p = ctypes.c_void_p(64)

    def call(S=3, R=2, desc=True, lists=True, pool=p, ppool=p, slots=p, row=p, first=None, origin=p, crop=p, vol=p, count=None, mean=None, valid=p, **kw):
        f = dict(B=2, V=2, FH=6, FW=8, C=8, X=4, Y=4, Z=2, feat_dtype=0, mode=MEAN, sampling=0, first=0)
        f.update(kw)
        d = _lib.BackprojectDesc(f['B'], f['V'], f['FH'], f['FW'], f['C'], f['X'], f['Y'], f['Z'], (ctypes.c_float * 3)(.5, .5, .5), f['feat_dtype'],
                                 f['mode'], f['sampling'], f['first'])
        l = _lib.LiftLists(S, R, slots, row, first)
        return fn(ctypes.byref(d) if desc else None, ctypes.byref(l) if lists else None, pool, ppool, origin, crop, vol, count, mean, valid, None)

    def accum(**kw):
        return call(**dict(dict(mode=ACCUM, count=p, valid=None), **kw))

    def err():
        return L.ivx_last_error()

    assert call(desc=False) == -1 and b'null descriptor' in err() and NAME.encode() in err()
    # ---- what this entry adds
    assert call(lists=False) == -1 and b'null lists' in err() and NAME.encode() in err()
    assert accum(lists=False) == -1 and b'null lists' in err()
    for R in (0, -1):
        assert call(R=R) == -1 and b'rows' in err() and NAME.encode() in err(), R
        assert accum(R=R) == -1 and b'rows' in err(), R
    assert call(R=1, row=None) == -1 and b'no row list' in err()                      # row b needs R >= B
    for mode in (SUM, 3, -1):
        assert call(mode=mode, count=p, valid=None) == -1 and b'IVX_LIFT_MEAN | IVX_LIFT_ACCUM' in err(), mode
    assert call(first=p) == -1 and b'the mean mode takes no first list' in err()
    # ---- the pointer rules of the two modes (ivx_backproject_fwd_ex)
    assert call(valid=None) == -1 and b'the mean mode writes valid' in err()
    assert call(count=p) == -1 and b'takes no count' in err()
    assert call(mean=p) == -1 and b'takes no count' in err()
    assert accum(count=None) == -1 and b'updates count' in err()
    assert accum(mean=p) == -1 and b'both be given or both be NULL' in err()
    assert accum(valid=p) == -1 and b'both be given or both be NULL' in err()
    # ---- the gather entry's list, in both modes
    for c in (call, accum):
        for ptr in ('pool', 'ppool', 'slots', 'origin', 'crop', 'vol'):
            assert c(**{ptr: None}) == -1 and b'null argument' in err(), ptr
        for S in (0, -2):
            assert c(S=S) == -1 and b'slots' in err() and NAME.encode() in err()
        for bad in (dict(B=0), dict(V=0), dict(FH=-1), dict(FW=0), dict(C=0), dict(X=0), dict(Y=-1), dict(Z=-3)):
            assert c(**bad) == -1 and b'non-positive' in err(), bad
        for C in (6, 10, 1026):
            assert c(C=C) == -1 and b'C % 4' in err(), C
        assert c(C=1028) == -1 and b'too large (max 1024)' in err()
        for s in (2, -1):
            assert c(sampling=s) == -1 and b'sampling' in err(), s
        for dt in (2, 3, -1):                                # IVX_FP8 and unknown
            assert c(feat_dtype=dt) == -1 and b'feat_dtype' in err(), dt
        assert c(X=2048, Y=2048, Z=512) == -1 and b'voxel grid too large' in err()                # X*Y*Z = 2^31
        assert c(S=1 << 15, FH=256, FW=256) == -1 and b'feature pool too large' in err()          # S*FH*FW = 2^31
        assert c(B=65536, R=65536) == -1 and b'batch too large' in err()
    with pytest.raises(ValueError, match=NAME):
        _lib.check(call(C=6), NAME)
    # the gather entry still refuses every mode but the mean, with its message (tests/test_host_scene_window.py pins it too)
    d = _lib.BackprojectDesc(1, 2, 6, 8, 8, 4, 4, 2, (ctypes.c_float * 3)(.5, .5, .5), 0, ACCUM, 0, 0)
    assert L.ivx_backproject_gather_fwd(ctypes.byref(d), 3, p, p, p, p, p, p, p, None) == -1 and b'IVX_LIFT_MEAN only' in err()


def _host_args(S=4, R=3, C=8):
    pool, ppool = torch.zeros(S, 1, 4, 4, C), torch.zeros(S, 3, 4)
    no, crop = torch.zeros(2, 3), torch.zeros(2, 2, dtype=torch.int32)
    st = dict(sum=torch.zeros(R, 2, 2, 2, C), count=torch.zeros(R, 2, 2, 2, dtype=torch.int32), mean=torch.zeros(R, 2, 2, 2, C),
              valid=torch.zeros(R, 2, 2, 2, dtype=torch.uint8))
    return pool, ppool, no, crop, st


def test_ops_reject_bad_lists_rows_and_host_tensors_before_any_launch():
    """Host tensors throughout, so nothing here can reach a launch: the list errors come first (ValueError / TypeError), and arguments
    that pass them stop at the first host tensor (RuntimeError)."""
    from imvoxelnet_amd import ops
    pool, ppool, no, crop, st = _host_args()
    vs = (1, 1, 1)

    def accum(lists=([0, 1, 2], [3]), rows=(2, 0), first=(True, False), pool=pool, ppool=ppool, no=no, crop=crop, mean=True, **kw):
        return ops.backproject_lists_accum_(pool, ppool, [list(l) for l in lists], list(rows), list(first), no, crop, vs, st['sum'], st['count'],
                                            st['mean'] if mean else None, st['valid'] if mean else None, **kw)

    def mean(lists=([0, 1, 2], [3]), rows=(2, 0), pool=pool, **kw):
        return ops.backproject_lists_mean_(pool, ppool, [list(l) for l in lists], list(rows), no, crop, vs, st['mean'], st['valid'], **kw)

    for op in (accum, mean):
        with pytest.raises(ValueError, match='distinct'):
            op(rows=(1, 1))
        for rows in ((0, 3), (-1, 0)):
            with pytest.raises(ValueError, match=r'rows must be in \[0, 3\)'):
                op(rows=rows)
        for rows in ((0,), (0, 1, 2)):
            with pytest.raises(ValueError, match='entries for 2 samples'):
                op(rows=rows)
        for lists, bad in ((([0, 4], [1]), r'\[4\]'), (([0, -2], [1]), r'\[-2\]'), (([-1, 0, 9], [-3]), r'\[-3, 9\]')):
            with pytest.raises(ValueError, match=r'outside \[0, 4\) other than the padding -1: ' + bad):
                op(lists=lists)
        with pytest.raises(TypeError, match='integers'):
            op(lists=([0.5], [1]))
        with pytest.raises(ValueError, match='sampling'):
            op(sampling='cubic')
        for dt in (torch.float16, torch.float64):
            with pytest.raises(TypeError, match='float32 or bfloat16'):
                op(pool=pool.to(dt))
        # ragged lists with -1 padding and an empty list pass the list checks: the host pool is refused next
        with pytest.raises(RuntimeError, match='pool must be a device'):
            op(lists=([0, -1, 2], []))
    with pytest.raises(TypeError, match='host list'):
        ops.backproject_lists_mean_(pool, ppool, torch.tensor([[0, 1], [2, 3]]), [0, 1], no, crop, vs, st['mean'], st['valid'])
    with pytest.raises(TypeError, match='host list'):
        ops.backproject_lists_mean_(pool, ppool, [[0], [1]], torch.tensor([0, 1]), no, crop, vs, st['mean'], st['valid'])
    for first in ((True,), (True, False, True)):
        with pytest.raises(ValueError, match='first must be a host list of 2'):
            accum(first=first)
    with pytest.raises(ValueError, match='both be given or both be None'):
        ops.backproject_lists_accum_(pool, ppool, [[0], [1]], [0, 1], [True, True], no, crop, vs, st['sum'], st['count'], st['mean'], None)
    with pytest.raises(ValueError, match='proj_pool'):
        accum(ppool=ppool[:2])
    with pytest.raises(ValueError, match=r'\[R,X,Y,Z,C\]'):
        ops.backproject_lists_mean_(pool, ppool, [[0], [1]], [0, 1], no, crop, vs, torch.zeros(3, 2, 2, 2, 4), st['valid'])
    # the existing op keeps its rule: -1 in a host list raises
    with pytest.raises(ValueError, match=r'outside \[0, 4\)'):
        ops.backproject_gather_mean(pool, ppool, [[0, -1]], no[:1], crop[:1], vs, (2, 2, 2))


# ------------------------------------------------------------------ the batch's pre-launch errors
K = np.array([[90., 0, 63.5, 0], [0, 90., 47.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
META = dict(img_shape=(96, 128, 3), ori_shape=(96, 128, 3), lidar2img=dict(intrinsic=K, origin=np.array([0, 0, .5], np.float32)))
E4 = np.eye(4, dtype=np.float32)


def _mock_model(**kw):
    """What SceneBatch touches before its first launch; any device work would fail on the missing attributes."""
    return types.SimpleNamespace(**dict(dict(head_2d=None), **kw))


def _batch(N=3, window=None, views=None):
    """A batch as after adds, without any device work: views = per-scene lists of (id, slot) (windowed) or view counts (unbounded)."""
    from imvoxelnet_amd import SceneBatch
    b = SceneBatch(_mock_model(), [META] * N, window=window)
    for s, v in enumerate(views or []):
        r = b._scenes[s]
        if window is None:
            r.n_views = v
            r.meta['lidar2img']['extrinsic'] = [E4 * (i + 1) for i in range(v)]
        else:
            r._views = [(i, slot, E4 * (i + 1)) for i, slot in v]
            r.meta['lidar2img']['extrinsic'] = [x[2] for x in r._views]
            r.n_views, r._next_id = len(v), max([i for i, _ in v], default=-1) + 1
    if any(b.n_views):
        b._hw = (96, 128)
    return b


def _snapshot(b):
    return ([b.view_ids(s) for s in range(len(b))], list(b.n_views), [list(m['lidar2img']['extrinsic']) for m in b.metas],
            [{k: v for k, v in m.items() if k != 'lidar2img'} for m in b.metas], [r._stale for r in b._scenes], b._hw)


def _same_snapshot(a, b):
    return a[:2] == b[:2] and a[3:] == b[3:] and all(x is y for la, lb in zip(a[2], b[2]) for x, y in zip(la, lb)) and [len(l) for l in a[2]] == [len(l) for l in b[2]]


def test_open_scenes_and_its_refusals():
    import imvoxelnet_amd as ia
    from kitti_cfg import kitti_model_cfg, KITTI_TEST_CFG
    model = ia.build_detector(kitti_model_cfg(n_voxels=(24, 28, 12), in_ch=16, out_ch=32), test_cfg=KITTI_TEST_CFG)
    b = model.open_scenes([META, META], window=2)
    assert isinstance(b, ia.SceneBatch) and len(b) == 2 and b._window == 2 and b.n_views == [0, 0] and b.view_ids(1) == []
    assert model.open_scenes([META])._window is None
    assert b.metas[0] is not b.metas[1] and b.metas[0]['lidar2img'] is not b.metas[1]['lidar2img'], 'every scene has a meta of its own'
    with pytest.raises(ValueError, match='window'):
        model.open_scenes([META], window=0)
    with pytest.raises(ValueError, match='at least one'):
        model.open_scenes([])
    with pytest.raises(ValueError, match='lidar2img'):
        model.open_scenes([META, dict(img_shape=(96, 128, 3))])
    with pytest.raises(NotImplementedError, match='head_2d'):
        ia.SceneBatch(_mock_model(head_2d=object()), [META])
    assert model._prepared_device is None
    assert 'batches of scenes in one session' not in ia.scene.__doc__


@pytest.mark.parametrize('window', [None, 2])
def test_calls_that_raise_leave_the_batch_as_it_was(window):
    b = _batch(3, window, [2, 0, 1] if window is None else [[(3, 1), (4, 0)], [], [(0, 4)]])
    before = _snapshot(b)
    assert before[1] == [2, 0, 1]
    img = torch.zeros(3, 3, 96, 128)
    for scene in ([0, 1], [0, 1, 2, 0], 1, None):
        with pytest.raises(ValueError, match='one scene index per view'):
            b.add_views(img, [E4] * 3, scene)
    for scene in ([0, 1, 3], [-1, 0, 0], [0, 1.0, 2], [True, 0, 0]):
        with pytest.raises(ValueError, match='unknown scene index'):
            b.add_views(img, [E4] * 3, scene)
    if window is not None:
        with pytest.raises(ValueError, match='3 views of scene 1 in one call do not fit a window of 2'):      # stops before the host-tensor check
            b.add_views(img, [E4] * 3, [1, 1, 1])
        with pytest.raises(ValueError, match='do not fit'):
            b.add_views_u8([np.zeros((48, 64, 3), np.uint8)] * 3, [E4] * 3, [2, 2, 2], (128, 96))
        for bad in ([6], [3, 9]):
            with pytest.raises(KeyError, match='no view with id'):
                b.remove_views(0, bad)
    else:
        with pytest.raises(RuntimeError, match='window='):
            b.remove_views(0, [0])
    with pytest.raises(ValueError, match='unknown scene index'):
        b.remove_views(3, [0])
    with pytest.raises(RuntimeError, match='device'):            # valid arguments: stops at the host tensor, before any launch
        b.add_views(img, [E4] * 3, [0, 0, 2] if window is None else [0, 1, 1])
    with pytest.raises(ValueError, match='differs'):
        b.add_views(torch.zeros(1, 3, 96, 160), [E4], [0])
    with pytest.raises(ValueError, match='2 extrinsics for 3 views'):
        b.add_views(img, [E4] * 2, [0, 1, 2])
    with pytest.raises(TypeError, match='float32'):
        b.add_views(img[:1], [E4.astype(np.float64)], [0])
    with pytest.raises(RuntimeError, match=r'scenes \[1\] have no views'):
        b.detect([0, 1])
    with pytest.raises(RuntimeError, match='no views'):
        b.volume(1)
    with pytest.raises(ValueError, match='unknown scene index'):
        b.detect([5])
    assert _same_snapshot(_snapshot(b), before)


def test_bookkeeping_reset_and_close():
    b = _batch(2, 3, [[(0, 0), (1, 1), (2, 2)], [(5, 4)]])
    assert b.remove_views(0, [1]) is b and b.view_ids(0) == [0, 2] and b.n_views == [2, 1] and b._scenes[0]._stale and not b._scenes[1]._stale
    assert b.reset(scenes=[1]) is b and b.n_views == [2, 0] and b.view_ids(0) == [0, 2] and b._hw == (96, 128)
    b.reset()
    assert b.n_views == [0, 0] and b._hw is None and all(m['lidar2img']['extrinsic'] == [] for m in b.metas)
    with pytest.raises(RuntimeError, match='no scene of the batch has views'):
        b.detect()
    b.close()
    for call in (lambda: b.add_views(torch.zeros(1, 3, 96, 128), [E4], [0]), lambda: b.remove_views(0, [0]), b.detect, lambda: b.volume(0), b.reset,
                 lambda: b.view_ids(0), lambda: b.add_views_u8([np.zeros((48, 64, 3), np.uint8)], [E4], [0], (128, 96))):
        with pytest.raises(RuntimeError, match='closed'):
            call()


def test_simple_test_ragged_argument_errors_before_any_launch():
    import imvoxelnet_amd as ia
    from kitti_cfg import kitti_model_cfg, KITTI_TEST_CFG
    model = ia.build_detector(kitti_model_cfg(n_voxels=(24, 28, 12), in_ch=16, out_ch=32), test_cfg=KITTI_TEST_CFG)

    def meta(n):
        return dict(META, lidar2img=dict(META['lidar2img'], extrinsic=[E4] * n))

    imgs = [torch.zeros(2, 3, 96, 128), torch.zeros(1, 3, 96, 128)]
    with pytest.raises(ValueError, match='1 img_metas for 2 samples'):
        model.simple_test_ragged(imgs, [meta(2)])
    with pytest.raises(ValueError, match='sample 1: 2 extrinsics for 1 views'):
        model.simple_test_ragged(imgs, [meta(2), meta(2)])
    with pytest.raises(ValueError, match='one image size'):
        model.simple_test_ragged([imgs[0], torch.zeros(1, 3, 96, 160)], [meta(2), meta(1)])
    with pytest.raises(RuntimeError, match='device'):
        model.simple_test_ragged(imgs, [meta(2), meta(1)])
    assert model._prepared_device is None
    model.head_2d = object()
    with pytest.raises(NotImplementedError, match='head_2d'):
        model.simple_test_ragged(imgs, [meta(2), meta(1)])
    # simple_test's rule for a dense batch stays
    model.head_2d = None
    with pytest.raises(ValueError, match='same number of views'):
        model._camera_setup([meta(2), meta(1)], 4, torch.device('cpu'))
