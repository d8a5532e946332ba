"""Warping scenes without a device: ivx_volume_warp_fwd is declared, bound and exported and rejects bad arguments before any launch;
ops.volume_warp raises its host errors (non-rigid, reflecting and non-finite transforms among them); warped_extrinsic, `frame` and the host side of
SceneSession.warp / SceneBatch.warp on empty and plain scenes; the numpy reference of tests/ref_volume_warp.py against itself: the identity, a
whole-voxel translation on a dyadic grid against ref_volume_scroll, a quarter turn about the centre of a square dyadic grid as a permutation."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import ref_volume_scroll as RS
import ref_volume_warp as RW
from helpers import ROOT

NAME = 'ivx_volume_warp_fwd'
EYE = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]


def test_entry_point_declared_bound_and_exported():
    from imvoxelnet_amd import _lib, _build
    header = open(os.path.join(ROOT, 'include', 'imvoxel.h')).read()
    declared = set(re.findall(r'\b(ivx_[a-z0-9_]+)\s*\(', header))
    L = _lib.lib()
    assert NAME in declared, f'{NAME} is not declared in include/imvoxel.h'
    assert NAME in _lib.EXPORTS and hasattr(L, NAME) and getattr(L, NAME).argtypes is not None and len(getattr(L, NAME).argtypes) == 20
    assert L.ivx_version() >= 540
    for src in ('model.cpp', 'api_common.cpp'):        # also compiled into the CPU restatement of the ABI, which does not define it
        assert NAME not in open(os.path.join(ROOT, 'imvoxelnet_amd', 'csrc', src)).read(), src
    entry = [e for e in _build.SOURCES if e[0] == 'volume_warp.hip']
    assert len(entry) == 1 and '-ffp-contract=off' in entry[0][1]


def _call(L, rows_src=(2, 0), rows_dst=(0, 1), xform=None, origin=None, vs=(0.25, 0.25, 0.5), forget=0.0, B=None, R=(3, 2), dims=(7, 5, 6), C=8,
          src=(1 << 20, 2 << 20, 3 << 20), dst=(4 << 20, 5 << 20, 6 << 20), null=()):
    """The entry with dummy device pointers (never dereferenced: every call here is rejected before any launch)."""
    n = len(rows_src)
    B = n if B is None else B
    f32, i32 = ctypes.c_float, ctypes.c_int32
    xform = EYE * n if xform is None else xform
    origin = [0.0] * (3 * n) if origin is None else origin
    host = dict(row_src=(i32 * max(1, n))(*rows_src), row_dst=(i32 * max(1, n))(*rows_dst), xform=(f32 * max(1, len(xform)))(*xform),
                new_origin=(f32 * max(1, len(origin)))(*origin), voxel_size=(f32 * 3)(*vs))
    p = lambda name, a: None if name in null else ctypes.c_void_p(a)     # noqa: E731
    h = lambda name: None if name in null else host[name]                # noqa: E731
    return getattr(L, NAME)(B, h('row_src'), h('row_dst'), h('xform'), h('new_origin'), h('voxel_size'), forget, R[0], R[1], *dims, C,
                            p('sum_src', src[0]), p('wsum_src', src[1]), p('count_src', src[2]), p('sum_dst', dst[0]), p('wsum_dst', dst[1]),
                            p('count_dst', dst[2]), None)


def test_argument_validation_without_gpu():
    """Every pre-launch rejection: status -1 with its message, which names the export; nothing is launched."""
    from imvoxelnet_amd import _lib
    L = _lib.lib()
    nan, inf = float('nan'), float('inf')

    def rejected(word, **kw):
        rc, err = _call(L, **kw), L.ivx_last_error()
        assert rc == -1 and word in err and NAME.encode() in err, (kw, rc, err)

    for name in ('row_src', 'row_dst', 'xform', 'new_origin', 'voxel_size', 'sum_src', 'wsum_src', 'count_src', 'sum_dst', 'wsum_dst', 'count_dst'):
        rejected(b'null argument', null=(name,))
    for kw in (dict(B=0), dict(B=-1), dict(R=(0, 2)), dict(R=(3, -1)), dict(dims=(0, 5, 6)), dict(dims=(7, -1, 6)), dict(dims=(7, 5, 0)), dict(C=0), dict(C=-4)):
        rejected(b'bad dims', **kw)
    for c in (1, 2, 6, 10):
        rejected(b'C % 4', C=c)
    for dims in ((2048, 1024, 1024), (65536, 32768, 1), (1290, 1290, 1291)):
        rejected(b'below 2^31', dims=dims)
    for rows in ((2, 3), (-1, 0)):
        rejected(b'row_src', rows_src=rows)
        rejected(b'outside [0, 3)', rows_src=rows)
    for rows in ((0, 2), (-1, 0)):
        rejected(b'row_dst', rows_dst=rows)
        rejected(b'outside [0, 2)', rows_dst=rows)
    rejected(b'distinct', rows_dst=(1, 1))
    assert b'row 1' in L.ivx_last_error()
    assert _call(L, rows_src=(1, 1), rows_dst=(3, 0), R=(3, 2)) == -1 and b'row_dst' in L.ivx_last_error()        # (two samples may READ one row; this one fails on its row_dst)
    row_bytes = 7 * 5 * 6 * 8 * 4
    for dst0 in ((1 << 20), (1 << 20) + 3 * row_bytes - 16, (1 << 20) - 2 * row_bytes + 16, (1 << 20) + row_bytes):       # the same pool, the last / first 16 bytes, a row inside
        rejected(b'overlap', dst=(dst0, 5 << 20, 6 << 20))
    for bad in (nan, inf, -inf):
        for at in (0, 3, 11, 23):
            x = EYE * 2
            x[at] = bad
            rejected(b'finite', xform=x)
        rejected(b'finite', origin=[0, 0, 0, 0, bad, 0])
        rejected(b'finite', vs=(0.25, bad, 0.5))
        rejected(b'forget_below', forget=bad)
    for vs in ((0.0, 0.25, 0.5), (0.25, -0.25, 0.5), (0.25, 0.25, -1e-30)):
        rejected(b'voxel_size must be positive', vs=vs)
    for f in (-1.0, -1e-30):
        rejected(b'forget_below', forget=f)
    with pytest.raises(ValueError, match=NAME):
        _lib.check(_call(L, rows_dst=(1, 1)), NAME)


def _state(R=3, dims=(7, 5, 6), C=8):
    return (torch.full((R,) + dims + (C,), 3.0), torch.full((R,) + dims, 5.0), torch.full((R,) + dims, 9, dtype=torch.int32))


def test_check_rigid():
    from imvoxelnet_amd import ops
    T = RW.rigid(0.3, -0.1, 0.05, (0.4, -0.2, 0.1), (1, 2, 3))
    for ok in (T, T[:3], T.astype(np.float32), torch.from_numpy(T), T.tolist(), np.eye(4)):
        got = ops.check_rigid(ok)
        assert got.dtype == np.float32 and got.shape == (3, 4) and np.array_equal(got, np.asarray(ok, np.float64)[:3].astype(np.float32))
    scale, shear, mirror, row = T.copy(), T.copy(), T.copy(), T.copy()
    scale[:3, :3] *= 1.001
    shear[0, 1] += 1e-3
    mirror[:3, 0] *= -1
    row[3] = [0, 0, 0, 2]
    for bad, word in ((scale, 'not rigid'), (shear, 'not rigid'), (mirror, 'reflection'), (row, 'last row'), (np.zeros((3, 4)), 'not rigid')):
        with pytest.raises(ValueError, match=word):
            ops.check_rigid(bad)
    for v in (np.nan, np.inf):
        for at in ((0, 0), (1, 3), (3, 3)):
            bad = T.copy()
            bad[at] = v
            with pytest.raises(ValueError, match='finite'):
                ops.check_rigid(bad)
    for bad in (np.eye(3), np.eye(5), np.zeros((2, 4, 4)), 1.0):
        with pytest.raises(ValueError, match='4x4 or 3x4'):
            ops.check_rigid(bad)
    for bad in ('abc', [['a'] * 4] * 4, None):
        with pytest.raises((TypeError, ValueError)):
            ops.check_rigid(bad)
    # the tolerance is a condition, not a measurement: a float32 rotation passes by three orders of magnitude, 2e-4 of scale does not
    R32 = T[:3, :3].astype(np.float32).astype(np.float64)
    assert np.abs(R32.T @ R32 - np.eye(3)).max() < 1e-6 and ops.RIGID_TOL == 1e-4
    barely = T.copy()
    barely[:3, :3] *= 1 + 2e-5                                               # R^T R - I = 4e-5
    ops.check_rigid(barely)
    off = T.copy()
    off[:3, :3] *= 1 + 1e-4                                                  # 2e-4
    with pytest.raises(ValueError, match='not rigid'):
        ops.check_rigid(off)


def test_ops_raise_their_host_errors_and_leave_the_buffers():
    """Host tensors throughout, so nothing can reach a launch: list, transform and shape errors come first, and arguments that pass them stop at the
    first host tensor.  The buffers keep every value."""
    from imvoxelnet_amd import ops
    vol, ws, cnt = _state()
    out = _state(2)
    keep = [t.clone() for t in (vol, ws, cnt) + out]
    T = RW.rigid(0.2, t=(0.1, 0, 0))

    def op(rows=(2, 0), Ts=(T, np.eye(4)), o=((0, 0, 0), (1, 1, 1)), vs=(0.25, 0.25, 0.5), v=vol, w=ws, c=cnt, out=out, out_rows=(0, 1), forget=0.0):
        return ops.volume_warp(v, w, c, list(rows), list(Ts), o, vs, out=out, out_rows=None if out_rows is None else list(out_rows), forget_below=forget)

    with pytest.raises(ValueError, match='distinct'):
        op(out_rows=(1, 1))
    with pytest.raises(ValueError, match=r'rows must be in \[0, 3\)'):
        op(rows=(0, 3))
    with pytest.raises(ValueError, match=r'out_rows must be in \[0, 2\)'):
        op(out_rows=(0, 2))
    with pytest.raises(ValueError, match=r'out_rows must be in \[0, 2\)'):
        op(out_rows=None)                                                    # None means rows, and row 2 is not in the out pools
    with pytest.raises(ValueError, match='at least one row'):
        op(rows=(), Ts=(), o=np.zeros((0, 3)), out_rows=())
    with pytest.raises(ValueError, match='out_rows has 1 entries'):
        op(out_rows=(0,))
    for bad in ((0.0, 1), (True, 2)):
        with pytest.raises(TypeError, match='integers'):
            op(rows=bad)
    with pytest.raises(ValueError, match='one matrix per row'):
        op(Ts=(T,))
    scale, mirror, nan = T.copy(), T.copy(), T.copy()
    scale[:3, :3] *= 1.01
    mirror[:3, 1] *= -1
    nan[1, 3] = np.nan
    for bad, word in ((scale, r'transforms\[1\] is not rigid'), (mirror, 'reflection'), (nan, r'transforms\[1\] must be finite'), (np.eye(3), '4x4 or 3x4')):
        with pytest.raises(ValueError, match=word):
            op(Ts=(T, bad))
    with pytest.raises(TypeError, match='transforms'):
        ops.volume_warp(vol, ws, cnt, [2, 0], 3.0, np.zeros((2, 3)), (0.25, 0.25, 0.5), out=out, out_rows=[0, 1])
    for o in (np.zeros((3, 3)), np.zeros(2), [[0, 0, np.nan], [0, 0, 0]], [[0, 0, np.inf], [0, 0, 0]]):
        with pytest.raises(ValueError, match='new_origin'):
            op(o=o)
    for vs in ((0.25, 0.25), (0.25, 0.0, 0.5), (0.25, -1, 0.5), (0.25, np.nan, 0.5)):
        with pytest.raises(ValueError, match='voxel_size'):
            op(vs=vs)
    for f in (-1.0, np.nan, np.inf, True, '1'):
        with pytest.raises(ValueError, match='forget_below'):
            op(forget=f)
    with pytest.raises(ValueError, match=r'\[R,X,Y,Z,C\]'):
        op(v=vol[0])
    with pytest.raises(ValueError, match='C % 4'):
        op(v=torch.zeros(3, 7, 5, 6, 6), out=(torch.zeros(2, 7, 5, 6, 6),) + out[1:])
    with pytest.raises(ValueError, match='wsum must be'):
        op(w=ws[:2])
    with pytest.raises(ValueError, match='count must be'):
        op(c=cnt[:, :3])
    with pytest.raises(ValueError, match=r'out\[0\] must be'):
        op(out=(torch.zeros(2, 7, 5, 6, 4),) + out[1:])
    with pytest.raises(ValueError, match=r'out\[2\] must be'):
        op(out=out[:2] + (cnt[:1],))
    with pytest.raises(TypeError, match='out must be a'):
        op(out=None)
    with pytest.raises(TypeError, match='out must be a'):
        op(out=out[:2])
    with pytest.raises(TypeError, match='vol_sum must be a torch.Tensor'):
        op(v=vol.numpy())
    with pytest.raises(RuntimeError, match='vol_sum must be a device'):      # everything host-checkable passed: the device check is last
        op()
    with pytest.raises(RuntimeError, match='device'):                        # one matrix alone for one row, one origin for all
        ops.volume_warp(vol, ws, cnt, [1], T, (0, 0, 0), (0.25, 0.25, 0.5), out=out, out_rows=[0])
    for t, k in zip((vol, ws, cnt) + out, keep):
        assert torch.equal(t, k)


# ------------------------------------------------------------------ warped_extrinsic, frame and the sessions' host side
VS = (0.16, 0.16, 0.2)
K4 = np.array([[90., 0, 63.5, 0], [0, 90., 47.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
ORIGIN = np.array([0.37, -1.21, .5], np.float32)
META = dict(img_shape=(96, 128, 3), ori_shape=(96, 128, 3), lidar2img=dict(intrinsic=K4, origin=ORIGIN))


def _mock_model(**kw):
    return types.SimpleNamespace(**dict(dict(head_2d=None, voxel_size=VS, n_voxels=(40, 40, 16)), **kw))


def test_warped_extrinsic_is_the_stated_rule():
    from imvoxelnet_amd import warped_extrinsic
    from imvoxelnet_amd.scene import warped_extrinsic as same
    assert same is warped_extrinsic
    rng = np.random.default_rng(3)
    for _ in range(50):
        E = RW.rigid(*rng.uniform(-3, 3, 3), rng.uniform(-5, 5, 3)).astype(np.float32)
        T = RW.rigid(*rng.uniform(-3, 3, 3), rng.uniform(-5, 5, 3))
        got = warped_extrinsic(E, T)
        assert got.dtype == np.float32 and got.shape == (4, 4) and np.array_equal(got, (E.astype(np.float64) @ T).astype(np.float32))
        x_new = rng.uniform(-4, 4, 3)                                         # the camera sees the same point: E x_old == E' x_new with x_old = T x_new
        x_old = T[:3, :3] @ x_new + T[:3, 3]
        assert np.allclose(E[:3, :3].astype(np.float64) @ x_old + E[:3, 3], got[:3, :3].astype(np.float64) @ x_new + got[:3, 3], atol=1e-4)
    assert np.array_equal(warped_extrinsic(np.eye(4, dtype=np.float32), np.eye(4)), np.eye(4, dtype=np.float32))


def test_session_warp_on_an_empty_scene_changes_only_the_frame():
    """No views, so no state and no launch: `frame` composes on the right, reset() makes it the identity, the identity changes nothing, bad
    transforms raise and change nothing; the origin never moves; a closed session raises."""
    from imvoxelnet_amd import SceneSession
    T1, T2 = RW.rigid(0.3, t=(0.5, 0.1, 0)), RW.rigid(-0.1, 0.02, 0.01, (0, 0.2, 0.05))
    for kw in (dict(decay=0.75), dict(decay=1.0, forget_below=0.5), dict(window=3)):
        s = SceneSession(_mock_model(), META, **kw)
        assert s.frame.dtype == np.float64 and np.array_equal(s.frame, np.eye(4))
        assert s.warp(T1) is s
        assert np.array_equal(s.frame, T1) and not s._stale and s.n_views == 0 and s.meta['lidar2img']['extrinsic'] == []
        s.warp(T2.astype(np.float32))
        want = T1 @ T2.astype(np.float32).astype(np.float64)
        assert np.array_equal(s.frame, want) and np.array_equal(s.meta['lidar2img']['origin'], ORIGIN)
        x = np.array([0.3, -0.2, 0.1, 1.0])                                   # x_opening = frame @ x_grid
        assert np.allclose(s.frame @ x, T1 @ (T2 @ x), atol=1e-6)
        s.frame[0, 0] = 7                                                     # a copy: read-only
        assert np.array_equal(s.frame, want)
        with pytest.raises(AttributeError):
            s.frame = np.eye(4)
        s.warp(np.eye(4))
        assert np.array_equal(s.frame, want)
        scale, mirror = T1.copy(), T1.copy()
        scale[:3, :3] *= 1.01
        mirror[:3, 2] *= -1
        for bad in (scale, mirror, T1[:3], np.eye(3), np.full((4, 4), np.nan), 'T', None, 2.0):
            with pytest.raises((ValueError, TypeError)):
                s.warp(bad)
        assert np.array_equal(s.frame, want)
        s.reset()
        assert np.array_equal(s.frame, np.eye(4))
        s.close()
        with pytest.raises(RuntimeError, match='closed'):
            s.warp(T1)


def test_plain_scenes_refuse_and_go_on():
    from imvoxelnet_amd import SceneSession, SceneBatch
    T = RW.rigid(0.3, t=(0.5, 0.1, 0))
    s = SceneSession(_mock_model(), META)
    with pytest.raises(NotImplementedError, match='decay=1.0'):
        s.warp(T)
    assert np.array_equal(s.frame, np.eye(4)) and s.n_views == 0 and not s._stale
    b = SceneBatch(_mock_model(), [META] * 2)
    with pytest.raises(NotImplementedError, match='decay=1.0'):
        b.warp(0, T)
    assert np.array_equal(b.frame(0), np.eye(4))


def test_batch_warp_host_side_and_a_raising_call_changes_nothing():
    from imvoxelnet_amd import SceneBatch
    T1, T2 = RW.rigid(0.3, t=(0.5, 0.1, 0)), RW.rigid(-0.2, t=(0, 0.3, 0))
    for kw in (dict(decay=0.9), dict(window=2)):
        b = SceneBatch(_mock_model(), [META] * 3, **kw)
        assert b.warp([2, 0], [T1, T2]) is b
        assert np.array_equal(b.frame(2), T1) and np.array_equal(b.frame(0), T2) and np.array_equal(b.frame(1), np.eye(4))
        b.warp(1, T1)                                                         # one index with one T
        b.warp(2, T2)
        assert np.array_equal(b.frame(1), T1) and np.array_equal(b.frame(2), T1 @ T2)
        bad = T1.copy()
        bad[:3, :3] *= 1.01
        for scenes, Ts, exc in (([0, 3], [T1, T1], ValueError), ([0, 0], [T1, T1], ValueError), ([0, 1], [T1], ValueError), (-1, T1, ValueError),
                                ([0, 1], [T1, bad], ValueError), ([0, 1], [T1, np.eye(3)], ValueError)):
            with pytest.raises(exc):
                b.warp(scenes, Ts)
        assert np.array_equal(b.frame(0), T2) and np.array_equal(b.frame(1), T1) and np.array_equal(b.frame(2), T1 @ T2)
        b.reset([0])
        assert np.array_equal(b.frame(0), np.eye(4)) and np.array_equal(b.frame(1), T1)
        b.close()
        with pytest.raises(RuntimeError, match='closed'):
            b.warp(0, T1)


def test_anchor_head_models_accept_warp_and_still_refuse_scroll():
    import imvoxelnet_amd as ia
    from kitti_cfg import kitti_model_cfg, KITTI_TEST_CFG
    model = ia.build_detector(kitti_model_cfg(n_voxels=(24, 28, 12), in_ch=16, out_ch=32), test_cfg=KITTI_TEST_CFG)
    T = RW.rigid(0.05, t=(0.4, 0.02, 0))
    s = model.open_scene(META, decay=0.9)
    assert s.warp(T) is s and np.array_equal(s.frame, T) and np.array_equal(s.meta['lidar2img']['origin'], ORIGIN)
    with pytest.raises(NotImplementedError, match='anchors'):
        s.scroll((1, 0, 0))
    b = model.open_scenes([META, META], window=2)
    b.warp([1], [T])
    assert np.array_equal(b.frame(1), T)


def test_the_docs_speak_of_warping():
    import imvoxelnet_amd as ia
    doc = ia.scene.__doc__
    assert 'Warping scenes' in doc and 'warped_extrinsic' in doc and 'ivx_volume_warp_fwd' in doc
    out = doc[doc.index('Out of scope'):]
    assert 'by a rotation' not in out and 'plain session' in out and 'non-rigid' in out and 'Anchor3DHead' in out
    assert 'twice' in ia.SceneSession.warp.__doc__
    assert 'volume_warp' in open(os.path.join(ROOT, 'DESIGN.md')).read() and 'warping scenes' in open(os.path.join(ROOT, 'README.md')).read().lower()
    assert os.path.exists(os.path.join(ROOT, 'profiles', 'scene_warp.md')) and os.path.exists(os.path.join(ROOT, 'tools', 'scene_warp_bench.py'))


# ------------------------------------------------------------------ the reference against itself
def _row(dims, C, seed):
    rng = np.random.default_rng(seed)
    W = rng.uniform(0.5, 4.0, dims).astype(np.float32)
    return (rng.standard_normal(dims + (C,)) * W[..., None]).astype(np.float32), W, rng.integers(1, 9, dims).astype(np.int32)


def test_reference_identity_keeps_every_value():
    for dims, vs, o in (((7, 5, 6), (0.25, 0.125, 0.5), (-0.75, 0.375, -1.0)), ((6, 6, 3), (0.25, 0.25, 0.5), (-0.75, -0.75, 0.0))):
        S, W, c = _row(dims, 4, 1)
        r = RW.warp_grid(S, W, c, vs, o, np.eye(4))
        # p * 1 + 0 + 0 + 0 is p, and (p - o) / vs gives back the index exactly on these dyadic grids: one corner of weight 1 per voxel.  (On a
        # grid like 0.16 the rounded chain does not return the index exactly; the scenes never launch the identity.)
        assert r['read'].sum() == np.prod(dims) and r['read'][..., 0].all()
        assert np.array_equal(r['S'], S.astype(np.float64)) and np.array_equal(r['W'], W.astype(np.float64)) and np.array_equal(r['cnt'], c)
        assert RW.K_WARP == 11


@pytest.mark.parametrize('shift', [(1, 0, 0), (0, -2, 0), (0, 0, 1), (2, -1, 1), (-3, 2, -2), (6, 0, 0), (0, 0, -4)], ids=lambda s: '_'.join(map(str, s)))
def test_reference_whole_voxel_translation_on_a_dyadic_grid_is_the_scroll(shift):
    """voxel sizes (0.25, 0.25, 0.5) and an origin on their lattice: every step of the chain is exact, g is the index plus the shift, and the warp by
    the translation t = shift * voxel_size equals ref_volume_scroll: the same values where the source stayed inside, unseen elsewhere."""
    dims, vs, o = (6, 5, 4), (0.25, 0.25, 0.5), (-0.75, 0.5, -1.0)
    S, W, c = _row(dims, 8, 2)
    T = np.eye(4)
    T[:3, 3] = np.asarray(shift) * np.asarray(vs)
    r = RW.warp_grid(S, W, c, vs, o, T)
    assert np.array_equal(r['S'].astype(np.float32), RS.scroll_grid(S, shift)) and np.array_equal(r['W'].astype(np.float32), RS.scroll_grid(W, shift))
    assert np.array_equal(r['cnt'], RS.scroll_grid(c, shift))
    assert np.array_equal(r['read'].any(-1), RS.stayed_inside(dims, shift)) and r['read'].sum(-1).max() <= 1


def test_reference_quarter_yaw_about_the_centre_of_a_square_dyadic_grid_is_a_permutation():
    """x_old = (cx - (y - cy), cy + (x - cx), z) about the centre of the voxel-centre lattice: new[i,j,k] = old[N-1-j, i, k], every value once."""
    N, Z, vs, o = 6, 3, (0.25, 0.25, 0.5), np.array([-0.75, 0.5, -1.0], np.float32)
    centre = o[:2].astype(np.float64) + (N - 1) / 2 * 0.25
    T = RW.quarter_yaw((centre[0], centre[1], 0.0))
    S, W, c = _row((N, N, Z), 4, 3)
    r = RW.warp_grid(S, W, c, vs, o, T)
    assert r['read'].sum() == N * N * Z
    i, j, k = np.meshgrid(np.arange(N), np.arange(N), np.arange(Z), indexing='ij')
    assert np.array_equal(r['S'].astype(np.float32), S[N - 1 - j, i, k]) and np.array_equal(r['W'].astype(np.float32), W[N - 1 - j, i, k])
    assert np.array_equal(r['cnt'], c[N - 1 - j, i, k])
    assert np.array_equal(np.sort(r['W'].ravel()), np.sort(W.astype(np.float64).ravel()))
    four = S
    for _ in range(4):                                                        # four quarter turns are the identity
        four = RW.warp_grid(four, W, c, vs, o, T)['S'].astype(np.float32)
    assert np.array_equal(four, S)


def test_reference_general_motion_properties():
    """A rotation plus a fractional translation: the weights of an interior voxel sum to 1, a constant mean survives, evidence only thins (W' <= max W),
    the mean is a convex combination of the neighbouring means, and forget_below forgets exactly the thin voxels."""
    dims, vs, o = (9, 8, 4), (0.16, 0.16, 0.2), np.array([-0.72, -0.64, -0.4], np.float32)
    T = RW.rigid(0.21, 0.02, -0.015, (0.07, -0.05, 0.03), (0, 0, 0))
    S, W, c = _row(dims, 4, 5)
    S = (2.5 * W[..., None] * np.ones(4)).astype(np.float32)                 # mean 2.5 everywhere
    r = RW.warp_grid(S, W, c, vs, o, T)
    seen = r['W'] > 0
    assert 0.3 < seen.mean() < 1.0 and r['read'].sum(-1).max() == 8 and (r['read'].sum(-1)[seen] < 8).any()
    assert np.allclose(r['S'][seen] / r['W'][seen][:, None], 2.5, rtol=1e-6) and (r['W'] <= W.max() * (1 + 1e-12)).all()
    assert not r['S'][~seen].any() and not r['cnt'][~seen].any() and (r['cnt'][seen] >= 1).all()
    w = np.sort(r['W'][seen])                                                # a robust threshold: midway in the widest gap of the sorted W'
    gap = int(np.argmax(np.diff(w)))
    fb = float((w[gap] + w[gap + 1]) / 2)
    rf = RW.warp_grid(S, W, c, vs, o, T, forget_below=fb)
    gone = seen & (r['W'] < fb)
    assert gone.any() and (seen & ~gone).any()
    assert not rf['W'][gone].any() and not rf['S'][gone].any() and not rf['cnt'][gone].any()
    assert np.array_equal(rf['W'][~gone], r['W'][~gone]) and np.array_equal(rf['cnt'][~gone], r['cnt'][~gone])
