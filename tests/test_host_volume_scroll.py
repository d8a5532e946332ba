"""Scrolling scenes without a device: ivx_volume_scroll_fwd is declared, bound and exported and rejects bad arguments before any launch;
ops.volume_scroll_ raises its host errors; the origin rule, scroll_to's rounding and the host side of SceneSession.scroll / SceneBatch.scroll
(empty scenes launch nothing); the numpy reference of tests/ref_volume_scroll.py against np.roll and against itself."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import ref_volume_scroll as RS
from helpers import ROOT

NAME = 'ivx_volume_scroll_fwd'


def test_entry_point_declared_bound_and_exported():
    from imvoxelnet_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'imvoxel.h')).read()
    declared = set(re.findall(r'\b(ivx_[a-z0-9_]+)\s*\(', header))
    L = _lib.lib()
    assert NAME in declared, f'{NAME} is not declared in include/imvoxel.h'
    assert NAME in _lib.EXPORTS and hasattr(L, NAME) and getattr(L, NAME).argtypes is not None and len(getattr(L, NAME).argtypes) == 12
    assert L.ivx_version() >= 490
    for src in ('model.cpp', 'api_common.cpp'):        # also compiled into the CPU restatement of the ABI, which does not define it
        assert NAME not in open(os.path.join(ROOT, 'imvoxelnet_amd', 'csrc', src)).read(), src
    from imvoxelnet_amd import _build
    assert 'volume_scroll.hip' in [e[0] for e in _build.SOURCES]


def _call(L, rows=(2, 0), shifts=((1, 0, 0), (0, -2, 3)), B=None, R=3, dims=(7, 5, 6), C=8, vol=64, count=128, wsum=None, row_null=False, shift_null=False):
    B = len(rows) if B is None else B
    r = None if row_null else (ctypes.c_int32 * max(1, len(rows)))(*rows)
    flat = [v for s in shifts for v in s]
    s = None if shift_null else (ctypes.c_int32 * max(1, len(flat)))(*flat)
    p = lambda a: None if a is None else ctypes.c_void_p(a)     # noqa: E731
    return getattr(L, NAME)(B, r, s, R, *dims, C, p(vol), p(count), p(wsum), None)


def test_argument_validation_without_gpu():
    """Every pre-launch rejection: status -1 with its message, which names the export; nothing is launched (the dummy device pointers are never
    dereferenced: shifts that would move something are only ever passed together with an argument that is rejected)."""
    from imvoxelnet_amd import _lib
    L = _lib.lib()

    def err():
        return L.ivx_last_error()

    for kw in (dict(row_null=True), dict(shift_null=True), dict(vol=None), dict(count=None)):
        assert _call(L, **kw) == -1 and b'null argument' in err() and NAME.encode() in err(), kw
    for kw in (dict(B=0), dict(B=-1), dict(R=0), dict(R=-3), dict(dims=(0, 5, 6)), dict(dims=(7, -1, 6)), dict(dims=(7, 5, 0)), dict(C=0), dict(C=-4)):
        assert _call(L, **kw) == -1 and b'bad dims' in err() and NAME.encode() in err(), kw
    for c in (1, 2, 6, 10):
        assert _call(L, C=c) == -1 and b'C % 4' in err() and NAME.encode() in err(), c
    for dims in ((2048, 1024, 1024), (65536, 32768, 1), (1290, 1290, 1291)):
        assert _call(L, dims=dims) == -1 and b'below 2^31' in err() and NAME.encode() in err(), dims
    for rows in ((2, 3), (-1, 0), (0, 7)):
        assert _call(L, rows=rows) == -1 and b'outside [0, 3)' in err() and NAME.encode() in err(), rows
    assert _call(L, rows=(1, 1)) == -1 and b'distinct' in err() and b'row 1' in err() and NAME.encode() in err()
    assert _call(L, rows=(2, 0, 2), shifts=((1, 0, 0),) * 3) == -1 and b'distinct' in err()
    with pytest.raises(ValueError, match=NAME):
        _lib.check(_call(L, rows=(1, 1)), NAME)


def test_zero_shifts_are_valid_and_launch_nothing():
    """IVX_OK with dummy pointers and no device: no launch is attempted when nothing moves, with and without a weight sum, for 1 and for 70 samples
    (more than one launch's worth of rows)."""
    from imvoxelnet_amd import _lib
    L = _lib.lib()
    assert _call(L, shifts=((0, 0, 0), (0, 0, 0))) == 0
    assert _call(L, shifts=((0, 0, 0), (0, 0, 0)), wsum=256) == 0
    assert _call(L, rows=(1,), shifts=((0, 0, 0),)) == 0
    assert _call(L, rows=tuple(range(70)), shifts=((0, 0, 0),) * 70, R=70) == 0


def _state(R=3, dims=(7, 5, 6), C=8):
    return (torch.full((R,) + dims + (C,), 3.0), torch.full((R,) + dims, 9, dtype=torch.int32), torch.full((R,) + dims, 5.0))


def test_ops_raise_their_host_errors_and_leave_the_buffers():
    """Host tensors throughout, so nothing can reach a launch: list and shape errors come first, and arguments that pass them stop at the
    first host tensor.  The buffers keep every value."""
    from imvoxelnet_amd import ops
    vol, cnt, ws = _state()
    before = [t.clone() for t in (vol, cnt, ws)]

    def op(rows=(2, 0), shifts=((1, 0, 0), (0, -2, 3)), v=vol, c=cnt, w=ws):
        return ops.volume_scroll_(v, c, list(rows), [list(s) for s in shifts], w)

    with pytest.raises(ValueError, match='distinct'):
        op(rows=(1, 1))
    with pytest.raises(ValueError, match=r'rows must be in \[0, 3\)'):
        op(rows=(0, 3))
    with pytest.raises(ValueError, match='at least one row'):
        op(rows=(), shifts=())
    with pytest.raises(TypeError, match='integers'):
        op(rows=(0.0, 1))
    with pytest.raises(TypeError, match='integers'):
        op(rows=(True, 2))
    for bad in (1.0, 0.5, '1', None, True):
        with pytest.raises(TypeError, match='integers'):
            op(shifts=((1, 0, 0), (0, bad, 3)))
    with pytest.raises(TypeError, match='shifts'):
        ops.volume_scroll_(vol, cnt, [0, 1], torch.zeros(2, 3, dtype=torch.int32), ws)
    with pytest.raises(ValueError, match='one .* triple per row'):
        op(shifts=((1, 0, 0),))
    with pytest.raises(ValueError, match='one .* triple per row'):
        op(shifts=((1, 0), (0, 0, 0)))
    with pytest.raises(ValueError, match='int32'):
        op(shifts=((2 ** 31, 0, 0), (0, 0, 0)))
    with pytest.raises(ValueError, match=r'\[R,X,Y,Z,C\]'):
        op(v=vol[0])
    with pytest.raises(ValueError, match='C % 4'):
        op(v=torch.zeros(3, 7, 5, 6, 6))
    with pytest.raises(ValueError, match='count must be'):
        op(c=cnt[:2])
    with pytest.raises(ValueError, match='wsum must be'):
        op(w=ws[:, :3])
    with pytest.raises(TypeError, match='vol_sum must be a torch.Tensor'):
        op(v=vol.numpy())
    for w in (ws, None):                                   # everything host-checkable passed: the device check is last
        with pytest.raises(RuntimeError, match='vol_sum must be a device'):
            op(w=w)
    with pytest.raises(RuntimeError, match='device'):      # one triple alone for one row
        ops.volume_scroll_(vol, cnt, [1], (1, 0, -1), ws)
    for t, b in zip((vol, cnt, ws), before):
        assert torch.equal(t, b)


# ------------------------------------------------------------------ the origin rule and the sessions' host side
VS = (0.16, 0.16, 0.2)
K4 = np.array([[90., 0, 63.5, 0], [0, 90., 47.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
ORIGIN = np.array([0.37, -1.21, .5], np.float32)
META = dict(img_shape=(96, 128, 3), ori_shape=(96, 128, 3), lidar2img=dict(intrinsic=K4, origin=ORIGIN))


def _mock_model(**kw):
    return types.SimpleNamespace(**dict(dict(head_2d=None, voxel_size=VS, n_voxels=(40, 40, 16)), **kw))


def test_scrolled_origin_is_the_numpy_rule():
    from imvoxelnet_amd import scrolled_origin
    from imvoxelnet_amd.scene import scrolled_origin as same
    assert same is scrolled_origin
    rng = np.random.default_rng(5)
    for _ in range(200):
        o = rng.standard_normal(3) * 7
        s = rng.integers(-50, 50, 3)
        vs = rng.choice([0.04, 0.08, 0.16, 0.2, 0.32, 0.25], 3)
        got, ref = scrolled_origin(o, s, vs), RS.scrolled_origin(o, s, vs)
        assert got.dtype == np.float32 and got.shape == (3,) and np.array_equal(got.view(np.int32), ref.view(np.int32)), (o, s, vs)
    # a list origin, a tuple shift; the product is rounded before the sum (0.1f * 3 is not 0.3f)
    got = scrolled_origin([0.5, 0.5, 0.5], (3, -3, 0), (0.1, 0.1, 0.1))
    assert np.array_equal(got, RS.scrolled_origin([0.5, 0.5, 0.5], (3, -3, 0), (0.1, 0.1, 0.1)))
    assert got[0] == np.float32(0.5) + np.float32(np.float32(3) * np.float32(0.1)) and got[2] == np.float32(0.5)


def test_session_scroll_on_an_empty_scene_changes_only_the_origin():
    """No views, so no state and no launch: the meta's origin follows the rule, `scrolled` accumulates, reset() zeroes it and keeps the origin;
    bad shifts raise and change nothing; a closed session raises."""
    from imvoxelnet_amd import SceneSession
    for kw in (dict(), dict(decay=0.75), dict(window=3)):
        s = SceneSession(_mock_model(), META, **kw)
        assert s.scrolled == (0, 0, 0)
        assert s.scroll((3, -2, 1)) is s
        o1 = RS.scrolled_origin(ORIGIN, (3, -2, 1), VS)
        got = s.meta['lidar2img']['origin']
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and np.array_equal(got, o1)
        assert s.scrolled == (3, -2, 1) and not s._stale and s._origin is None and s.n_views == 0
        assert np.array_equal(META['lidar2img']['origin'], ORIGIN), 'the caller\'s meta stays as it was'
        s.scroll(np.array([-1, 0, 4]))
        assert s.scrolled == (2, -2, 5) and np.array_equal(s.meta['lidar2img']['origin'], RS.scrolled_origin(o1, (-1, 0, 4), VS))
        keep = s.meta['lidar2img']['origin'].copy()
        s.scroll((0, 0, 0))
        assert s.scrolled == (2, -2, 5) and np.array_equal(s.meta['lidar2img']['origin'], keep)
        for bad, exc in (((1.0, 0, 0), TypeError), ((1, 0), ValueError), ((1, 0, 0, 0), ValueError), ((True, 0, 0), TypeError), (3, TypeError),
                         ((2 ** 31, 0, 0), ValueError), (torch.tensor([1, 0, 0]), TypeError)):
            with pytest.raises(exc):
                s.scroll(bad)
        assert s.scrolled == (2, -2, 5) and np.array_equal(s.meta['lidar2img']['origin'], keep)
        s.reset()
        assert s.scrolled == (0, 0, 0) and np.array_equal(s.meta['lidar2img']['origin'], keep)
        s.close()
        with pytest.raises(RuntimeError, match='closed'):
            s.scroll((1, 0, 0))
        with pytest.raises(RuntimeError, match='closed'):
            s.scroll_to((0, 0, 0))


def test_scroll_to_rounds_as_stated():
    """rint((center - origin) / voxel_size) per axis in float64 (halves go to the even integer); applied when non-zero, returned always."""
    from imvoxelnet_amd import SceneSession
    o = np.array([1.0, -2.0, 0.5], np.float32)                           # exact in fp32 and fp64
    s = SceneSession(_mock_model(voxel_size=(0.25, 0.5, 0.125)), dict(META, lidar2img=dict(intrinsic=K4, origin=o)))
    assert s.scroll_to((1.0, -2.0, 0.5)) == (0, 0, 0) and s.scrolled == (0, 0, 0)
    assert s.scroll_to((1.1, -2.2, 0.55)) == (0, 0, 0) and s.scrolled == (0, 0, 0)              # 0.4, -0.4, 0.4 voxels
    # 2.5 -> 2 and -1.5 -> -2 (half to even), 3.49 -> 3
    c = (1.0 + 2.5 * 0.25, -2.0 - 1.5 * 0.5, 0.5 + 3.49 * 0.125)
    want = tuple(int(v) for v in np.rint((np.asarray(c, np.float64) - o.astype(np.float64)) / np.array([0.25, 0.5, 0.125])))
    assert want == (2, -2, 3)
    assert s.scroll_to(c) == want and s.scrolled == want
    assert np.array_equal(s.meta['lidar2img']['origin'], RS.scrolled_origin(o, want, (0.25, 0.5, 0.125)))
    assert s.scroll_to(c) == (0, 0, 0) and s.scrolled == want                                   # already there: what is left rounds to zero
    for bad in ((1, 2), (1, 2, float('nan')), (1, 2, float('inf'))):
        with pytest.raises(ValueError, match='center'):
            s.scroll_to(bad)
    assert s.scrolled == want


def test_batch_scroll_host_side_and_a_raising_call_changes_nothing():
    from imvoxelnet_amd import SceneBatch
    b = SceneBatch(_mock_model(), [META] * 3)
    assert b.scroll([2, 0], [(1, 0, -2), (0, 3, 0)]) is b
    assert [b.scrolled(i) for i in range(3)] == [(0, 3, 0), (0, 0, 0), (1, 0, -2)]
    assert np.array_equal(b.metas[2]['lidar2img']['origin'], RS.scrolled_origin(ORIGIN, (1, 0, -2), VS))
    assert np.array_equal(b.metas[0]['lidar2img']['origin'], RS.scrolled_origin(ORIGIN, (0, 3, 0), VS))
    assert np.array_equal(b.metas[1]['lidar2img']['origin'], ORIGIN) and b._cam == [None] * 3
    b.scroll(1, (0, 0, 5))                                                # one index with one triple
    assert b.scrolled(1) == (0, 0, 5)
    keep = [m['lidar2img']['origin'].copy() for m in b.metas]
    for scenes, voxels, exc in (([0, 3], [(1, 0, 0), (1, 0, 0)], ValueError), ([0, 1], [(1, 0, 0), (0, 1.5, 0)], TypeError), ([0, 0], [(1, 0, 0), (1, 0, 0)], ValueError),
                                ([0, 1], [(1, 0, 0)], ValueError), (-1, (1, 0, 0), ValueError), ([0, 1], [(1, 0, 0), (1, 0)], ValueError)):
        with pytest.raises(exc):
            b.scroll(scenes, voxels)
    assert [b.scrolled(i) for i in range(3)] == [(0, 3, 0), (0, 0, 5), (1, 0, -2)]
    assert all(np.array_equal(m['lidar2img']['origin'], k) for m, k in zip(b.metas, keep))
    b.reset([0])
    assert b.scrolled(0) == (0, 0, 0) and np.array_equal(b.metas[0]['lidar2img']['origin'], keep[0])
    b.close()
    with pytest.raises(RuntimeError, match='closed'):
        b.scroll(0, (1, 0, 0))


def test_anchor_head_models_refuse_to_scroll():
    """The anchors of an Anchor3DHead are fixed in the LiDAR frame: scroll says so, for sessions and batches, and changes nothing."""
    import imvoxelnet_amd as ia
    from kitti_cfg import kitti_model_cfg, KITTI_TEST_CFG
    model = ia.build_detector(kitti_model_cfg(n_voxels=(24, 28, 12), in_ch=16, out_ch=32), test_cfg=KITTI_TEST_CFG)
    s = model.open_scene(META)
    with pytest.raises(NotImplementedError, match='anchors'):
        s.scroll((1, 0, 0))
    with pytest.raises(NotImplementedError, match='anchors'):
        s.scroll_to((5.0, 0, 0))
    assert s.scroll_to(ORIGIN) == (0, 0, 0)                               # nothing to move: nothing refused
    b = model.open_scenes([META, META])
    with pytest.raises(NotImplementedError, match='anchors'):
        b.scroll([0, 1], [(0, 0, 0), (0, 1, 0)])
    assert s.scrolled == (0, 0, 0) and b.scrolled(1) == (0, 0, 0) and np.array_equal(s.meta['lidar2img']['origin'], ORIGIN)


def test_the_docs_speak_of_scrolling():
    import imvoxelnet_amd as ia
    doc = ia.scene.__doc__
    assert 'Scrolling scenes' in doc and 'scrolled_origin' in doc
    out = doc[doc.index('Out of scope'):]
    assert 'fraction of a voxel' in out and 'Anchor3DHead' in out
    assert 'volume_scroll' in open(os.path.join(ROOT, 'DESIGN.md')).read() and 'scrolling scenes' in open(os.path.join(ROOT, 'README.md')).read().lower()


# ------------------------------------------------------------------ the reference against np.roll and against itself
def _random_words(shape, seed):
    return np.random.default_rng(seed).integers(-2 ** 31, 2 ** 31, shape, dtype=np.int64).astype(np.int32)


SHIFTS = [(1, 0, 0), (-1, 0, 0), (0, 4, 0), (0, -4, 0), (0, 0, 5), (0, 0, -5), (2, -1, 3), (-6, 4, -5), (0, 0, 0), (7, 0, 0), (0, -5, 0), (0, 0, 9), (10, 0, 0)]


@pytest.mark.parametrize('shift', SHIFTS, ids=lambda s: '_'.join(map(str, s)))
def test_reference_agrees_with_roll_inside_and_is_zero_outside(shift):
    """np.roll(a, -s) wraps where the scroll zeroes: equal on the voxels whose source stayed inside, zero on the rest; float views keep their bits."""
    for C in (None, 4):
        shape = (7, 5, 6) + ((C,) if C else ())
        a = _random_words(shape, 11)
        got = RS.scroll_grid(a, shift)
        inside = RS.stayed_inside((7, 5, 6), shift)
        rolled = np.roll(a, tuple(-s for s in shift), axis=(0, 1, 2))
        assert np.array_equal(got[inside], rolled[inside]) and not got[~inside].any()
        assert int(inside.sum()) == max(0, 7 - abs(shift[0])) * max(0, 5 - abs(shift[1])) * max(0, 6 - abs(shift[2]))
        f = a.view(np.float32)
        assert np.isnan(f).any() and np.array_equal(RS.scroll_grid(f, shift).view(np.int32), got)
    # per index, from the definition
    a = _random_words((7, 5, 6), 12)
    got = RS.scroll_grid(a, shift)
    for i in range(7):
        for j in range(5):
            for k in range(6):
                q = (i + shift[0], j + shift[1], k + shift[2])
                want = a[q] if all(0 <= q[d] < (7, 5, 6)[d] for d in range(3)) else 0
                assert got[i, j, k] == want


def test_reference_there_and_back_zeroes_exactly_the_vacated_shell():
    """s then -s: the voxels that stayed inside under s keep their bits, the shell that s pushed out is zero and nothing else is; two scrolls compose
    by adding where nothing left the grid in between; rows not named keep their bits."""
    a = _random_words((7, 5, 6, 8), 13)
    assert (a != 0).all(axis=-1).all(), 'every voxel must hold something for "zero" to mean "vacated"'
    for s in SHIFTS:
        back = RS.scroll_grid(RS.scroll_grid(a, s), tuple(-v for v in s))
        kept = RS.stayed_inside((7, 5, 6), tuple(-v for v in s))          # the voxels that have a place in the scrolled grid
        assert np.array_equal(back[kept], a[kept]) and not back[~kept].any()
    one = RS.scroll_grid(RS.scroll_grid(a, (1, 0, 2)), (2, -1, 1))
    assert np.array_equal(one, RS.scroll_grid(a, (3, -1, 3)))
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):                       # the axis passes commute
        step = a
        for ax in order:
            step = RS.scroll_grid(step, tuple(v if d == ax else 0 for d, v in enumerate((2, -1, 3))))
        assert np.array_equal(step, RS.scroll_grid(a, (2, -1, 3)))
    pool = _random_words((3, 7, 5, 6), 14)
    out = RS.scroll_rows(pool, [2, 0], [(1, 0, 0), (0, -2, 3)])
    assert np.array_equal(out[1], pool[1]) and np.array_equal(out[2], RS.scroll_grid(pool[2], (1, 0, 0))) and np.array_equal(out[0], RS.scroll_grid(pool[0], (0, -2, 3)))
