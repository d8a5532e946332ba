"""Merging scenes without a device: ivx_volume_merge_fwd is declared, bound and exported and rejects bad arguments before any launch (the memory
rules among them: partial overlap, one pool with a shared row, one pool with disjoint rows getting past); ops.volume_merge_ raises its host errors;
the numpy reference of tests/ref_volume_merge.py against itself (the identity is the plain sum, a zero destination is ref_volume_warp.warp_grid,
an all-unseen source leaves the destination's bits); the host side of SceneSession.merge / SceneBatch.merge on empty, plain and windowed scenes."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import ref_volume_merge as RM
import ref_volume_warp as RW
from helpers import ROOT

NAME = 'ivx_volume_merge_fwd'
EYE = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]


def test_entry_point_declared_bound_and_exported():
    from imvoxelnet_amd import _lib, _build
    header = open(os.path.join(ROOT, 'include', 'imvoxel.h')).read()
    declared = set(re.findall(r'\b(ivx_[a-z0-9_]+)\s*\(', header))
    L = _lib.lib()
    assert NAME in declared, f'{NAME} is not declared in include/imvoxel.h'
    assert NAME in _lib.EXPORTS and hasattr(L, NAME) and getattr(L, NAME).argtypes is not None and len(getattr(L, NAME).argtypes) == 22
    assert L.ivx_version() >= 550
    for src in ('model.cpp', 'api_common.cpp'):        # also compiled into the CPU restatement of the ABI, which does not define it
        assert NAME not in open(os.path.join(ROOT, 'imvoxelnet_amd', 'csrc', src)).read(), src
    entry = [e for e in _build.SOURCES if e[0] == 'volume_warp.hip']    # the merge is a second instantiation of the resample kernel: no new source file
    assert len(entry) == 1 and '-ffp-contract=off' in entry[0][1] and not any('merge' in e[0] for e in _build.SOURCES)
    assert NAME in open(os.path.join(ROOT, 'imvoxelnet_amd', 'csrc', 'volume_warp.hip')).read()


def _call(L, rows_src=(2, 0), rows_dst=(0, 1), xform=None, origin_dst=None, origin_src=None, alpha=None, vs=(0.25, 0.25, 0.5), forget=0.0, B=None, R=(3, 2),
          dims=(7, 5, 6), C=8, src=(1 << 20, 2 << 20, 3 << 20), dst=(4 << 20, 5 << 20, 6 << 20), null=()):
    """The entry with dummy device pointers (never dereferenced: every call here is rejected before any launch)."""
    n = len(rows_src)
    B = n if B is None else B
    f32, i32 = ctypes.c_float, ctypes.c_int32
    xform = EYE * n if xform is None else xform
    origin_dst = [0.0] * (3 * n) if origin_dst is None else origin_dst
    origin_src = [0.0] * (3 * n) if origin_src is None else origin_src
    alpha = [1.0] * n if alpha is None else alpha
    arr = lambda v: (f32 * max(1, len(v)))(*v)                           # noqa: E731
    host = dict(row_src=(i32 * max(1, n))(*rows_src), row_dst=(i32 * max(1, n))(*rows_dst), xform=arr(xform), origin_dst=arr(origin_dst),
                origin_src=arr(origin_src), alpha=arr(alpha), voxel_size=(f32 * 3)(*vs))
    p = lambda name, a: None if name in null else ctypes.c_void_p(a)     # noqa: E731
    h = lambda name: None if name in null else host[name]                # noqa: E731
    return getattr(L, NAME)(B, h('row_src'), h('row_dst'), h('xform'), h('origin_dst'), h('origin_src'), h('alpha'), h('voxel_size'), forget, R[0], R[1],
                            *dims, C, p('sum_src', src[0]), p('wsum_src', src[1]), p('count_src', src[2]), p('sum_dst', dst[0]), p('wsum_dst', dst[1]),
                            p('count_dst', dst[2]), None)


def test_argument_validation_without_gpu():
    """Every pre-launch rejection: status -1 with its message, which names the export; nothing is launched."""
    from imvoxelnet_amd import _lib
    L = _lib.lib()
    nan, inf = float('nan'), float('inf')

    def rejected(word, **kw):
        rc, err = _call(L, **kw), L.ivx_last_error()
        assert rc == -1 and word in err and NAME.encode() in err, (kw, rc, err)

    for name in ('row_src', 'row_dst', 'xform', 'origin_dst', 'origin_src', 'alpha', 'voxel_size', 'sum_src', 'wsum_src', 'count_src', 'sum_dst', 'wsum_dst',
                 'count_dst'):
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
    for at in (1, 4, 8):
        rejected(b'16-byte aligned', src=((1 << 20) + at, 2 << 20, 3 << 20))
        rejected(b'16-byte aligned', dst=((4 << 20) + at, 5 << 20, 6 << 20))
    # the memory rules.  Partial overlap: the last / first 16 bytes, a row inside, and the same base with another row count
    row_bytes = 7 * 5 * 6 * 8 * 4
    for dst0 in ((1 << 20) + 3 * row_bytes - 16, (1 << 20) - 2 * row_bytes + 16, (1 << 20) + row_bytes, (1 << 20)):
        rejected(b'without being the same pool', dst=(dst0, 5 << 20, 6 << 20))
    same = dict(R=(3, 3), dst=(1 << 20, 2 << 20, 3 << 20))
    rejected(b'both as a source and as a destination', rows_src=(2, 0), rows_dst=(0, 1), **same)
    assert b'row 0' in L.ivx_last_error()
    rejected(b'both as a source and as a destination', rows_src=(1, 1), rows_dst=(0, 1), **same)
    # ... and the same pool with disjoint rows gets past that check: the next rule that fails is reported instead
    rejected(b'alpha', rows_src=(2, 2), rows_dst=(0, 1), alpha=[1.0, 0.0], **same)
    assert b'same pool' not in L.ivx_last_error() and b'both as' not in L.ivx_last_error()
    for bad in (0.0, -0.0, -1.0, -1e-30, nan, inf, -inf):
        for at in (0, 1):
            a = [1.0, 0.5]
            a[at] = bad
            rejected(b'alpha[%d]' % at, alpha=a)
            assert b'finite and > 0' in L.ivx_last_error()
    for bad in (nan, inf, -inf):
        for at in (0, 3, 11, 23):
            x = EYE * 2
            x[at] = bad
            rejected(b'finite', xform=x)
        rejected(b'finite', origin_dst=[0, 0, 0, 0, bad, 0])
        rejected(b'finite', origin_src=[bad, 0, 0, 0, 0, 0])
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


def test_ops_raise_their_host_errors_and_leave_the_buffers():
    """Host tensors throughout, so nothing can reach a launch: list, transform and shape errors come first, and arguments that pass them stop at the
    first host tensor.  The buffers keep every value."""
    from imvoxelnet_amd import ops
    vol, ws, cnt = _state(2)
    src = _state(3)
    keep = [t.clone() for t in (vol, ws, cnt) + src]
    T = RW.rigid(0.2, t=(0.1, 0, 0))

    def op(rows=(0, 1), src_rows=(2, 0), Ts=(T, np.eye(4)), o=((0, 0, 0), (1, 1, 1)), so=(0, 0, 0), vs=(0.25, 0.25, 0.5), v=vol, w=ws, c=cnt, src=src,
           alpha=1.0, forget=0.0):
        return ops.volume_merge_(v, w, c, list(rows), src, list(src_rows), list(Ts), o, so, vs, alpha=alpha, forget_below=forget)

    with pytest.raises(ValueError, match='rows must be distinct'):
        op(rows=(1, 1))
    with pytest.raises(ValueError, match=r'rows must be in \[0, 2\)'):
        op(rows=(0, 2))
    with pytest.raises(ValueError, match=r'src_rows must be in \[0, 3\)'):
        op(src_rows=(0, 3))
    with pytest.raises(ValueError, match='at least one row'):
        op(rows=(), src_rows=(), Ts=(), o=np.zeros((0, 3)))
    with pytest.raises(ValueError, match='src_rows has 1 entries'):
        op(src_rows=(0,))
    for bad in ((0.0, 1), (True, 1)):
        with pytest.raises(TypeError, match='integers'):
            op(rows=bad)
        with pytest.raises(TypeError, match='integers'):
            op(src_rows=bad)
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
        ops.volume_merge_(vol, ws, cnt, [0, 1], src, [2, 0], 3.0, np.zeros((2, 3)), (0, 0, 0), (0.25, 0.25, 0.5))
    for o in (np.zeros((3, 3)), np.zeros(2), [[0, 0, np.nan], [0, 0, 0]], [[0, 0, np.inf], [0, 0, 0]]):
        with pytest.raises(ValueError, match='new_origin'):
            op(o=o)
        with pytest.raises(ValueError, match='src_origin'):
            op(so=o)
    for vs in ((0.25, 0.25), (0.25, 0.0, 0.5), (0.25, -1, 0.5), (0.25, np.nan, 0.5)):
        with pytest.raises(ValueError, match='voxel_size'):
            op(vs=vs)
    for a in (0.0, -1.0, np.nan, np.inf, [1.0, 0.0], [1.0, -2.0], [1.0, np.nan], 1e-60, [1.0], [1.0, 1.0, 1.0], True):
        with pytest.raises(ValueError, match='alpha'):
            op(alpha=a)
    for a in ('one', [['a']], None):
        with pytest.raises((TypeError, ValueError), match='alpha'):
            op(alpha=a)
    for f in (-1.0, np.nan, np.inf, True, '1'):
        with pytest.raises(ValueError, match='forget_below'):
            op(forget=f)
    with pytest.raises(ValueError, match=r'\[R,X,Y,Z,C\]'):
        op(v=vol[0])
    with pytest.raises(ValueError, match='C % 4'):
        op(v=torch.zeros(2, 7, 5, 6, 6), src=(torch.zeros(3, 7, 5, 6, 6),) + src[1:])
    with pytest.raises(ValueError, match='wsum must be'):
        op(w=ws[:1])
    with pytest.raises(ValueError, match='count must be'):
        op(c=cnt[:, :3])
    with pytest.raises(ValueError, match=r'src\[0\] must be'):
        op(src=(torch.zeros(3, 7, 5, 6, 4),) + src[1:])
    with pytest.raises(ValueError, match=r'src\[2\] must be'):
        op(src=src[:2] + (cnt[:1],))
    with pytest.raises(TypeError, match='src must be a'):
        op(src=None)
    with pytest.raises(TypeError, match='src must be a'):
        op(src=src[:2])
    with pytest.raises(TypeError, match='vol_sum must be a torch.Tensor'):
        op(v=vol.numpy())
    with pytest.raises(RuntimeError, match='vol_sum must be a device'):      # everything host-checkable passed: the device check is last
        op()
    with pytest.raises(RuntimeError, match='device'):                        # one matrix alone for one row, one origin for all, B alphas
        ops.volume_merge_(vol, ws, cnt, [1], src, [0], T, (0, 0, 0), (0, 0, 0), (0.25, 0.25, 0.5), alpha=[0.5])
    for t, k in zip((vol, ws, cnt) + src, keep):
        assert torch.equal(t, k)


# ------------------------------------------------------------------ the reference against itself
def _row(dims, C, seed, unseen=0.15):
    rng = np.random.default_rng(seed)
    W = rng.uniform(0.5, 4.0, dims).astype(np.float32)
    S, c = (rng.standard_normal(dims + (C,)) * W[..., None]).astype(np.float32), rng.integers(1, 9, dims).astype(np.int32)
    gone = rng.random(dims) < unseen
    S[gone], W[gone], c[gone] = 0, 0, 0
    return S, W, c


DYADIC = (((7, 5, 6), (0.25, 0.125, 0.5), (-0.75, 0.375, -1.0)), ((6, 6, 3), (0.25, 0.25, 0.5), (-0.75, -0.75, 0.0)))


@pytest.mark.parametrize('alpha', [1.0, 0.5])
def test_reference_identity_is_the_plain_sum(alpha):
    """M = I, equal origins, a dyadic grid: one corner of weight 1 per voxel; where the source is seen the merge is S_d + alpha * S_s, exactly in
    float64 -- so its float32 rounding is the correctly rounded sum, torch's add -- the counts add, and the destination stays where the source is unseen."""
    for dims, vs, o in DYADIC:
        d, s = _row(dims, 4, 1), _row(dims, 4, 2)
        r = RM.merge_grid(d, s, vs, o, o, np.eye(4), alpha)
        seen = s[1] > 0
        assert np.array_equal(r['merged'], seen) and seen.any() and (~seen).any() and (r['read'].sum(-1) == 1).all() and r['inside'].all()
        assert np.array_equal(r['S'], d[0].astype(np.float64) + alpha * np.where(seen[..., None], s[0], 0).astype(np.float64))
        assert np.array_equal(r['W'], d[1].astype(np.float64) + alpha * s[1].astype(np.float64))
        assert np.array_equal(r['cnt'], d[2] + s[2])
        want = (torch.from_numpy(d[0]) + alpha * torch.from_numpy(s[0])).numpy()
        assert np.array_equal(r['S'].astype(np.float32)[seen], want[seen])
        assert RM.K_WARP == 11 and (r['bound_S'] >= RM.U * np.abs(r['S'])).all()


def test_reference_zero_destination_is_the_warp():
    """An all-zero destination, alpha = 1, equal origins: the merge reference equals ref_volume_warp.warp_grid, values, counts and corners read,
    with and without a threshold."""
    dims, vs, o = (9, 8, 4), (0.16, 0.16, 0.2), np.array([-0.72, -0.64, -0.4], np.float32)
    T = RW.rigid(0.21, 0.02, -0.015, (0.07, -0.05, 0.03))
    s = _row(dims, 4, 5)
    zero = (np.zeros(dims + (4,), np.float32), np.zeros(dims, np.float32), np.zeros(dims, np.int32))
    w0 = RW.warp_grid(*s, vs, o, T)
    w = np.sort(w0['W'][w0['W'] > 0])
    gap = int(np.argmax(np.diff(w)))
    for fb in (0.0, float((w[gap] + w[gap + 1]) / 2)):
        r, w_ = RM.merge_grid(zero, s, vs, o, o, T, 1.0, fb), RW.warp_grid(*s, vs, o, T, fb)
        assert np.array_equal(r['S'], w_['S']) and np.array_equal(r['W'], w_['W']) and np.array_equal(r['cnt'], w_['cnt']) and np.array_equal(r['read'], w_['read'])
        assert np.array_equal(r['merged'], w0['W'] > 0) and 0.3 < r['merged'].mean() < 1.0
    # ... and against a source grid of another origin the sample is the warp's at a transform that carries the difference of the origins
    so = o + np.float32(0.05)
    r = RM.merge_grid(zero, s, vs, o, so, T, 1.0)
    assert r['merged'].any() and not np.array_equal(r['W'], w0['W'])


def test_reference_an_unseen_source_leaves_the_destination():
    """A source with no evidence at all, or none where the destination looks: no voxel is merged, and values that are not even valid (NaN, -1)
    pass through untouched.  Forgetting never fires on an unmerged voxel."""
    dims, vs, o = (7, 5, 6), (0.16, 0.16, 0.2), np.array([-0.5, -0.4, -0.6], np.float32)
    T = RW.rigid(0.3, 0.02, 0.01, (0.06, 0.04, 0.02))
    d = _row(dims, 4, 7)
    d[0][1, 2, 3], d[1][1, 2, 3], d[2][1, 2, 3] = np.nan, np.nan, -1
    d[1][0, 0, 0] = 1e-3                                                      # below the threshold, and it stays: the voxel is not merged
    zero = (np.zeros(dims + (4,), np.float32), np.zeros(dims, np.float32), np.zeros(dims, np.int32))
    far = RW.rigid(t=(50.0, 0, 0))
    for src, M in ((zero, T), (_row(dims, 4, 8), far)):
        r = RM.merge_grid(d, src, vs, o, o, M, 0.7, forget_below=0.25)
        assert not r['merged'].any()
        assert np.array_equal(r['S'].astype(np.float32).view(np.int32), d[0].view(np.int32)) and np.array_equal(r['W'].astype(np.float32).view(np.int32), d[1].view(np.int32))
        assert np.array_equal(r['cnt'], d[2])
    with pytest.raises(AssertionError, match='robust'):                       # a positive W_s below MIN_WS is refused, not decided
        tiny = _row(dims, 4, 9, unseen=0.0)
        tiny[1][:] = 1e-9
        RM.merge_grid(d, tiny, vs, o, o, T, 1.0)


# ------------------------------------------------------------------ the sessions' host side
VS = (0.16, 0.16, 0.2)
K4 = np.array([[90., 0, 63.5, 0], [0, 90., 47.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
ORIGIN = np.array([0.37, -1.21, .5], np.float32)
META = dict(img_shape=(96, 128, 3), ori_shape=(96, 128, 3), lidar2img=dict(intrinsic=K4, origin=ORIGIN))


def _mock_model(**kw):
    return types.SimpleNamespace(**dict(dict(head_2d=None, voxel_size=VS, n_voxels=(40, 40, 16)), **kw))


def _record(r):
    """What a merge may change in a session's host record, as a comparable tuple."""
    return (r.n_views, r._stale, r._hw, len(r.meta['lidar2img']['extrinsic']), r.frame.tobytes(), r.scrolled, r._sum is None)


def test_session_merge_of_empty_scenes_launches_nothing_and_checks_everything(monkeypatch):
    """Two empty fading sessions of one model: the merge is host work only -- nothing is launched (ops.volume_merge_ is replaced by a counter), both
    records stay, self is returned.  Every refusal comes before that and leaves both scenes as they were."""
    from imvoxelnet_amd import SceneSession, ops
    calls = []
    monkeypatch.setattr(ops, 'volume_merge_', lambda *a, **k: calls.append(a))
    m = _mock_model()
    a, b = SceneSession(m, META, decay=0.9, forget_below=0.25), SceneSession(m, META, decay=1.0)
    before = _record(a), _record(b)
    T = RW.rigid(0.3, t=(0.5, 0.1, 0))
    assert a.merge(b) is a and a.merge(b, T) is a and a.merge(b, T.astype(np.float32), weight=0.5) is a and a.merge(b, torch.from_numpy(T), 2) is a
    assert (_record(a), _record(b)) == before and not calls
    with pytest.raises(ValueError, match='other is self'):
        a.merge(a)
    with pytest.raises(TypeError, match='SceneSession'):
        a.merge(None)
    with pytest.raises(TypeError, match='SceneSession'):
        a.merge(META)
    scale, mirror = T.copy(), T.copy()
    scale[:3, :3] *= 1.01
    mirror[:3, 2] *= -1
    for bad in (scale, mirror, T[:3], np.eye(3), np.full((4, 4), np.nan), 'T', 2.0):
        with pytest.raises((ValueError, TypeError)):
            a.merge(b, bad)
    for w in (0.0, -1.0, np.nan, np.inf, 1e-60):
        with pytest.raises(ValueError, match='weight'):
            a.merge(b, T, weight=w)
    for w in (True, '1', None, [1.0]):
        with pytest.raises(TypeError, match='weight'):
            a.merge(b, T, weight=w)
    with pytest.raises(ValueError, match='same prepared model'):
        a.merge(SceneSession(_mock_model(), META, decay=0.9))
    plain, windowed = SceneSession(m, META), SceneSession(m, META, window=3)
    for x, y in ((a, plain), (plain, a), (plain, plain.__class__(m, META))):
        with pytest.raises(NotImplementedError, match='decay=1.0'):
            x.merge(y, T)
    for x, y in ((a, windowed), (windowed, a), (windowed, plain), (plain, windowed)):
        with pytest.raises(NotImplementedError, match='window'):
            x.merge(y, T)
    c = SceneSession(m, META, decay=0.9)
    c.close()
    for x, y in ((a, c), (c, a)):
        with pytest.raises(RuntimeError, match='closed'):
            x.merge(y, T)
    assert (_record(a), _record(b)) == before and not calls and _record(plain)[0] == 0 and windowed.view_ids == []


def test_t_none_is_the_transform_between_the_frames():
    """T=None: the two scenes were opened in one common frame, so x_other = inv(other.frame) @ self.frame @ x_self, in float64, last row exact; the
    record rule on stub records: the other's extrinsics by warped_extrinsic behind this scene's own, n_views add, stale, frame / origin / scrolled stay."""
    from imvoxelnet_amd import SceneSession, warped_extrinsic
    from imvoxelnet_amd.scene import _merge_transform
    m = _mock_model()
    a, b = SceneSession(m, META, decay=0.9), SceneSession(m, META, decay=0.9)
    Ta, Tb = RW.rigid(0.3, t=(0.5, 0.1, 0)), RW.rigid(-0.2, 0.01, 0.02, (0, 0.3, 0.1))
    a.warp(Ta)
    b.warp(Tb)
    b.warp(Ta)
    T = _merge_transform(a, b, None)
    assert T.dtype == np.float64 and np.array_equal(T[3], [0, 0, 0, 1]) and np.allclose(T, np.linalg.inv(Tb @ Ta) @ Ta, atol=1e-12)
    x = np.array([0.3, -0.2, 0.1, 1.0])                                       # one point of the common frame, named in both grids
    assert np.allclose(b.frame @ (T @ x), a.frame @ x, atol=1e-12)
    assert np.array_equal(_merge_transform(a, b, Tb), Tb) and np.array_equal(_merge_transform(a, a.__class__(m, META, decay=1.0), None), np.linalg.inv(np.eye(4)) @ Ta)
    # the record rule
    E = [RW.rigid(0.1 * i, t=(i, 0, 1)).astype(np.float32) for i in range(5)]
    a.meta['lidar2img']['extrinsic'], a.n_views, a._hw = E[:2], 2, (96, 128)
    b.meta['lidar2img']['extrinsic'], b.n_views, b._hw = E[2:], 3, (96, 128)
    frame, origin = a.frame, a.meta['lidar2img']['origin'].copy()
    a._merged(b, T)
    got = a.meta['lidar2img']['extrinsic']
    assert a.n_views == 5 and a._stale and len(got) == 5 and all(np.array_equal(g, e) for g, e in zip(got[:2], E[:2]))
    assert all(g.dtype == np.float32 and np.array_equal(g, warped_extrinsic(e, T)) for g, e in zip(got[2:], E[2:]))
    assert np.array_equal(a.frame, frame) and np.array_equal(a.meta['lidar2img']['origin'], origin) and a.scrolled == (0, 0, 0)
    assert b.n_views == 3 and len(b.meta['lidar2img']['extrinsic']) == 3 and not b._stale


def test_batch_merge_host_side_and_a_raising_call_changes_nothing(monkeypatch):
    from imvoxelnet_amd import SceneBatch, ops
    calls = []
    monkeypatch.setattr(ops, 'volume_merge_', lambda *a, **k: calls.append(a))
    T1, T2 = RW.rigid(0.3, t=(0.5, 0.1, 0)), RW.rigid(-0.2, t=(0, 0.3, 0))
    b = SceneBatch(_mock_model(), [META] * 4, decay=0.9)
    assert b.merge(0, 2) is b and b.merge(0, 2, T1) is b and b.merge(0, 2, T1, 0.5) is b          # sources without views are skipped: nothing to launch
    assert b.merge([0, 1], [2, 2], [T1, T2], [1.0, 2.0]) is b and b.merge([0, 1], [3, 2]) is b
    bad = T1.copy()
    bad[:3, :3] *= 1.01
    for args in (([0, 4], [1, 2]), ([0, 0], [1, 2]), ([0, 1], [1, 2]), ([0, 1], [2]), ([], []), (-1, 2), (0, 0), ([0, 1], [2, 3], [T1]), ([0, 1], [2, 3], [T1, bad]),
                 ([0, 1], [2, 3], [T1, np.eye(3)]), ([0, 1], [2, 3], None, [1.0]), ([0, 1], [2, 3], None, [1.0, 0.0]), ([0, 1], [2, 3], None, [1.0, np.nan]),
                 (0, 2, T1, -1.0), (True, 2)):
        with pytest.raises(ValueError):
            b.merge(*args)
    with pytest.raises(TypeError, match='weight'):
        b.merge(0, 2, T1, '1')
    assert b.n_views == [0, 0, 0, 0] and not calls and all(np.array_equal(b.frame(s), np.eye(4)) for s in range(4))
    with pytest.raises(NotImplementedError, match='decay=1.0'):
        SceneBatch(_mock_model(), [META] * 2).merge(0, 1)
    with pytest.raises(NotImplementedError, match='window'):
        SceneBatch(_mock_model(), [META] * 2, window=2).merge(0, 1, T1)
    b.close()
    with pytest.raises(RuntimeError, match='closed'):
        b.merge(0, 2)


def test_a_batch_scene_that_got_its_views_by_merge_has_its_camera_record(monkeypatch):
    """A destination without views adopts a state, so it must also hold what its first add would have stored: the host camera record that warp, scroll
    and the refresh read.  Stub model, host pools and stubbed ops: merge into the empty scene 3, then warp it, scroll it and merge it onwards."""
    from imvoxelnet_amd import SceneBatch, ops
    m = _mock_model(n_voxels=(2, 2, 2), _new_origin=lambda o: torch.tensor(np.asarray(o, np.float32)) - torch.tensor([0.16, 0.16, 0.2]))
    b = SceneBatch(m, [META] * 4, decay=0.9)
    b._sum, b._wsum, b._count = torch.ones(4, 2, 2, 2, 4), torch.ones(4, 2, 2, 2), torch.ones(4, 2, 2, 2, dtype=torch.int32)
    r, E = b._scenes[2], RW.rigid(0.1, t=(1, 0, 1)).astype(np.float32)
    r.meta['lidar2img']['extrinsic'], r.n_views, r._hw, b._hw = [E], 1, (96, 128), (96, 128)
    b._cam[2] = (m._new_origin(ORIGIN), torch.tensor([24, 32], dtype=torch.int32))        # as the add of a 96 x 128 view stores it
    seen = []
    monkeypatch.setattr(ops, 'volume_merge_', lambda *a, **k: seen.append(('merge', a[3], a[5], np.asarray(a[7]), np.asarray(a[8]))))
    monkeypatch.setattr(ops, 'volume_warp', lambda *a, **k: seen.append(('warp', a[3], np.asarray(a[5]))))
    monkeypatch.setattr(ops, 'volume_scroll_', lambda *a, **k: seen.append(('scroll', a[2], a[3])))
    T = RW.rigid(0.3, t=(0.5, 0.1, 0))
    b.merge(3, 2, T)
    assert b.n_views == [0, 0, 1, 1] and not b._sum[3].any() and not b._wsum[3].any() and not b._count[3].any() and b._sum[2].all()
    assert b._cam[3] is not None and torch.equal(b._cam[3][0], b._cam[2][0]) and torch.equal(b._cam[3][1], b._cam[2][1]) and b._cam[3][1].dtype == torch.int32
    assert b._cam[0] is None and b._cam[1] is None
    b.warp(3, T)                                                              # read _cam[3] before the fix: TypeError
    b.scroll(3, (1, 0, 0))
    moved = m._new_origin(b.metas[3]['lidar2img']['origin'])
    assert torch.equal(b._cam[3][0], moved) and not torch.equal(moved, b._cam[2][0])
    b.merge(0, 3)                                                             # ... and onwards, from its scrolled grid
    kinds = [c[0] for c in seen]
    assert kinds == ['merge', 'warp', 'scroll', 'merge'] and seen[1][1] == [3] and np.array_equal(seen[1][2][0], b._cam[2][0].numpy())
    assert seen[3][1:3] == ([0], [3]) and np.array_equal(seen[3][4][0], moved.numpy()) and np.array_equal(seen[3][3][0], b._cam[2][0].numpy())
    assert b.n_views == [1, 0, 1, 1] and torch.equal(b._cam[0][0], b._cam[2][0])


def test_the_docs_speak_of_merging():
    import imvoxelnet_amd as ia
    doc = ia.scene.__doc__
    assert 'Merging scenes' in doc and 'ivx_volume_merge_fwd' in doc and 'volume_merge_' in doc
    out = doc[doc.index('Out of scope'):]
    for words in ('merging windowed scenes', 'merging plain scenes', 'a session and a batch row', 'several sources into one destination', 'de-duplicating',
                  'estimating T', 'saving a scene', 'different devices or ranks'):
        assert words in out, words
    assert 'counts twice' in ia.SceneSession.merge.__doc__ and 'counts twice' in ia.SceneBatch.merge.__doc__
    header = open(os.path.join(ROOT, 'include', 'imvoxel.h')).read()
    for words in ('Untouched.', 'Empty destination.', 'Identity.', 'Error.'):
        assert words in header[header.index('(0.5.5) Rigid merge'):header.index('int ivx_volume_merge_fwd')], words
    assert 'volume_merge' in open(os.path.join(ROOT, 'DESIGN.md')).read() and 'merging scenes' in open(os.path.join(ROOT, 'README.md')).read().lower()
    assert os.path.exists(os.path.join(ROOT, 'profiles', 'scene_merge.md')) and os.path.exists(os.path.join(ROOT, 'tools', 'scene_merge_bench.py'))
    assert 'merge' not in ia.__all__ if hasattr(ia, '__all__') else True      # nothing new is exported beyond the methods
