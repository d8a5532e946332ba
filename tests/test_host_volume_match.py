"""Matching scenes without a device: ivx_volume_match_fwd and its scratch-size function are declared, bound and exported and reject bad arguments
before any launch; ops.volume_match raises its host errors; the numpy reference of tests/ref_volume_match.py against itself (the identity on a
dyadic grid has ncc == 1 and pairs == the intersection of the seen sets, a row against its own scroll peaks at that translation, an all-unseen
source pairs nothing); pose_candidates and MatchResult; the host refusals of SceneSession / SceneBatch match and register; and the coarse-to-fine
search of register converging on the CPU with the reference playing match."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import ref_volume_match as RX
import ref_volume_warp as RW
from helpers import ROOT

NAME, SCRATCH = 'ivx_volume_match_fwd', 'ivx_volume_match_scratch_bytes'
EYE = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]


def test_entry_point_declared_bound_and_exported():
    from imvoxelnet_amd import _lib, _build
    header = open(os.path.join(ROOT, 'include', 'imvoxel.h')).read()
    declared = set(re.findall(r'\b(ivx_[a-z0-9_]+)\s*\(', header))
    L = _lib.lib()
    for name, n_args in ((NAME, 24), (SCRATCH, 6)):
        assert name in declared, f'{name} is not declared in include/imvoxel.h'
        assert name in _lib.EXPORTS and hasattr(L, name) and getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == n_args, name
        decl = re.search(r'^(?:int|int64_t) ' + name + r'\(([^;]*)\);', header, re.M).group(1)
        assert re.sub(r'/\*.*?\*/', '', decl).count(',') + 1 == n_args, name
        for src in ('model.cpp', 'api_common.cpp'):    # also compiled into the CPU restatement of the ABI, which does not define it
            assert name not in open(os.path.join(ROOT, 'imvoxelnet_amd', 'csrc', src)).read(), (name, src)
    assert L.ivx_version() >= 570 and getattr(L, SCRATCH).restype is ctypes.c_int64
    entry = [e for e in _build.SOURCES if e[0] == 'volume_match.hip']
    assert len(entry) == 1 and '-ffp-contract=off' in entry[0][1]
    csrc = os.path.join(ROOT, 'imvoxelnet_amd', 'csrc')
    text = {f: open(os.path.join(csrc, f)).read() for f in ('volume_match.hip', 'volume_warp.hip', 'warp_geometry.h')}
    assert NAME in text['volume_match.hip']
    for fn in ('bool warp_axis(', 'float warp_weight('):                     # the trilinear rule stays written once, in the shared header
        assert fn in text['warp_geometry.h'] and fn not in text['volume_warp.hip'] and fn not in text['volume_match.hip'], fn
    assert all('#include "warp_geometry.h"' in text[f] for f in ('volume_match.hip', 'volume_warp.hip'))


def test_scratch_bytes():
    from imvoxelnet_amd import _lib
    fn = getattr(_lib.lib(), SCRATCH)
    for bad in ((0, 1, 7, 5, 6, 8), (1, 0, 7, 5, 6, 8), (1, 1, 0, 5, 6, 8), (1, 1, 7, -1, 6, 8), (1, 1, 7, 5, 0, 8), (1, 1, 7, 5, 6, 0), (1, 1, 7, 5, 6, 6),
                (-1, 1, 7, 5, 6, 8), (1, 1, 2048, 1024, 1024, 8)):
        assert fn(*bad) == -1, bad
    one, many = fn(1, 1, 7, 5, 6, 8), fn(2, 81, 7, 5, 6, 8)
    assert one > 0 and one % 256 == 0 and many > one and many % 256 == 0
    # one 32-byte partial per (sample, candidate, workgroup) and one 8-byte own count per (sample, workgroup); at most 1024 workgroups however large the grid
    assert fn(1, 81, 216, 248, 12, 64) <= 256 + 1024 * (81 * 32 + 8) and fn(3, 2, 216, 248, 12, 64) >= 3 * fn(1, 2, 216, 248, 12, 64) - 3 * 256


def _call(L, rows_src=(2, 0), rows_dst=(0, 1), K=2, xform=None, origin_dst=None, origin_src=None, vs=(0.25, 0.25, 0.5), step=(1, 1, 1), B=None, R=(3, 2),
          dims=(7, 5, 6), C=8, src=(1 << 20, 2 << 20), dst=(4 << 20, 5 << 20), outs=(6 << 20, 7 << 20, 8 << 20), scratch=9 << 20, null=(), Kcall=None):
    """The entry with dummy device pointers (never dereferenced: every call here is rejected before any launch)."""
    n = len(rows_src)
    B = n if B is None else B
    f32, i32 = ctypes.c_float, ctypes.c_int32
    xform = EYE * (n * K) if xform is None else xform
    origin_dst = [0.0] * (3 * n) if origin_dst is None else origin_dst
    origin_src = [0.0] * (3 * n) if origin_src is None else origin_src
    arr = lambda v: (f32 * max(1, len(v)))(*v)                           # noqa: E731
    host = dict(row_src=(i32 * max(1, n))(*rows_src), row_dst=(i32 * max(1, n))(*rows_dst), xform=arr(xform), origin_dst=arr(origin_dst),
                origin_src=arr(origin_src), voxel_size=(f32 * 3)(*vs), step=None if step is None else (i32 * 3)(*step))
    p = lambda name, a: None if name in null else ctypes.c_void_p(a)     # noqa: E731
    h = lambda name: None if name in null else host[name]                # noqa: E731
    return getattr(L, NAME)(B, K if Kcall is None else Kcall, h('row_src'), h('row_dst'), h('xform'), h('origin_dst'), h('origin_src'), h('voxel_size'),
                            h('step'), R[0], R[1], *dims, C, p('sum_src', src[0]), p('wsum_src', src[1]), p('sum_dst', dst[0]), p('wsum_dst', dst[1]),
                            p('pairs_out', outs[0]), p('own_out', outs[1]), p('stats_out', outs[2]), p('scratch', scratch), None)


def test_argument_validation_without_gpu():
    """Every pre-launch rejection: status -1 with its message, which names the export; nothing is launched."""
    from imvoxelnet_amd import _lib
    L = _lib.lib()
    nan, inf = float('nan'), float('inf')

    def rejected(word, **kw):
        rc, err = _call(L, **kw), L.ivx_last_error()
        assert rc == -1 and word in err and NAME.encode() in err, (kw, rc, err)

    for name in ('row_src', 'row_dst', 'xform', 'origin_dst', 'origin_src', 'voxel_size', 'sum_src', 'wsum_src', 'sum_dst', 'wsum_dst', 'pairs_out', 'own_out',
                 'stats_out'):
        rejected(b'null argument', null=(name,))
    rejected(b'null scratch', null=('scratch',))
    rejected(b'8-byte aligned', scratch=(9 << 20) + 4)
    for kw in (dict(B=0), dict(B=-1), dict(Kcall=0), dict(Kcall=-3), dict(R=(0, 2)), dict(R=(3, -1)), dict(dims=(0, 5, 6)), dict(dims=(7, -1, 6)),
               dict(dims=(7, 5, 0)), dict(C=0), dict(C=-4)):
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
    for at in (1, 4, 8):
        rejected(b'16-byte aligned', src=((1 << 20) + at, 2 << 20))
        rejected(b'16-byte aligned', dst=((4 << 20) + at, 5 << 20))
    for bad in (nan, inf, -inf):
        for at in (0, 3, 11, 23, 47):                                         # the last candidate of the last sample too
            x = EYE * 4
            x[at] = bad
            rejected(b'finite', xform=x)
        rejected(b'finite', origin_dst=[0, 0, 0, 0, bad, 0])
        rejected(b'finite', origin_src=[bad, 0, 0, 0, 0, 0])
        rejected(b'finite', vs=(0.25, bad, 0.5))
    for vs in ((0.0, 0.25, 0.5), (0.25, -0.25, 0.5), (0.25, 0.25, -1e-30)):
        rejected(b'voxel_size must be positive', vs=vs)
    for step in ((0, 1, 1), (1, -1, 1), (1, 1, 0), (-2 ** 31, 1, 1)):
        rejected(b'step must be >= 1', step=step)
    # read only: one pool on both sides, a row against itself and repeated destination rows get past every memory rule there is -- the next check reports
    rejected(b'step must be >= 1', rows_src=(1, 1), rows_dst=(1, 1), R=(3, 3), dst=(1 << 20, 2 << 20), step=(0, 1, 1))
    with pytest.raises(ValueError, match=NAME):
        _lib.check(_call(L, step=(0, 0, 0)), NAME)


def _state(R=3, dims=(7, 5, 6), C=8):
    return torch.full((R,) + dims + (C,), 3.0), torch.full((R,) + dims, 5.0)


def test_ops_raise_their_host_errors_and_leave_the_buffers():
    """Host tensors throughout, so nothing can reach a launch: list, transform, step and shape errors come first, and arguments that pass them stop
    at the first host tensor."""
    from imvoxelnet_amd import ops
    vol, ws = _state(2)
    src = _state(3)
    keep = [t.clone() for t in (vol, ws) + src]
    T = RW.rigid(0.2, t=(0.1, 0, 0))

    def op(rows=(0, 1), src_rows=(2, 0), Ts=((T, np.eye(4)), (np.eye(4), T)), o=((0, 0, 0), (1, 1, 1)), so=(0, 0, 0), vs=(0.25, 0.25, 0.5), v=vol, w=ws, src=src,
           step=(1, 1, 1)):
        return ops.volume_match(v, w, list(rows), src, list(src_rows), [list(c) for c in Ts], o, so, vs, step)

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
    with pytest.raises(ValueError, match='same number K'):                    # ragged K
        op(Ts=((T, T), (T,)))
    with pytest.raises(ValueError, match='same number K'):
        op(Ts=((), ()))
    with pytest.raises(TypeError, match='one per row'):
        op(Ts=((T, T),))
    with pytest.raises(TypeError, match='one per row'):
        ops.volume_match(vol, ws, [0, 1], src, [2, 0], 3.0, np.zeros((2, 3)), (0, 0, 0), (0.25, 0.25, 0.5))
    scale, mirror, nan = T.copy(), T.copy(), T.copy()
    scale[:3, :3] *= 1.01
    mirror[:3, 1] *= -1
    nan[1, 3] = np.nan
    for bad, word in ((scale, r'transforms\[1\]\[0\] is not rigid'), (mirror, 'reflection'), (nan, r'transforms\[1\]\[0\] must be finite'), (np.eye(3), '4x4 or 3x4')):
        with pytest.raises(ValueError, match=word):
            op(Ts=((T, T), (bad, T)))
    for step in (0, (1, 0, 1), (1, 1), (1, 1, 1, 1), -2, (1.5, 1, 1), True, 'x', None, 2 ** 31):
        with pytest.raises(ValueError, match='step'):
            op(step=step)
    for o in (np.zeros((3, 3)), np.zeros(2), [[0, 0, np.nan], [0, 0, 0]]):
        with pytest.raises(ValueError, match='new_origin'):
            op(o=o)
        with pytest.raises(ValueError, match='src_origin'):
            op(so=o)
    for vs in ((0.25, 0.25), (0.25, 0.0, 0.5), (0.25, np.nan, 0.5)):
        with pytest.raises(ValueError, match='voxel_size'):
            op(vs=vs)
    with pytest.raises(ValueError, match=r'\[R,X,Y,Z,C\]'):
        op(v=vol[0])
    with pytest.raises(ValueError, match='C % 4'):
        op(v=torch.zeros(2, 7, 5, 6, 6), src=(torch.zeros(3, 7, 5, 6, 6), src[1]))
    with pytest.raises(ValueError, match='wsum must be'):
        op(w=ws[:1])
    with pytest.raises(ValueError, match=r'src\[0\] must be'):
        op(src=(torch.zeros(3, 7, 5, 6, 4), src[1]))
    with pytest.raises(ValueError, match=r'src\[1\] must be'):
        op(src=(src[0], ws[:1]))
    with pytest.raises(TypeError, match='src must be a'):
        op(src=None)
    with pytest.raises(TypeError, match='vol_sum must be a torch.Tensor'):
        op(v=vol.numpy())
    with pytest.raises(RuntimeError, match='vol_sum must be a device'):      # everything host-checkable passed: the device check is last
        op()
    with pytest.raises(RuntimeError, match='device'):                        # one integer step, one origin for all, a (sum, wsum, count) triple
        ops.volume_match(vol, ws, [1], src + (torch.zeros(3, 7, 5, 6, dtype=torch.int32),), [0], [[T]], (0, 0, 0), (0, 0, 0), (0.25, 0.25, 0.5), step=2)
    for t, k in zip((vol, ws) + src, keep):
        assert torch.equal(t, k)


# ------------------------------------------------------------------ the reference against itself
def _row(dims, C, seed, unseen=0.15):
    rng = np.random.default_rng(seed)
    W = rng.uniform(0.5, 4.0, dims).astype(np.float32)
    S = (rng.standard_normal(dims + (C,)) * W[..., None]).astype(np.float32)
    gone = rng.random(dims) < unseen
    S[gone], W[gone] = 0, 0
    return S, W


DYADIC = (((7, 5, 6), (0.25, 0.125, 0.5), (-0.75, 0.375, -1.0)), ((6, 6, 3), (0.25, 0.25, 0.5), (-0.75, -0.75, 0.0)))


def test_reference_identity_on_a_dyadic_grid():
    """M = I, equal origins, a dyadic grid: one corner of weight 1 per voxel, so a row against itself has b == a, dot == na == nb and ncc == 1 up to
    fp64; against another row pairs is the intersection of the two seen sets and own the destination's."""
    for dims, vs, o in DYADIC:
        d, s = _row(dims, 4, 1), _row(dims, 4, 2)
        r = RX.match_grid(d, d, vs, o, o, np.eye(4))
        seen = d[1] > 0
        assert r['pairs'] == r['own'] == int(seen.sum()) and np.array_equal(r['paired'], seen) and (r['read'].sum(-1)[seen] == 1).all()
        assert r['stats'][0] == r['stats'][1] == r['stats'][2] > 0
        sc, ov = RX.score([r['pairs']], r['own'], r['stats'])
        assert abs(sc[0] - 1) <= 1e-15 and ov[0] == 1
        r = RX.match_grid(d, s, vs, o, o, np.eye(4))
        both = seen & (s[1] > 0)
        assert r['pairs'] == int(both.sum()) and np.array_equal(r['paired'], both) and r['own'] == int(seen.sum()) and 0 < r['pairs'] < r['own']
        assert abs(RX.score([r['pairs']], r['own'], r['stats'])[0][0]) < 0.5      # two unrelated rows do not correlate
        assert (r['bound'] > 0).all() and RX.K_DOT == 31 and RX.K_NA == 9 and RX.K_NB == 53
        # the lattice step: own and pairs count the visited voxels only
        r2 = RX.match_grid(d, s, vs, o, o, np.eye(4), step=(2, 1, 2))
        lat = RX.lattice(dims, (2, 1, 2)).reshape(dims)
        assert r2['own'] == int((seen & lat).sum()) and r2['pairs'] == int((both & lat).sum()) and 0 < r2['pairs'] < r['pairs']
        r3 = RX.match_grid(d, d, vs, o, o, np.eye(4), step=(99, 99, 99))
        assert r3['visited'].sum() == 1 and r3['visited'][0, 0, 0] and r3['own'] == int(seen[0, 0, 0])


def test_reference_a_scrolled_row_peaks_at_its_translation():
    """A row and its own scroll by s voxels (the scrolled grid's origin moves with it, so the identity relates the two frames): among whole-voxel
    translations the one that undoes the index shift, t = 0 with the moved origin, scores 1; and with EQUAL origins the peak sits at the
    translation by s voxels."""
    dims, vs, o = DYADIC[0]
    S, W = _row(dims, 8, 3, unseen=0.0)
    s = (1, -1, 2)
    S2, W2 = np.zeros_like(S), np.zeros_like(W)
    src = tuple(slice(max(0, a), d + min(0, a)) for a, d in zip(s, dims))
    dst = tuple(slice(max(0, -a), d + min(0, -a)) for a, d in zip(s, dims))
    S2[dst], W2[dst] = S[src], W[src]                                         # new[i] = old[i + s]: ops.volume_scroll_'s rule
    shifts = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (0, 2)]
    Ms = [RW.rigid(t=np.array(t) * np.array(vs)) for t in shifts]
    r = RX.match_rows((S2, W2), (S, W), vs, o, o, Ms)                         # equal origins: x_old = x_new + s * vs
    sc, ov = RX.score(r['pairs'], r['own'], r['stats'], 0.0)
    assert shifts[int(np.argmax(sc))] == s and abs(sc.max() - 1) <= 1e-12 and np.sort(sc)[-2] < 0.5
    moved = np.asarray(o, np.float32) + np.asarray(s, np.float32) * np.asarray(vs, np.float32)
    r = RX.match_rows((S2, W2), (S, W), vs, moved, o, [np.eye(4)] + Ms)       # the scrolled grid's own origin: the identity
    sc, _ = RX.score(r['pairs'], r['own'], r['stats'], 0.0)
    assert int(np.argmax(sc)) == 0 and abs(sc[0] - 1) <= 1e-12 and r['pairs'][0] == r['own']


def test_reference_an_unseen_source_pairs_nothing():
    dims, vs, o = (7, 5, 6), (0.16, 0.16, 0.2), np.array([-0.5, -0.4, -0.6], np.float32)
    T = RW.rigid(0.3, 0.02, 0.01, (0.06, 0.04, 0.02))
    d = _row(dims, 4, 7)
    zero = (np.zeros(dims + (4,), np.float32), np.zeros(dims, np.float32))
    for src, M in ((zero, T), (_row(dims, 4, 8), RW.rigid(t=(50.0, 0, 0)))):
        r = RX.match_grid(d, src, vs, o, o, M)
        assert r['pairs'] == 0 and r['own'] == int((d[1] > 0).sum()) and not r['stats'].any()
        sc, ov = RX.score([r['pairs']], r['own'], r['stats'])
        assert sc[0] == -np.inf and ov[0] == 0
    with pytest.raises(AssertionError, match='robust'):                       # a positive W_s below MIN_WS is refused, not decided
        tiny = _row(dims, 4, 9, unseen=0.0)
        tiny[1][:] = 1e-9
        RX.match_grid(d, tiny, vs, o, o, T)


# ------------------------------------------------------------------ candidates and results
def test_pose_candidates():
    import imvoxelnet_amd as ia
    T_c, about = RW.rigid(0.3, t=(0.5, 0.1, -0.2)), np.array([0.4, -1.2, 0.5])
    yaw, shift = np.radians(8), (0.32, 0.32, 0.2)
    c = ia.pose_candidates(T_c, yaw, shift, about)
    assert len(c) == 81 and all(x.shape == (4, 4) and x.dtype == np.float64 for x in c) and np.array_equal(c[40], T_c)
    from imvoxelnet_amd import ops
    for x in c:
        ops.check_rigid(x)
        assert np.array_equal(x[3], [0, 0, 0, 1])
    assert len({x.tobytes() for x in c}) == 81
    inv = np.linalg.inv(T_c)
    for i in range(81):                                                       # symmetric: i and 80 - i carry opposite offsets about the centre
        a, b = inv @ c[i], inv @ c[80 - i]
        assert np.isclose(np.arctan2(a[1, 0], a[0, 0]), -np.arctan2(b[1, 0], b[0, 0]), atol=1e-12)
        assert np.allclose((a @ np.append(about, 1))[:3] - about, -((b @ np.append(about, 1))[:3] - about), atol=1e-12)
    off = inv @ c[0]                                                          # the first: every offset at -h; the turn goes through `about`
    assert np.isclose(np.arctan2(off[1, 0], off[0, 0]), -yaw) and np.allclose((off @ np.append(about, 1))[:3] - about, -np.asarray(shift))
    last = inv @ c[41]                                                        # z is the fastest offset
    assert np.allclose(last[:3, :3], np.eye(3)) and np.allclose(last[:3, 3], (0, 0, shift[2]))
    assert np.allclose(ia.pose_candidates(T_c, yaw, shift, about)[7], c[7] @ np.eye(4)) and np.array_equal(ia.pose_candidates(T_c, 0.0, (0, 0, 0))[3], T_c)
    bad = T_c.copy()
    bad[:3, :3] *= 1.01
    for args in ((bad, yaw, shift), (T_c[:3], yaw, shift), (T_c, -0.1, shift), (T_c, np.nan, shift), (T_c, yaw, (0.1, 0.1)), (T_c, yaw, (0.1, -0.1, 0.1)),
                 (T_c, yaw, shift, (0, 0)), (T_c, yaw, shift, (0, np.inf, 0))):
        with pytest.raises(ValueError):
            ia.pose_candidates(*args)


def test_match_result_eligibility_follows_min_overlap():
    import imvoxelnet_amd as ia
    Ts = [RW.rigid(0.1 * k) for k in range(5)]
    pairs, own = [50, 29, 30, 0, 100], 100
    stats = [[0.9, 1, 1], [0.99, 1, 1], [0.5, 1, 1], [0, 0, 0], [2.0, 4.0, 4.0]]
    r = ia.MatchResult(pairs, own, stats, Ts, min_overlap=0.3)
    assert np.array_equal(r.overlap, [0.5, 0.29, 0.3, 0.0, 1.0]) and r.own == 100 and r.pairs.dtype == np.int64 and r.score.dtype == np.float64
    assert np.array_equal(r.score, [0.9, -np.inf, 0.5, -np.inf, 0.5]) and r.best == 0 and np.array_equal(r.T, Ts[0]) and r.T is not r.Ts[0]
    assert ia.MatchResult(pairs, own, stats, Ts, min_overlap=0.0).best == 1                          # the best ncc once it is eligible
    r = ia.MatchResult(pairs, own, stats, Ts, min_overlap=0.6)
    assert r.best == 4 and np.array_equal(np.isfinite(r.score), [False, False, False, False, True])
    r = ia.MatchResult(pairs[:4], own, stats[:4], Ts[:4], min_overlap=0.6)
    assert r.best is None and r.T is None and (r.score == -np.inf).all()
    r = ia.MatchResult([0, 0], 0, [[0, 0, 0]] * 2, Ts[:2], min_overlap=0.0)                          # nothing own: no division by zero
    assert r.best is None and not r.overlap.any()
    assert ia.MatchResult([5], 10, [[1.0, 0.0, 3.0]], Ts[:1], 0.0).best is None                      # a norm that is not positive
    for bad in (-0.1, 1.5, np.nan, True, '0.3', None):
        with pytest.raises(ValueError, match='min_overlap'):
            ia.MatchResult(pairs, own, stats, Ts, min_overlap=bad)
    with pytest.raises(ValueError, match='candidates'):
        ia.MatchResult(pairs, own, stats, Ts[:2])


# ------------------------------------------------------------------ the sessions' host side
VS = (0.16, 0.16, 0.2)
K4 = np.array([[90., 0, 63.5, 0], [0, 90., 47.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
ORIGIN = np.array([0.37, -1.21, .5], np.float32)
META = dict(img_shape=(96, 128, 3), ori_shape=(96, 128, 3), lidar2img=dict(intrinsic=K4, origin=ORIGIN))


def _mock_model(**kw):
    return types.SimpleNamespace(**dict(dict(head_2d=None, voxel_size=VS, n_voxels=(40, 40, 16)), **kw))


def test_session_refusals_of_match_and_register(monkeypatch):
    """Plain, windowed, closed and empty sessions, another model, something that is no session: every refusal comes before any launch
    (ops.volume_match is replaced by a counter) and follows merge's wording."""
    from imvoxelnet_amd import SceneSession, ops
    calls = []
    monkeypatch.setattr(ops, 'volume_match', lambda *a, **k: calls.append(a))
    m = _mock_model()
    a, b = SceneSession(m, META, decay=0.9), SceneSession(m, META, decay=1.0)
    plain, windowed = SceneSession(m, META), SceneSession(m, META, window=3)
    T = RW.rigid(0.3, t=(0.5, 0.1, 0))
    for op in ('match', 'register'):
        arg = [T] if op == 'match' else T
        for x, y in ((a, plain), (plain, a), (plain, SceneSession(m, META))):
            with pytest.raises(NotImplementedError, match='decay=1.0'):
                getattr(x, op)(y, arg)
        for x, y in ((a, windowed), (windowed, a), (windowed, plain), (plain, windowed)):
            with pytest.raises(NotImplementedError, match='window'):
                getattr(x, op)(y, arg)
        with pytest.raises(ValueError, match=f'{op}: this scene is empty'):
            getattr(a, op)(b, arg)
        with pytest.raises(ValueError, match='same prepared model'):
            getattr(a, op)(SceneSession(_mock_model(), META, decay=0.9), arg)
        for other in (None, META):
            with pytest.raises(TypeError, match='SceneSession'):
                getattr(a, op)(other)
        c = SceneSession(m, META, decay=0.9)
        c.close()
        for x, y in ((a, c), (c, a)):
            with pytest.raises(RuntimeError, match='closed'):
                getattr(x, op)(y, arg)
    a.n_views = 2                                                             # this scene holds views, the other does not
    with pytest.raises(ValueError, match='the other scene is empty'):
        a.match(b)
    assert not calls


def test_session_argument_checks_come_before_the_launch(monkeypatch):
    """Two stub sessions with host state: Ts, step, min_overlap, levels, yaw and shift are checked before ops.volume_match is reached; T=None is the
    merge's default candidate; what reaches ops is rows [0] of both states, K candidates and each scene's own corner origin."""
    from imvoxelnet_amd import SceneSession, ops
    from imvoxelnet_amd.scene import _merge_transform
    m = _mock_model(n_voxels=(2, 2, 2), _new_origin=lambda o: torch.tensor(np.asarray(o, np.float32)) - torch.tensor([0.16, 0.16, 0.2]))
    a, b = SceneSession(m, META, decay=0.9), SceneSession(m, dict(META, lidar2img=dict(intrinsic=K4, origin=ORIGIN + np.float32(0.16))), decay=0.9)
    for s in (a, b):
        s._sum, s._wsum, s.n_views = torch.ones(1, 2, 2, 2, 4), torch.ones(1, 2, 2, 2), 1
    seen = []

    def fake(vol, ws, rows, src, src_rows, Ts, o, so, vs, step):
        seen.append((rows, src_rows, [np.asarray(T) for T in Ts[0]], np.asarray(o), np.asarray(so), step))
        K = len(Ts[0])
        return torch.full((1, K), 4), torch.tensor([8]), torch.tensor([[[0.5 + 0.001 * k, 1.0, 1.0] for k in range(K)]], dtype=torch.float64)

    monkeypatch.setattr(ops, 'volume_match', fake)
    T = RW.rigid(0.3, t=(0.5, 0.1, 0))
    bad = T.copy()
    bad[:3, :3] *= 1.01
    for kw in (dict(Ts=[]), dict(Ts=T), dict(Ts=[bad]), dict(Ts=[T[:3]]), dict(Ts='T'), dict(step=0), dict(step=(1, 1)), dict(min_overlap=2), dict(min_overlap=None)):
        with pytest.raises((ValueError, TypeError)):
            a.match(b, **kw)
    for kw in (dict(T0=bad), dict(levels=0), dict(levels=1.5), dict(yaw=-1), dict(shift=(1, 1)), dict(step=[1, 2]), dict(min_overlap=-1)):
        with pytest.raises((ValueError, TypeError)):
            a.register(b, **kw)
    assert not seen
    r = a.match(b)
    assert len(seen) == 1 and seen[0][0] == [0] and seen[0][1] == [0] and len(seen[0][2]) == 1 and np.array_equal(seen[0][2][0], _merge_transform(a, b, None))
    assert np.array_equal(seen[0][3][0], m._new_origin(ORIGIN).numpy()) and np.array_equal(seen[0][4][0], m._new_origin(ORIGIN + np.float32(0.16)).numpy())
    assert seen[0][5] == [1, 1, 1] and r.best == 0 and r.own == 8 and r.overlap[0] == 0.5
    r = a.match(b, [T, np.eye(4)], step=2, min_overlap=0.5)
    assert seen[1][5] == [2, 2, 2] and len(seen[1][2]) == 2 and r.best == 1
    del seen[:]
    Tr, res = a.register(b, T0=T, levels=3, step=[2, 1, 1])
    assert [c[5] for c in seen] == [[2, 2, 2], [1, 1, 1], [1, 1, 1]] and all(len(c[2]) == 81 for c in seen) and res.best == 80
    assert np.array_equal(seen[0][2][40], T) and np.array_equal(seen[1][2][40], seen[0][2][80]) and np.array_equal(Tr, seen[2][2][80])
    from imvoxelnet_amd import pose_candidates                                # the offsets halve per level, about the grid's centre
    want = pose_candidates(seen[0][2][80], math.radians(8) / 2, np.array([0.32, 0.32, 0.2]) / 2, ORIGIN.astype(np.float64))
    assert all(np.array_equal(x, y) for x, y in zip(seen[1][2], want))


def test_batch_refusals_of_match_and_register(monkeypatch):
    from imvoxelnet_amd import SceneBatch, ops
    calls = []
    monkeypatch.setattr(ops, 'volume_match', lambda *a, **k: calls.append(a))
    T = RW.rigid(0.3, t=(0.5, 0.1, 0))
    b = SceneBatch(_mock_model(), [META] * 4, decay=0.9)
    for args in (([0, 4], [1, 2]), ([0, 1], [2]), ([], []), (-1, 2), (True, 2), ([0, 1], [2, 3], [[T]])):
        with pytest.raises(ValueError):
            b.match(*args)
    with pytest.raises(ValueError, match=r'scenes \[0, 2\] are empty'):
        b.match(0, 2, [T])
    with pytest.raises(ValueError, match='are empty'):
        b.register(0, 2, T)
    for op, arg in (('match', [T]), ('register', T)):
        with pytest.raises(NotImplementedError, match='decay=1.0'):
            getattr(SceneBatch(_mock_model(), [META] * 2), op)(0, 1, arg)
        with pytest.raises(NotImplementedError, match='window'):
            getattr(SceneBatch(_mock_model(), [META] * 2, window=2), op)(0, 1, arg)
    for r in b._scenes:
        r.n_views = 1
    with pytest.raises(ValueError, match='same number of candidates'):
        b.match([0, 1], [2, 3], [[T], [T, T]])
    b.close()
    for op, arg in (('match', [T]), ('register', T)):
        with pytest.raises(RuntimeError, match='closed'):
            getattr(b, op)(0, 2, arg)
    assert not calls


# ------------------------------------------------------------------ register on the CPU, the reference playing match
def test_reference_register_converges():
    """The search of register (scene._register, the function sessions and batches share) with ref_volume_match as its match: a smooth 12 x 12 x 6
    state of 8 channels, dst = the reference warp of src under T_true = rigid(yaw 0.21, t (0.23, -0.17, 0.06)) about the grid's centre; from the
    identity with yaw 8 degrees, shift (2 vs_x, 2 vs_y, vs_z), 6 levels and min_overlap 0.3 the search ends within the last level's step of
    T_true, in yaw and in each axis at the grid's centre.  (Only here the reference runs without its robustness assertion: at the identity the
    grid coordinates are whole numbers up to rounding and some corner weights are 1e-7; no device is compared with.)"""
    from imvoxelnet_amd import MatchResult
    from imvoxelnet_amd.scene import _register
    dims, C = (12, 12, 6), 8
    centre = np.array([0.03, -0.02, 0.01])
    o = (centre - np.asarray(dims) / 2 * np.asarray(VS)).astype(np.float32)
    src = RX.smooth_state(dims, C, 5, unseen=0.1, voxel_size=VS)
    T_true = RW.rigid(0.21, t=(0.23, -0.17, 0.06), about=centre)
    w = RW.warp_grid(*src, VS, o, T_true)
    dst = (w['S'].astype(np.float32), w['W'].astype(np.float32))

    def play(Ts, step, robust=False):
        refs = [RX.match_grid(dst, src, VS, o, o, T, step, robust=robust) for T in Ts]
        return MatchResult([r['pairs'] for r in refs], refs[0]['own'], [r['stats'] for r in refs], Ts, 0.3)

    at = play([T_true, np.eye(4)], (1, 1, 1))
    print(f'ncc at T_true {at.score[0]:.4f} (overlap {at.overlap[0]:.2f}), at the identity {at.score[1]:.4f}')
    assert at.score[0] > 0.999 and at.score[1] < at.score[0] and at.best == 0
    levels, yaw0, shift0 = 6, np.radians(8), np.array([2 * VS[0], 2 * VS[1], VS[2]])
    T, res = _register(play, np.eye(4), yaw0, None, levels, 1, 0.3, centre, VS)
    last = 2.0 ** -(levels - 1)
    D = np.linalg.inv(T_true) @ T
    yaw_err = abs(np.arctan2(D[1, 0], D[0, 0]))
    pos_err = np.abs((T @ np.append(centre, 1) - T_true @ np.append(centre, 1))[:3])
    print(f'register: yaw error {np.degrees(yaw_err):.3f} deg against a step of {np.degrees(yaw0 * last):.3f}; position error {pos_err.round(4).tolist()} m against '
          f'{(shift0 * last).round(4).tolist()}; final ncc {res.score[res.best]:.5f}')
    assert yaw_err <= yaw0 * last and (pos_err <= shift0 * last).all() and res.best is not None and res.score[res.best] > 0.999


def test_the_docs_speak_of_matching():
    import imvoxelnet_amd as ia
    doc = ia.scene.__doc__
    assert 'Matching scenes' in doc and NAME in doc and 'volume_match' in doc
    out = doc[doc.index('Out of scope'):]
    assert 'estimating T (registration)' not in out
    for words in ('a global search', 'pitch and roll', 'weighting pairs by evidence', 'Pearson', 'gradient-based', 'matching plain or windowed', 'de-duplicating'):
        assert words in out, words
    assert 'LOCAL search' in ia.SceneSession.register.__doc__ and 'local' in ia.SceneBatch.register.__doc__
    header = open(os.path.join(ROOT, 'include', 'imvoxel.h')).read()
    for words in ('Read only.', 'Deterministic.', 'Identity.', 'Error.', 'paired', 'four rounded'):
        assert words in header[header.index('(0.5.7) Scoring candidate poses'):header.index('int ivx_volume_match_fwd')], words
    assert 'volume_match' in open(os.path.join(ROOT, 'DESIGN.md')).read() and 'matching scenes' in open(os.path.join(ROOT, 'README.md')).read().lower()
    assert os.path.exists(os.path.join(ROOT, 'profiles', 'scene_match.md')) and os.path.exists(os.path.join(ROOT, 'tools', 'scene_match_bench.py'))
