"""Aligning scenes without a device: ivx_volume_align_fwd and its scratch-size function are declared, bound and exported and reject bad arguments
before any launch; ops.volume_align raises volume_match's host errors and its own for `about`; the numpy reference of tests/ref_volume_align.py
against itself (its g against central finite differences of its own e, the identity on a dyadic grid with e == 0 and g == 0 exactly); the
Levenberg-Marquardt loop of refine (scene._refine) converging on the CPU with the reference playing align; rigid_increment, solve_align and
AlignResult; the host refusals and argument checks of SceneSession / SceneBatch refine and register(refine=True); and the documents."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ref_volume_align as RA
import ref_volume_warp as RW
from helpers import ROOT
from test_host_volume_match import EYE, META, K4, ORIGIN, VS, _mock_model, _state, _row, DYADIC

NAME, SCRATCH = 'ivx_volume_align_fwd', 'ivx_volume_align_scratch_bytes'
DEG = np.pi / 180


def test_entry_point_declared_bound_and_exported():
    from imvoxelnet_amd import _lib, _build
    header = open(os.path.join(ROOT, 'include', 'imvoxel.h')).read()
    declared = set(re.findall(r'\b(ivx_[a-z0-9_]+)\s*\(', header))
    L = _lib.lib()
    for name, n_args in ((NAME, 26), (SCRATCH, 6)):
        assert name in declared, f'{name} is not declared in include/imvoxel.h'
        assert name in _lib.EXPORTS and hasattr(L, name) and getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == n_args, name
        decl = re.search(r'^(?:int|int64_t) ' + name + r'\(([^;]*)\);', header, re.M).group(1)
        assert re.sub(r'/\*.*?\*/', '', decl).count(',') + 1 == n_args, name
        for src in ('model.cpp', 'api_common.cpp'):    # also compiled into the CPU restatement of the ABI, which does not define it
            assert name not in open(os.path.join(ROOT, 'imvoxelnet_amd', 'csrc', src)).read(), (name, src)
    assert L.ivx_version() >= 580 and getattr(L, SCRATCH).restype is ctypes.c_int64
    assert header.index('int ivx_volume_align_fwd(') > header.index('int ivx_volume_match_fwd(')       # the new section comes after the match's
    csrc = os.path.join(ROOT, 'imvoxelnet_amd', 'csrc')
    text = {f: open(os.path.join(csrc, f)).read() for f in ('volume_match.hip', 'warp_geometry.h')}
    entry = [e for e in _build.SOURCES if e[0] == 'volume_match.hip']
    assert len(entry) == 1 and '-ffp-contract=off' in entry[0][1] and NAME in text['volume_match.hip']         # one file, one kernel template
    assert 'template <bool ALIGN>' in text['volume_match.hip'] and 'volume_match_kernel<ALIGN>' in text['volume_match.hip']
    assert 'float warp_corner_diff(' in text['warp_geometry.h'] and 'float warp_corner_diff(' not in text['volume_match.hip']


def test_scratch_bytes():
    from imvoxelnet_amd import _lib
    L = _lib.lib()
    fn = getattr(L, SCRATCH)
    for bad in ((0, 1, 7, 5, 6, 8), (1, 0, 7, 5, 6, 8), (1, 1, 0, 5, 6, 8), (1, 1, 7, -1, 6, 8), (1, 1, 7, 5, 0, 8), (1, 1, 7, 5, 6, 0), (1, 1, 7, 5, 6, 6),
                (-1, 1, 7, 5, 6, 8), (1, 1, 2048, 1024, 1024, 8)):
        assert fn(*bad) == -1, bad
    one, many = fn(1, 1, 7, 5, 6, 8), fn(2, 33, 7, 5, 6, 8)
    assert one > 0 and one % 256 == 0 and many > one and many % 256 == 0
    # one partial of 33 words of 8 bytes per (sample, candidate, workgroup) and one own count per (sample, workgroup); at most 1024 workgroups
    assert fn(1, 4, 216, 248, 12, 64) <= 256 + 1024 * (4 * 264 + 8) and fn(1, 1, 216, 248, 12, 64) > L.ivx_volume_match_scratch_bytes(1, 1, 216, 248, 12, 64)


def _call(L, rows_src=(2, 0), rows_dst=(0, 1), K=2, xform=None, about=None, origin_dst=None, origin_src=None, vs=(0.25, 0.25, 0.5), step=(1, 1, 1), B=None,
          R=(3, 2), dims=(7, 5, 6), C=8, src=(1 << 20, 2 << 20), dst=(4 << 20, 5 << 20), outs=(6 << 20, 7 << 20, 8 << 20, 10 << 20), scratch=9 << 20,
          null=(), Kcall=None):
    """The entry with dummy device pointers (never dereferenced: every call here is rejected before any launch)."""
    n = len(rows_src)
    B = n if B is None else B
    f32, i32 = ctypes.c_float, ctypes.c_int32
    xform = EYE * (n * K) if xform is None else xform
    zeros = [0.0] * (3 * n)
    about, origin_dst, origin_src = (zeros if v is None else v for v in (about, origin_dst, origin_src))
    arr = lambda v: (f32 * max(1, len(v)))(*v)                           # noqa: E731
    host = dict(row_src=(i32 * max(1, n))(*rows_src), row_dst=(i32 * max(1, n))(*rows_dst), xform=arr(xform), about=arr(about), origin_dst=arr(origin_dst),
                origin_src=arr(origin_src), voxel_size=(f32 * 3)(*vs), step=None if step is None else (i32 * 3)(*step))
    p = lambda name, a: None if name in null else ctypes.c_void_p(a)     # noqa: E731
    h = lambda name: None if name in null else host[name]                # noqa: E731
    return getattr(L, NAME)(B, K if Kcall is None else Kcall, h('row_src'), h('row_dst'), h('xform'), h('about'), h('origin_dst'), h('origin_src'),
                            h('voxel_size'), h('step'), R[0], R[1], *dims, C, p('sum_src', src[0]), p('wsum_src', src[1]), p('sum_dst', dst[0]),
                            p('wsum_dst', dst[1]), p('pairs_out', outs[0]), p('used_out', outs[1]), p('own_out', outs[2]), p('stats_out', outs[3]),
                            p('scratch', scratch), None)


def test_argument_validation_without_gpu():
    """Every pre-launch rejection -- the match's, and those of `about` and used_out: status -1 with its message, which names the export."""
    from imvoxelnet_amd import _lib
    L = _lib.lib()
    nan, inf = float('nan'), float('inf')

    def rejected(word, **kw):
        rc, err = _call(L, **kw), L.ivx_last_error()
        assert rc == -1 and word in err and NAME.encode() in err, (kw, rc, err)

    for name in ('row_src', 'row_dst', 'xform', 'about', 'origin_dst', 'origin_src', 'voxel_size', 'sum_src', 'wsum_src', 'sum_dst', 'wsum_dst', 'pairs_out',
                 'used_out', 'own_out', 'stats_out'):
        rejected(b'null argument', null=(name,))
    rejected(b'null scratch', null=('scratch',))
    rejected(b'ivx_volume_align_scratch_bytes', null=('scratch',))
    rejected(b'8-byte aligned', scratch=(9 << 20) + 4)
    for kw in (dict(B=0), dict(B=-1), dict(Kcall=0), dict(Kcall=-3), dict(R=(0, 2)), dict(R=(3, -1)), dict(dims=(0, 5, 6)), dict(dims=(7, -1, 6)),
               dict(dims=(7, 5, 0)), dict(C=0), dict(C=-4)):
        rejected(b'bad dims', **kw)
    for c in (1, 2, 6, 10):
        rejected(b'C % 4', C=c)
    for dims in ((2048, 1024, 1024), (65536, 32768, 1), (1290, 1290, 1291)):
        rejected(b'below 2^31', dims=dims)
    for rows in ((2, 3), (-1, 0)):
        rejected(b'outside [0, 3)', rows_src=rows)
    for rows in ((0, 2), (-1, 0)):
        rejected(b'outside [0, 2)', rows_dst=rows)
    for at in (1, 4, 8):
        rejected(b'16-byte aligned', src=((1 << 20) + at, 2 << 20))
        rejected(b'16-byte aligned', dst=((4 << 20) + at, 5 << 20))
    for bad in (nan, inf, -inf):
        for at in (0, 3, 11, 23, 47):
            x = EYE * 4
            x[at] = bad
            rejected(b'finite', xform=x)
        rejected(b'finite', origin_dst=[0, 0, 0, 0, bad, 0])
        rejected(b'finite', origin_src=[bad, 0, 0, 0, 0, 0])
        rejected(b'finite', vs=(0.25, bad, 0.5))
        for at in (0, 5):
            a = [0.0] * 6
            a[at] = bad
            rejected(b'about must be finite', about=a)
    for vs in ((0.0, 0.25, 0.5), (0.25, -0.25, 0.5), (0.25, 0.25, -1e-30)):
        rejected(b'voxel_size must be positive', vs=vs)
    for step in ((0, 1, 1), (1, -1, 1), (1, 1, 0), (-2 ** 31, 1, 1)):
        rejected(b'step must be >= 1', step=step)
    rejected(b'step must be >= 1', rows_src=(1, 1), rows_dst=(1, 1), R=(3, 3), dst=(1 << 20, 2 << 20), step=(0, 1, 1))      # read only: no memory rule
    with pytest.raises(ValueError, match=NAME):
        _lib.check(_call(L, step=(0, 0, 0)), NAME)


def test_ops_raise_their_host_errors_and_leave_the_buffers():
    """Host tensors throughout, so nothing can reach a launch: volume_match's errors through the shared path, `about` by the origins' rule, and
    arguments that pass them stop at the first host tensor."""
    from imvoxelnet_amd import ops
    vol, ws = _state(2)
    src = _state(3)
    keep = [t.clone() for t in (vol, ws) + src]
    T = RW.rigid(0.2, t=(0.1, 0, 0))

    def op(rows=(0, 1), src_rows=(2, 0), Ts=((T, np.eye(4)), (np.eye(4), T)), about=(0.1, 0.2, 0.3), o=((0, 0, 0), (1, 1, 1)), so=(0, 0, 0), vs=(0.25, 0.25, 0.5),
           v=vol, w=ws, src=src, step=(1, 1, 1)):
        return ops.volume_align(v, w, list(rows), src, list(src_rows), [list(c) for c in Ts], about, o, so, vs, step)

    with pytest.raises(ValueError, match=r'rows must be in \[0, 2\)'):
        op(rows=(0, 2))
    with pytest.raises(ValueError, match=r'src_rows must be in \[0, 3\)'):
        op(src_rows=(0, 3))
    with pytest.raises(ValueError, match='at least one row'):
        op(rows=(), src_rows=(), Ts=(), o=np.zeros((0, 3)))
    with pytest.raises(ValueError, match='same number K'):
        op(Ts=((T, T), (T,)))
    with pytest.raises(TypeError, match='one per row'):
        op(Ts=((T, T),))
    scale = T.copy()
    scale[:3, :3] *= 1.01
    with pytest.raises(ValueError, match=r'transforms\[1\]\[0\] is not rigid'):
        op(Ts=((T, T), (scale, T)))
    for step in (0, (1, 0, 1), (1, 1), True, None):
        with pytest.raises(ValueError, match='step'):
            op(step=step)
    for bad in (np.zeros((3, 3)), np.zeros(2), [[0, 0, np.nan], [0, 0, 0]], (0, np.inf, 0)):
        with pytest.raises(ValueError, match='about'):
            op(about=bad)
    with pytest.raises(ValueError, match='new_origin'):
        op(o=np.zeros(2))
    with pytest.raises(TypeError, match='about'):
        op(about=None)
    with pytest.raises(TypeError, match='about'):
        op(about='centre')
    for vs in ((0.25, 0.25), (0.25, 0.0, 0.5)):
        with pytest.raises(ValueError, match='voxel_size'):
            op(vs=vs)
    with pytest.raises(ValueError, match='C % 4'):
        op(v=torch.zeros(2, 7, 5, 6, 6), src=(torch.zeros(3, 7, 5, 6, 6), src[1]))
    with pytest.raises(ValueError, match=r'src\[1\] must be'):
        op(src=(src[0], ws[:1]))
    with pytest.raises(RuntimeError, match='vol_sum must be a device'):      # everything host-checkable passed: the device check is last
        op()
    with pytest.raises(RuntimeError, match='device'):                        # about [B,3], one integer step
        op(about=np.zeros((2, 3)), step=2)
    for t, k in zip((vol, ws) + src, keep):
        assert torch.equal(t, k)


# ------------------------------------------------------------------ the reference against itself
def test_reference_gradient_against_finite_differences():
    """g of the reference against central finite differences of its own e along T @ rigid_increment(+-h e_i, about): float64 geometry, h = 1e-6, two
    unrelated smooth rows at (9, 8, 5), C = 8, the pose rigid(0.05, 0.03, -0.02, t=(0.05, 0.03, 0.02)); `used` is equal at both offsets, so no
    voxel changed its set and e is smooth between them.  d e / d xi = 2 g.  Required: relative agreement within 1e-6 on all six components
    (measured: 3e-9).  With fp32 geometry or h = 1e-4 points change cells and the check is void."""
    from imvoxelnet_amd import rigid_increment
    dims, C, h = (9, 8, 5), 8, 1e-6
    A, B = RA.smooth_state(dims, C, 1, voxel_size=VS), RA.smooth_state(dims, C, 2, voxel_size=VS)
    about, o = np.asarray(dims) * np.asarray(VS) / 2, (0.0, 0.0, 0.0)
    T = RW.rigid(0.05, 0.03, -0.02, t=(0.05, 0.03, 0.02))
    at = lambda M: RA.align_grid(A, B, VS, o, o, M, about, geometry='float64', robust=False)       # noqa: E731
    r0 = at(T)
    assert r0['used'] > 100 and r0['e'] > 0
    worst = 0.0
    for i in range(6):
        xi = np.zeros(6)
        xi[i] = h
        plus, minus = at(T @ rigid_increment(xi, about)), at(T @ rigid_increment(-xi, about))
        assert plus['used'] == minus['used'] == r0['used'] and plus['pairs'] == minus['pairs'] == r0['pairs']
        fd = (plus['e'] - minus['e']) / (2 * h) / 2
        worst = max(worst, abs(fd - r0['g'][i]) / abs(fd))
    print(f'g against central differences of e: worst relative difference {worst:.2e}')
    assert worst <= 1e-6
    # H is the Gauss-Newton matrix of the same J: symmetric, positive semi-definite, and fp32 geometry moves the sums only a little
    assert np.array_equal(r0['H'], r0['H'].T) and np.linalg.eigvalsh(r0['H']).min() > -1e-9 * np.abs(r0['H']).max()
    r32 = RA.align_grid(A, B, VS, o, o, T, about)
    assert r32['used'] == r0['used'] and np.allclose(r32['stats'], r0['stats'], rtol=1e-3, atol=1e-3 * np.abs(r0['stats']).max())


def test_reference_identity_on_a_dyadic_grid():
    """M = I, equal origins, a dyadic grid, a row against itself: b == a bit for bit so e == 0 and g == 0 exactly; used is the seen voxels whose
    eight forward corners are all in the grid and seen; H is not zero.  The reference refuses inputs whose decisions are not robust."""
    for dims, vs, o in DYADIC:
        d = _row(dims, 4, 1)
        about = np.asarray(o) + np.asarray(dims) * np.asarray(vs) / 2
        r = RA.align_grid(d, d, vs, o, o, np.eye(4), about)
        seen = d[1] > 0
        full = np.zeros(dims, bool)
        full[:-1, :-1, :-1] = True
        for c in range(8):
            full[:-1, :-1, :-1] &= seen[(c >> 2):dims[0] - 1 + (c >> 2), ((c >> 1) & 1):dims[1] - 1 + ((c >> 1) & 1), (c & 1):dims[2] - 1 + (c & 1)]
        assert r['pairs'] == r['own'] == int(seen.sum()) and r['used'] == int(full.sum()) > 0 and np.array_equal(r['used_mask'], full)
        assert r['e'] == 0 and not r['g'].any() and r['H'][0, 0] > 0 and (r['bound'] > 0).all()
        assert r['stats'].shape == (31,) and r['stats'][3] == 0 and np.array_equal(RA.full_H(r['stats'][10:]), r['H'])
    assert RA.K_E == 55 and RA.K_G.tolist() == [81, 81, 81, 83, 83, 83] and sorted(set(RA.K_H.tolist())) == [107, 109, 111] and len(RA.K_ALIGN) == 31
    dims, vs, o = DYADIC[0]
    tiny = _row(dims, 4, 9, unseen=0.0)
    tiny[1][2, 2, 2] = 1e-9
    with pytest.raises(AssertionError, match='robust'):                       # a positive corner weight sum below MIN_WS is refused, not decided
        RA.align_grid(_row(dims, 4, 7), tiny, vs, o, o, np.eye(4), (0, 0, 0))
    with pytest.raises(AssertionError, match='cell face'):                    # a point an fp32 rounding below a cell face is refused, not decided
        M = np.eye(4)
        M[0, 3] = -2.0 ** -26
        RA.align_grid(_row(dims, 4, 7), _row(dims, 4, 8, unseen=0.0), vs, o, o, M, (0, 0, 0))


# ------------------------------------------------------------------ refine on the CPU, the reference playing align
POSES = (dict(yaw=12 * DEG, t=(1.4 * VS[0], 0, 0)), dict(yaw=3 * DEG, pitch=2 * DEG, roll=-2.5 * DEG), dict(yaw=6 * DEG, pitch=4 * DEG, roll=-3 * DEG, t=(VS[0], 0, 0)))


def _play(dst, src, o, about, calls=None):
    def align(idx, Ts):
        if calls is not None:
            calls.append(list(idx))
        out = []
        for T in Ts:
            r = RA.align_grid(dst, src, VS, o, o, T, about, robust=False)
            out.append((r['pairs'], r['used'], r['own'], r['stats']))
        return out
    return align


def _pose_error(T, T_true, centre):
    D = np.linalg.inv(T_true) @ T
    ang = np.degrees(np.arccos(np.clip((np.trace(D[:3, :3]) - 1) / 2, -1, 1)))
    return ang, np.abs((T @ np.append(centre, 1) - T_true @ np.append(centre, 1))[:3])


@pytest.mark.parametrize('dims', [(12, 12, 6), (16, 14, 8)], ids=str)
def test_reference_refine_converges(dims):
    """The loop of refine (scene._refine, the function sessions and batches share) with ref_volume_align as its align (without its robustness
    assertion, as in the register test: no device is compared with): a smooth state of 8 channels and its reference warp under three poses --
    yaw 12 deg with a shift of 1.4 voxels; yaw 3, pitch 2, roll -2.5 deg; yaw 6, pitch 4, roll -3 deg with a shift of one voxel -- about the
    grid's centre.  From the identity every run ends within 12 evaluations, below 1e-3 of a voxel edge and 0.01 deg of the truth, with every
    accepted cost strictly lower than the last.  (Measured: 5 - 6 evaluations, used / own 0.63 - 0.72.)"""
    from imvoxelnet_amd.scene import _refine, _check_refine, ALIGN_DOF
    C, o = 8, (0.0, 0.0, 0.0)
    centre = np.asarray(dims) * np.asarray(VS) / 2
    src = RA.smooth_state(dims, C, 3, voxel_size=VS)
    args = _check_refine(12, ALIGN_DOF, 0.3, 1e-3, None, 1e-5, VS)
    assert args[4] == 1e-3 * 0.16
    for pose in POSES:
        T_true = RW.rigid(about=centre, **pose)
        w = RW.warp_grid(*src, VS, o, T_true)
        dst = (w['S'].astype(np.float32), w['W'].astype(np.float32))
        calls = []
        T, res = _refine(_play(dst, src[:2], o, centre, calls), [np.eye(4)], [centre], C, *args)[0]
        ang, pos = _pose_error(T, T_true, centre)
        print(f'{dims} {pose}: {res}; error {ang:.2e} deg, {pos.max():.2e} m; costs {[f"{c:.3g}" for c in res.history]}')
        assert res.ok and res.converged and res.evaluations == len(calls) <= 12 and res.accepted == len(res.history) - 1 >= 3
        assert ang < 0.01 and (pos < 1e-3 * np.asarray(VS)).all() and np.array_equal(T, res.T)
        assert all(b < a for a, b in zip(res.history, res.history[1:])) and res.cost == res.history[-1] and res.overlap >= 0.3


def test_refine_rules():
    """The stated rule of the loop: pairs run in lockstep and a pair's answer does not depend on the pairs beside it; `iters` bounds the evaluations;
    a dof subset leaves the other degrees where they were; a T0 that is not eligible comes back as it is, ok False, after one evaluation; a
    rejected trial multiplies the damping until the cap ends the pair."""
    from imvoxelnet_amd.scene import _refine, _check_refine, ALIGN_DOF, DAMPING_CAP
    dims, C, o = (12, 12, 6), 8, (0.0, 0.0, 0.0)
    centre = np.asarray(dims) * np.asarray(VS) / 2
    src = RA.smooth_state(dims, C, 3, voxel_size=VS)
    T_true = RW.rigid(about=centre, **POSES[1])
    w = RW.warp_grid(*src, VS, o, T_true)
    dst = (w['S'].astype(np.float32), w['W'].astype(np.float32))
    args = _check_refine(12, ALIGN_DOF, 0.3, 1e-3, None, 1e-5, VS)
    alone = _refine(_play(dst, src[:2], o, centre), [np.eye(4)], [centre], C, *args)[0]
    calls = []
    far = RW.rigid(t=(50.0, 0, 0))
    both = _refine(_play(dst, src[:2], o, centre, calls), [far, np.eye(4), RW.rigid(0.01)], [centre] * 3, C, *args)
    assert np.array_equal(both[1][0], alone[0]) and both[1][1].stats.tobytes() == alone[1].stats.tobytes() and both[1][1].history == alone[1].history
    assert calls[0] == [0, 1, 2] and all(0 not in c for c in calls[1:]) and calls[1] == [1, 2]      # one call per iteration over the pairs still running
    T, res = both[0]
    assert np.array_equal(T, far) and not res.ok and res.evaluations == 1 and res.used == 0 and res.cost == np.inf and not res.converged
    few = _refine(_play(dst, src[:2], o, centre), [np.eye(4)], [centre], C, *_check_refine(3, ALIGN_DOF, 0.3, 1e-3, None, 1e-5, VS))[0]
    assert few[1].evaluations == 3 and not few[1].converged and few[1].history == alone[1].history[:len(few[1].history)]
    T, res = _refine(_play(dst, src[:2], o, centre), [np.eye(4)], [centre], C, *_check_refine(12, ('x', 'y', 'rz'), 0.3, 1e-3, None, 1e-5, VS))[0]
    assert T[2, 3] == 0 and np.array_equal(T[2, :3], [0, 0, 1]) and np.array_equal(T[:3, 2], [0, 0, 1]) and res.cost < res.history[0]
    # a cost that never falls: every trial is rejected, the damping climbs past the cap, and the pose is the start's

    def flat(idx, Ts):
        return [(10, 10, 10, np.concatenate([[1.0, 1.0, 1.0, 5.0], np.ones(6), RA.full_H(np.ones(21))[np.triu_indices(6)] + 6 * np.eye(6)[np.triu_indices(6)]]))
                for _ in Ts]
    T, res = _refine(flat, [np.eye(4)], [centre], C, *_check_refine(50, ALIGN_DOF, 0.3, 1e-3, 0.0, 0.0, VS))[0]
    n = res.evaluations - 1
    assert np.array_equal(T, np.eye(4)) and res.accepted == 0 and n in (9, 10) and DAMPING_CAP == 1e6 and not res.converged      # 1e-3 * 10^n passes 1e6


# ------------------------------------------------------------------ the helpers
def test_rigid_increment_and_solve_align():
    import imvoxelnet_amd as ia
    from imvoxelnet_amd import ops
    about = np.array([0.4, -1.2, 0.5])
    assert np.array_equal(ia.rigid_increment(np.zeros(6), about), np.eye(4))
    T = ia.rigid_increment([0.1, -0.2, 0.3, 0, 0, 0.25], about)
    assert np.allclose(T, RW.rigid(0.25, t=(0.1, -0.2, 0.3), about=about), atol=1e-15) and T.dtype == np.float64
    T = ia.rigid_increment([0, 0, 0, 0.3, 0, 0], about)
    assert np.allclose(T, RW.rigid(roll=0.3, about=about), atol=1e-15)
    T = ia.rigid_increment([0.01, 0.02, 0.03, 0.2, -0.1, 0.15], about)
    ops.check_rigid(T)
    assert np.allclose((T @ np.append(about, 1))[:3], about + [0.01, 0.02, 0.03], atol=1e-15)       # the rotation goes through `about`
    w = np.array([0.2, -0.1, 0.15])
    assert np.allclose(T[:3, :3] @ w, w, atol=1e-15) and np.isclose(np.trace(T[:3, :3]), 1 + 2 * np.cos(np.linalg.norm(w)))
    small = ia.rigid_increment([0, 0, 0, 1e-9, -2e-9, 3e-9])
    assert np.allclose(small[:3, :3] - np.eye(3), [[0, -3e-9, -2e-9], [3e-9, 0, -1e-9], [2e-9, 1e-9, 0]], atol=1e-17)
    for bad in ((np.zeros(5),), (np.full(6, np.nan),), (np.zeros(6), (0, 0)), (np.zeros(6), (0, np.inf, 0))):
        with pytest.raises(ValueError):
            ia.rigid_increment(*bad)
    rng = np.random.default_rng(0)
    J = rng.standard_normal((40, 6))
    H, g = J.T @ J, rng.standard_normal(6)
    d = ia.solve_align(H, g)
    assert np.allclose(H @ d, -g) and d.dtype == np.float64
    d = ia.solve_align(H, g, 0.5)
    assert np.allclose((H + 0.5 * np.diag(np.diag(H))) @ d, -g)
    d = ia.solve_align(H, g, 0.1, dof=('rz', 'x', 'y'))                       # a subset, in any order: the other degrees stay 0
    sel = [0, 1, 5]
    A = H[np.ix_(sel, sel)]
    assert not d[[2, 3, 4]].any() and np.allclose((A + 0.1 * np.diag(np.diag(A))) @ d[sel], -g[sel])
    assert np.isnan(ia.solve_align(np.zeros((6, 6)), g)).all()                # singular: not finite, which ends a refinement
    assert np.isnan(ia.solve_align(np.zeros((6, 6)), g, dof=('x',))[0]) and not ia.solve_align(np.zeros((6, 6)), g, dof=('x',))[1:].any()
    assert np.isnan(ia.solve_align(H, np.full(6, np.nan))).all()
    for bad in (dict(dof=()), dict(dof='x'), dict(dof=('x', 'x')), dict(dof=('yaw',)), dict(damping=-1), dict(damping=np.nan), dict(damping=True)):
        with pytest.raises(ValueError):
            ia.solve_align(H, g, **bad)
    with pytest.raises(ValueError):
        ia.solve_align(H[:3, :3], g)


def test_align_result():
    import imvoxelnet_amd as ia
    stats = np.concatenate([[2.0, 4.0, 4.0, 8.0], np.arange(6.0), np.arange(21.0) + 10])
    r = ia.AlignResult(np.eye(4), 80, 50, 100, stats, channels=8, min_overlap=0.3)
    assert r.ok and r.used == 50 and r.pairs == 80 and r.own == 100 and r.overlap == 0.5 and r.cost == 8.0 / (50 * 8) and r.ncc == 0.5
    assert np.array_equal(r.g, np.arange(6.0)) and np.array_equal(r.H, r.H.T) and r.H[0, 5] == 15 and r.H[1, 1] == 16 and r.H[5, 5] == 30
    assert r.evaluations == 1 and r.accepted == 0 and not r.converged and r.history == [r.cost] and np.array_equal(r.T, np.eye(4))
    assert not ia.AlignResult(np.eye(4), 80, 29, 100, stats, 8, 0.3).ok and ia.AlignResult(np.eye(4), 80, 30, 100, stats, 8, 0.3).ok
    none = ia.AlignResult(np.eye(4), 0, 0, 0, np.zeros(31), 8, 0.0)
    assert not none.ok and none.cost == np.inf and none.overlap == 0 and none.ncc == -np.inf
    for bad in (-0.1, 1.5, None):
        with pytest.raises(ValueError, match='min_overlap'):
            ia.AlignResult(np.eye(4), 80, 50, 100, stats, 8, bad)
    with pytest.raises(ValueError):
        ia.AlignResult(np.eye(4), 80, 50, 100, stats[:3], 8)


# ------------------------------------------------------------------ the sessions' host side
def _stub_sessions():
    from imvoxelnet_amd import SceneSession
    m = _mock_model(n_voxels=(2, 2, 2), _new_origin=lambda o: torch.tensor(np.asarray(o, np.float32)) - torch.tensor([0.16, 0.16, 0.2]))
    a, b = SceneSession(m, META, decay=0.9), SceneSession(m, dict(META, lidar2img=dict(intrinsic=K4, origin=ORIGIN + np.float32(0.16))), decay=0.9)
    for s in (a, b):
        s._sum, s._wsum, s.n_views = torch.ones(1, 2, 2, 2, 4), torch.ones(1, 2, 2, 2), 1
    return m, a, b


def _bowl(seen):
    """A stand-in for ops.volume_align: the cost is the squared distance of T's translation from (0.05, 0, 0), with the exact normal equations of
    a translation increment in the destination frame (t' = t + R delta: J = R, g = R^T r, H = I)."""
    def fake(vol, ws, rows, src, src_rows, Ts, about, o, so, vs, step):
        seen.append((rows, src_rows, [np.asarray(c[0]) for c in Ts], np.asarray(about), np.asarray(o), np.asarray(so), step))
        B = len(rows)
        stats = np.zeros((B, 1, 31))
        for p, c in enumerate(Ts):
            assert len(c) == 1
            r = np.asarray(c[0])[:3, 3] - np.array([0.05, 0, 0])
            stats[p, 0, :4] = (1.0, 1.0, 1.0, r @ r)
            stats[p, 0, 4:7] = np.asarray(c[0])[:3, :3].T @ r
            stats[p, 0, [10, 16, 21, 25, 28, 30]] = 1.0                      # H = I
        return torch.full((B, 1), 6), torch.full((B, 1), 4), torch.full((B,), 8), torch.from_numpy(stats)
    return fake


def test_session_refusals_and_argument_checks_of_refine(monkeypatch):
    """Refusals are match's, through the same checks, before any launch (ops.volume_align and ops.volume_match are replaced by recorders); iters, dof,
    step, min_overlap, damping and the tolerances are checked before the first launch; what reaches ops is rows [0] of both states, K = 1, the
    grid's centre as `about` and each scene's own corner origin."""
    from imvoxelnet_amd import SceneSession, ops
    from imvoxelnet_amd.scene import _merge_transform
    seen, matches = [], []
    monkeypatch.setattr(ops, 'volume_align', _bowl(seen))
    monkeypatch.setattr(ops, 'volume_match', lambda *a, **k: matches.append(a))
    m = _mock_model()
    a, e = SceneSession(m, META, decay=0.9), SceneSession(m, META, decay=1.0)
    plain, windowed = SceneSession(m, META), SceneSession(m, META, window=3)
    T = RW.rigid(0.3, t=(0.5, 0.1, 0))
    for x, y in ((a, plain), (plain, a)):
        with pytest.raises(NotImplementedError, match='refine: a plain session'):
            x.refine(y, T)
    for x, y in ((a, windowed), (windowed, a)):
        with pytest.raises(NotImplementedError, match='window'):
            x.refine(y, T)
    with pytest.raises(ValueError, match='refine: this scene is empty'):
        a.refine(e, T)
    with pytest.raises(ValueError, match='same prepared model'):
        a.refine(SceneSession(_mock_model(), META, decay=0.9), T)
    with pytest.raises(TypeError, match='SceneSession'):
        a.refine(None)
    c = SceneSession(m, META, decay=0.9)
    c.close()
    with pytest.raises(RuntimeError, match='closed'):
        a.refine(c, T)
    m, a, b = _stub_sessions()
    bad = T.copy()
    bad[:3, :3] *= 1.01
    for kw in (dict(T0=bad), dict(iters=0), dict(iters=2.5), dict(iters=True), dict(dof=()), dict(dof=('x', 'pitch')), dict(dof='x'), dict(step=0), dict(step=(1, 1)),
               dict(min_overlap=2), dict(damping=0), dict(damping=-1), dict(damping=np.inf), dict(tol_shift=-1), dict(tol_rot=np.nan), dict(tol_rot=None)):
        with pytest.raises((ValueError, TypeError)):
            a.refine(b, **kw)
    for kw in (dict(refine=1), dict(refine=True, dof=('q',)), dict(dof=('x',))):
        with pytest.raises(ValueError):
            a.register(b, **kw)
    assert not seen and not matches
    Tr, res = a.refine(b, step=2)
    assert res.ok and res.converged and res.accepted >= 1 and res.evaluations == len(seen) <= 12 and np.allclose(Tr[:3, 3], (0.05, 0, 0), atol=2e-4)
    assert all(s[0] == [0] and s[1] == [0] and s[6] == [2, 2, 2] for s in seen) and np.array_equal(seen[0][2][0], _merge_transform(a, b, None))
    assert np.array_equal(seen[0][3], ORIGIN.astype(np.float64)) and np.array_equal(seen[0][4], m._new_origin(ORIGIN).numpy())
    assert np.array_equal(seen[0][5], m._new_origin(ORIGIN + np.float32(0.16)).numpy()) and res.used == 4 and res.pairs == 6 and res.own == 8
    del seen[:]
    Tr, res = a.refine(b, T0=np.eye(4), dof=('y', 'z'))                       # x may not move: the start is the best it can do
    assert Tr[0, 3] == 0 and len(seen) == 1 and res.converged and res.accepted == 0


def test_register_with_refine(monkeypatch):
    """register(refine=True) runs the lattice as before and then refine from the last level's pose over x, y, z, rz (or the given dof) with the last
    level's lattice step; the default makes the launches it made before and none of align's."""
    from imvoxelnet_amd import ops
    from imvoxelnet_amd.scene import MatchResult
    m, a, b = _stub_sessions()
    seen, matches = [], []

    def fake_match(vol, ws, rows, src, src_rows, Ts, o, so, vs, step):
        matches.append(step)
        K = len(Ts[0])
        return torch.full((1, K), 4), torch.tensor([8]), torch.tensor([[[0.5 + 0.001 * k, 1.0, 1.0] for k in range(K)]], dtype=torch.float64)

    monkeypatch.setattr(ops, 'volume_match', fake_match)
    monkeypatch.setattr(ops, 'volume_align', _bowl(seen))
    T = RW.rigid(0.3, t=(0.5, 0.1, 0))
    T0, r0 = a.register(b, T0=T, levels=2, step=[2, 1])
    assert matches == [[2, 2, 2], [1, 1, 1]] and not seen and isinstance(r0, MatchResult)
    T1, r1 = a.register(b, T0=T, levels=2, step=[2, 3], refine=True)
    assert len(matches) == 4 and seen and np.array_equal(seen[0][2][0], T0) and all(s[6] == [3, 3, 3] for s in seen)
    assert r1.match.best == r0.best and r1.cost < r1.history[0] and np.allclose(T1[:3, 3], (0.05, 0, 0), atol=2e-4)
    assert np.allclose(T1[:3, :3], T0[:3, :3], atol=1e-12)                    # H = I on the translations only: the turn stays


def test_batch_refine(monkeypatch):
    """SceneBatch.refine: the refusals of match; one ops.volume_align per iteration over the pairs still running, K = 1; each pair's `about` and
    origins are its scene's; one pair alone gives one answer, lists give a list."""
    from imvoxelnet_amd import SceneBatch, ops
    seen = []
    monkeypatch.setattr(ops, 'volume_align', _bowl(seen))
    T = RW.rigid(0.3, t=(0.5, 0.1, 0))
    b = SceneBatch(_mock_model(), [META] * 4, decay=0.9)
    for args in (([0, 4], [1, 2]), ([0, 1], [2]), ([], []), (-1, 2), (True, 2), ([0, 1], [2, 3], [T])):
        with pytest.raises(ValueError):
            b.refine(*args)
    with pytest.raises(ValueError, match=r'refine: scenes \[0, 2\] are empty'):
        b.refine(0, 2, T)
    with pytest.raises(NotImplementedError, match='decay=1.0'):
        SceneBatch(_mock_model(), [META] * 2).refine(0, 1, T)
    with pytest.raises(NotImplementedError, match='window'):
        SceneBatch(_mock_model(), [META] * 2, window=2).refine(0, 1, T)
    assert not seen
    m = _mock_model(n_voxels=(2, 2, 2), _new_origin=lambda o: torch.tensor(np.asarray(o, np.float32)) - torch.tensor([0.16, 0.16, 0.2]))
    b = SceneBatch(m, [META, META, dict(META, lidar2img=dict(intrinsic=K4, origin=ORIGIN + np.float32(0.16)))], decay=0.9)
    b._sum, b._wsum = torch.ones(3, 2, 2, 2, 4), torch.ones(3, 2, 2, 2)
    for r in b._scenes:
        r.n_views = 1
    for kw in (dict(iters=0), dict(dof=('a',)), dict(damping=0), dict(step=0)):
        with pytest.raises(ValueError):
            b.refine(0, 1, np.eye(4), **kw)
    assert not seen
    near = np.eye(4)
    near[0, 3] = 0.05                                                         # already at the minimum: converged after one evaluation
    out = b.refine([2, 0], [0, 1], [near, np.eye(4)])
    assert len(out) == 2 and out[0][1].converged and out[0][1].evaluations == 1 and out[1][1].accepted >= 1 and np.allclose(out[1][0][:3, 3], (0.05, 0, 0), atol=2e-4)
    assert seen[0][0] == [2, 0] and seen[0][1] == [0, 1] and all(s[0] == [0] and s[1] == [1] for s in seen[1:]) and len(seen) == out[1][1].evaluations
    assert np.array_equal(seen[0][3], np.stack([ORIGIN + np.float32(0.16), ORIGIN]).astype(np.float64))
    assert np.array_equal(seen[0][4][0], m._new_origin(ORIGIN + np.float32(0.16)).numpy()) and np.array_equal(seen[0][5][1], m._new_origin(ORIGIN).numpy())
    T1, r1 = b.refine(0, 1, np.eye(4))
    assert np.array_equal(T1, out[1][0]) and r1.history == out[1][1].history
    b.close()
    with pytest.raises(RuntimeError, match='closed'):
        b.refine(0, 1, T)


def test_the_docs_speak_of_aligning():
    import imvoxelnet_amd as ia
    doc = ia.scene.__doc__
    assert 'Aligning scenes' in doc and NAME in doc and 'volume_align' in doc and 'LOCAL' in doc[doc.index('Aligning scenes'):doc.index('Scene snapshots')]
    out = doc[doc.index('Out of scope'):]
    for words in ('a global search', 'pitch and roll', 'weighting pairs by evidence', 'Pearson', 'gradient-based', 'matching plain or windowed', 'de-duplicating',
                  'robust loss', 'refining against a snapshot', 'on the device'):
        assert words in out, words
    for fn in (ia.SceneSession.refine, ia.SceneBatch.refine):
        assert 'LOCAL' in fn.__doc__ and 'register' in fn.__doc__ and 'a voxel' in fn.__doc__
    assert 'refine=True' in ia.SceneSession.register.__doc__ and 'refine=True' in ia.SceneBatch.register.__doc__
    assert 'volume_match' in ia.ops.volume_align.__doc__ and all(hasattr(ia, n) for n in ('AlignResult', 'rigid_increment', 'solve_align'))
    header = open(os.path.join(ROOT, 'include', 'imvoxel.h')).read()
    section = header[header.index('(0.5.8) The Gauss-Newton normal equations'):header.index('int ivx_volume_align_fwd')]
    for words in ('Read only', 'Deterministic', 'Match parity.', 'Zero weights.', 'Identity.', 'Error.', 'used', 'about', 'four rounded', 'bit for bit'):
        assert words in section, words
    assert 'volume_align' in open(os.path.join(ROOT, 'DESIGN.md')).read() and 'aligning scenes' in open(os.path.join(ROOT, 'README.md')).read().lower()
    assert os.path.exists(os.path.join(ROOT, 'profiles', 'scene_align.md')) and os.path.exists(os.path.join(ROOT, 'tools', 'scene_align_bench.py'))
