"""-m gpu: the rigid resample of the state pools (ops.volume_warp, ivx_volume_warp_fwd, csrc/volume_warp.hip) against the numpy reference of its
definition (tests/ref_volume_warp.py): within the derived bound for a general motion, bit for bit where the definition moves bits (a whole-voxel
translation against ops.volume_scroll_, a quarter turn as a permutation), the guards (destination rows pre-filled with NaN, canaries in the rows no
sample names, a NaN cell under a zero-weight corner), constant means, forgetting, two samples with different transforms and row maps, and more
samples than one launch holds."""
import numpy as np
import pytest
import torch

import ref_volume_warp as RW

pytestmark = pytest.mark.gpu

# (X, Y, Z), C: one, two, sixteen and sixty-four 16-byte words per voxel; voxel counts that are no multiple of the voxels a wave owns
GRIDS = [((7, 5, 6), 8), ((9, 8, 4), 64), ((5, 4, 3), 256), ((6, 6, 3), 4)]
VS = (0.16, 0.16, 0.2)


@pytest.fixture(scope='module')
def ops():
    from imvoxelnet_amd import _lib, ops
    _lib.lib()
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    return ops


def _origin(dims, vs=VS):
    """A new_origin that centres the grid near (0.03, -0.02, 0.01): fractional, so nothing is exact by accident."""
    return (np.array([0.03, -0.02, 0.01]) - np.asarray(dims) / 2 * np.asarray(vs)).astype(np.float32)


def _src(R, dims, C, seed, unseen=0.15):
    """Host source pools (sum, wsum, count) with R rows: weight sums in [0.5, 4), sums = mean * weight, counts in 1 .. 8, and a share of unseen
    voxels (all zero), as a fused scene has."""
    rng = np.random.default_rng(seed)
    W = rng.uniform(0.5, 4.0, (R,) + dims).astype(np.float32)
    S = (rng.standard_normal((R,) + dims + (C,)) * W[..., None]).astype(np.float32)
    cnt = rng.integers(1, 9, (R,) + dims).astype(np.int32)
    gone = rng.random((R,) + dims) < unseen
    S[gone], W[gone], cnt[gone] = 0, 0, 0
    return S, W, cnt


CANARY_F, CANARY_I = -12345.5, -77


def _run(ops, src, rows, Ts, origins, vs, R_out, out_rows, forget=0.0):
    """Upload, warp into destination pools whose every row is NaN / -1 first, except that the rows no sample names carry canaries -> host (sum, wsum, count)."""
    S, W, c = (torch.from_numpy(a).cuda() for a in src)
    named = set(out_rows)
    out = (torch.full((R_out,) + tuple(S.shape[1:]), float('nan'), device='cuda'), torch.full((R_out,) + tuple(W.shape[1:]), float('nan'), device='cuda'),
           torch.full((R_out,) + tuple(c.shape[1:]), -1, device='cuda', dtype=torch.int32))
    for r in range(R_out):
        if r not in named:
            out[0][r], out[1][r], out[2][r] = CANARY_F, CANARY_F, CANARY_I
    keep = [t.clone() for t in (S, W, c)]
    got = ops.volume_warp(S, W, c, rows, Ts, origins, vs, out=out, out_rows=out_rows, forget_below=forget)
    assert got is out
    torch.cuda.synchronize()
    for t, k in zip((S, W, c), keep):
        assert torch.equal(t.view(torch.int32), k.view(torch.int32)), 'the source pools are read only'
    host = [t.cpu().numpy() for t in out]
    for r in range(R_out):
        if r not in named:
            assert (host[0][r] == CANARY_F).all() and (host[1][r] == CANARY_F).all() and (host[2][r] == CANARY_I).all(), f'row {r} is named by no sample'
    return host


def _compare(got_row, ref, what=''):
    """One destination row against the reference within the bound; count equal.  -> the worst ratios (S, W)."""
    S, W, c = got_row
    assert np.isfinite(S).all() and np.isfinite(W).all(), 'every voxel of a named row is written'
    rs, rw = RW.worst_ratio(S, ref['S'], ref['bound_S']), RW.worst_ratio(W, ref['W'], ref['bound_W'])
    print(f'{what}: worst |got - ref| / bound  sums {rs:.3f}  weight sum {rw:.3f}  (K = {RW.K_WARP}); seen {int((ref["W"] > 0).sum())} of {ref["W"].size}')
    assert np.array_equal(c, ref['cnt']), (what, int((c != ref['cnt']).sum()))
    assert rs <= 1 and rw <= 1, (what, rs, rw)
    return rs, rw


@pytest.mark.parametrize('dims,C', GRIDS, ids=lambda v: str(v).replace(' ', ''))
def test_general_motion_within_the_bound(ops, dims, C):
    """A rotation about all three axes plus a fractional translation, row 1 of 3 into row 2 of 4: sums and weight sum within K * 2^-24 * sum |w S| of
    the float64 reference on the device's own i0 and f, count equal; the border thins (voxels with fewer than eight corners exist) and part of the
    grid leaves."""
    src, o = _src(3, dims, C, 10 + C), _origin(dims)
    T = RW.rigid(0.23, 0.04, -0.03, (0.11, -0.07, 0.05))
    got = _run(ops, src, [1], [T], o[None], VS, 4, [2])
    ref = RW.warp_grid(src[0][1], src[1][1], src[2][1], VS, o, T)
    n_read = ref['read'].sum(-1)
    assert (n_read == 8).any() and ((n_read > 0) & (n_read < 8)).any() and (n_read == 0).any()
    _compare([g[2] for g in got], ref, f'{dims} C={C}')
    # a second geometry, through the 3x4 form, one matrix alone and one origin for all
    T2 = RW.rigid(-1.1, t=(0.3, 0.2, -0.1))
    got = _run(ops, src, [0], T2[:3], o, VS, 1, [0])
    _compare([g[0] for g in got], RW.warp_grid(src[0][0], src[1][0], src[2][0], VS, o, T2), f'{dims} C={C} yaw -1.1')


DY_VS = (0.25, 0.25, 0.5)


def _dyadic_origin(dims):
    return (-(np.asarray(dims) // 2) * np.asarray(DY_VS)).astype(np.float32)


@pytest.mark.parametrize('dims,C', GRIDS, ids=lambda v: str(v).replace(' ', ''))
def test_whole_voxel_translation_gives_the_bits_of_the_scroll(ops, dims, C):
    """Dyadic voxel sizes and an origin on their lattice: the chain is exact, g is the index plus the shift, every voxel has one corner of weight 1, and
    the warp by t = shift * voxel_size gives the bits ops.volume_scroll_ gives on a copy -- sums, weight sum and count, the vacated shell zero."""
    src, o = _src(2, dims, C, 20 + C), _dyadic_origin(dims)
    for shift in ((1, 0, 0), (0, -2, 0), (0, 0, 1), (2, -1, 1), (-3, 2, -2), (0, 0, dims[2]), (-dims[0] - 2, 0, 0)):
        T = np.eye(4)
        T[:3, 3] = np.asarray(shift) * np.asarray(DY_VS)
        got = _run(ops, src, [1], [T], o[None], DY_VS, 2, [0])
        S, W, c = (torch.from_numpy(a[1:2].copy()).cuda() for a in src)
        ops.volume_scroll_(S, c, [0], [shift], W)
        for name, g, w in zip(('sum', 'wsum', 'count'), got, (S, W, c)):
            assert np.array_equal(g[0].view(np.int32), w[0].cpu().numpy().view(np.int32)), (name, shift)
        if max(abs(s) >= d for s, d in zip(shift, dims)):
            assert not got[0][0].any() and not got[1][0].any() and not got[2][0].any()


def test_quarter_yaw_is_the_exact_permutation(ops):
    """The quarter turn about the centre of the square dyadic grid (6, 6, 3): new[i,j,k] = old[N-1-j, i, k], bit for bit, and four turns are the identity."""
    dims, C, N = (6, 6, 3), 4, 6
    src, o = _src(1, dims, C, 31, unseen=0.2), _dyadic_origin(dims)
    centre = o[:2].astype(np.float64) + (N - 1) / 2 * 0.25
    T = RW.quarter_yaw((centre[0], centre[1], 0.0))
    i, j, k = np.meshgrid(np.arange(N), np.arange(N), np.arange(3), indexing='ij')
    cur = src
    for turn in range(4):
        got = _run(ops, cur, [0], [T], o[None], DY_VS, 1, [0])
        for g, s in zip(got, cur):
            assert np.array_equal(g[0].view(np.int32), s[0][N - 1 - j, i, k].view(np.int32)), turn
        cur = got
    for g, s in zip(cur, src):
        assert np.array_equal(g.view(np.int32), s.view(np.int32))


@pytest.mark.parametrize('dims,C', GRIDS, ids=lambda v: str(v).replace(' ', ''))
def test_translation_beyond_the_grid_leaves_the_row_all_zero(ops, dims, C):
    src, o = _src(1, dims, C, 40 + C, unseen=0.0), _origin(dims)
    for t in ((dims[0] * VS[0] + 0.01, 0, 0), (0, -(dims[1] + 1) * VS[1], 0), (0.05, 0.03, 50.0), (1e30, 0, 0)):
        got = _run(ops, src, [0], [RW.rigid(t=t)], o[None], VS, 1, [0])
        assert all(not g.view(np.int32).any() for g in got), t


def test_a_nan_cell_under_a_zero_weight_corner_does_not_propagate(ops):
    """Dyadic grid, translation by (1, 0.5, 0) voxels: f = (0, 0.5, 0), so of the eight corners only (0,0,0) and (0,1,0) have weight.  Source cells that
    are only ever a zero-weight corner hold NaN sums, NaN weight and a huge count: none of it shows.  The same cells under a non-zero weight do show."""
    dims, C = (7, 5, 6), 8
    src, o = _src(1, dims, C, 51, unseen=0.0), _dyadic_origin(dims)
    T = np.eye(4)
    T[:3, 3] = (1 * 0.25, 0.5 * 0.25, 0.0)
    ref = RW.warp_grid(*(a[0] for a in src), DY_VS, o, T)
    used = np.zeros(dims, bool)                                               # the source cells some destination reads
    inside, i0, f = RW.grid_coords(dims, DY_VS, o, T)
    assert set(np.unique(f[inside])) == {0.0, 0.5} and (f[inside][:, 1] == 0.5).all() and not f[inside][:, [0, 2]].any()
    for c in range(8):
        idx = (i0 + np.array([c >> 2, (c >> 1) & 1, c & 1]))[ref['read'].reshape(-1, 8)[:, c]]
        used[idx[:, 0], idx[:, 1], idx[:, 2]] = True
    assert used.any() and (~used).any()
    S, W, c = (a.copy() for a in src)
    S[0][~used], W[0][~used], c[0][~used] = np.nan, np.nan, 2 ** 30
    got = _run(ops, (S, W, c), [0], [T], o[None], DY_VS, 1, [0])
    _compare([g[0] for g in got], ref, 'NaN under zero-weight corners')
    assert got[2].max() <= 8
    S2, W2 = src[0].copy(), src[1].copy()                                     # ... and a NaN where a weight is not zero does propagate: the guard is the weight
    cell = tuple(np.argwhere(used)[0])
    S2[0][cell], W2[0][cell] = np.nan, np.nan
    got = _run(ops, (S2, W2, src[2]), [0], [T], o[None], DY_VS, 1, [0])
    assert np.isnan(got[1]).any() and np.isnan(got[0]).any()


@pytest.mark.parametrize('dims,C', GRIDS, ids=lambda v: str(v).replace(' ', ''))
def test_a_constant_mean_survives(ops, dims, C):
    """S = m_c * W per channel with uneven W: wherever the warped voxel is seen, S' / W' == m_c within (2 K + 1) * 2^-24 relative -- both sums within
    K * 2^-24 of exact sums of positive terms, and one rounding in the quotient."""
    rng = np.random.default_rng(60 + C)
    W = rng.uniform(0.25, 8.0, (1,) + dims).astype(np.float32)
    m = rng.uniform(0.5, 3.0, C).astype(np.float32)
    S = (W[..., None].astype(np.float64) * m).astype(np.float32)
    m_eff = S.astype(np.float64) / W[..., None]                               # the means as stored (one rounding in S): within 2^-24 of m
    src, o = (S, W, np.ones((1,) + dims, np.int32)), _origin(dims)
    got = _run(ops, src, [0], [RW.rigid(0.4, -0.05, 0.02, (0.05, 0.02, -0.03))], o[None], VS, 1, [0])
    seen = got[1][0] > 0
    assert seen.sum() >= 10
    ratio = got[0][0][seen].astype(np.float64) / got[1][0][seen][:, None]
    lo, hi = m_eff.min(axis=(0, 1, 2, 3)), m_eff.max(axis=(0, 1, 2, 3))
    tol = (2 * RW.K_WARP + 1) * RW.U
    print(f'{dims} C={C}: worst relative departure of the mean {float(np.abs(ratio / m - 1).max()):.3e} (allowed {tol + RW.U:.3e})')
    assert (ratio >= lo * (1 - tol)).all() and (ratio <= hi * (1 + tol)).all()
    assert not got[0][0][~seen].any() and (got[2][0][seen] == 1).all() and not got[2][0][~seen].any()


@pytest.mark.parametrize('dims,C', GRIDS, ids=lambda v: str(v).replace(' ', ''))
def test_forget_below_on_robust_inputs(ops, dims, C):
    """The threshold sits midway in the widest gap of the reference's sorted W' (the reference asserts the margin): the voxels below it are unseen,
    all bits zero, the others equal the call without a threshold bit for bit."""
    src, o = _src(1, dims, C, 70 + C), _origin(dims)
    T = RW.rigid(0.3, 0.02, 0.01, (0.06, 0.04, 0.02))
    ref0 = RW.warp_grid(*(a[0] for a in src), VS, o, T)
    w = np.sort(ref0['W'][ref0['W'] > 0])
    lo, hi = len(w) // 4, 3 * len(w) // 4                                     # ... of the middle half, so that both sides are populated
    gap = lo + int(np.argmax(np.diff(w[lo:hi])))
    fb = float(np.float32((w[gap] + w[gap + 1]) / 2))
    ref = RW.warp_grid(*(a[0] for a in src), VS, o, T, forget_below=fb)
    plain, got = _run(ops, src, [0], [T], o[None], VS, 1, [0]), _run(ops, src, [0], [T], o[None], VS, 1, [0], forget=fb)
    _compare([g[0] for g in got], ref, f'{dims} C={C} forget_below={fb:.4f}')
    gone = (ref0['W'] > 0) & (ref0['W'] < fb)
    assert gone.sum() >= 5 and (~gone & (ref0['W'] > 0)).sum() >= 5
    for g, p in zip(got, plain):
        assert not g[0][gone].view(np.int32).any() and np.array_equal(g[0][~gone].view(np.int32), p[0][~gone].view(np.int32))


def test_two_samples_with_different_transforms_and_row_maps(ops):
    """B = 2: source rows [2, 0] of 3 into destination rows [1, 3] of 5, each with its own transform and its own origin; and two samples that read ONE
    source row under different transforms."""
    dims, C = (9, 8, 4), 64
    src = _src(3, dims, C, 80)
    o = np.stack([_origin(dims), _origin(dims) + np.float32(0.05)])
    Ts = [RW.rigid(0.2, t=(0.1, 0, 0.02)), RW.rigid(-0.35, 0.03, 0.0, (-0.08, 0.12, 0))]
    got = _run(ops, src, [2, 0], Ts, o, VS, 5, [1, 3])
    for b, (rs, rd) in enumerate(((2, 1), (0, 3))):
        _compare([g[rd] for g in got], RW.warp_grid(src[0][rs], src[1][rs], src[2][rs], VS, o[b], Ts[b]), f'sample {b}: row {rs} -> {rd}')
    got = _run(ops, src, [1, 1], Ts, o, VS, 2, [1, 0])
    for b, rd in enumerate((1, 0)):
        _compare([g[rd] for g in got], RW.warp_grid(src[0][1], src[1][1], src[2][1], VS, o[b], Ts[b]), f'shared source row, sample {b}')


def test_more_samples_than_one_launch_carries(ops):
    """35 samples on the (6, 6, 3) grid at C = 4: rows, transforms and origins travel by value, 32 per launch, so this call is chunked."""
    dims, C, B = (6, 6, 3), 4, 35
    src, o = _src(B, dims, C, 90), _origin(dims)
    rows, out_rows = [(r * 12) % B for r in range(B)], [(r * 3 + 1) % (B + 2) for r in range(B)]
    assert len(set(rows)) == B and len(set(out_rows)) == B
    Ts = [RW.rigid(0.05 * (b - 17), t=(0.01 * b, -0.02 * (b % 5), 0.0)) for b in range(B)]
    origins = np.stack([o + np.float32(0.01 * (b % 4)) for b in range(B)])
    got = _run(ops, src, rows, Ts, origins, VS, B + 2, out_rows)
    worst = 0.0
    for b in range(B):
        ref = RW.warp_grid(src[0][rows[b]], src[1][rows[b]], src[2][rows[b]], VS, origins[b], Ts[b])
        assert np.array_equal(got[2][out_rows[b]], ref['cnt']), b
        worst = max(worst, RW.worst_ratio(got[0][out_rows[b]], ref['S'], ref['bound_S']), RW.worst_ratio(got[1][out_rows[b]], ref['W'], ref['bound_W']))
    print(f'35 samples: worst |got - ref| / bound {worst:.3f}')
    assert worst <= 1
