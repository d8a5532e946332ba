"""-m gpu: scoring candidate poses between rows of the state pools (ops.volume_match, ivx_volume_match_fwd, csrc/volume_match.hip) against the numpy
reference of its definition (tests/ref_volume_match.py): pairs and own equal and the statistics within the derived bound for general candidates
between grids of different origins -- more candidates than one launch carries --, nothing written (both pools keep their bits, NaN in the rows no
sample names, under zero-weight corners and at unpaired voxels does not show), bit-equal answers from call to call and from any rows of any pools,
one pool on both sides and a row against itself, the lattice step, the identity on a dyadic grid with dot == na == nb bit for bit, the recovery of a
known transform among candidates a voxel and ten degrees away, and a candidate with no overlap.  Grids, voxel sizes and source states are the warp
tests'."""
import numpy as np
import pytest
import torch

import ref_volume_match as RX
import ref_volume_warp as RW
from test_gpu_volume_warp import GRIDS, VS, DY_VS, _origin, _dyadic_origin, _src

pytestmark = pytest.mark.gpu
IDS = lambda v: str(v).replace(' ', '')      # noqa: E731


@pytest.fixture(scope='module')
def ops():
    from imvoxelnet_amd import _lib, ops
    _lib.lib()
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    return ops


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def _slabs(dst, src):
    """Unseen slabs instead of scattered unseen voxels (a lone seen voxel among unseen ones makes W_s > 0 a matter of one tiny corner weight, which
    the reference refuses): the low-x third of every source row and the high-y quarter of every destination row hold nothing."""
    nx, ny = max(1, src[0].shape[1] // 3), max(1, dst[0].shape[2] // 4)
    for a in src:
        a[:, :nx] = 0
    for a in dst:
        a[:, :, -ny:] = 0
    return dst, src


def _pools(dims, C, seed, R_dst=4, R_src=3):
    return _slabs(_src(R_dst, dims, C, seed, unseen=0.0)[:2], _src(R_src, dims, C, seed + 1, unseen=0.0)[:2])


def _candidates(K=35):
    """Rotations about three axes with fractional shifts, all different."""
    return [RW.rigid(0.05 * (k - 17) + 0.013, 0.02 * (k % 5 - 2), 0.015 * (k % 3 - 1), (0.011 * k - 0.15, 0.05 - 0.02 * (k % 7), 0.013 * (k % 4) - 0.01)) for k in range(K)]


def _device(ops, dst, src, rows, src_rows, cands, od, os_, vs=VS, step=(1, 1, 1)):
    """Upload (src None: the destination pools are their own source), match, check that no bit of a pool changed -> host (pairs [B,K], own [B], stats
    [B,K,3]) and the device pools."""
    dev = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in dst)
    sdev = dev if src is None else tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in src)
    keep = [_bits(t).clone() for t in dev + sdev]
    pairs, own, stats = ops.volume_match(*dev, rows, sdev, src_rows, cands, od, os_, vs, step)
    torch.cuda.synchronize()
    B, K = len(rows), len(cands[0])
    assert pairs.shape == (B, K) and pairs.dtype == torch.int64 and own.shape == (B,) and own.dtype == torch.int64
    assert stats.shape == (B, K, 3) and stats.dtype == torch.float64 and pairs.is_cuda and own.is_cuda and stats.is_cuda
    for t, k in zip(dev + sdev, keep):
        assert torch.equal(_bits(t), k), 'the pools are read only'
    return pairs.cpu().numpy(), own.cpu().numpy(), stats.cpu().numpy()


@pytest.mark.parametrize('dims,C', GRIDS, ids=IDS)
def test_general_candidates_against_the_reference(ops, dims, C):
    """35 candidates (a call crosses the 32-per-launch chunk), a source grid whose origin is off by 0.05, destination row 2 of 4 and source row 1
    of 3.  pairs and own are equal, the statistics lie within the derived bound, and every class of voxel occurs: not own, outside, inside with
    the source unseen, fewer than eight corners read, paired."""
    dst, src = _pools(dims, C, 300 + C)
    o, Ts = _origin(dims), _candidates()
    ref = RX.match_rows([a[2] for a in dst], [a[1] for a in src], VS, o, o + np.float32(0.05), Ts)
    pairs, own, stats = _device(ops, dst, src, [2], [1], [Ts], o, o + np.float32(0.05))
    RX.check((pairs[0], own[0], stats[0]), ref, f'{dims} C={C}, 35 candidates')
    classes = dict(not_own=0, outside=0, unseen=0, fewer=0, paired=0)
    for r in ref['refs']:
        n_read = r['read'].sum(-1)
        classes['not_own'] += int((r['visited'] & ~r['own_mask']).sum())
        classes['outside'] += int((r['own_mask'] & ~r['inside']).sum())
        classes['unseen'] += int((r['own_mask'] & r['inside'] & ~r['paired']).sum())
        classes['fewer'] += int((r['paired'] & (n_read < 8)).sum())
        classes['paired'] += int(r['paired'].sum())
    print(f'{dims} C={C}: {classes}')
    assert all(v > 0 for v in classes.values()), classes
    assert len(set(ref['pairs'].tolist())) > 5 and np.isfinite(stats).all()


def test_nothing_is_written_and_nan_does_not_leak(ops):
    """Both pools keep their bits (_device checks every call of this file); the rows no sample names are all NaN; the half-voxel translation of the
    warp test on the dyadic grid gives two corners weight, and the source cells that are only ever a zero-weight corner hold NaN, as do the sums
    of every destination voxel that is not paired and the weight sums of the rows beside: the answer is the clean reference's."""
    dims, C = (7, 5, 6), 8
    dst, src = _pools(dims, C, 320, R_dst=3, R_src=3)
    o = _dyadic_origin(dims)
    T = np.eye(4)
    T[:3, 3] = (1 * 0.25, 0.5 * 0.25, 0.0)
    Ts = [T, RW.rigid(t=(0.25, 0.375, 0.0))]
    d_row, s_row = [a[1] for a in dst], [a[2] for a in src]
    ref = RX.match_rows(d_row, s_row, DY_VS, o, o, Ts)
    used, paired = np.zeros(dims, bool), np.zeros(dims, bool)
    for r, M in zip(ref['refs'], Ts):
        _, i0, f = RX.grid_coords(dims, DY_VS, o, o, M)
        assert set(np.unique(f[r['inside'].reshape(-1)])) == {0.0, 0.5}
        for c in range(8):
            idx = (i0 + np.array([c >> 2, (c >> 1) & 1, c & 1]))[r['read'].reshape(-1, 8)[:, c]]
            used[idx[:, 0], idx[:, 1], idx[:, 2]] = True
        paired |= r['paired']
    assert used.any() and (~used).any() and paired.any() and (~paired).any()
    dirty_d, dirty_s = [a.copy() for a in dst], [a.copy() for a in src]
    dirty_s[0][2][~used], dirty_s[1][2][~used] = np.nan, np.nan                # never read with a weight: NaN sums and NaN weight
    dirty_d[0][1][~paired] = np.nan                                           # the sums of a voxel that no candidate pairs are not read
    for r in (0, 2):
        dirty_d[0][r], dirty_d[1][r] = np.nan, np.nan                         # rows no sample names
    for r in (0, 1):
        dirty_s[0][r], dirty_s[1][r] = np.nan, np.nan
    pairs, own, stats = _device(ops, dirty_d, dirty_s, [1], [2], [Ts], o, o, vs=DY_VS)
    assert np.isfinite(stats).all()
    RX.check((pairs[0], own[0], stats[0]), ref, 'NaN under zero-weight corners and at unpaired voxels')


def test_determinism_rows_and_pools(ops):
    """Two calls give bit-equal statistics; the same two states in other rows of larger pools, beside other samples and with other candidates in the
    same call, give the same bits; one pool serves as source and destination; a row is matched against itself."""
    dims, C = (9, 8, 4), 64
    dst, src = _pools(dims, C, 340)
    o, os_, Ts = _origin(dims), _origin(dims) + np.float32(0.05), _candidates(5)
    first = _device(ops, dst, src, [2], [1], [Ts], o, os_)
    again = _device(ops, dst, src, [2], [1], [Ts], o, os_)
    for a, b in zip(first, again):
        assert np.array_equal(a, b) and a.tobytes() == b.tobytes()
    rng = np.random.default_rng(341)
    big_d = [rng.uniform(0.5, 2, (7,) + a.shape[1:]).astype(np.float32) for a in dst]
    big_s = [rng.uniform(0.5, 2, (6,) + a.shape[1:]).astype(np.float32) for a in src]
    for a, b in zip(big_d, dst):
        a[5] = b[2]
    for a, b in zip(big_s, src):
        a[0] = b[1]
    other = _candidates(10)[5:]
    moved = _device(ops, big_d, big_s, [1, 5, 3], [4, 0, 0], [other, Ts, other], np.stack([o, o, os_]), np.stack([o, os_, o]))
    assert moved[0][1].tobytes() == first[0][0].tobytes() and moved[1][1] == first[1][0] and moved[2][1].tobytes() == first[2][0].tobytes()
    # one pool on both sides: rows 0 and 3 of the destination pools, and row 1 against itself
    ref = RX.match_rows([a[0] for a in dst], [a[3] for a in dst], VS, o, os_, Ts)
    own_ref = RX.match_rows([a[1] for a in dst], [a[1] for a in dst], VS, o, os_, Ts)
    same = _device(ops, dst, None, [0, 1], [3, 1], [Ts, Ts], o, os_)
    RX.check((same[0][0], same[1][0], same[2][0]), ref, 'one pool as source and destination')
    RX.check((same[0][1], same[1][1], same[2][1]), own_ref, 'a row against itself')
    assert own_ref['pairs'].min() > 0


@pytest.mark.parametrize('dims,C', GRIDS, ids=IDS)
def test_lattice_step(ops, dims, C):
    """step = (2, 1, 2) equals the reference on the sub-lattice; one integer means all three axes; a step larger than the grid leaves the voxel at
    the origin only."""
    dst, src = _pools(dims, C, 360 + C)
    o, Ts = _origin(dims), _candidates(4)
    d_row, s_row = [a[2] for a in dst], [a[1] for a in src]
    for step in ((2, 1, 2), (1, 3, 1), 2):
        p = (step,) * 3 if isinstance(step, int) else step
        ref = RX.match_rows(d_row, s_row, VS, o, o + np.float32(0.05), Ts, p)
        pairs, own, stats = _device(ops, dst, src, [2], [1], [Ts], o, o + np.float32(0.05), step=step)
        RX.check((pairs[0], own[0], stats[0]), ref, f'{dims} C={C}, step {step}')
        assert ref['own'] == int((RX.lattice(dims, p).reshape(dims) & (d_row[1] > 0)).sum())
    far = RW.rigid(0.01, t=(0.02, 0.01, 0.0))
    ref = RX.match_rows(d_row, s_row, VS, o, o, [far], (99, 99, 99))
    pairs, own, stats = _device(ops, dst, src, [2], [1], [[far]], o, o, step=(99, 99, 99))
    assert ref['refs'][0]['visited'].sum() == 1 and ref['own'] == 1 and own[0] == 1 and pairs[0, 0] == ref['pairs'][0] <= 1
    RX.check((pairs[0], own[0], stats[0]), ref, f'{dims} C={C}, step 99')


@pytest.mark.parametrize('dims,C', GRIDS, ids=IDS)
def test_identity_on_the_dyadic_grid(ops, dims, C):
    """M = I, equal origins, dyadic voxel sizes and an origin on their lattice, a state against itself: one corner of weight 1 per voxel, so b == a bit
    for bit, dot == na == nb bit for bit, ncc == 1 and pairs == own == the seen voxels."""
    S, W, _ = _src(2, dims, C, 380 + C)
    o = _dyadic_origin(dims)
    pairs, own, stats = _device(ops, (S, W), None, [1], [1], [[np.eye(4)]], o, o, vs=DY_VS)
    seen = int((W[1] > 0).sum())
    assert pairs[0, 0] == own[0] == seen and 0 < seen < W[1].size
    dot, na, nb = stats[0, 0]
    assert dot == na == nb > 0 and dot / np.sqrt(na * nb) == 1.0
    ref = RX.match_rows((S[1], W[1]), (S[1], W[1]), DY_VS, o, o, [np.eye(4)])
    RX.check((pairs[0], own[0], stats[0]), ref, f'{dims} C={C}, identity')


@pytest.mark.parametrize('kind', ['iid', 'smooth'])
def test_recovery_of_a_known_transform(ops, kind):
    """dst = ops.volume_warp(src, T_true); the candidates are pose_candidates around T_true with offsets of one voxel and ten degrees, the truth at
    index 40: the best score is the truth's, on the random state of the warp tests and on a smooth one."""
    from imvoxelnet_amd import pose_candidates, MatchResult
    if kind == 'iid':
        dims, C = (9, 8, 4), 64
        src = _src(1, dims, C, 400)
    else:
        dims, C = (12, 12, 6), 8
        src = tuple(a[None] for a in RX.smooth_state(dims, C, 5, unseen=0.1, voxel_size=VS))
    o = _origin(dims)
    centre = o.astype(np.float64) + np.asarray(dims) / 2 * np.asarray(VS)
    T_true = RW.rigid(0.21, t=(0.23, -0.17, 0.06), about=centre)
    S, W, c = (torch.from_numpy(a).cuda() for a in src)
    out = tuple(torch.zeros_like(t) for t in (S, W, c))
    ops.volume_warp(S, W, c, [0], [T_true], o[None], VS, out=out)
    Ts = pose_candidates(T_true, np.radians(10), VS, centre)
    pairs, own, stats = ops.volume_match(out[0], out[1], [0], (S, W), [0], [Ts], o, o, VS)
    r = MatchResult(pairs[0].cpu().numpy(), int(own[0]), stats[0].cpu().numpy(), Ts, 0.3)
    order = np.argsort(r.score)
    print(f'{kind}: ncc at the truth {r.score[40]:.6f} (overlap {r.overlap[40]:.2f}), next best {r.score[order[-2]]:.6f} at {order[-2]}; eligible {int(np.isfinite(r.score).sum())} of 81')
    assert r.best == 40 and int(np.argmax(r.score)) == 40 and r.score[40] > 0.999 and np.array_equal(r.T, T_true)
    assert np.isfinite(r.score).sum() > 40


def test_zero_overlap(ops):
    """A candidate that moves the source wholly outside: pairs == 0, statistics all +0, score -inf; its neighbour in the same call is unaffected."""
    dims, C = (6, 6, 3), 4
    dst, src = _pools(dims, C, 420)
    o = _origin(dims)
    near, far = RW.rigid(0.1, t=(0.03, 0.02, 0.01)), RW.rigid(0.1, t=(50.0, 0, 0))
    pairs, own, stats = _device(ops, dst, src, [0], [0], [[far, near, far]], o, o)
    ref = RX.match_rows([a[0] for a in dst], [a[0] for a in src], VS, o, o, [far, near, far])
    RX.check((pairs[0], own[0], stats[0]), ref, 'zero overlap')
    assert pairs[0, 0] == pairs[0, 2] == 0 and pairs[0, 1] > 0 and not stats[0, 0].any() and not stats[0, 2].any() and not np.signbit(stats[0, [0, 2]]).any()
    sc, ov = RX.score(pairs[0], own[0], stats[0], 0.0)
    assert sc[0] == sc[2] == -np.inf and np.isfinite(sc[1]) and ov[0] == 0
