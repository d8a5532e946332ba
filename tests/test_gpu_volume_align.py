"""-m gpu: the Gauss-Newton normal equations of a pose between rows of the state pools (ops.volume_align, ivx_volume_align_fwd, the ALIGN instantiation
of csrc/volume_match.hip) against the numpy reference of its definition (tests/ref_volume_align.py): pairs, used and own equal and the 31 statistics
within the derived bound, for 33 candidates (a call crosses the 32-per-launch chunk) between grids of unequal origins, two samples, rows of pools
of 3 and 2, the lattice step (2, 1, 3), a candidate that leaves half the grid outside and one wholly outside; pairs, own, dot, na, nb == those of
ops.volume_match; the identity on a dyadic grid with e == 0 and g == 0 exactly; NaN in the source sums wherever W == 0 leaves e, g, H bit-equal;
bit-equal answers from call to call and from any rows of any pools; all four pools read only; and one 64 x 64 x 65 row whose waves walk more than
one tile.  Each (grid, C) computes its pools, device answer and reference once."""
import functools

import numpy as np
import pytest
import torch

import ref_volume_align as RA
import ref_volume_warp as RW
from test_gpu_volume_warp import VS, DY_VS, _origin, _dyadic_origin, _src
from test_gpu_volume_match import _bits, _slabs

pytestmark = pytest.mark.gpu
IDS = lambda v: str(v).replace(' ', '')      # noqa: E731
GRIDS = [((7, 5, 6), 8), ((9, 8, 5), 64), ((6, 5, 4), 256), ((5, 4, 3), 4)]
K = 33
STEP = (2, 1, 3)


@pytest.fixture(scope='module')
def ops():
    from imvoxelnet_amd import _lib, ops
    _lib.lib()
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    return ops


def _pools(dims, C, seed, R_dst=3, R_src=2):
    return _slabs(_src(R_dst, dims, C, seed, unseen=0.0)[:2], _src(R_src, dims, C, seed + 1, unseen=0.0)[:2])


def _centre(dims, o, vs=VS):
    return (np.asarray(o, np.float64) + np.asarray(dims) / 2 * np.asarray(vs)).astype(np.float32)


def _candidates(dims, about, flip=1.0):
    """Candidate 0: a six-DoF pose; 1: leaves about half the grid outside; 2: wholly outside; 3 .. 32: small six-DoF poses, all different."""
    half = dims[0] / 2 * VS[0]
    out = [RW.rigid(0.05 * flip, 0.03, -0.02, (0.05, 0.03 * flip, 0.02), about),
           RW.rigid(0.02, -0.01 * flip, 0.015, (half, 0.02, -0.01), about),
           RW.rigid(0.1, t=(50.0, 0, 0))]
    for k in range(3, K):
        out.append(RW.rigid(0.012 * (k - 17) * flip + 0.003, 0.008 * (k % 5 - 2), 0.006 * (k % 3 - 1) * flip,
                            (0.007 * k - 0.1, 0.04 - 0.013 * (k % 7), 0.011 * (k % 4) - 0.01), about))
    return out


def _device(ops, dst, src, rows, src_rows, cands, about, od, os_, vs=VS, step=(1, 1, 1), match=False):
    """Upload (src None: the destination pools are their own source), align, check that no bit of any of the four pools changed -> host (pairs
    [B,K], used [B,K], own [B], stats [B,K,31]); match=True: also ops.volume_match's host (pairs, own, stats) on the same device pools."""
    dev = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in dst)
    sdev = dev if src is None else tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in src)
    keep = [_bits(t).clone() for t in dev + sdev]
    pairs, used, own, stats = ops.volume_align(*dev, rows, sdev, src_rows, cands, about, od, os_, vs, step)
    torch.cuda.synchronize()
    B, Kn = len(rows), len(cands[0])
    for t in (pairs, used):
        assert t.shape == (B, Kn) and t.dtype == torch.int64 and t.is_cuda
    assert own.shape == (B,) and own.dtype == torch.int64 and stats.shape == (B, Kn, 31) and stats.dtype == torch.float64 and stats.is_cuda
    got = tuple(t.cpu().numpy() for t in (pairs, used, own, stats))
    if match:
        got += (tuple(t.cpu().numpy() for t in ops.volume_match(*dev, rows, sdev, src_rows, cands, od, os_, vs, step)),)
    for t, k in zip(dev + sdev, keep):
        assert torch.equal(_bits(t), k), 'the pools are read only'
    return got


@functools.lru_cache(maxsize=None)
def _case(dims, C):
    """The shared inputs of one (grid, C): pools of 3 and 2 rows, two samples naming non-zero rows, unequal origins, 33 candidates each."""
    dst, src = _pools(dims, C, 500 + C)
    od = np.stack([_origin(dims), _origin(dims) + np.float32(0.02)])
    os_ = np.stack([_origin(dims) + np.float32(0.05), _origin(dims) - np.float32(0.03)])
    about = np.stack([_centre(dims, od[0]), _centre(dims, od[1])])
    cands = [_candidates(dims, about[0].astype(np.float64)), _candidates(dims, about[1].astype(np.float64), -1.0)]
    return dict(dst=dst, src=src, rows=[2, 1], src_rows=[1, 1], od=od, os=os_, about=about, cands=cands)


@functools.lru_cache(maxsize=None)
def _answers(dims, C, step):
    """-> (the device's host arrays with ops.volume_match's as the fifth, [the reference of sample 0, of sample 1]), computed once per (grid, C, step)."""
    from imvoxelnet_amd import ops
    c = _case(dims, C)
    got = _device(ops, c['dst'], c['src'], c['rows'], c['src_rows'], c['cands'], c['about'], c['od'], c['os'], step=step, match=True)
    refs = [RA.align_rows([a[c['rows'][b]] for a in c['dst']], [a[c['src_rows'][b]] for a in c['src']], VS, c['od'][b], c['os'][b], c['cands'][b],
                          c['about'][b], step) for b in range(2)]
    return got, refs


@pytest.mark.parametrize('step', [(1, 1, 1), STEP], ids=IDS)
@pytest.mark.parametrize('dims,C', GRIDS, ids=IDS)
def test_against_the_reference(ops, dims, C, step):
    """Counts equal the reference's, the 31 statistics lie within the derived bound (the worst ratios are printed), on every voxel and on the
    lattice (2, 1, 3).  Candidate 0 uses voxels and leaves some paired voxels unused; candidate 1 loses about half; candidate 2 is wholly outside
    and all its counts and statistics are +0."""
    got, refs = _answers(dims, C, step)
    for b in range(2):
        RA.check((got[0][b], got[1][b], got[2][b], got[3][b]), refs[b], f'{dims} C={C} step {step}, sample {b}, {K} candidates')
        pairs, used = refs[b]['pairs'], refs[b]['used']
        assert pairs[2] == 0 and used[2] == 0 and not got[3][b, 2].any() and not np.signbit(got[3][b, 2]).any()
        assert 0 < pairs[1] <= pairs[0] and (used <= pairs).all()
        if step == (1, 1, 1):
            assert 0 < used[0] < pairs[0] and pairs[1] < pairs[0] and 0 < used[1], (pairs[:3], used[:3])
    assert np.isfinite(got[3]).all()


@pytest.mark.parametrize('step', [(1, 1, 1), STEP], ids=IDS)
@pytest.mark.parametrize('dims,C', GRIDS, ids=IDS)
def test_match_parity(ops, dims, C, step):
    """pairs, own, dot, na, nb are ops.volume_match's on the same pools and candidates, with ==."""
    got, _ = _answers(dims, C, step)
    m_pairs, m_own, m_stats = got[4]
    assert np.array_equal(got[0], m_pairs) and np.array_equal(got[2], m_own)
    assert got[3][..., :3].tobytes() == m_stats.tobytes() and (m_pairs > 0).any()


@pytest.mark.parametrize('dims,C', GRIDS, ids=IDS)
def test_identity_on_the_dyadic_grid(ops, dims, C):
    """M = I, equal origins, dyadic voxel sizes and an origin on their lattice, a state against itself: b == a bit for bit, so e == 0 and g == 0
    exactly, while H is not zero; used counts the seen voxels whose eight forward corners are all in the grid and seen."""
    S, W, _ = _src(2, dims, C, 580 + C)
    o = _dyadic_origin(dims)
    about = _centre(dims, o, DY_VS)
    pairs, used, own, stats = _device(ops, (S, W), None, [1], [1], [[np.eye(4)]], about, o, o, vs=DY_VS)
    seen = W[1] > 0
    full = seen[:-1, :-1, :-1].copy()
    for c in range(1, 8):
        full &= seen[(c >> 2):seen.shape[0] - 1 + (c >> 2), ((c >> 1) & 1):seen.shape[1] - 1 + ((c >> 1) & 1), (c & 1):seen.shape[2] - 1 + (c & 1)]
    assert pairs[0, 0] == own[0] == int(seen.sum()) and used[0, 0] == int(full.sum()) > 0
    assert stats[0, 0, 3] == 0 and not stats[0, 0, 4:10].any() and stats[0, 0, 10] > 0 and stats[0, 0, 0] == stats[0, 0, 1] == stats[0, 0, 2] > 0
    ref = RA.align_rows((S[1], W[1]), (S[1], W[1]), DY_VS, o, o, [np.eye(4)], about)
    RA.check((pairs[0], used[0], own[0], stats[0]), ref, f'{dims} C={C}, identity')


def test_nan_where_the_source_is_unseen(ops):
    """NaN written into the source sums wherever W == 0 -- the unseen slab and scattered unseen voxels -- leaves used, e, g and H bit-equal to the
    clean run: a corner with W <= 0 makes its voxel unused, by selection."""
    dims, C = (9, 8, 5), 64
    c = _case(dims, C)
    src = [a.copy() for a in c['src']]
    hole = np.random.default_rng(7).random(src[1].shape) < 0.1
    src[0][hole], src[1][hole] = 0, 0
    cands = [c['cands'][0][:3], c['cands'][1][:3]]
    args = (c['rows'], c['src_rows'], cands, c['about'], c['od'], c['os'])
    clean = _device(ops, c['dst'], src, *args)
    dirty = [a.copy() for a in src]
    dirty[0][src[1] == 0] = np.nan
    assert np.isnan(dirty[0]).any()
    got = _device(ops, c['dst'], dirty, *args)
    assert np.array_equal(got[1], clean[1]) and (clean[1][:, 0] > 0).all() and (clean[1] < clean[0])[:, 0].all()
    assert got[3][..., 3:].tobytes() == clean[3][..., 3:].tobytes() and np.isfinite(got[3][..., 3:]).all()


def test_determinism_rows_and_pools(ops):
    """Two calls give bit-equal answers; the same two states in other rows of larger pools, beside other samples and with other candidates in the
    same call, give the same bits; and alone (B = 1, K = 1) the same bits again."""
    dims, C = (9, 8, 5), 64
    c = _case(dims, C)
    got, _ = _answers(dims, C, (1, 1, 1))
    again = _device(ops, c['dst'], c['src'], c['rows'], c['src_rows'], c['cands'], c['about'], c['od'], c['os'])
    for a, b in zip(got[:4], again):
        assert a.tobytes() == b.tobytes()
    rng = np.random.default_rng(541)
    big_d = [rng.uniform(0.5, 2, (6,) + a.shape[1:]).astype(np.float32) for a in c['dst']]
    big_s = [rng.uniform(0.5, 2, (5,) + a.shape[1:]).astype(np.float32) for a in c['src']]
    for a, b in zip(big_d, c['dst']):
        a[4] = b[2]
    for a, b in zip(big_s, c['src']):
        a[3] = b[1]
    Ts, other = c['cands'][0][:5], c['cands'][1][5:10]
    moved = _device(ops, big_d, big_s, [1, 4, 0], [2, 3, 0], [other, Ts, other], np.stack([c['about'][1], c['about'][0], c['about'][1]]),
                    np.stack([c['od'][1], c['od'][0], c['od'][1]]), np.stack([c['os'][1], c['os'][0], c['os'][0]]))
    for i in (0, 1, 3):
        assert moved[i][1].tobytes() == got[i][0, :5].tobytes(), i
    assert moved[2][1] == got[2][0]
    alone = _device(ops, c['dst'], c['src'], [2], [1], [[c['cands'][0][4]]], c['about'][0], c['od'][0], c['os'][0])
    for i in (0, 1, 3):
        assert alone[i][0, 0].tobytes() == got[i][0, 4].tobytes(), i


def test_a_wave_walks_more_than_one_tile(ops):
    """64 x 64 x 65 voxels at C = 4: tiles of 64 voxels, 4160 of them, more than the 4096 waves of a launch, so every wave walks two tiles.  One
    sample, one candidate, against the reference, and the match's numbers with ==.  Among 266240 points under a rotation some always lie within an
    fp32 rounding of a cell face, which the reference refuses; so the grid is dyadic and the candidate a translation by dyadic fractions of a voxel
    (the geometry chain is exact, f = (1/4, 1/2, 3/4) everywhere) -- the rotation columns of J, g and H do not depend on the candidate's kind."""
    dims, C = (64, 64, 65), 4
    dst, src = _slabs(_src(1, dims, C, 590, unseen=0.0)[:2], _src(1, dims, C, 591, unseen=0.0)[:2])
    od = _dyadic_origin(dims)
    about = _centre(dims, od, DY_VS)
    T = np.eye(4)
    T[:3, 3] = (0.0625, 0.125 + 0.25, 0.125)
    got = _device(ops, dst, src, [0], [0], [[T]], about, od, od + np.float32(0.25), vs=DY_VS, match=True)
    ref = RA.align_rows([a[0] for a in dst], [a[0] for a in src], DY_VS, od, od + np.float32(0.25), [T], about)
    RA.check((got[0][0], got[1][0], got[2][0], got[3][0]), ref, f'{dims} C={C}')
    assert ref['used'][0] > 100000 and got[3][0, :, :3].tobytes() == got[4][2][0].tobytes() and np.array_equal(got[0], got[4][0])
