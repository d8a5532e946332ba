"""-m gpu: ops.view_coverage (ivx_view_coverage_fwd) against the numpy reference of tests/ref_view_coverage.py, with exact ==.

Grids: the 7x6x5 dyadic scene of ref_unproject (N = 210: less than one workgroup, a partial wave) and 13x11x9 with a voxel size of 0.14
(N = 1287: six workgroups' worth of voxels and a ragged tail, non-dyadic numbers, so that the LDS combine, the cross-workgroup atomics and the
roundings of the chain are exercised); the larger grid also runs with IVX_COVERAGE_WGS=6, which leaves two workgroups per sample to walk the
stride loop three times each.  Candidates V = 1, 3 and 70 (more than one wave's worth) in ragged lists with -1 in the middle of a row, B = 3
samples on rows [2, 0, 1] of R = 3 pools, all four state kinds (counts in {0,1,2} with ties at fresh_below = 2, weight sums with exact ties, NaN
and 0, a mask with a byte other than 1), with and without the maps of ref_unproject_maps (a dyadic depth with a dyadic gate, a general weight
map with its blockers).  The inputs are shown to be non-degenerate on the reference before any device call.  The seen counts equal the lift's
own mask over that single view, and a reused out= buffer does not accumulate."""
import functools

import numpy as np
import pytest
import torch

import ref_unproject as R
import ref_unproject_maps as RM
import ref_view_coverage as RC

pytestmark = pytest.mark.gpu

FHW = (R.FH, R.FW)
ROWS = [2, 0, 1]
S_POOL = 11                                   # slots 0 .. 8 hold views, 9 and 10 hold NaN and are never listed
GRIDS = {
    'dyadic': dict(n_voxels=R.N_VOXELS, voxel_size=R.VOXEL_SIZE, new_origin=[R.NEW_ORIGIN, R.NEW_ORIGIN_2, R.NEW_ORIGIN], crop=[R.CROP, R.CROP_2, (4, 7)]),
    'ragged': dict(n_voxels=(13, 11, 9), voxel_size=(0.14, 0.14, 0.14), new_origin=[(0.6, -0.77, -0.38), (0.35, -0.5, -0.13), (0.62, -0.75, -0.4)],
                   crop=[R.CROP, R.CROP_2, (4, 7)]),
}
FRESH_BELOW = {RC.NONE: 1.0, RC.COUNT: 2.0, RC.WSUM: 0.75, RC.MASK: 1.0}
KINDS = {'none': RC.NONE, 'count': RC.COUNT, 'wsum': RC.WSUM, 'mask': RC.MASK}


@functools.lru_cache(maxsize=None)
def _proj_pool():
    """[S_POOL,3,4] fp32: the three dyadic views, then six views whose translations are moved by non-dyadic amounts; the last two slots are NaN."""
    base = R.dyadic_proj().astype(np.float64)
    P = [base[v] for v in range(3)]
    rng = np.random.default_rng(17)
    for i in range(6):
        R_, t = R.EXTRINSICS[i % 3]
        t = np.asarray(t, np.float64) + rng.uniform(-0.07, 0.07, 3)
        P.append(R.K @ np.concatenate([R_, t[:, None]], 1))
    P += [np.full((3, 4), np.nan)] * 2
    return np.stack(P).astype(np.float32)


def _lists(V):
    """B = 3 ragged lists, the longest of V entries, with a -1 in the middle of a row wherever a row is long enough to have a middle."""
    if V == 1:
        return [[4], [0], [-1]]
    if V == 3:
        return [[2, -1, 7], [1], [5, 3]]
    a = [(5 * i + 1) % 9 for i in range(70)]
    b = [(2 * i + 3) % 9 for i in range(33)]
    c = [(7 * i) % 9 for i in range(65)]
    a[35], b[16], c[64], c[0] = -1, -1, -1, -1
    return [a, b, c]


@functools.lru_cache(maxsize=None)
def _state(grid, kind):
    """[3, N] of the kind's dtype (None for an empty scene): every row differs, and every value class the definition names is present."""
    N = int(np.prod(GRIDS[grid]['n_voxels']))
    rng = np.random.default_rng(100 + N)
    if kind == RC.NONE:
        return None
    if kind == RC.COUNT:
        return rng.integers(0, 3, (3, N)).astype(np.int32)
    if kind == RC.WSUM:
        s = rng.choice(np.array([0.0, 0.5, 0.75, np.nextafter(np.float32(0.75), np.float32(0)), 1.5, np.nan], np.float32), (3, N))
        assert (s == np.float32(0.75)).any() and np.isnan(s).any() and (s == 0).any()
        return s
    return rng.choice(np.array([0, 1, 1, 7], np.uint8), (3, N))


@functools.lru_cache(maxsize=None)
def _maps(with_maps):
    if not with_maps:
        return {}
    return dict(pixel_weight=RM.general_weight_map(V=S_POOL), depth=RM.dyadic_depth(V=S_POOL), gate=RM.GATE)


@functools.lru_cache(maxsize=None)
def _reference(grid, V, kind, with_maps):
    g = GRIDS[grid]
    return RC.coverage_lists(_proj_pool(), _lists(V), ROWS, g['n_voxels'], g['voxel_size'], g['new_origin'], g['crop'], FHW, _state(grid, kind), kind,
                             FRESH_BELOW[kind], **_maps(with_maps))


@functools.lru_cache(maxsize=None)
def _non_degenerate():
    """On the reference alone: every unpadded candidate sees something; every state kind has a case with 0 < fresh < seen; the maps drop at
    least one voxel that was seen and keep at least one, per candidate."""
    for grid in GRIDS:
        for V in (1, 3, 70):
            lists = _lists(V)
            for kind in KINDS.values():
                plain, gated = _reference(grid, V, kind, False), _reference(grid, V, kind, True)
                between = 0
                for b, l in enumerate(lists):
                    for i, s in enumerate(l):
                        if s == -1:
                            assert not plain[b, i].any() and not gated[b, i].any()
                            continue
                        assert plain[b, i, 0] > 0, (grid, V, b, i, s)
                        assert 0 < gated[b, i, 0] < plain[b, i, 0], (grid, V, b, i, s, 'the maps must drop some seen voxels and keep some')
                        between += 0 < plain[b, i, 1] < plain[b, i, 0]
                    assert not plain[b, len(l):].any()
                if kind == RC.NONE:
                    assert np.array_equal(plain[..., 0], plain[..., 1])
                else:
                    assert between > 0, (grid, V, kind)
    return True


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


def _run(grid, V, kind, with_maps, out=None):
    from imvoxelnet_amd import ops
    g = GRIDS[grid]
    st = _state(grid, kind)
    maps = _maps(with_maps)
    return ops.view_coverage(_dev(_proj_pool()), _lists(V), ROWS, _dev(np.asarray(g['new_origin'], np.float32)), _dev(np.asarray(g['crop'], np.int32)),
                             g['voxel_size'], g['n_voxels'], FHW, None if st is None else _dev(st.reshape((3,) + tuple(g['n_voxels']))), FRESH_BELOW[kind],
                             None if not maps else _dev(maps['pixel_weight']), None if not maps else _dev(maps['depth']), maps.get('gate'), out=out)


@pytest.fixture(scope='module', autouse=True)
def _device():
    from imvoxelnet_amd import _lib
    _lib.lib()
    assert _non_degenerate()
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'


@pytest.mark.parametrize('with_maps', [False, True], ids=['plain', 'maps'])
@pytest.mark.parametrize('kind', list(KINDS), ids=list(KINDS))
@pytest.mark.parametrize('V', [1, 3, 70])
@pytest.mark.parametrize('grid', list(GRIDS))
def test_counts_equal_the_reference(grid, V, kind, with_maps):
    ref = _reference(grid, V, KINDS[kind], with_maps)
    got = _run(grid, V, KINDS[kind], with_maps)
    assert got.dtype == torch.int32 and tuple(got.shape) == ref.shape and got.is_cuda
    got = got.cpu().numpy().astype(np.int64)
    print(grid, V, kind, with_maps, 'seen', got[..., 0].sum(), 'fresh', got[..., 1].sum())
    assert np.array_equal(got, ref)


@pytest.mark.parametrize('with_maps', [False, True], ids=['plain', 'maps'])
@pytest.mark.parametrize('kind', ['count', 'wsum'])
def test_stride_loop_gives_the_same_counts(monkeypatch, kind, with_maps):
    """Two workgroups per sample (IVX_COVERAGE_WGS=6 for B = 3) walk the six voxel blocks of the 13x11x9 grid, three each."""
    monkeypatch.setenv('IVX_COVERAGE_WGS', '6')
    got = _run('ragged', 70, KINDS[kind], with_maps).cpu().numpy().astype(np.int64)
    assert np.array_equal(got, _reference('ragged', 70, KINDS[kind], with_maps))
    monkeypatch.setenv('IVX_COVERAGE_WGS', '1')      # one workgroup per sample walks all six
    got = _run('ragged', 3, KINDS[kind], with_maps).cpu().numpy().astype(np.int64)
    assert np.array_equal(got, _reference('ragged', 3, KINDS[kind], with_maps))


def test_a_reused_out_buffer_does_not_accumulate():
    out = torch.full((3, 70, 2), 12345, dtype=torch.int32, device='cuda')
    ref = _reference('ragged', 70, RC.WSUM, True)
    for _ in range(2):
        assert _run('ragged', 70, RC.WSUM, True, out=out) is out
        assert np.array_equal(out.cpu().numpy().astype(np.int64), ref)


@pytest.mark.parametrize('with_maps', [False, True], ids=['plain', 'maps'])
@pytest.mark.parametrize('grid', list(GRIDS))
def test_seen_equals_the_lifts_own_mask(grid, with_maps):
    """out[..., 0] of every (sample, slot) equals valid.sum() of ops.backproject_mapped_mean_ over that single view with unit weight and the same
    maps: the header the coverage kernel takes its chain from and the lift's own statement of it decide alike on the device."""
    from imvoxelnet_amd import ops
    g = GRIDS[grid]
    X, Y, Z = g['n_voxels']
    maps = _maps(with_maps)
    proj, no, crop = _dev(_proj_pool()), _dev(np.asarray(g['new_origin'], np.float32)), _dev(np.asarray(g['crop'], np.int32))
    pw, dp = (None if not maps else _dev(maps[k]) for k in ('pixel_weight', 'depth'))
    feat = torch.randn(S_POOL, 1, R.FH, R.FW, 4, generator=torch.Generator().manual_seed(3)).cuda()
    lists = [list(range(9))] * 3
    cov = ops.view_coverage(proj, lists, [0, 1, 2], no, crop, g['voxel_size'], g['n_voxels'], FHW, None, 1.0, pw, dp, maps.get('gate')).cpu().numpy()
    vol = torch.empty((3, X, Y, Z, 4), device='cuda')
    valid = torch.empty((3, X, Y, Z), device='cuda', dtype=torch.uint8)
    for s in range(9):
        ops.backproject_mapped_mean_(feat, proj, [[s]] * 3, None, [0, 1, 2], no, crop, g['voxel_size'], vol, valid, pixel_weight=pw, depth=dp,
                                     gate=maps.get('gate', (float('inf'), float('inf'))))
        lift = valid.view(3, -1).sum(1).cpu().numpy()
        assert np.array_equal(cov[:, s, 0], lift) and (lift > 0).all(), (s, cov[:, s, 0], lift)
    assert np.array_equal(cov[..., 0], cov[..., 1]), 'an empty scene: every seen voxel is fresh'
