"""-m gpu: the rigid merge of rows of the state pools (ops.volume_merge_, ivx_volume_merge_fwd, the MERGE instantiation of csrc/volume_warp.hip)
against the numpy reference of its definition (tests/ref_volume_merge.py): merged voxels within the derived bound for a general motion between
grids of different origins, every other voxel untouched (unmerged destination voxels pre-set to NaN / -1, canaries in the rows no sample names,
read-only sources), an empty destination as the bits of ops.volume_warp, the identity on a dyadic grid as the bits of torch's add, count
saturation, a NaN cell under a zero-weight corner, forgetting, and samples and pools (own transforms, origins and alphas; one pool as source and
destination; a shared source row; more samples than one launch carries).  Grids, voxel sizes and source states are the warp tests'."""
import numpy as np
import pytest
import torch

import ref_volume_merge as RM
import ref_volume_warp as RW
from test_gpu_volume_warp import GRIDS, VS, DY_VS, CANARY_F, CANARY_I, _origin, _dyadic_origin, _src

pytestmark = pytest.mark.gpu
IDS = lambda v: str(v).replace(' ', '')      # noqa: E731


@pytest.fixture(scope='module')
def ops():
    from imvoxelnet_amd import _lib, ops
    _lib.lib()
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    return ops


def _bits(a):
    return a.view(np.int32)


def _merge(ops, dst, src, rows, src_rows, Ts, od, os_, alpha, vs=VS, forget=0.0, check=True):
    """Reference, then device.  dst / src: host pools (sum, wsum, count) of valid states; src None: the destination pools are their own source.
    Per sample the reference merge of the two rows; then, in the destination pools that go to the device, every unmerged voxel of a named row is
    pre-set to NaN sums, NaN weight and count -1 and every row that no sample names (and none reads) carries canaries.  After the call: those
    bits are where they were, the sources are unchanged, and (check) each named row passes RM.check_row.  -> (host pools after, refs, worst ratio)."""
    B, same = len(rows), src is None
    od, os_ = np.broadcast_to(np.asarray(od, np.float32), (B, 3)), np.broadcast_to(np.asarray(os_, np.float32), (B, 3))
    al = [alpha] * B if isinstance(alpha, float) else list(alpha)
    spool = dst if same else src
    refs = [RM.merge_grid([a[rows[b]] for a in dst], [a[src_rows[b]] for a in spool], vs, od[b], os_[b], Ts[b], al[b], forget) for b in range(B)]
    before = [a.copy() for a in dst]
    for b in range(B):
        un = ~refs[b]['merged']
        before[0][rows[b]][un], before[1][rows[b]][un], before[2][rows[b]][un] = np.nan, np.nan, -1
    quiet = [r for r in range(len(dst[0])) if r not in rows and not (same and r in src_rows)]
    for r in quiet:
        before[0][r], before[1][r], before[2][r] = CANARY_F, CANARY_F, CANARY_I
    dev = tuple(torch.from_numpy(a).cuda() for a in before)
    sdev = dev if same else tuple(torch.from_numpy(a).cuda() for a in src)
    keep = [t.clone() for t in sdev]
    out = ops.volume_merge_(*dev, rows, sdev, src_rows, Ts, od, os_, vs, alpha=alpha, forget_below=forget)
    assert all(o is d for o, d in zip(out, dev))
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in dev]
    for r in (src_rows if same else range(len(src[0]))):
        for t, k in zip(sdev, keep):
            assert torch.equal(t[r].view(torch.int32), k[r].view(torch.int32)), f'source row {r} is read only'
    for r in quiet:
        for g, b4 in zip(got, before):
            assert np.array_equal(_bits(g[r]), _bits(b4[r])), f'row {r} is named by no sample'
    worst = 0.0
    if check:
        for b in range(B):
            worst = max(worst, *RM.check_row([g[rows[b]] for g in got], refs[b], [a[rows[b]] for a in before], f'sample {b}: row {src_rows[b]} -> {rows[b]}'))
    return got, refs, worst


@pytest.mark.parametrize('dims,C', GRIDS, ids=IDS)
def test_general_motion_within_the_bound_and_nothing_else_written(ops, dims, C):
    """A rotation about all three axes plus a fractional translation, a source grid whose origin differs by 0.05, alpha = 0.37, source row 1 of 3
    into destination row 2 of 4; the source has its random 15 % unseen plus an unseen slab, so every class of voxel exists: outside, eight corners
    read, fewer than eight read, inside but source unseen, merged."""
    src, dst, o = _src(3, dims, C, 110 + C), _src(4, dims, C, 120 + C), _origin(dims)
    for a in src:
        a[1][:max(1, dims[0] // 3)] = 0
    T = RW.rigid(0.23, 0.04, -0.03, (0.11, -0.07, 0.05))
    got, (ref,), _ = _merge(ops, dst, src, [2], [1], [T], o, o + np.float32(0.05), 0.37)
    n_read, inside, merged = ref['read'].sum(-1), ref['inside'], ref['merged']
    classes = dict(outside=int((~inside).sum()), eight=int((n_read == 8).sum()), fewer=int((inside & (n_read < 8)).sum()),
                   unseen=int((inside & ~merged).sum()), merged=int(merged.sum()))
    print(f'{dims} C={C}: {classes}; smallest positive W_s {ref["Ws"][merged].min():.4f}')
    assert all(v > 0 for v in classes.values()), classes
    assert np.isnan(got[0][2][~merged]).all() and np.isnan(got[1][2][~merged]).all() and (got[2][2][~merged] == -1).all()
    assert np.isfinite(got[0][2][merged]).all() and np.isfinite(got[1][2][merged]).all()


@pytest.mark.parametrize('dims,C', GRIDS, ids=IDS)
def test_an_empty_destination_takes_the_bits_of_the_warp(ops, dims, C):
    """All-zero destination row, alpha = 1, equal origins: the row after the merge is, bit for bit, what ops.volume_warp writes for the same source,
    transform and forget_below -- without a threshold and with one in the widest gap of the reference's W'."""
    src, o = _src(2, dims, C, 130 + C), _origin(dims)
    T = RW.rigid(0.3, 0.02, 0.01, (0.06, 0.04, 0.02))
    warped = RW.warp_grid(*(a[1] for a in src), VS, o, T)['W']
    w = np.sort(warped[warped > 0])
    lo, hi = len(w) // 4, 3 * len(w) // 4
    gap = lo + int(np.argmax(np.diff(w[lo:hi])))
    fb = float(np.float32((w[gap] + w[gap + 1]) / 2))
    S, W, c = (torch.from_numpy(a).cuda() for a in src)
    for forget in (0.0, fb):
        RW.warp_grid(*(a[1] for a in src), VS, o, T, forget_below=forget)     # (asserts that the forget decision is robust)
        dst = tuple(torch.zeros_like(t[:1]) for t in (S, W, c))
        ops.volume_merge_(*dst, [0], (S, W, c), [1], [T], o, o, VS, alpha=1.0, forget_below=forget)
        out = tuple(torch.full_like(t[:1], -3) for t in (S, W, c))
        ops.volume_warp(S, W, c, [1], [T], o[None], VS, out=out, out_rows=[0], forget_below=forget)
        for name, d, w_ in zip(('sum', 'wsum', 'count'), dst, out):
            assert torch.equal(d.view(torch.int32), w_.view(torch.int32)), (name, forget)
        assert (dst[1] > 0).sum() >= 10
        if forget:
            assert ((out[1].cpu().numpy()[0] == 0) & (warped > 0)).sum() >= 5, 'the threshold forgets some voxels'


@pytest.mark.parametrize('dims,C', GRIDS, ids=IDS)
@pytest.mark.parametrize('alpha', [1.0, 0.5])
def test_identity_on_the_dyadic_grid_is_the_plain_sum(ops, dims, C, alpha):
    """M = I, equal origins, dyadic voxel sizes and an origin on their lattice: one corner of weight 1 per voxel, so the merged voxels hold the bits
    of torch's S_d + S_s (alpha = 1) or S_d + 0.5 * S_s (alpha = 0.5; the product is exact), the weight sum likewise, the counts add, and where the
    source is unseen the destination keeps its bits."""
    src, dst, o = _src(1, dims, C, 140 + C), _src(1, dims, C, 150 + C), _dyadic_origin(dims)
    got, (ref,), _ = _merge(ops, dst, src, [0], [0], [np.eye(4)], o, o, alpha, vs=DY_VS, check=False)
    seen = src[1][0] > 0
    assert np.array_equal(ref['merged'], seen) and seen.any() and (~seen).any() and (ref['read'].sum(-1) == 1).all()
    Sd, Wd, Ss, Ws = (torch.from_numpy(a[0]).cuda() for a in (dst[0], dst[1], src[0], src[1]))
    want_S, want_W = (Sd + Ss, Wd + Ws) if alpha == 1.0 else (Sd + 0.5 * Ss, Wd + 0.5 * Ws)
    assert np.array_equal(_bits(got[0][0][seen]), _bits(want_S.cpu().numpy()[seen]))
    assert np.array_equal(_bits(got[1][0][seen]), _bits(want_W.cpu().numpy()[seen]))
    assert np.array_equal(got[2][0][seen], (dst[2][0] + src[2][0])[seen])
    assert np.isnan(got[0][0][~seen]).all() and np.isnan(got[1][0][~seen]).all() and (got[2][0][~seen] == -1).all()


def test_the_count_saturates(ops):
    """One cell with cnt_d = 2^31 - 2 and cnt_s = 5: the sum is formed in 64 bits and stops at 2^31 - 1; its neighbours add as usual."""
    dims, C = (6, 6, 3), 4
    src, dst, o = _src(1, dims, C, 161, unseen=0.0), _src(1, dims, C, 162, unseen=0.0), _dyadic_origin(dims)
    dst[2][0][2, 3, 1], src[2][0][2, 3, 1] = 2 ** 31 - 2, 5
    dst[2][0][2, 3, 2], src[2][0][2, 3, 2] = 2 ** 31 - 6, 5
    got, _, _ = _merge(ops, dst, src, [0], [0], [np.eye(4)], o, o, 1.0, vs=DY_VS)
    assert got[2][0][2, 3, 1] == 2 ** 31 - 1 and got[2][0][2, 3, 2] == 2 ** 31 - 1
    rest = np.ones(dims, bool)
    rest[2, 3, 1:] = False
    assert np.array_equal(got[2][0][rest], (dst[2][0] + src[2][0])[rest])


def test_a_nan_cell_under_a_zero_weight_corner_does_not_show(ops):
    """The half-voxel translation of the warp test on the dyadic grid: f = (0, 0.5, 0), two corners carry weight.  Source cells that are only ever a
    zero-weight corner hold NaN sums, NaN weight and a huge count: the merge equals the reference on the clean source."""
    dims, C = (7, 5, 6), 8
    src, dst, o = _src(1, dims, C, 171, unseen=0.0), _src(1, dims, C, 172), _dyadic_origin(dims)
    T = np.eye(4)
    T[:3, 3] = (1 * 0.25, 0.5 * 0.25, 0.0)
    ref = RM.merge_grid([a[0] for a in dst], [a[0] for a in src], DY_VS, o, o, T, 0.75)
    inside, i0, f = RM.grid_coords(dims, DY_VS, o, o, T)
    assert set(np.unique(f[inside])) == {0.0, 0.5} and (f[inside][:, 1] == 0.5).all()
    used = np.zeros(dims, bool)
    for c in range(8):
        idx = (i0 + np.array([c >> 2, (c >> 1) & 1, c & 1]))[ref['read'].reshape(-1, 8)[:, c]]
        used[idx[:, 0], idx[:, 1], idx[:, 2]] = True
    assert used.any() and (~used).any()
    dirty = [a.copy() for a in src]
    dirty[0][0][~used], dirty[1][0][~used], dirty[2][0][~used] = np.nan, np.nan, 2 ** 30
    before = [a.copy() for a in dst]
    dev = tuple(torch.from_numpy(a).cuda() for a in before)
    ops.volume_merge_(*dev, [0], tuple(torch.from_numpy(a).cuda() for a in dirty), [0], [T], o, o, DY_VS, alpha=0.75)
    got = [t.cpu().numpy()[0] for t in dev]
    RM.check_row(got, ref, [a[0] for a in before], 'NaN under zero-weight corners')
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and got[2].max() <= 16


@pytest.mark.parametrize('dims,C', GRIDS, ids=IDS)
def test_forget_below_on_robust_inputs(ops, dims, C):
    """The threshold sits midway in the widest gap of the reference's W' over the merged voxels (the reference asserts the margin): the merged
    voxels below it are unseen, all bits zero; every other voxel equals the call without a threshold bit for bit."""
    src, dst, o = _src(1, dims, C, 180 + C), _src(1, dims, C, 190 + C, unseen=0.5), _origin(dims)
    T = RW.rigid(0.3, 0.02, 0.01, (0.06, 0.04, 0.02))
    args = ([0], [0], [T], o, o + np.float32(0.03), 0.6)
    plain, (ref0,), _ = _merge(ops, dst, src, *args)
    m = ref0['merged']
    w = np.sort(ref0['W'][m])
    lo, hi = len(w) // 4, 3 * len(w) // 4                                     # ... of the middle half, so that both sides are populated
    gap = lo + int(np.argmax(np.diff(w[lo:hi])))
    fb = float(np.float32((w[gap] + w[gap + 1]) / 2))
    got, _, _ = _merge(ops, dst, src, *args, forget=fb)
    gone = m & (ref0['W'] < fb)
    assert gone.sum() >= 5 and (m & ~gone).sum() >= 5
    for g, p in zip(got, plain):
        assert not _bits(g[0][gone]).any() and np.array_equal(_bits(g[0][~gone]), _bits(p[0][~gone]))


def test_samples_and_pools(ops):
    """B = 2 with own transforms, origins and alphas between two pools; ONE pool as source and destination on disjoint rows (the batch case); two
    samples that read one source row."""
    dims, C = (9, 8, 4), 64
    src, dst = _src(3, dims, C, 200), _src(5, dims, C, 201)
    o = np.stack([_origin(dims), _origin(dims) + np.float32(0.05)])
    os_ = np.stack([_origin(dims) - np.float32(0.02), _origin(dims)])
    Ts = [RW.rigid(0.2, t=(0.1, 0, 0.02)), RW.rigid(-0.35, 0.03, 0.0, (-0.08, 0.12, 0))]
    _merge(ops, dst, src, [1, 3], [2, 0], Ts, o, os_, [0.8, 1.7])
    _merge(ops, dst, None, [1, 3], [2, 0], Ts, o, os_, [0.8, 1.7])
    _merge(ops, dst, None, [4, 0], [2, 2], Ts, o, os_, [1.0, 0.25])
    _merge(ops, dst, src, [0, 4], [1, 1], Ts, o, os_, [1.0, 0.25])


def test_more_samples_than_one_launch_carries(ops):
    """35 samples on the (6, 6, 3) grid at C = 4: rows, transforms, origins and alphas travel by value, 32 per launch, so this call is chunked."""
    dims, C, B = (6, 6, 3), 4, 35
    src, dst, o = _src(B, dims, C, 210), _src(B + 2, dims, C, 211), _origin(dims)
    src_rows, rows = [(r * 12) % B for r in range(B)], [(r * 3 + 1) % (B + 2) for r in range(B)]
    assert len(set(src_rows)) == B and len(set(rows)) == B
    # (a step of 0.011, not the warp test's 0.01: sample 17 turns by nothing, and 0.17 + 0.01 lands within rounding of a whole voxel of the source
    # grid, where a corner weight of 1e-7 would make W_s > 0 a matter of the last bit; the reference asserts that no input is that close)
    Ts = [RW.rigid(0.05 * (b - 17), t=(0.011 * b, -0.02 * (b % 5), 0.0)) for b in range(B)]
    od =np.stack([o + np.float32(0.01 * (b % 4)) for b in range(B)])
    os_ = np.stack([o + np.float32(0.01 * (b % 3)) for b in range(B)])
    _, _, worst = _merge(ops, dst, src, rows, src_rows, Ts, od, os_, [0.5 + 0.05 * b for b in range(B)])
    print(f'35 samples: worst |got - ref| / bound {worst:.3f}')
