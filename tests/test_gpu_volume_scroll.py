"""-m gpu: the in-place voxel scroll of the state pools (ops.volume_scroll_, ivx_volume_scroll_fwd, csrc/volume_scroll.hip) against the numpy
reference of its definition (tests/ref_volume_scroll.py), bit for bit: small hard shapes with every kind of shift, the in-place hazard at a size
with many workgroups in flight, and the geometry -- a lifted state scrolled by s is the same views lifted at the scrolled origin."""
import numpy as np
import pytest
import torch

import ref_volume_scroll as RS
from helpers import load_npz, sub

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from imvoxelnet_amd import _lib, ops
    _lib.lib()
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    return ops


def _words(shape, seed):
    """Random int32 bit patterns: viewed as fp32 they hold NaNs with payloads, -0-like signs, infinities and denormals."""
    return torch.randint(-2 ** 31, 2 ** 31, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.int64).to(torch.int32)


def _pools(R, dims, C, seed, guard=1):
    """Host words of (sum [G+R+G,X,Y,Z,C], count, wsum): `guard` extra rows before and after the pools, which no call may touch."""
    n = R + 2 * guard
    return _words((n,) + dims + (C,), seed), _words((n,) + dims, seed + 1), _words((n,) + dims, seed + 2)


def _run(ops, host, R, rows, shifts, with_wsum=True, guard=1):
    """Upload, scroll rows of the middle R rows in place, download as words: (sum, count, wsum) including the guard rows."""
    dev = [h.cuda() for h in host]
    vol, cnt, ws = dev[0].view(torch.float32)[guard:guard + R], dev[1][guard:guard + R], dev[2].view(torch.float32)[guard:guard + R]
    assert vol.is_contiguous() and cnt.is_contiguous() and ws.is_contiguous()
    out = ops.volume_scroll_(vol, cnt, rows, shifts, ws if with_wsum else None)
    assert out[0] is vol and out[1] is cnt
    torch.cuda.synchronize()
    return [d.cpu() for d in dev]


def _expect(host, R, rows, shifts, with_wsum=True, guard=1):
    out = []
    for f, h in enumerate(host):
        a = h.numpy().copy()
        if f < 2 or with_wsum:
            a[guard:guard + R] = RS.scroll_rows(a[guard:guard + R], rows, shifts)
        out.append(torch.from_numpy(a))
    return out


DIMS = (7, 5, 6)
SHIFTS = [tuple(sign * m if a == ax else 0 for a in range(3)) for ax, L in enumerate(DIMS) for m in (1, L - 1, L, L + 3) for sign in (1, -1)] + [(2, -1, 3), (0, 0, 0)]
assert len(SHIFTS) == 26 and len(set(SHIFTS)) == 26


@pytest.mark.parametrize('C', [4, 8, 72])
def test_small_hard_shapes_equal_the_reference_bit_for_bit(ops, C):
    """Grid 7 x 5 x 6, C in {4, 8, 72}: 1, 2 and 18 sixteen-byte chunks per voxel, and line counts (30 .. 756 for the sums, 30 .. 42 for the words) that
    are no multiple of the workgroup.  R = 3, rows [2, 0] with different shifts per row: each axis alone at +-1, +-(L-1), +-L, +-(L+3), a three-axis shift and
    the zero shift.  Sums, count and wsum equal the reference on int views; row 1 and the guard rows around the pools keep every bit; without a weight sum
    the wsum buffer is not touched."""
    host = _pools(3, DIMS, C, 100 + C)
    assert bool(torch.isnan(host[0].view(torch.float32)).any()) and bool((host[0].view(torch.float32).abs() < 1e-38).any())
    for n, s in enumerate(SHIFTS):
        other = SHIFTS[(n + 7) % len(SHIFTS)]                              # row 0 takes another shift than row 2 (once the zero shift, once beside it)
        got, want = _run(ops, host, 3, [2, 0], [s, other]), _expect(host, 3, [2, 0], [s, other])
        for name, g, w, h in zip(('sum', 'count', 'wsum'), got, want, host):
            assert torch.equal(g, w), (name, s, other, int((g != w).sum()))
            assert torch.equal(g[2], h[2]) and torch.equal(g[0], h[0]) and torch.equal(g[4], h[4]), (name, s, 'row 1 and the guard rows keep their bits')
    for s in ((1, 0, 0), (0, -4, 0), (2, -1, 3), (0, 0, 9)):                # the form without a weight sum; one row alone with one triple
        got, want = _run(ops, host, 3, [1], s, with_wsum=False), _expect(host, 3, [1], [s], with_wsum=False)
        for name, g, w in zip(('sum', 'count', 'wsum'), got, want):
            assert torch.equal(g, w), (name, s)
        assert torch.equal(got[2], host[2])


def test_more_samples_than_one_launch_carries(ops):
    """70 rows of a 3 x 4 x 2 grid with 70 different shifts: the rows and shifts travel by value, 32 per launch, so this call is chunked."""
    R = 70
    host = _pools(R, (3, 4, 2), 4, 300)
    rows = [(r * 37) % R for r in range(R)]
    shifts = [((r % 7) - 3, (r % 5) - 2, (r % 3) - 1) for r in range(R)]
    assert len(set(rows)) == R
    got, want = _run(ops, host, R, rows, shifts), _expect(host, R, rows, shifts)
    for g, w in zip(got, want):
        assert torch.equal(g, w)


BIG = (40, 40, 16)


@pytest.fixture(scope='module')
def big_host():
    return _pools(2, BIG, 64, 500, guard=0)


@pytest.mark.parametrize('shift', [(1, 0, 0), (0, 1, 0), (0, 0, 1), (-3, 2, -5), (39, 0, 0)], ids=lambda s: '_'.join(map(str, s)))
def test_in_place_hazard_with_many_workgroups_in_flight(ops, big_host, shift):
    """The ScanNet-fast grid at C = 64 (6.5 MB per row; 10 240 .. 25 600 lines per pass of the sums): a lane that read what another step had already
    written would show here.  Row 1 moves, row 0 keeps its bits; a second run from the same start gives the same bits."""
    want = _expect(big_host, 2, [1], [shift], guard=0)
    first = _run(ops, big_host, 2, [1], [shift], guard=0)
    for name, g, w in zip(('sum', 'count', 'wsum'), first, want):
        assert torch.equal(g, w), (name, int((g != w).sum()))
    again = _run(ops, big_host, 2, [1], [shift], guard=0)
    for g, f in zip(again, first):
        assert torch.equal(g, f)


@pytest.mark.parametrize('shift', [(2, 0, 0), (0, -3, 0), (0, 0, 1), (-2, 1, -1), (3, -2, 2)], ids=lambda s: '_'.join(map(str, s)))
def test_scrolled_state_is_the_lift_at_the_scrolled_origin(ops, shift):
    """Geometry, exact by construction: voxel_size 0.25 and an origin on the 0.25 lattice (golden case B: two cameras, a 12 x 12 x 6 grid), so every
    i * vs + new_origin is exact in fp32 under both framings.  Lift random features at origin o, scroll by s: on the voxels that stayed inside, sum and
    count equal, bit for bit, the same views lifted at scrolled_origin(o, s, vs); the voxels that entered are zero."""
    from imvoxelnet_amd import scrolled_origin
    c = sub(load_npz('backproject_cases.npz'), 'B::')
    nv, vs, o = tuple(int(v) for v in c['n_voxels']), c['voxel_size'], c['origin']
    assert np.all(vs == 0.25) and np.all(np.mod(o, 0.25) == 0)
    P = torch.from_numpy(c['projection'])[None].cuda().contiguous()
    crop = torch.tensor([[int(c['img_shape'][0]) // 4, int(c['img_shape'][1]) // 4]], dtype=torch.int32).cuda()
    feat = torch.randn(2, 1, 24, 32, 8, generator=torch.Generator().manual_seed(77)).cuda()

    def lift(origin):
        new_origin = (torch.from_numpy(np.asarray(origin, np.float32)) - torch.tensor(nv) / 2. * torch.from_numpy(vs))[None].cuda().contiguous()
        vol = torch.full((1,) + nv + (8,), float('nan'), device='cuda')
        cnt = torch.full((1,) + nv, -5, device='cuda', dtype=torch.int32)
        ops.backproject_accum_(feat, P, new_origin, crop, vs, vol, cnt, True)
        return vol, cnt

    o2 = scrolled_origin(o, shift, vs)
    assert np.array_equal(o2, o + np.asarray(shift, np.float32) * 0.25)       # exact here: no rounding to argue about
    vol, cnt = lift(o)
    ops.volume_scroll_(vol, cnt, [0], [shift])
    vol2, cnt2 = lift(o2)
    inside = torch.from_numpy(RS.stayed_inside(nv, shift)).cuda()
    seen = int((cnt2[0][inside] > 0).sum())
    print('shift', shift, 'voxels that stayed inside:', int(inside.sum()), 'of them seen:', seen, 'entered and seen at the new origin:', int((cnt2[0][~inside] > 0).sum()))
    assert seen >= 50, 'the views must see the overlap for the test to mean anything'
    assert torch.equal(cnt[0][inside], cnt2[0][inside])
    assert torch.equal(vol[0][inside].view(torch.int32), vol2[0][inside].view(torch.int32))
    assert not bool(cnt[0][~inside].any()) and not bool(vol[0][~inside].view(torch.int32).any())
