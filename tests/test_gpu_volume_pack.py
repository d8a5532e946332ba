"""-m gpu: ivx_volume_pack_fwd / ivx_volume_unpack_fwd through ops.volume_pack_count / volume_pack / volume_unpack_ against the numpy restatement of
tests/ref_volume_pack.py.  Named rows sit between guard rows that no call may touch.  F32 records and restored rows are compared with == on the
words: the sums of kept voxels are random bit patterns (NaNs, -0, denormals among them) and zero elsewhere, the precondition of the exact round
trip.  Shapes: (7,5,6) with C = 4, 8, 72, 256 (two lanes per record, one wave per record, a C/4 that does not divide 64), a grid whose voxel count
is neither a multiple of the wave nor of the 256-voxel chunk, and one with more chunks (279) than the scan workgroup has lanes (256).  The bf16
round trip is held to (2^-8 + 2^-22) |S| in fp64."""
import ctypes

import numpy as np
import pytest
import torch

import ref_volume_pack as RP

pytestmark = pytest.mark.gpu

SHAPES = [((7, 5, 6), 4), ((7, 5, 6), 8), ((7, 5, 6), 72), ((7, 5, 6), 256), ((37, 29, 3), 8), ((67, 41, 26), 4)]
PATTERNS = ['none', 'all', 'first', 'last', 'alternate', 'third', 'chunks', 'mixed']


@pytest.fixture(scope='module')
def ops():
    from imvoxelnet_amd import _lib, ops
    _lib.lib()
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    return ops


def _pools(seed, dims, C, patterns, wsum=True, raw=True):
    """R = 2 B + 1 rows: row 2 b + 1 holds a state of patterns[b], the rows between are guards that hold evidence too -> host (S, count, wsum), rows."""
    rng = np.random.default_rng(seed)
    R = 2 * len(patterns) + 1
    S, cnt, ws = RP.random_state(rng, dims, C, 'third', wsum, R, raw)
    rows = [2 * b + 1 for b in range(len(patterns))]
    for r, p in zip(rows, patterns):
        s1, c1, w1 = RP.random_state(rng, dims, C, p, wsum, 1, raw)
        S[r], cnt[r] = s1[0], c1[0]
        if wsum:
            ws[r] = w1[0]
    return (S, cnt, ws), rows


def _dev(host):
    return tuple(None if a is None else torch.from_numpy(a).cuda() for a in host)


def _same(t, a):
    """A device tensor against a host array, on the words."""
    return np.array_equal(RP.words(t.cpu().numpy()), RP.words(a))


def _junk(host, seed):
    """Pools of the same shapes filled with other evidence: an unpack must write every voxel of a named row."""
    rng = np.random.default_rng(seed)
    return tuple(None if a is None else rng.integers(1, 2 ** 31 - 1, a.shape, dtype=np.int64).astype(np.int32).view(a.dtype) for a in host)


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('dims,C', SHAPES)
def test_f32_pack_and_unpack_against_the_reference(ops, dims, C, pattern):
    """Two rows of different n in one call, named out of order: the records are the reference's, the count-only form agrees, the pools are read
    only; unpacked into pools full of other evidence the named rows are the originals bit for bit and the guard rows keep every bit."""
    host, rows = _pools(sum(dims) * 1000 + C * 10 + PATTERNS.index(pattern), dims, C, [pattern, 'third'])
    dev = _dev(host)
    order = [rows[1], rows[0]]
    ref = [RP.pack(host[0][r], host[1][r], host[2][r]) for r in order]
    assert ops.volume_pack_count(dev[0], dev[1], order, dev[2]) == [len(x[0]) for x in ref]
    recs = ops.volume_pack(dev[0], dev[1], order, dev[2])
    for got, want in zip(recs, ref):
        assert got[0].dtype == torch.int32 and got[1].dtype == torch.float32 and tuple(got[1].shape) == (len(want[0]), C)
        assert all(_same(g, w) for g, w in zip(got, want)), (dims, C, pattern)
    assert all(_same(t, a) for t, a in zip(dev, host)), 'the source pools are read only'
    junk = _junk(host, 3)
    out = _dev(junk)
    assert ops.volume_unpack_(out[0], out[1], order, recs, out[2])[0] is out[0]
    for r in range(host[0].shape[0]):
        want = host if r in rows else junk
        assert all(_same(t[r], a[r]) for t, a in zip(out, want)), ('named row' if r in rows else 'guard row', r)
    # host records (numpy, as a snapshot holds them) restore the same rows
    out2 = _dev(junk)
    ops.volume_unpack_(out2[0], out2[1], order, ref, out2[2])
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out, out2))


@pytest.mark.parametrize('dims,C', [((7, 5, 6), 8), ((37, 29, 3), 72)])
def test_a_state_without_a_weight_sum(ops, dims, C):
    host, rows = _pools(11, dims, C, ['third', 'alternate', 'none'], wsum=False)
    dev = _dev(host)
    recs = ops.volume_pack(dev[0], dev[1], rows, None)
    for got, r in zip(recs, rows):
        want = RP.pack(host[0][r], host[1][r])
        assert got[2] is None and want[2] is None and all(_same(g, w) for g, w in zip(got[:2] + got[3:], want[:2] + want[3:]))
    assert recs[2][0].numel() == 0 and tuple(recs[2][1].shape) == (0, C)
    junk = _junk(host, 4)
    out = _dev(junk)
    assert len(ops.volume_unpack_(out[0], out[1], rows, recs)) == 2
    for r in range(host[0].shape[0]):
        want = host if r in rows else junk
        assert _same(out[0][r], want[0][r]) and _same(out[1][r], want[1][r]), r


def test_all_unseen_rows_launch_no_second_call(ops, monkeypatch):
    host, rows = _pools(12, (7, 5, 6), 8, ['none', 'none'])
    dev = _dev(host)
    calls = []
    real = ops._pack_call
    monkeypatch.setattr(ops, '_pack_call', lambda *a: calls.append(a[6]) or real(*a))
    recs = ops.volume_pack(dev[0], dev[1], rows, dev[2])
    assert calls == [0] and all(r[0].numel() == 0 and tuple(r[1].shape) == (0, 8) and r[2].numel() == 0 and r[3].numel() == 0 for r in recs)
    out = _dev(_junk(host, 5))
    ops.volume_unpack_(out[0], out[1], rows, recs, out[2])                     # no records at all: the named rows become unseen
    assert all(not bool(t[r].view(torch.int32).any()) for t in out for r in rows)


def test_more_than_32_rows_in_one_call(ops):
    """35 samples: two launches' worth of rows passed by value, each with its own pattern and n."""
    pats = [PATTERNS[b % len(PATTERNS)] for b in range(35)]
    host, rows = _pools(13, (7, 5, 6), 4, pats)
    dev = _dev(host)
    recs = ops.volume_pack(dev[0], dev[1], rows, dev[2])
    ns = [int(r[0].numel()) for r in recs]
    assert len(set(ns)) > 4 and ops.volume_pack_count(dev[0], dev[1], rows, dev[2]) == ns
    for got, r in zip(recs, rows):
        assert all(_same(g, w) for g, w in zip(got, RP.pack(host[0][r], host[1][r], host[2][r]))), r
    junk = _junk(host, 6)
    out = _dev(junk)
    ops.volume_unpack_(out[0], out[1], rows, recs, out[2])
    for r in range(host[0].shape[0]):
        want = host if r in rows else junk
        assert all(_same(t[r], a[r]) for t, a in zip(out, want)), r


@pytest.mark.parametrize('dims,C', [((7, 5, 6), 8), ((67, 41, 26), 4)])
def test_cap_smaller_than_n(ops, dims, C):
    """The entry itself with a cap below the largest n: n_out is the true count, a sample fills at most its cap records -- the next sample's region
    holds that sample's own records -- and nothing at or beyond min(n, cap) of any output is written (outputs pre-filled with a guard word, and one
    guard sample behind the last)."""
    from imvoxelnet_amd import _lib
    L = _lib.lib()
    host, rows = _pools(14, dims, C, ['all', 'first', 'third', 'none'])
    dev = _dev(host)
    ref = [RP.pack(host[0][r], host[1][r], host[2][r]) for r in rows]
    ns = [len(x[0]) for x in ref]
    cap = ns[2] - 3                                                            # below 'all' and 'third', above 'first' and 'none'
    assert ns[0] > cap and ns[2] > cap > ns[1] > ns[3] == 0
    B, (R, X, Y, Z) = len(rows), host[1].shape
    G = 0x5a5a5a5a
    fill = lambda shape, dt: torch.full(shape, G, dtype=torch.int32, device='cuda').view(dt)      # noqa: E731
    index, payload, wout, cout = fill((B + 1, cap), torch.int32), fill((B + 1, cap, C), torch.float32), fill((B + 1, cap), torch.float32), fill((B + 1, cap), torch.int32)
    n_out = torch.full((B + 1,), G, dtype=torch.int32, device='cuda')
    scratch = torch.empty((L.ivx_volume_pack_scratch_bytes(B, X, Y, Z) // 4,), dtype=torch.int32, device='cuda')
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                # noqa: E731
    rc = L.ivx_volume_pack_fwd(B, (ctypes.c_int32 * B)(*rows), R, X, Y, Z, C, p(dev[0]), p(dev[1]), p(dev[2]), 0, cap, p(index), p(payload), p(wout), p(cout),
                               p(n_out), p(scratch), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.ivx_last_error()
    torch.cuda.synchronize()
    assert n_out.tolist() == ns + [G], 'n_out is the true count, also beyond cap'
    for b, want in enumerate(ref):
        k = min(ns[b], cap)
        for got, w in zip((index, payload, wout, cout), want):
            assert _same(got[b, :k], w[:k]), ('records below cap', b)
            assert bool((got[b, k:].view(torch.int32) == G).all()), ('nothing at or beyond min(n, cap) is written', b)
    assert all(bool((t[B].view(torch.int32) == G).all()) for t in (index, payload, wout, cout))


@pytest.mark.parametrize('wsum', [True, False])
@pytest.mark.parametrize('dims,C', [((7, 5, 6), 8), ((7, 5, 6), 72), ((37, 29, 3), 256)])
def test_bf16_round_trip_within_the_derived_bound(ops, dims, C, wsum):
    """Every |S / den| lies in bf16's normal range: the restored sums lie within (2^-8 + 2^-22) |S| of the originals in fp64, count and weight sum
    come back bit for bit, unseen voxels come back all zero, and the payload is within one bf16 step of the fp64 reference's."""
    host, rows = _pools(15, dims, C, ['third', 'all'], wsum=wsum, raw=False)
    dev = _dev(host)
    recs = ops.volume_pack(dev[0], dev[1], rows, dev[2], dtype=torch.bfloat16)
    junk = _junk(host, 7)
    out = _dev(junk)
    ops.volume_unpack_(out[0], out[1], rows, recs, out[2])
    worst = 0.0
    for got, r in zip(recs, rows):
        want = RP.pack(host[0][r], host[1][r], None if not wsum else host[2][r], bf16=True)
        assert got[1].dtype == torch.bfloat16 and _same(got[0], want[0]) and _same(got[3], want[3]) and (not wsum or _same(got[2], want[2]))
        words = got[1].view(torch.int16).cpu().numpy().view(np.uint16)
        assert np.abs(words.astype(np.int64) - want[1].astype(np.int64)).max() <= 1, 'one division in fp32, then one rounding: at most a step from the fp64 mean'
        S, S2 = host[0][r].astype(np.float64), out[0][r].cpu().numpy().astype(np.float64)
        seen = (host[1][r] != 0)[..., None] & np.ones(C, bool)
        assert np.isfinite(S2).all() and not S2[~seen].any() and (np.abs(S[seen]) >= 2.0 ** -100).all()
        frac = (np.abs(S2 - S)[seen] / (RP.BF16_BOUND * np.abs(S[seen]))).max()
        worst = max(worst, float(frac))
        assert _same(out[1][r], host[1][r]) and (not wsum or _same(out[2][r], host[2][r]))
    print(f'bf16 round trip {dims} C={C} wsum={wsum}: worst |S\' - S| / ((2^-8 + 2^-22) |S|) = {worst:.4f}')
    assert 0 < worst <= 1.0
    for r in range(host[0].shape[0]):
        if r not in rows:
            assert all(a is None or _same(t[r], a[r]) for t, a in zip(out, junk)), ('guard row', r)
