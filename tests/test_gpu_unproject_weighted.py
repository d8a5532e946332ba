"""-m gpu: the weighted listed lift (ops.backproject_weighted_accum_ / _mean_ / volume_wmean, ivx_backproject_weighted_fwd, the WEIGHTED forms of
csrc/backproject.hip) on the dyadic scene of tests/ref_unproject.py: bit for bit against the unweighted listed lift where the definition says so
(unit weights, guarded weights, power-of-two scales, a sample that adds nothing), and against the fp64 reference of tests/ref_unproject_weighted.py
within the bound counted there (general weights, fading, forgetting).  Every state / output buffer starts as NaN / garbage / sentinels."""
import functools

import numpy as np
import pytest
import torch

import ref_unproject as R
import ref_unproject_weighted as RW

pytestmark = pytest.mark.gpu

GARBAGE = 0x7f7f7f7f
NV = R.N_VOXELS
N = NV[0] * NV[1] * NV[2]
S_POOL = 8
PERM = [5, 2, 7, 0, 3, 6]          # view v of sample b sits in slot PERM[b * 3 + v]; slots 1 and 4 stay NaN
ROWS = [3, 1]                      # sample b owns row ROWS[b] of R = 4; rows 0 and 2 are named by nobody
NROWS = 4
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope='module')
def ia():
    import imvoxelnet_amd
    from imvoxelnet_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    return imvoxelnet_amd


def slot(b, v):
    return PERM[b * 3 + v]


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _scenes():
    s0, s1 = R.dyadic_scene(R.NEW_ORIGIN, R.CROP), R.dyadic_scene(R.NEW_ORIGIN_2, R.CROP_2)
    ok = R.valid_views(s0['xf'], s0['yf'], s0['d'], s0['hc'], s0['wc'])
    # non-vacuous: the voxels view 0 sees and view 1 does not fade alone, the common ones keep growing, some are never seen
    assert (int((ok[0] & ~ok[1]).sum()), int((ok[0] & ok[1]).sum()), int((~ok.any(0)).sum())) == (131, 73, 6)
    assert R.scene_classes(s0)['counts'] == [6, 110, 82, 12]
    return s0, s1


@functools.lru_cache(maxsize=None)
def _inputs(Cn, bf16):
    """The six maps in scattered slots of a NaN pool [S,1,FH,FW,C], the projection pool, new_origin [2,3], crop [2,2], and the host maps
    [2,3,FH,FW,C] (fp32 values; bf16-representable when bf16)."""
    s0, s1 = _scenes()
    host = torch.randn(2, 3, R.FH, R.FW, Cn, generator=torch.Generator().manual_seed(2000 + Cn))
    if bf16:
        host = host.bfloat16().float()
    dtype = BF16 if bf16 else F32
    pool = torch.full((S_POOL, 1, R.FH, R.FW, Cn), float('nan'), dtype=dtype, device='cuda')
    ppool = torch.full((S_POOL, 3, 4), float('nan'), device='cuda')
    idx = torch.tensor(PERM, device='cuda')
    pool[idx] = host.reshape(6, 1, R.FH, R.FW, Cn).to(dtype).cuda()
    ppool[idx] = torch.from_numpy(np.concatenate([s0['proj'], s1['proj']])).cuda()
    no = torch.from_numpy(np.stack([s0['new_origin'], s1['new_origin']])).cuda().contiguous()
    crop = torch.from_numpy(np.stack([s0['crop'], s1['crop']])).cuda().contiguous()
    return pool, ppool, no, crop, host.numpy()


def _state(Cn, dtype=F32, rows=NROWS):
    dev = 'cuda'
    return dict(sum=torch.full((rows,) + NV + (Cn,), float('nan'), device=dev), wsum=torch.full((rows,) + NV, float('nan'), device=dev),
                count=torch.full((rows,) + NV, GARBAGE, device=dev, dtype=torch.int32), mean=torch.full((rows,) + NV + (Cn,), -7.0, device=dev, dtype=dtype),
                valid=torch.full((rows,) + NV, 7, device=dev, dtype=torch.uint8))


def _is_sentinel(st, r):
    ok = bool(torch.isnan(st['sum'][r]).all()) and bool((st['count'][r] == GARBAGE).all()) and bool((st['mean'][r].float() == -7.0).all()) and bool((st['valid'][r] == 7).all())
    return ok and ('wsum' not in st or bool(torch.isnan(st['wsum'][r]).all()))


def _slot_weights(per_view, fill=1.0):
    """Per-view weights (the same three for both samples) -> the host list of per-slot weights [S]."""
    w = [fill] * S_POOL
    for b in range(2):
        for v, x in enumerate(per_view):
            w[slot(b, v)] = x
    return w


def _accum(ops, z, st, lists, weights, first, decay=None, emit=True, sampling='nearest', forget_below=0.0):
    pool, ppool, no, crop, _ = z
    return ops.backproject_weighted_accum_(pool, ppool, lists, weights, ROWS, first, decay, no, crop, R.VOXEL_SIZE, st['sum'], st['wsum'], st['count'],
                                           st['mean'] if emit else None, st['valid'] if emit else None, forget_below=forget_below, sampling=sampling)


def _np(t):
    return t.float().cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------ 1. unit weights
UNIT = [(c, d, s) for c in (8, 68, 520) for d in (F32, BF16) for s in ('nearest', 'bilinear')]
# the views of the two samples, in their own order (ragged: three and two), cut into chunks
VIEWS = [[0, 1, 2], [2, 0]]


def _chunk_lists(chunks):
    out, v0 = [], 0
    for n in chunks:
        out.append([[slot(b, v) for v in VIEWS[b][v0:v0 + n]] for b in range(2)])     # sample 1 runs out of views: an empty list adds nothing
        v0 += n
    return out


@pytest.mark.parametrize('Cn,dtype,sampling', UNIT, ids=[f'C{c}-{str(d).split(".")[1]}-{s}' for c, d, s in UNIT])
def test_unit_weights_are_the_unweighted_listed_lift_bit_for_bit(ia, Cn, dtype, sampling):
    """Weights 1, decay 1, forget_below 0: volume, count, mean_out and valid are ops.backproject_lists_accum_ / _mean_'s bits, chunk by chunk, for
    chunks (1,1,1), (2,1), (3); wsum == count.float(); rows 0 and 2 keep their sentinels.  Unit weights are given as NULL, as a host list and as a
    device list; the decay as NULL and as ones.  C = 8: two lanes per voxel (three views: a second, partial projection round); C = 68: 17 chunks on
    32 lanes; C = 520: 130 chunks on 64 lanes, three per lane, the last partial."""
    from imvoxelnet_amd import ops
    z = _inputs(Cn, dtype == BF16)
    pool, ppool, no, crop, _ = z
    forms = [(None, None), ([1.0] * S_POOL, [1.0, 1.0]), (torch.ones(S_POOL, device='cuda'), None)]
    for (weights, decay), chunks in zip(forms, [(3,), (1, 1, 1), (2, 1)]):
        st, ref = _state(Cn, dtype), _state(Cn, dtype)
        del ref['wsum']
        for i, lists in enumerate(_chunk_lists(chunks)):
            out = _accum(ops, z, st, lists, weights, [i == 0] * 2, decay, sampling=sampling)
            assert out[0] is st['sum'] and out[1] is st['wsum'] and out[2] is st['count']
            ops.backproject_lists_accum_(pool, ppool, lists, ROWS, [i == 0] * 2, no, crop, R.VOXEL_SIZE, ref['sum'], ref['count'], ref['mean'], ref['valid'],
                                         sampling=sampling)
            for k in ref:
                assert _same_bits(st[k], ref[k]), (chunks, i, k)
            for r in ROWS:
                assert torch.equal(st['wsum'][r], st['count'][r].float()), (chunks, i, r)
        assert _is_sentinel(st, 0) and _is_sentinel(st, 2), 'a row that no sample names was written'
        assert int(st['count'][ROWS[0]].max()) == 3 and int(st['count'][ROWS[1]].max()) == 2 and not bool(torch.isnan(st['sum'][ROWS]).any())
        # the mean mode on the same ragged lists
        lists = _chunk_lists((3,))[0]
        mt, mref = _state(Cn, dtype), _state(Cn, dtype)
        vol, valid = ops.backproject_weighted_mean_(pool, ppool, lists, weights, ROWS, no, crop, R.VOXEL_SIZE, mt['mean'], mt['valid'], sampling=sampling)
        ops.backproject_lists_mean_(pool, ppool, lists, ROWS, no, crop, R.VOXEL_SIZE, mref['mean'], mref['valid'], sampling=sampling)
        assert vol is mt['mean'] and valid.dtype == torch.bool
        assert _same_bits(mt['mean'], mref['mean']) and _same_bits(mt['valid'], mref['valid'])
        assert _same_bits(mt['mean'][ROWS], st['mean'][ROWS]), 'the mean mode is the accumulate mode from zero'
        assert bool((mt['mean'][0].float() == -7.0).all()) and bool((mt['valid'][2] == 7).all())


# ------------------------------------------------------------------ 2. guarded weights
@pytest.mark.parametrize('Cn,sampling', [(8, 'nearest'), (68, 'bilinear')])
def test_a_zero_nan_negative_or_infinite_weight_is_the_view_not_listed(ia, Cn, sampling):
    """Weights (1, w, 1) with w = 0, NaN, -1, +inf (a device list: the kernel's guard; 0 also as a host list) against the lists without view 1, in
    both modes, bit for bit."""
    from imvoxelnet_amd import ops
    z = _inputs(Cn, False)
    pool, ppool, no, crop, _ = z
    full = [[slot(b, v) for v in (0, 1, 2)] for b in range(2)]
    short = [[slot(b, v) for v in (0, 2)] for b in range(2)]
    ref = _state(Cn)
    _accum(ops, z, ref, short, None, [True, True], sampling=sampling)
    mref = _state(Cn)
    ops.backproject_weighted_mean_(pool, ppool, short, None, ROWS, no, crop, R.VOXEL_SIZE, mref['mean'], mref['valid'], sampling=sampling)
    all3 = _state(Cn)
    _accum(ops, z, all3, full, None, [True, True], sampling=sampling)
    assert not _same_bits(all3['mean'], ref['mean']), 'dropping view 1 must change the mean'
    for w in (0.0, float('nan'), -1.0, float('inf'), 'host 0'):
        weights = _slot_weights((1.0, 0.0, 1.0)) if w == 'host 0' else torch.tensor(_slot_weights((1.0, w, 1.0)), device='cuda')
        st = _state(Cn)
        _accum(ops, z, st, full, weights, [True, True], sampling=sampling)
        for k in st:
            assert _same_bits(st[k], ref[k]), (w, k)
        mt = _state(Cn)
        ops.backproject_weighted_mean_(pool, ppool, full, weights, ROWS, no, crop, R.VOXEL_SIZE, mt['mean'], mt['valid'], sampling=sampling)
        assert _same_bits(mt['mean'], mref['mean']) and _same_bits(mt['valid'], mref['valid']), w


# ------------------------------------------------------------------ 3. power-of-two scale
@pytest.mark.parametrize('Cn,dtype,sampling', [(8, F32, 'nearest'), (8, BF16, 'bilinear'), (68, F32, 'bilinear'), (520, BF16, 'nearest')])
def test_weights_times_four_keep_the_mean_and_scale_the_sums_exactly(ia, Cn, dtype, sampling):
    from imvoxelnet_amd import ops
    z = _inputs(Cn, dtype == BF16)
    pool, ppool, no, crop, _ = z
    full = [[slot(b, v) for v in (0, 1, 2)] for b in range(2)]
    a, b = _state(Cn, dtype), _state(Cn, dtype)
    _accum(ops, z, a, full, _slot_weights((0.5, 2.0, 1.0)), [True, True], sampling=sampling)
    _accum(ops, z, b, full, _slot_weights((2.0, 8.0, 4.0)), [True, True], sampling=sampling)
    assert _same_bits(a['mean'], b['mean']) and _same_bits(a['valid'], b['valid']) and _same_bits(a['count'], b['count'])
    assert _same_bits(a['sum'][ROWS] * 4, b['sum'][ROWS]) and _same_bits(a['wsum'][ROWS] * 4, b['wsum'][ROWS])
    unit = _state(Cn, dtype)
    _accum(ops, z, unit, full, None, [True, True], sampling=sampling)
    assert not _same_bits(a['mean'], unit['mean']), 'the weights must matter'
    ma, mb = _state(Cn, dtype), _state(Cn, dtype)
    ops.backproject_weighted_mean_(pool, ppool, full, _slot_weights((0.5, 2.0, 1.0)), ROWS, no, crop, R.VOXEL_SIZE, ma['mean'], ma['valid'], sampling=sampling)
    ops.backproject_weighted_mean_(pool, ppool, full, _slot_weights((2.0, 8.0, 4.0)), ROWS, no, crop, R.VOXEL_SIZE, mb['mean'], mb['valid'], sampling=sampling)
    assert _same_bits(ma['mean'], mb['mean']) and _same_bits(ma['valid'], mb['valid']) and _same_bits(ma['mean'], a['mean'])


# ------------------------------------------------------------------ 4. - 6. against the fp64 reference
def _refs(host, bilinear, forget_below=0.0):
    return [RW.WeightedReference(host[b], sc['xf'], sc['yf'], sc['d'], sc['hc'], sc['wc'], bilinear, forget_below) for b, sc in enumerate(_scenes())]


def _check(name, st, refs, K, bf16, sums=True, wsum_ulps=None):
    """Rows ROWS of the state against the two samples' references: valid and count exact, the mean (and the sums) within the bound."""
    worst = 0.0
    for b, r in enumerate(ROWS):
        ref = refs[b].result()
        assert np.array_equal(st['valid'][r].cpu().numpy().reshape(-1).astype(bool), ref['valid']), (name, b, 'valid')
        assert np.array_equal(st['count'][r].cpu().numpy().reshape(-1), ref['count']), (name, b, 'count')
        got = _np(st['mean'][r]).reshape(ref['mean'].shape)
        diff, bnd = np.abs(got - ref['mean']), RW.bound(ref['A'], K, ref['mean'], bf16)
        ratio = float((diff / bnd).max())
        print(f'{name} sample {b}: worst |mean - ref| / bound = {ratio:.3f} (K = {K})')
        assert np.all(diff <= bnd), (name, b, 'mean', ratio)
        worst = max(worst, ratio)
        if sums:
            gs = _np(st['sum'][r]).reshape(ref['S'].shape)
            ds, bs = np.abs(gs - ref['S']), RW.bound(ref['M'], K)
            print(f'{name} sample {b}: worst |sum - ref| / bound = {float((ds / bs).max()):.3f}')
            assert np.all(ds <= bs), (name, b, 'sum')
        gw = _np(st['wsum'][r]).reshape(-1)
        if wsum_ulps is None:
            assert np.array_equal(gw, ref['W']), (name, b, 'wsum')
        else:
            ulp = np.spacing(ref['W'].astype(np.float32)).astype(np.float64)
            assert np.all(np.abs(gw - ref['W']) <= wsum_ulps * ulp), (name, b, 'wsum')
    return worst


GENERAL = [(8, False, 'nearest'), (8, False, 'bilinear'), (68, False, 'bilinear'), (520, False, 'nearest'), (8, True, 'bilinear'), (68, True, 'nearest')]


@pytest.mark.parametrize('Cn,bf16,sampling', GENERAL, ids=[f'C{c}-{"bf16" if b else "f32"}-{s}' for c, b, s in GENERAL])
def test_general_weights_within_the_fp64_bound(ia, Cn, bf16, sampling):
    """Weights (0.3, 1.7, 0.9): |mean - ref| <= K * 2^-24 * A + 2^-126 with K = ref_unproject_weighted.k_weighted(3 views, no fade) and no further
    margin (bf16: plus the store term); valid and count exact; wsum within 2 ulp (three additions, the first exact).  Both modes."""
    from imvoxelnet_amd import ops
    z = _inputs(Cn, bf16)
    pool, ppool, no, crop, host = z
    bil = sampling == 'bilinear'
    w = (0.3, 1.7, 0.9)
    full = [[slot(b, v) for v in (0, 1, 2)] for b in range(2)]
    refs = _refs(host, bil)
    for ref in refs:
        ref.tick([0, 1, 2], w, first=True)
    K = RW.k_weighted(3, 0, bil)
    st = _state(Cn, BF16 if bf16 else F32)
    _accum(ops, z, st, full, _slot_weights(w), [True, True], sampling=sampling)
    _check(f'general C{Cn} {sampling}', st, refs, K, bf16, wsum_ulps=2)
    mt = _state(Cn, BF16 if bf16 else F32)
    ops.backproject_weighted_mean_(pool, ppool, full, _slot_weights(w), ROWS, no, crop, R.VOXEL_SIZE, mt['mean'], mt['valid'], sampling=sampling)
    assert _same_bits(mt['mean'][ROWS], st['mean'][ROWS]) and _same_bits(mt['valid'][ROWS], st['valid'][ROWS]) and _is_sentinel(st, 0) and _is_sentinel(st, 2)


@pytest.mark.parametrize('Cn,sampling', [(8, 'nearest'), (68, 'bilinear'), (520, 'nearest')])
def test_fading_and_forgetting_exact_bookkeeping(ia, Cn, sampling):
    """lambda = 0.5, forget_below = 0.25, unit weights: tick 0 adds view 0, ticks 1 - 3 add view 1 only.  After every tick wsum, count and valid equal
    the reference EXACTLY (every W is a small dyadic number).  The 131 voxels of sample 0 that view 0 sees and view 1 does not carry W = 1, 0.5,
    0.25 and at tick 3 are forgotten: S == +0 bit for bit, W == 0, count == 0, valid == 0.  Sums and means stay within the bound."""
    from imvoxelnet_amd import ops
    z = _inputs(Cn, False)
    host = z[4]
    bil = sampling == 'bilinear'
    refs = _refs(host, bil, forget_below=0.25)
    s0 = _scenes()[0]
    ok = R.valid_views(s0['xf'], s0['yf'], s0['d'], s0['hc'], s0['wc'])
    only0 = torch.from_numpy(ok[0] & ~ok[1]).cuda()
    assert int(only0.sum()) == 131
    st = _state(Cn)
    r0 = ROWS[0]
    for t, expect in enumerate((1.0, 0.5, 0.25, 0.0)):
        v = 0 if t == 0 else 1
        _accum(ops, z, st, [[slot(b, v)] for b in range(2)], None, [t == 0] * 2, [0.5, 0.5], sampling=sampling, forget_below=0.25)
        for ref in refs:
            ref.tick([v], [1.0], decay=0.5, first=t == 0)
        _check(f'fade tick {t} C{Cn} {sampling}', st, refs, RW.k_weighted(t + 1, t, bil), False)
        w = st['wsum'][r0].reshape(-1)[only0]
        assert bool((w == expect).all()), (t, w.unique())
    gone = lambda k: st[k][r0].reshape(N, -1)[only0]          # noqa: E731
    assert not bool(_bits(gone('sum')).any()), 'a forgotten sum is +0, bit for bit'
    assert not bool(_bits(gone('wsum')).any()) and not bool(gone('count').any()) and not bool(gone('valid').any()) and not bool(_bits(gone('mean')).any())
    both = torch.from_numpy(ok[0] & ok[1]).cuda()
    assert bool((st['wsum'][r0].reshape(-1)[both] == 1.875).all()) and bool((st['count'][r0].reshape(-1)[both] == 4).all())


FADE = [(8, False, 'nearest'), (8, False, 'bilinear'), (68, False, 'bilinear'), (68, True, 'nearest'), (520, False, 'bilinear')]


@pytest.mark.parametrize('Cn,bf16,sampling', FADE, ids=[f'C{c}-{"bf16" if b else "f32"}-{s}' for c, b, s in FADE])
def test_fading_with_general_weights_within_the_fp64_bound(ia, Cn, bf16, sampling):
    """lambda = 0.75, weights (1.5, 0.5, 1.25), forget_below = 0, three ticks (views (0,1,2), then (1,2), then (0)): mean and sums within the bound
    with K = k_weighted(views counted so far, fading ticks so far); valid and count exact; wsum within one ulp per rounding."""
    from imvoxelnet_amd import ops
    z = _inputs(Cn, bf16)
    host = z[4]
    bil = sampling == 'bilinear'
    w = (1.5, 0.5, 1.25)
    refs = _refs(host, bil)
    st = _state(Cn, BF16 if bf16 else F32)
    n = 0
    for t, views in enumerate(((0, 1, 2), (1, 2), (0,))):
        n += len(views)
        _accum(ops, z, st, [[slot(b, v) for v in views] for b in range(2)], _slot_weights(w), [t == 0] * 2, [0.75, 0.75], sampling=sampling)
        for ref in refs:
            ref.tick(list(views), [w[v] for v in views], decay=0.75, first=t == 0)
        _check(f'fade-general tick {t} C{Cn} {sampling}', st, refs, RW.k_weighted(n, t, bil), bf16, wsum_ulps=n + t)
    assert _is_sentinel(st, 0) and _is_sentinel(st, 2)


# ------------------------------------------------------------------ 7. a sample that adds nothing
def test_a_sample_that_adds_nothing(ia):
    """A row of -1 slots.  decay 1 (NULL or ones), first 0: the row is stored back with every bit pattern intact (random words in sum, wsum and
    count: NaNs, negative weight sums, denormals).  decay 0.75: the faded row, S * 0.75 and W * 0.75 rounded once, the count as it was.  first 1:
    the zero state.  The other sample of the launch is served as usual."""
    from imvoxelnet_amd import ops
    Cn = 8
    z = _inputs(Cn, False)
    lists = [[-1, -1, -1], [slot(1, v) for v in (0, 1, 2)]]
    ref = _state(Cn)
    _accum(ops, z, ref, [[slot(0, 0)], lists[1]], None, [True, True])
    g = torch.Generator().manual_seed(77)
    words = lambda shape: torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=g, dtype=torch.int64).to(torch.int32).cuda()          # noqa: E731
    for decay in (None, [1.0, 1.0]):
        st = _state(Cn)
        r0 = ROWS[0]
        st['sum'][r0] = words(NV + (Cn,)).view(torch.float32)
        st['wsum'][r0] = words(NV).view(torch.float32)
        st['count'][r0] = words(NV)
        assert bool(torch.isnan(st['wsum'][r0]).any()) or bool((st['wsum'][r0] < 0).any())
        before = {k: v.clone() for k, v in st.items()}
        _accum(ops, z, st, lists, None, [False, True], decay, emit=False)
        for k in st:
            assert _same_bits(st[k][[0, 2, 3]], before[k][[0, 2, 3]]), (decay, k)          # row 3 adds nothing, rows 0 and 2 are not named
        assert _same_bits(st['sum'][ROWS[1]], ref['sum'][ROWS[1]]) and _same_bits(st['wsum'][ROWS[1]], ref['wsum'][ROWS[1]])
    # the faded row
    st = _state(Cn)
    st['sum'][r0] = torch.randn(NV + (Cn,), generator=torch.Generator().manual_seed(5)).cuda()
    st['wsum'][r0] = torch.rand(NV, generator=torch.Generator().manual_seed(6)).cuda() + 0.5
    st['count'][r0] = 3
    before = {k: v.clone() for k, v in st.items()}
    _accum(ops, z, st, lists, None, [False, True], [0.75, 1.0])
    cpu = lambda t: t.cpu()          # noqa: E731  (the expected values by the host's IEEE fp32 product and quotient)
    assert _same_bits(cpu(st['sum'][r0]), cpu(before['sum'][r0]) * 0.75) and _same_bits(cpu(st['wsum'][r0]), cpu(before['wsum'][r0]) * 0.75)
    assert torch.equal(st['count'][r0], before['count'][r0]) and not _same_bits(st['sum'][r0], before['sum'][r0])
    assert _same_bits(cpu(st['mean'][r0]), cpu(st['sum'][r0]) / cpu(st['wsum'][r0])[..., None]) and bool((st['valid'][r0] == 1).all())
    # first: the zero state
    _accum(ops, z, st, lists, None, [True, True], [0.75, 1.0])
    for k in ('sum', 'wsum', 'count', 'mean', 'valid'):
        assert not bool(_bits(st[k][r0]).any()), k
    assert _is_sentinel(st, 0) and _is_sentinel(st, 2)


# ------------------------------------------------------------------ 8. volume_wmean
@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16'])
def test_volume_wmean_is_the_mean_out_of_the_same_state(ia, dtype):
    from imvoxelnet_amd import ops
    Cn = 68
    z = _inputs(Cn, dtype == BF16)
    st = _state(Cn, dtype)
    w = _slot_weights((0.3, 1.7, 0.9))
    _accum(ops, z, st, [[slot(b, v) for v in (0, 1)] for b in range(2)], w, [True, True])
    _accum(ops, z, st, [[slot(b, 2)] for b in range(2)], w, [False, False], [0.75, 0.5], forget_below=0.5)
    quiet = _state(Cn, dtype)
    _accum(ops, z, quiet, [[slot(b, v) for v in (0, 1)] for b in range(2)], w, [True, True], emit=False)
    _accum(ops, z, quiet, [[slot(b, 2)] for b in range(2)], w, [False, False], [0.75, 0.5], emit=False, forget_below=0.5)
    assert bool((quiet['mean'].float() == -7.0).all()) and bool((quiet['valid'] == 7).all()), 'emit=False writes no mean'
    for k in ('sum', 'wsum', 'count'):
        assert _same_bits(quiet[k], st[k]), k
    for r in ROWS:
        before = quiet['sum'][r].clone()
        mean, valid = ops.volume_wmean(quiet['sum'][r:r + 1], quiet['wsum'][r:r + 1], dtype)
        assert mean.dtype == dtype and valid.dtype == torch.bool
        assert _same_bits(mean[0], st['mean'][r]) and torch.equal(valid[0], st['valid'][r].bool()) and _same_bits(quiet['sum'][r], before)
        assert 0 < int(valid.sum()) < valid.numel()
        out, vout = torch.full_like(mean, 3.0), torch.full((1,) + NV, 9, device='cuda', dtype=torch.uint8)
        m2, _ = ops.volume_wmean(quiet['sum'][r:r + 1], quiet['wsum'][r:r + 1], dtype, out=out, valid_out=vout)
        assert m2 is out and _same_bits(out, mean) and torch.equal(vout.bool(), valid)
