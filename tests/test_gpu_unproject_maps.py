"""-m gpu: the weighted listed lift with pixel maps (ops.backproject_mapped_accum_ / _mean_, ivx_backproject_mapped_fwd, the MAPPED forms of
csrc/backproject.hip) on the dyadic scene of tests/ref_unproject.py, in the set-up of test_gpu_unproject_weighted (scattered slots of NaN pools,
rows [3, 1] of 4, sentinel-filled state): every property the header states bit for bit against ops.backproject_weighted_accum_ / _mean_, and
general maps with general view weights across chunked ticks with decay and forgetting against the fp64 reference of tests/ref_unproject_maps.py
within the bound counted there.  The maps' unlisted slots are NaN."""
import functools

import numpy as np
import pytest
import torch

import ref_unproject as R
import ref_unproject_maps as RM
import test_gpu_unproject_weighted as TW
from test_gpu_unproject_weighted import ia  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

F32, BF16, ROWS, S_POOL, slot = TW.F32, TW.BF16, TW.ROWS, TW.S_POOL, TW.slot
INF, NAN = float('inf'), float('nan')
FULL = [[slot(b, v) for v in (0, 1, 2)] for b in range(2)]
SHORT = [[slot(b, v) for v in (0, 2)] for b in range(2)]
WV = (0.3, 1.7, 0.9)


def _slot_maps(per_view):
    """Per-view maps [3,FH,FW] (the same three for both samples) -> the device pool [S,FH,FW] of per-slot maps; slots 1 and 4 stay NaN."""
    m = torch.full((S_POOL, R.FH, R.FW), NAN)
    for b in range(2):
        for v in range(3):
            m[slot(b, v)] = torch.from_numpy(np.asarray(per_view[v], np.float32))
    return m.cuda()


@functools.lru_cache(maxsize=None)
def _maps():
    """dict(pw, depth: the general maps of ref_unproject_maps, per view; ones; holes: a depth map of nothing but non-measurements), on the host."""
    holes = np.asarray(RM.HOLES, np.float32)[np.arange(3 * R.FH * R.FW) % 4].reshape(3, R.FH, R.FW)
    return dict(pw=RM.general_weight_map(), depth=RM.dyadic_depth(), ones=np.ones((3, R.FH, R.FW), np.float32), holes=holes)


def _accum(ops, z, st, lists, weights, first, decay=None, sampling='nearest', forget_below=0.0, **maps):
    pool, ppool, no, crop, _ = z
    return ops.backproject_mapped_accum_(pool, ppool, lists, weights, ROWS, first, decay, no, crop, R.VOXEL_SIZE, st['sum'], st['wsum'], st['count'], st['mean'],
                                         st['valid'], forget_below=forget_below, sampling=sampling, **maps)


def _mean(ops, z, st, lists, weights, sampling='nearest', **maps):
    pool, ppool, no, crop, _ = z
    return ops.backproject_mapped_mean_(pool, ppool, lists, weights, ROWS, no, crop, R.VOXEL_SIZE, st['mean'], st['valid'], sampling=sampling, **maps)


def _same_state(a, b, what):
    for k in a:
        assert TW._same_bits(a[k], b[k]), (what, k)


FORMS = [(8, F32, 'nearest'), (8, BF16, 'bilinear'), (68, F32, 'bilinear'), (68, BF16, 'nearest'), (520, F32, 'nearest'), (520, BF16, 'bilinear')]
IDS = [f'C{c}-{str(d).split(".")[1]}-{s}' for c, d, s in FORMS]


# ------------------------------------------------------------------ 1. no maps, neutral maps
@pytest.mark.parametrize('Cn,dtype,sampling', FORMS, ids=IDS)
def test_neutral_maps_are_the_weighted_lift_bit_for_bit(ia, Cn, dtype, sampling):
    """General view weights, two chunked ticks with decays (0.75, 0.5) and forget_below 0.5.  No maps; a pixel_weight of ones; a depth of nothing but
    non-measurements (0, NaN, -1, +inf) under the tightest gate (0, 0); the general depth map with behind = front = +inf; ones and holes together, as
    [S,1,FH,FW]: sum, wsum, count, mean and valid are ops.backproject_weighted_accum_'s bits after every tick, and the mean mode's are
    backproject_weighted_mean_'s.  Rows 0 and 2 keep their sentinels."""
    from imvoxelnet_amd import ops
    z = TW._inputs(Cn, dtype == BF16)
    pool, ppool, no, crop, _ = z
    w = TW._slot_weights(WV)
    ticks = [([[slot(b, v) for v in (0, 1)] for b in range(2)], [True, True]), ([[slot(b, 2)] for b in range(2)], [False, False])]
    ref = TW._state(Cn, dtype)
    refs = []
    for lists, first in ticks:
        TW._accum(ops, z, ref, lists, w, first, [0.75, 0.5], sampling=sampling, forget_below=0.5)
        refs.append({k: v.clone() for k, v in ref.items()})
    mref = TW._state(Cn, dtype)
    ops.backproject_weighted_mean_(pool, ppool, FULL, w, ROWS, no, crop, R.VOXEL_SIZE, mref['mean'], mref['valid'], sampling=sampling)
    m = _maps()
    ones, holes, depth = _slot_maps(m['ones']), _slot_maps(m['holes']), _slot_maps(m['depth'])
    neutral = dict(none=dict(), ones=dict(pixel_weight=ones), holes=dict(depth=holes, gate=(0.0, 0.0)), open_gate=dict(depth=depth, gate=(INF, INF)),
                   default_gate=dict(depth=depth), both=dict(pixel_weight=ones[:, None], depth=holes[:, None], gate=(0.0, 0.0)))
    for name, kw in neutral.items():
        st = TW._state(Cn, dtype)
        for (lists, first), want in zip(ticks, refs):
            out = _accum(ops, z, st, lists, w, first, [0.75, 0.5], sampling=sampling, forget_below=0.5, **kw)
            assert out[0] is st['sum'] and out[1] is st['wsum'] and out[2] is st['count']
            _same_state(st, want, name)
        assert TW._is_sentinel(st, 0) and TW._is_sentinel(st, 2), name
        mt = TW._state(Cn, dtype)
        vol, valid = _mean(ops, z, mt, FULL, w, sampling, **kw)
        assert vol is mt['mean'] and valid.dtype == torch.bool
        assert TW._same_bits(mt['mean'], mref['mean']) and TW._same_bits(mt['valid'], mref['valid']), name
    gated = TW._state(Cn, dtype)
    _accum(ops, z, gated, FULL, w, [True, True], sampling=sampling, depth=depth, gate=RM.GATE)
    full = TW._state(Cn, dtype)
    TW._accum(ops, z, full, FULL, w, [True, True], sampling=sampling)
    assert not TW._same_bits(gated['count'], full['count']) and not TW._same_bits(gated['mean'], full['mean']), 'the gate must matter'


# ------------------------------------------------------------------ 2. constant map
@pytest.mark.parametrize('Cn,dtype,sampling', FORMS[:4], ids=IDS[:4])
def test_a_constant_map_is_the_view_weight_times_the_constant(ia, Cn, dtype, sampling):
    """pixel_weight[slot] == c_v everywhere (c = 1.1, 0.7, 2.3: the products round): bit for bit the weighted lift whose view weights are the
    rounded fp32 products wv * c_v, in both modes, with a decayed second tick."""
    from imvoxelnet_amd import ops
    z = TW._inputs(Cn, dtype == BF16)
    pool, ppool, no, crop, _ = z
    c = np.asarray([1.1, 0.7, 2.3], np.float32)
    prod = [float(np.float32(w) * x) for w, x in zip(WV, c)]
    assert any(np.float64(np.float32(w)) * np.float64(x) != p for w, x, p in zip(WV, c, prod)), 'a product that rounds'
    pw = _slot_maps(_maps()['ones'] * c[:, None, None])
    st, ref = TW._state(Cn, dtype), TW._state(Cn, dtype)
    for t, views in enumerate(((0, 1), (2, 1))):
        lists = [[slot(b, v) for v in views] for b in range(2)]
        _accum(ops, z, st, lists, TW._slot_weights(WV), [t == 0] * 2, [0.75, 0.75], sampling=sampling, pixel_weight=pw)
        TW._accum(ops, z, ref, lists, TW._slot_weights(prod), [t == 0] * 2, [0.75, 0.75], sampling=sampling)
        _same_state(st, ref, t)
    mt, mref = TW._state(Cn, dtype), TW._state(Cn, dtype)
    _mean(ops, z, mt, FULL, TW._slot_weights(WV), sampling, pixel_weight=pw)
    ops.backproject_weighted_mean_(pool, ppool, FULL, TW._slot_weights(prod), ROWS, no, crop, R.VOXEL_SIZE, mref['mean'], mref['valid'], sampling=sampling)
    assert TW._same_bits(mt['mean'], mref['mean']) and TW._same_bits(mt['valid'], mref['valid'])
    plain = TW._state(Cn, dtype)
    ops.backproject_weighted_mean_(pool, ppool, FULL, TW._slot_weights(WV), ROWS, no, crop, R.VOXEL_SIZE, plain['mean'], plain['valid'], sampling=sampling)
    assert not TW._same_bits(mt['mean'], plain['mean']), 'the constants must matter'


# ------------------------------------------------------------------ 3. blocked view
@pytest.mark.parametrize('Cn,dtype,sampling', FORMS[:4], ids=IDS[:4])
def test_a_blocked_view_is_the_view_not_listed(ia, Cn, dtype, sampling):
    """View 1 blocked on every pixel -- by a pixel_weight of 0, NaN, a negative number, +inf, or a mixture of them, and by a depth map that puts a
    surface in front of every voxel the view sees (behind = 0) -- while views 0 and 2 keep the general maps: bit for bit the same call without
    view 1 in the lists, in both modes."""
    from imvoxelnet_amd import ops
    z = TW._inputs(Cn, dtype == BF16)
    m = _maps()
    w = TW._slot_weights(WV)
    for s0 in TW._scenes():
        ok = R.valid_views(s0['xf'], s0['yf'], s0['d'], s0['hc'], s0['wc'])
        assert ok[1].sum() > 0 and float(s0['d'][1][ok[1]].min()) > 2.0 ** -6, 'the near surface below lies in front of every voxel view 1 sees'

    def blocked_by(kind):
        pw, depth = m['pw'].copy(), m['depth'].copy()
        if kind == 'gate':
            depth[1] = 2.0 ** -6
        else:
            pw[1] = np.asarray([0.0, NAN, -2.0, INF], np.float32)[np.arange(R.FH * R.FW) % 4].reshape(R.FH, R.FW) if kind == 'mixed' else kind
        return dict(pixel_weight=_slot_maps(pw), depth=_slot_maps(depth), gate=(0.0, INF) if kind == 'gate' else RM.GATE)

    for kind in (0.0, NAN, -1.0, INF, 'mixed', 'gate'):
        kw = blocked_by(kind)
        st, ref, every = TW._state(Cn, dtype), TW._state(Cn, dtype), TW._state(Cn, dtype)
        _accum(ops, z, st, FULL, w, [True, True], sampling=sampling, **kw)
        _accum(ops, z, ref, SHORT, w, [True, True], sampling=sampling, **kw)
        _same_state(st, ref, kind)
        mt, mref = TW._state(Cn, dtype), TW._state(Cn, dtype)
        _mean(ops, z, mt, FULL, w, sampling, **kw)
        _mean(ops, z, mref, SHORT, w, sampling, **kw)
        assert TW._same_bits(mt['mean'], mref['mean']) and TW._same_bits(mt['valid'], mref['valid']), kind
        assert TW._same_bits(mt['mean'][ROWS], st['mean'][ROWS]), 'the mean mode is the accumulate mode from zero'
        _accum(ops, z, every, FULL, w, [True, True], sampling=sampling, pixel_weight=_slot_maps(m['pw']), depth=_slot_maps(m['depth']), gate=kw['gate'])
        assert not TW._same_bits(every['mean'], st['mean']) and not TW._same_bits(every['count'], st['count']), ('view 1 must matter when it is not blocked', kind)


# ------------------------------------------------------------------ 4. power of two
@pytest.mark.parametrize('Cn,dtype,sampling', FORMS[:4], ids=IDS[:4])
def test_maps_times_four_keep_the_mean_and_scale_the_sums_exactly(ia, Cn, dtype, sampling):
    from imvoxelnet_amd import ops
    z = TW._inputs(Cn, dtype == BF16)
    m = _maps()
    w, depth = TW._slot_weights(WV), _slot_maps(m['depth'])
    a, b = TW._state(Cn, dtype), TW._state(Cn, dtype)
    _accum(ops, z, a, FULL, w, [True, True], sampling=sampling, pixel_weight=_slot_maps(m['pw']), depth=depth, gate=RM.GATE)
    _accum(ops, z, b, FULL, w, [True, True], sampling=sampling, pixel_weight=_slot_maps(m['pw'] * 4), depth=depth, gate=RM.GATE)
    assert TW._same_bits(a['mean'], b['mean']) and TW._same_bits(a['valid'], b['valid']) and TW._same_bits(a['count'], b['count'])
    assert TW._same_bits(a['sum'][ROWS] * 4, b['sum'][ROWS]) and TW._same_bits(a['wsum'][ROWS] * 4, b['wsum'][ROWS])
    ma, mb = TW._state(Cn, dtype), TW._state(Cn, dtype)
    _mean(ops, z, ma, FULL, w, sampling, pixel_weight=_slot_maps(m['pw']), depth=depth, gate=RM.GATE)
    _mean(ops, z, mb, FULL, w, sampling, pixel_weight=_slot_maps(m['pw'] * 4), depth=depth, gate=RM.GATE)
    assert TW._same_bits(ma['mean'], mb['mean']) and TW._same_bits(ma['valid'], mb['valid']) and TW._same_bits(ma['mean'], a['mean'])
    gate_only = TW._state(Cn, dtype)
    _accum(ops, z, gate_only, FULL, w, [True, True], sampling=sampling, depth=depth, gate=RM.GATE)
    assert not TW._same_bits(a['mean'], gate_only['mean']) and not TW._same_bits(a['count'], gate_only['count']), 'the weight map must matter'


# ------------------------------------------------------------------ 5. general maps against the fp64 reference
GENERAL = [(8, False, 'nearest'), (8, False, 'bilinear'), (68, False, 'bilinear'), (520, False, 'nearest'), (8, True, 'bilinear'), (68, True, 'nearest'),
           (520, True, 'bilinear')]
TICKS = ((0, 1, 2), (1, 2), (0,), (2,))
DECAY, FORGET = (0.75, 0.5), 0.6
WG = (1.5, 0.5, 1.25)


@pytest.mark.parametrize('Cn,bf16,sampling', GENERAL, ids=[f'C{c}-{"bf16" if b else "f32"}-{s}' for c, b, s in GENERAL])
def test_general_maps_fading_and_forgetting_within_the_fp64_bound(ia, Cn, bf16, sampling):
    """The general weight map (confidences in [0.25, 1.75), blocked pixels sprinkled in), the dyadic depth map with its four kinds of holes under the
    gate (0.25, 0.5), view weights (1.5, 0.5, 1.25), decays (0.75, 0.5) per sample, forget_below 0.6, four ticks (views (0,1,2), (1,2), (0), (2)).
    After every tick: valid and count -- hence the set of forgotten voxels, whose counts restart -- equal the reference exactly; the mean and the
    sums are within K * 2^-24 * A (+ the bf16 store term) with K = ref_unproject_maps.k_mapped(views counted so far, fading ticks so far) and
    no further margin; wsum within one ulp per rounding (a product and an addition per view, a product per fade).  The forgetting decision compares a
    rounded W with the threshold, so the test first shows, on the reference alone, that no faded W comes within 64 ulp of it.  Rows 0 and 2 keep
    their sentinels; the mean mode gives the first tick's bits."""
    from imvoxelnet_amd import ops
    z = TW._inputs(Cn, bf16)
    host = z[4]
    bil = sampling == 'bilinear'
    m = _maps()
    kw = dict(pixel_weight=_slot_maps(m['pw']), depth=_slot_maps(m['depth']), gate=RM.GATE)
    refs = [RM.MappedReference(host[b], sc['xf'], sc['yf'], sc['d'], sc['hc'], sc['wc'], bil, FORGET, m['pw'], m['depth'], RM.GATE)
            for b, sc in enumerate(TW._scenes())]
    dtype = BF16 if bf16 else F32
    st = TW._state(Cn, dtype)
    n, forgotten = 0, 0
    for t, views in enumerate(TICKS):
        n += len(views)
        for b, ref in enumerate(refs):
            if t:
                faded = ref.W * float(np.float32(DECAY[b]))
                assert np.all(np.abs(faded - FORGET)[ref.W > 0] > 64 * np.spacing(np.float32(FORGET))), 'a weight sum too near the threshold to decide in fp32'
                forgotten += int(((faded < FORGET) & (ref.W > 0)).sum())
            ref.tick(list(views), [WG[v] for v in views], decay=DECAY[b], first=t == 0)
        _accum(ops, z, st, [[slot(b, v) for v in views] for b in range(2)], TW._slot_weights(WG), [t == 0] * 2, list(DECAY), sampling=sampling,
               forget_below=FORGET, **kw)
        TW._check(f'maps tick {t} C{Cn} {sampling}', st, refs, RM.k_mapped(n, t, bil), bf16, wsum_ulps=2 * n + t)
        if t == 0:
            mt = TW._state(Cn, dtype)
            _mean(ops, z, mt, FULL, TW._slot_weights(WG), sampling, **kw)
            assert TW._same_bits(mt['mean'][ROWS], st['mean'][ROWS]) and TW._same_bits(mt['valid'][ROWS], st['valid'][ROWS])
            assert bool((mt['mean'][0].float() == -7.0).all()) and bool((mt['valid'][2] == 7).all())
    print('voxels forgotten over the ticks:', forgotten)
    assert forgotten > 20, 'the forgetting rule must have acted'
    assert TW._is_sentinel(st, 0) and TW._is_sentinel(st, 2), 'a row that no sample names was written'
    counts = [refs[b].result()['count'] for b in range(2)]
    assert all(0 < int((c == 0).sum()) < c.size for c in counts) and max(int(c.max()) for c in counts) >= 3
