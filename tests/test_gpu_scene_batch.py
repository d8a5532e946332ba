"""-m gpu: scene batches -- the listed lift with per-sample rows and `first` flags (ops.backproject_lists_accum_ / _mean_,
ivx_backproject_lists_fwd) against the imported reference's golden vectors and against the B = 1 launches of the existing kernels, bit for
bit; SceneBatch (model.open_scenes) against the one-shot lift, against independent SceneSessions and against the model's batched detection
stage; ragged one-shot batches (model.simple_test_ragged)."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_scene_stream import _golden, _wide_case, _state, _indoor_small, _same_results, _full_meta, GOLDEN_CHUNKS, GARBAGE
from test_gpu_scene_window import _pool, _family, GOLDEN_SLOTS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ia():
    import imvoxelnet_amd
    from imvoxelnet_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    return imvoxelnet_amd


def _bits(t):
    """A tensor as integers, so that NaN sentinels compare."""
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _is_sentinel(st, r):
    """Row r of a _state() still holds what _state() wrote."""
    return (bool(torch.isnan(st['sum'][r]).all()) and bool((st['count'][r] == GARBAGE).all()) and bool((st['mean'][r].float() == -7.0).all())
            and bool((st['valid'][r] == 7).all()))


# ------------------------------------------------------------------ golden, pinned to the imported reference
@pytest.fixture(scope='module')
def golden(ia):
    out = {}
    for case, (slots, S) in GOLDEN_SLOTS.items():
        c, feat, P, no, crop, vs, nv = _golden(case)
        pool, ppool = _pool(feat, P[0], slots, S)
        out[case] = dict(c=c, pool=pool, ppool=ppool, slots=slots, no=no, crop=crop, vs=vs, nv=nv)
    return out


@pytest.mark.parametrize('case,chunks', GOLDEN_CHUNKS, ids=[f'{k}-{"_".join(map(str, c))}' for k, c in GOLDEN_CHUNKS])
def test_listed_accumulate_equals_reference_bit_for_bit(ia, golden, case, chunks):
    """The golden maps sit in scattered slots of a NaN pool; the state pools have R = 3 rows of NaN / garbage / sentinels and the sample
    owns row 2.  Views added chunk by chunk, the first chunk with first = 1: mean, mask and count of row 2 after the last chunk are the
    imported reference's, bit for bit; rows 0 and 1 keep their sentinels.  C = 8: a 2-lane group, partial projection rounds, a partial
    last workgroup."""
    from imvoxelnet_amd import ops
    g = golden[case]
    c = g['c']
    st = _state(3, g['nv'], g['pool'].shape[-1])
    v0 = 0
    for n in chunks:
        ops.backproject_lists_accum_(g['pool'], g['ppool'], [[g['slots'][v] for v in range(v0, v0 + n)]], [2], [v0 == 0], g['no'], g['crop'], g['vs'],
                                     st['sum'], st['count'], st['mean'], st['valid'])
        v0 += n
    assert v0 == c['volume'].shape[0]
    got = st['mean'][2].permute(3, 0, 1, 2).cpu().numpy()
    assert np.array_equal(got, c['mean']), f'{(got != c["mean"]).sum()} voxel-channels differ'
    assert np.array_equal(st['valid'][2].cpu().numpy().astype(bool), c['mean_valid'][0])
    assert np.array_equal(st['count'][2].cpu().numpy(), c['valid'].sum(0)[0])
    assert _is_sentinel(st, 0) and _is_sentinel(st, 1), 'a row that no sample names was written'
    assert bool(torch.isnan(g['pool']).any()), 'the pool keeps its NaN slots'


# ------------------------------------------------------------------ a ragged batch against per-sample B = 1 launches
WIDE = [(8, torch.float32, 'nearest'), (256, torch.float32, 'nearest'), (512, torch.float32, 'nearest'), (256, torch.bfloat16, 'nearest'),
        (8, torch.float32, 'bilinear'), (256, torch.float32, 'bilinear')]
PERM = [9, 3, 12, 0, 7, 5, 13, 1, 10, 4, 8, 2]              # view i of _wide_case's 12 sits in slot PERM[i]; slots 6 and 11 stay NaN
RAGGED = [[4, 1, 3, 1, 0], [2, 5]]                          # per sample: its own views, in its own order; sample 0 repeats view 1


def _wide_pool(C, dtype):
    feat, P, no, crop, vs, nv = _wide_case(C, dtype)
    pool, ppool = _pool(feat, P.reshape(12, 3, 4), PERM, 14)
    return dict(feat=feat, P=P, no=no, crop=crop, vs=vs, nv=nv, pool=pool, ppool=ppool)


def _sample(z, b, views):
    """Contiguous copies of these views of sample b, with that sample's origin and crop: the arguments of a B = 1 launch."""
    idx = torch.tensor([b * 6 + v for v in views], device='cuda')
    return z['feat'][idx].contiguous(), z['P'][b:b + 1, torch.tensor(views, device='cuda')].contiguous(), z['no'][b:b + 1].contiguous(), z['crop'][b:b + 1].contiguous()


@pytest.mark.parametrize('C,dtype,sampling', WIDE, ids=[f'C{c}-{str(d).split(".")[1]}-{s}' for c, d, s in WIDE])
def test_ragged_batch_equals_per_sample_launches(ia, C, dtype, sampling):
    """Two samples of 5 and 2 listed views (-1 padding in the middle of the first row, at the end of the second after the op's own
    padding), rows [2, 0] of R = 3, first [True, False]: row 0 carries the state of an earlier call.  torch.equal to ops.backproject_accum_
    at B = 1 over contiguous copies, for sum, count, mean and valid; row 1 is untouched.  The mean mode against ops.backproject_mean per
    sample; identity rows and equal-length lists against ops.backproject_gather_mean."""
    from imvoxelnet_amd import ops
    z = _wide_pool(C, dtype)
    nv, vs = z['nv'], z['vs']
    slot = lambda b, v: PERM[b * 6 + v]
    # the references: B = 1 accumulate launches; sample 1's state has seen its views (0, 1) before
    ref = [_state(1, nv, C, dtype), _state(1, nv, C, dtype)]
    f, P, no, crop = _sample(z, 1, [0, 1])
    ops.backproject_accum_(f, P, no, crop, vs, ref[1]['sum'], ref[1]['count'], True, ref[1]['mean'], ref[1]['valid'], sampling=sampling)
    st = _state(3, nv, C, dtype)
    for k in ('sum', 'count', 'mean', 'valid'):
        st[k][0].copy_(ref[1][k][0])
    for b, first in ((0, True), (1, False)):
        f, P, no, crop = _sample(z, b, RAGGED[b])
        ops.backproject_accum_(f, P, no, crop, vs, ref[b]['sum'], ref[b]['count'], first, ref[b]['mean'], ref[b]['valid'], sampling=sampling)
    l0 = [slot(0, v) for v in RAGGED[0]]
    lists = [l0[:2] + [-1] + l0[2:], [slot(1, v) for v in RAGGED[1]]]
    out = ops.backproject_lists_accum_(z['pool'], z['ppool'], lists, [2, 0], [True, False], z['no'], z['crop'], vs, st['sum'], st['count'], st['mean'], st['valid'],
                                       sampling=sampling)
    assert out[0] is st['sum'] and out[1] is st['count']
    for b, r in ((0, 2), (1, 0)):
        for k in ('sum', 'count', 'mean', 'valid'):
            assert torch.equal(st[k][r], ref[b][k][0]), (b, k)
    assert st['mean'].dtype == dtype and not bool(torch.isnan(st['sum'][[0, 2]]).any())
    assert _is_sentinel(st, 1), 'row 1 is named by no sample'
    assert not torch.equal(st['valid'][2], st['valid'][0]), 'the two samples must differ for the sample and row indices to be tested'
    # the mean mode, same ragged lists
    mt = _state(3, nv, C, dtype)
    vol, valid = ops.backproject_lists_mean_(z['pool'], z['ppool'], lists, [2, 0], z['no'], z['crop'], vs, mt['mean'], mt['valid'], sampling=sampling)
    assert vol is mt['mean'] and valid.dtype == torch.bool
    for b, r in ((0, 2), (1, 0)):
        f, P, no, crop = _sample(z, b, RAGGED[b])
        rv, rok = ops.backproject_mean(f, P, no, crop, vs, nv, sampling=sampling)
        assert torch.equal(mt['mean'][r], rv[0]) and torch.equal(valid[r], rok[0]), b
    assert bool((mt['mean'][1].float() == -7.0).all()) and bool((mt['valid'][1] == 7).all())
    # identity rows, equal lengths: the gathered launch's bits
    eq = [[slot(0, v) for v in (4, 1, 3, 0, 2)], [slot(1, v) for v in (2, 5, 0, 0, 3)]]
    gv, gok = ops.backproject_gather_mean(z['pool'], z['ppool'], eq, z['no'], z['crop'], vs, nv, sampling=sampling)
    m2 = _state(2, nv, C, dtype)
    vol, valid = ops.backproject_lists_mean_(z['pool'], z['ppool'], eq, [0, 1], z['no'], z['crop'], vs, m2['mean'], m2['valid'], sampling=sampling)
    assert torch.equal(vol, gv) and torch.equal(valid, gok)


# ------------------------------------------------------------------ the raw binding: device lists, NULL lists
def _raw(mode, pool, ppool, view_slot, row, first, no, crop, vs, vol, count, mean, valid, R, sampling=0, d_first=0):
    """ivx_backproject_lists_fwd with device lists as they are (view_slot [B,V], row [B] / None, first [B] / None: int32 device tensors)."""
    from imvoxelnet_amd import _lib, ops
    p = ops._ptr
    B, V = view_slot.shape
    S, _, FH, FW, C = pool.shape
    X, Y, Z = vol.shape[1:4]
    d = _lib.BackprojectDesc(B, V, FH, FW, C, X, Y, Z, (ctypes.c_float * 3)(*[float(v) for v in vs]), ops._DT[pool.dtype], mode, sampling, d_first)
    l = _lib.LiftLists(S, R, view_slot.data_ptr(), row.data_ptr() if row is not None else None, first.data_ptr() if first is not None else None)
    _lib.check(_lib.lib().ivx_backproject_lists_fwd(ctypes.byref(d), ctypes.byref(l), p(pool), p(ppool), p(no), p(crop), p(vol), p(count), p(mean), p(valid),
                                                    ops._stream()), 'ivx_backproject_lists_fwd')
    torch.cuda.synchronize()


def _dev(l):
    return torch.tensor(l, dtype=torch.int32).cuda()


def test_null_row_and_first_lists_equal_the_gather_and_the_plain_accumulate(ia, golden):
    """row == NULL, first == NULL: the mean mode is the gathered launch (same bits); the accumulate mode takes d->first for every sample
    and row b for sample b."""
    from imvoxelnet_amd import ops
    g = golden['C']
    slots = _dev([[g['slots'][v] for v in (0, 1, 2, 3, 4, 5)]])
    gv, gok = ops.backproject_gather_mean(g['pool'], g['ppool'], slots, g['no'], g['crop'], g['vs'], g['nv'])
    st = _state(1, g['nv'], 8)
    _raw(0, g['pool'], g['ppool'], slots, None, None, g['no'], g['crop'], g['vs'], st['mean'], None, None, st['valid'], R=1)
    assert torch.equal(st['mean'], gv) and torch.equal(st['valid'].view(torch.bool), gok)
    st = _state(1, g['nv'], 8)
    _raw(2, g['pool'], g['ppool'], slots[:, :2].contiguous(), None, None, g['no'], g['crop'], g['vs'], st['sum'], st['count'], None, None, R=1, d_first=1)
    _raw(2, g['pool'], g['ppool'], slots[:, 2:].contiguous(), None, None, g['no'], g['crop'], g['vs'], st['sum'], st['count'], st['mean'], st['valid'], R=1, d_first=0)
    assert np.array_equal(st['mean'][0].permute(3, 0, 1, 2).cpu().numpy(), g['c']['mean'])


# ------------------------------------------------------------------ the order of a list is observable
@pytest.fixture(scope='module')
def circle(ia):
    """The four circle cameras and the 24 x 24 x 8 grid of _indoor_small, seeded random 24 x 32 maps with C = 8."""
    model, scene_meta, E, _ = _indoor_small(ia)
    proj, no, crop = model._camera_setup([_full_meta(scene_meta, E)], 4, torch.device('cuda'))
    feat = torch.randn(4, 1, 24, 32, 8, generator=torch.Generator().manual_seed(41)).cuda()
    return dict(feat=feat, proj=proj, no=no, crop=crop, vs=model.voxel_size, nv=model.n_voxels)


def test_list_order_changes_bits_as_the_contiguous_kernel(ia, circle):
    """Precondition as in test_circle_case_can_show_the_order: >= 100 voxels seen by three or more views, and the contiguous kernel's
    own result depends on the order.  Two samples list the same four views in different orders: each row is the contiguous kernel's
    result for its order, so the two rows differ as those do."""
    from imvoxelnet_amd import ops
    z = circle
    _, count = ops.backproject_sum(z['feat'], z['proj'], z['no'], z['crop'], z['vs'], z['nv'])
    assert int((count >= 3).sum()) >= 100
    slots = [4, 0, 5, 2]
    pool, ppool = _pool(z['feat'], z['proj'][0], slots, 6)
    orders = [(0, 1, 2, 3), (3, 2, 1, 0), (2, 0, 3, 1)]
    refs = []
    for o in orders:
        idx = torch.tensor(o, device='cuda')
        refs.append(ops.backproject_mean(z['feat'][idx].contiguous(), z['proj'][:, idx].contiguous(), z['no'], z['crop'], z['vs'], z['nv']))
    assert not torch.equal(refs[0][0], refs[1][0]), 'reversing the views must change some bits, or the order is not observable here'
    st = _state(4, z['nv'], 8)
    no, crop = z['no'].repeat(3, 1).contiguous(), z['crop'].repeat(3, 1).contiguous()
    ops.backproject_lists_accum_(pool, ppool, [[slots[v] for v in o] for o in orders], [3, 0, 1], [True] * 3, no, crop, z['vs'], st['sum'], st['count'],
                                 st['mean'], st['valid'])
    for (rv, rok), r in zip(refs, (3, 0, 1)):
        assert torch.equal(st['mean'][r], rv[0]) and torch.equal(st['valid'][r].view(torch.bool), rok[0]), r
    assert not torch.equal(st['mean'][3], st['mean'][0]) and torch.equal(st['count'][3], st['count'][0])
    assert _is_sentinel(st, 2)


# ------------------------------------------------------------------ the guards, reading only memory this test owns
def _guarded_state(R, nv, C):
    """State pools that are the inner R rows of allocations two rows larger: the outer rows keep _state()'s sentinels."""
    big = _state(R + 2, nv, C)
    return big, {k: v[1:1 + R] for k, v in big.items()}


@pytest.mark.parametrize('bad_row', [-1, 2], ids=['row_minus1', 'row_R'])
def test_out_of_range_row_does_nothing(ia, golden, bad_row):
    """R = 2.  A sample whose row is -1 or R, in a device list, changes nothing anywhere: the allocations around the pools (which a
    missing guard would hit: rows -1 and R of the pools are rows 0 and 3 of the allocations) keep their sentinels, row 0 of the pools too,
    and the other sample's row equals the launch without the bad sample."""
    g = golden['C']
    C, R = 8, 2
    views = [g['slots'][v] for v in range(6)]
    no, crop = g['no'].repeat(2, 1).contiguous(), g['crop'].repeat(2, 1).contiguous()
    for mode in (2, 0):
        big, st = _guarded_state(R, g['nv'], C)
        assert all(v.is_contiguous() for v in st.values())
        alone_big, alone = _guarded_state(R, g['nv'], C)
        if mode == 2:
            _raw(2, g['pool'], g['ppool'], _dev([views]), _dev([1]), _dev([1]), g['no'], g['crop'], g['vs'], alone['sum'], alone['count'], alone['mean'], alone['valid'], R)
            _raw(2, g['pool'], g['ppool'], _dev([views, views[::-1]]), _dev([1, bad_row]), _dev([1, 1]), no, crop, g['vs'], st['sum'], st['count'], st['mean'],
                 st['valid'], R)
        else:
            _raw(0, g['pool'], g['ppool'], _dev([views]), _dev([1]), None, g['no'], g['crop'], g['vs'], alone['mean'], None, None, alone['valid'], R)
            _raw(0, g['pool'], g['ppool'], _dev([views, views[::-1]]), _dev([1, bad_row]), None, no, crop, g['vs'], st['mean'], None, None, st['valid'], R)
        for k in big:
            assert _same_bits(big[k], alone_big[k]), (mode, k)
        for r in (0, 1, 3):                       # allocation rows: below the pools, pool row 0, above the pools
            assert _is_sentinel(big, r), (mode, r)
        assert np.array_equal(st['mean'][1].permute(3, 0, 1, 2).cpu().numpy(), g['c']['mean'])


@pytest.mark.parametrize('sampling', ['nearest', 'bilinear'])
def test_out_of_range_slots_are_unseen_views_in_the_accumulate_mode(ia, sampling):
    """As test_out_of_range_slots_are_unseen_views: the pools are views [1 : 1 + S] of allocations whose outer slots hold 1e30, so a
    missing guard reads memory this test owns and 1e30 shows up in the sums.  Slots -1 and S in a device list give exactly the state of
    the list without them."""
    from imvoxelnet_amd import _lib
    c, feat, P, no, crop, vs, nv = _golden('C')
    S = 6
    big, pbig = _pool(feat, P[0], list(range(1, 1 + S)), S + 2, fill=1e30)
    pool, ppool = big[1:1 + S], pbig[1:1 + S]
    assert pool.is_contiguous() and float(big[0].min()) > 1e29 and float(big[S + 1].min()) > 1e29 and float(pbig[0].min()) > 1e29
    smp = _lib.sampling_id(sampling)
    a, b = _state(2, nv, 8), _state(2, nv, 8)
    _raw(2, pool, ppool, _dev([[0, 1, 2, 3, 4, 5]]), _dev([1]), _dev([1]), no, crop, vs, a['sum'], a['count'], a['mean'], a['valid'], 2, smp)
    _raw(2, pool, ppool, _dev([[0, -1, 1, S, 2, 3, 4, 5]]), _dev([1]), _dev([1]), no, crop, vs, b['sum'], b['count'], b['mean'], b['valid'], 2, smp)
    assert float(b['sum'][1].abs().max()) < 1e20, 'a sentinel slot was read'
    for k in a:
        assert _same_bits(a[k], b[k]), k
    if sampling == 'nearest':
        assert np.array_equal(b['mean'][1].permute(3, 0, 1, 2).cpu().numpy(), c['mean'])
    assert _is_sentinel(b, 0)


def test_zero_view_rows(ia, golden):
    """A sample with no in-range slot adds nothing: with first its row becomes zero sum / zero count / mean 0 / valid 0; without first
    its row is stored back bit-unchanged (NaN sums and a garbage count included).  The other sample of the launch is served as usual."""
    from imvoxelnet_amd import ops
    g = golden['C']
    views = [g['slots'][v] for v in range(6)]
    no, crop = g['no'].repeat(2, 1).contiguous(), g['crop'].repeat(2, 1).contiguous()
    st = _state(3, g['nv'], 8)
    ops.backproject_lists_accum_(g['pool'], g['ppool'], [[], views], [0, 2], [True, True], no, crop, g['vs'], st['sum'], st['count'], st['mean'], st['valid'])
    assert not bool(st['sum'][0].any()) and not bool(st['count'][0].any()) and not bool(st['mean'][0].any()) and not bool(st['valid'][0].any())
    assert torch.equal(_bits(st['sum'][0]), torch.zeros_like(_bits(st['sum'][0]))), 'the zero sums are +0'
    assert np.array_equal(st['mean'][2].permute(3, 0, 1, 2).cpu().numpy(), g['c']['mean']) and _is_sentinel(st, 1)
    st2 = _state(3, g['nv'], 8)
    st2['sum'][1, ..., 1] = 3.25                       # some of the stored state is finite, and some of it NaN
    before = {k: v.clone() for k, v in st2.items()}
    ops.backproject_lists_accum_(g['pool'], g['ppool'], [[-1, -1, -1], views], [1, 2], [False, True], no, crop, g['vs'], st2['sum'], st2['count'])
    for k in st2:
        assert _same_bits(st2[k][:2], before[k][:2]), k
    assert torch.equal(st2['sum'][2], st['sum'][2]) and torch.equal(st2['count'][2], st['count'][2])
    m = _state(2, g['nv'], 8)                          # the mean mode: an empty list gives zeros and nothing valid
    ops.backproject_lists_mean_(g['pool'], g['ppool'], [[]], [1], g['no'], g['crop'], g['vs'], m['mean'], m['valid'])
    assert not bool(m['mean'][1].any()) and not bool(m['valid'][1].any()) and bool((m['mean'][0] == -7.0).all())


# ------------------------------------------------------------------ SceneBatch against the lift
TICKS = [([0, 1, 2], [0, 0, 2]), ([3, 4], [1, 2]), ([2], [0])]          # (views of _family's five, their scenes): scene 1 stays empty until the second tick


@pytest.fixture(scope='module')
def families(ia):
    cache = {}

    def get(family):
        if family not in cache:
            cache[family] = _family(ia, family)
        return cache[family]
    return get


def _scene_metas(z, N=3):
    """N scene metas on one model: scene 1 has another focal length, the last another origin."""
    metas = [dict(z['scene_meta'], lidar2img=dict(z['scene_meta']['lidar2img'])) for _ in range(N)]
    if N > 1:
        K = metas[1]['lidar2img']['intrinsic'].copy()
        K[:2, :2] *= np.float32(0.9375)
        metas[1]['lidar2img']['intrinsic'] = K
        metas[-1]['lidar2img']['origin'] = (np.asarray(metas[-1]['lidar2img']['origin']) + np.array([0.08, -0.04, 0.02], np.float32)).astype(np.float32)
    return metas


def _run_ticks(z, ticks=TICKS, check_each_tick=True):
    """The ticks on a batch of three scenes and on three independent sessions.  Asserted after every tick, whatever the trunk's mode:
    every scene's volume() is bit for bit ONE ops.backproject_mean over the features batch._features gave for that scene's views, in
    order; mask and count are the one-shot lift's.  Returns the figures against the sessions."""
    from imvoxelnet_amd import ops
    model, E, img = z['model'], z['E'], z['img']
    metas = _scene_metas(z)
    batch = model.open_scenes(metas)
    sessions = [model.open_scene(m) for m in metas]
    feats, feats_s, views = [[] for _ in metas], [[] for _ in metas], [[] for _ in metas]
    for vs, sc in ticks:
        x = img[torch.tensor(vs, device='cuda')].contiguous()
        assert batch.add_views(x, [E[v] for v in vs], sc) is batch
        f = batch._features(x).clone()                      # the same trunk call again: the same bits
        for i, (v, s) in enumerate(zip(vs, sc)):
            feats[s].append(f[i:i + 1])
            views[s].append(v)
        for s in sorted(set(sc)):                           # the sessions get their views of this tick in one call each
            mine = [v for v, q in zip(vs, sc) if q == s]
            xs = img[torch.tensor(mine, device='cuda')].contiguous()
            sessions[s].add_views(xs, [E[v] for v in mine])
            feats_s[s].append(sessions[s]._features(xs).clone())
        assert batch.n_views == [len(v) for v in views]
        if not check_each_tick:
            continue
        for s, vl in enumerate(views):
            if not vl:
                with pytest.raises(RuntimeError, match='no views'):
                    batch.volume(s)
                continue
            meta = _full_meta(metas[s], [E[v] for v in vl])
            assert all(np.array_equal(a, b) for a, b in zip(batch.metas[s]['lidar2img']['extrinsic'], meta['lidar2img']['extrinsic']))
            proj, no, crop = model._camera_setup([meta], 4, img.device)
            p = torch.cat(feats[s]).contiguous()
            ref, ref_ok = ops.backproject_mean(p, proj, no, crop, model.voxel_size, model.n_voxels, sampling=model.sampling)
            got, ok = batch.volume(s)
            assert got.dtype == ref.dtype and torch.equal(got, ref) and torch.equal(ok, ref_ok), f'scene {s} is not the one-shot lift of the features it was given'
            _, one_ok = model.lift_cl(model.features_2d_cl(img[torch.tensor(vl, device='cuda')][None].contiguous()), [meta])
            _, cnt = ops.backproject_sum(p.float(), proj, no, crop, model.voxel_size, model.n_voxels)
            assert torch.equal(ok, one_ok) and torch.equal(batch._count[s:s + 1], cnt), 'mask and count do not depend on the features'
    figs = []
    for s, sess in enumerate(sessions):
        got, ref = batch.volume(s)[0].float(), sess.volume()[0].float()
        feats_equal = torch.equal(torch.cat(feats[s]), torch.cat(feats_s[s]))
        vol_equal = torch.equal(got, ref)
        assert vol_equal or not feats_equal, 'equal features must give equal volumes'
        assert torch.equal(batch.volume(s)[1], sess.volume()[1])
        figs.append((float((got - ref).abs().max()), float(ref.abs().max()), feats_equal, vol_equal))
        sess.close()
    return batch, metas, figs


@pytest.mark.parametrize('family', ['indoor', 'anchor'])
def test_batch_volumes_are_the_one_shot_lift_of_their_features(ia, families, family):
    """Three scenes, ticks scene = [0,0,2], [1,2], [0] (_run_ticks has the exact claims).  Against three independent SceneSessions fed the
    same views the bar is the project's own, max|d| <= 2e-4 * max|ref|: with the default fp16-pair trunk the per-tensor operand scales
    depend on which views share a trunk call.  The figures are printed before the bar is asserted."""
    z = families(family)
    batch, _, figs = _run_ticks(z)
    assert tuple(batch._sum.shape[:1]) == (3,) and batch._sum.dtype == torch.float32 and batch._ring is None
    for s, (d, scale, fe, ve) in enumerate(figs):
        print(f'{family} scene {s}: batch vs session max|d| {d:.3e} max|ref| {scale:.3e} ratio {d / scale:.3e} features bit-equal {fe} volume bit-equal {ve}')
    for d, scale, _, _ in figs:
        assert d <= 2e-4 * scale
    batch.close()
    with pytest.raises(RuntimeError, match='closed'):
        batch.detect()


def test_batch_with_fp32_operand_trunk(ia):
    """FusedConv.trunk_operands = 0: no per-tensor operand scale couples the views of a trunk call.  The exact rules of _run_ticks, among
    them: wherever a scene's per-view features are bit-equal to the session's, so is its volume; and the 2e-4 bar."""
    from imvoxelnet_amd.conv import FusedConv
    keep = FusedConv.trunk_operands
    FusedConv.trunk_operands = 0
    try:
        z = _family(ia, 'indoor')
        batch, _, figs = _run_ticks(z, check_each_tick=False)
    finally:
        FusedConv.trunk_operands = keep
    for s, (d, scale, fe, ve) in enumerate(figs):
        print(f'fp32-operand trunk, scene {s}: max|d| {d:.3e} max|ref| {scale:.3e} features bit-equal {fe} volume bit-equal {ve}')
        assert d <= 2e-4 * scale
    batch.close()


@pytest.mark.parametrize('prepare_kw', [dict(sampling='bilinear'), dict(dtype=torch.bfloat16)], ids=['bilinear', 'bf16'])
def test_batch_exact_claim_with_the_bilinear_rule_and_bf16_storage(ia, prepare_kw):
    z = _family(ia, 'indoor', **prepare_kw)
    batch, _, _ = _run_ticks(z, ticks=TICKS[:2])
    assert batch._mean.dtype == prepare_kw.get('dtype', torch.float32) and batch._sum.dtype == torch.float32
    batch.close()


def test_emit_false_and_add_views_u8(ia, families):
    """emit=False stores no mean until it is asked; uint8 frames through add_views_u8 == add_views on prepare_images_device's output."""
    from imvoxelnet_amd.data import prepare_images_device
    z = families('indoor')
    model, E = z['model'], z['E']
    rng = np.random.default_rng(72)
    frames = [rng.integers(0, 256, (190, 256, 3), dtype=np.uint8) for _ in range(3)]
    user = {k: v for k, v in z['scene_meta'].items() if k not in ('img_shape', 'ori_shape', 'pad_shape')}
    img, shapes = prepare_images_device([frames], (128, 96))
    a, b = model.open_scenes([dict(user, **shapes[0])] * 2), model.open_scenes([user] * 2)
    a.add_views(img[0], E[:3], [1, 0, 1])
    b.add_views_u8(frames, E[:3], [1, 0, 1], (128, 96), emit=False)
    assert all(tuple(m[k]) == tuple(shapes[0][k]) for m in b.metas for k in ('img_shape', 'ori_shape', 'pad_shape'))
    assert [r._stale for r in b._scenes] == [True, True] and [r._stale for r in a._scenes] == [False, False]
    for s in range(2):
        (va, oa), (vb, ob) = a.volume(s), b.volume(s)
        assert torch.equal(va, vb) and torch.equal(oa, ob) and 0 < int(oa.sum())
    a.close()
    b.close()


# ------------------------------------------------------------------ detect
def _stage(model, vol, valid, metas):
    """The model's batched detection stage on stacked rows, as result dicts."""
    from imvoxelnet_amd.boxes import bbox3d2result
    from imvoxelnet_amd.heads import Anchor3DHead
    if isinstance(model.bbox_head, Anchor3DHead):
        return model._results_one_copy(*model.detect_cl(vol, metas), metas)
    return [bbox3d2result(b, s, l) for b, s, l in model.detect_indoor_cl(vol, valid, metas)]


@pytest.mark.parametrize('family', ['indoor', 'anchor'])
def test_detect_is_the_batched_detection_stage(ia, families, family):
    z = families(family)
    model = z['model']
    batch, _, _ = _run_ticks(z, check_each_tick=False)
    rows = [batch.volume(s) for s in range(3)]
    vol, valid = torch.cat([r[0] for r in rows]).clone(), torch.cat([r[1] for r in rows]).clone()
    n_valid = [int(r[1].sum()) for r in rows]
    ref = _stage(model, vol, valid, batch.metas)
    res = batch.detect()
    n_det = [len(r['scores_3d']) for r in res]
    print(family, 'detections per scene', n_det, 'valid voxels per scene', n_valid, 'of', rows[0][1].numel())
    assert len(res) == 3 and sum(n_det) > 0 and all(0 < n < rows[0][1].numel() for n in n_valid)
    for i in range(3):
        _same_results([res[i]], [ref[i]])
    idx = torch.tensor([2, 0], device='cuda')
    ref = _stage(model, vol[idx].contiguous(), valid[idx].contiguous(), [batch.metas[2], batch.metas[0]])
    res = batch.detect([2, 0])
    assert len(res) == 2
    for i in range(2):
        _same_results([res[i]], [ref[i]])
    batch.reset(scenes=[1])
    assert batch.n_views[1] == 0 and len(batch.detect()) == 2, 'None means every scene that has views'
    batch.close()


@pytest.mark.parametrize('family', ['indoor', 'anchor'])
def test_batch_of_one_fed_all_views_is_simple_test(ia, families, family):
    z = families(family)
    model, E, img = z['model'], z['E'], z['img']
    meta = _full_meta(z['scene_meta'], E)
    ref = model.simple_test(img[None], [meta])
    assert model._native is not None, 'simple_test must run on the native handle here'
    batch = model.open_scenes([z['scene_meta']])
    batch.add_views(img, E, [0] * len(E))
    vol, valid = batch.volume(0)
    rv, rok = model.lift_cl(model.features_2d_cl(img[None]), [meta])
    assert torch.equal(vol, rv) and torch.equal(valid, rok)
    print(family, 'detections', len(ref[0]['scores_3d']), 'valid voxels', int(valid.sum()), 'of', valid.numel())
    assert len(ref[0]['scores_3d']) > 0 and 0 < int(valid.sum()) < valid.numel()
    _same_results(batch.detect(), ref)
    batch.close()


# ------------------------------------------------------------------ the windowed batch
def _fresh_window(z, meta, views, feat_of, W):
    """A fresh windowed SceneSession that holds these views, given the batch's features for them instead of running the trunk."""
    s = z['model'].open_scene(meta, window=W)
    for v in views:
        s._features = lambda img, f=feat_of[v]: f
        s.add_views(z['img'][v:v + 1], [z['E'][v]])
    vol, valid = s.volume()
    out = vol.clone(), valid.clone()
    s.close()
    return out


def test_windowed_batch_equals_fresh_windowed_sessions(ia, families):
    """N = 2, W = 2: FIFO eviction per scene, remove_views, refill, reset(scenes=[1]).  After every step each scene's volume is torch.equal
    to a fresh windowed SceneSession holding the same views' features.  A tick that touches only scene 0 does not re-lift scene 1: a
    sentinel written into its valid row survives and its mean row keeps its bits."""
    z = families('indoor')
    model, E, img = z['model'], z['E'], z['img']
    metas = _scene_metas(z, 2)
    batch = model.open_scenes(metas, window=2)
    feat_of, held = {}, [[], []]

    def tick(vs, sc):
        x = img[torch.tensor(vs, device='cuda')].contiguous()
        batch.add_views(x, [E[v] for v in vs], sc)
        f = batch._features(x).clone()
        for i, (v, s) in enumerate(zip(vs, sc)):
            feat_of[v, s] = f[i:i + 1]
            held[s] = (held[s] + [v])[-2:]

    def check(ids):
        for s in range(2):
            if not held[s]:
                assert batch.n_views[s] == 0
                continue
            vol, valid = _fresh_window(z, metas[s], held[s], {v: feat_of[v, s] for v in held[s]}, 2)
            got, ok = batch.volume(s)
            assert torch.equal(got, vol) and torch.equal(ok, valid) and 0 < int(ok.sum()) < ok.numel(), s
            assert batch.view_ids(s) == ids[s] and not batch._scenes[s]._stale

    tick([0, 1, 2], [0, 1, 0])
    assert batch._sum is None and tuple(batch._ring.shape[:2]) == (4, 1) and [r._stale for r in batch._scenes] == [True, True]
    check([[0, 1], [0]])
    tick([3, 4], [0, 1])                                   # scene 0 is full: its view 0 leaves
    check([[1, 2], [0, 1]])
    keep = batch._mean[1].clone()
    batch._valid[1].fill_(9)
    tick([0], [0])                                         # touches scene 0 only
    assert [r._stale for r in batch._scenes] == [True, False]
    batch.volume(0)
    assert len(batch.detect([0])) == 1
    assert bool((batch._valid[1] == 9).all()) and _same_bits(batch._mean[1], keep), 'scene 1 was lifted again'
    batch._scenes[1]._stale = True                         # the sentinel goes: lift scene 1 again
    check([[2, 3], [0, 1]])
    assert not torch.equal(batch._mean[1], torch.zeros_like(keep)) and torch.equal(batch._mean[1], keep)
    batch.remove_views(1, [0])
    held[1] = held[1][1:]
    check([[2, 3], [1]])
    tick([2], [1])                                         # refill: the freed slot of scene 1's part of the ring
    assert sorted(v[1] for v in batch._scenes[1]._views) == [2, 3]
    check([[2, 3], [1, 2]])
    batch.reset(scenes=[1])
    held[1] = []
    check([[2, 3], []])
    tick([1], [1])
    check([[2, 3], [0]])
    assert len(batch.detect()) == 2
    batch.close()


# ------------------------------------------------------------------ ragged one-shot batches
@pytest.mark.parametrize('family,counts', [('indoor', (4, 2)), ('anchor', (2, 1)), ('indoor', (2, 2))], ids=['indoor-4_2', 'anchor-2_1', 'indoor-2_2'])
def test_simple_test_ragged(ia, families, family, counts):
    """Per-sample volume and mask are torch.equal to lift_cl of that sample's slice of the shared features; the results equal the batched
    detection stage on them; equal view counts give simple_test's composition-path results."""
    z = families(family)
    model, E, img = z['model'], z['E'], z['img']
    first = [0, 1]                                          # sample b takes views first[b] .. first[b] + counts[b] - 1
    views = [list(range(first[b], first[b] + counts[b])) for b in range(2)]
    imgs = [img[torch.tensor(v, device='cuda')].contiguous() for v in views]
    sm = _scene_metas(z, 2)
    metas = [_full_meta(sm[b], [E[v] for v in views[b]]) for b in range(2)]
    p0 = model.features_2d_cl(torch.cat(imgs)[None])
    vol, valid = model.lift_ragged_cl(p0, metas, list(counts))
    assert valid.dtype == torch.bool and vol.shape[0] == 2
    start = 0
    for b in range(2):
        rv, rok = model.lift_cl(p0[start:start + counts[b]].contiguous(), [metas[b]])
        assert torch.equal(vol[b:b + 1], rv) and torch.equal(valid[b:b + 1], rok) and 0 < int(rok.sum()) < rok.numel(), b
        start += counts[b]
    assert not torch.equal(valid[0], valid[1])
    ref = _stage(model, vol, valid, metas)
    res = model.simple_test_ragged(imgs, metas)
    assert len(res) == 2 and sum(len(r['scores_3d']) for r in res) > 0
    for i in range(2):
        _same_results([res[i]], [ref[i]])
    if counts[0] == counts[1]:
        x = torch.stack(imgs)
        dense = _stage(model, *model.lift_cl(model.features_2d_cl(x), metas), metas)
        for i in range(2):
            _same_results([res[i]], [dense[i]])
    with pytest.raises(ValueError, match='extrinsics for'):
        model.simple_test_ragged(imgs, [metas[0], _full_meta(sm[1], E[:counts[1] + 1])])
    with pytest.raises(ValueError, match='img_metas for'):
        model.simple_test_ragged(imgs, metas[:1])
