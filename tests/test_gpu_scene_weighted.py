"""-m gpu: fading and weighted scenes (model.open_scene / open_scenes with decay=, add_views(weights=), reweight) on the tiny models of the scene
tests: a session / batch opened with decay=1.0 and fed unit weights holds the bits of a plain one, tick by tick; a decayed session is
ops.backproject_weighted_accum_ driven by hand with the same features; a windowed scene with weights is ops.backproject_weighted_mean_ over the
kept views, its weights survive eviction and slot reuse, and reweight(id, 0.0) is remove_views(id); untouched scenes of a batch do not fade."""
import pytest
import torch

from test_gpu_scene_stream import _same_results
from test_gpu_scene_window import _family

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ia():
    import imvoxelnet_amd
    from imvoxelnet_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    return imvoxelnet_amd


@pytest.fixture(scope='module')
def families(ia):
    cache = {}

    def get(family):
        if family not in cache:
            cache[family] = _family(ia, family)
        return cache[family]
    return get


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _views(z, vs):
    return z['img'][torch.tensor(vs, device='cuda')].contiguous(), [z['E'][v] for v in vs]


CALLS = [[0], [1, 2], [3], [4]]


@pytest.mark.parametrize('family', ['indoor', 'anchor'])
def test_session_opened_with_decay_one_holds_the_bits_of_a_plain_session(ia, families, family):
    """The same calls into a plain session and into one opened with decay=1.0 (unit weights, given or not): after every tick sum, count, mean and
    mask are equal bit for bit and wsum == count; emit=False ticks read through volume_wmean give the same mean; detect() returns the plain
    detect_cl's boxes on that volume."""
    z = families(family)
    model = z['model']
    plain, unit, quiet = model.open_scene(z['scene_meta']), model.open_scene(z['scene_meta'], decay=1.0), model.open_scene(z['scene_meta'], decay=1.0)
    assert plain._decay is None and unit._decay == 1.0
    for t, vs in enumerate(CALLS):
        img, E = _views(z, vs)
        plain.add_views(img, E)
        assert unit.add_views(img, E, weights=[1.0] * len(vs) if t % 2 else None) is unit
        quiet.add_views(img, E, emit=False)
        assert plain._wsum is None and unit._wsum is not None and quiet._stale
        for k in ('_sum', '_count', '_mean', '_valid'):
            assert _same_bits(getattr(unit, k), getattr(plain, k)), (t, k)
        assert torch.equal(unit._wsum, unit._count.float()) and _same_bits(quiet._sum, plain._sum) and _same_bits(quiet._wsum, unit._wsum)
        (vp, okp), (vq, okq) = plain.volume(), quiet.volume()
        assert _same_bits(vq, vp) and torch.equal(okq, okp) and not quiet._stale and 0 < int(okp.sum()) < okp.numel()
    assert unit.n_views == plain.n_views == 5 and unit.view_ids == plain.view_ids
    res, ref = unit.detect(), plain.detect()
    print(family, 'detections', len(ref[0]['scores_3d']))
    assert len(ref[0]['scores_3d']) > 0
    _same_results(res, ref)
    for s in (plain, unit, quiet):
        s.close()
    assert unit._wsum is None


def test_decayed_session_is_the_weighted_lift_driven_by_hand(ia, families):
    """decay = 0.75, forget_below = 0.4, weights per call: the session's state equals ops.backproject_weighted_accum_ called by hand with the
    features the session's trunk calls produced, tick by tick; voxels get forgotten on the way; reset() starts again from zero."""
    from imvoxelnet_amd import ops
    z = families('indoor')
    model = z['model']
    s = model.open_scene(z['scene_meta'], decay=0.75, forget_below=0.4)
    W = [[0.5], [1.5, 0.0], [0.25], [2.0]]
    st, forgot = None, 0
    for t, (vs, w) in enumerate(zip(CALLS, W)):
        img, E = _views(z, vs)
        s.add_views(img, E, weights=w)
        f = s._features(img).clone()                       # the same trunk call again: the same bits
        meta = dict(z['scene_meta'], lidar2img=dict(z['scene_meta']['lidar2img'], extrinsic=E))
        proj, no, crop = model._camera_setup([meta], 4, img.device)
        if st is None:
            X, Y, Z = model.n_voxels
            st = dict(sum=torch.full((1, X, Y, Z, f.shape[-1]), float('nan'), device='cuda'), wsum=torch.full((1, X, Y, Z), float('nan'), device='cuda'),
                      count=torch.full((1, X, Y, Z), 7, device='cuda', dtype=torch.int32), mean=torch.empty((1, X, Y, Z, f.shape[-1]), device='cuda', dtype=f.dtype),
                      valid=torch.empty((1, X, Y, Z), device='cuda', dtype=torch.uint8))
        before = st['count'].clone()
        ops.backproject_weighted_accum_(f, proj[0].contiguous(), [list(range(len(vs)))], w, [0], [t == 0], [0.75], no, crop, model.voxel_size, st['sum'], st['wsum'],
                                        st['count'], st['mean'], st['valid'], forget_below=0.4, sampling=model.sampling)
        if t:
            forgot += int(((before > 0) & (st['count'] == 0)).sum())
        for k in ('sum', 'wsum', 'count', 'mean', 'valid'):
            assert _same_bits(getattr(s, '_' + k), st[k]), (t, k)
        vol, ok = s.volume()
        assert _same_bits(vol, st['mean']) and torch.equal(ok, st['valid'].bool())
    print('voxels forgotten on the way:', forgot)
    assert forgot > 0, 'the threshold must bite for the test to mean anything'
    assert not torch.equal(s._wsum, s._count.float())
    assert len(s.detect()) == 1
    s.reset()
    img, E = _views(z, CALLS[0])
    s.add_views(img, E, weights=W[0])
    fresh = model.open_scene(z['scene_meta'], decay=0.75, forget_below=0.4)
    fresh.add_views(img, E, weights=W[0])
    assert _same_bits(s._sum, fresh._sum) and _same_bits(s._wsum, fresh._wsum) and _same_bits(s._count, fresh._count)
    s.close()
    fresh.close()


def test_windowed_scene_with_weights_and_reweight(ia, families):
    """window = 3: the volume is ops.backproject_weighted_mean_ over the kept views with their weights, bit for bit; the weights survive
    eviction and slot reuse (a reused slot takes its new view's weight, 1 when none is given); reweight(id, 0.0) is remove_views(id) bit for bit;
    without any weight the windowed scene runs the unweighted re-lift (no weight ring)."""
    from imvoxelnet_amd import ops
    z = families('indoor')
    model = z['model']
    win = model.open_scene(z['scene_meta'], window=3)
    feats, given = {}, {0: 0.5, 1: 2.0, 2: 1.25, 3: None, 4: 0.75}

    def add(v):
        img, E = _views(z, [v])
        win.add_views(img, E, weights=None if given[v] is None else [given[v]])
        feats[v] = win._features(img).clone()

    def by_hand(views, weights):
        """One weighted mean lift over a contiguous pool of these views' features, in order."""
        meta = dict(z['scene_meta'], lidar2img=dict(z['scene_meta']['lidar2img'], extrinsic=[z['E'][v] for v in views]))
        proj, no, crop = model._camera_setup([meta], 4, torch.device('cuda'))
        X, Y, Z = model.n_voxels
        pool = torch.cat([feats[v] for v in views]).contiguous()
        vol = torch.empty((1, X, Y, Z, pool.shape[-1]), device='cuda', dtype=pool.dtype)
        valid = torch.empty((1, X, Y, Z), device='cuda', dtype=torch.uint8)
        ops.backproject_weighted_mean_(pool, proj[0].contiguous(), [list(range(len(views)))], weights, [0], no, crop, model.voxel_size, vol, valid,
                                       sampling=model.sampling)
        return vol, valid.bool()

    def check(views, weights):
        vol, ok = win.volume()
        rv, rok = by_hand(views, weights)
        assert _same_bits(vol, rv) and torch.equal(ok, rok) and 0 < int(ok.sum()) < ok.numel()
        return vol.clone()

    for v in (0, 1, 2):
        add(v)
    assert win._wring is not None and [v[1] for v in win._views] == [0, 1, 2]
    a = check([0, 1, 2], [0.5, 2.0, 1.25])
    unit, _ = by_hand([0, 1, 2], None)
    assert not _same_bits(a, unit), 'the weights must matter'
    add(3)                                                # evicts view 0; its slot 0 is reused by view 3, which comes without a weight: 1
    assert win.view_ids == [1, 2, 3] and [v[1] for v in win._views] == [1, 2, 0] and win._wring == [1.0, 2.0, 1.25]
    check([1, 2, 3], [2.0, 1.25, 1.0])
    add(4)                                                # evicts view 1; slot 1 now carries view 4's weight
    assert win.view_ids == [2, 3, 4] and win._wring == [1.0, 0.75, 1.25]
    b = check([2, 3, 4], [1.25, 1.0, 0.75])
    # reweight
    assert win.reweight([3, 2], [4.0, 0.5]) is win and win._stale
    c = check([2, 3, 4], [0.5, 4.0, 0.75])
    assert not _same_bits(b, c)
    win.reweight(3, 0.0)
    zero = check([2, 3, 4], [0.5, 0.0, 0.75])
    det_zero = win.detect()
    win.remove_views(3)
    assert win.view_ids == [2, 4]
    removed, _ = win.volume()
    assert _same_bits(removed, zero), 'a view of weight 0 is the view removed'
    _same_results(win.detect(), det_zero)
    check([2, 4], [0.5, 0.75])
    with pytest.raises(KeyError):
        win.reweight([3], [1.0])
    win.close()
    # never given a weight: today's path, no ring of weights, and the same bits as unit weights
    plain = model.open_scene(z['scene_meta'], window=3)
    for v in (0, 1, 2):
        img, E = _views(z, [v])
        plain.add_views(img, E)
    assert plain._wring is None
    assert _same_bits(plain.volume()[0], unit)
    plain.close()


def test_batch_with_decay_one_holds_the_bits_of_a_plain_batch_and_untouched_scenes_do_not_fade(ia, families):
    """Three scenes, ticks that touch subsets.  decay=1.0 with unit weights: the pools of a plain batch, bit for bit, tick by tick, and detect()
    as the plain batch's.  decay=[0.5, 0.75, 0.5]: a scene that a tick does not touch keeps every bit of its row (it does not fade); a touched one
    equals the weighted lift driven by hand on its row."""
    from imvoxelnet_amd import ops
    z = families('indoor')
    model = z['model']
    metas = [z['scene_meta']] * 3
    ticks = [([0, 1, 2], [0, 0, 2]), ([3, 4], [1, 2]), ([2], [0])]
    plain, unit = model.open_scenes(metas), model.open_scenes(metas, decay=1.0)
    for vs, sc in ticks:
        img, E = _views(z, vs)
        plain.add_views(img, E, sc)
        unit.add_views(img, E, sc, weights=[1.0] * len(vs))
        for s in sorted(set(sc)):
            for k in ('_sum', '_count', '_mean', '_valid'):
                assert _same_bits(getattr(unit, k)[s], getattr(plain, k)[s]), (vs, s, k)
            assert torch.equal(unit._wsum[s], unit._count[s].float())
    ref, res = plain.detect(), unit.detect()
    assert len(res) == 3 and sum(len(r['scores_3d']) for r in ref) > 0
    for i in range(3):
        _same_results([res[i]], [ref[i]])
    plain.close()
    unit.close()
    # a fading batch
    decays = [0.5, 0.75, 0.5]
    fb = model.open_scenes(metas, decay=decays, forget_below=0.2)
    hand = None
    seen = [0, 0, 0]
    for t, (vs, sc) in enumerate(ticks):
        img, E = _views(z, vs)
        w = [0.5 + 0.25 * i for i in range(len(vs))]
        keep = None if fb._sum is None else {k: getattr(fb, k).clone() for k in ('_sum', '_wsum', '_count', '_mean', '_valid')}
        fb.add_views(img, E, sc, weights=w)
        f = fb._features(img).clone()
        touched = sorted(set(sc))
        if keep is not None:
            for s in range(3):
                if s not in touched:
                    for k, v in keep.items():
                        assert _same_bits(getattr(fb, k)[s], v[s]), f'tick {t}: scene {s} was not touched and must keep its bits ({k})'
        if hand is None:
            hand = {k: torch.full_like(getattr(fb, '_' + k), 3) for k in ('sum', 'wsum', 'count', 'mean', 'valid')}
        proj_rows, nos, crops = [], [], []
        for s in touched:
            mine = [i for i, q in enumerate(sc) if q == s]
            meta = dict(metas[s], lidar2img=dict(metas[s]['lidar2img'], extrinsic=[E[i] for i in mine]))
            proj, no, crop = model._camera_setup([meta], 4, img.device)
            proj_rows.append((mine, proj[0]))
            nos.append(no)
            crops.append(crop)
        ppool = torch.empty((len(vs), 3, 4), device='cuda')
        for mine, p in proj_rows:
            ppool[torch.tensor(mine, device='cuda')] = p
        ops.backproject_weighted_accum_(f, ppool, [[i for i, q in enumerate(sc) if q == s] for s in touched], w, touched, [seen[s] == 0 for s in touched],
                                        [decays[s] for s in touched], torch.cat(nos).contiguous(), torch.cat(crops).contiguous(), model.voxel_size, hand['sum'],
                                        hand['wsum'], hand['count'], hand['mean'], hand['valid'], forget_below=0.2, sampling=model.sampling)
        for s in touched:
            seen[s] += 1
            for k in hand:
                assert _same_bits(getattr(fb, '_' + k)[s], hand[k][s]), (t, s, k)
    assert fb.n_views == [3, 1, 2] and len(fb.detect()) == 3
    fb.close()
