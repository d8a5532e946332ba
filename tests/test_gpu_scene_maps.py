"""-m gpu: pixel maps on streaming scenes (open_scene / open_scenes with depth_gate=, add_views(pixel_weights=, depths=)) on the tiny indoor model of
the scene tests: a fading session with maps is ops.backproject_mapped_accum_ driven by hand, and a map at the input size gives the bits of its
strided pick; a session opened with depth_gate that never sees a map holds the bits of one opened without; a windowed scene's maps travel with
their slots through eviction, remove_views, slot reuse without a map and a scroll; the batch forms hold the sessions' volumes."""
import pytest
import torch

import ref_volume_scroll as RS
from test_gpu_scene_scroll import _meta_at
from test_gpu_scene_weighted import _same_bits, _views
from test_gpu_scene_window import _family

pytestmark = pytest.mark.gpu

GATE = (0.5, 0.75)
STATE = ('_sum', '_wsum', '_count', '_mean', '_valid')


@pytest.fixture(scope='module')
def indoor():
    import imvoxelnet_amd
    from imvoxelnet_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    z = _family(imvoxelnet_amd, 'indoor')
    H, W = z['img'].shape[2:]
    FH, FW = z['model'].open_scene(z['scene_meta'])._features(z['img'][:1]).shape[-3:-1]
    s = H // FH
    assert s >= 2 and (FH * s, FW * s) == (H, W)
    g = torch.Generator().manual_seed(41)
    # at the input size, on the host: confidences in [0.25, 1.75) with blocked pixels (0, NaN), depths in [0.5, 3.5) with holes (0, NaN, -1, inf)
    pw = 0.25 + 1.5 * torch.rand(5, H, W, generator=g)
    dp = 0.5 + 3.0 * torch.rand(5, H, W, generator=g)
    kind = torch.randint(0, 16, (5, H, W), generator=g)
    pw[kind == 0], pw[kind == 1] = 0.0, float('nan')
    for k, v in ((2, 0.0), (3, float('nan')), (4, -1.0), (5, float('inf'))):
        dp[kind == k] = v
    z.update(full=(pw, dp), feat=(pw[:, ::s, ::s].contiguous().cuda(), dp[:, ::s, ::s].contiguous().cuda()), stride=s)
    return z


def _maps(z, vs, which='feat', use=(True, True)):
    idx = torch.tensor(vs)
    return {name: (m[idx.to(m.device)].contiguous() if u else None) for name, m, u in zip(('pixel_weights', 'depths'), z[which], use)}


def _hand_state(model, f):
    X, Y, Z = model.n_voxels
    return dict(sum=torch.full((1, X, Y, Z, f.shape[-1]), float('nan'), device='cuda'), wsum=torch.full((1, X, Y, Z), float('nan'), device='cuda'),
                count=torch.full((1, X, Y, Z), 7, device='cuda', dtype=torch.int32), mean=torch.empty((1, X, Y, Z, f.shape[-1]), device='cuda', dtype=f.dtype),
                valid=torch.empty((1, X, Y, Z), device='cuda', dtype=torch.uint8))


CALLS = [[0], [1, 2], [3], [4]]
USE = [(True, True), (True, False), (False, False), (False, True)]        # which maps each call brings
WEIGHTS = [[0.5], [1.5, 0.75], None, [2.0]]


def test_fading_session_with_maps_is_the_mapped_lift_driven_by_hand(indoor):
    """decay 0.75, forget_below 0.3, depth_gate (0.5, 0.75); the calls bring both maps, the weights alone, nothing, the depths alone.  The session's
    state equals ops.backproject_mapped_accum_ (backproject_weighted_accum_ for the call without maps) called by hand on the same features, tick by
    tick; a second session fed the maps at the input size, from the host, holds the same bits (the strided pick); the session keeps no map."""
    from imvoxelnet_amd import ops
    z, model = indoor, indoor['model']
    s, big = (model.open_scene(z['scene_meta'], decay=0.75, forget_below=0.3, depth_gate=GATE) for _ in range(2))
    plain = model.open_scene(z['scene_meta'], decay=0.75, forget_below=0.3)
    st = None
    for t, (vs, use, w) in enumerate(zip(CALLS, USE, WEIGHTS)):
        img, E = _views(z, vs)
        m = _maps(z, vs, 'feat', use)
        assert s.add_views(img, E, weights=w, **m) is s
        big.add_views(img, E, weights=w, **_maps(z, vs, 'full', use))
        plain.add_views(img, E, weights=w)
        f = s._features(img).clone()
        proj, no, crop = model._camera_setup([_meta_at(z, z['scene_meta']['lidar2img']['origin'], E)], 4, img.device)
        st = st or _hand_state(model, f)
        args = (f, proj[0].contiguous(), [list(range(len(vs)))], w, [0], [t == 0], [0.75], no, crop, model.voxel_size, st['sum'], st['wsum'], st['count'], st['mean'],
                st['valid'])
        if any(use):
            ops.backproject_mapped_accum_(*args, forget_below=0.3, sampling=model.sampling, pixel_weight=m['pixel_weights'], depth=m['depths'], gate=GATE)
        else:
            ops.backproject_weighted_accum_(*args, forget_below=0.3, sampling=model.sampling)
        for k in STATE:
            assert _same_bits(getattr(s, k), st[k[1:]]), (t, k)
            assert _same_bits(getattr(big, k), st[k[1:]]), (t, k, 'maps at the input size')
        vol, ok = s.volume()
        assert _same_bits(vol, st['mean']) and 0 < int(ok.sum()) < ok.numel()
    assert not _same_bits(s._count, plain._count) and not _same_bits(s._mean, plain._mean), 'the maps must matter'
    assert s._mring is None and s._dring is None and s._ring is None
    assert len(s.detect()) == 1
    for x in (s, big, plain):
        x.close()


def test_a_gate_that_never_sees_a_map_changes_nothing(indoor):
    """Sessions opened with depth_gate but never given a map -- fading and windowed -- hold the bits of sessions opened without it."""
    z, model = indoor, indoor['model']
    for kw in (dict(decay=0.75, forget_below=0.3), dict(window=3)):
        a, b = model.open_scene(z['scene_meta'], depth_gate=GATE, **kw), model.open_scene(z['scene_meta'], **kw)
        for vs, w in zip(CALLS, WEIGHTS):
            img, E = _views(z, vs)
            a.add_views(img, E, weights=w)
            b.add_views(img, E, weights=w)
            (va, oka), (vb, okb) = a.volume(), b.volume()
            assert _same_bits(va, vb) and torch.equal(oka, okb)
            if 'decay' in kw:
                for k in STATE:
                    assert _same_bits(getattr(a, k), getattr(b, k)), k
        assert a._mring is None and a._dring is None
        a.close()
        b.close()


def _by_hand_mean(z, model, feats, views, weights, origin, maps_of):
    """One mapped mean lift over a contiguous pool of these views' features and maps, in order, at this origin."""
    from imvoxelnet_amd import ops
    proj, no, crop = model._camera_setup([_meta_at(z, origin, [z['E'][v] for v in views])], 4, torch.device('cuda'))
    X, Y, Z = model.n_voxels
    pool = torch.cat([feats[v] for v in views]).contiguous()
    vol = torch.empty((1, X, Y, Z, pool.shape[-1]), device='cuda', dtype=pool.dtype)
    valid = torch.empty((1, X, Y, Z), device='cuda', dtype=torch.uint8)
    pw, dp = (torch.stack([maps_of[v][i] for v in views]).contiguous() for i in range(2))
    ops.backproject_mapped_mean_(pool, proj[0].contiguous(), [list(range(len(views)))], weights, [0], no, crop, model.voxel_size, vol, valid, sampling=model.sampling,
                                 pixel_weight=pw, depth=dp, gate=GATE)
    return vol, valid.bool()


def _neutral(z):
    return torch.ones_like(z['feat'][0][0]), torch.zeros_like(z['feat'][1][0])


def test_windowed_scene_maps_travel_with_their_slots(indoor):
    """window = 3, depth_gate (0.5, 0.75).  Views 0 (both maps), 1 (depths), 2 (weights + a view weight), then 3 without any map, which evicts view 0
    and reuses its slot -- the slot's maps go back to 1 / 0 --, then remove_views(1), then view 4 with both maps into the freed slot, then a scroll:
    every time volume() is bit for bit ONE ops.backproject_mapped_mean_ over the kept views with their maps (ones / zeros for a view that brought
    none) on a contiguous pool, at the scene's origin."""
    z, model = indoor, indoor['model']
    win = model.open_scene(z['scene_meta'], window=3, depth_gate=GATE)
    ones, zeros = _neutral(z)
    use = {0: (True, True), 1: (False, True), 2: (True, False), 3: (False, False), 4: (True, True)}
    weight = {0: None, 1: None, 2: 1.5, 3: None, 4: 0.5}
    maps_of = {v: (z['feat'][0][v] if u[0] else ones, z['feat'][1][v] if u[1] else zeros) for v, u in use.items()}
    feats = {}
    origin = z['scene_meta']['lidar2img']['origin']

    def add(v):
        img, E = _views(z, [v])
        win.add_views(img, E, weights=None if weight[v] is None else [weight[v]], **_maps(z, [v], 'full' if v % 2 else 'feat', use[v]))
        feats[v] = win._features(img).clone()

    def check(views, origin=origin):
        vol, ok = win.volume()
        rv, rok = _by_hand_mean(z, model, feats, views, [1.0 if weight[v] is None else weight[v] for v in views], origin, maps_of)
        assert _same_bits(vol, rv) and torch.equal(ok, rok) and 0 < int(ok.sum()) < ok.numel(), views
        return vol.clone()

    add(0)
    assert win._mring is not None and win._dring is not None and win._wring is None and tuple(win._mring.shape) == (3,) + tuple(ones.shape)
    add(1)
    add(2)
    a = check([0, 1, 2])
    ungated, _ = _by_hand_mean(z, model, feats, [0, 1, 2], [1.0, 1.0, 1.5], origin, {v: (ones, zeros) for v in range(3)})
    assert not _same_bits(a, ungated), 'the maps must matter'
    add(3)                                                    # evicts view 0; slot 0 is reused by a view without maps
    assert win.view_ids == [1, 2, 3] and [v[1] for v in win._views] == [1, 2, 0]
    assert bool((win._mring[0] == 1).all()) and bool((win._dring[0] == 0).all()) and _same_bits(win._dring[1], z['feat'][1][1])
    check([1, 2, 3])
    win.remove_views(1)
    check([2, 3])
    add(4)                                                    # into the freed slot 1, maps at the input size
    assert [v[1] for v in win._views] == [2, 0, 1] and _same_bits(win._mring[1], z['feat'][0][4]) and _same_bits(win._dring[1], z['feat'][1][4])
    b = check([2, 3, 4])
    shift = (2, -1, 1)
    win.scroll(shift)
    c = check([2, 3, 4], RS.scrolled_origin(origin, shift, model.voxel_size))
    assert not _same_bits(b, c)
    assert len(win.detect()) == 1
    win.close()
    assert win._mring is None and win._dring is None


@pytest.mark.parametrize('kw', [dict(decay=[0.75, 0.5], forget_below=0.3), dict(window=2)], ids=['fading', 'windowed'])
def test_batch_forms_hold_the_sessions_volumes(indoor, kw):
    """Two scenes, ticks that touch both, one, both: every scene's volume in the batch is bit for bit the volume of a session of the same kind that
    is fed the batch's features for its views with the same weights and maps, tick by tick (the windowed batch evicts per scene)."""
    z, model = indoor, indoor['model']
    metas = [z['scene_meta']] * 2
    ticks = [([0, 1, 2], [0, 1, 0]), ([3], [1]), ([4, 0], [0, 1]), ([1], [1])]
    use = [(True, True), (True, False), (False, True), (False, False)]
    batch = model.open_scenes(metas, depth_gate=GATE, **kw)
    per_scene = [dict(kw, decay=kw['decay'][s]) if 'decay' in kw else kw for s in range(2)]
    sessions = [model.open_scene(metas[s], depth_gate=GATE, **per_scene[s]) for s in range(2)]
    for t, ((vs, sc), u) in enumerate(zip(ticks, use)):
        img, E = _views(z, vs)
        w = [0.5 + 0.25 * i for i in range(len(vs))]
        m = _maps(z, vs, 'full' if t == 0 else 'feat', u)
        assert batch.add_views(img, E, sc, weights=w, **m) is batch
        f = batch._features(img).clone()
        for s in sorted(set(sc)):
            mine = [i for i, q in enumerate(sc) if q == s]
            sessions[s]._features = lambda _img, f=f[torch.tensor(mine, device='cuda')].contiguous(): f
            sessions[s].add_views(img[torch.tensor(mine, device='cuda')].contiguous(), [E[i] for i in mine], weights=[w[i] for i in mine],
                                  **{k: (None if v is None else v[torch.tensor(mine).to(v.device)].contiguous()) for k, v in m.items()})
        for s in range(2):
            (vb, okb), (vs_, oks) = batch.volume(s), sessions[s].volume()
            assert _same_bits(vb, vs_) and torch.equal(okb, oks) and 0 < int(okb.sum()) < okb.numel(), (t, s)
    if 'window' in kw:
        assert tuple(batch._mring.shape[:1]) == (4,) and batch._dring is not None and batch.n_views == [2, 2]
    else:
        assert batch._mring is None and batch._dring is None
        for s in range(2):
            assert _same_bits(batch._wsum[s:s + 1], sessions[s]._wsum) and _same_bits(batch._count[s:s + 1], sessions[s]._count)
    assert len(batch.detect()) == 2
    batch.close()
    for s in sessions:
        s.close()
