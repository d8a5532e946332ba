"""-m gpu: scrolling scenes (SceneSession.scroll / scroll_to, SceneBatch.scroll) on the tiny models of the scene tests.  A scrolled session is
ops.volume_scroll_ plus the existing lift at the scrolled origin, driven by hand with the features the session's trunk produced, bit for bit; an
empty session scrolled is a session opened at the new origin; a windowed session re-lifts its kept views there; a batch moves the named scenes'
rows in one call and leaves the others alone; a call that raises changes nothing; the anchor family refuses."""
import numpy as np
import pytest
import torch

import ref_volume_scroll as RS
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
def indoor(ia):
    return _family(ia, 'indoor')


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _views(z, vs):
    return z['img'][torch.tensor(vs, device='cuda')].contiguous(), [z['E'][v] for v in vs]


def _meta_at(z, origin, E=None):
    l2i = dict(z['scene_meta']['lidar2img'], origin=origin)
    if E is not None:
        l2i['extrinsic'] = list(E)
    return dict(z['scene_meta'], lidar2img=l2i)


SHIFT = (3, -2, 1)
STATE = ('_sum', '_count', '_wsum', '_mean', '_valid')


@pytest.mark.parametrize('decay', [None, 0.75], ids=['plain', 'decay0.75'])
def test_session_add_scroll_add_is_the_ops_driven_by_hand(ia, indoor, decay):
    """Add, scroll, add.  By hand: clone the state after the first add, apply ops.volume_scroll_, then run the existing accumulate op at the scrolled
    origin with the features the session's trunk produced.  Sum, count, weight sum, mean and mask are equal bit for bit; between the scroll and
    the second add the session's volume() is the mean of the moved state; the meta's origin follows the rule; detect() runs and returns boxes."""
    from imvoxelnet_amd import ops, scrolled_origin
    z, model = indoor, indoor['model']
    kw = {} if decay is None else dict(decay=decay)
    s = model.open_scene(z['scene_meta'], **kw)
    img0, E0 = _views(z, [0, 1, 2])
    s.add_views(img0, E0)
    hand = {k: getattr(s, k).clone() for k in STATE if getattr(s, k) is not None}
    assert ('_wsum' in hand) == (decay is not None)
    o = z['scene_meta']['lidar2img']['origin']
    assert s.scroll(SHIFT) is s and s.scrolled == SHIFT and s._stale
    o2 = RS.scrolled_origin(o, SHIFT, model.voxel_size)
    got = s.meta['lidar2img']['origin']
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and np.array_equal(got, o2) and np.array_equal(got, scrolled_origin(o, SHIFT, model.voxel_size))
    assert np.array_equal(z['scene_meta']['lidar2img']['origin'], o), 'the caller\'s meta stays as it was'
    ops.volume_scroll_(hand['_sum'], hand['_count'], [0], [SHIFT], hand.get('_wsum'))
    for k in ('_sum', '_count', '_wsum'):
        if k in hand:
            assert _same_bits(getattr(s, k), hand[k]), k
    inside = torch.from_numpy(RS.stayed_inside(model.n_voxels, SHIFT)).cuda()
    assert not bool(s._count[0][~inside].any()) and int((s._count[0][inside] > 0).sum()) > 100
    vol, ok = s.volume()                                                  # stale: the existing refresh of the moved state; a scroll is not a tick
    if decay is None:
        mean, valid = ops.volume_mean(hand['_sum'], hand['_count'], vol.dtype)
    else:
        mean, valid = ops.volume_wmean(hand['_sum'], hand['_wsum'], vol.dtype)
    assert _same_bits(vol, mean) and torch.equal(ok, valid) and not s._stale and not bool(ok[0][~inside].any())
    # the second add: the existing lift at the new origin
    img1, E1 = _views(z, [3, 4])
    s.add_views(img1, E1)
    f = s._features(img1).clone()                                         # the same trunk call again: the same bits
    proj, no, crop = model._camera_setup([_meta_at(z, o2, E1)], 4, img1.device)
    assert _same_bits(s._origin, no)
    hand['_mean'], hand['_valid'] = torch.empty_like(s._mean), torch.empty_like(s._valid)
    if decay is None:
        ops.backproject_accum_(f, proj, no, crop, model.voxel_size, hand['_sum'], hand['_count'], False, hand['_mean'], hand['_valid'], sampling=model.sampling)
    else:
        ops.backproject_weighted_accum_(f, proj[0].contiguous(), [[0, 1]], None, [0], [False], [decay], no, crop, model.voxel_size, hand['_sum'], hand['_wsum'],
                                        hand['_count'], hand['_mean'], hand['_valid'], sampling=model.sampling)
    for k, v in hand.items():
        assert _same_bits(getattr(s, k), v), k
    assert s.n_views == 5 and int(s._count.max()) <= 5
    res = s.detect()
    assert len(res) == 1 and len(res[0]['boxes_3d'].tensor) == len(res[0]['scores_3d'])
    print('decay', decay, 'detections after the scroll:', len(res[0]['scores_3d']))
    assert len(res[0]['scores_3d']) > 0
    s.close()


def test_scrolling_an_empty_session_is_opening_at_the_new_origin(ia, indoor):
    """No views, no launch: only the origin changes, and every later add is the lift there -- state, volume and boxes of a session opened at
    scrolled_origin.  scroll_to brings the same session there as well."""
    z, model = indoor, indoor['model']
    o = z['scene_meta']['lidar2img']['origin']
    o2 = RS.scrolled_origin(o, SHIFT, model.voxel_size)
    img, E = _views(z, [0, 1, 2, 3, 4])
    a, b, c = model.open_scene(z['scene_meta']), model.open_scene(_meta_at(z, o2)), model.open_scene(z['scene_meta'])
    a.scroll(SHIFT)
    assert a._sum is None and a._origin is None
    assert c.scroll_to(o2.astype(np.float64) + np.array([0.4, -0.4, 0.3]) * np.asarray(model.voxel_size)) == SHIFT and c.scrolled == SHIFT
    for s in (a, b, c):
        s.add_views(img, E)
    for s in (a, c):
        for k in ('_sum', '_count', '_mean', '_valid', '_origin'):
            assert _same_bits(getattr(s, k), getattr(b, k)), k
        _same_results(s.detect(), b.detect())
    plain = model.open_scene(z['scene_meta'])
    plain.add_views(img, E)
    assert not _same_bits(plain._count, a._count), 'the scroll must show'
    for s in (a, b, c, plain):
        s.close()


def test_windowed_session_relifts_its_kept_views_at_the_new_origin(ia, indoor):
    """window = 3: nothing to move.  After scroll, volume() is ops.backproject_mean of the ring's kept maps at the scrolled origin, bit for bit --
    before and after a further arrival evicts the oldest view."""
    from imvoxelnet_amd import ops
    z, model = indoor, indoor['model']
    win = model.open_scene(z['scene_meta'], window=3)
    feats = {}

    def add(v):
        img, E = _views(z, [v])
        win.add_views(img, E)
        feats[v] = win._features(img).clone()

    def by_hand(views, origin):
        proj, no, crop = model._camera_setup([_meta_at(z, origin, [z['E'][v] for v in views])], 4, torch.device('cuda'))
        return ops.backproject_mean(torch.cat([feats[v] for v in views]).contiguous(), proj, no, crop, model.voxel_size, model.n_voxels, sampling=model.sampling)

    for v in (0, 1, 2):
        add(v)
    o = z['scene_meta']['lidar2img']['origin']
    before = win.volume()[0].clone()
    assert _same_bits(before, by_hand([0, 1, 2], o)[0]) and not win._stale
    win.scroll(SHIFT)
    o2 = RS.scrolled_origin(o, SHIFT, model.voxel_size)
    assert win._stale and win._sum is None and np.array_equal(win.meta['lidar2img']['origin'], o2)
    vol, ok = win.volume()
    rv, rok = by_hand([0, 1, 2], o2)
    assert _same_bits(vol, rv) and torch.equal(ok, rok) and 0 < int(ok.sum()) < ok.numel() and not _same_bits(vol, before)
    add(3)                                                                # evicts view 0
    vol, ok = win.volume()
    rv, rok = by_hand([1, 2, 3], o2)
    assert _same_bits(vol, rv) and torch.equal(ok, rok)
    assert len(win.detect()) == 1
    win.close()


@pytest.mark.parametrize('decay', [None, 0.75], ids=['plain', 'decay0.75'])
def test_batch_scrolls_the_named_scenes_rows_and_no_others(ia, indoor, decay):
    """Three scenes with views.  scroll([2, 0], two shifts): the rows of scene 1 keep every bit in every pool; rows 2 and 0 equal the single-row op on
    a clone; metas and host camera records follow the rule; the next tick on scene 0 is the lift at its new origin, by hand; raising calls (bad index,
    non-integer shift, a scene named twice) change nothing."""
    from imvoxelnet_amd import ops
    z, model = indoor, indoor['model']
    kw = {} if decay is None else dict(decay=decay)
    b = model.open_scenes([z['scene_meta']] * 3, **kw)
    img, E = _views(z, [0, 1, 2, 3])
    b.add_views(img, E, [0, 1, 2, 1])
    pools = [k for k in STATE if getattr(b, k) is not None]
    keep = {k: getattr(b, k).clone() for k in pools}
    o = z['scene_meta']['lidar2img']['origin']
    for scenes, voxels, exc in (([2, 3], [(1, 0, 0), (1, 0, 0)], ValueError), ([2, 0], [(1, 0, 0), (0, 0.5, 0)], TypeError), ([2, 2], [(1, 0, 0), (0, 1, 0)], ValueError)):
        with pytest.raises(exc):
            b.scroll(scenes, voxels)
    for k in pools:
        assert _same_bits(getattr(b, k), keep[k]), k
    assert all(np.array_equal(m['lidar2img']['origin'], o) for m in b.metas) and [b.scrolled(i) for i in range(3)] == [(0, 0, 0)] * 3
    shifts = {2: (3, -2, 1), 0: (-4, 0, 2)}
    assert b.scroll([2, 0], [shifts[2], shifts[0]]) is b
    hand = {k: keep[k].clone() for k in ('_sum', '_count', '_wsum') if k in keep}
    for s in (2, 0):                                                      # the single-row op, one call per scene
        ops.volume_scroll_(hand['_sum'][s:s + 1], hand['_count'][s:s + 1], [0], [shifts[s]], hand['_wsum'][s:s + 1] if '_wsum' in hand else None)
    for k in pools:
        assert _same_bits(getattr(b, k)[1], keep[k][1]), (k, 'scene 1 was not named')
    for k in hand:
        assert _same_bits(getattr(b, k), hand[k]), k
        assert not _same_bits(getattr(b, k)[0], keep[k][0]) and not _same_bits(getattr(b, k)[2], keep[k][2])
    for s in (0, 2):
        o2 = RS.scrolled_origin(o, shifts[s], model.voxel_size)
        assert np.array_equal(b.metas[s]['lidar2img']['origin'], o2) and b.scrolled(s) == shifts[s]
        assert torch.equal(b._cam[s][0], model._new_origin(o2)) and b._scenes[s]._stale
        vol, ok = b.volume(s)
        mean, valid = (ops.volume_mean(hand['_sum'][s:s + 1], hand['_count'][s:s + 1], vol.dtype) if decay is None else
                       ops.volume_wmean(hand['_sum'][s:s + 1], hand['_wsum'][s:s + 1], vol.dtype))
        assert _same_bits(vol, mean) and torch.equal(ok, valid)
    assert np.array_equal(b.metas[1]['lidar2img']['origin'], o) and not b._scenes[1]._stale
    # the next tick: scene 0 gets a view at its new origin, scene 1 one at its old
    img1, E1 = _views(z, [4, 2])
    b.add_views(img1, E1, [0, 1])
    f = b._features(img1).clone()
    proj, no, crop = model._camera_setup([_meta_at(z, RS.scrolled_origin(o, shifts[0], model.voxel_size), E1[:1])], 4, img1.device)
    row = {k: hand[k][0:1].clone() for k in hand}
    mean, valid = torch.empty_like(b._mean[0:1]), torch.empty_like(b._valid[0:1])
    if decay is None:
        ops.backproject_accum_(f[0:1].contiguous(), proj, no, crop, model.voxel_size, row['_sum'], row['_count'], False, mean, valid, sampling=model.sampling)
    else:
        ops.backproject_weighted_accum_(f[0:1].contiguous(), proj[0].contiguous(), [[0]], None, [0], [False], [decay], no, crop, model.voxel_size, row['_sum'], row['_wsum'],
                                        row['_count'], mean, valid, sampling=model.sampling)
    for k in row:
        assert _same_bits(getattr(b, k)[0:1], row[k]), k
    assert _same_bits(b._mean[0:1], mean) and _same_bits(b._valid[0:1], valid)
    assert len(b.detect()) == 3
    b.close()


def test_a_raising_scroll_leaves_the_session_as_it_was(ia, indoor):
    z, model = indoor, indoor['model']
    s = model.open_scene(z['scene_meta'], decay=0.9)
    img, E = _views(z, [0, 1])
    s.add_views(img, E)
    keep = {k: getattr(s, k).clone() for k in STATE}
    o = s.meta['lidar2img']['origin']
    for bad, exc in (((1.5, 0, 0), TypeError), ((1, 0), ValueError), ((2 ** 31, 0, 0), ValueError), (None, TypeError)):
        with pytest.raises(exc):
            s.scroll(bad)
    s.scroll((0, 0, 0))                                                   # and a zero shift is no scroll at all
    for k in STATE:
        assert _same_bits(getattr(s, k), keep[k]), k
    assert s.meta['lidar2img']['origin'] is o and s.scrolled == (0, 0, 0) and not s._stale
    s.close()
    with pytest.raises(RuntimeError, match='closed'):
        s.scroll((1, 0, 0))


def test_anchor_family_refuses(ia):
    """An Anchor3DHead has its anchors fixed in the LiDAR frame: scroll raises NotImplementedError and the session goes on as before."""
    z = _family(ia, 'anchor')
    s = z['model'].open_scene(z['scene_meta'])
    img, E = _views(z, [0, 1])
    s.add_views(img, E)
    keep, ref = s._sum.clone(), s.detect()
    with pytest.raises(NotImplementedError, match='anchors'):
        s.scroll((1, 0, 0))
    b = z['model'].open_scenes([z['scene_meta']] * 2)
    with pytest.raises(NotImplementedError, match='anchors'):
        b.scroll(0, (0, 1, 0))
    assert _same_bits(s._sum, keep) and s.scrolled == (0, 0, 0)
    _same_results(s.detect(), ref)
    s.close()
    b.close()
