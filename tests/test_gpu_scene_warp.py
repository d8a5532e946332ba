"""-m gpu: warping scenes (SceneSession.warp, SceneBatch.warp) on the tiny models of the scene tests.  A fading session's state after a warp is
the reference resample (tests/ref_volume_warp.py) of its state before, within the bound, and detect() runs; the anchor family warps and keeps its
origin; a windowed session is bit for bit a fresh windowed session fed the warped extrinsics; a plain session refuses and goes on; a batch warps the
named scenes and leaves the others' rows alone; a session that never warps never calls ops.volume_warp."""
import numpy as np
import pytest
import torch

import ref_volume_warp as RW
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


@pytest.fixture(scope='module')
def anchor(ia):
    return _family(ia, 'anchor')


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _views(z, vs):
    return z['img'][torch.tensor(vs, device='cuda')].contiguous(), [z['E'][v] for v in vs]


def _motion(model, yaw=0.12, pitch=0.01):
    """A turn about the vertical through the grid's centre plus (0.7, -0.4, 0.2) voxels: what a robot does between two frames, exaggerated."""
    return lambda origin: RW.rigid(yaw, pitch, 0.0, np.array([0.7, -0.4, 0.2]) * np.asarray(model.voxel_size), np.asarray(origin, np.float64))


STATE = ('_sum', '_wsum', '_count')


def _state_against_reference(model, before, after, origin, T, forget, what):
    """The three state fields after a warp against ref_volume_warp of the fields before -> the worst ratios."""
    new_origin = model._new_origin(origin).numpy()
    ref = RW.warp_grid(before[0][0], before[1][0], before[2][0], model.voxel_size, new_origin, np.asarray(T, np.float64).astype(np.float32), forget)
    rs, rw = RW.worst_ratio(after[0][0], ref['S'], ref['bound_S']), RW.worst_ratio(after[1][0], ref['W'], ref['bound_W'])
    print(f'{what}: worst |got - ref| / bound  sums {rs:.3f}  weight sum {rw:.3f}; seen before {int((before[1][0] > 0).sum())}, after {int((ref["W"] > 0).sum())} '
          f'of {ref["W"].size}')
    assert np.array_equal(after[2][0], ref['cnt']) and rs <= 1 and rw <= 1, (what, rs, rw)
    return ref


def test_fading_session_state_after_a_warp_is_the_reference_resample(ia, indoor):
    """Three views, a warp, then volume(): state and mean follow the reference within the bound; frame, extrinsics and staleness follow the rules; the
    origin does not move; a further add and detect() run in the new frame and return finite boxes.  The twin appears with the first warp and the
    second warp swaps back into the first buffers."""
    from imvoxelnet_amd import ops, warped_extrinsic
    z, model = indoor, indoor['model']
    o = z['scene_meta']['lidar2img']['origin']
    s = model.open_scene(z['scene_meta'], decay=0.8)
    img0, E0 = _views(z, [0, 1, 2])
    s.add_views(img0, E0)
    assert s._twin is None
    first = tuple(getattr(s, k) for k in STATE)
    before = [t.cpu().numpy().copy() for t in first]
    keep_origin = s._origin.clone()
    T = _motion(model)(o)
    assert s.warp(T) is s and s._stale and np.array_equal(s.frame, T)
    assert s._twin is not None and all(a is b for a, b in zip(s._twin, first)), 'the old state is the twin now'
    after = [getattr(s, k).cpu().numpy() for k in STATE]
    ref = _state_against_reference(model, before, after, o, T, 0.0, 'fading session')
    assert 0.3 < (ref['W'] > 0).mean() < 1 and (ref['read'].sum(-1) == 8).any()
    assert _same_bits(s._origin, keep_origin) and np.array_equal(s.meta['lidar2img']['origin'], o)
    ext = s.meta['lidar2img']['extrinsic']
    assert len(ext) == 3 and all(e.dtype == np.float32 and np.array_equal(e, warped_extrinsic(E0[i], T)) for i, e in enumerate(ext))
    vol, ok = s.volume()                                                      # the existing refresh of the resampled state
    mean, valid = ops.volume_wmean(s._sum, s._wsum, vol.dtype)
    assert _same_bits(vol, mean) and torch.equal(ok, valid) and not s._stale
    assert torch.equal(ok.cpu(), torch.from_numpy(ref['W'] > 0)[None])
    # the caller goes on in the new frame: its extrinsics are warped_extrinsic of what they would have been
    img1, E1 = _views(z, [3, 4])
    s.add_views(img1, [warped_extrinsic(e, T) for e in E1])
    res = s.detect()
    n = len(res[0]['scores_3d'])
    print('detections after the warp:', n)
    assert n > 0 and bool(torch.isfinite(res[0]['boxes_3d'].tensor).all()) and bool(torch.isfinite(res[0]['scores_3d']).all())
    # a second warp, back: into the first buffers again; the frame composes to (nearly) the identity
    mid = [getattr(s, k).cpu().numpy().copy() for k in STATE]
    s.warp(np.linalg.inv(T))
    assert all(a is b for a, b in zip((s._sum, s._wsum, s._count), first)) and np.allclose(s.frame, np.eye(4), atol=1e-12)
    _state_against_reference(model, mid, [getattr(s, k).cpu().numpy() for k in STATE], o, np.linalg.inv(T), 0.0, 'fading session, back')
    s.close()
    assert s._twin is None


def test_fading_session_passes_its_forget_below_through(ia, indoor):
    """forget_below of the session applies to the thinned weight sums: the threshold sits in the widest gap of the reference's W' (asserted robust there)."""
    z, model = indoor, indoor['model']
    o = z['scene_meta']['lidar2img']['origin']
    T = _motion(model)(o)
    probe = model.open_scene(z['scene_meta'], decay=1.0)
    probe.add_views(*_views(z, [0, 1, 2]))
    before = [getattr(probe, k).cpu().numpy().copy() for k in STATE]
    ref0 = RW.warp_grid(before[0][0], before[1][0], before[2][0], model.voxel_size, model._new_origin(o).numpy(), T.astype(np.float32))
    w = np.sort(ref0['W'][ref0['W'] > 0])
    lo, hi = len(w) // 4, 3 * len(w) // 4
    gap = lo + int(np.argmax(np.diff(w[lo:hi])))
    fb = float(np.float32((w[gap] + w[gap + 1]) / 2))
    s = model.open_scene(z['scene_meta'], decay=1.0, forget_below=fb)
    s.add_views(*_views(z, [0, 1, 2]))
    assert all(np.array_equal(getattr(s, k).cpu().numpy().view(np.int32), b.view(np.int32)) for k, b in zip(STATE, before)), 'nothing is forgotten by the add'
    s.warp(T)
    ref = _state_against_reference(model, before, [getattr(s, k).cpu().numpy() for k in STATE], o, T, fb, f'forget_below={fb:.4f}')
    gone = (ref0['W'] > 0) & (ref['W'] == 0)
    assert gone.sum() > 10 and (ref['W'] > 0).sum() > 10
    for x in (probe, s):
        x.close()


def test_anchor_head_session_warps_and_keeps_its_origin(ia, anchor):
    """The small KITTI model (Anchor3DHead): warp is accepted where scroll refuses, the state follows the reference, the origin and the device
    new_origin are untouched, and detect() runs through the unchanged head."""
    from imvoxelnet_amd import warped_extrinsic
    from imvoxelnet_amd.heads import Anchor3DHead
    z, model = anchor, anchor['model']
    assert isinstance(model.bbox_head, Anchor3DHead)
    o = z['scene_meta']['lidar2img']['origin']
    s = model.open_scene(z['scene_meta'], decay=0.9)
    s.add_views(*_views(z, [0, 1]))
    with pytest.raises(NotImplementedError, match='anchors'):
        s.scroll((1, 0, 0))
    before = [getattr(s, k).cpu().numpy().copy() for k in STATE]
    keep_origin = s._origin.clone()
    T = RW.rigid(0.04, 0.0, 0.0, np.array([1.6, 0.1, 0.0]) * np.asarray(model.voxel_size), np.asarray(o, np.float64))      # a car: forward and a little yaw
    s.warp(T)
    _state_against_reference(model, before, [getattr(s, k).cpu().numpy() for k in STATE], o, T, 0.0, 'anchor head session')
    assert _same_bits(s._origin, keep_origin) and np.array_equal(s.meta['lidar2img']['origin'], o) and s.scrolled == (0, 0, 0)
    img, E = _views(z, [2])
    s.add_views(img, [warped_extrinsic(e, T) for e in E])
    res = s.detect()
    assert len(res) == 1 and len(res[0]['boxes_3d'].tensor) == len(res[0]['scores_3d'])
    assert bool(torch.isfinite(res[0]['boxes_3d'].tensor).all()) and bool(torch.isfinite(res[0]['scores_3d']).all())
    print('anchor head: detections after the warp:', len(res[0]['scores_3d']))
    s.close()


@pytest.mark.parametrize('maps', [False, True], ids=['plain_ring', 'weights_and_maps'])
def test_windowed_session_is_a_fresh_one_fed_the_warped_extrinsics(ia, indoor, maps):
    """window = 3, five arrivals one at a time with a warp after the third: volume, mask and detections equal, bit for bit, those of a fresh windowed
    session that is given the same views with warped_extrinsic poses (and never warps).  With weights and a confidence map per view the rings travel
    with their slots, unchanged.  No call to ops.volume_warp is made."""
    from imvoxelnet_amd import ops, warped_extrinsic
    z, model = indoor, indoor['model']
    o = z['scene_meta']['lidar2img']['origin']
    T = _motion(model)(o)
    a, b = model.open_scene(z['scene_meta'], window=3), model.open_scene(z['scene_meta'], window=3)
    calls, real = [], ops.volume_warp
    ops.volume_warp = lambda *args, **kw: calls.append(1) or real(*args, **kw)
    try:
        for v in range(5):
            img, E = _views(z, [v])
            kw = {}
            if maps:
                p0 = a._features(img)
                g = torch.Generator().manual_seed(40 + v)
                kw = dict(weights=[0.5 + 0.25 * v], pixel_weights=torch.rand((1,) + tuple(p0.shape[-3:-1]), generator=g))
            Ew = [warped_extrinsic(e, T) for e in E]
            a.add_views(img, Ew if v >= 3 else E, **kw)                       # arrivals after the warp come in the new frame
            b.add_views(img, Ew, **kw)                                        # the fresh session lives in the new frame from the start
            if v == 2:
                va, _ = a.volume()
                va = va.clone()
                assert a.warp(T) is a and a._stale and np.array_equal(a.frame, T)
                ext = a.meta['lidar2img']['extrinsic']
                assert all(np.array_equal(e, warped_extrinsic(z['E'][i], T)) for i, e in enumerate(ext)) and all(w[2] is e for w, e in zip(a._views, ext))
                vol, ok = a.volume()
                volb, okb = b.volume()
                assert _same_bits(vol, volb) and torch.equal(ok, okb) and not _same_bits(vol, va), 'the warp must show'
                _same_results(a.detect(), b.detect())
    finally:
        ops.volume_warp = real
    assert a.view_ids == b.view_ids == [2, 3, 4] and not calls
    vol, ok = a.volume()
    volb, okb = b.volume()
    assert _same_bits(vol, volb) and torch.equal(ok, okb) and 0 < int(ok.sum()) < ok.numel()
    _same_results(a.detect(), b.detect())
    for k in ('_pring', '_ring', '_mring'):
        if getattr(a, k) is not None:
            assert _same_bits(getattr(a, k), getattr(b, k)), k
    assert a._wring == b._wring and (a._mring is not None) == maps
    for s in (a, b):
        s.close()


def test_plain_session_refuses_and_goes_on_like_an_untouched_twin(ia, indoor):
    z, model = indoor, indoor['model']
    T = _motion(model)(z['scene_meta']['lidar2img']['origin'])
    s, twin = model.open_scene(z['scene_meta']), model.open_scene(z['scene_meta'])
    for x in (s, twin):
        x.add_views(*_views(z, [0, 1, 2]))
    keep = {k: getattr(s, k).clone() for k in ('_sum', '_count', '_mean', '_valid')}
    with pytest.raises(NotImplementedError, match='decay=1.0'):
        s.warp(T)
    assert np.array_equal(s.frame, np.eye(4)) and not s._stale and s._twin is None and all(_same_bits(getattr(s, k), v) for k, v in keep.items())
    assert all(np.array_equal(e, z['E'][i]) for i, e in enumerate(s.meta['lidar2img']['extrinsic']))
    for x in (s, twin):
        x.add_views(*_views(z, [3, 4]))
    _same_results(s.detect(), twin.detect())
    for x in (s, twin):
        x.close()


def test_batch_warp_moves_the_named_scenes_and_leaves_the_others(ia, indoor):
    """Three fading scenes; scenes 2 and 0 warp by different transforms in one call (scene 1 is not named, and an identity for it would launch nothing):
    the named rows follow the reference, row 1 keeps every bit of sum, weight sum, count, and the batch holds no second copy of its pools afterwards.  A
    windowed batch re-poses the named scenes' views only."""
    from imvoxelnet_amd import ops, warped_extrinsic
    z, model = indoor, indoor['model']
    o = z['scene_meta']['lidar2img']['origin']
    b = model.open_scenes([z['scene_meta']] * 3, decay=[0.9, 0.8, 1.0])
    img, E = _views(z, [0, 1, 2, 3, 4])
    b.add_views(img, E, scene=[0, 0, 1, 2, 2])
    before = [t.cpu().numpy().copy() for t in (b._sum, b._wsum, b._count)]
    pools = (b._sum, b._wsum, b._count)
    T2, T0 = _motion(model)(o), _motion(model, -0.2, 0.0)(o)
    seen = []
    real = ops.volume_warp
    ops.volume_warp = lambda *args, **kw: seen.append((args[3], kw.get('out_rows'), tuple(kw['out'][0].shape))) or real(*args, **kw)
    try:
        assert b.warp([2, 0, 1], [T2, T0, np.eye(4)]) is b
    finally:
        ops.volume_warp = real
    assert seen == [([2, 0], [0, 1], (2,) + tuple(b._sum.shape[1:]))], 'one call, a scratch pool of as many rows as scenes that move'
    assert all(p is q for p, q in zip(pools, (b._sum, b._wsum, b._count)))
    after = [t.cpu().numpy() for t in pools]
    for s, T in ((2, T2), (0, T0)):
        _state_against_reference(model, [x[s:s + 1] for x in before], [x[s:s + 1] for x in after], o, T, 0.0, f'batch scene {s}')
        assert np.array_equal(b.frame(s), T) and b._scenes[s]._stale
    assert all(np.array_equal(x[1].view(np.int32), y[1].view(np.int32)) for x, y in zip(before, after)), 'scene 1 keeps every bit'
    assert np.array_equal(b.frame(1), np.eye(4)) and not b._scenes[1]._stale
    assert all(np.array_equal(e, warped_extrinsic(E[i], T0)) for i, e in enumerate(b.metas[0]['lidar2img']['extrinsic']))
    assert np.array_equal(b.metas[1]['lidar2img']['extrinsic'][0], E[2])
    res = b.detect()
    assert len(res) == 3 and all(bool(torch.isfinite(r['boxes_3d'].tensor).all()) for r in res)
    b.close()
    # windowed: scene 1 warps, scene 0 keeps its projection rows and its volume
    w, fresh = model.open_scenes([z['scene_meta']] * 2, window=2), model.open_scenes([z['scene_meta']] * 2, window=2)
    w.add_views(img[:4], E[:4], scene=[0, 1, 0, 1])
    fresh.add_views(img[:4], [E[0], warped_extrinsic(E[1], T2), E[2], warped_extrinsic(E[3], T2)], scene=[0, 1, 0, 1])
    v0 = w.volume(0)[0].clone()
    w.warp(1, T2)
    assert w._scenes[1]._stale and not w._scenes[0]._stale
    for s in (0, 1):
        assert _same_bits(w.volume(s)[0], fresh.volume(s)[0]) and torch.equal(w.volume(s)[1], fresh.volume(s)[1]), s
    assert _same_bits(w.volume(0)[0], v0) and _same_bits(w._pring, fresh._pring)
    for x in (w, fresh):
        x.close()


def test_a_session_that_never_warps_never_calls_the_op(ia, indoor):
    """The spy: adds, a scroll, volume() and detect() on a fading session, a windowed one and a batch make no call to ops.volume_warp and allocate no twin."""
    from imvoxelnet_amd import ops
    z, model = indoor, indoor['model']
    calls, real = [], ops.volume_warp
    ops.volume_warp = lambda *args, **kw: calls.append(1) or real(*args, **kw)
    try:
        s, w = model.open_scene(z['scene_meta'], decay=0.9), model.open_scene(z['scene_meta'], window=2)
        b = model.open_scenes([z['scene_meta']] * 2, decay=0.9)
        for x in (s, w):
            x.add_views(*_views(z, [0, 1]))
            x.scroll((1, 0, -1))
            x.add_views(*_views(z, [2]))
            x.detect()
        b.add_views(*_views(z, [0, 1]), scene=[0, 1])
        b.detect()
        assert not calls and s._twin is None and np.array_equal(s.frame, np.eye(4))
        s.warp(np.eye(4))                                                     # the identity launches nothing either
        assert not calls and s._twin is None and not s._stale
        s.warp(RW.rigid(0.1))
        assert calls == [1] and s._twin is not None
        for x in (s, w, b):
            x.close()
    finally:
        ops.volume_warp = real
