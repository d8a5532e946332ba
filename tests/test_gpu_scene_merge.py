"""-m gpu: merging scenes (SceneSession.merge, SceneBatch.merge) on the tiny models of the scene tests.  A fading session's state after a merge is
the reference merge (tests/ref_volume_merge.py) of the two states before, within the bound, the other scene keeps every bit, the host record follows
the rule and detect() runs; the anchor family merges too; merging is fusing (two sessions of two views each, merged, hold the weight sum and count
of one session of the four views exactly and its sums within the reassociation bound); T=None is the transform between the frames; an empty other
launches nothing and an empty self adopts the state; every refusal leaves both scenes bit-identical; a batch merges rows of its own pools in one
call; a scene that never merges never calls ops.volume_merge_."""
import numpy as np
import pytest
import torch

import ref_volume_merge as RM
import ref_volume_warp as RW
from test_gpu_scene_window import _family
from test_gpu_scene_warp import _bits, _same_bits, _views, _motion, STATE

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


def _host(s):
    return [getattr(s, k).cpu().numpy().copy() for k in STATE]


def _snapshot(s):
    """Everything a merge may touch in a session: the state's bits (None before the first add) and the host record."""
    state = tuple(None if getattr(s, k) is None else _bits(getattr(s, k)).clone() for k in STATE)
    return state, s.n_views, s._stale, s._hw, [e.copy() for e in s.meta['lidar2img']['extrinsic']], s.frame, s.scrolled, np.array(s.meta['lidar2img']['origin'])


def _unchanged(s, snap):
    now = _snapshot(s)
    return all((a is None and b is None) or torch.equal(a, b) for a, b in zip(now[0], snap[0])) and now[1:4] == snap[1:4] and len(now[4]) == len(snap[4]) \
        and all(np.array_equal(a, b) for a, b in zip(now[4], snap[4])) and np.array_equal(now[5], snap[5]) and now[6] == snap[6] and np.array_equal(now[7], snap[7])


def _merge_against_reference(model, a, b, T, weight, what):
    """a.merge(b, T, weight) against the reference merge of the two states before; b keeps every bit; the record follows the rule."""
    from imvoxelnet_amd import warped_extrinsic
    before, other, snap_b = _host(a), _host(b), _snapshot(b)
    Ea, Eb, n = list(a.meta['lidar2img']['extrinsic']), list(b.meta['lidar2img']['extrinsic']), a.n_views + b.n_views
    oa, ob = model._new_origin(a.meta['lidar2img']['origin']).numpy(), model._new_origin(b.meta['lidar2img']['origin']).numpy()
    ref = RM.merge_grid([x[0] for x in before], [x[0] for x in other], model.voxel_size, oa, ob, np.asarray(T, np.float64).astype(np.float32), weight, a._forget)
    frame, origin, scrolled = a.frame, np.array(a.meta['lidar2img']['origin']), a.scrolled
    assert a.merge(b, T, weight) is a
    RM.check_row([x[0] for x in _host(a)], ref, [x[0] for x in before], what)
    assert _unchanged(b, snap_b), 'the other scene keeps every bit and its record'
    ext = a.meta['lidar2img']['extrinsic']
    assert a.n_views == n and len(ext) == n and a._stale
    assert all(np.array_equal(e, w) for e, w in zip(ext, Ea + [warped_extrinsic(e, T) for e in Eb])) and all(e.dtype == np.float32 for e in ext)
    assert np.array_equal(a.frame, frame) and np.array_equal(a.meta['lidar2img']['origin'], origin) and a.scrolled == scrolled
    return ref


def test_fading_session_state_after_a_merge_is_the_reference_merge(ia, indoor):
    """A (views 0, 1) takes B (views 2, 3; scrolled by one voxel, so the two grids have different origins) under a general motion with weight 0.6."""
    from imvoxelnet_amd import ops
    z, model = indoor, indoor['model']
    a, b = model.open_scene(z['scene_meta'], decay=0.8), model.open_scene(z['scene_meta'], decay=0.9)
    a.add_views(*_views(z, [0, 1]))
    b.add_views(*_views(z, [2, 3]))
    b.scroll((1, 0, 0))
    assert not np.array_equal(a.meta['lidar2img']['origin'], b.meta['lidar2img']['origin'])
    T = _motion(model)(a.meta['lidar2img']['origin'])
    ref = _merge_against_reference(model, a, b, T, 0.6, 'fading session')
    assert ref['merged'].sum() > 50 and (ref['inside'] & ~ref['merged']).any() and (ref['read'].sum(-1) == 8).any()
    vol, ok = a.volume()                                                      # the existing refresh of the merged state
    mean, valid = ops.volume_wmean(a._sum, a._wsum, vol.dtype)
    assert _same_bits(vol, mean) and torch.equal(ok, valid) and not a._stale
    res = a.detect()
    print('detections after the merge:', len(res[0]['scores_3d']))
    assert bool(torch.isfinite(res[0]['boxes_3d'].tensor).all()) and bool(torch.isfinite(res[0]['scores_3d']).all())
    a.add_views(*_views(z, [4]))                                              # the scene goes on: the next add is a tick on the merged state
    assert a.n_views == 5 and bool(torch.isfinite(a.detect()[0]['boxes_3d'].tensor).all())
    assert b.detect() is not None and b.n_views == 2                          # ... and the other stays usable
    for x in (a, b):
        x.close()


def test_anchor_head_sessions_merge(ia, anchor):
    z, model = anchor, anchor['model']
    a, b = model.open_scene(z['scene_meta'], decay=1.0, forget_below=0.0), model.open_scene(z['scene_meta'], decay=0.9)
    a.add_views(*_views(z, [0, 1]))
    b.add_views(*_views(z, [2, 3]))
    o = a.meta['lidar2img']['origin']
    # a car: forward, a little yaw, and -- unlike the warp test's motion -- a third of a voxel up: with no motion along z every g_z is a whole number up to
    # rounding, the upper corners get weights of 1e-7, and whether such a corner alone makes W_s > 0 is a matter of the last bit (the reference refuses)
    T = RW.rigid(0.04, 0.0, 0.0, np.array([1.6, 0.1, 0.3]) * np.asarray(model.voxel_size), np.asarray(o, np.float64))
    _merge_against_reference(model, a, b, T, 1.0, 'anchor head session')
    res = a.detect()
    assert len(res) == 1 and bool(torch.isfinite(res[0]['boxes_3d'].tensor).all()) and bool(torch.isfinite(res[0]['scores_3d']).all())
    for x in (a, b):
        x.close()


def test_merging_is_fusing(ia, indoor):
    """decay=1.0 sessions fed one view per call, so every view's features are the same bits in each: A has views 0, 1, B has 2, 3, C has all four,
    and one session per view holds that view's term alone.  After the identity merge of B into A -- through the sessions where the model's grid makes
    the identity exact, else through the op on the sessions' states with a dyadic grid, which asks nothing of where a state came from -- weight sum and
    count are C's exactly and the sums lie within 2 (V - 1) 2^-24 sum_v |term_v| of C's: two fp32 sums of the same V terms in different association,
    each within (V - 1) 2^-24 sum |term| of the exact sum."""
    from imvoxelnet_amd import ops
    z, model = indoor, indoor['model']
    def fed(views):                                                           # noqa: E306
        s = model.open_scene(z['scene_meta'], decay=1.0)
        for v in views:
            s.add_views(*_views(z, [v]), emit=False)
        return s
    a, b, c = fed([0, 1]), fed([2, 3]), fed([0, 1, 2, 3])
    terms = [fed([v]) for v in range(4)]
    absum = sum(t._sum.abs().double() for t in terms)
    assert torch.equal(sum(t._wsum for t in terms), c._wsum) and torch.equal(sum(t._count for t in terms), c._count), 'unit weights: the weight sum is a count'
    dims, o = tuple(model.n_voxels), model._new_origin(z['scene_meta']['lidar2img']['origin']).numpy()
    inside, i0, f = RM.grid_coords(dims, model.voxel_size, o, o, np.eye(4))
    if inside.all() and not f.any():                                          # the identity is exact on this grid: through the sessions
        a.merge(b, np.eye(4))
        got = (a._sum, a._wsum, a._count)
    else:
        got = tuple(getattr(a, k).clone() for k in STATE)
        vs = (0.25, 0.25, 0.5)
        o = (-(np.asarray(dims) // 2) * np.asarray(vs)).astype(np.float32)
        ops.volume_merge_(*got, [0], tuple(getattr(b, k) for k in STATE), [0], np.eye(4), o, o, vs)
    assert torch.equal(got[1], c._wsum) and torch.equal(got[2], c._count)
    V = 4
    err, bound = (got[0].double() - c._sum.double()).abs(), 2 * (V - 1) * RM.U * absum + RM.TINY
    print(f'merging is fusing: worst |merged - fused| / bound {float((err / bound).max()):.3f}; voxels seen {int((c._wsum > 0).sum())} of {c._wsum.numel()}')
    assert bool((err <= bound).all()) and (c._wsum > 0).sum() > 50
    for x in [a, b, c] + terms:
        x.close()


def test_t_none_is_the_transform_between_the_frames(ia, indoor):
    """Both scenes have warped since they were opened in one common frame: merge(other) equals merge(other, inv(other.frame) @ self.frame) bit for bit."""
    z, model = indoor, indoor['model']
    o = z['scene_meta']['lidar2img']['origin']
    Ta, Tb = _motion(model)(o), _motion(model, -0.2, 0.0)(o)
    b = model.open_scene(z['scene_meta'], decay=0.9)
    b.add_views(*_views(z, [2, 3]))
    b.warp(Tb)
    pair = []
    for explicit in (False, True):
        a = model.open_scene(z['scene_meta'], decay=0.9)
        a.add_views(*_views(z, [0, 1]))
        a.warp(Ta)
        a.merge(b, np.linalg.inv(b.frame) @ a.frame) if explicit else a.merge(b)
        pair.append(a)
    assert all(_same_bits(getattr(pair[0], k), getattr(pair[1], k)) for k in STATE) and (pair[0]._wsum != 0).any()
    assert all(np.array_equal(e, f) for e, f in zip(pair[0].meta['lidar2img']['extrinsic'], pair[1].meta['lidar2img']['extrinsic'])) and pair[0].n_views == 4
    for x in pair + [b]:
        x.close()


def test_empty_other_launches_nothing_and_empty_self_adopts_the_state(ia, indoor, monkeypatch):
    from imvoxelnet_amd import ops, warped_extrinsic
    z, model = indoor, indoor['model']
    calls, real = [], ops.volume_merge_
    monkeypatch.setattr(ops, 'volume_merge_', lambda *args, **kw: calls.append(1) or real(*args, **kw))
    a, empty = model.open_scene(z['scene_meta'], decay=0.9), model.open_scene(z['scene_meta'], decay=0.9)
    a.add_views(*_views(z, [0, 1]))
    a.detect()
    snap, snap_e = _snapshot(a), _snapshot(empty)
    T = _motion(model)(z['scene_meta']['lidar2img']['origin'])
    assert a.merge(empty, T) is a and a.merge(empty) is a
    assert not calls and _unchanged(a, snap) and _unchanged(empty, snap_e) and not a._stale
    # an empty self: its state starts from zero, as its first add would start it, and takes what the other holds
    assert empty._sum is None
    zero = [np.zeros_like(x[0]) for x in _host(a)]
    ref = RM.merge_grid(zero, [x[0] for x in _host(a)], model.voxel_size, *[model._new_origin(z['scene_meta']['lidar2img']['origin']).numpy()] * 2,
                        T.astype(np.float32), 0.5)
    assert empty.merge(a, T, weight=0.5) is empty and calls == [1]
    RM.check_row([x[0] for x in _host(empty)], ref, zero, 'empty self')
    assert _unchanged(a, snap) and empty.n_views == 2 and empty._hw == a._hw and empty._stale and empty._sum.device == a._sum.device
    assert all(np.array_equal(e, warped_extrinsic(f, T)) for e, f in zip(empty.meta['lidar2img']['extrinsic'], a.meta['lidar2img']['extrinsic']))
    vol, ok = empty.volume()
    assert torch.equal(ok.cpu(), torch.from_numpy(ref['merged'])[None]) and bool(torch.isfinite(empty.detect()[0]['boxes_3d'].tensor).all())
    empty.add_views(*_views(z, [2]))                                          # and it goes on as a scene with views: the add does not start it over
    assert empty.n_views == 3 and bool(((empty._wsum > 0).cpu() | ~torch.from_numpy(ref['merged'])[None]).all())
    empty.reset()                                                             # after reset() the kept buffers are started from zero again
    empty.merge(a, T, weight=0.5)
    RM.check_row([x[0] for x in _host(empty)], ref, zero, 'empty self after reset()')
    for x in (a, empty):
        x.close()


def test_refusals_leave_both_scenes_bit_identical(ia, indoor):
    z, model = indoor, indoor['model']
    T = _motion(model)(z['scene_meta']['lidar2img']['origin'])
    a, b = model.open_scene(z['scene_meta'], decay=0.9), model.open_scene(z['scene_meta'], decay=0.8)
    plain, windowed, closed = model.open_scene(z['scene_meta']), model.open_scene(z['scene_meta'], window=2), model.open_scene(z['scene_meta'], decay=0.9)
    for s, vs in ((a, [0, 1]), (b, [2, 3]), (plain, [0, 1]), (windowed, [0, 1]), (closed, [0])):
        s.add_views(*_views(z, vs))
    closed.close()
    other_size = model.open_scene(z['scene_meta'], decay=0.9)
    other_size.add_views(*_views(z, [4]))
    other_size._hw = (other_size._hw[0] + 32, other_size._hw[1])             # (as if its views had come at another size: the check is a host rule)
    snaps = {s: _snapshot(s) for s in (a, b)}
    pstate = (_bits(plain._sum).clone(), _bits(plain._count).clone())
    bad = T.copy()
    bad[:3, :3] *= 1.01
    for x, y, exc, word in ((a, plain, NotImplementedError, 'decay=1.0'), (plain, a, NotImplementedError, 'decay=1.0'), (a, windowed, NotImplementedError, 'window'),
                            (windowed, a, NotImplementedError, 'window'), (a, closed, RuntimeError, 'closed'), (closed, a, RuntimeError, 'closed'),
                            (a, a, ValueError, 'other is self'), (a, other_size, ValueError, 'image size'), (other_size, a, ValueError, 'image size')):
        with pytest.raises(exc, match=word):
            x.merge(y, T)
    for args in ((b, bad), (b, T, 0.0), (b, T, float('nan')), (b, T[:3])):
        with pytest.raises(ValueError):
            a.merge(*args)
    assert all(_unchanged(s, snap) for s, snap in snaps.items())
    assert torch.equal(_bits(plain._sum), pstate[0]) and torch.equal(_bits(plain._count), pstate[1]) and plain.n_views == 2 and windowed.view_ids == [0, 1]
    a.merge(b, T)                                                             # after all that the merge itself still works
    assert a.n_views == 4
    for x in (a, b, plain, windowed, other_size):
        x.close()


def test_batch_merge_is_one_op_call_on_the_pools(ia, indoor, monkeypatch):
    """Four scenes: 0 (views 0, 1), 1 (view 2), 2 (views 3, 4), 3 empty.  merge([0], [2], [T]) equals ops.volume_merge_ on clones of the pools, rows 1,
    2 and 3 keep every bit; then merge([3, 1], [2, 2]): the empty destination's row is zeroed first and a source may repeat -- still one call, with
    the pools as their own source and no scratch.  Scene 3, which got its views by merge, then warps, scrolls and takes a view like any other scene:
    its row follows ops.volume_warp and ops.volume_scroll_ on a copy, bit for bit, and the other rows stay."""
    from imvoxelnet_amd import ops, warped_extrinsic
    z, model = indoor, indoor['model']
    o = z['scene_meta']['lidar2img']['origin']
    bt = model.open_scenes([z['scene_meta']] * 4, decay=[0.9, 0.8, 1.0, 1.0], forget_below=0.0)
    img, E = _views(z, [0, 1, 2, 3, 4])
    bt.add_views(img, E, scene=[0, 0, 1, 2, 2])
    bt.scroll(2, (0, 1, 0))
    pools = (bt._sum, bt._wsum, bt._count)
    T, T3 = _motion(model)(o), _motion(model, -0.2, 0.0)(o)
    no, no2 = model._new_origin(bt.metas[0]['lidar2img']['origin']).numpy(), model._new_origin(bt.metas[2]['lidar2img']['origin']).numpy()
    assert not np.array_equal(no, no2)
    want = tuple(t.clone() for t in pools)
    real = ops.volume_merge_
    real(*want, [0], want, [2], [T], no[None], no2[None], model.voxel_size, alpha=0.7)
    seen = []
    monkeypatch.setattr(ops, 'volume_merge_', lambda *args, **kw: seen.append((args[3], args[5], args[4][0] is args[0])) or real(*args, **kw))
    before, stale2 = [_bits(t).clone() for t in pools], bt._scenes[2]._stale
    assert bt.merge([0], [2], [T], [0.7]) is bt
    assert seen == [([0], [2], True)] and all(p is q for p, q in zip(pools, (bt._sum, bt._wsum, bt._count)))
    for p, w, b4 in zip(pools, want, before):
        assert torch.equal(_bits(p), _bits(w)) and torch.equal(_bits(p)[1:], b4[1:]) and not torch.equal(_bits(p)[0], b4[0])
    ext = bt.metas[0]['lidar2img']['extrinsic']
    assert bt.n_views == [4, 1, 2, 0] and bt._scenes[0]._stale and bt._scenes[2]._stale == stale2 and len(ext) == 4
    assert all(np.array_equal(e, w) for e, w in zip(ext, E[:2] + [warped_extrinsic(e, T) for e in E[3:]]))
    # an empty destination and a repeated source, in one call; a pair whose source is empty is skipped
    want = tuple(t.clone() for t in pools)
    for t in want:
        t[3].zero_()
    real(*want, [3, 1], want, [2, 2], [T3, T], np.stack([no, no]), np.stack([no2, no2]), model.voxel_size, alpha=[1.0, 1.0])
    del seen[:]
    bt.merge([3, 1], [2, 2], [T3, T])
    assert seen == [([3, 1], [2, 2], True)]
    for p, w in zip(pools, want):
        assert torch.equal(_bits(p), _bits(w))
    assert bt.n_views == [4, 3, 2, 2] and (bt._wsum[3] > 0).any()
    res = bt.detect()
    assert len(res) == 4 and all(bool(torch.isfinite(r['boxes_3d'].tensor).all()) for r in res)
    # scene 3 got its views by merge: it holds the camera record its first add would have stored, and warps, scrolls and takes views like any other
    assert bt._cam[3] is not None and torch.equal(bt._cam[3][0], bt._cam[0][0]) and torch.equal(bt._cam[3][1], bt._cam[0][1])
    want = tuple(t[3:4].clone() for t in pools)
    out = tuple(torch.empty_like(t) for t in want)
    ops.volume_warp(*want, [0], [T], no[None], model.voxel_size, out=out)
    ops.volume_scroll_(out[0], out[2], [0], [(1, 0, -1)], out[1])
    others = [_bits(t)[:3].clone() for t in pools]
    bt.warp(3, T)
    bt.scroll(3, (1, 0, -1))
    for p, w, o3 in zip(pools, out, others):
        assert torch.equal(_bits(p)[3:4], _bits(w)) and torch.equal(_bits(p)[:3], o3)
    assert np.array_equal(bt.frame(3), T) and bt.scrolled(3) == (1, 0, -1) and (bt._wsum[3] > 0).any()
    bt.add_views(img[:1], [warped_extrinsic(E[0], T)], scene=[3])
    res = bt.detect([3])
    assert bt.n_views == [4, 3, 2, 3] and bool(torch.isfinite(res[0]['boxes_3d'].tensor).all())
    bt.reset([2])
    del seen[:]
    bt.merge(0, 2)
    assert not seen and bt.n_views == [4, 3, 0, 3]
    bt.close()


def test_scenes_that_never_merge_never_call_the_op(ia, indoor, monkeypatch):
    from imvoxelnet_amd import ops
    z, model = indoor, indoor['model']
    calls = []
    monkeypatch.setattr(ops, 'volume_merge_', lambda *args, **kw: calls.append(1))
    s, w = model.open_scene(z['scene_meta'], decay=0.9), model.open_scene(z['scene_meta'], window=2)
    b = model.open_scenes([z['scene_meta']] * 2, decay=0.9)
    for x in (s, w):
        x.add_views(*_views(z, [0, 1]))
        x.scroll((1, 0, -1))
        x.warp(RW.rigid(0.1))
        x.add_views(*_views(z, [2]))
        x.detect()
    b.add_views(*_views(z, [0, 1]), scene=[0, 1])
    b.warp(0, RW.rigid(0.1))
    b.detect()
    assert not calls
    for x in (s, w, b):
        x.close()
