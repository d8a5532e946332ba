"""-m gpu: scene snapshots (SceneSession.snapshot, ImVoxelNet.restore_scene, SceneBatch.snapshot / restore, SceneSnapshot.save / load) on the tiny
indoor model of the scene tests.  A fading session that was fused, faded, made to forget, scrolled, warped and merged into holds all-zero sums at
every unseen voxel -- the precondition of the exact round trip, on a state the library made -- and after snapshot, save, load and restore_scene the
new session holds its (sum, weight sum, count) bit for bit, gives the same volume and boxes, and stays bit-equal when both take a further view.  The
same for a plain session, between a batch row and a session in both directions, and for an empty scene; a bf16 snapshot restores sums within
(2^-8 + 2^-22) |S| and a mean within (2^-8 + 2^-21) |mean|."""
import numpy as np
import pytest
import torch

import ref_volume_pack as RP
import ref_volume_warp as RW
from test_gpu_scene_window import _family
from test_gpu_scene_warp import _bits, _same_bits, _views, _motion

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def indoor():
    import imvoxelnet_amd
    from imvoxelnet_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    return _family(imvoxelnet_amd, 'indoor')


def _state(s):
    return [t for t in (s._sum, s._wsum, s._count) if t is not None]


def _same_state(a, b):
    return len(a) == len(b) and all(_same_bits(x, y) for x, y in zip(a, b))


def _same_record(a, b):
    ea, eb = a.meta['lidar2img']['extrinsic'], b.meta['lidar2img']['extrinsic']
    return (a.n_views, a._hw, a.scrolled, a._decay, a._forget, a._gate, a._window) == (b.n_views, b._hw, b.scrolled, b._decay, b._forget, b._gate, b._window) \
        and np.array_equal(a.frame, b.frame) and len(ea) == len(eb) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(ea, eb)) \
        and np.array_equal(np.asarray(a.meta['lidar2img']['origin'], np.float32), np.asarray(b.meta['lidar2img']['origin'], np.float32)) \
        and np.array_equal(a.meta['lidar2img']['intrinsic'], b.meta['lidar2img']['intrinsic']) \
        and all(tuple(a.meta[k]) == tuple(b.meta[k]) for k in ('img_shape', 'ori_shape') if k in a.meta) and a.meta.get('box_type_3d') is b.meta.get('box_type_3d')


def _same_boxes(ra, rb):
    return len(ra) == len(rb) and all(torch.equal(x['boxes_3d'].tensor, y['boxes_3d'].tensor) and torch.equal(x['scores_3d'], y['scores_3d']) and
                                      torch.equal(x['labels_3d'], y['labels_3d']) for x, y in zip(ra, rb))


def _unseen_sums_are_zero(s):
    """The precondition: wherever count and the weight-sum word are zero, every bit of the sums is zero -> (unseen, all) voxel counts."""
    unseen = _bits(s._count) == 0
    if s._wsum is not None:
        unseen &= _bits(s._wsum) == 0
    assert not bool(_bits(s._sum)[unseen].any()), 'an unseen voxel holds a sum that is not +0'
    return int(unseen.sum()), unseen.numel()


def _round_trip(model, s, tmp_path, dtype=torch.float32):
    """snapshot -> save -> load -> restore_scene; the session itself keeps every bit."""
    from imvoxelnet_amd import SceneSnapshot
    before = [_bits(t).clone() for t in _state(s)]
    snap = s.snapshot(dtype)
    assert all(torch.equal(_bits(t), b) for t, b in zip(_state(s), before)), 'a snapshot changes nothing'
    path = str(tmp_path / f'scene_{dtype}.npz'.replace('torch.', ''))
    loaded = SceneSnapshot.load(snap.save(path))
    assert loaded.n_seen == snap.n_seen and loaded.payload.tobytes() == snap.payload.tobytes() and loaded.index.tobytes() == snap.index.tobytes()
    return snap, model.restore_scene(loaded)


def test_fading_session_round_trip_is_exact_and_the_scene_goes_on(indoor, tmp_path):
    z, model = indoor, indoor['model']
    a, b = model.open_scene(z['scene_meta'], decay=0.8, forget_below=0.05), model.open_scene(z['scene_meta'], decay=0.9)
    img, E = _views(z, [0, 1])
    a.add_views(img, E, weights=[1.0, 0.055])                                  # the second view's own voxels fall below the threshold at the next tick
    seen_before = int((a._wsum > 0).sum())
    a.add_views(*_views(z, [2]), emit=False)
    a.scroll((1, 0, 0))
    a.warp(_motion(model)(a.meta['lidar2img']['origin']))
    b.add_views(*_views(z, [3]))
    a.merge(b, RW.rigid(0.05, t=(0.1, -0.05, 0.0)), 0.7)
    unseen, total = _unseen_sums_are_zero(a)
    print(f'fading state after fuse / fade / forget / scroll / warp / merge: {total - unseen} of {total} voxels seen ({seen_before} after the first tick)')
    assert 0 < unseen < total
    snap, r = _round_trip(model, a, tmp_path)
    assert snap.n_seen == total - unseen and snap.kind == 'fading' and snap.payload_dtype == 'float32' and snap.n_views == 4 and snap.scrolled == (1, 0, 0)
    assert abs(snap.seen_fraction - (total - unseen) / total) < 1e-12 and snap.nbytes == snap.n_seen * (12 + 4 * snap.channels)
    assert r is not a and r._stale and r._twin is None and _same_record(a, r)
    assert _same_state(_state(a), _state(r)), 'the restored (sum, weight sum, count) are the original bit for bit'
    (va, oka), (vr, okr) = a.volume(), r.volume()
    assert _same_bits(va, vr) and torch.equal(oka, okr) and not r._stale
    da, dr = a.detect(), r.detect()
    print('detections:', len(da[0]['scores_3d']))
    assert _same_boxes(da, dr)
    for s in (a, r):                                                          # both go on: the same further view, one more tick
        s.add_views(*_views(z, [4]))
    assert _same_state(_state(a), _state(r)) and _same_bits(a.volume()[0], r.volume()[0]) and _same_record(a, r) and _same_boxes(a.detect(), r.detect())
    r.warp(RW.rigid(0.02))                                                    # ... and the restored session warps, scrolls and merges like any other
    r.scroll((0, 1, 0))
    r.merge(b)
    assert bool(torch.isfinite(r.detect()[0]['boxes_3d'].tensor).all())
    for s in (a, b, r):
        s.close()


def test_plain_session_round_trip_is_exact(indoor, tmp_path):
    z, model = indoor, indoor['model']
    a = model.open_scene(z['scene_meta'])
    a.add_views(*_views(z, [0, 1]))
    a.scroll((0, -1, 1))
    a.add_views(*_views(z, [2]))
    unseen, total = _unseen_sums_are_zero(a)
    assert 0 < unseen < total
    snap, r = _round_trip(model, a, tmp_path)
    assert snap.kind == 'plain' and snap.wsum is None and snap.decay is None and snap.n_seen == total - unseen
    assert r._wsum is None and r._decay is None and _same_record(a, r) and _same_state(_state(a), _state(r))
    assert _same_bits(a.volume()[0], r.volume()[0]) and torch.equal(a.volume()[1], r.volume()[1]) and _same_boxes(a.detect(), r.detect())
    for s in (a, r):
        s.add_views(*_views(z, [3]))
    assert _same_state(_state(a), _state(r)) and _same_bits(a.volume()[0], r.volume()[0])
    with pytest.raises(ValueError, match='plain snapshot into a fading batch'):
        model.open_scenes([z['scene_meta']] * 2, decay=0.9).restore(0, snap)
    for s in (a, r):
        s.close()


def test_between_a_batch_row_and_a_session(indoor, tmp_path):
    """A row of a fading batch opens as a session with the row's state; a session's snapshot goes into a row of a batch whose other rows keep every
    bit; lists of scenes go in one call, into a batch that has no pools yet."""
    from imvoxelnet_amd import ops
    z, model = indoor, indoor['model']
    bt = model.open_scenes([z['scene_meta']] * 3, decay=0.9)
    img, E = _views(z, [0, 1, 2])
    bt.add_views(img, E, scene=[0, 0, 2])
    bt.scroll(0, (1, 0, 0))
    snap0 = bt.snapshot(0)
    assert snap0.n_views == 2 and snap0.scrolled == (1, 0, 0) and snap0.n_seen == ops.volume_pack_count(bt._sum, bt._count, [0], bt._wsum)[0]
    r = model.restore_scene(snap0)
    assert all(_same_bits(x[0], y[0]) for x, y in zip(_state(r), (bt._sum, bt._wsum, bt._count))) and r.n_views == 2 and r.scrolled == (1, 0, 0)
    assert _same_bits(r.volume()[0], bt.volume(0)[0]) and torch.equal(r.volume()[1], bt.volume(0)[1])
    # a session into row 1, between rows 0 and 2
    s = model.open_scene(z['scene_meta'], decay=0.9)
    s.add_views(*_views(z, [3, 4]))
    s.warp(RW.rigid(0.03))
    keep = [_bits(t).clone() for t in (bt._sum, bt._wsum, bt._count)]
    assert bt.restore(1, s.snapshot()) is bt and bt.n_views == [2, 2, 1]
    for pool, was, mine in zip((bt._sum, bt._wsum, bt._count), keep, _state(s)):
        assert torch.equal(_bits(pool)[0], was[0]) and torch.equal(_bits(pool)[2], was[2]), 'rows that are not named keep every bit'
        assert _same_bits(pool[1], mine[0])
    assert _same_record(s, bt._scenes[1]) and bt._cam[1] is not None
    assert _same_bits(bt.volume(1)[0], s.volume()[0]) and torch.equal(bt.volume(1)[1], s.volume()[1])
    res = bt.detect()
    assert len(res) == 3 and all(bool(torch.isfinite(x['boxes_3d'].tensor).all()) for x in res)
    for x in (s, ):                                                           # the row goes on like the session: counts and weight sums do not depend on features
        x.add_views(*_views(z, [0]))
    bt.add_views(*_views(z, [0]), scene=[1])
    assert torch.equal(bt._count[1], s._count[0]) and torch.equal(bt._wsum[1], s._wsum[0]) and bt.n_views == [2, 3, 1]
    # lists: two rows out in one pack, into a batch without pools in one unpack
    snaps = bt.snapshot([2, 0])
    assert [x.n_views for x in snaps] == [1, 2]
    b2 = model.open_scenes([z['scene_meta']] * 3, decay=0.9)
    assert b2._sum is None and b2.restore([0, 2], snaps) is b2 and b2.n_views == [1, 0, 2] and b2._hw == bt._hw
    for dst, src in ((0, 2), (2, 0)):
        assert all(_same_bits(p[dst], q[src]) for p, q in zip((b2._sum, b2._wsum, b2._count), (bt._sum, bt._wsum, bt._count)))
        assert _same_bits(b2.volume(dst)[0], bt.volume(src)[0])
    b2.add_views(*_views(z, [1]), scene=[1])                                  # the row the restore did not name starts like any first add
    assert b2.n_views == [1, 1, 2] and bool(torch.isfinite(b2.detect([1])[0]['boxes_3d'].tensor).all())
    for x in (bt, b2, s, r):
        x.close()


def test_an_empty_scene_round_trips_and_then_fuses_like_a_fresh_one(indoor, tmp_path, monkeypatch):
    from imvoxelnet_amd import ops
    z, model = indoor, indoor['model']
    calls = []
    for name in ('volume_pack', 'volume_unpack_'):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _real=real, _name=name, **k: calls.append(_name) or _real(*a, **k))
    a = model.open_scene(z['scene_meta'], decay=0.7, forget_below=0.1)
    snap, r = _round_trip(model, a, tmp_path)
    assert snap.n_seen == 0 and snap.n_views == 0 and not calls and r.n_views == 0 and r._sum is None and _same_record(a, r)
    fresh = model.open_scene(z['scene_meta'], decay=0.7, forget_below=0.1)
    for s in (r, fresh):
        s.add_views(*_views(z, [0, 1]))
    assert _same_state(_state(r), _state(fresh)) and _same_bits(r.volume()[0], fresh.volume()[0])
    assert not calls, 'a session that never snapshots calls what it called before'
    r.snapshot()
    assert calls == ['volume_pack']
    for s in (a, r, fresh):
        s.close()


def test_bf16_snapshot_restores_within_the_derived_bound(indoor, tmp_path):
    """Payload: the bf16 mean.  Weight sum and count come back bit for bit; the sums within (2^-8 + 2^-22) |S| wherever |S / W| is a normal bf16 number;
    the mean the restored session computes, fl32(S' / W), within (2^-8 + 2^-21) |mean| of the original's fl32(S / W): the two divisions add 2^-24 each."""
    z, model = indoor, indoor['model']
    a = model.open_scene(z['scene_meta'], decay=0.9)
    a.add_views(*_views(z, [0, 1, 2]), weights=[1.0, 0.5, 2.0])
    snap, r = _round_trip(model, a, tmp_path, torch.bfloat16)
    f32 = a.snapshot()
    assert snap.payload.dtype == np.uint16 and snap.payload_dtype == 'bfloat16' and snap.n_seen == f32.n_seen and snap.nbytes < 0.52 * f32.nbytes + 12 * snap.n_seen
    assert _same_bits(a._wsum, r._wsum) and _same_bits(a._count, r._count)
    S, S2, W = a._sum.double().cpu().numpy(), r._sum.double().cpu().numpy(), a._wsum.double().cpu().numpy()[..., None]
    seen = W[..., 0] > 0
    q = np.abs(S[seen] / W[seen])
    ok = (q >= RP.BF16_MIN_NORMAL) & (q <= RP.BF16_MAX)
    frac = np.abs(S2 - S)[seen][ok] / (RP.BF16_BOUND * np.abs(S[seen][ok]))
    print(f'bf16 snapshot: worst |S\' - S| / ((2^-8 + 2^-22) |S|) = {frac.max():.4f} over {int(ok.sum())} sums ({int((~ok).sum())} outside the normal range)')
    assert ok.mean() > 0.99 and 0 < frac.max() <= 1.0 and not S2[~seen].any()
    (va, oka), (vr, okr) = a.volume(), r.volume()
    assert torch.equal(oka, okr)
    ma, mr = va.double().cpu().numpy()[seen][ok], vr.double().cpu().numpy()[seen][ok]
    big = np.abs(ma) >= 2.0 ** -100
    mfrac = np.abs(mr - ma)[big] / ((2.0 ** -8 + 2.0 ** -21) * np.abs(ma[big]))
    print(f'bf16 snapshot: worst |mean\' - mean| / ((2^-8 + 2^-21) |mean|) = {mfrac.max():.4f}')
    assert mfrac.max() <= 1.0 and bool(torch.isfinite(r.detect()[0]['boxes_3d'].tensor).all())
    for s in (a, r):
        s.close()
