"""-m gpu: matching scenes (SceneSession.match / register, SceneBatch.match / register) on the tiny models of the scene tests.  A restored copy of a
scene, warped by D, matches the original at D (T=None is that candidate) and prefers it to 80 candidates around it; both scenes keep every bit;
register finds D again from a start a few degrees and half a voxel away, and the merge under the found transform runs; a scrolled scene matches with
pairs equal to the reference on the pools read back; a batch's answers are bit for bit those of sessions restored from the same states."""
import math

import numpy as np
import pytest
import torch

import ref_volume_match as RX
import ref_volume_warp as RW
from test_gpu_scene_window import _family
from test_gpu_scene_warp import _bits, _views, _motion, STATE

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


def _snapshot(s):
    """Everything a match must leave alone in a session: the state's bits and the host record."""
    return tuple(_bits(getattr(s, k)).clone() for k in STATE), s.n_views, s._stale, [e.copy() for e in s.meta['lidar2img']['extrinsic']], s.frame, s.scrolled


def _unchanged(s, snap):
    now = _snapshot(s)
    return all(torch.equal(a, b) for a, b in zip(now[0], snap[0])) and now[1:3] == snap[1:3] and len(now[3]) == len(snap[3]) \
        and all(np.array_equal(a, b) for a, b in zip(now[3], snap[3])) and np.array_equal(now[4], snap[4]) and now[5] == snap[5]


def _pose_error(T, D, centre):
    """(yaw error in radians, position error per axis at `centre`) of T against D."""
    E = np.linalg.inv(D) @ T
    return abs(math.atan2(E[1, 0], E[0, 0])), np.abs((T @ np.append(centre, 1) - D @ np.append(centre, 1))[:3])


def test_a_warped_copy_matches_registers_and_merges(ia, indoor):
    z, model = indoor, indoor['model']
    vs = np.asarray(model.voxel_size, np.float64)
    a = model.open_scene(z['scene_meta'], decay=0.8)
    a.add_views(*_views(z, [0, 1, 2]))
    b = model.restore_scene(a.snapshot())
    centre = np.asarray(a.meta['lidar2img']['origin'], np.float64)
    D = _motion(model)(centre)
    b.warp(D)
    snaps = _snapshot(a), _snapshot(b)
    r = b.match(a)                                                            # T=None: inv(a.frame) @ b.frame == D
    assert len(r.Ts) == 1 and np.allclose(r.Ts[0], D, atol=1e-12) and r.best == 0 and r.own == int((b._wsum > 0).sum()) and r.pairs[0] > 0.9 * r.own
    print(f'a warped copy at D: ncc {r.score[0]:.6f}, overlap {r.overlap[0]:.3f}, own {r.own}')
    assert r.score[0] > 0.999
    cands = ia.pose_candidates(D, math.radians(10), vs, centre)
    r = b.match(a, cands)
    order = np.argsort(r.score)
    print(f'81 candidates a voxel and ten degrees apart: best {r.best} ({r.score[r.best]:.6f}), next {order[-2]} ({r.score[order[-2]]:.6f})')
    assert r.best == 40 and np.array_equal(r.T, D) and isinstance(r, ia.MatchResult) and r.score.shape == (81,) and r.pairs.dtype == np.int64
    coarse = b.match(a, cands, step=2)
    assert coarse.best == 40 and coarse.own < r.own
    assert _unchanged(a, snaps[0]) and _unchanged(b, snaps[1]), 'a match leaves both scenes bit-unchanged'
    off = RW.rigid(math.radians(3), t=np.array([0.5, -0.5, 0.25]) * vs, about=centre)
    levels = 6
    T, last = b.register(a, T0=D @ off, levels=levels)
    yaw_err, pos_err = _pose_error(T, D, centre)
    h_yaw, h = math.radians(8) / 2 ** (levels - 1), np.array([2 * vs[0], 2 * vs[1], vs[2]]) / 2 ** (levels - 1)
    print(f'register: yaw error {math.degrees(yaw_err):.3f} deg against a step of {math.degrees(h_yaw):.3f}; position error {pos_err.round(4).tolist()} m against '
          f'{h.round(4).tolist()}; ncc {last.score[last.best]:.6f}')
    assert yaw_err <= h_yaw and (pos_err <= h).all() and last.best is not None
    assert _unchanged(a, snaps[0]) and _unchanged(b, snaps[1]), 'register leaves both scenes bit-unchanged'
    n = a.n_views + b.n_views
    assert b.merge(a, T=T) is b and b.n_views == n and bool(torch.isfinite(b._sum).all())
    for x in (a, b):
        x.close()


def test_a_scrolled_scene_matches_the_reference(ia, indoor):
    """A (views 0, 1) against B (views 2, 3; scrolled by one voxel, so the two grids have different origins) under a general motion: pairs, own and
    the statistics are the reference's on the pools read back."""
    z, model = indoor, indoor['model']
    a, b = model.open_scene(z['scene_meta'], decay=0.8), model.open_scene(z['scene_meta'], decay=0.9)
    a.add_views(*_views(z, [0, 1]))
    b.add_views(*_views(z, [2, 3]))
    b.scroll((1, 0, 0))
    assert not np.array_equal(a.meta['lidar2img']['origin'], b.meta['lidar2img']['origin'])
    Ts = [_motion(model)(a.meta['lidar2img']['origin']), _motion(model, -0.2, 0.02)(a.meta['lidar2img']['origin'])]
    oa, ob = model._new_origin(a.meta['lidar2img']['origin']).numpy(), model._new_origin(b.meta['lidar2img']['origin']).numpy()
    host = lambda s: (s._sum.cpu().numpy()[0], s._wsum.cpu().numpy()[0])      # noqa: E731
    ref = RX.match_rows(host(a), host(b), model.voxel_size, oa, ob, [T.astype(np.float32) for T in Ts])
    r = a.match(b, Ts, min_overlap=0.0)
    RX.check((r.pairs, r.own, r.stats), ref, 'a scrolled scene')
    assert ref['pairs'].min() > 50 and np.array_equal(r.overlap, ref['pairs'] / ref['own'])
    for x in (a, b):
        x.close()


def test_a_batch_answers_as_sessions_do(ia, indoor):
    """Three fading scenes of a batch and three sessions restored from their snapshots: SceneBatch.match over two pairs in ONE call equals, bit
    for bit in the statistics and exactly in pairs and own, the two SceneSession.match results; register agrees as well."""
    z, model = indoor, indoor['model']
    bt = model.open_scenes([z['scene_meta']] * 3, decay=0.9)
    img, E = _views(z, [0, 1, 2, 3, 4])
    bt.add_views(img, E, scene=[0, 0, 1, 1, 2])
    s = [model.restore_scene(bt.snapshot(i)) for i in range(3)]
    centre = np.asarray(z['scene_meta']['lidar2img']['origin'], np.float64)
    Ts = [_motion(model)(centre), _motion(model, -0.2, 0.02)(centre), np.eye(4)]
    keep = [_bits(t).clone() for t in (bt._sum, bt._wsum, bt._count)]
    got = bt.match([0, 1], [1, 2], [Ts, Ts[::-1]])
    want = [s[0].match(s[1], Ts), s[1].match(s[2], Ts[::-1])]
    assert len(got) == 2 and all(isinstance(g, ia.MatchResult) for g in got)
    for g, w in zip(got, want):
        assert g.stats.tobytes() == w.stats.tobytes() and np.array_equal(g.pairs, w.pairs) and g.own == w.own and g.best == w.best and g.pairs.max() > 0
    one = bt.match(0, 1, Ts)
    assert one.stats.tobytes() == want[0].stats.tobytes()
    assert bt.match(0, 1).stats.tobytes() == s[0].match(s[1]).stats.tobytes()  # T=None: the frames' transform, the identity here
    Tb, rb = bt.register(0, 1, T0=Ts[0], levels=3)
    Ts_, rs = s[0].register(s[1], T0=Ts[0], levels=3)
    assert np.array_equal(Tb, Ts_) and rb.stats.tobytes() == rs.stats.tobytes() and np.array_equal(rb.pairs, rs.pairs) and rb.best == rs.best
    assert all(torch.equal(_bits(t), k) for t, k in zip((bt._sum, bt._wsum, bt._count), keep)), 'the batch keeps every bit'
    bt.close()
    for x in s:
        x.close()
