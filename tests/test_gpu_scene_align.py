"""-m gpu: aligning scenes (SceneSession.refine, SceneBatch.refine, register(refine=True)) on the tiny models of the scene tests.  Two fading sessions
take the same views and one is warped by a known D: from a start that is off by under half a voxel and 2 degrees in all six degrees of freedom,
refine ends with a lower cost than it started with and nearer D than the start; the same loop with the numpy reference playing align on the
states read back ends at the same pose within twice the tolerances; a batch's answers are bit for bit those of sessions restored from the same
states; register(refine=True) ends no worse than register; every scene keeps every bit."""
import math

import numpy as np
import pytest
import torch

import ref_volume_align as RA
import ref_volume_warp as RW
from test_gpu_scene_window import _family
from test_gpu_scene_warp import _bits, _views, _motion
from test_gpu_scene_match import _snapshot, _unchanged

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


def _off(vs, centre, sign=1.0):
    """A start error in all six degrees of freedom: under 2 degrees in total and under half a voxel per axis."""
    return RW.rigid(math.radians(1.0) * sign, math.radians(-0.8), math.radians(0.9) * sign, np.array([0.4, -0.3, 0.35]) * vs * sign, about=centre)


def _error(T, D, centre):
    """(rotation angle in radians of inv(D) @ T, distance of the images of `centre`)."""
    E = np.linalg.inv(D) @ T
    return math.acos(min(1.0, max(-1.0, (np.trace(E[:3, :3]) - 1) / 2))), float(np.linalg.norm((T @ np.append(centre, 1) - D @ np.append(centre, 1))[:3]))


def test_refine_finds_a_known_warp_and_agrees_with_the_reference(ia, indoor):
    from imvoxelnet_amd.scene import _refine, _check_refine, ALIGN_DOF
    z, model = indoor, indoor['model']
    vs = np.asarray(model.voxel_size, np.float64)
    a, b = model.open_scene(z['scene_meta'], decay=0.8), model.open_scene(z['scene_meta'], decay=0.8)
    for s in (a, b):
        s.add_views(*_views(z, [0, 1, 2]))
    centre = np.asarray(a.meta['lidar2img']['origin'], np.float64)
    D = _motion(model)(centre)
    b.warp(D)                                                                 # x_a = D x_b: the truth of b.refine(a)
    T0 = D @ _off(vs, centre)
    rot0, pos0 = _error(T0, D, centre)
    assert rot0 < math.radians(2) and pos0 < 0.5 * vs.min() * math.sqrt(3) and min(rot0, pos0) > 0
    snaps = _snapshot(a), _snapshot(b)
    T, res = b.refine(a, T0=T0)
    rot, pos = _error(T, D, centre)
    print(f'refine from {math.degrees(rot0):.3f} deg, {pos0:.4f} m off: {res}; ends {math.degrees(rot):.4f} deg, {pos:.5f} m off; cost {res.history[0]:.4g} -> '
          f'{res.cost:.4g}; used / own {res.overlap:.3f}, ncc {res.ncc:.5f}')
    assert isinstance(res, ia.AlignResult) and res.ok and res.accepted >= 1 and res.evaluations <= 12 and np.array_equal(T, res.T)
    assert res.cost < res.history[0] and all(y < x for x, y in zip(res.history, res.history[1:]))
    assert rot < rot0 and pos < pos0, 'nearer the truth than the start'
    assert _unchanged(a, snaps[0]) and _unchanged(b, snaps[1]), 'refine leaves both scenes bit-unchanged'
    # the same loop, the reference playing align on the states read back
    host = lambda s: (s._sum.cpu().numpy()[0], s._wsum.cpu().numpy()[0])      # noqa: E731
    dst, src = host(b), host(a)
    ob, oa = model._new_origin(b.meta['lidar2img']['origin']).numpy(), model._new_origin(a.meta['lidar2img']['origin']).numpy()
    about = np.asarray(b.meta['lidar2img']['origin'], np.float64)

    def play(idx, Ts):
        out = []
        for M in Ts:
            r = RA.align_grid(dst, src, model.voxel_size, ob, oa, M, about, robust=False)
            out.append((r['pairs'], r['used'], r['own'], r['stats']))
        return out

    args = _check_refine(12, ALIGN_DOF, 0.3, 1e-3, None, 1e-5, model.voxel_size)
    T_ref, r_ref = _refine(play, [T0], [about], int(a._sum.shape[-1]), *args)[0]
    d_rot, d_pos = _error(T, T_ref, centre)
    tol_shift, tol_rot = args[4], args[5]
    print(f'device against the reference loop: {d_rot:.3e} rad and {d_pos:.3e} m apart (tolerances {tol_rot:.1e} rad, {tol_shift:.1e} m); evaluations '
          f'{res.evaluations} / {r_ref.evaluations}, accepted {res.accepted} / {r_ref.accepted}, used {res.used} / {r_ref.used}')
    assert d_rot <= 2 * tol_rot and d_pos <= 2 * tol_shift
    for s in (a, b):
        s.close()


def test_a_batch_refines_as_sessions_do(ia, indoor):
    """Scenes 0 and 1 of a batch take the same views and scene 1 is warped by D; scene 2 takes others.  SceneBatch.refine over two pairs -- ONE
    ops.volume_align per iteration -- equals, in T and statistics with ==, SceneSession.refine on sessions restored from the same states; one pair
    alone as well; register(refine=True) agrees too.  The batch keeps every bit."""
    z, model = indoor, indoor['model']
    vs = np.asarray(model.voxel_size, np.float64)
    bt = model.open_scenes([z['scene_meta']] * 3, decay=0.9)
    img, E = _views(z, [0, 1, 2, 0, 1, 2, 3, 4])
    bt.add_views(img, E, scene=[0, 0, 0, 1, 1, 1, 2, 2])
    centre = np.asarray(z['scene_meta']['lidar2img']['origin'], np.float64)
    D = _motion(model)(centre)
    bt.warp([1], [D])
    s = [model.restore_scene(bt.snapshot(i)) for i in range(3)]
    T0s = [D @ _off(vs, centre), _motion(model, -0.05, 0.01)(centre)]
    keep = [_bits(t).clone() for t in (bt._sum, bt._wsum, bt._count)]
    got = bt.refine([1, 2], [0, 0], T0s, min_overlap=0.1)
    want = [s[1].refine(s[0], T0s[0], min_overlap=0.1), s[2].refine(s[0], T0s[1], min_overlap=0.1)]
    for (Tg, g), (Tw, w) in zip(got, want):
        print(f'batch {g} / session {w}')
        assert np.array_equal(Tg, Tw) and g.stats.tobytes() == w.stats.tobytes() and g.history == w.history and (g.evaluations, g.accepted, g.converged, g.ok) == \
            (w.evaluations, w.accepted, w.converged, w.ok) and (g.pairs, g.used, g.own) == (w.pairs, w.used, w.own)
    assert got[0][1].ok and got[0][1].accepted >= 1 and got[0][1].used > 0
    Tg, g = bt.refine(1, 0, T0s[0], min_overlap=0.1)
    assert np.array_equal(Tg, want[0][0]) and g.stats.tobytes() == want[0][1].stats.tobytes()
    Tb, rb = bt.register(1, 0, T0=T0s[0], levels=2, refine=True)
    Ts_, rs = s[1].register(s[0], T0=T0s[0], levels=2, refine=True)
    assert np.array_equal(Tb, Ts_) and rb.stats.tobytes() == rs.stats.tobytes() and rb.match.stats.tobytes() == rs.match.stats.tobytes()
    assert all(torch.equal(_bits(t), k) for t, k in zip((bt._sum, bt._wsum, bt._count), keep)), 'the batch keeps every bit'
    bt.close()
    for x in s:
        x.close()


def test_register_with_refine_ends_no_worse(ia, indoor):
    """register(refine=True) starts its refinement at register's own answer (the same launches before it) and only ever accepts a strictly lower
    cost: it ends at a cost no higher than register's pose has, by default over x, y, z, rz; both scenes keep every bit."""
    z, model = indoor, indoor['model']
    vs = np.asarray(model.voxel_size, np.float64)
    a, b = model.open_scene(z['scene_meta'], decay=0.8), model.open_scene(z['scene_meta'], decay=0.8)
    for s in (a, b):
        s.add_views(*_views(z, [0, 1, 2]))
    centre = np.asarray(a.meta['lidar2img']['origin'], np.float64)
    D = _motion(model)(centre)
    b.warp(D)
    T0 = D @ RW.rigid(math.radians(3), t=np.array([0.5, -0.5, 0.25]) * vs, about=centre)
    snaps = _snapshot(a), _snapshot(b)
    T_reg, last = b.register(a, T0=T0, levels=4)
    T_ref, res = b.register(a, T0=T0, levels=4, refine=True)
    _, at_reg = b.refine(a, T0=T_reg, iters=1)                                # one evaluation: the cost of register's pose
    e_reg, e_ref = _error(T_reg, D, centre), _error(T_ref, D, centre)
    print(f'register: {math.degrees(e_reg[0]):.4f} deg, {e_reg[1]:.5f} m off, cost {at_reg.cost:.4g}; with refine: {math.degrees(e_ref[0]):.4f} deg, {e_ref[1]:.5f} m '
          f'off, cost {res.cost:.4g} ({res})')
    assert isinstance(last, ia.MatchResult) and isinstance(res, ia.AlignResult) and np.array_equal(res.match.T, T_reg) and res.match.stats.tobytes() == last.stats.tobytes()
    assert res.history[0] == at_reg.cost and res.cost <= at_reg.cost and res.ok
    D_ = np.linalg.inv(T_reg) @ T_ref                                         # x, y, z, rz moved: the increment turns about the vertical only
    assert abs(D_[2, 2] - 1) < 1e-12 and abs(D_[0, 2]) < 1e-12 and abs(D_[2, 1]) < 1e-12
    T6, r6 = b.register(a, T0=T0, levels=4, refine=True, dof=ia.scene.ALIGN_DOF)
    assert r6.cost <= at_reg.cost
    assert _unchanged(a, snaps[0]) and _unchanged(b, snaps[1]), 'register and refine leave both scenes bit-unchanged'
    for s in (a, b):
        s.close()
