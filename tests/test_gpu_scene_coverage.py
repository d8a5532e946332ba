"""-m gpu: view coverage and the keyframe gate on streaming scenes (SceneSession.coverage / SceneBatch.coverage, add_views(..., min_novelty=)) on the
tiny indoor model of the scene tests.  coverage() equals the numpy reference of tests/ref_view_coverage.py evaluated on the session's own camera
set-up and on its DOWNLOADED state, with ==, for plain, fading and windowed sessions and a batch of three; a pose that is in the scene finds
nothing fresh and is rejected before the trunk runs, leaving every state tensor bit-identical; a call of a redundant and a new view leaves the
session equal, bit for bit, to a twin that was handed only the admitted view; in a batch a scene whose views were all rejected does not fade; an
ungated add launches the ops it launched before."""
import collections

import numpy as np
import pytest
import torch

import ref_view_coverage as RC
from test_gpu_scene_batch import _scene_metas
from test_gpu_scene_weighted import _same_bits, _views
from test_gpu_scene_window import _family

pytestmark = pytest.mark.gpu

GATE = (0.5, 0.75)
STATE = ('_sum', '_count', '_wsum', '_mean', '_valid', '_ring', '_pring')
KINDS = {'plain': (dict(), '_count', RC.COUNT), 'fading': (dict(decay=0.75, forget_below=0.3, depth_gate=GATE), '_wsum', RC.WSUM),
         'windowed': (dict(window=3, depth_gate=GATE), '_valid', RC.MASK)}


@pytest.fixture(scope='module')
def z():
    import imvoxelnet_amd
    from imvoxelnet_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    z = _family(imvoxelnet_amd, 'indoor')
    H, W = z['img'].shape[2:]
    z['fhw'] = (H // 4, W // 4)
    g = torch.Generator().manual_seed(43)
    pw = 0.25 + 1.5 * torch.rand(5, *z['fhw'], generator=g)
    dp = 0.5 + 3.0 * torch.rand(5, *z['fhw'], generator=g)
    kind = torch.randint(0, 12, (5,) + z['fhw'], generator=g)
    pw[kind == 0], pw[kind == 1] = 0.0, float('nan')
    for k, v in ((2, 0.0), (3, float('nan')), (4, float('inf'))):
        dp[kind == k] = v
    z['maps'] = (pw, dp)
    return z


def _reference(z, meta, E, state, kind, fresh_below=1.0, pw=None, dp=None, gate=(np.inf, np.inf)):
    """The reference on the model's own host camera set-up for these views of this meta and on a downloaded state row."""
    model = z['model']
    view_meta = dict(meta, lidar2img=dict(meta['lidar2img'], extrinsic=list(E)))
    proj, no, crop = (t.numpy() for t in model._camera_setup([view_meta], 4, 'cpu'))
    return RC.coverage(proj[0], model.n_voxels, model.voxel_size, no[0], crop[0], z['fhw'], None if state is None else state.cpu().numpy(), kind, fresh_below,
                       None if pw is None else pw.numpy(), None if dp is None else dp.numpy(), gate)


def _snapshot(s):
    return {k: getattr(s, k).clone() for k in STATE if getattr(s, k, None) is not None}, s.n_views, list(s.view_ids), [e.copy() for e in s.meta['lidar2img']['extrinsic']]


def _unchanged(s, snap):
    tensors, n_views, ids, E = snap
    return (all(_same_bits(getattr(s, k), v) for k, v in tensors.items()) and {k for k in STATE if getattr(s, k, None) is not None} == set(tensors)
            and s.n_views == n_views and list(s.view_ids) == ids and len(s.meta['lidar2img']['extrinsic']) == len(E)
            and all(np.array_equal(a, b) for a, b in zip(s.meta['lidar2img']['extrinsic'], E)))


def _count_features(s):
    calls, inner = [], s._features

    def counted(img):
        calls.append(int(img.shape[0]))
        return inner(img)
    s._features = counted
    return calls


@pytest.mark.parametrize('name', list(KINDS))
def test_session_coverage_equals_the_reference_on_the_downloaded_state(z, name):
    kw, field, kind = KINDS[name]
    model, E = z['model'], z['E']
    s = model.open_scene(z['scene_meta'], **kw)
    pw, dp = z['maps']
    # an empty scene: nothing is held, every seen voxel is fresh; the meta's pad_shape gives the feature-map size
    c = s.coverage(E)
    assert isinstance(c, np.ndarray) and c.dtype == np.int64 and c.shape == (5, 2)
    assert np.array_equal(c, _reference(z, z['scene_meta'], E, None, RC.NONE)) and np.array_equal(c[:, 0], c[:, 1]) and (c[:, 0] > 0).all()
    img, E01 = _views(z, [0, 1])
    s.add_views(img, E01, **({} if name == 'plain' else dict(weights=[1.0, 0.5])))
    s.volume()
    snap = _snapshot(s)
    for fb in (None, 0.6, 2.0):
        c = s.coverage(E, fresh_below=fb)
        state = getattr(s, field)[0]
        ref = _reference(z, z['scene_meta'], E, state, kind, 1.0 if fb is None else fb)
        print(name, fb, c.tolist())
        assert np.array_equal(c, ref), (name, fb)
    c = s.coverage(E)
    assert c[0, 1] == 0 and c[0, 0] > 0, 'a pose that is in the scene with full weight finds nothing fresh'
    assert (c[2:4, 1] > 0).all() and (c[1:, 1] < c[1:, 0]).any(), 'the poses on the other side find some fresh voxels, and one pose some that are not'
    # maps: the confidence on every kind of session, the depth where a gate was given at open; at feature resolution and at the input size
    use_depth = 'depth_gate' in kw
    c = s.coverage(E, pixel_weights=pw, depths=dp if use_depth else None)
    ref = _reference(z, z['scene_meta'], E, getattr(s, field)[0], kind, 1.0, pw, dp if use_depth else None, GATE if use_depth else (np.inf, np.inf))
    assert np.array_equal(c, ref) and (c[:, 0] < s.coverage(E)[:, 0]).all() and (c[:, 0] > 0).all()
    big = torch.full((5,) + tuple(z['img'].shape[2:]), float('nan'))
    big[:, ::4, ::4] = pw
    assert np.array_equal(s.coverage(E, pixel_weights=big, depths=dp.cuda() if use_depth else None), c)
    assert _unchanged(s, snap), 'coverage changes nothing in the session'
    if name == 'windowed':                          # a stale windowed scene refreshes first: the evidence is the mask of the kept views
        img, E23 = _views(z, [2, 3])
        s.add_views(img, E23)                       # evicts view 0
        assert s._stale and s.view_ids == [1, 2, 3]
        c = s.coverage(E)
        assert not s._stale and np.array_equal(c, _reference(z, z['scene_meta'], E, s._valid[0], RC.MASK))
        assert c[0, 1] > 0 and (c[1:4, 1] == 0).all()
    s.close()
    with pytest.raises(RuntimeError, match='closed'):
        s.coverage(E)


@pytest.mark.parametrize('name', list(KINDS))
def test_gate_rejects_a_redundant_view_before_the_trunk(z, name):
    kw = KINDS[name][0]
    s = z['model'].open_scene(z['scene_meta'], **kw)
    img, E0 = _views(z, [0])
    s.add_views(img, E0)
    assert s.last_admitted is None
    s.volume()
    snap, calls = _snapshot(s), _count_features(s)
    assert s.add_views(img, E0, min_novelty=0.01) is s
    assert s.last_admitted == [False] and calls == [] and _unchanged(s, snap) and not s._stale
    img2, E02 = _views(z, [0, 0])
    s.add_views(img2, E02, min_novelty=1.0, fresh_below=0.5, **({} if name == 'plain' else dict(weights=[1.0, 2.0])))
    assert s.last_admitted == [False, False] and calls == [] and _unchanged(s, snap)
    s.add_views(img, E0)                            # ungated: the view goes in as it always did
    assert s.last_admitted is None and calls == [1] and s.n_views == 2 and not _unchanged(s, snap)
    s.close()


@pytest.mark.parametrize('name', list(KINDS))
def test_gated_call_equals_a_twin_that_got_only_the_admitted_view(z, name):
    """Views 0 (in the scene already) and 2 (the camera on the other side of the circle) in one call: 0 is rejected, 2 admitted, and the session
    is afterwards, bit for bit, a twin session that was handed view 2 alone -- the rejected view's image, extrinsic, weight and maps were
    sliced away before the trunk."""
    kw = KINDS[name][0]
    model = z['model']
    s, twin = model.open_scene(z['scene_meta'], **kw), model.open_scene(z['scene_meta'], **kw)
    img0, E0 = _views(z, [0])
    for x in (s, twin):
        x.add_views(img0, E0)
    cov = s.coverage([z['E'][0], z['E'][2]])
    novelty = cov[:, 1] / cov[:, 0]
    assert novelty[0] == 0 and novelty[1] > 0, cov
    thr = float(novelty[1]) / 2
    img, E = _views(z, [0, 2])
    extra, extra_twin = {}, {}
    if name != 'plain':
        pw, dp = z['maps']
        extra = dict(weights=[3.0, 0.5], pixel_weights=pw[[0, 2]], depths=dp[[0, 2]])
        extra_twin = dict(weights=[0.5], pixel_weights=pw[[2]], depths=dp[[2]])
        cov = s.coverage(E, pixel_weights=pw[[0, 2]], depths=dp[[0, 2]])
        assert cov[0, 1] == 0 and cov[1, 0] > 0 and cov[1, 1] / cov[1, 0] >= thr, cov
    calls = _count_features(s)
    s.add_views(img, E, min_novelty=thr, **extra)
    assert s.last_admitted == [False, True] and calls == [1]
    twin.add_views(*_views(z, [2]), **extra_twin)
    (va, oka), (vb, okb) = s.volume(), twin.volume()
    assert _same_bits(va, vb) and torch.equal(oka, okb)
    for k in STATE + ('_mring', '_dring'):
        a, b = getattr(s, k), getattr(twin, k)
        if a is not None and k in ('_ring', '_pring'):          # (the rings are allocated uninitialised: the slots in use are what a scene holds)
            used = torch.tensor([v[1] for v in s._views], device='cuda')
            a, b = a[used], b[used]
        assert (a is None) == (b is None) and (a is None or _same_bits(a, b)), k
    assert s.n_views == twin.n_views == 2 and s.view_ids == twin.view_ids and s._wring == twin._wring
    assert all(np.array_equal(a, b) for a, b in zip(s.meta['lidar2img']['extrinsic'], twin.meta['lidar2img']['extrinsic']))
    s.close()
    twin.close()


def test_add_views_u8_gates_after_the_pipeline_first_and_before_it_later(z):
    from imvoxelnet_amd import data
    model, E = z['model'], z['E']
    rng = np.random.default_rng(70)
    frames = [rng.integers(0, 256, (190, 256, 3), dtype=np.uint8) for _ in range(2)]
    user = {k: v for k, v in z['scene_meta'].items() if k not in ('img_shape', 'ori_shape', 'pad_shape')}
    s = model.open_scene(user)
    s.add_views_u8(frames[:1], E[:1], (128, 96), min_novelty=0.5)          # the first call: the shapes come from the pipeline, then the gate
    assert s.last_admitted == [True] and s.n_views == 1
    snap, calls = _snapshot(s), _count_features(s)
    pipeline, runs = data.prepare_images_device, []
    data.prepare_images_device = lambda *a, **k: (runs.append(1), pipeline(*a, **k))[1]
    try:
        s.add_views_u8(frames[:1], E[:1], (128, 96), min_novelty=0.01)     # redundant: rejected before the frame is even resized
        assert s.last_admitted == [False] and runs == [] and calls == [] and _unchanged(s, snap)
        s.add_views_u8(frames, [E[0], E[2]], (128, 96), min_novelty=0.01)
        assert s.last_admitted == [False, True] and runs == [1] and calls == [1] and s.n_views == 2
    finally:
        data.prepare_images_device = pipeline
    s.close()


def test_batch_of_three(z):
    """A fading batch of three scenes with their own intrinsics, origins and decays: coverage() in one launch equals the per-scene references on
    the downloaded weight sums, in the order of the call's views; a scene without views counts as empty; a gated tick whose views for scenes 0
    and 1 are redundant leaves those scenes unfaded, bit for bit, and equals a twin batch that got only the admitted view."""
    model, E, img = z['model'], z['E'], z['img']
    metas = _scene_metas(z)
    kw = dict(decay=[1.0, 0.5, 0.75], forget_below=0.3)
    b, twin = model.open_scenes(metas, **kw), model.open_scenes(metas, **kw)
    # before any view: every scene is empty
    order = [0, 1, 2, 0, 2]
    c = b.coverage(E, order)
    assert c.shape == (5, 2) and c.dtype == np.int64
    for t, sc in enumerate(order):
        assert np.array_equal(c[t], _reference(z, metas[sc], [E[t]], None, RC.NONE)[0]), t
    for x in (b, twin):
        x.add_views(img[:2].contiguous(), E[:2], [0, 1])
    # scene 2 has no view yet, the pools exist: its row counts as empty
    c = b.coverage(E, order)
    for t, sc in enumerate(order):
        state = b._wsum[sc] if sc < 2 else None
        assert np.array_equal(c[t], _reference(z, metas[sc], [E[t]], state, RC.WSUM if sc < 2 else RC.NONE)[0]), t
    assert c[0, 1] == 0 and c[1, 1] == 0 and c[2, 1] == c[2, 0] > 0 and 0 < c[3, 1]
    assert b.n_views == [1, 1, 0] and _same_bits(b._wsum[:2], twin._wsum[:2]) and _same_bits(b._sum[:2], twin._sum[:2])
    for x in (b, twin):
        x.add_views(img[2:3].contiguous(), E[2:3], [2])
    pw, _ = z['maps']
    c = b.coverage(E, order, pixel_weights=pw, fresh_below=0.6)
    for t, sc in enumerate(order):
        assert np.array_equal(c[t], _reference(z, metas[sc], [E[t]], b._wsum[sc], RC.WSUM, 0.6, pw[t:t + 1])[0]), t
    # the gated tick: view 0 again for scene 0, view 1 again for scene 1 (both redundant), view 3 for scene 2 (new)
    before = {k: getattr(b, k).clone() for k in ('_sum', '_wsum', '_count', '_mean', '_valid')}
    vs, sc = [0, 1, 3], [0, 1, 2]
    cov = b.coverage([E[v] for v in vs], sc)
    assert cov[0, 1] == 0 and cov[1, 1] == 0 and cov[2, 1] > 0
    thr = float(cov[2, 1] / cov[2, 0]) / 2
    calls = _count_features(b)
    x = img[torch.tensor(vs, device='cuda')].contiguous()
    assert b.add_views(x, [E[v] for v in vs], sc, weights=[1.0, 1.0, 0.5], min_novelty=thr) is b
    assert b.last_admitted == [False, False, True] and calls == [1] and b.n_views == [1, 1, 2]
    for k, v in before.items():
        assert _same_bits(getattr(b, k)[:2], v[:2]), (k, 'scenes 0 and 1 were rejected whole: untouched, not faded')
    assert not _same_bits(b._wsum[2], before['_wsum'][2])
    twin.add_views(img[3:4].contiguous(), E[3:4], [2], weights=[0.5])
    for k in before:
        assert _same_bits(getattr(b, k), getattr(twin, k)), k
    # every view rejected: nothing runs, nothing changes
    now = {k: getattr(b, k).clone() for k in before}
    b.add_views(img[:1].contiguous(), E[:1], [0], min_novelty=0.01)
    assert b.last_admitted == [False] and calls == [1] and all(_same_bits(getattr(b, k), v) for k, v in now.items()) and b.n_views == [1, 1, 2]
    b.add_views(img[4:5].contiguous(), E[4:5], [1])
    assert b.last_admitted is None and b.n_views == [1, 2, 2]
    assert len(b.detect()) == 3
    b.close()
    twin.close()


def test_windowed_batch_coverage_reads_the_refreshed_masks(z):
    model, E, img = z['model'], z['E'], z['img']
    metas = _scene_metas(z)
    b = model.open_scenes(metas, window=2)
    b.add_views(img[:3].contiguous(), E[:3], [0, 2, 0])
    order = [0, 1, 2, 2, 0]
    c = b.coverage(E, order)
    assert not b._scenes[0]._stale and not b._scenes[2]._stale
    for t, sc in enumerate(order):
        state = b._valid[sc] if sc != 1 else None
        assert np.array_equal(c[t], _reference(z, metas[sc], [E[t]], state, RC.MASK if sc != 1 else RC.NONE)[0]), t
    assert c[0, 1] == 0 and c[1, 1] == c[1, 0] > 0
    b.close()


def test_an_ungated_add_launches_what_it_launched_before(z, monkeypatch):
    """min_novelty=None: the ops of tests/test_gpu_scene_dispatch.py and no coverage launch; a gated add launches one view_coverage before them, a
    rejected one the view_coverage alone."""
    from imvoxelnet_amd import ops
    seen = []
    for name in ('backproject_accum_', 'backproject_lists_accum_', 'backproject_weighted_accum_', 'backproject_gather_mean_', 'volume_mean', 'view_coverage'):
        monkeypatch.setattr(ops, name, (lambda n, fn: (lambda *a, **k: (seen.append(n), fn(*a, **k))[1]))(name, getattr(ops, name)))

    def take():
        got = dict(collections.Counter(seen))
        seen.clear()
        return got

    s = z['model'].open_scene(z['scene_meta'])
    s.add_views(*_views(z, [0, 1]))
    assert take() == {'backproject_accum_': 1}
    s.volume()
    assert take() == {}
    s.add_views(*_views(z, [2]), min_novelty=0.01)
    assert take() == {'view_coverage': 1, 'backproject_accum_': 1} and s.last_admitted == [True]
    s.add_views(*_views(z, [2]), min_novelty=0.01)
    assert take() == {'view_coverage': 1} and s.last_admitted == [False]
    s.add_views(*_views(z, [3]), emit=False)
    s.volume()
    assert take() == {'backproject_accum_': 1, 'volume_mean': 1}
    s.close()
    b = z['model'].open_scenes(_scene_metas(z))
    b.add_views(z['img'][:2].contiguous(), z['E'][:2], [1, 0])
    assert take() == {'backproject_lists_accum_': 1}
    b.add_views(z['img'][:3].contiguous(), z['E'][:3], [1, 0, 2], min_novelty=0.01)
    assert take() == {'view_coverage': 1, 'backproject_lists_accum_': 1} and b.last_admitted == [False, False, True]
    b.close()
