"""-m gpu: sliding-window scenes -- the gathered lift (ops.backproject_gather_mean, ivx_backproject_gather_fwd) against the imported
reference's golden vectors and against the contiguous lift of the same views, bit for bit, and windowed SceneSessions
(model.open_scene(meta, window=W)) against fresh unbounded sessions that are given only the views in the window."""
import numpy as np
import pytest
import torch

from imvoxelnet_amd.workloads import _look_at
from test_gpu_scene_stream import _golden, _wide_case, _indoor_small, _anchor_small, _same_results

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ia():
    import imvoxelnet_amd
    from imvoxelnet_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    return imvoxelnet_amd


def _pool(feat, proj, slots, S, fill=float('nan')):
    """feat [n,1,FH,FW,C] / proj [n,3,4] -> pools of S slots with view i in slot slots[i]; every other slot holds `fill`."""
    pool = torch.full((S,) + tuple(feat.shape[1:]), fill, device=feat.device, dtype=feat.dtype)
    ppool = torch.full((S, 3, 4), fill, device=feat.device, dtype=torch.float32)
    idx = torch.tensor(slots, device=feat.device)
    pool[idx] = feat
    ppool[idx] = proj
    return pool, ppool


# ------------------------------------------------------------------ golden, pinned to the imported reference
def _restate(c, views):
    """The mean over the listed views from the golden PER-VIEW volumes / masks: a sequential fp32 sum in list order, divided by the
    count, 0 where no view sees the voxel (detectors/imvoxelnet.py:70-74).  -> mean [C,X,Y,Z], valid [X,Y,Z]."""
    vol, ok = c['volume'], c['valid']
    s, n = np.zeros(vol.shape[1:], np.float32), np.zeros(ok.shape[1:], np.int32)
    for v in views:
        s = s + np.where(ok[v], vol[v], np.float32(0))
        n = n + ok[v]
    assert s.dtype == np.float32
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = np.where(n > 0, s / n.astype(np.float32), np.float32(0)).astype(np.float32)
    return mean, n[0] > 0


GOLDEN_SLOTS = {'C': ([7, 2, 5, 0, 8, 3], 9), 'B': ([3, 1], 4)}
GOLDEN_LISTS = [('C', v) for v in [(0, 1, 2, 3, 4, 5), (1, 2, 3, 4), (2, 3, 4, 5), (4, 5), (5,), (0, 2, 3)]] + [('B', v) for v in [(0, 1), (0,), (1,)]]


@pytest.fixture(scope='module')
def golden(ia):
    out = {}
    for case, (slots, S) in GOLDEN_SLOTS.items():
        c, feat, P, no, crop, vs, nv = _golden(case)
        pool, ppool = _pool(feat, P[0], slots, S)
        out[case] = dict(c=c, pool=pool, ppool=ppool, slots=slots, no=no, crop=crop, vs=vs, nv=nv)
    return out


@pytest.mark.parametrize('case,views', GOLDEN_LISTS, ids=[f'{k}-{"_".join(map(str, v))}' for k, v in GOLDEN_LISTS])
def test_gathered_lift_equals_reference_bit_for_bit(ia, golden, case, views):
    """The golden maps sit in scattered slots of a pool whose other slots are NaN.  Listed in view order the lift is the imported
    reference's mean and mask; a sublist is the reference's per-view volumes summed in list order (fp32) and divided by the count.
    C = 8: a 2-lane group, so (0, 2, 3) takes a partial second round of the projection loop and (5,) a single partial one; 784 / 864
    voxels: a partial last workgroup.  No NaN may come out: an unlisted slot is never read."""
    from imvoxelnet_amd import ops
    g = golden[case]
    c = g['c']
    mean, ok = _restate(c, views)
    if len(views) == c['volume'].shape[0]:
        assert np.array_equal(mean, c['mean']) and np.array_equal(ok, c['mean_valid'][0]), 'the restatement must reproduce the golden mean'
    else:
        assert (mean != c['mean']).sum() > 1000, 'a sublist that does not change the mean tests nothing'
    vol, valid = ops.backproject_gather_mean(g['pool'], g['ppool'], [[g['slots'][v] for v in views]], g['no'], g['crop'], g['vs'], g['nv'])
    got = vol[0].permute(3, 0, 1, 2).cpu().numpy()
    assert not np.isnan(got).any()
    assert np.array_equal(got, mean), f'{(got != mean).sum()} voxel-channels differ'
    assert valid.dtype == torch.bool and np.array_equal(valid[0].cpu().numpy(), ok)
    assert bool(torch.isnan(g['pool']).any()), 'the pool keeps its NaN slots'


# ------------------------------------------------------------------ the order of the list is observable
@pytest.fixture(scope='module')
def circle(ia):
    """The four circle cameras and the 24 x 24 x 8 grid of _indoor_small, seeded random 24 x 32 maps with C = 8."""
    model, scene_meta, E, _ = _indoor_small(ia)
    meta = dict(scene_meta, lidar2img=dict(scene_meta['lidar2img'], extrinsic=list(E)))
    proj, no, crop = model._camera_setup([meta], 4, torch.device('cuda'))
    feat = torch.randn(4, 1, 24, 32, 8, generator=torch.Generator().manual_seed(41)).cuda()
    return dict(feat=feat, proj=proj, no=no, crop=crop, vs=model.voxel_size, nv=model.n_voxels)


def _contiguous(ops, z, order, **kw):
    idx = torch.tensor(order, device='cuda')
    return ops.backproject_mean(z['feat'][idx].contiguous(), z['proj'][:, idx].contiguous(), z['no'], z['crop'], z['vs'], z['nv'], **kw)


def test_circle_case_can_show_the_order(ia, circle):
    """The preconditions of the next test: enough voxels are seen by three or more views, and the parent kernel's own result depends
    on the order of the views somewhere (a sum of two terms commutes; a sum of three does not)."""
    from imvoxelnet_amd import ops
    _, count = ops.backproject_sum(circle['feat'], circle['proj'], circle['no'], circle['crop'], circle['vs'], circle['nv'])
    print('voxels seen by >= 3 views:', int((count >= 3).sum()), 'by none:', int((count == 0).sum()), 'of', count.numel())
    assert int((count >= 3).sum()) >= 100
    a, b = _contiguous(ops, circle, (0, 1, 2, 3))[0], _contiguous(ops, circle, (3, 2, 1, 0))[0]
    assert not torch.equal(a, b), 'reversing the views must change some bits, or the order is not observable here'


@pytest.mark.parametrize('order', [(0, 1, 2, 3), (3, 2, 1, 0), (2, 0, 3, 1), (1, 1, 3)], ids=lambda o: '_'.join(map(str, o)))
def test_gathered_lift_follows_the_list_order(ia, circle, order):
    """The gathered lift over a list == ops.backproject_mean over the contiguous copy in that order (the non-gathered kernel, pinned to
    the reference); (1, 1, 3): a slot listed twice counts twice."""
    from imvoxelnet_amd import ops
    slots = [4, 0, 5, 2]
    pool, ppool = _pool(circle['feat'], circle['proj'][0], slots, 6)
    ref, ref_valid = _contiguous(ops, circle, order)
    vol, valid = ops.backproject_gather_mean(pool, ppool, [[slots[v] for v in order]], circle['no'], circle['crop'], circle['vs'], circle['nv'])
    assert torch.equal(vol, ref) and torch.equal(valid, ref_valid) and not bool(torch.isnan(vol).any())


# ------------------------------------------------------------------ width, batch, element types, sampling rule
WIDE = [(256, torch.float32, 'nearest'), (512, torch.float32, 'nearest'), (256, torch.bfloat16, 'nearest'), (256, torch.float32, 'bilinear'),
        (8, torch.float32, 'bilinear'), (8, torch.bfloat16, 'bilinear')]


@pytest.mark.parametrize('C,dtype,sampling', WIDE, ids=[f'C{c}-{str(d).split(".")[1]}-{s}' for c, d, s in WIDE])
def test_wide_channels_batch_types_and_rule_equal_contiguous(ia, C, dtype, sampling):
    """B = 2 over one pool of 14 slots: each sample lists five of its own six views in its own order (the second with a repeat) and
    has its own crop.  C = 256: 64 lanes per voxel; C = 512: two channel chunks per lane; bf16 maps; the bilinear rule at both widths.
    torch.equal to ops.backproject_mean over the contiguous copy with the same rule; as a device list the same."""
    from imvoxelnet_amd import ops
    feat, P, no, crop, vs, nv = _wide_case(C, dtype)
    perm = [9, 3, 12, 0, 7, 5, 13, 1, 10, 4, 8, 2]                           # view i of the 12 sits in slot perm[i]; slots 6 and 11 stay NaN
    pool, ppool = _pool(feat, P.reshape(12, 3, 4), perm, 14)
    lists = [[4, 1, 3, 0, 2], [2, 5, 0, 0, 3]]
    idx = torch.tensor([b * 6 + v for b in range(2) for v in lists[b]], device='cuda')
    ref, ref_valid = ops.backproject_mean(feat[idx].contiguous(), torch.stack([P[b, torch.tensor(lists[b], device='cuda')] for b in range(2)]).contiguous(),
                                          no, crop, vs, nv, sampling=sampling)
    view_slot = [[perm[b * 6 + v] for v in lists[b]] for b in range(2)]
    vol, valid = ops.backproject_gather_mean(pool, ppool, view_slot, no, crop, vs, nv, sampling=sampling)
    assert vol.dtype == dtype and torch.equal(vol, ref) and torch.equal(valid, ref_valid) and not bool(torch.isnan(vol.float()).any())
    assert not torch.equal(ref_valid[0], ref_valid[1]), 'the two samples must differ for the batch index to be tested'
    vol2, valid2 = ops.backproject_gather_mean(pool, ppool, torch.tensor(view_slot, dtype=torch.int32).cuda(), no, crop, vs, nv, sampling=sampling)
    assert torch.equal(vol2, ref) and torch.equal(valid2, ref_valid)


# ------------------------------------------------------------------ the guard
@pytest.mark.parametrize('sampling', ['nearest', 'bilinear'])
def test_out_of_range_slots_are_unseen_views(ia, sampling):
    """A device list is used as it is.  Slots -1 and S in it give exactly the result of the list without them.  The pools are views
    [1 : 1 + S] of allocations two slots larger whose outer slots hold a large finite sentinel, so a missing guard reads memory this
    test owns: a sentinel projection row puts every voxel at pixel (1, 1) of a sentinel map, and 1e30 shows up in the volume."""
    from imvoxelnet_amd import ops
    c, feat, P, no, crop, vs, nv = _golden('C')
    S = 6
    big, pbig = _pool(feat, P[0], list(range(1, 1 + S)), S + 2, fill=1e30)
    pool, ppool = big[1:1 + S], pbig[1:1 + S]
    assert pool.is_contiguous() and float(big[0].min()) > 1e29 and float(big[S + 1].min()) > 1e29 and float(pbig[0].min()) > 1e29

    def dev(l):
        return torch.tensor([l], dtype=torch.int32).cuda()

    ref, ref_valid = ops.backproject_gather_mean(pool, ppool, dev([0, 1, 2, 3, 4, 5]), no, crop, vs, nv, sampling=sampling)
    if sampling == 'nearest':
        assert np.array_equal(ref[0].permute(3, 0, 1, 2).cpu().numpy(), c['mean'])
    vol, valid = ops.backproject_gather_mean(pool, ppool, dev([0, -1, 1, S, 2, 3, 4, 5]), no, crop, vs, nv, sampling=sampling)
    assert float(vol.abs().max()) < 1e20, 'a sentinel slot was read'
    assert torch.equal(vol, ref) and torch.equal(valid, ref_valid)
    vol, valid = ops.backproject_gather_mean(pool, ppool, dev([S, -1]), no, crop, vs, nv, sampling=sampling)      # nothing but unseen views
    assert not bool(vol.any()) and not bool(valid.any())


# ------------------------------------------------------------------ the session
def _family(ia, family, **prepare_kw):
    """Five views of a small scene: model, scene meta, extrinsics, images [5,3,H,W]."""
    if family == 'indoor':
        model, scene_meta, E, img = _indoor_small(ia)                          # V = 4 on the circle, and a fifth camera off it
        E = list(E) + [_look_at((1.8 * np.cos(1.9), 1.8 * np.sin(1.9), 1.0), (0, 0, .5))]
        img = torch.cat([img, torch.randn(1, 3, *img.shape[2:], generator=torch.Generator().manual_seed(10)).cuda()]).contiguous()
    else:
        model, scene_meta, E, img = _anchor_small(ia, V=5)
    model.prepare(torch.device('cuda'), **prepare_kw)
    assert all(e.dtype == np.float32 for e in E)
    return dict(model=model, scene_meta=scene_meta, E=E, img=img)


@pytest.fixture(scope='module')
def families(ia):
    cache = {}

    def get(family):
        if family not in cache:
            cache[family] = _family(ia, family)
        return cache[family]
    return get


def _fresh(z, views):
    """What the parent commit gives for exactly these views: an unbounded session that gets them one at a time, in this order."""
    s = z['model'].open_scene(z['scene_meta'])
    for v in views:
        s.add_views(z['img'][v:v + 1], [z['E'][v]])
    vol, valid = s.volume()
    out = dict(vol=vol.clone(), valid=valid.clone(), det=s.detect(), E=list(s.meta['lidar2img']['extrinsic']))
    assert s._sum is not None and s._ring is None
    s.close()
    return out


def _assert_scene_is(win, z, views, ids):
    ref = _fresh(z, views)
    assert win.view_ids == list(ids) and win.n_views == len(views)
    ext = win.meta['lidar2img']['extrinsic']
    assert len(ext) == len(views) and all(np.array_equal(a, z['E'][v]) for a, v in zip(ext, views))
    vol, valid = win.volume()
    assert not win._stale
    assert vol.dtype == ref['vol'].dtype and torch.equal(vol, ref['vol']) and torch.equal(valid, ref['valid'])
    assert 0 < int(valid.sum()) < valid.numel()
    _same_results(win.detect(), ref['det'])
    return ref


def _add(win, z, v):
    return win.add_views(z['img'][v:v + 1], [z['E'][v]])


def _window_of_two(z):
    win = z['model'].open_scene(z['scene_meta'], window=2)
    assert win._window == 2 and win.view_ids == []
    n_det = []
    for k in range(4):
        _add(win, z, k)
        assert win._stale and win._sum is None and win._count is None
        views = list(range(max(0, k - 1), k + 1))
        ref = _assert_scene_is(win, z, views, views)
        n_det.append(len(ref['det'][0]['scores_3d']))
    assert tuple(win._ring.shape[:2]) == (2, 1) and win._ring.dtype == win.volume()[0].dtype and tuple(win._pring.shape) == (2, 3, 4)
    win.close()
    return n_det


@pytest.mark.parametrize('family', ['indoor', 'anchor'])
def test_window_of_two_equals_fresh_sessions(ia, families, family):
    """window=2, views arriving one at a time: after every arrival volume(), detect(), view_ids, n_views and the meta's extrinsics are
    those of a fresh unbounded session given only the views in the window, in order (same trunk calls, so the same features; the
    accumulate path is the one-shot lift bit for bit)."""
    n_det = _window_of_two(families(family))
    print(family, 'detections per arrival', n_det)
    assert max(n_det) > 0


@pytest.mark.parametrize('family', ['indoor', 'anchor'])
def test_remove_refill_and_reset(ia, families, family):
    """W = 4 with four views in: remove_views([1]) == a fresh session of 0, 2, 3; the next arrival fills the freed slot and the scene
    == a fresh session of 0, 2, 3, 4; reset() and re-adding reproduces the first result, ids from 0 again."""
    z = families(family)
    win = z['model'].open_scene(z['scene_meta'], window=4)
    for v in range(4):
        _add(win, z, v)
    first = _assert_scene_is(win, z, [0, 1, 2, 3], [0, 1, 2, 3])
    assert [v[1] for v in win._views] == [0, 1, 2, 3]
    assert win.remove_views([1]) is win and win._stale
    after = _assert_scene_is(win, z, [0, 2, 3], [0, 2, 3])
    assert not torch.equal(after['vol'], first['vol'])
    _add(win, z, 4)
    assert [v[1] for v in win._views] == [0, 2, 3, 1], 'the new view takes the freed slot'
    _assert_scene_is(win, z, [0, 2, 3, 4], [0, 2, 3, 4])
    ring = win._ring
    win.reset()
    assert win.view_ids == [] and win.n_views == 0 and win.meta['lidar2img']['extrinsic'] == []
    with pytest.raises(RuntimeError, match='no views'):
        win.volume()
    for v in range(4):
        _add(win, z, v)
    assert win._ring is ring, 'reset() keeps the buffers'
    vol, valid = win.volume()
    assert win.view_ids == [0, 1, 2, 3] and torch.equal(vol, first['vol']) and torch.equal(valid, first['valid'])
    _same_results(win.detect(), first['det'])
    with pytest.raises(KeyError):
        win.remove_views([4])
    with pytest.raises(ValueError, match='do not fit'):
        win.add_views(z['img'], z['E'])
    assert win.view_ids == [0, 1, 2, 3] and torch.equal(win.volume()[0], first['vol'])
    win.close()
    assert win._ring is None
    with pytest.raises(RuntimeError, match='closed'):
        win.detect()


def test_two_windowed_sessions_do_not_disturb_each_other(ia, families):
    z = families('indoor')
    a, b = z['model'].open_scene(z['scene_meta'], window=2), z['model'].open_scene(z['scene_meta'], window=2)
    """Two windowed sessions on one model, adds interleaved: each has its own ring and list."""
    for va, vb in zip((0, 1, 2), (3, 2, 0)):
        _add(a, z, va)
        _add(b, z, vb)
    va, vb = a.volume()[0].clone(), b.volume()[0].clone()      # views (1, 2) and views (2, 0)
    assert not torch.equal(va, vb)
    _add(b, z, 1)
    b.volume()
    assert torch.equal(a.volume()[0], va), "`b`'s add and lift touched `a`'s volume"
    _assert_scene_is(a, z, [1, 2], [1, 2])
    _assert_scene_is(b, z, [0, 1], [2, 3])
    a.close()
    b.close()


def test_add_views_u8_on_a_windowed_session(ia, families):
    """uint8 frames through add_views_u8 == add_views on prepare_images_device's output, call by call, on windowed sessions."""
    from imvoxelnet_amd.data import prepare_images_device
    z = families('indoor')
    model, E = z['model'], z['E']
    rng = np.random.default_rng(71)
    frames = [rng.integers(0, 256, (190, 256, 3), dtype=np.uint8) for _ in range(3)]       # -> 95 x 128 in a 96 x 128 plane
    user = {k: v for k, v in z['scene_meta'].items() if k not in ('img_shape', 'ori_shape', 'pad_shape')}
    calls = [(0, 2), (2, 3)]                             # two frames, then one more: the window of two drops frame 0
    img0, shapes = prepare_images_device([frames[:2]], (128, 96))
    a, b = model.open_scene(dict(user, **shapes[0]), window=2), model.open_scene(user, window=2)
    for lo, hi in calls:
        img, _ = prepare_images_device([frames[lo:hi]], (128, 96))
        a.add_views(img[0], E[lo:hi])
        b.add_views_u8(frames[lo:hi], E[lo:hi], (128, 96))
        assert all(tuple(b.meta[k]) == tuple(shapes[0][k]) for k in ('img_shape', 'ori_shape', 'pad_shape'))
        (va, oa), (vb, ob) = a.volume(), b.volume()
        assert a.view_ids == b.view_ids == list(range(hi - 2, hi)) and torch.equal(va, vb) and torch.equal(oa, ob) and 0 < int(oa.sum())
        _same_results(b.detect(), a.detect())
    a.close()
    b.close()


@pytest.mark.parametrize('prepare_kw', [dict(sampling='bilinear'), dict(dtype=torch.bfloat16)], ids=['bilinear', 'bf16'])
def test_window_identity_with_the_bilinear_rule_and_bf16_storage(ia, prepare_kw):
    z = _family(ia, 'indoor', **prepare_kw)
    _window_of_two(z)
    s = z['model'].open_scene(z['scene_meta'], window=2)
    _add(s, z, 0)
    assert s.volume()[0].dtype == prepare_kw.get('dtype', torch.float32) and s._ring.dtype == s._mean.dtype


def test_default_sessions_keep_their_state_and_path(ia, families):
    """open_scene(meta) is what it was: a (sum, count) state, no ring; a windowed session has the ring and no sums."""
    z = families('indoor')
    s = z['model'].open_scene(z['scene_meta'])
    _add(s, z, 0)
    assert s._window is None and s._sum is not None and s._count is not None and s._ring is None and s._pring is None and s._views == []
    assert s.view_ids == [0] and not s._stale
    with pytest.raises(RuntimeError, match='window='):
        s.remove_views([0])
    w = z['model'].open_scene(z['scene_meta'], window=3)
    _add(w, z, 0)
    assert w._sum is None and w._count is None and w._ring is not None and w._ring.shape[0] == 3
    assert torch.equal(w.volume()[0], s.volume()[0]) and torch.equal(w.volume()[1], s.volume()[1])
    s.close()
    w.close()
