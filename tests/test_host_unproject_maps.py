"""Pixel maps for the weighted lift without a device: ivx_backproject_mapped_fwd is declared, bound and exported and rejects bad arguments before
any launch; ops.backproject_mapped_accum_ / _mean_ and the sessions raise their host errors and leave buffers and scenes as they were; the strided
pick and the map rings follow their rules; the fp64 reference of tests/ref_unproject_maps.py is checked against ref_unproject_weighted and the
maps the GPU tests use are shown not to be vacuous."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import ref_unproject as R
import ref_unproject_maps as RM
import ref_unproject_weighted as RW
from helpers import ROOT

NAME = 'ivx_backproject_mapped_fwd'
MEAN, SUM, ACCUM = 0, 1, 2
INF, NAN = float('inf'), float('nan')


def test_entry_point_declared_bound_and_exported():
    from imvoxelnet_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'imvoxel.h')).read()
    assert NAME in set(re.findall(r'\b(ivx_[a-z0-9_]+)\s*\(', header)), f'{NAME} is not declared in include/imvoxel.h'
    L = _lib.lib()
    assert NAME in _lib.EXPORTS and hasattr(L, NAME) and getattr(L, NAME).argtypes is not None and len(getattr(L, NAME).argtypes) == 13
    assert L.ivx_version() >= 500
    assert 'typedef struct ivx_lift_maps' in header
    assert [f[0] for f in _lib.LiftMaps._fields_] == ['pixel_weight', 'depth', 'behind', 'front']
    body = header[header.index('typedef struct ivx_lift_maps'):header.index('} ivx_lift_maps;')]
    order = [body.index(f) for f in ('*pixel_weight;', '*depth;', 'behind,', 'front;')]
    assert order == sorted(order), 'the header and the binding list the fields in one order'
    assert ctypes.sizeof(_lib.LiftMaps) == 2 * ctypes.sizeof(ctypes.c_void_p) + 8
    for prop in ('No maps.', 'Neutral maps.', 'Constant map.', 'Blocked view.', 'Power of two.'):
        assert prop in header, prop
    for src in ('model.cpp', 'api_common.cpp'):        # also compiled into the CPU restatement of the ABI, which does not define it
        text = open(os.path.join(ROOT, 'imvoxelnet_amd', 'csrc', src)).read()
        for name in (NAME, 'ivx_lift_maps'):
            assert name not in text, (src, name)


def test_mapped_argument_validation_without_gpu():
    """Every pre-launch rejection: status -1 with its message, which names the export; nothing launched (the dummy pointers are never dereferenced)."""
    from imvoxelnet_amd import _lib
    L = _lib.lib()
    fn = getattr(L, NAME)
    p = ctypes.c_void_p(64)

    def call(maps=True, pw=p, depth=p, gate=(0.25, 0.5), weights=True, forget_below=0.0, wsum=None, decay=None, lists=True, count=None, valid=p, mode=MEAN, C=8,
             R_=2):
        d = _lib.BackprojectDesc(2, 2, 6, 8, C, 4, 4, 2, (ctypes.c_float * 3)(.5, .5, .5), 0, mode, 0, 0)
        l = _lib.LiftLists(3, R_, p, p, None)
        w = _lib.LiftWeights(p, decay, forget_below, wsum)
        m = _lib.LiftMaps(pw, depth, *gate)
        return fn(ctypes.byref(d), ctypes.byref(l) if lists else None, ctypes.byref(w) if weights else None, ctypes.byref(m) if maps else None, p, p, p, p, p,
                  count, None, valid, None)

    def accum(**kw):
        return call(**dict(dict(mode=ACCUM, count=p, valid=None, wsum=p), **kw))

    def err():
        return L.ivx_last_error()

    for c in (call, accum):
        for gate in ((-0.25, 0.5), (0.25, -1e-30), (NAN, 0.5), (0.25, NAN), (-INF, INF)):
            assert c(gate=gate) == -1 and b'gate' in err() and b'>= 0' in err() and NAME.encode() in err(), gate
            assert c(gate=gate, pw=None) == -1 and b'gate' in err(), gate
        # everything the weighted entry rejects, with maps, without the struct and with an empty struct
        for kw in (dict(), dict(maps=False), dict(pw=None, depth=None), dict(depth=None, gate=(NAN, -1.0))):
            assert c(weights=False, **kw) == -1 and b'null weights' in err() and NAME.encode() in err(), kw
            assert c(forget_below=-1.0, **kw) == -1 and b'forget_below' in err() and NAME.encode() in err(), kw
            assert c(lists=False, **kw) == -1 and b'null lists' in err(), kw
            assert c(C=6, **kw) == -1 and b'C % 4' in err(), kw
            assert c(R_=0, **kw) == -1 and b'rows' in err(), kw
    assert accum(wsum=None) == -1 and b'null wsum' in err() and NAME.encode() in err()
    assert call(wsum=p) == -1 and b'the mean mode takes no wsum' in err()
    assert call(decay=p) == -1 and b'the mean mode takes no decay list' in err()
    assert call(mode=SUM, count=p, valid=None) == -1 and b'IVX_LIFT_MEAN | IVX_LIFT_ACCUM' in err()
    with pytest.raises(ValueError, match=NAME):
        _lib.check(call(gate=(-1.0, 0.0)), NAME)


def _host_args(S=4, R_=3, C=8):
    pool, ppool = torch.zeros(S, 1, 4, 5, C), torch.zeros(S, 3, 4)
    no, crop = torch.zeros(2, 3), torch.zeros(2, 2, dtype=torch.int32)
    st = dict(sum=torch.full((R_, 2, 2, 2, C), 3.0), wsum=torch.full((R_, 2, 2, 2), 5.0), count=torch.full((R_, 2, 2, 2), 9, dtype=torch.int32),
              mean=torch.full((R_, 2, 2, 2, C), -7.0), valid=torch.full((R_, 2, 2, 2), 7, dtype=torch.uint8))
    return pool, ppool, no, crop, st


def test_ops_raise_their_host_errors_and_leave_the_buffers():
    """Host tensors throughout, so nothing here can reach a launch: the gate and the maps' shapes are host rules (ValueError / TypeError) and come
    before the first device check; arguments that pass them stop at the first host tensor (RuntimeError).  The state buffers keep every value."""
    from imvoxelnet_amd import ops
    pool, ppool, no, crop, st = _host_args()
    before = {k: v.clone() for k, v in st.items()}
    vs = (1, 1, 1)
    good = torch.ones(4, 4, 5)

    def accum(lists=([0, 1, 2], [3]), weights=(1, .5, 2, 0), rows=(2, 0), **kw):
        return ops.backproject_mapped_accum_(pool, ppool, [list(l) for l in lists], weights, list(rows), [True, False], (1.0, .5), no, crop, vs, st['sum'], st['wsum'],
                                             st['count'], st['mean'], st['valid'], **kw)

    def mean(lists=([0, 1, 2], [3]), weights=(1, .5, 2, 0), rows=(2, 0), **kw):
        return ops.backproject_mapped_mean_(pool, ppool, [list(l) for l in lists], weights, list(rows), no, crop, vs, st['mean'], st['valid'], **kw)

    for op in (accum, mean):
        for gate in ((-1.0, 0.0), (0.0, -0.5), (NAN, 1.0), (1.0, NAN)):
            for kw in (dict(depth=good), dict()):                 # the gate is checked whether or not a depth map is there
                with pytest.raises(ValueError, match='gate'):
                    op(gate=gate, **kw)
        for gate in (1.0, (1.0,), (1.0, 2.0, 3.0), 'ab', torch.ones(2), (True, 1.0), ('a', 1.0)):
            with pytest.raises(TypeError, match='gate'):
                op(depth=good, gate=gate)
        for name in ('pixel_weight', 'depth'):
            for bad in (torch.ones(3, 4, 5), torch.ones(4, 5, 4), torch.ones(4, 2, 4, 5), torch.ones(4, 4, 5, 1), torch.ones(80)):
                with pytest.raises(ValueError, match=name + r' must be \[S,FH,FW\] = \[4,4,5\]'):
                    op(**{name: bad})
            with pytest.raises(TypeError, match=name):
                op(**{name: [[1.0]]})
        # what the weighted form rejects is rejected here, with and without maps
        for kw in (dict(), dict(pixel_weight=good), dict(depth=good, gate=(0.5, INF))):
            with pytest.raises(ValueError, match='distinct'):
                op(rows=(1, 1), **kw)
            with pytest.raises(ValueError, match=r'outside \[0, 4\)'):
                op(lists=([0, 4], [1]), **kw)
            with pytest.raises(ValueError, match='weights must be finite and >= 0'):
                op(weights=(1, NAN, 1, 1), **kw)
            with pytest.raises(ValueError, match='sampling'):
                op(sampling='cubic', **kw)
            with pytest.raises(RuntimeError, match='pool must be a device'):     # everything host-checkable passed ([S,1,FH,FW] too)
                op(**{k: (v[:, None] if isinstance(v, torch.Tensor) else v) for k, v in kw.items()})
    with pytest.raises(ValueError, match='both be given or both be None'):
        ops.backproject_mapped_accum_(pool, ppool, [[0], [1]], None, [0, 1], [True, True], None, no, crop, vs, st['sum'], st['wsum'], st['count'], st['mean'], None,
                                      pixel_weight=good)
    assert ops.check_gate((0, INF)) == (0.0, INF) and ops.check_gate([np.float32(0.25), 1]) == (0.25, 1.0)
    for k in st:
        assert torch.equal(st[k], before[k]), k


# ------------------------------------------------------------------ sessions
K4 = np.array([[90., 0, 63.5, 0], [0, 90., 47.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
META = dict(img_shape=(96, 128, 3), ori_shape=(96, 128, 3), lidar2img=dict(intrinsic=K4, origin=np.array([0, 0, .5], np.float32)))
E4 = np.eye(4, dtype=np.float32)


def _mock_model(**kw):
    return types.SimpleNamespace(**dict(dict(head_2d=None), **kw))


def test_sessions_decide_at_open_and_refuse_before_any_launch():
    from imvoxelnet_amd import SceneBatch, SceneSession
    m = _mock_model()
    for bad in ((-1.0, 0.0), (0.0, NAN), (NAN, NAN)):
        with pytest.raises(ValueError, match='gate'):
            SceneSession(m, META, decay=1.0, depth_gate=bad)
        with pytest.raises(ValueError, match='gate'):
            SceneBatch(m, [META, META], window=2, depth_gate=bad)
    for bad in (0.5, (1.0,), 'xy'):
        with pytest.raises(TypeError, match='gate'):
            SceneSession(m, META, window=2, depth_gate=bad)
    with pytest.raises(ValueError, match='depth_gate needs a session that takes weights'):
        SceneSession(m, META, depth_gate=(0.25, 0.5))
    img = torch.zeros(2, 3, 96, 128)
    fmap, imap = torch.ones(2, 24, 32), torch.ones(2, 96, 128)
    u8 = [np.zeros((48, 64, 3), np.uint8)] * 2
    # a plain session / batch refuses maps in the wording of the weights' refusal
    plain, pb = SceneSession(m, META), SceneBatch(m, [META, META])
    assert plain._gate is None and pb._scenes[0]._gate is None
    for kw in (dict(pixel_weights=fmap), dict(depths=fmap), dict(pixel_weights=imap, depths=imap)):
        with pytest.raises(ValueError, match=r'opened plain and takes no pixel maps: open it with decay=1\.0'):
            plain.add_views(img, [E4, E4], **kw)
        with pytest.raises(ValueError, match=r'decay=1\.0'):
            plain.add_views_u8(u8, [E4, E4], (128, 96), **kw)
        with pytest.raises(ValueError, match=r'batch was opened plain and takes no pixel maps'):
            pb.add_views(img, [E4, E4], [0, 1], **kw)
        with pytest.raises(ValueError, match=r'decay=1\.0'):
            pb.add_views_u8(u8, [E4, E4], [0, 1], (128, 96), **kw)
    assert plain.n_views == 0 and pb.n_views == [0, 0]
    # sessions that take weights: depths need the gate, and every argument is checked before anything else happens
    fading, win = SceneSession(m, META, decay=0.75), SceneSession(m, META, window=2)
    gated = [SceneSession(m, META, decay=0.75, depth_gate=(0.25, INF)), SceneSession(m, META, window=2, depth_gate=[0, 0.5])]
    assert gated[0]._gate == (0.25, INF) and gated[1]._gate == (0.0, 0.5) and fading._gate is None
    fb, wb = SceneBatch(m, [META, META], decay=[1.0, 0.5], depth_gate=(1, 2)), SceneBatch(m, [META, META], window=2)
    assert [r._gate for r in fb._scenes] == [(1.0, 2.0)] * 2
    for s in (fading, win):
        with pytest.raises(ValueError, match='opened without depth_gate and takes no depths'):
            s.add_views(img, [E4, E4], depths=fmap)
        with pytest.raises(ValueError, match='without depth_gate'):
            s.add_views_u8(u8, [E4, E4], (128, 96), depths=fmap)
    with pytest.raises(ValueError, match='batch was opened without depth_gate'):
        wb.add_views(img, [E4, E4], [0, 1], depths=fmap)
    for s in [fading, win] + gated:
        for name in ('pixel_weights',) + (('depths',) if s._gate else ()):
            for bad in (torch.ones(3, 24, 32), torch.ones(24, 32), torch.ones(2, 1, 24, 32)):
                with pytest.raises(ValueError, match=name + r' must be \[V,FH,FW\]'):
                    s.add_views(img, [E4, E4], **{name: bad})
            for bad in (fmap.double(), fmap.half(), fmap.int()):
                with pytest.raises(TypeError, match=name + ' must be float32'):
                    s.add_views(img, [E4, E4], **{name: bad})
            for bad in (fmap.numpy(), [fmap[0], fmap[1]], 1.0):
                with pytest.raises(TypeError, match=name + ' must be None or one float32'):
                    s.add_views(img, [E4, E4], **{name: bad})
            with pytest.raises(RuntimeError, match='device'):          # valid arguments: stops at the host image, before any launch
                s.add_views(img, [E4, E4], **{name: fmap})
            with pytest.raises(RuntimeError, match='device'):
                s.add_views(img, [E4, E4], **{name: imap})
        assert s.n_views == 0 and s.meta['lidar2img']['extrinsic'] == [] and s._mring is None and s._dring is None and not s._stale
    with pytest.raises(ValueError, match=r'depths must be \[V,FH,FW\]'):
        fb.add_views(img, [E4, E4], [0, 1], depths=torch.ones(1, 24, 32))
    with pytest.raises(RuntimeError, match='device'):
        fb.add_views(img, [E4, E4], [0, 1], pixel_weights=fmap, depths=imap)
    assert fb.n_views == [0, 0] and fb._mring is None and fb._dring is None


def test_open_scene_passes_the_gate_on():
    import imvoxelnet_amd as ia
    from kitti_cfg import kitti_model_cfg, KITTI_TEST_CFG
    model = ia.build_detector(kitti_model_cfg(n_voxels=(24, 28, 12), in_ch=16, out_ch=32), test_cfg=KITTI_TEST_CFG)
    assert model.open_scene(META, window=2, depth_gate=(0.25, 0.5))._gate == (0.25, 0.5) and model.open_scene(META, decay=1.0)._gate is None
    assert model.open_scenes([META, META], decay=0.5, depth_gate=(0, INF))._scenes[1]._gate == (0.0, INF)
    with pytest.raises(ValueError, match='gate'):
        model.open_scene(META, window=2, depth_gate=(-1, 0))
    assert model._prepared_device is None


def test_the_strided_pick_rule():
    """A map at feature resolution is taken as it is; one at the input size becomes map[:, ::s, ::s], s = H // FH: feature pixel (x, y) is input
    pixel (s*x, s*y).  The pick moves numbers: every value is one of the input's, bit for bit.  Anything else raises."""
    from imvoxelnet_amd.scene import pick_map
    H, W, FH, FW = 96, 128, 24, 32
    full = torch.arange(2 * H * W, dtype=torch.float32).reshape(2, H, W)
    full[0, 4, 8], full[1, 0, 4] = NAN, INF
    got = pick_map(full, 'depths', (H, W), (FH, FW))
    assert tuple(got.shape) == (2, FH, FW)
    for v, y, x in ((0, 0, 0), (1, 23, 31), (0, 5, 7), (1, 11, 2)):
        assert got[v, y, x] == full[v, 4 * y, 4 * x]
    assert torch.isnan(got[0, 1, 2]) and got[1, 0, 1] == INF
    assert torch.equal(got.contiguous().view(torch.int32), full[:, ::4, ::4].contiguous().view(torch.int32))
    feat = torch.rand(2, FH, FW)
    assert pick_map(feat, 'depths', (H, W), (FH, FW)) is feat
    assert pick_map(feat, 'depths', (H, W), (FH, FW), strided=False) is feat
    with pytest.raises(ValueError, match=r'pixel_weights must be \[V,24,32\] at feature resolution \(frames that are resized'):
        pick_map(full, 'pixel_weights', (H, W), (FH, FW), strided=False)
    for bad in (torch.ones(2, 48, 64), torch.ones(2, 96, 127), torch.ones(2, 25, 32), torch.ones(2, 32, 24)):
        with pytest.raises(ValueError, match=r'depths must be \[V,24,32\] at feature resolution or \[V,96,128\] at the input size'):
            pick_map(bad, 'depths', (H, W), (FH, FW))
    # sizes the stride does not divide: the pick must come out at exactly FH x FW, with one stride for both axes
    assert tuple(pick_map(torch.ones(1, 100, 132), 'depths', (100, 132), (25, 33)).shape) == (1, 25, 33)       # s = 4 for both
    for hw in ((98, 130), (100, 130), (100, 136)):          # s = 3 gives 33 rows; s = 4 for H but 3 for W; s = 4 gives 34 columns
        with pytest.raises(ValueError, match='depths must be'):
            pick_map(torch.ones(1, *hw), 'depths', hw, (25, 33))


def test_the_map_rings_bookkeeping():
    """_ring_map on host tensors, driven by the slot rule of a windowed record: no ring until the first map; it starts filled (weights 1, depths 0);
    a reused slot takes its new view's map, or goes back to the fill when the view brings none; a ring of another feature size is dropped."""
    from imvoxelnet_amd import SceneBatch, SceneSession
    from imvoxelnet_amd.scene import MAP_FILL, _ring_map
    assert MAP_FILL == {'pixel_weights': 1.0, 'depths': 0.0}
    cpu, fhw = torch.device('cpu'), (3, 4)
    s = SceneSession(_mock_model(), META, window=3, depth_gate=(0.25, 0.5))
    rings = {'pixel_weights': None, 'depths': None}

    def add(V, **maps):                                     # what _add_windowed does with the rings, and the record's admit
        kept, slots = s._free_slots(V)
        for name, fill in MAP_FILL.items():
            rings[name] = _ring_map(rings[name], 3, fhw, cpu, slots, maps.get(name), fill)
        s._admit(kept, slots, [E4] * V, (96, 128))
        return slots

    assert add(1) == [0] and rings == {'pixel_weights': None, 'depths': None}, 'no map given: no ring'
    w1 = torch.full((2, 3, 4), 0.5)
    assert add(2, pixel_weights=w1) == [1, 2]
    assert rings['depths'] is None and torch.equal(rings['pixel_weights'], torch.stack([torch.ones(3, 4), w1[0], w1[1]]))
    d2 = torch.full((1, 3, 4), 2.0)
    assert add(1, depths=d2) == [0]                         # the oldest view leaves, its slot is reused: no weight map -> back to 1
    assert torch.equal(rings['depths'], torch.stack([d2[0], torch.zeros(3, 4), torch.zeros(3, 4)])) and bool((rings['pixel_weights'][0] == 1).all())
    rings['pixel_weights'][0] = 7.0
    s.remove_views([1])                                     # frees slot 1; eviction and removal touch no ring
    assert bool((rings['pixel_weights'][1] == 0.5).all())
    assert add(1) == [1]                                    # reused without any map: weight 1, depth 0 (no measurement)
    assert bool((rings['pixel_weights'][1] == 1).all()) and bool((rings['depths'][1] == 0).all())
    assert bool((rings['pixel_weights'][0] == 7).all()) and bool((rings['pixel_weights'][2] == 0.5).all()) and bool((rings['depths'][0] == 2).all())
    assert add(2, pixel_weights=w1 * 4, depths=torch.cat([d2, d2 * 2])) == [0, 2]        # views 3 and 4 stay newest of W - V = 1 ... slot 1 is kept
    assert bool((rings['pixel_weights'][0] == 2).all()) and bool((rings['depths'][2] == 4).all()) and bool((rings['pixel_weights'][1] == 1).all())
    # another feature size: the old ring is dropped, and without a map none is made
    assert _ring_map(rings['depths'], 3, (2, 2), cpu, [0], None, 0.0) is None
    r = _ring_map(rings['depths'], 3, (2, 2), cpu, [1], torch.ones(1, 2, 2), 0.0)
    assert tuple(r.shape) == (3, 2, 2) and r.dtype == torch.float32 and float(r.sum()) == 4.0
    # a batch: scene s owns slots s*W .. s*W+W-1 of rings of N*W slots
    b = SceneBatch(_mock_model(), [META, META], window=2)
    assert b._scenes[1]._free_slots(2, 2)[1] == [2, 3] and b._scenes[0]._free_slots(1, 0)[1] == [0]
    r = _ring_map(None, 4, fhw, cpu, [2, 0, 3], torch.stack([torch.full(fhw, float(i)) for i in (5, 6, 7)]), 1.0)
    assert [float(r[i, 0, 0]) for i in range(4)] == [6.0, 1.0, 5.0, 7.0]
    # reset forgets the session's rings
    s._mring, s._dring = rings['pixel_weights'], rings['depths']
    s.reset()
    assert s._mring is None and s._dring is None and s._wring is None


# ------------------------------------------------------------------ the reference against ref_unproject_weighted and against itself
def _scene_feat(sample=1, Cn=5, seed=3):
    sc = R.dyadic_scene(R.NEW_ORIGIN_2, R.CROP_2) if sample else R.dyadic_scene(R.NEW_ORIGIN, R.CROP)
    feat = np.random.default_rng(seed).standard_normal((3, R.FH, R.FW, Cn)).astype(np.float32)
    return sc, feat


KEYS = ('mean', 'valid', 'count', 'W', 'A', 'S', 'M')


def _equal(a, b, keys=KEYS):
    return all(np.array_equal(a[k], b[k]) for k in keys)


@pytest.mark.parametrize('bilinear', [False, True])
def test_reference_identities(bilinear):
    sc, feat = _scene_feat()
    g = (sc['xf'], sc['yf'], sc['d'], sc['hc'], sc['wc'])
    wv = [0.5, 2.0, 1.25]
    plain = RW.weighted_mean_reference(feat, *g, [0, 1, 2], wv, bilinear)
    ones, D = np.ones((3, R.FH, R.FW), np.float32), RM.dyadic_depth()
    holes = np.asarray(RM.HOLES, np.float32)[np.arange(3 * R.FH * R.FW) % 4].reshape(3, R.FH, R.FW)

    def mapped(views=(0, 1, 2), weights=wv, **kw):
        return RM.mapped_mean_reference(feat, *g, list(views), list(weights), bilinear, **kw)

    # no maps / neutral maps: the weighted reference, in every field
    for kw in (dict(), dict(pixel_weight=ones), dict(depth=holes, gate=(0.0, 0.0)), dict(depth=D), dict(depth=D, gate=(INF, INF)), dict(pixel_weight=ones, depth=holes)):
        assert _equal(mapped(**kw), plain), sorted(kw)
    gated = mapped(depth=D, gate=RM.GATE)
    assert not np.array_equal(gated['count'], plain['count']) and not np.array_equal(gated['mean'], plain['mean']), 'the gate must matter'
    # chunked ticks with maps and fading are WeightedReference's ticks when the maps are neutral
    a, b = RM.MappedReference(feat, *g, bilinear, 0.25, ones, holes, (0.0, 0.0)), RW.WeightedReference(feat, *g, bilinear, 0.25)
    for t, views in enumerate(([0], [1, 2], [1])):
        assert _equal(a.tick(views, [wv[v] for v in views], 0.5, t == 0), b.tick(views, [wv[v] for v in views], 0.5, t == 0)), t
    # constant map: the weights become wv * c (dyadic here, so the product the reference uses as a value is the rounded one)
    c = np.asarray([1.5, 0.25, 3.0], np.float32)
    const = mapped(pixel_weight=ones * c[:, None, None])
    assert _equal(const, RW.weighted_mean_reference(feat, *g, [0, 1, 2], [w * float(x) for w, x in zip(wv, c)], bilinear))
    assert not np.array_equal(const['mean'], plain['mean'])
    # blocked view: by a weight map of nothing but 0 / NaN / negative / inf, and by a gate that excludes every voxel the view sees
    drop = RW.weighted_mean_reference(feat, *g, [0, 2], [wv[0], wv[2]], bilinear)
    assert not np.array_equal(drop['mean'], plain['mean'])
    for bad in (0.0, NAN, -1.0, INF, None):
        pw = ones.copy()
        pw[1] = np.asarray([0.0, NAN, -2.0, INF], np.float32)[np.arange(R.FH * R.FW) % 4].reshape(R.FH, R.FW) if bad is None else bad
        assert _equal(mapped(pixel_weight=pw), drop), bad
    far = np.zeros((3, R.FH, R.FW), np.float32)
    far[1] = 2.0 ** -6                                       # a surface nearer than every voxel: with behind = 0 the view counts nowhere
    ref = RM.MappedReference(feat, *g, bilinear, depth=far, gate=(0.0, INF))
    assert len(ref.classes(1)[3]) == 0 and len(ref.classes(1)[0]) == 0 and len(ref.classes(1)[1]) == int(ref.ok[1].sum()) > 0
    assert _equal(ref.tick([0, 1, 2], wv, first=True), drop)
    # x 4: the mean and the mask unchanged, the sums exactly x 4
    pw = RM.general_weight_map()
    x1, x4 = mapped(pixel_weight=pw, depth=D, gate=RM.GATE), mapped(pixel_weight=pw * 4, depth=D, gate=RM.GATE)
    assert _equal(x1, x4, ('mean', 'valid', 'count', 'A')) and np.array_equal(4 * x1['S'], x4['S']) and np.array_equal(4 * x1['W'], x4['W'])
    assert not np.array_equal(x1['mean'], gated['mean']) and not np.array_equal(x1['count'], gated['count']), 'the weight map must matter'
    assert RM.k_mapped(3, 0, False) == RW.k_weighted(3, 0, False) + 3 == 10 and RM.k_mapped(5, 2, True) == RW.k_weighted(5, 2, True) + 5 == 26
    assert RM.k_mapped(4, 1, True, weight_map=False) == RW.k_weighted(4, 1, True)


def test_the_maps_are_not_vacuous():
    """The literal class counts of the committed depth map over the (view, voxel) pairs that pass validity: holes / too far / too near / pass.
    Every kind of hole occurs under a counted pair, and the general weight map blocks some pairs and leaves most."""
    D = RM.dyadic_depth()
    assert np.array_equal(D[np.isfinite(D) & (D > 0)] * 4 % 1, np.zeros(int((np.isfinite(D) & (D > 0)).sum()))), 'quarter steps: every D +- gate is exact'
    assert D[0, 0, 1] == 1.25 and D[2, 5, 8] == 1 + 0.25 * ((8 + 10 + 2) % 5) and D[0, 0, 0] == 0 and np.isnan(D[0, 3, 1]) and D[0, 2, 2] == -1 and D[0, 1, 3] == INF
    expect = {(0, RM.GATE): [65, 86, 56, 103], (0, (0.25, INF)): [65, 86, 0, 159], (1, RM.GATE): [94, 66, 85, 138], (1, (0.25, INF)): [94, 66, 0, 223]}
    for (sample, gate), counts in expect.items():
        sc, feat = _scene_feat(sample, Cn=1)
        ref = RM.MappedReference(feat, sc['xf'], sc['yf'], sc['d'], sc['hc'], sc['wc'], depth=D, gate=gate)
        cls = [ref.classes(v) for v in range(3)]
        got = [sum(len(c[i]) for c in cls) for i in range(4)]
        print(sample, gate, got)
        assert got == counts, (sample, gate, got)
        assert sum(got) == int(ref.ok.sum())
    for sample in (0, 1):
        sc, feat = _scene_feat(sample, Cn=1)
        ref = RM.MappedReference(feat, sc['xf'], sc['yf'], sc['d'], sc['hc'], sc['wc'], depth=D, gate=RM.GATE)
        kinds = set()
        for v in range(3):
            n = ref.classes(v)[0]
            kinds |= {repr(float(x)) for x in D[v, np.rint(sc['yf'][v, n]).astype(int), np.rint(sc['xf'][v, n]).astype(int)]}
        assert kinds == {'0.0', 'nan', '-1.0', 'inf'}, kinds
        pw = RM.MappedReference(feat, sc['xf'], sc['yf'], sc['d'], sc['hc'], sc['wc'], pixel_weight=RM.general_weight_map())
        kept, seen = sum(len(pw.counted(v, 1.0)[0]) for v in range(3)), int(pw.ok.sum())
        print(sample, 'weight map: counted', kept, 'of', seen)
        assert 0.5 * seen < kept < seen


def test_the_docs():
    import imvoxelnet_amd as ia
    doc = ia.scene.__doc__
    assert 'Pixel maps' in doc and 'depth_gate' in doc
    scope = doc[doc.index('Out of scope:'):]
    assert 'per-pixel weight maps' not in scope and 'fraction of a voxel' in scope and 'Anchor3DHead' in scope
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert NAME in design and 'MAPPED' in design
    assert NAME in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert 'depth_gate' in readme and 'profiles/scene_maps.md' in readme
    for f in ('tools/scene_maps_bench.py', 'profiles/scene_maps.md'):
        assert os.path.exists(os.path.join(ROOT, f)), f
