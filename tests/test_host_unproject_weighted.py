"""The weighted listed lift without a device: ivx_backproject_weighted_fwd / ivx_volume_wmean_fwd are declared, bound and exported and reject bad
arguments before any launch; ops.backproject_weighted_accum_ / _mean_ and the fading / weighted sessions raise their host errors and leave their
buffers and scenes as they were; the fp64 reference of tests/ref_unproject_weighted.py is checked against ref_unproject and against itself."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import ref_unproject as R
import ref_unproject_weighted as RW
from helpers import ROOT

NAMES = ('ivx_backproject_weighted_fwd', 'ivx_volume_wmean_fwd')
NAME = NAMES[0]
MEAN, SUM, ACCUM = 0, 1, 2


def test_entry_points_declared_bound_and_exported():
    from imvoxelnet_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'imvoxel.h')).read()
    declared = set(re.findall(r'\b(ivx_[a-z0-9_]+)\s*\(', header))
    L = _lib.lib()
    for name in NAMES:
        assert name in declared, f'{name} is not declared in include/imvoxel.h'
        assert name in _lib.EXPORTS and hasattr(L, name) and getattr(L, name).argtypes is not None
    assert 'typedef struct ivx_lift_weights' in header
    assert L.ivx_version() >= 480
    assert [f[0] for f in _lib.LiftWeights._fields_] == ['view_weight', 'decay', 'forget_below', 'wsum']
    body = header[header.index('typedef struct ivx_lift_weights'):header.index('} ivx_lift_weights;')]
    order = [body.index(f) for f in ('view_weight;', 'decay;', 'forget_below;', 'wsum;')]
    assert order == sorted(order), 'the header and the binding list the fields in one order'
    for src in ('model.cpp', 'api_common.cpp'):        # also compiled into the CPU restatement of the ABI, which does not define them
        text = open(os.path.join(ROOT, 'imvoxelnet_amd', 'csrc', src)).read()
        for name in NAMES + ('ivx_lift_weights',):
            assert name not in text, (src, name)


def test_weighted_argument_validation_without_gpu():
    """Every pre-launch rejection: status -1 with its message, which names the export; nothing launched (the dummy pointers are never dereferenced)."""
    from imvoxelnet_amd import _lib
    L = _lib.lib()
    fn = getattr(L, NAME)
    p = ctypes.c_void_p(64)

    def call(weights=True, vw=p, decay=None, forget_below=0.0, wsum=None, lists=True, count=None, valid=p, mode=MEAN, C=8, R_=2):
        d = _lib.BackprojectDesc(2, 2, 6, 8, C, 4, 4, 2, (ctypes.c_float * 3)(.5, .5, .5), 0, mode, 0, 0)
        l = _lib.LiftLists(3, R_, p, p, None)
        w = _lib.LiftWeights(vw, decay, forget_below, wsum)
        return fn(ctypes.byref(d), ctypes.byref(l) if lists else None, ctypes.byref(w) if weights else None, p, p, p, p, p, count, None, valid, None)

    def accum(**kw):
        return call(**dict(dict(mode=ACCUM, count=p, valid=None, wsum=p), **kw))

    def err():
        return L.ivx_last_error()

    for c in (call, accum):
        assert c(weights=False) == -1 and b'null weights' in err() and NAME.encode() in err()
        for fb in (-1.0, -1e-30, float('inf'), float('nan')):
            assert c(forget_below=fb) == -1 and b'forget_below' in err() and b'finite' in err() and NAME.encode() in err(), fb
        assert c(lists=False) == -1 and b'null lists' in err() and NAME.encode() in err()          # the listed entry's rules hold
        assert c(C=6) == -1 and b'C % 4' in err()
        assert c(R_=0) == -1 and b'rows' in err()
    assert accum(wsum=None) == -1 and b'null wsum' in err() and NAME.encode() in err()
    assert call(wsum=p) == -1 and b'the mean mode takes no wsum' in err() and NAME.encode() in err()
    assert call(decay=p) == -1 and b'the mean mode takes no decay list' in err() and NAME.encode() in err()
    assert call(forget_below=0.25) == -1 and b'forget_below' in err() and b'mean mode' in err() and NAME.encode() in err()
    assert call(mode=SUM, count=p, valid=None) == -1 and b'IVX_LIFT_MEAN | IVX_LIFT_ACCUM' in err()
    assert accum(count=None) == -1 and b'updates count' in err()
    with pytest.raises(ValueError, match=NAME):
        _lib.check(accum(wsum=None), NAME)
    # ivx_volume_wmean_fwd
    wm = L.ivx_volume_wmean_fwd
    q = ctypes.c_void_p(128)
    for args in ((None, p, 8, 8, q, 0, p), (p, None, 8, 8, q, 0, p), (p, p, 8, 8, None, 0, p), (p, p, 8, 8, q, 0, None)):
        assert wm(*args, None) == -1 and b'ivx_volume_wmean_fwd: null argument' in err()
    assert wm(p, p, 8, 8, p, 0, p, None) == -1 and b'out must not be volume_sum' in err()
    assert wm(p, p, 8, 6, q, 0, p, None) == -1 and b'C % 4' in err()
    assert wm(p, p, 0, 8, q, 0, p, None) == -1 and b'bad dims' in err()
    assert wm(p, p, 8, 8, q, 2, p, None) == -1 and b'out_dtype' in err()


def _host_args(S=4, R_=3, C=8):
    pool, ppool = torch.zeros(S, 1, 4, 4, C), torch.zeros(S, 3, 4)
    no, crop = torch.zeros(2, 3), torch.zeros(2, 2, dtype=torch.int32)
    st = dict(sum=torch.full((R_, 2, 2, 2, C), 3.0), wsum=torch.full((R_, 2, 2, 2), 5.0), count=torch.full((R_, 2, 2, 2), 9, dtype=torch.int32),
              mean=torch.full((R_, 2, 2, 2, C), -7.0), valid=torch.full((R_, 2, 2, 2), 7, dtype=torch.uint8))
    return pool, ppool, no, crop, st


def test_ops_raise_their_host_errors_and_leave_the_buffers():
    """Host tensors throughout, so nothing here can reach a launch: the list, weight and decay errors come first (ValueError / TypeError), and
    arguments that pass them stop at the first host tensor (RuntimeError).  The state buffers keep every value."""
    from imvoxelnet_amd import ops
    pool, ppool, no, crop, st = _host_args()
    before = {k: v.clone() for k, v in st.items()}
    vs = (1, 1, 1)

    def accum(lists=([0, 1, 2], [3]), weights=(1, .5, 2, 0), rows=(2, 0), first=(True, False), decay=(1.0, .5), **kw):
        return ops.backproject_weighted_accum_(pool, ppool, [list(l) for l in lists], weights, list(rows), list(first), decay, no, crop, vs, st['sum'], st['wsum'],
                                               st['count'], st['mean'], st['valid'], **kw)

    def mean(lists=([0, 1, 2], [3]), weights=(1, .5, 2, 0), rows=(2, 0), **kw):
        return ops.backproject_weighted_mean_(pool, ppool, [list(l) for l in lists], weights, list(rows), no, crop, vs, st['mean'], st['valid'], **kw)

    for op in (accum, mean):
        with pytest.raises(ValueError, match='distinct'):
            op(rows=(1, 1))
        with pytest.raises(ValueError, match=r'rows must be in \[0, 3\)'):
            op(rows=(0, 3))
        with pytest.raises(ValueError, match=r'outside \[0, 4\)'):
            op(lists=([0, 4], [1]))
        for bad in (float('nan'), -1.0, -1e-9, float('inf')):
            with pytest.raises(ValueError, match='weights must be finite and >= 0'):
                op(weights=(1, bad, 1, 1))
        for n in (3, 5):                                   # one weight per slot of the pool
            with pytest.raises(ValueError, match='weights has'):
                op(weights=[1.0] * n)
        with pytest.raises(TypeError, match='weights'):
            op(weights=torch.ones(4))                      # a host tensor is neither a host list nor a device list
        with pytest.raises(ValueError, match='sampling'):
            op(sampling='cubic')
        with pytest.raises(RuntimeError, match='pool must be a device'):     # everything host-checkable passed
            op()
        with pytest.raises(RuntimeError, match='pool must be a device'):
            op(weights=None)
    for bad in (0.0, 1.5, -0.5, float('nan')):
        with pytest.raises(ValueError, match=r'decay must be in \(0, 1\]'):
            accum(decay=(1.0, bad))
    with pytest.raises(ValueError, match='decay has'):
        accum(decay=(1.0,))
    for fb in (-0.5, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='forget_below'):
            accum(forget_below=fb)
    with pytest.raises(ValueError, match='first must be a host list of 2'):
        accum(first=(True,))
    with pytest.raises(ValueError, match='both be given or both be None'):
        ops.backproject_weighted_accum_(pool, ppool, [[0], [1]], None, [0, 1], [True, True], None, no, crop, vs, st['sum'], st['wsum'], st['count'], st['mean'], None)
    with pytest.raises(RuntimeError, match='device'):
        ops.volume_wmean(st['sum'], st['wsum'])
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
    with pytest.raises(ValueError, match='decay together with window'):
        SceneSession(m, META, window=3, decay=0.5)
    with pytest.raises(ValueError, match='decay together with window'):
        SceneBatch(m, [META, META], window=3, decay=0.5)
    for bad in (0.0, 1.5, -1.0, float('nan')):
        with pytest.raises(ValueError, match=r'decay must be in \(0, 1\]'):
            SceneSession(m, META, decay=bad)
    with pytest.raises(TypeError, match='decay'):
        SceneSession(m, META, decay='fast')
    for bad in (-1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='forget_below'):
            SceneSession(m, META, decay=0.5, forget_below=bad)
    with pytest.raises(ValueError, match='forget_below needs a fading session'):
        SceneSession(m, META, forget_below=0.5)
    with pytest.raises(ValueError, match='2 decays for 3 scenes'):
        SceneBatch(m, [META] * 3, decay=[0.5, 0.5])
    with pytest.raises(NotImplementedError, match='head_2d'):
        SceneSession(_mock_model(head_2d=object()), META, decay=0.5)
    img = torch.zeros(2, 3, 96, 128)
    # a plain session / batch was opened plain: weights raise, and say how to open
    plain = SceneSession(m, META)
    assert plain._decay is None and plain._wsum is None
    with pytest.raises(ValueError, match=r'decay=1\.0'):
        plain.add_views(img, [E4, E4], weights=[1.0, 0.5])
    with pytest.raises(ValueError, match=r'decay=1\.0'):
        plain.add_views_u8([np.zeros((48, 64, 3), np.uint8)] * 2, [E4, E4], (128, 96), weights=[1.0, 0.5])
    pb = SceneBatch(m, [META, META])
    with pytest.raises(ValueError, match=r'decay=1\.0'):
        pb.add_views(img, [E4, E4], [0, 1], weights=[1.0, 0.5])
    assert plain.n_views == 0 and pb.n_views == [0, 0]
    # fading and windowed sessions check the weights before anything else happens
    fading = SceneSession(m, META, decay=0.75, forget_below=0.125)
    assert (fading._decay, fading._forget) == (0.75, 0.125)
    fb = SceneBatch(m, [META, META], decay=[1.0, 0.5])
    assert [r._decay for r in fb._scenes] == [1.0, 0.5] and fb._fading
    win = SceneSession(m, META, window=2)
    for s in (fading, win):
        with pytest.raises(ValueError, match='3 weights for 2 views'):
            s.add_views(img, [E4, E4], weights=[1, 1, 1])
        for bad in (float('nan'), -0.5, float('inf')):
            with pytest.raises(ValueError, match='weights must be finite and >= 0'):
                s.add_views(img, [E4, E4], weights=[1.0, bad])
        with pytest.raises(RuntimeError, match='device'):          # valid arguments: stops at the host tensor, before any launch
            s.add_views(img, [E4, E4], weights=[1.0, 0.0])
        assert s.n_views == 0 and s.meta['lidar2img']['extrinsic'] == []
    with pytest.raises(ValueError, match='weights must be finite'):
        fb.add_views(img, [E4, E4], [0, 1], weights=[1.0, float('nan')])
    with pytest.raises(RuntimeError, match='window='):
        fading.reweight([0], [1.0])
    with pytest.raises(RuntimeError, match='window='):
        fb.reweight(0, [0], [1.0])
    # reweight on a windowed scene: bookkeeping without a device
    win._views = [(4, 1, E4), (5, 0, E4)]
    win.n_views = 2
    with pytest.raises(KeyError, match='no view with id'):
        win.reweight([4, 7], [1.0, 2.0])
    with pytest.raises(ValueError, match='weights must be finite'):
        win.reweight([4], [-1.0])
    assert win._wring is None and not win._stale
    assert win.reweight(4, 0.25) is win and win._wring == [1.0, 0.25] and win._stale
    win.reweight([5, 4], [2.0, 0.0])
    assert win._wring == [2.0, 0.0]
    wb = SceneBatch(m, [META, META], window=2)
    wb._scenes[1]._views, wb._scenes[1].n_views = [(0, 3, E4), (1, 2, E4)], 2
    with pytest.raises(KeyError, match='no view with id'):
        wb.reweight(1, [2], [1.0])
    assert wb._wring is None
    wb.reweight(1, [1], [0.5])
    assert wb._wring == [1.0, 1.0, 0.5, 1.0] and wb._scenes[1]._stale and not wb._scenes[0]._stale


def test_the_docs_no_longer_call_reweighting_out_of_scope():
    import imvoxelnet_amd as ia
    assert 're-weighting views' not in ia.scene.__doc__
    assert 're-weighting views' not in open(os.path.join(ROOT, 'DESIGN.md')).read()


# ------------------------------------------------------------------ the reference against ref_unproject and against itself
def _scene_feat(Cn=5, seed=3):
    sc = R.dyadic_scene(R.NEW_ORIGIN_2, R.CROP_2)
    feat = np.random.default_rng(seed).standard_normal((3, R.FH, R.FW, Cn)).astype(np.float32)
    return sc, feat


def test_the_dyadic_scene_is_not_vacuous():
    """Sample 1 of the GPU tests: 131 voxels seen by view 0 but not by view 1, 73 by both, 6 by no view; view counts 6 / 110 / 82 / 12 in sample 0."""
    s0, s1 = R.dyadic_scene(R.NEW_ORIGIN, R.CROP), R.dyadic_scene(R.NEW_ORIGIN_2, R.CROP_2)
    assert R.scene_classes(s0)['counts'] == [6, 110, 82, 12]
    for sc in (s0, s1):
        ok = R.valid_views(sc['xf'], sc['yf'], sc['d'], sc['hc'], sc['wc'])
        print('0 not 1:', int((ok[0] & ~ok[1]).sum()), 'both:', int((ok[0] & ok[1]).sum()), 'none:', int((~ok.any(0)).sum()), R.scene_classes(sc)['counts'])
    ok = R.valid_views(s0['xf'], s0['yf'], s0['d'], s0['hc'], s0['wc'])
    assert (int((ok[0] & ~ok[1]).sum()), int((ok[0] & ok[1]).sum()), int((~ok.any(0)).sum())) == (131, 73, 6)


@pytest.mark.parametrize('bilinear', [False, True])
def test_reference_identities(bilinear):
    sc, feat = _scene_feat()
    g = (sc['xf'], sc['yf'], sc['d'], sc['hc'], sc['wc'])
    one = RW.weighted_mean_reference(feat, *g, [0, 1, 2], [1, 1, 1], bilinear)
    if bilinear:
        mean, valid, cnt, A = R.bilinear_reference(feat, *g)
        assert np.allclose(one['A'], A, rtol=1e-14, atol=0)
    else:
        mean, valid, cnt = R.nearest_reference(feat, *g)
    assert np.allclose(one['mean'], mean, rtol=1e-14, atol=1e-300) and np.array_equal(one['valid'], valid) and np.array_equal(one['count'], cnt)
    assert np.array_equal(one['W'], cnt.astype(np.float64))
    # chunked ticks with decay 1 are the one-shot mean
    ref = RW.WeightedReference(feat, *g, bilinear)
    ref.tick([0], [1], first=True)
    ref.tick([1], [1])
    chunked = ref.tick([2], [1])
    assert np.allclose(chunked['mean'], one['mean'], rtol=1e-14, atol=1e-300) and np.array_equal(chunked['count'], one['count'])
    # a zero (NaN, negative, inf) weight is the view dropped
    drop = RW.weighted_mean_reference(feat, *g, [0, 2], [1, 1], bilinear)
    for w in (0.0, float('nan'), -1.0, float('inf')):
        z = RW.weighted_mean_reference(feat, *g, [0, 1, 2], [1, w, 1], bilinear)
        for k in ('mean', 'valid', 'count', 'W', 'A'):
            assert np.array_equal(z[k], drop[k]), (w, k)
    assert not np.array_equal(drop['mean'], one['mean'])
    # weights x 4: the mean and the mask unchanged, the sums exactly x 4
    a = RW.weighted_mean_reference(feat, *g, [0, 1, 2], [0.5, 2, 1], bilinear)
    b = RW.weighted_mean_reference(feat, *g, [0, 1, 2], [2, 8, 4], bilinear)
    assert np.array_equal(a['mean'], b['mean']) and np.array_equal(a['valid'], b['valid']) and np.array_equal(4 * a['S'], b['S']) and np.array_equal(4 * a['W'], b['W'])
    assert not np.array_equal(a['mean'], one['mean'])


def test_reference_fading_and_forgetting():
    """lambda = 0.5, forget_below = 0.25, unit weights: tick 0 adds view 0, ticks 1 - 3 add view 1.  The voxels view 0 sees and view 1 does not carry
    W = 1, 0.5, 0.25 and are forgotten at tick 3."""
    sc, feat = _scene_feat()
    g = (sc['xf'], sc['yf'], sc['d'], sc['hc'], sc['wc'])
    ok = R.valid_views(*g)
    only0 = ok[0] & ~ok[1]
    assert only0.sum() > 0
    ref = RW.WeightedReference(feat, *g, False, forget_below=0.25)
    out = ref.tick([0], [1], decay=0.5, first=True)
    for t, w in ((1, 0.5), (2, 0.25), (3, 0.0)):
        out = ref.tick([1], [1], decay=0.5)
        assert np.all(out['W'][only0] == w), t
        assert np.all(out['count'][only0] == (1 if w else 0)) and np.all(out['valid'][only0] == (w > 0))
    assert not out['S'][only0].any()
    both = ok[0] & ok[1]
    assert np.all(out['W'][both] == 0.125 + 0.25 + 0.5 + 1) and np.all(out['count'][both] == 4)
    assert RW.k_weighted(3, 0, True) == 13 and RW.k_weighted(4, 3, False) == 15
