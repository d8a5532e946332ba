"""-m gpu: the bilinear sampling rule of the unprojection (ivx_backproject_fwd_ex, BP_BILINEAR of csrc/backproject.hip) against the fp64
reference of tests/ref_unproject.py within the bound counted from the kernel's roundings (ref_unproject.k_bilinear: K = V + 6), against the
nearest kernel where the two rules coincide, across its modes bit for bit, and through the model: native handle, layer-by-layer path and
streaming sessions.  Every output buffer is pre-filled with NaN / sentinels, so an unwritten voxel fails.  The worst measured ratios are printed."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ref_unproject as R
import kitti_cfg as kc
from imvoxelnet_amd.workloads import _look_at

pytestmark = pytest.mark.gpu

GARBAGE = 0x7f7f7f7f
MEAN, SUM, ACCUM = 0, 1, 2
NEAREST, BILINEAR = 0, 1
F32, BF16 = 0, 1
NV = R.N_VOXELS
N = NV[0] * NV[1] * NV[2]


@pytest.fixture(scope='module')
def ia():
    import imvoxelnet_amd
    from imvoxelnet_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    return imvoxelnet_amd


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _ex(feat, P, no, crop, *, mode=MEAN, sampling=BILINEAR, volume=None, count=None, mean=None, valid=None, first=1, nv=NV, vs=R.VOXEL_SIZE, desc=None,
        feat_ptr=True):
    """One raw ivx_backproject_fwd_ex call on the current stream; returns the status."""
    from imvoxelnet_amd import _lib
    B, V = P.shape[0], P.shape[1]
    _, _, FH, FW, Cn = feat.shape
    d = dict(B=B, V=V, FH=FH, FW=FW, C=Cn, X=nv[0], Y=nv[1], Z=nv[2], feat_dtype=BF16 if feat.dtype == torch.bfloat16 else F32, mode=mode, sampling=sampling,
             first=int(first))
    d.update(desc or {})
    dd = _lib.BackprojectDesc(d['B'], d['V'], d['FH'], d['FW'], d['C'], d['X'], d['Y'], d['Z'], (C.c_float * 3)(*vs), d['feat_dtype'], d['mode'],
                              d['sampling'], d['first'])
    return _lib.lib().ivx_backproject_fwd_ex(C.byref(dd), _p(feat) if feat_ptr else None, _p(P), _p(no), _p(crop), _p(volume), _p(count), _p(mean), _p(valid),
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _bufs(B, Cn, dtype=torch.float32, nv=NV):
    """Output buffers pre-filled with NaN / garbage / sentinels."""
    return dict(vol=torch.full((B,) + nv + (Cn,), float('nan'), device='cuda', dtype=dtype), sum=torch.full((B,) + nv + (Cn,), float('nan'), device='cuda'),
                count=torch.full((B,) + nv, GARBAGE, device='cuda', dtype=torch.int32), valid=torch.full((B,) + nv, 7, device='cuda', dtype=torch.uint8))


def _mean_ex(feat, P, no, crop, sampling=BILINEAR, nv=NV, vs=R.VOXEL_SIZE):
    b = _bufs(P.shape[0], feat.shape[-1], feat.dtype, nv)
    assert _ex(feat, P, no, crop, sampling=sampling, volume=b['vol'], valid=b['valid'], nv=nv, vs=vs) == 0
    assert not bool(torch.isnan(b['vol'].float()).any()) and int(b['valid'].max()) <= 1, 'a voxel was not written'
    return b['vol'], b['valid']


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------ the dyadic scene, two samples
@functools.lru_cache(maxsize=None)
def _scenes():
    s0, s1 = R.dyadic_scene(R.NEW_ORIGIN, R.CROP), R.dyadic_scene(R.NEW_ORIGIN_2, R.CROP_2)
    c0, c1 = R.scene_classes(s0), R.scene_classes(s1)
    # the classes a sampling kernel can get wrong are all there (a changed scene cannot quietly stop covering them)
    assert c0 == dict(valid=[204, 73, 33], behind=[0, 35, 90], band=[12, 17, 8], integer=[0, 18, 0], tie=[0, 31, 10], counts=[6, 110, 82, 12])
    assert min(c0['valid']) > 0 and max(c0['behind']) > 0 and min(c0['band']) > 0 and max(c0['integer']) > 0 and max(c0['tie']) > 0 and min(c0['counts']) > 0
    assert min(c1['valid']) > 0 and max(c1['behind']) > 0 and min(c1['band']) > 0 and max(c1['tie']) > 0
    return s0, s1


@functools.lru_cache(maxsize=None)
def _inputs(Cn, bf16, views=(0, 1, 2)):
    """(feat [2*V,1,FH,FW,C], P [2,V,3,4], new_origin [2,3], crop [2,2]) on the device, and the host copy of the features [2,V,FH,FW,C] (fp32 values;
    bf16-representable when bf16).  Seeded per channel count; a view subset takes the same features."""
    s0, s1 = _scenes()
    g = torch.Generator().manual_seed(1000 + Cn)
    host = torch.randn(2, 3, R.FH, R.FW, Cn, generator=g)
    if bf16:
        host = host.bfloat16().float()
    host = host[:, list(views)].contiguous()
    V = len(views)
    feat = host.reshape(2 * V, 1, R.FH, R.FW, Cn).to(torch.bfloat16 if bf16 else torch.float32).cuda().contiguous()
    P = torch.from_numpy(np.stack([s0['proj'][list(views)], s1['proj'][list(views)]])).cuda().contiguous()
    no = torch.from_numpy(np.stack([s0['new_origin'], s1['new_origin']])).cuda().contiguous()
    crop = torch.from_numpy(np.stack([s0['crop'], s1['crop']])).cuda().contiguous()
    return feat, P, no, crop, host.numpy()


@functools.lru_cache(maxsize=None)
def _reference(Cn, bf16, views=(0, 1, 2)):
    """fp64 reference of both samples: (mean [2,N,C], valid [2,N], count [2,N], A [2,N,C]); computed once per case and shared."""
    host = _inputs(Cn, bf16, views)[4]
    out = []
    for b, sc in enumerate(_scenes()):
        v = list(views)
        out.append(R.bilinear_reference(host[b], sc['xf'][v], sc['yf'][v], sc['d'][v], sc['hc'], sc['wc']))
    return tuple(np.stack([o[i] for o in out]) for i in range(4))


def _check_bound(name, got, ref, A, V, bf16):
    got = got.float().cpu().numpy().astype(np.float64).reshape(ref.shape)
    diff, bnd = np.abs(got - ref), R.bound(A, V, ref, bf16)
    ratio32 = float((diff / (R.U * A + R.TINY)).max())
    worst = float((diff / bnd).max())
    print(f'{name}: worst |got - ref| / bound = {worst:.3f}' + ('' if bf16 else f', |got - ref| / (2^-24 A) = {ratio32:.3f} of K = {R.k_bilinear(V)}'))
    assert np.all(diff <= bnd), (name, worst)
    return ratio32 if not bf16 else worst


CASES = [(8, False), (8, True), (6, False), (64, False), (64, True), (512, False), (512, True)]


@pytest.mark.parametrize('Cn,bf16', CASES, ids=[f'C{c}-{"bf16" if b else "f32"}' for c, b in CASES])
def test_bilinear_mean_within_the_fp64_bound(ia, Cn, bf16):
    """The dyadic scene, B = 2 (another origin and the whole map as crop for the second sample), all three views and each view alone:
    |got - ref| <= K * 2^-24 * A + 2^-126 with K = V + 6 (ref_unproject.k_bilinear counts the roundings: 2 for the weights, 4 through the blend,
    V - 1 view additions, 1 division), A = the fp64 mean over the valid views of sum_i w_i |f_i|; bf16 storage adds the one rounding of the result.
    C = 8: float4 chunks, 2 lanes per voxel, 3 views > lanes; C = 6: the scalar form; C = 512: two chunks per lane.  Mask and count: torch.equal
    with the NEAREST kernel's on the same inputs.  Measured worst ratios: DESIGN.md section 4."""
    from imvoxelnet_amd import ops
    worst = 0.0
    for views in ((0, 1, 2), (0,), (1,), (2,)):
        feat, P, no, crop, _ = _inputs(Cn, bf16, views)
        ref, rvalid, rcount, A = _reference(Cn, bf16, views)
        vol, valid = _mean_ex(feat, P, no, crop)
        assert vol.dtype == feat.dtype
        worst = max(worst, _check_bound(f'C={Cn} {"bf16" if bf16 else "f32"} views {views}', vol, ref, A, len(views), bf16))
        assert np.array_equal(valid.cpu().numpy().reshape(2, N).astype(bool), rvalid)
        assert bool((vol.float().reshape(2, N, Cn)[torch.from_numpy(~rvalid).cuda()] == 0).all())
        near_vol, near_valid = ops.backproject_mean(feat, P, no, crop, R.VOXEL_SIZE, NV)
        assert torch.equal(valid.view(torch.bool), near_valid)
        assert not torch.equal(vol, near_vol), 'the scene must tell the two rules apart'
        if Cn % 4 == 0 and not bf16:
            b = _bufs(2, Cn)
            assert _ex(feat, P, no, crop, mode=SUM, volume=b['sum'], count=b['count']) == 0
            _, near_count = ops.backproject_sum(feat, P, no, crop, R.VOXEL_SIZE, NV)
            assert torch.equal(b['count'], near_count) and np.array_equal(b['count'].cpu().numpy().reshape(2, N), rcount)
    print(f'C={Cn} {"bf16" if bf16 else "f32"}: worst ratio over the view sets {worst:.3f}')


# ------------------------------------------------------------------ where the two rules coincide
def _integer_camera(bf16, V):
    """Fronto-parallel cameras with constant depth 1 whose u / d, v / d are integers for every voxel: u = i + c, v = j + c' on the 0.25 grid
    (rows 4 * x + ..., 4 * y + ..., d = 1); part of the grid falls outside the 5 x 8 crop."""
    no = np.array([[0.5, 0.25, 0.0]], np.float32)
    rows = [[[4, 0, 0, -3], [0, 4, 0, -1], [0, 0, 0, 1]], [[4, 0, 0, -1], [0, 4, 0, -2], [0, 0, 0, 1]]][2 - V:]  # u = i - 1, v = j; u = i + 1, v = j - 1 (alone when V = 1)
    P = torch.tensor([rows], dtype=torch.float32).cuda().contiguous()
    feat = torch.randn(V, 1, R.FH, R.FW, 8, generator=torch.Generator().manual_seed(77)).to(torch.bfloat16 if bf16 else torch.float32).cuda()
    crop = torch.tensor([[5, 8]], dtype=torch.int32).cuda()
    xf, yf, d = R.project(P[0].cpu().numpy(), R.points(NV, R.VOXEL_SIZE, no[0]))
    assert np.array_equal(xf, np.rint(xf)) and np.array_equal(yf, np.rint(yf)) and np.all(d == 1)
    ok = R.valid_views(xf, yf, d, 5, 8)
    assert 0 < ok.sum() < ok.size and (xf[ok] == 7).any() and (yf[ok] == 4).any()          # invalid samples too, and hits on the last row / column
    return feat, P, torch.from_numpy(no).cuda(), crop


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('V', [2, 1])
def test_bilinear_equals_nearest_at_integer_projections(ia, bf16, V):
    """ax = ay = 0 everywhere: the sample is the nearest pixel's value, so the volume equals the nearest kernel's (torch.equal) and so does the mask."""
    from imvoxelnet_amd import ops
    feat, P, no, crop = _integer_camera(bf16, V)
    vol, valid = _mean_ex(feat, P, no, crop)
    near_vol, near_valid = ops.backproject_mean(feat, P, no, crop, R.VOXEL_SIZE, NV)
    assert torch.equal(vol, near_vol) and torch.equal(valid.view(torch.bool), near_valid) and 0 < int(near_valid.sum()) < near_valid.numel()


# ------------------------------------------------------------------ sampling = 0 is the old entry points
def test_ex_with_nearest_sampling_equals_every_legacy_entry(ia):
    """ivx_backproject_fwd_ex with sampling = IVX_SAMPLE_NEAREST: the bits of ivx_backproject_mean_fwd (float4 and scalar form, three views and one),
    _mean_fwd_bf16, _sum_fwd, _accum_fwd and _accum_fwd_bf16."""
    from imvoxelnet_amd import ops
    for Cn, views in ((8, (0, 1, 2)), (8, (1,)), (6, (0, 1, 2)), (6, (0,))):
        feat, P, no, crop, _ = _inputs(Cn, False, views)
        vol, valid = _mean_ex(feat, P, no, crop, sampling=NEAREST)
        ref, rvalid = ops.backproject_mean(feat, P, no, crop, R.VOXEL_SIZE, NV)
        assert _same_bits(vol, ref) and torch.equal(valid.view(torch.bool), rvalid), (Cn, views)
    feat, P, no, crop, _ = _inputs(8, True)
    vol, valid = _mean_ex(feat, P, no, crop, sampling=NEAREST)
    ref, rvalid = ops.backproject_mean(feat, P, no, crop, R.VOXEL_SIZE, NV)
    assert _same_bits(vol, ref) and torch.equal(valid.view(torch.bool), rvalid)
    feat, P, no, crop, _ = _inputs(8, False)
    b = _bufs(2, 8)
    assert _ex(feat, P, no, crop, mode=SUM, sampling=NEAREST, volume=b['sum'], count=b['count']) == 0
    rs, rc = ops.backproject_sum(feat, P, no, crop, R.VOXEL_SIZE, NV)
    assert _same_bits(b['sum'], rs) and torch.equal(b['count'], rc)
    for bf16 in (False, True):
        feat, P, no, crop, _ = _inputs(8, bf16)
        dt = feat.dtype
        b, r = _bufs(2, 8, dt), _bufs(2, 8, dt)
        f = feat.view(2, 3, *feat.shape[1:])
        for i, (v0, v1) in enumerate(((0, 1), (1, 3))):
            fc, Pc = f[:, v0:v1].reshape(-1, *feat.shape[1:]).contiguous(), P[:, v0:v1].contiguous()
            assert _ex(fc, Pc, no, crop, mode=ACCUM, sampling=NEAREST, volume=b['sum'], count=b['count'], mean=b['vol'], valid=b['valid'], first=i == 0) == 0
            ops.backproject_accum_(fc, Pc, no, crop, R.VOXEL_SIZE, r['sum'], r['count'], i == 0, r['vol'], r['valid'])
        assert _same_bits(b['sum'], r['sum']) and torch.equal(b['count'], r['count']) and _same_bits(b['vol'], r['vol']) and torch.equal(b['valid'], r['valid'])
        assert not bool(torch.isnan(b['vol'].float()).any())


# ------------------------------------------------------------------ the modes agree
@pytest.mark.parametrize('Cn,bf16', [(8, False), (8, True), (512, False), (64, True)], ids=['C8-f32', 'C8-bf16', 'C512-f32', 'C64-bf16'])
def test_bilinear_modes_agree_bit_for_bit(ia, Cn, bf16):
    """Bilinear rule: sum + ivx_volume_normalize_fwd == mean; accumulate in chunks 1+2, 2+1, 1+1+1 (first = 1 over a NaN / garbage state) == mean;
    accumulate with mean_out = NULL + ivx_volume_mean_fwd == mean; all under torch.equal, mask and count included."""
    from imvoxelnet_amd import ops
    feat, P, no, crop, _ = _inputs(Cn, bf16)
    dt = feat.dtype
    vol, valid = _mean_ex(feat, P, no, crop)
    s = _bufs(2, Cn)
    assert _ex(feat, P, no, crop, mode=SUM, volume=s['sum'], count=s['count']) == 0
    count = s['count'].clone()
    assert int(count.max()) == 3 and int(count.min()) == 0
    m2, v2 = ops.volume_mean(s['sum'], s['count'], dt)
    assert torch.equal(m2, vol) and torch.equal(v2, valid.view(torch.bool))
    norm, v3 = ops.volume_normalize_(s['sum'].clone(), s['count'])
    assert torch.equal(norm.to(dt), vol) and torch.equal(v3, valid.view(torch.bool))
    f = feat.view(2, 3, *feat.shape[1:])
    for chunks in ((1, 2), (2, 1), (1, 1, 1)):
        for emit in (True, False):
            b = _bufs(2, Cn, dt)
            v0 = 0
            for n in chunks:
                fc, Pc = f[:, v0:v0 + n].reshape(-1, *feat.shape[1:]).contiguous(), P[:, v0:v0 + n].contiguous()
                assert _ex(fc, Pc, no, crop, mode=ACCUM, volume=b['sum'], count=b['count'], mean=b['vol'] if emit else None,
                           valid=b['valid'] if emit else None, first=v0 == 0) == 0
                v0 += n
            assert torch.equal(b['sum'], s['sum']) and torch.equal(b['count'], count), (chunks, emit)
            if emit:
                assert torch.equal(b['vol'], vol) and torch.equal(b['valid'], valid), chunks
            else:
                assert bool(torch.isnan(b['vol'].float()).all()) and bool((b['valid'] == 7).all())          # not passed: not written
                m, v = ops.volume_mean(b['sum'], b['count'], dt)
                assert torch.equal(m, vol) and torch.equal(v, valid.view(torch.bool)), chunks
    # the ops wrappers take the same route
    ov, ovalid = ops.backproject_mean(feat, P, no, crop, R.VOXEL_SIZE, NV, sampling='bilinear')
    assert torch.equal(ov, vol) and torch.equal(ovalid, valid.view(torch.bool))
    if not bf16:
        os_, oc = ops.backproject_sum(feat, P, no, crop, R.VOXEL_SIZE, NV, sampling='bilinear')
        assert torch.equal(os_, s['sum']) and torch.equal(oc, count)


# ------------------------------------------------------------------ argument errors
def test_ex_argument_errors_leave_the_outputs_untouched(ia):
    from imvoxelnet_amd import _lib
    L = _lib.lib()
    feat, P, no, crop, _ = _inputs(8, False)
    feat6 = _inputs(6, False)[0]
    b = _bufs(2, 8)
    mean_kw = dict(volume=b['vol'], valid=b['valid'])
    sum_kw = dict(mode=SUM, volume=b['sum'], count=b['count'])
    acc_kw = dict(mode=ACCUM, volume=b['sum'], count=b['count'], mean=b['vol'], valid=b['valid'])
    bad = [('sampling', dict(desc=dict(sampling=2), **mean_kw)), ('sampling', dict(desc=dict(sampling=-1), **mean_kw)), ('mode', dict(desc=dict(mode=3), **mean_kw)),
           ('feat_dtype', dict(desc=dict(feat_dtype=2), **mean_kw))]
    for s in (NEAREST, BILINEAR):
        bad += [('null', dict(sampling=s, feat_ptr=False, **mean_kw)), ('null', dict(sampling=s, volume=b['vol'])), ('null', dict(sampling=s, valid=b['valid'])),
                ('null', dict(sampling=s, mode=SUM, volume=b['sum'])), ('null', dict(sampling=s, mode=ACCUM, volume=b['sum'], mean=b['vol'], valid=b['valid'])),
                ('both', dict(sampling=s, mode=ACCUM, volume=b['sum'], count=b['count'], mean=b['vol'])),
                ('mean mode', dict(sampling=s, count=b['count'], **mean_kw)), ('sum mode', dict(sampling=s, valid=b['valid'], **sum_kw)),
                ('non-positive', dict(sampling=s, desc=dict(V=0), **mean_kw)), ('non-positive', dict(sampling=s, desc=dict(Z=0), **sum_kw)),
                ('non-positive', dict(sampling=s, desc=dict(FH=-1), **acc_kw)), ('too large', dict(sampling=s, desc=dict(X=2048, Y=2048, Z=512), **mean_kw)),
                ('too large', dict(sampling=s, desc=dict(C=1028), **mean_kw))]
    for what, kw in bad:
        assert L.ivx_volume_mean_fwd(_p(b['sum']), _p(b['count']), 0, 8, _p(b['vol']), 0, _p(b['valid']), None) == -1        # leaves another message behind
        assert _ex(feat, P, no, crop, **kw) == -1, (what, kw.get('sampling'))
        assert what.encode() in L.ivx_last_error(), (what, L.ivx_last_error())
    for s in (NEAREST, BILINEAR):                           # C % 4 != 0 outside the fp32 mean
        for kw in (sum_kw, acc_kw):
            assert _ex(feat6, P, no, crop, sampling=s, **dict(kw, volume=b['sum'][..., :6])) == -1 and b'C % 4' in L.ivx_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(b['vol']).all()) and bool(torch.isnan(b['sum']).all()) and bool((b['count'] == GARBAGE).all()) and bool((b['valid'] == 7).all())
    with pytest.raises(ValueError, match='sampling'):
        _lib.check(_ex(feat, P, no, crop, desc=dict(sampling=2), **mean_kw), 'ivx_backproject_fwd_ex')


# ------------------------------------------------------------------ through the model
def _anchor_small(ia, hw=(96, 160)):
    """KITTI family (stack neck + Anchor3DHead) at the size of the smoke run: one view."""
    nv = (24, 28, 12)
    cfg = kc.kitti_model_cfg(n_voxels=nv, in_ch=16, out_ch=32)
    ox = 0.5 + nv[0] * .32 / 2
    cfg['bbox_head']['anchor_generator']['ranges'] = [[ox - nv[0] * .16, -nv[1] * .16, -1.78, ox + nv[0] * .16 - .32, nv[1] * .16 - .32, -1.78]]
    model = ia.build_detector(cfg, test_cfg=dict(kc.KITTI_TEST_CFG, score_thr=0.05))
    ia.randomize_(model, 7)
    with torch.no_grad():
        model.bbox_head.conv_cls.weight.normal_(0, 0.05, generator=torch.Generator().manual_seed(1))
        model.bbox_head.conv_cls.bias.fill_(-1.5)
    K = np.array([[36., 0, 40, 0], [0, 36., 22, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
    E = [np.array([[0, -1, 0, 0.0], [0, 0, -1, 0.2], [1, 0, 0, 0.1], [0, 0, 0, 1]], np.float32)]
    scene_meta = dict(img_shape=(hw[0], hw[1], 3), ori_shape=(hw[0] // 2, hw[1] // 2, 3), box_type_3d=ia.LiDARInstance3DBoxes,
                      lidar2img=dict(intrinsic=K, origin=np.array([ox, 0, -1.0], np.float32)))
    img = torch.randn(1, 3, *hw, generator=torch.Generator().manual_seed(2)).cuda()
    return model, scene_meta, E, img


def _indoor_small(ia, V=4, hw=(96, 128)):
    """ScanNet-fast family with a 24 x 24 x 8 grid, V cameras on a circle inside it, looking at its centre."""
    mcfg = kc.scannet_fast_model_cfg()
    mcfg['n_voxels'] = (24, 24, 8)
    model = ia.build_detector(mcfg, test_cfg=dict(kc.SCANNET_FAST_TEST_CFG))
    ia.randomize_(model, 33)
    with torch.no_grad():
        g = torch.Generator().manual_seed(5)
        model.bbox_head.cls_conv.weight.normal_(0, 0.01, generator=g)
        model.bbox_head.cls_conv.bias.fill_(-2.0)
        model.bbox_head.centerness_conv.weight.normal_(0, 0.005, generator=g)
        model.bbox_head.reg_conv.weight.normal_(0, 0.002, generator=g)       # keeps exp(reg) finite
    K = np.array([[200., 0, 63.5, 0], [0, 200., 47.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)       # narrow: part of the grid stays unseen
    E = [_look_at((1.8 * np.cos(2 * np.pi * i / V + 0.3), 1.8 * np.sin(2 * np.pi * i / V + 0.3), 1.2), (0, 0, .5)) for i in range(V)]
    scene_meta = dict(img_shape=(hw[0], hw[1], 3), ori_shape=(hw[0], hw[1], 3), pad_shape=(hw[0], hw[1], 3), box_type_3d=ia.DepthInstance3DBoxes,
                      lidar2img=dict(intrinsic=K, origin=np.array([0, 0, .5], np.float32)))
    img = torch.randn(V, 3, *hw, generator=torch.Generator().manual_seed(9)).cuda()
    return model, scene_meta, E, img


def _model_reference(model, p0, meta):
    """fp64 bilinear reference of the model's lift, fed the model's own FPN level-0 output and the host-side camera set-up."""
    proj, no, crop = (t.numpy() for t in model._camera_setup([meta], 4, 'cpu'))
    feat = p0.float().cpu().numpy()[:, 0]
    xf, yf, d = R.project(proj[0], R.points(model.n_voxels, model.voxel_size, no[0]))
    hc, wc = min(int(crop[0, 0]), feat.shape[1]), min(int(crop[0, 1]), feat.shape[2])
    return R.bilinear_reference(feat, xf, yf, d, hc, wc)


@pytest.mark.parametrize('family', ['anchor', 'indoor'])
def test_model_with_bilinear_sampling(ia, family):
    """prepare(sampling='bilinear'): the native handle and the layer-by-layer path give the same detections, neck levels and mask bit for bit (the
    handle does not expose its volume; everything computed from it is compared), the volume meets the fp64 bound on the model's own FPN output
    and differs from the nearest volume, a streaming session reproduces the one-shot lift, and sampling='nearest' gives the result of a model
    prepared without the option."""
    from imvoxelnet_amd import ops
    model, scene_meta, E, img = (_anchor_small if family == 'anchor' else _indoor_small)(ia)
    meta = dict(scene_meta, lidar2img=dict(scene_meta['lidar2img'], extrinsic=list(E)))
    V, hw = len(E), tuple(img.shape[-2:])
    model.prepare(torch.device('cuda'), sampling='bilinear')
    assert model._native is not None and model._native.cfg.sampling == 1 and model.sampling == 'bilinear'
    p0 = model.features_2d_cl(img[None])
    vol, valid = model.lift_cl(p0, [meta])
    proj, no, crop = model._camera_setup([meta], 4, img.device)
    x = img.contiguous()
    if family == 'anchor':
        ref = model.detect_cl(vol, [meta])
        out = model._native.forward(x, 1, V, hw[0], hw[1], proj, no, crop, want_valid=True)
        for a, b in zip(out[:4], ref):
            assert torch.equal(a, b)
        assert torch.equal(out[4], valid) and int(ref[3].sum()) > 0
        res = model.simple_test(img[None], [meta])
        n = int(ref[3][0])
        assert torch.equal(res[0]['scores_3d'], ref[1][0, :n].cpu()) and torch.equal(res[0]['boxes_3d'].tensor, ref[0][0, :n].cpu())
    else:
        levels, ok = model._native.forward_levels(x, 1, V, hw[0], hw[1], proj, no, crop)
        assert torch.equal(ok, valid)
        for a, b in zip(levels, model.neck_3d.forward_cl(vol)):
            assert torch.equal(a, b)
        ref = model.detect_indoor_cl(vol, valid, [meta])
        res = model.simple_test(img[None], [meta])
        assert len(res[0]['scores_3d']) > 0
        for (rb, rs, rl), r in zip(ref, res):
            assert torch.equal(r['scores_3d'], rs.cpu()) and torch.equal(r['labels_3d'], rl.cpu()) and torch.equal(r['boxes_3d'].tensor, rb.tensor.cpu())
    # the fp64 bound on the model's own features
    rmean, rvalid, rcount, A = _model_reference(model, p0, meta)
    Cn = p0.shape[-1]
    assert np.array_equal(valid.cpu().numpy().reshape(-1), rvalid) and 0 < rvalid.sum() < rvalid.size
    _check_bound(f'{family} model volume (V = {V}, C = {Cn})', vol[0].reshape(-1, Cn), rmean, A, V, False)
    assert torch.equal(ops.backproject_mean(p0, proj, no, crop, model.voxel_size, model.n_voxels, sampling='bilinear')[0], vol)
    # a streaming session on this model: all views at once, and chunk by chunk against the one-shot lift of the features it was given
    scene = model.open_scene(scene_meta)
    scene.add_views(img, E)
    v, ok = scene.volume()
    assert torch.equal(v, vol) and torch.equal(ok, valid)
    scene.reset()
    per_chunk = []
    for v0 in range(V):
        scene.add_views(img[v0:v0 + 1], E[v0:v0 + 1], emit=v0 % 2 == 0)
        per_chunk.append(scene._features(img[v0:v0 + 1].contiguous()).clone())
    one_shot = ops.backproject_mean(torch.cat(per_chunk).contiguous(), proj, no, crop, model.voxel_size, model.n_voxels, sampling='bilinear')
    v, ok = scene.volume()
    assert scene.n_views == V and torch.equal(v, one_shot[0]) and torch.equal(ok, one_shot[1]) and torch.equal(ok, valid)
    scene.close()
    # the nearest rule, chosen explicitly, is the model of before
    near_default = ops.backproject_mean(p0, proj, no, crop, model.voxel_size, model.n_voxels)
    model.prepare(torch.device('cuda'), sampling='nearest')
    assert model._native is not None and model._native.cfg.sampling == 0
    nvol, nvalid = model.lift_cl(p0, [meta])
    assert _same_bits(nvol, near_default[0]) and torch.equal(nvalid, near_default[1]) and torch.equal(nvalid, valid)
    assert not torch.equal(nvol, vol), 'the bilinear volume must differ from the nearest volume somewhere'
    res_near = model.simple_test(img[None], [meta])
    model.prepare(torch.device('cuda'))
    res_plain = model.simple_test(img[None], [meta])
    assert torch.equal(res_near[0]['scores_3d'], res_plain[0]['scores_3d']) and torch.equal(res_near[0]['boxes_3d'].tensor, res_plain[0]['boxes_3d'].tensor)
