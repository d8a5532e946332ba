"""-m gpu: bf16 storage with DCNv2 stages (nuScenes) and the LayoutHead (SUN RGB-D Total).

The op-level kernels (ivx_dcn_im2col_fwd_bf16, ivx_global_avgpool_fwd_bf16) against their fp32 counterparts, the native handle
against the layer-by-layer composition in bf16 (the same kernels with the same plans: identical bits), bf16 against fp32 at the
reference sizes, and the fp8 trunk staying refused on these configurations."""
import ctypes as C

import numpy as np
import pytest
import torch

import kitti_cfg as kc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ia():
    import imvoxelnet_amd
    from imvoxelnet_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return imvoxelnet_amd


def _offset_mask(B, Ho, Wo, H, W, seed):
    """[B,1,Ho,Wo,28] fp32: offsets of a few pixels, some far outside the map (the zero-corner and h_im > -1 paths), masks with some
    strongly negative logits (mask 0), channel 27 unused (the zero channel of csrc/model.cpp cout_zero)."""
    g = torch.Generator().manual_seed(seed)
    om = torch.zeros(B, 1, Ho, Wo, 28)
    off = torch.randn(B, 1, Ho, Wo, 18, generator=g) * 2.0
    far = torch.rand(B, 1, Ho, Wo, 18, generator=g) < 0.1
    off[far] += torch.randn(int(far.sum()), generator=g).sign() * float(max(H, W))
    om[..., :18] = off
    m = torch.randn(B, 1, Ho, Wo, 9, generator=g) * 2.0
    m[torch.rand(B, 1, Ho, Wo, 9, generator=g) < 0.1] = -200.0
    om[..., 18:27] = m
    return om.cuda()


@pytest.mark.parametrize('stride,Cn', [(1, 256), (2, 256), (1, 512), (2, 512)])
def test_dcn_im2col_bf16_within_one_rounding_of_fp32(ia, stride, Cn):
    """ivx_dcn_im2col_fwd_bf16 = the fp32 columns of the same bf16 map (blend and mask in fp32, same expression), rounded once: within
    2^-8 of each value, and exactly 0 where the fp32 column is 0 (corners outside the map, masks that underflow).  The compiler contracts
    the four-term blend into FMAs and may fuse a different product in each kernel (measured: 1 - 12 of ~10^7 values per shape off the
    pure-rounding bound, all where the blend cancels): the bound carries the fp32 evaluation error of the blend, 2^-20 max |x|."""
    from imvoxelnet_amd import ops
    B, H, W = 2, 23, 37
    x = torch.randn(B, 1, H, W, Cn, generator=torch.Generator().manual_seed(stride * 1000 + Cn)).to(torch.bfloat16).cuda()
    Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    om = _offset_mask(B, Ho, Wo, H, W, seed=Cn + stride)
    got = ops.dcn_im2col(x, om, 3, stride, 1, 1)
    ref = ops.dcn_im2col(x.float(), om, 3, stride, 1, 1)
    assert got.dtype == torch.bfloat16 and got.shape == ref.shape == (B, 1, Ho, Wo, 9 * Cn)
    g = got.float()
    zero = ref == 0
    assert 0.01 < float(zero.float().mean()) < 0.9, 'the offsets / masks must exercise the zero paths'
    assert torch.equal(g[zero], ref[zero])
    d = (g - ref).abs()
    loose = d > ref.abs() * 2.0 ** -8
    print(f'stride {stride} C {Cn}: {int(loose.sum())} of {ref.numel()} beyond pure rounding; |ref| there {ref[loose][:4].tolist()}, |d| {d[loose][:4].tolist()}')
    bad = d > ref.abs() * 2.0 ** -8 + 2.0 ** -20 * float(x.float().abs().max())
    assert not bool(bad.any()), (int(bad.sum()), d[bad][:8].tolist(), ref[bad][:8].tolist())


def test_dcn_im2col_bf16_argument_checks(ia):
    from imvoxelnet_amd import ops
    om = _offset_mask(1, 9, 9, 9, 9, seed=1)
    with pytest.raises(ValueError, match='C % 8'):
        ops.dcn_im2col(torch.zeros(1, 1, 9, 9, 12, dtype=torch.bfloat16, device='cuda'), om)
    flat = torch.zeros(9 * 9 * 16 + 1, dtype=torch.bfloat16, device='cuda')
    x = flat[1:].view(1, 1, 9, 9, 16)                     # contiguous, 2 bytes past a 16-byte boundary
    with pytest.raises(ValueError, match='16-byte aligned'):
        ops.dcn_im2col(x, om)


@pytest.mark.parametrize('shape', [(2, 1, 15, 20, 2048), (3, 1, 7, 5, 100)])
def test_global_avgpool_bf16_bit_identical_to_fp32_pool(ia, shape):
    from imvoxelnet_amd import ops
    c5 = (torch.randn(*shape, generator=torch.Generator().manual_seed(shape[-1])) * 3).to(torch.bfloat16).cuda()
    got = ops.global_avgpool(c5)
    assert got.dtype == torch.float32 and got.shape == (shape[0], 1, 1, 1, shape[-1])
    assert torch.equal(got, ops.global_avgpool(c5.float()))


def _nuscenes_model(ia, n_voxels, seed=33):
    model = ia.build_detector(kc.nuscenes_model_cfg(n_voxels=n_voxels, dcn=True), test_cfg=dict(kc.NUSCENES_TEST_CFG))
    ia.randomize_(model, seed)
    with torch.no_grad():
        g = torch.Generator().manual_seed(5)
        for name, m in model.backbone.named_modules():
            if name.endswith('conv_offset'):                  # non-trivial offsets and masks (test_host_cpu.py, DCN trunk)
                m.weight.normal_(0, 0.02, generator=g)
                m.bias.normal_(0, 0.5, generator=g)
        model.bbox_head.conv_cls.weight.normal_(0, 0.02, generator=g)
        model.bbox_head.conv_cls.bias.fill_(-2.0)
        model.bbox_head.conv_reg.weight.normal_(0, 0.002, generator=g)
    return model


def _small_nuscenes(ia):
    model = _nuscenes_model(ia, (104, 104, 12))
    hw = (224, 416)
    meta = kc.nuscenes_meta(img_hw=hw, box_type=ia.LiDARInstance3DBoxes)
    for e in meta['lidar2img']['extrinsic']:       # the synthetic rig is built for 928 x 1600 images: rescale K to this size
        e[0] *= np.float32(hw[1] / 1600.)
        e[1] *= np.float32(hw[0] / 928.)
    img = torch.randn(1, 6, 3, *hw, generator=torch.Generator().manual_seed(8)).cuda()
    return model, img, [meta]


def _total_model(ia, seed=33):
    mcfg, tcfg = kc.sunrgbd_fast_model_cfg(), dict(kc.SUNRGBD_FAST_TEST_CFG)
    mcfg['head_2d'] = dict(type='LayoutHead', n_channels=2048, linear_size=256, dropout=0.0)
    model = ia.build_detector(mcfg, test_cfg=tcfg)
    ia.randomize_(model, seed)
    with torch.no_grad():
        g = torch.Generator().manual_seed(5)
        model.bbox_head.cls_conv.weight.normal_(0, 0.01, generator=g)
        model.bbox_head.cls_conv.bias.fill_(-2.0)
        model.bbox_head.centerness_conv.weight.normal_(0, 0.005, generator=g)
        model.bbox_head.reg_conv.weight.normal_(0, 0.002, generator=g)
        for i, sc in enumerate(model.bbox_head.scales):
            sc.scale.fill_(1.0 + 0.125 * i)
        model.head_2d.angle_mlp[6].weight.mul_(0.02)          # predicted (pitch, roll) near a pose that sees the volume
        model.head_2d.angle_mlp[6].bias.copy_(torch.tensor([-0.26, 0.43]))
    hw = (480, 640)
    metas = [kc.indoor_meta(1, img_hw=hw, origin=(0, 3, -1), box_type=ia.DepthInstance3DBoxes)]
    img = torch.randn(1, 1, 3, *hw, generator=torch.Generator().manual_seed(9)).cuda()
    return model, img, metas


@pytest.mark.parametrize('cfg_name', ['nuscenes_dcn', 'sunrgbd_total'])
def test_native_bf16_equals_layerwise_dcn_and_layout(ia, cfg_name):
    """bf16 storage inside the native handle with DCNv2 stages (fp32 conv_offset output, bf16 columns, bf16 1x1 over K = 9 C) and with
    the LayoutHead (bf16 C5 pooled to fp32, fp32 MLPs on the bf16 handle): one native call against the layer-by-layer bf16 composition
    -- identical detections, angles and layouts bit for bit."""
    total = cfg_name == 'sunrgbd_total'
    model, img, metas = _total_model(ia) if total else _small_nuscenes(ia)
    model.prepare(torch.device('cuda'), dtype=torch.bfloat16, native=False)
    ref = model.simple_test(img, metas)
    model.prepare(torch.device('cuda'), dtype=torch.bfloat16)
    assert model._native is not None and model._native.cfg.storage == 1
    res = model.simple_test(img, metas)
    assert len(res) == len(ref) == 1 and len(ref[0]['scores_3d']) >= 5
    for a, b in zip(res, ref):
        assert torch.equal(a['scores_3d'], b['scores_3d']) and torch.equal(a['labels_3d'], b['labels_3d'])
        assert torch.equal(a['boxes_3d'].tensor, b['boxes_3d'].tensor)
        if total:
            assert torch.equal(a['angles'], b['angles']) and torch.equal(a['layout'].tensor, b['layout'].tensor)
    print(cfg_name, 'bf16 storage: detections', len(res[0]['scores_3d']))


def _rel(a, b):
    return (a.float() - b.float()).abs().max().item() / a.float().abs().max().item()


def test_nuscenes_bf16_tracks_fp32(ia):
    """bf16 storage against THIS library's fp32 path at the BASELINE nuScenes size (6 views, 928 x 1600, 312 x 312 x 12, batch 1), with
    non-trivial offsets.  Bars relative to each tensor's max, as the KITTI bf16 test: FPN level 0 3e-2, neck 5e-2, head 5e-2; identical
    valid mask (geometry only); the best detections close.  The deformable sampling reads fp32 offsets computed from bf16 operands.
    Measured (MI355X): FPN level 0 0.021, neck 0.019, head 0.024 -- the KITTI bars hold without loosening."""
    model = _nuscenes_model(ia, (312, 312, 12))
    meta = kc.nuscenes_meta(box_type=ia.LiDARInstance3DBoxes)
    img = torch.randn(1, 6, 3, 928, 1600, generator=torch.Generator().manual_seed(11)).cuda()
    outs = {}
    for name, dt in (('f32', torch.float32), ('bf16', torch.bfloat16)):
        model.prepare(torch.device('cuda'), dtype=dt)
        with torch.no_grad():
            p0 = model.features_2d_cl(img)
            vol, valid = model.lift_cl(p0, [meta])
            assert p0.dtype == dt and vol.dtype == dt
            y = model.neck_3d.forward_cl(vol)
            h = model.bbox_head.forward_cl(y)
            assert h.dtype == torch.float32
            det = model.simple_test(img, [meta])
        outs[name] = (p0.float(), valid, y.float(), h, det)
        del p0, vol, y, h
        torch.cuda.empty_cache()
    model.prepare(torch.device('cuda'))
    a, b = outs['f32'], outs['bf16']
    assert torch.equal(a[1], b[1]), 'the valid mask is geometry only'
    for nm, i, tol in (('fpn0', 0, 3e-2), ('neck', 2, 5e-2), ('head', 3, 5e-2)):
        err = _rel(a[i], b[i])
        print(f'nuScenes bf16 vs f32 {nm}: max err / max |x| = {err:.4f}')
        assert err < tol, (nm, err)
    for da, db in zip(a[4], b[4]):
        na, nb = len(da['scores_3d']), len(db['scores_3d'])
        print('detections f32', na, 'bf16', nb)
        assert na > 0 and abs(na - nb) <= max(3, na // 5)
        k = min(10, na, nb)
        ca, cb = da['boxes_3d'].tensor[:k, :3], db['boxes_3d'].tensor[:k, :3]
        d = torch.cdist(ca, cb).min(dim=1).values
        print('top-k centre distance to the nearest bf16 detection', d.tolist())
        assert (d < 0.3).float().mean().item() >= 0.8
        assert abs(float(da['scores_3d'][0]) - float(db['scores_3d'][0])) < 0.05


def test_total_bf16_tracks_fp32(ia):
    """SUN RGB-D Total at its reference size (1 view, 480 x 640, 40 x 40 x 16): the predicted angles within 1e-2 rad of fp32 and the
    layout box within 5e-2 of its largest entry (the valid mask is not compared: the predicted angles move the projection)."""
    model, img, metas = _total_model(ia)
    outs = {}
    for name, dt in (('f32', torch.float32), ('bf16', torch.bfloat16)):
        model.prepare(torch.device('cuda'), dtype=dt)
        r = model.simple_test(img, metas)[0]
        outs[name] = (r['angles'].float(), r['layout'].tensor.float(), len(r['scores_3d']))
    model.prepare(torch.device('cuda'))
    (a32, l32, n32), (a16, l16, n16) = outs['f32'], outs['bf16']
    da = (a32 - a16).abs().max().item()
    dl = _rel(l32, l16)
    print(f'Total bf16 vs f32: angles max |d| = {da:.2e} rad, layout max |d| / max |x| = {dl:.2e}; detections f32 {n32} bf16 {n16}')
    assert da < 1e-2 and dl < 5e-2


@pytest.mark.parametrize('cfg_name', ['nuscenes_dcn', 'sunrgbd_total'])
def test_fp8_trunk_refused_on_dcn_and_layout(ia, cfg_name):
    """calibrate_fp8 stays refused on these configurations: NotImplementedError in Python, IVX_ERR_UNSUPPORTED (-3) from the handle."""
    model, img, _ = _total_model(ia) if cfg_name == 'sunrgbd_total' else _small_nuscenes(ia)
    model.prepare(torch.device('cuda'), dtype=torch.bfloat16)
    nat = model._native
    assert nat is not None and nat.cfg.storage == 1
    with pytest.raises(NotImplementedError):
        model.calibrate_fp8(img)
    x = img.reshape(-1, *img.shape[-3:]).contiguous()
    BV, _, H, W = x.shape
    L = nat.L
    n = L.ivx_backbone_fpn_workspace_bytes(nat.h, BV, H, W)
    assert n > 0
    ws = torch.empty(n, dtype=torch.uint8, device='cuda')
    rc = L.ivx_model_calibrate_fp8_ex(nat.h, C.c_void_p(x.data_ptr()), BV, H, W, C.c_float(1.0), 2, 1, C.c_void_p(ws.data_ptr()), C.c_int64(n), None)
    assert rc == -3, (rc, L.ivx_last_error())
    assert b'DCNv2' in L.ivx_last_error()
