"""-m gpu: the model-level C-ABI (csrc/model.cpp: ivx_create / ivx_weights_load / ivx_model_forward ...).

The native handle and the layer-by-layer Python composition run the same kernels with the same plans, so their results
must be BIT-identical; the handle is also driven by a C program with no Python in the process (tests/c/e2e_small.c) on
the reference's end-to-end golden case."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kitti_cfg as kc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def ia():
    import imvoxelnet_amd
    from imvoxelnet_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return imvoxelnet_amd


def _kitti_model(ia, n_voxels, seed=21):
    model = ia.build_detector(kc.kitti_model_cfg(n_voxels=n_voxels), test_cfg=kc.KITTI_TEST_CFG)
    ia.randomize_(model, seed)
    with torch.no_grad():
        model.bbox_head.conv_cls.weight.normal_(0, 0.03, generator=torch.Generator().manual_seed(5))
        model.bbox_head.conv_cls.bias.fill_(-1.5)
        model.bbox_head.conv_reg.weight.normal_(0, 0.002, generator=torch.Generator().manual_seed(6))
        model.bbox_head.conv_dir_cls.weight.normal_(0, 0.02, generator=torch.Generator().manual_seed(7))
    return model


def _assert_same_detections(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x, y), f'{(x != y).sum().item()} values differ'


@pytest.mark.parametrize('shape', ['small', 'full'])
def test_native_model_equals_layerwise_kitti(ia, shape):
    """ivx_model_forward == features_2d_cl -> lift_cl -> detect_cl, bit for bit (boxes, scores, labels, counts, valid mask),
    and the sub-path entry points ivx_backbone_fpn_fwd / ivx_neck3d_kitti_fwd == backbone+FPN / neck_3d.forward_cl."""
    if shape == 'small':
        nv, hw, B = (104, 120, 12), (192, 640), 2
    else:
        nv, hw, B = (216, 248, 12), (384, 1280), 4      # BASELINE config 2 as benchmarked
    model = _kitti_model(ia, nv)
    model.prepare(torch.device('cuda'))
    assert model._native is not None, 'the KITTI configuration must run on the native model handle'
    img = torch.randn(B, 1, 3, *hw, generator=torch.Generator().manual_seed(3)).cuda()
    metas = [kc.kitti_meta(img_hw=hw, t=(0.02 * b, 0.01 * b, 0.0), box_type=ia.LiDARInstance3DBoxes) for b in range(B)]
    # layer by layer over the op-level C-ABI
    p0 = model.features_2d_cl(img)
    vol, valid = model.lift_cl(p0, metas)
    y = model.neck_3d.forward_cl(vol)
    ref = model.detect_cl(vol, metas)
    # one native call
    proj, new_origin, crop = model._camera_setup(metas, 4, img.device)
    out = model._native.forward(img.reshape(B, 3, *hw).contiguous(), B, 1, hw[0], hw[1], proj, new_origin, crop, want_valid=True)
    _assert_same_detections(out[:4], ref)
    assert torch.equal(out[4], valid)
    assert int(ref[3].sum()) > 0
    # sub-paths
    assert torch.equal(model._native.backbone_fpn(img.reshape(B, 3, *hw).contiguous()), p0)
    assert torch.equal(model._native.neck3d(vol), y)
    # and the public call goes through the handle
    res = model.simple_test(img, metas)
    for b in range(B):
        n = int(ref[3][b])
        assert len(res[b]['scores_3d']) == n
        assert torch.equal(res[b]['scores_3d'], ref[1][b, :n].cpu()) and torch.equal(res[b]['boxes_3d'].tensor, ref[0][b, :n].cpu())
        assert torch.equal(res[b]['labels_3d'], ref[2][b, :n].cpu())


def test_native_model_nuscenes_plain_resnet(ia):
    """NuScenesImVoxelNeck family (6 views, dir_offset pi/4, nms_pre 1000) on the handle with the plain ResNet-50 (the reference's
    DCNv2 backbone on the handle: test_native_detect_equals_layerwise[nuscenes_dcn])."""
    from imvoxelnet_amd import engine
    cfg = kc.nuscenes_model_cfg(n_voxels=(104, 104, 12), dcn=False)
    model = ia.build_detector(cfg, test_cfg=kc.NUSCENES_TEST_CFG)
    ia.randomize_(model, 4)
    with torch.no_grad():
        model.bbox_head.conv_cls.weight.normal_(0, 0.03, generator=torch.Generator().manual_seed(5))
        model.bbox_head.conv_cls.bias.fill_(-1.5)
        model.bbox_head.conv_reg.weight.normal_(0, 0.002, generator=torch.Generator().manual_seed(6))
    model.prepare(torch.device('cuda'))
    assert model._native is not None
    hw = (224, 416)
    meta = kc.nuscenes_meta(img_hw=hw, box_type=ia.LiDARInstance3DBoxes)
    for e in meta['lidar2img']['extrinsic']:       # the synthetic rig is built for 928 x 1600 images: rescale K to this size
        e[0] *= np.float32(hw[1] / 1600.)
        e[1] *= np.float32(hw[0] / 928.)
    img = torch.randn(1, 6, 3, *hw, generator=torch.Generator().manual_seed(8)).cuda()
    p0 = model.features_2d_cl(img)
    vol, valid = model.lift_cl(p0, [meta])
    ref = model.detect_cl(vol, [meta])
    proj, new_origin, crop = model._camera_setup([meta], 4, img.device)
    out = model._native.forward(img.reshape(6, 3, *hw).contiguous(), 1, 6, hw[0], hw[1], proj, new_origin, crop, want_valid=True)
    _assert_same_detections(out[:4], ref)
    assert torch.equal(out[4], valid) and 0.05 < float(valid.float().mean()) < 1.0
    dcn_model = ia.build_detector(kc.nuscenes_model_cfg(n_voxels=(104, 104, 12)), test_cfg=kc.NUSCENES_TEST_CFG)
    assert engine.family(dcn_model) == 'anchor' and list(engine.model_cfg(dcn_model).dcn_stages) == [0, 0, 1, 1]   # round 3: DCNv2 stages inside the handle


def test_native_model_trace_and_errors(ia):
    """ivx_model_trace: one record per launch group with plausible durations; bad arguments fail loudly."""
    import ctypes as C
    from imvoxelnet_amd import _lib
    model = _kitti_model(ia, (104, 120, 12))
    model.prepare(torch.device('cuda'))
    nat = model._native
    hw, B = (192, 640), 2
    img = torch.randn(B, 1, 3, *hw, generator=torch.Generator().manual_seed(3)).cuda()
    metas = [kc.kitti_meta(img_hw=hw, box_type=ia.LiDARInstance3DBoxes) for _ in range(B)]
    model.simple_test(img, metas)
    nat.trace(True)
    model.simple_test(img, metas)
    torch.cuda.synchronize()
    recs = nat.trace_records()
    nat.trace(False)
    stages = [r['stage'] for r in recs]
    assert stages.count(4) == 1 and stages.count(5) == 1 and stages.count(2) >= 9, stages
    assert stages.count(1) == stages.count(2) == stages.count(3)
    assert all(r['ms'] > 0 for r in recs) and all(b['start_ms'] >= a['start_ms'] for a, b in zip(recs, recs[1:]))
    neck_gemm = [r for r in recs if r['stage'] == 2 and r['is3d']]
    assert len(neck_gemm) == 9 and all(r['flops'] > 0 for r in neck_gemm)
    # coarse level: the trunk is one span whose FLOPs are the sum of its layers', the neck stages stay individual
    full_2d = sum(r['flops'] for r in recs if not r['is3d'] and r['step'] < min(q['step'] for q in recs if q['stage'] == 4))
    nat.trace(1)
    model.simple_test(img, metas)
    torch.cuda.synchronize()
    coarse = nat.trace_records()
    nat.trace(0)
    span = [r for r in coarse if r['stage'] == 6]
    assert len(span) == 1 and span[0]['ms'] > 0 and abs(span[0]['flops'] - full_2d) <= 1e-6 * full_2d
    assert len([r for r in coarse if r['stage'] == 2 and r['is3d']]) == 9 and len(coarse) < len(recs) // 2
    # errors: unpadded image size, too small a workspace, a handle without the trunk asked for the trunk
    L = _lib.lib()
    assert L.ivx_model_workspace_bytes(nat.h, 1, 1, 100, 640) == -1
    proj, new_origin, crop = model._camera_setup(metas, 4, img.device)
    x = img.reshape(B, 3, *hw).contiguous()
    small = torch.empty(4096, device='cuda', dtype=torch.uint8)
    rc = L.ivx_model_forward(nat.h, C.c_void_p(x.data_ptr()), B, 1, hw[0], hw[1], C.c_void_p(proj.data_ptr()), C.c_void_p(new_origin.data_ptr()),
                             C.c_void_p(crop.data_ptr()), C.c_void_p(small.data_ptr()), small.numel(), None, None, None, None, None, None)
    assert rc == -4 and b'workspace too small' in L.ivx_last_error()
    from imvoxelnet_amd.engine import NativeModel
    headless = NativeModel(model, torch.device('cuda'), with_trunk=False)
    assert L.ivx_backbone_fpn_workspace_bytes(headless.h, 2, 192, 640) == -1
    p0 = model.features_2d_cl(img)
    out = headless.forward(p0, B, 1, hw[0], hw[1], proj, new_origin, crop)
    ref = nat.forward(x, B, 1, hw[0], hw[1], proj, new_origin, crop)
    _assert_same_detections(out, ref)


def test_c_program_e2e_small_without_python(ia):
    """tests/c/e2e_small.c: a C host (no Python in the process) drives ivx_create / ivx_weights_load / ivx_model_forward on
    the reference's end-to-end golden case and checks detections and valid mask against the reference's outputs."""
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'c'))
    import build as cbuild
    exe = cbuild.build('e2e_small')
    fx = os.path.join(ROOT, 'tests', 'golden', 'e2e_small.bin')
    out = subprocess.run([exe, fx], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'C e2e_small OK' in out.stdout


def test_c_program_e2e_indoor_without_python(ia):
    """tests/c/e2e_indoor.c: a C host (no Python in the process) drives ivx_create / ivx_weights_load / ivx_model_detect on the
    reference's end-to-end INDOOR golden cases (ScanNet head + aligned NMS, SUN RGB-D head + rotated multi-class NMS; camera set-up
    inside the library) and checks detections and valid masks against the reference's outputs."""
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'c'))
    import build as cbuild
    exe = cbuild.build('e2e_indoor')
    fx = os.path.join(ROOT, 'tests', 'golden', 'e2e_indoor.bin')
    out = subprocess.run([exe, fx], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'C e2e_indoor OK' in out.stdout


# ('scannet_fast', 12): 12 x 120 x 160 positions >= 200 000 -- the 256-channel FPN output conv takes its Winograd form in BOTH hosts (wants_pair /
# FusedConv.prefers_winograd); at 5 views it is a link of the pair chain
@pytest.mark.parametrize('cfg_name,views', [('scannet_fast', 5), ('scannet_fast', 12), ('sunrgbd_fast', 1), ('scannet_v1', 4), ('sunrgbd_total', 1), ('nuscenes_dcn', 6)])
def test_native_detect_equals_layerwise(ia, cfg_name, views):
    """The WHOLE of simple_test inside the native handle (round 3): the anchor-free heads + per-level candidates + cross-level NMS
    (ScanNet fast / SUN RGB-D fast / ScanNet v1), the LayoutHead with its predicted angles feeding the unprojection (SUN RGB-D Total),
    and the DCNv2 trunk stages (the reference nuScenes backbone) -- one C-ABI call (ivx_model_detect / ivx_model_forward) against the
    layer-by-layer Python composition over the op-level ABI: identical detections bit for bit."""
    total = cfg_name == 'sunrgbd_total'
    if cfg_name == 'nuscenes_dcn':
        mcfg, tcfg = kc.nuscenes_model_cfg(dcn=True), dict(kc.NUSCENES_TEST_CFG)
        hw, metas = (928, 1600), [kc.nuscenes_meta(box_type=ia.LiDARInstance3DBoxes)]
    else:
        base = 'sunrgbd_fast' if total else cfg_name
        mcfg, tcfg = getattr(kc, f'{base}_model_cfg')(), dict(getattr(kc, f'{base.upper()}_TEST_CFG'))
        if total:
            mcfg['head_2d'] = dict(type='LayoutHead', n_channels=2048, linear_size=256, dropout=0.0)
        hw = (480, 640)
        metas = [kc.indoor_meta(views, img_hw=hw, origin=(0, 3, -1) if base == 'sunrgbd_fast' else (0, 0, .5), box_type=ia.DepthInstance3DBoxes)]
    model = ia.build_detector(mcfg, test_cfg=tcfg)
    ia.randomize_(model, 33)
    with torch.no_grad():
        g = torch.Generator().manual_seed(5)
        if cfg_name == 'nuscenes_dcn':
            for name, m in model.backbone.named_modules():
                if name.endswith('conv_offset'):
                    m.weight.normal_(0, 0.02, generator=g)
                    m.bias.normal_(0, 0.5, generator=g)
            model.bbox_head.conv_cls.weight.normal_(0, 0.02, generator=g)
            model.bbox_head.conv_cls.bias.fill_(-2.0)
            model.bbox_head.conv_reg.weight.normal_(0, 0.002, generator=g)
        else:
            model.bbox_head.cls_conv.weight.normal_(0, 0.01, generator=g)
            model.bbox_head.cls_conv.bias.fill_(-2.0)
            model.bbox_head.centerness_conv.weight.normal_(0, 0.005, generator=g)
            model.bbox_head.reg_conv.weight.normal_(0, 0.002, generator=g)
            for i, sc in enumerate(model.bbox_head.scales):
                sc.scale.fill_(1.0 + 0.125 * i)
            if total:                                       # predicted (pitch, roll) near a pose that sees the volume
                model.head_2d.angle_mlp[6].weight.mul_(0.02)
                model.head_2d.angle_mlp[6].bias.copy_(torch.tensor([-0.26, 0.43]))
    img = torch.randn(1, views, 3, *hw, generator=torch.Generator().manual_seed(9)).cuda()
    model.prepare(torch.device('cuda'), native=False)
    ref = model.simple_test(img, metas)                       # layer by layer over the op-level ABI
    model.prepare(torch.device('cuda'))
    assert model._native is not None and model._native.family == ('anchor' if cfg_name == 'nuscenes_dcn' else 'indoor')
    res = model.simple_test(img, metas)                       # one native call
    assert len(res) == len(ref) == 1 and len(ref[0]['scores_3d']) > 5
    for a, b in zip(res, ref):
        assert torch.equal(a['scores_3d'], b['scores_3d']) and torch.equal(a['labels_3d'], b['labels_3d'])
        assert torch.equal(a['boxes_3d'].tensor, b['boxes_3d'].tensor)
        assert a['boxes_3d'].with_yaw == b['boxes_3d'].with_yaw and type(a['boxes_3d']) is type(b['boxes_3d'])
        if total:
            assert torch.equal(a['angles'], b['angles']) and torch.equal(a['layout'].tensor, b['layout'].tensor)
    print(cfg_name, 'detections', len(res[0]['scores_3d']))


@pytest.mark.parametrize('cfg_name,views', [('scannet_fast', 5), ('sunrgbd_fast', 1), ('scannet_v1', 4)])
def test_native_levels_equal_layerwise_indoor(ia, cfg_name, views):
    """Indoor families on the handle (IVX_NECK_FAST / IVX_NECK_UNET): ivx_model_forward_levels == features_2d_cl -> lift_cl
    -> neck_3d.forward_cl bit for bit on every level and on the valid mask, ivx_neck3d_{fast,unet}_fwd == neck_3d.forward_cl,
    and simple_test (which routes extract_feat through the handle) returns the layer-by-layer detections."""
    mcfg = getattr(kc, f'{cfg_name}_model_cfg')()
    tcfg = dict(getattr(kc, f'{cfg_name.upper()}_TEST_CFG'))
    model = ia.build_detector(mcfg, test_cfg=tcfg)
    ia.randomize_(model, 33)
    with torch.no_grad():
        g = torch.Generator().manual_seed(5)
        model.bbox_head.cls_conv.weight.normal_(0, 0.01, generator=g)
        model.bbox_head.cls_conv.bias.fill_(-2.0)
        model.bbox_head.centerness_conv.weight.normal_(0, 0.005, generator=g)
        model.bbox_head.reg_conv.weight.normal_(0, 0.002, generator=g)       # keeps exp(reg) finite: NaN != NaN would fail torch.equal
    model.prepare(torch.device('cuda'))
    assert model._native is not None and model._native.family == 'indoor'
    B, hw = 1, (480, 640)
    img = torch.randn(B, views, 3, *hw, generator=torch.Generator().manual_seed(9)).cuda()
    box_type = ia.DepthInstance3DBoxes
    metas = [kc.indoor_meta(views, img_hw=hw, box_type=box_type)]
    p0 = model.features_2d_cl(img)
    vol, valid = model.lift_cl(p0, metas)
    ref_levels = model.neck_3d.forward_cl(vol)
    proj, new_origin, crop = model._camera_setup(metas, 4, img.device)
    levels, ok = model._native.forward_levels(img.reshape(B * views, 3, *hw).contiguous(), B, views, hw[0], hw[1], proj, new_origin, crop)
    assert torch.equal(ok, valid)
    assert len(levels) == len(ref_levels) == 3
    for l, (a, b) in enumerate(zip(levels, ref_levels)):
        assert a.shape == b.shape, (l, a.shape, b.shape)
        assert torch.equal(a, b), f'level {l}: {(a != b).sum().item()} of {a.numel()} differ, max {(a - b).abs().max().item():.3e}'
    for l, (a, b) in enumerate(zip(model._native.neck3d_levels(vol), ref_levels)):
        assert torch.equal(a, b), f'neck-only level {l} differs'
    ref = model.detect_indoor_cl(vol, valid, metas)
    res = model.simple_test(img, metas)
    for (rb, rs, rl), r in zip(ref, res):
        assert torch.equal(r['scores_3d'], rs.cpu()) and torch.equal(r['labels_3d'], rl.cpu()) and torch.equal(r['boxes_3d'].tensor, rb.tensor.cpu())
    # the anchor entry points refuse an indoor handle, loudly
    with pytest.raises(ValueError, match='ivx_model_forward_levels'):
        model._native.forward(img.reshape(B * views, 3, *hw).contiguous(), B, views, hw[0], hw[1], proj, new_origin, crop)


def test_edge_cases_no_detections_and_no_valid_voxels(ia):
    """Edge cases of the whole path through the public call: (a) no anchor above score_thr -> empty results ([0, 7] boxes, empty
    scores / labels) for every sample, on the native handle and layer by layer alike; (b) a camera that sees none of the voxels ->
    valid mask all False, a zero volume, and the indoor tail still returns (every score is 0: the candidate top-k degenerates to
    204 800 ties, taken in index order by both top-k forms); (c) samples of one batch with different un-padded image sizes (crop)."""
    from imvoxelnet_amd import _lib
    # (a)
    model = _kitti_model(ia, (104, 120, 12))
    with torch.no_grad():
        model.bbox_head.conv_cls.bias.fill_(-30.0)
    model.prepare(torch.device('cuda'))
    hw = (192, 640)
    img = torch.randn(2, 1, 3, *hw, generator=torch.Generator().manual_seed(3)).cuda()
    metas = [kc.kitti_meta(img_hw=hw, box_type=ia.LiDARInstance3DBoxes) for _ in range(2)]
    assert model._native is not None
    res = model.simple_test(img, metas)
    p0 = model.features_2d_cl(img)
    vol, valid = model.lift_cl(p0, metas)
    ref = model.detect_cl(vol, metas)
    assert int(ref[3].sum()) == 0
    for r in res:
        assert tuple(r['boxes_3d'].tensor.shape) == (0, 7) and r['scores_3d'].numel() == 0 and r['labels_3d'].numel() == 0
    # (c) the second sample's image is smaller inside the same padded batch
    metas_c = [kc.kitti_meta(img_hw=hw, box_type=ia.LiDARInstance3DBoxes), kc.kitti_meta(img_hw=(160, 608), box_type=ia.LiDARInstance3DBoxes)]
    metas_c[1]['pad_shape'] = (hw[0], hw[1], 3)
    with torch.no_grad():
        model.bbox_head.conv_cls.bias.fill_(-1.5)
    model.prepare(torch.device('cuda'))
    proj, new_origin, crop = model._camera_setup(metas_c, 4, img.device)
    assert crop.tolist() == [[48, 160], [40, 152]]
    out = model._native.forward(img.reshape(2, 3, *hw).contiguous(), 2, 1, hw[0], hw[1], proj, new_origin, crop, want_valid=True)
    vol_c, valid_c = model.lift_cl(model.features_2d_cl(img), metas_c)
    _assert_same_detections(out[:4], model.detect_cl(vol_c, metas_c))
    assert torch.equal(out[4], valid_c) and int(valid_c[1].sum()) < int(valid_c[0].sum())
    # (b)
    m2 = ia.build_detector(kc.scannet_fast_model_cfg(), test_cfg=dict(kc.SCANNET_FAST_TEST_CFG))
    ia.randomize_(m2, 12)
    m2.prepare(torch.device('cuda'))
    V = 2
    img2 = torch.randn(1, V, 3, 480, 640, generator=torch.Generator().manual_seed(4)).cuda()
    meta = kc.indoor_meta(V, box_type=ia.DepthInstance3DBoxes)
    far = np.eye(4, dtype=np.float32)
    far[2, 3] = -100.0                        # every voxel ends up behind the camera (z < 0): nothing projects
    meta['lidar2img']['extrinsic'] = [far.copy() for _ in range(V)]
    out = {}
    for mode in (0, 1):
        _lib.lib().ivx_topk_set_mode(mode)
        try:
            out[mode] = m2.simple_test(img2, [meta])
        finally:
            _lib.lib().ivx_topk_set_mode(0)
    p0 = m2.features_2d_cl(img2)
    vol2, valid2 = m2.lift_cl(p0, [meta])
    assert not bool(valid2.any()) and float(vol2.abs().max()) == 0.0
    a, b = out[0][0], out[1][0]
    assert torch.equal(a['scores_3d'], b['scores_3d']) and torch.equal(a['boxes_3d'].tensor, b['boxes_3d'].tensor) and torch.equal(a['labels_3d'], b['labels_3d'])
    assert bool(torch.isfinite(a['boxes_3d'].tensor).all())


@pytest.mark.parametrize('name', ['kitti', 'nuscenes', 'fast', 'atlas'])
def test_native_handle_necks_vs_reference_golden(ia, name):
    """The four neck builders of the native handle (csrc/model.cpp) driven through the C-ABI alone -- ivx_create, the reference's
    state-dict keys via ivx_weights_load, ivx_neck3d_{kitti,nuscenes,fast,unet}_fwd -- against the imported reference modules'
    outputs (tests/golden/necks.npz): the same 1e-3 / 1e-4 bar as the Python composition's test_neck_golden."""
    import ctypes as C
    from helpers import load_npz
    from gpu_util import assert_close
    from imvoxelnet_amd import _lib
    from imvoxelnet_amd._lib import ModelCfg, check
    L = _lib.lib()
    g = load_npz('necks.npz')
    x = torch.from_numpy(g[name + '::x']).cuda()                                   # [B, C, X, Y, Z]
    B, Cin, X, Y, Z = x.shape
    cfg = ModelCfg()
    cfg.neck_type = {'kitti': 0, 'nuscenes': 1, 'fast': 2, 'atlas': 3}[name]
    cfg.with_trunk, cfg.fpn_channels, cfg.winograd = 0, Cin, 1
    cfg.neck_out_channels = 4 if name == 'atlas' else 8
    cfg.n_voxels[:] = [X, Y, Z]
    cfg.voxel_size[:] = [.1, .1, .1]
    if name in ('kitti', 'nuscenes'):           # the anchor head of these handles is not exercised here: any valid settings
        cfg.num_classes, cfg.n_sizes, cfg.n_rotations, cfg.nms_pre, cfg.max_num = 1, 1, 2, 10, 5
        cfg.anchor_range[:] = [0, 0, 0, 1, 1, 0]
        cfg.anchor_sizes[:3] = [1, 1, 1]
        cfg.anchor_rotations[:2] = [0, 1.57]
    if name == 'fast':
        cfg.fast_n_blocks[:] = [1, 1, 1]
    if name == 'atlas':
        cfg.unet_channels[:] = [4, 8, 16, 0]
        cfg.unet_down_layers[:] = [1, 2, 2, 0]
        cfg.unet_up_layers[:] = [2, 1, 0]
    h = C.c_void_p()
    check(L.ivx_create(C.byref(cfg), C.byref(h)), 'ivx_create')
    try:
        keep = []
        for k in g.files:
            if not k.startswith(name + '::sd::') or 'num_batches_tracked' in k:
                continue
            a = np.ascontiguousarray(g[k], dtype=np.float32)
            keep.append(a)
            shape = (C.c_int64 * max(a.ndim, 1))(*a.shape)
            check(L.ivx_weights_load(h, ('neck_3d.' + k.split('::sd::')[1]).encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim), k)
        if name in ('kitti', 'nuscenes'):       # the fused head conv of the handle wants its three tensors: zeros
            for key, co in (('bbox_head.conv_cls', 2), ('bbox_head.conv_reg', 14), ('bbox_head.conv_dir_cls', 4)):
                for sfx, shp in (('.weight', (co, 8, 1, 1)), ('.bias', (co,))):
                    a = np.zeros(shp, np.float32)
                    keep.append(a)
                    check(L.ivx_weights_load(h, (key + sfx).encode(), a.ctypes.data_as(C.c_void_p), (C.c_int64 * len(shp))(*shp), len(shp)), key)
        check(L.ivx_weights_finalize(h, None), 'ivx_weights_finalize')
        vol = x.permute(0, 2, 3, 4, 1).contiguous()                                  # channels-last [B, X, Y, Z, C]
        n = L.ivx_neck3d_workspace_bytes(h, B)
        assert n > 0, L.ivx_last_error()
        ws = torch.empty((n,), device='cuda', dtype=torch.uint8)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if name in ('kitti', 'nuscenes'):
            Xo, Yo, Co = C.c_int32(), C.c_int32(), C.c_int32()
            check(L.ivx_neck3d_out_dims(h, B, C.byref(Xo), C.byref(Yo), C.byref(Co)), 'ivx_neck3d_out_dims')
            out = torch.empty((B, Xo.value, Yo.value, 1, Co.value), device='cuda')
            fn = L.ivx_neck3d_kitti_fwd if name == 'kitti' else L.ivx_neck3d_nuscenes_fwd
            check(fn(h, C.c_void_p(vol.data_ptr()), B, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), n, st), 'neck fwd')
            got = [out[:, :, :, 0].permute(0, 3, 2, 1)]                              # the reference returns [B, C, Y', X'] (necks/imvoxelnet.py:120)
        else:
            dims = ((C.c_int32 * 4) * 3)()
            check(L.ivx_neck3d_levels(h, B, dims), 'ivx_neck3d_levels')
            outs = [torch.empty((B, d[0], d[1], d[2], d[3]), device='cuda') for d in dims if d[3] > 0]
            ptrs = (C.c_void_p * 3)(*([o.data_ptr() for o in outs] + [None] * (3 - len(outs))))
            fn = L.ivx_neck3d_fast_fwd if name == 'fast' else L.ivx_neck3d_unet_fwd
            check(fn(h, C.c_void_p(vol.data_ptr()), B, ptrs, C.c_void_p(ws.data_ptr()), n, st), 'neck fwd')
            got = [o.permute(0, 4, 1, 2, 3) for o in outs]
        torch.cuda.synchronize()
        n_out = len([k for k in g.files if k.startswith(name + '::y')])
        assert len(got) == n_out
        for i, y in enumerate(got):
            assert_close(f'{name} native neck level {i}', y.contiguous().cpu().numpy(), g[f'{name}::y{i}'], 1e-3, 1e-4)
    finally:
        L.ivx_destroy(h)


def test_bench_rccl_path_at_world_size_1(ia):
    """bench.py under the driver's launcher with IVX_BENCH_FORCE_DIST=1: the process group is RCCL ('nccl'), every timed step runs
    simple_test(gather=True) -> all_gather_into_tensor of the padded detections, and the JSON line carries the self-checks of the
    N > 1 line (rccl_ranks from an actual all-reduce, per-rank ms) -- so the collective path executes on the GPU box every round even
    though the box has one GPU."""
    import json
    env = dict(os.environ, IVX_BENCH_FORCE_DIST='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '1', '--master-addr', '127.0.0.1', '--master-port', '29533',
           os.path.join(ROOT, 'bench.py'), '--full', '--gpus', '1', '--steps', '3', '--warmup', '1', '--no-cpu-baseline']
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert out.returncode == 0 and len(lines) == 1, out.stdout[-2000:] + out.stderr[-2000:]
    rec = json.loads(lines[0])
    assert rec['n_gpus'] == 1 and rec['config']['rccl_ranks'] == 1 and len(rec['config']['ms_per_step_by_rank']) == 1
    assert rec['config']['collective'] and rec['value'] > 50 and rec['config']['detections_last_step'] > 0
    # default operands: fp16 pairs priced against the 16-bit MFMA peak (every product counted); in fp32 multiply-adds the GEMMs must beat
    # what the fp32 MFMA form could ever reach
    assert rec['roofline']['frac'] > 0.2 and rec['roofline']['fp32_equivalent_tflops'] > 160 and rec['measured_ceilings']['hbm_copy_gbps'] > 3000


def test_bench_plain_line_and_dump_outputs(ia, tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W` times exactly K steps and prints the headline figure only (the stage figures,
    ceilings and CPU legs are behind --full); --dump-outputs writes the last timed step's detections, identical from run to run."""
    import json
    recs = []
    for d in ('a', 'b'):
        cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--dump-outputs', str(tmp_path / d)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
        lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
        assert out.returncode == 0 and len(lines) == 1, out.stdout[-2000:] + out.stderr[-2000:]
        recs.append(json.loads(lines[0]))
    rec = recs[0]
    assert rec['steps'] == 3 and rec['warmup'] == 1 and rec['unit'] == 'images/s' and rec['higher_is_better'] is True and rec['dtype']
    assert rec['ms_per_step'] > 0 and abs(rec['value'] - 4 * 1e3 / rec['ms_per_step']) <= 0.01 * rec['value']
    assert not any(k in rec for k in ('roofline', 'measured_ceilings', 'exact_fp32_mfma', 'extra_configs', 'cpu_baseline'))
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == sorted(f'{k}_{b}.npy' for k in ('boxes_3d', 'scores_3d', 'labels_3d') for b in range(4))
    assert sum(len(np.load(tmp_path / 'a' / f'scores_3d_{b}.npy')) for b in range(4)) == rec['config']['detections_last_step'] > 0
    for n in names:
        a, b = np.load(tmp_path / 'a' / n), np.load(tmp_path / 'b' / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n


def test_rccl_two_gpus_gather_and_slab_exchange(ia):
    """First contact with a multi-GPU node (round-4 verdict item 8): two ranks over RCCL -- simple_test(gather=True) on the halves of a
    batch equals simple_test over the whole batch on one GPU, and the view-sharded step (reduce-scatter over x-slabs / all-reduce) equals
    the single-GPU call.  On the one-GPU boxes of this pool the same worker runs at world size 1; tests/test_host_cpu.py covers the
    exchanges between ranks on gloo."""
    import json
    n = 2 if torch.cuda.device_count() >= 2 else 1       # one-GPU boxes: the same worker at world size 1 (RCCL group of one rank), so the code runs every round
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
        env.pop(k, None)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n), '--master-addr', '127.0.0.1', '--master-port', '29541',
           os.path.join(ROOT, 'tests', 'rccl_worker.py')]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert out.returncode == 0 and len(lines) == 1, out.stdout[-2000:] + out.stderr[-2000:]
    rec = json.loads(lines[0])
    assert rec['world'] == n and rec['rccl_ranks'] == n
    assert rec['gather_len'] == 2 * n and rec['gather_same'] and rec['gather_detections'] > 0
    assert rec['ragged_gather_len'] == 2 * n + 1 and rec['ragged_gather_same']           # shards that differ by one sample
    assert rec['view_sharded_same']


@pytest.mark.parametrize('cfg_name,views', [('scannet_v1', 6), ('scannet_fast', 4), ('sunrgbd_fast', 1), ('kitti', 1)])
def test_native_bf16_storage_equals_layerwise(ia, cfg_name, views):
    """The optional reduced-precision mode BASELINE config 5 names, INSIDE the model-level C-ABI (ivx_model_cfg.storage = IVX_BF16):
    simple_test through one native call (bf16 activations and weights, the s2d stem, bf16 unprojection / trilinear steps, fp32 head
    outputs and tails) against the layer-by-layer bf16 composition over the op-level ABI -- the same kernels with the same plans:
    identical detections bit for bit."""
    if cfg_name == 'kitti':
        mcfg, tcfg = kc.kitti_model_cfg(n_voxels=(104, 120, 12)), dict(kc.KITTI_TEST_CFG)
        hw, metas = (192, 640), [kc.kitti_meta(img_hw=(192, 640), box_type=ia.LiDARInstance3DBoxes) for _ in range(2)]
        B = 2
    else:
        mcfg, tcfg = getattr(kc, f'{cfg_name}_model_cfg')(), dict(getattr(kc, f'{cfg_name.upper()}_TEST_CFG'))
        hw = (480, 640)
        metas = [kc.indoor_meta(views, img_hw=hw, origin=(0, 3, -1) if cfg_name == 'sunrgbd_fast' else (0, 0, .5), box_type=ia.DepthInstance3DBoxes)]
        B = 1
    model = ia.build_detector(mcfg, test_cfg=tcfg)
    ia.randomize_(model, 41)
    with torch.no_grad():
        g = torch.Generator().manual_seed(5)
        if cfg_name == 'kitti':
            model.bbox_head.conv_cls.weight.normal_(0, 0.05, generator=g)
            model.bbox_head.conv_cls.bias.fill_(-1.0)
            model.bbox_head.conv_reg.weight.normal_(0, 0.002, generator=g)
        else:
            model.bbox_head.cls_conv.weight.normal_(0, 0.01, generator=g)
            model.bbox_head.cls_conv.bias.fill_(-2.0)
            model.bbox_head.centerness_conv.weight.normal_(0, 0.005, generator=g)
            model.bbox_head.reg_conv.weight.normal_(0, 0.002, generator=g)
    img = torch.randn(B, views, 3, *hw, generator=torch.Generator().manual_seed(9)).cuda()
    model.prepare(torch.device('cuda'), dtype=torch.bfloat16, native=False)
    ref = model.simple_test(img, metas)
    model.prepare(torch.device('cuda'), dtype=torch.bfloat16)
    assert model._native is not None and model._native.cfg.storage == 1
    res = model.simple_test(img, metas)
    assert len(res) == len(ref) == B and sum(len(r['scores_3d']) for r in ref) > 5
    for a, b in zip(res, ref):
        assert torch.equal(a['scores_3d'], b['scores_3d']) and torch.equal(a['labels_3d'], b['labels_3d'])
        assert torch.equal(a['boxes_3d'].tensor, b['boxes_3d'].tensor)
    print(cfg_name, 'bf16 storage: detections', [len(r['scores_3d']) for r in res])


def test_c_program_e2e_indoor_bf16_storage_without_python(ia):
    """The third C host run (verdict round 3, item 6): tests/c/e2e_indoor.c with `bf16` -- ivx_model_cfg.storage = IVX_BF16 -- on the
    reference's indoor end-to-end goldens: valid masks identical, at least 80 % of the fp32 reference's detections found."""
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'c'))
    import build as cbuild
    exe = cbuild.build('e2e_indoor')
    fx = os.path.join(ROOT, 'tests', 'golden', 'e2e_indoor.bin')
    out = subprocess.run([exe, fx, 'bf16'], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'C e2e_indoor OK (bf16 storage)' in out.stdout


@pytest.mark.parametrize('cfg_name,views,variant', [('scannet_v1', 6, 'conv3'), ('scannet_fast', 4, 'conv3'), ('scannet_v1', 6, 'full')])
def test_native_config5_named_mode_equals_layerwise(ia, cfg_name, views, variant):
    """BASELINE config 5's named mode -- bf16 storage with the fp8 2-D conv trunk (e4m3 bottleneck interiors, bf16 residual stream) --
    behind the C-ABI (ivx_model_cfg.storage = IVX_BF16 + ivx_model_calibrate_fp8): one native call against the layer-by-layer
    composition of ImVoxelNet.calibrate_fp8(residual='bf16'): the same calibration maxima, the same e4m3 filters and epilogue vectors,
    the same kernels -- identical detections."""
    mcfg, tcfg = getattr(kc, f'{cfg_name}_model_cfg')(), dict(getattr(kc, f'{cfg_name.upper()}_TEST_CFG'))
    hw = (480, 640)
    metas = [kc.indoor_meta(views, img_hw=hw, origin=(0, 0, .5), box_type=ia.DepthInstance3DBoxes)]
    model = ia.build_detector(mcfg, test_cfg=tcfg)
    ia.randomize_(model, 43)
    with torch.no_grad():
        g = torch.Generator().manual_seed(5)
        model.bbox_head.cls_conv.weight.normal_(0, 0.01, generator=g)
        model.bbox_head.cls_conv.bias.fill_(-2.0)
        model.bbox_head.centerness_conv.weight.normal_(0, 0.005, generator=g)
        model.bbox_head.reg_conv.weight.normal_(0, 0.002, generator=g)
    img = torch.randn(1, views, 3, *hw, generator=torch.Generator().manual_seed(9)).cuda()
    model.prepare(torch.device('cuda'), dtype=torch.bfloat16, native=False)
    model.calibrate_fp8(img, variant=variant)      # 'conv3': e4m3 on conv3 of stages 3 - 4 only (round 6, the default); 'full': the round-3 mode
    assert model._native is None
    ref = model.simple_test(img, metas)
    fpn_ref = model.features_2d_cl(img).float()
    model.prepare(torch.device('cuda'), dtype=torch.bfloat16)
    model.calibrate_fp8(img, variant=variant)
    assert model._native is not None and model._native.cfg.storage == 1
    fpn_nat = model._native.backbone_fpn(img.reshape(views, 3, *hw)).float()
    res = model.simple_test(img, metas)
    torch.cuda.synchronize()
    d = float((fpn_nat - fpn_ref).abs().max())
    print(cfg_name, 'fp8 trunk: max |FPN native - layerwise|', d, 'detections', len(res[0]['scores_3d']), len(ref[0]['scores_3d']))
    assert torch.equal(fpn_nat, fpn_ref)
    assert len(ref[0]['scores_3d']) > 5
    for a, b in zip(res, ref):
        assert torch.equal(a['scores_3d'], b['scores_3d']) and torch.equal(a['labels_3d'], b['labels_3d'])
        assert torch.equal(a['boxes_3d'].tensor, b['boxes_3d'].tensor)
