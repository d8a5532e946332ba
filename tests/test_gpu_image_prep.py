"""-m gpu: the device-side image pipeline (include/imvoxel.h ivx_image_prep_u8, csrc/image_prep.hip; ops.image_prep_u8,
data.prepare_images_device, ImVoxelNet.simple_test_u8) against the host pipeline it restates: data.imresize_cv2_linear for the resize alone,
data.prepare_image for Resize -> Normalize -> Pad.  Both are integer-exact restatements with one fp32 subtract and one IEEE divide per value,
so every comparison is torch.equal / np.array_equal: NO tolerance.  The single exception is the independent fp64 bilinear check of one
up-scale, whose bound of one grey level is the one tests/test_host_cpu.py already holds the host function to."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kitti_cfg as kc

pytestmark = pytest.mark.gpu

# source (h, w) and img_scale of the four reference test pipelines
GEOMETRIES = {'kitti': ((375, 1242), (1280, 384)), 'nuscenes': ((900, 1600), (1600, 900)), 'scannet': ((968, 1296), (640, 480)),
              'sunrgbd': ((530, 730), (640, 480))}


@pytest.fixture(scope='module')
def ia():
    import imvoxelnet_amd
    assert torch.cuda.is_available()
    return imvoxelnet_amd


def _frame(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _nan(*shape):
    return torch.full(shape, float('nan'), device='cuda')


def _resize_gpu(ia, img, size_hw, src=None):
    """The resize alone: mean 0, std 1, no channel swap, no padding -> the output floats are the resized uint8 values."""
    src = torch.from_numpy(img)[None].cuda() if src is None else src
    out = ia.ops.image_prep_u8(src, size_hw, size_hw, (0, 0, 0), (1, 1, 1), to_rgb=False, out=_nan(1, 3, *size_hw))
    got = out[0].permute(1, 2, 0).cpu().numpy()
    assert np.array_equal(got, np.rint(got)) and got.min() >= 0 and got.max() <= 255
    return got.astype(np.uint8)


RESIZE_CASES = [
    ('kitti', (375, 1242), (384, 1272)), ('nuscenes', (900, 1600), (900, 1600)), ('scannet', (968, 1296), (478, 640)),
    ('sunrgbd', (530, 730), (465, 640)),
    ('half_both', (768, 2560), (384, 1280)),                     # the INTER_AREA shortcut
    ('half_h_only', (96, 200), (48, 150)), ('half_w_only', (90, 200), (64, 100)),      # must NOT take it
    ('identity', (37, 53), (37, 53)), ('same_h', (37, 53), (37, 80)), ('up', (37, 53), (74, 159)), ('up_2x', (40, 30), (80, 60)),
    ('down_3x', (300, 420), (100, 140)), ('down_odd', (301, 97), (43, 31)),
    ('row', (1, 97), (1, 40)), ('row_up', (1, 40), (3, 97)), ('col', (97, 1), (40, 1)), ('col_up', (40, 1), (97, 5)), ('dot', (1, 1), (7, 9)),
    ('border_2x2', (2, 2), (9, 11)),                              # every position is border-clamped or between the only two samples
]


@pytest.mark.parametrize('name,src_hw,dst_hw', RESIZE_CASES, ids=[c[0] for c in RESIZE_CASES])
def test_resize_equals_imresize_cv2_linear(ia, name, src_hw, dst_hw):
    if name in GEOMETRIES:
        assert ia.data.rescale_size(src_hw, GEOMETRIES[name][1]) == dst_hw
    img = _frame(11, *src_hw)
    ref = ia.data.imresize_cv2_linear(img, dst_hw)
    got = _resize_gpu(ia, img, dst_hw)
    bad = np.argwhere(got != ref)
    print(f'{name}: {src_hw} -> {dst_hw}: {len(bad)} of {ref.size} values differ')
    assert np.array_equal(got, ref), f'first differences at {bad[:5].tolist()}: got {got[got != ref][:5]} ref {ref[got != ref][:5]}'


def test_resize_half_on_one_axis_is_not_the_area_mean(ia):
    """The shortcut needs an exact half on BOTH axes: with one axis halved the 2x2 mean of a matching crop is a different image."""
    img = _frame(12, 96, 200)
    got = _resize_gpu(ia, img, (48, 150))
    area = ia.data.imresize_cv2_linear(img[:, :100], (48, 50))                  # what the shortcut computes on a 96 x 100 crop
    lin = ia.data.imresize_cv2_linear(img, (48, 150))
    assert np.array_equal(got, lin) and not np.array_equal(got[:, :50], area)


def test_resize_hand_derived_vectors(ia):
    """The vectors of test_imresize_cv2_linear_hand_derived_vectors, on the device."""
    def line(vals, n):
        img = np.repeat(np.array(vals, np.uint8)[None, :, None], 3, axis=2)      # 1 x len x 3
        return _resize_gpu(ia, img, (1, n))[0, :, 0].tolist(), _resize_gpu(ia, np.ascontiguousarray(img.transpose(1, 0, 2)), (n, 1))[:, 0, 1].tolist()
    assert line([0, 100], 4) == ([0, 25, 75, 100],) * 2
    assert line([10, 20, 40], 5) == ([10, 14, 20, 32, 40],) * 2
    block = np.repeat(np.array([[1, 2], [3, 5]], np.uint8)[:, :, None], 3, axis=2)
    assert _resize_gpu(ia, block, (1, 1)).tolist() == [[[3, 3, 3]]]                 # exact half: (11 + 2) >> 2
    for hw, to in (((5, 7), (13, 4)), ((8, 8), (4, 4)), ((3, 3), (3, 3))):
        const = np.full(hw + (3,), 77, np.uint8)
        assert (_resize_gpu(ia, const, to) == 77).all()


def test_resize_row_pitch_and_frame_stride(ia):
    """src_row_bytes above 3 * W (a decoder pitch) and a frame stride above H * pitch: the padding bytes are never read into the result."""
    img = np.stack([_frame(13, 45, 61), _frame(14, 45, 61)])
    buf = torch.full((2, 50, 3 * 61 + 17), 255, dtype=torch.uint8, device='cuda')
    view = torch.as_strided(buf, (2, 45, 61, 3), (buf.stride(0), buf.stride(1), 3, 1))
    view.copy_(torch.from_numpy(img).cuda())
    assert view.stride() == (50 * 200, 200, 3, 1) and not view.is_contiguous()
    out = ia.ops.image_prep_u8(view, (32, 40), (32, 40), (0, 0, 0), (1, 1, 1), to_rgb=False, out=_nan(2, 3, 32, 40))
    for i in range(2):
        assert np.array_equal(out[i].permute(1, 2, 0).cpu().numpy().astype(np.uint8), ia.data.imresize_cv2_linear(img[i], (32, 40)))
    assert torch.equal(out, ia.ops.image_prep_u8(torch.from_numpy(img).cuda(), (32, 40), (32, 40), (0, 0, 0), (1, 1, 1), to_rgb=False))


def test_resize_within_one_grey_level_of_fp64_bilinear(ia):
    """Second, independent reference for one up-scale: F.interpolate(bilinear, align_corners=False) in fp64.  The bound (one grey level: 11-bit
    weights and two truncating shifts against exact arithmetic) is the one the project holds data.imresize_cv2_linear to; it is asserted for the
    host function on this input first, then for the kernel."""
    img = _frame(15, 37, 53)
    exact = F.interpolate(torch.from_numpy(img).double().permute(2, 0, 1)[None], size=(74, 159), mode='bilinear', align_corners=False)[0]
    exact = exact.permute(1, 2, 0).numpy()
    host = ia.data.imresize_cv2_linear(img, (74, 159)).astype(np.float64)
    assert np.abs(host - exact).max() <= 1.0
    got = _resize_gpu(ia, img, (74, 159)).astype(np.float64)
    print('max |kernel - fp64 bilinear|', np.abs(got - exact).max(), 'host', np.abs(host - exact).max())
    assert np.abs(got - exact).max() <= 1.0


# ------------------------------------------------------------------ Resize -> Normalize -> Pad
def _pipeline_gpu(ia, img, img_scale, cfg, pad_hw=None, out=None):
    nh, nw = ia.data.rescale_size(img.shape[:2], img_scale)
    ph, pw = pad_hw or ((nh + 31) // 32 * 32, (nw + 31) // 32 * 32)
    out = _nan(1, 3, ph, pw) if out is None else out
    res = ia.ops.image_prep_u8(torch.from_numpy(img)[None].cuda(), (nh, nw), (ph, pw), cfg['mean'], cfg['std'], cfg['to_rgb'], out=out)
    assert res.data_ptr() == out.data_ptr()
    return res[0].cpu()


@pytest.mark.parametrize('to_rgb', [True, False])
@pytest.mark.parametrize('name', list(GEOMETRIES))
def test_pipeline_bit_equal_to_prepare_image(ia, name, to_rgb):
    """The four dataset geometries with IMG_NORM_CFG, channel swap on and off, into a NaN-filled tensor: every bit of prepare_image's tensor,
    the zero pad region included."""
    src_hw, scale = GEOMETRIES[name]
    img = _frame(21, *src_hw)
    cfg = dict(ia.data.IMG_NORM_CFG, to_rgb=to_rgb)
    ref, meta = ia.data.prepare_image(img, scale, cfg)
    got = _pipeline_gpu(ia, img, scale, cfg)
    assert got.shape == ref.shape == (3,) + meta['pad_shape'][:2]
    nh, nw = meta['img_shape'][:2]
    assert not torch.isnan(got).any() and (got[:, nh:] == 0).all() and (got[:, :, nw:] == 0).all()
    assert not torch.signbit(got[:, nh:]).any() and not torch.signbit(got[:, :, nw:]).any()           # +0.0f
    n_bad = int((got.view(torch.int32) != ref.view(torch.int32)).sum())
    print(f'{name} to_rgb={to_rgb}: {src_hw} -> {(nh, nw)} in {tuple(ref.shape[1:])}: {n_bad} of {ref.numel()} words differ')
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))


def test_pipeline_scalar_store_path(ia):
    """pad_w % 4 != 0 and an `out` that is 4 bytes off 16-byte alignment are accepted and give the same bits as the 16-byte path."""
    img = _frame(22, 375, 1242)
    cfg = ia.data.IMG_NORM_CFG
    ref, _ = ia.data.prepare_image(img, (1280, 384), cfg)
    base = _pipeline_gpu(ia, img, (1280, 384), cfg)
    assert torch.equal(base.view(torch.int32), ref.view(torch.int32))
    buf = _nan(3 * 384 * 1280 + 8)
    assert buf.data_ptr() % 16 == 0
    off = buf[1:1 + 3 * 384 * 1280].view(1, 3, 384, 1280)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    got = _pipeline_gpu(ia, img, (1280, 384), cfg, out=off)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    assert torch.isnan(buf[0]) and torch.isnan(buf[1 + 3 * 384 * 1280:]).all()                # nothing outside the view is written
    for pw in (1273, 1274, 1275, 1272):                                                       # 1272 % 4 == 0: no pad columns at all
        got = _pipeline_gpu(ia, img, (1280, 384), cfg, pad_hw=(385, pw))
        want = F.pad(ref[:, :384, :1272], (0, pw - 1272, 0, 1))
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), pw
    small = _frame(23, 7, 5)                                                                  # dst_w not a multiple of 4 inside a 16-byte plane
    ref, _ = ia.data.prepare_image(small, (5, 7), cfg, size_divisor=4)
    nan_out = _nan(1, 3, 8, 8)
    got = ia.ops.image_prep_u8(torch.from_numpy(small)[None].cuda(), (7, 5), (8, 8), cfg['mean'], cfg['std'], True, out=nan_out)[0].cpu()
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))


def test_batch_of_50_equals_50_single_calls(ia):
    """n = 50 SUN RGB-D frames in one launch == 50 launches of one frame == prepare_image.  50 x 480 x 160 work items are 15 000 workgroups of
    256 against a grid capped at 2 048, so the grid-stride loop runs about seven times per thread; the NaN pre-fill shows every word written."""
    frames = np.stack([_frame(100 + i, 530, 730) for i in range(50)])
    cfg = ia.data.IMG_NORM_CFG
    src = torch.from_numpy(frames).cuda()
    assert 50 * 480 * (640 // 4) > 2048 * 256
    batch = ia.ops.image_prep_u8(src, (465, 640), (480, 640), cfg['mean'], cfg['std'], True, out=_nan(50, 3, 480, 640))
    assert not torch.isnan(batch).any()
    single = torch.cat([ia.ops.image_prep_u8(src[i:i + 1], (465, 640), (480, 640), cfg['mean'], cfg['std'], True, out=_nan(1, 3, 480, 640)) for i in range(50)])
    assert torch.equal(batch.view(torch.int32), single.view(torch.int32))
    for i in (0, 17, 49):
        ref, _ = ia.data.prepare_image(frames[i], (640, 480), cfg)
        assert torch.equal(batch[i].cpu().view(torch.int32), ref.view(torch.int32)), i


def _expected(ia, frames, img_scale, plane):
    out = torch.zeros(len(frames), 3, *plane)
    metas = []
    for i, f in enumerate(frames):
        t, m = ia.data.prepare_image(f, img_scale)
        out[i, :, :t.shape[1], :t.shape[2]] = t
        metas.append(m)
    return out, metas


def test_prepare_images_device_mixed_sizes_and_multi_view(ia):
    """The mixed-size KITTI batch and a [2][3] multi-view input == per-frame prepare_image placed into the common pad plane."""
    frames = [_frame(31, 375, 1242), _frame(32, 370, 1224), _frame(33, 375, 1242), _frame(34, 370, 1224)]
    img, metas = ia.prepare_images_device(frames, (1280, 384))
    ref, ref_metas = _expected(ia, frames, (1280, 384), (384, 1280))
    assert img.is_cuda and img.shape == (4, 3, 384, 1280) and metas == ref_metas
    assert torch.equal(img.cpu().view(torch.int32), ref.view(torch.int32))
    # device frames and a stacked device batch are used where they are
    img2, _ = ia.prepare_images_device([torch.from_numpy(f).cuda() for f in frames], (1280, 384))
    assert torch.equal(img2, img)
    img3, _ = ia.prepare_images_device(torch.from_numpy(np.stack(frames[0::2])).cuda(), (1280, 384))
    assert torch.equal(img3, img[0::2])
    views = [[_frame(40 + 3 * b + v, 530, 730) for v in range(3)] for b in range(2)]
    views[1][2] = _frame(50, 480, 600)                       # the last view of sample 1: another size (and a smaller pad plane of its own)
    img, metas = ia.prepare_images_device(views, (640, 480))
    flat = [f for s in views for f in s]
    ref, ref_metas = _expected(ia, flat, (640, 480), (480, 640))
    assert img.shape == (2, 3, 3, 480, 640) and metas == [ref_metas[2], ref_metas[5]] and metas[1]['ori_shape'] == (480, 600, 3)
    assert torch.equal(img.cpu().view(torch.int32), ref.view(2, 3, 3, 480, 640).view(torch.int32))


# ------------------------------------------------------------------ end to end
def _same_results(res, ref):
    assert len(res) == len(ref)
    for a, b in zip(res, ref):
        assert torch.equal(a['scores_3d'], b['scores_3d']) and torch.equal(a['labels_3d'], b['labels_3d'])
        assert torch.equal(a['boxes_3d'].tensor, b['boxes_3d'].tensor) and type(a['boxes_3d']) is type(b['boxes_3d'])


def test_simple_test_u8_equals_simple_test_kitti(ia):
    """The smoke-sized KITTI model of __graft_entry__.smoke: simple_test_u8 on uint8 frames returns exactly the boxes, scores and labels of
    simple_test on the tensor prepare_image builds (the inputs are bit-identical).  96 x 318 frames up-scale to 384 x 1272 and pad to
    384 x 1280, multiples of 32, so the native handle takes them."""
    nv = (24, 28, 12)
    cfg = kc.kitti_model_cfg(n_voxels=nv, in_ch=16, out_ch=32)
    ox = 0.5 + nv[0] * .32 / 2
    cfg['bbox_head']['anchor_generator']['ranges'] = [[ox - nv[0] * .16, -nv[1] * .16, -1.78, ox + nv[0] * .16 - .32, nv[1] * .16 - .32, -1.78]]
    model = ia.build_detector(cfg, test_cfg=dict(kc.KITTI_TEST_CFG, score_thr=0.05))
    ia.randomize_(model, 7)
    with torch.no_grad():
        model.bbox_head.conv_cls.weight.normal_(0, 0.05, generator=torch.Generator().manual_seed(1))
        model.bbox_head.conv_cls.bias.fill_(-1.5)
    frames = [_frame(60, 96, 318), _frame(61, 96, 318)]
    K = np.array([[143., 0, 159, 0], [0, 143., 48, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)      # in ori_shape pixels, as the dataset's
    user = []
    for b in range(2):
        E = np.array([[0, -1, 0, 0.03 * b], [0, 0, -1, 0.2], [1, 0, 0, 0.1], [0, 0, 0, 1]], np.float32)
        user.append(dict(box_type_3d=ia.LiDARInstance3DBoxes, lidar2img=dict(intrinsic=K, extrinsic=[E], origin=np.array([ox, 0, -1.0], np.float32))))
    prepared = [ia.data.prepare_image(f, (1280, 384)) for f in frames]
    img = torch.stack([t for t, _ in prepared])[:, None].cuda()
    assert img.shape == (2, 1, 3, 384, 1280)
    ref = model.simple_test(img, [dict(u, **m) for u, (_, m) in zip(user, prepared)])
    assert model._native is not None
    res = model.simple_test_u8(frames, user, (1280, 384))
    assert all('img_shape' not in u for u in user)
    print('kitti detections', [len(r['scores_3d']) for r in ref])
    assert sum(len(r['scores_3d']) for r in ref) > 0
    _same_results(res, ref)


def test_simple_test_u8_equals_simple_test_indoor_multi_view(ia):
    """The same with the multi-view ScanNet fast model of workloads.py: one sample of 4 views, 968 x 1296 frames -> 478 x 640 in 480 x 640."""
    V = 4
    model = ia.build_detector(kc.scannet_fast_model_cfg(), test_cfg=dict(kc.SCANNET_FAST_TEST_CFG))
    ia.randomize_(model, 33)
    with torch.no_grad():
        g = torch.Generator().manual_seed(5)
        model.bbox_head.cls_conv.weight.normal_(0, 0.01, generator=g)
        model.bbox_head.cls_conv.bias.fill_(-2.0)
        model.bbox_head.centerness_conv.weight.normal_(0, 0.005, generator=g)
        model.bbox_head.reg_conv.weight.normal_(0, 0.002, generator=g)
        for i, sc in enumerate(model.bbox_head.scales):
            sc.scale.fill_(1.0 + 0.125 * i)
    views = [[_frame(70 + v, 968, 1296) for v in range(V)]]
    meta = kc.indoor_meta(V, box_type=ia.DepthInstance3DBoxes)
    user = [{k: v for k, v in meta.items() if k not in ('img_shape', 'ori_shape')}]
    prepared = [ia.data.prepare_image(f, (640, 480)) for f in views[0]]
    img = torch.stack([t for t, _ in prepared])[None].cuda()
    assert img.shape == (1, V, 3, 480, 640)
    ref = model.simple_test(img, [dict(user[0], **prepared[-1][1])])
    assert model._native is not None
    res = model.simple_test_u8(views, user, (640, 480))
    print('scannet fast detections', len(ref[0]['scores_3d']))
    assert len(ref[0]['scores_3d']) > 5
    _same_results(res, ref)
