"""-m gpu: streaming scenes -- the accumulate mode of the unprojection kernel (ops.backproject_accum_ / ops.volume_mean) against the
imported reference's golden vectors and the one-shot lift, bit for bit, and SceneSession (model.open_scene) against simple_test."""
import numpy as np
import pytest
import torch

from helpers import load_npz, sub
from gpu_util import cl
import kitti_cfg as kc
from imvoxelnet_amd.workloads import _look_at

pytestmark = pytest.mark.gpu

GARBAGE = 0x7f7f7f7f


@pytest.fixture(scope='module')
def ia():
    import imvoxelnet_amd
    from imvoxelnet_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    return imvoxelnet_amd


# ------------------------------------------------------------------ the kernel
def _golden(case):
    c = sub(load_npz('backproject_cases.npz'), case + '::')
    nv, vs = tuple(int(v) for v in c['n_voxels']), c['voxel_size']
    P = torch.from_numpy(c['projection'])[None].cuda().contiguous()
    new_origin = (torch.from_numpy(c['origin']) - torch.tensor(nv) / 2. * torch.from_numpy(vs))[None].cuda().contiguous()
    crop = torch.tensor([[int(c['img_shape'][0]) // 4, int(c['img_shape'][1]) // 4]], dtype=torch.int32).cuda()
    return c, cl(c['feat']), P, new_origin, crop, vs, nv


def _state(B, nv, C, dtype=torch.float32):
    """A running state and output buffers pre-filled with NaN / garbage / sentinels."""
    dev = 'cuda'
    return dict(sum=torch.full((B,) + nv + (C,), float('nan'), device=dev), count=torch.full((B,) + nv, GARBAGE, device=dev, dtype=torch.int32),
                mean=torch.full((B,) + nv + (C,), -7.0, device=dev, dtype=dtype), valid=torch.full((B,) + nv, 7, device=dev, dtype=torch.uint8))


def _accumulate(ops, st, feat, P, new_origin, crop, vs, chunks, emit):
    """The views of feat [B*V,1,FH,FW,C] / P [B,V,3,4] in chunks of the given sizes, the first with first=1."""
    B, V = P.shape[0], P.shape[1]
    assert sum(chunks) == V
    f = feat.view(B, V, *feat.shape[1:])
    v0 = 0
    for n in chunks:
        ops.backproject_accum_(f[:, v0:v0 + n].reshape(B * n, *feat.shape[1:]).contiguous(), P[:, v0:v0 + n].contiguous(), new_origin, crop, vs,
                               st['sum'], st['count'], v0 == 0, st['mean'] if emit else None, st['valid'] if emit else None)
        v0 += n


GOLDEN_CHUNKS = [('C', c) for c in [(1, 1, 1, 1, 1, 1), (2, 4), (5, 1), (3, 3), (6,)]] + [('B', c) for c in [(1, 1), (2,)]]


@pytest.mark.parametrize('case,chunks', GOLDEN_CHUNKS, ids=[f'{k}-{"_".join(map(str, c))}' for k, c in GOLDEN_CHUNKS])
def test_chunked_accumulate_equals_reference_bit_for_bit(ia, case, chunks):
    """Views added chunk by chunk, the first chunk with first=1 over a NaN / garbage state: mean, mask and count after the last chunk
    are the imported reference's, bit for bit.  784 / 864 voxels: a partial last workgroup; the chunk of 3 is wider than the lane
    group (2 lanes at C = 8), so it takes a second, partial round of the projection loop."""
    from imvoxelnet_amd import ops
    c, feat, P, no, crop, vs, nv = _golden(case)
    st = _state(1, nv, feat.shape[-1])
    _accumulate(ops, st, feat, P, no, crop, vs, chunks, emit=True)
    got = st['mean'][0].permute(3, 0, 1, 2).cpu().numpy()
    assert np.array_equal(got, c['mean']), f'{(got != c["mean"]).sum()} voxel-channels differ'
    assert np.array_equal(st['valid'][0].cpu().numpy().astype(bool), c['mean_valid'][0])
    assert np.array_equal(st['count'][0].cpu().numpy(), c['valid'].sum(0)[0])


@pytest.mark.parametrize('case,chunks', GOLDEN_CHUNKS, ids=[f'{k}-{"_".join(map(str, c))}' for k, c in GOLDEN_CHUNKS])
def test_no_emit_then_volume_mean(ia, case, chunks):
    """The same chunks with mean_out=None throughout, then ops.volume_mean: the reference's bits again; the outputs that were not
    passed keep their sentinels; volume_mean leaves sum and count as they are."""
    from imvoxelnet_amd import ops
    c, feat, P, no, crop, vs, nv = _golden(case)
    st = _state(1, nv, feat.shape[-1])
    _accumulate(ops, st, feat, P, no, crop, vs, chunks, emit=False)
    assert bool((st['mean'] == -7.0).all()) and bool((st['valid'] == 7).all())
    s0, c0 = st['sum'].clone(), st['count'].clone()
    mean, valid = ops.volume_mean(st['sum'], st['count'], torch.float32)
    assert torch.equal(st['sum'], s0) and torch.equal(st['count'], c0)
    assert np.array_equal(mean[0].permute(3, 0, 1, 2).cpu().numpy(), c['mean'])
    assert valid.dtype == torch.bool and np.array_equal(valid[0].cpu().numpy(), c['mean_valid'][0])
    assert np.array_equal(c0[0].cpu().numpy(), c['valid'].sum(0)[0])
    # into caller-owned buffers: the same bits
    ops.volume_mean(st['sum'], st['count'], torch.float32, out=st['mean'], valid_out=st['valid'])
    assert torch.equal(st['mean'], mean) and torch.equal(st['valid'].view(torch.bool), valid)


def _wide_case(C, dtype=torch.float32):
    """Case C's six cameras and grid for two samples (the second sees them in reverse order through a smaller crop), seeded features."""
    c, _, P, no, _, vs, nv = _golden('C')
    P = torch.cat([P, P.flip(1)]).contiguous()
    no = no.repeat(2, 1).contiguous()
    crop = torch.tensor([[24, 32], [13, 17]], dtype=torch.int32).cuda()
    feat = torch.randn(2 * 6, 1, 24, 32, C, generator=torch.Generator().manual_seed(100 + C)).to(dtype).cuda()
    return feat, P, no, crop, vs, nv


@pytest.mark.parametrize('C', [256, 512])
def test_wide_channels_and_batch_equal_one_shot(ia, C):
    """C = 256 (64 lanes per voxel) and C = 512 (two channel chunks per lane), B = 2 with different crops, chunks (2, 3, 1):
    torch.equal to ONE ops.backproject_mean over the six views; the count is ops.backproject_sum's."""
    from imvoxelnet_amd import ops
    feat, P, no, crop, vs, nv = _wide_case(C)
    ref, ref_valid = ops.backproject_mean(feat, P, no, crop, vs, nv)
    _, ref_count = ops.backproject_sum(feat, P, no, crop, vs, nv)
    st = _state(2, nv, C)
    _accumulate(ops, st, feat, P, no, crop, vs, (2, 3, 1), emit=True)
    assert torch.equal(st['mean'], ref) and torch.equal(st['valid'].view(torch.bool), ref_valid)
    assert torch.equal(st['count'], ref_count)
    assert not torch.equal(ref_valid[0], ref_valid[1]), 'the two samples must differ for the batch index to be tested'
    mean, valid = ops.volume_mean(st['sum'], st['count'], torch.float32)
    assert torch.equal(mean, ref) and torch.equal(valid, ref_valid)


def test_bf16_features_equal_one_shot(ia):
    """bf16 features at C = 256: fp32 running sum, bf16 mean with one rounding at the store == ops.backproject_mean on the bf16 input."""
    from imvoxelnet_amd import ops
    feat, P, no, crop, vs, nv = _wide_case(256, torch.bfloat16)
    ref, ref_valid = ops.backproject_mean(feat, P, no, crop, vs, nv)
    assert ref.dtype == torch.bfloat16
    st = _state(2, nv, 256, torch.bfloat16)
    _accumulate(ops, st, feat, P, no, crop, vs, (2, 3, 1), emit=True)
    assert st['sum'].dtype == torch.float32
    assert torch.equal(st['mean'], ref) and torch.equal(st['valid'].view(torch.bool), ref_valid)
    st2 = _state(2, nv, 256, torch.bfloat16)
    _accumulate(ops, st2, feat, P, no, crop, vs, (2, 3, 1), emit=False)
    mean, valid = ops.volume_mean(st2['sum'], st2['count'], torch.bfloat16)
    assert mean.dtype == torch.bfloat16 and torch.equal(mean, ref) and torch.equal(valid, ref_valid)
    assert torch.equal(st2['sum'], st['sum'])


# ------------------------------------------------------------------ the session
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


def _anchor_small(ia, V=2, hw=(96, 160)):
    """KITTI family (stack neck + Anchor3DHead) at the size of the smoke run, V slightly shifted cameras."""
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
    E = [np.array([[0, -1, 0, 0.3 * v], [0, 0, -1, 0.2], [1, 0, 0, 0.1], [0, 0, 0, 1]], np.float32) for v in range(V)]
    scene_meta = dict(img_shape=(hw[0], hw[1], 3), ori_shape=(hw[0] // 2, hw[1] // 2, 3), box_type_3d=ia.LiDARInstance3DBoxes,
                      lidar2img=dict(intrinsic=K, origin=np.array([ox, 0, -1.0], np.float32)))
    img = torch.randn(V, 3, *hw, generator=torch.Generator().manual_seed(2)).cuda()
    return model, scene_meta, E, img


def _full_meta(scene_meta, E):
    return dict(scene_meta, lidar2img=dict(scene_meta['lidar2img'], extrinsic=list(E)))


def _same_results(res, ref):
    assert len(res) == len(ref) == 1
    for a, b in zip(res, ref):
        assert torch.equal(a['scores_3d'], b['scores_3d']) and torch.equal(a['labels_3d'], b['labels_3d'])
        assert torch.equal(a['boxes_3d'].tensor, b['boxes_3d'].tensor) and type(a['boxes_3d']) is type(b['boxes_3d'])
        assert a['boxes_3d'].with_yaw == b['boxes_3d'].with_yaw


@pytest.fixture(scope='module')
def indoor(ia):
    model, scene_meta, E, img = _indoor_small(ia)
    model.prepare(torch.device('cuda'))
    meta = _full_meta(scene_meta, E)
    vol, valid = model.lift_cl(model.features_2d_cl(img[None]), [meta])
    return dict(model=model, scene_meta=scene_meta, E=E, img=img, meta=meta, vol=vol, valid=valid, ref=model.simple_test(img[None], [meta]))


@pytest.mark.parametrize('family', ['indoor', 'anchor'])
def test_session_all_views_equals_one_shot(ia, indoor, family):
    """add_views(all views) -> volume() is the one-shot lift of features_2d_cl, detect() is simple_test, bit for bit; detect() twice;
    again after reset(); two interleaved sessions on one model do not disturb each other."""
    if family == 'indoor':
        model, scene_meta, E, img, meta = (indoor[k] for k in ('model', 'scene_meta', 'E', 'img', 'meta'))
        vol, valid, ref = indoor['vol'], indoor['valid'], indoor['ref']
    else:
        model, scene_meta, E, img = _anchor_small(ia)
        model.prepare(torch.device('cuda'))
        meta = _full_meta(scene_meta, E)
        vol, valid = model.lift_cl(model.features_2d_cl(img[None]), [meta])
        ref = model.simple_test(img[None], [meta])
    assert model._native is not None, 'simple_test must run on the native handle here'
    print(family, 'detections', len(ref[0]['scores_3d']), 'valid voxels', int(valid.sum()), 'of', valid.numel())
    assert len(ref[0]['scores_3d']) > 0 and 0 < int(valid.sum()) < valid.numel()
    scene = model.open_scene(scene_meta)
    assert isinstance(scene, ia.SceneSession) and scene.n_views == 0
    for _ in range(2):                                       # the second pass runs after reset()
        scene.add_views(img, E)
        assert scene.n_views == len(E)
        v, ok = scene.volume()
        assert v.dtype == vol.dtype and torch.equal(v, vol) and torch.equal(ok, valid)
        _same_results(scene.detect(), ref)
        _same_results(scene.detect(), ref)
        scene.reset()
        assert scene.n_views == 0
    # two sessions, interleaved: `other` holds the views in reverse order (another scene), `scene` must not notice
    other = model.open_scene(scene_meta)
    scene.add_views(img[:1], E[:1])
    other.add_views(img.flip(0).contiguous(), E[::-1])
    scene.add_views(img[1:], E[1:], emit=False)
    ref_other = model.simple_test(img.flip(0)[None].contiguous(), [_full_meta(scene_meta, E[::-1])])
    _same_results(other.detect(), ref_other)
    assert torch.equal(scene.volume()[1], valid) and torch.equal(scene._count, other._count)
    alone = model.open_scene(scene_meta)                     # the same (1, 3) adds with no other session in between
    alone.add_views(img[:1], E[:1]).add_views(img[1:], E[1:])
    assert torch.equal(scene.volume()[0], alone.volume()[0]) and torch.equal(scene._sum, alone._sum), "`other`'s add touched `scene`'s sum"
    alone.close()
    scene.close()
    with pytest.raises(RuntimeError):
        scene.detect()
    other.close()


def _chunked_vs_one_shot(model, scene_meta, E, img, chunks=(1, 2, 1)):
    """Views added in `chunks` against the one-shot lift.  Asserted here, whatever the trunk's mode: mask and count are the one-shot
    lift's; the session's volume is bit for bit ONE ops.backproject_mean over the features the trunk gave chunk by chunk (the order
    of the views inside and across the chunks, the carried sum); and where those features are the one-shot run's bits, so is the volume."""
    from imvoxelnet_amd import ops
    meta = _full_meta(scene_meta, E)
    p0 = model.features_2d_cl(img[None])
    vol, valid = model.lift_cl(p0, [meta])
    proj, no, crop = model._camera_setup([meta], 4, img.device)
    _, count = ops.backproject_sum(p0, proj, no, crop, model.voxel_size, model.n_voxels)
    scene = model.open_scene(scene_meta)
    v0, per_chunk = 0, []
    for n in chunks:
        scene.add_views(img[v0:v0 + n], E[v0:v0 + n])
        per_chunk.append(scene._features(img[v0:v0 + n].contiguous()).clone())
        v0 += n
    pc = torch.cat(per_chunk).contiguous()
    feats_equal = torch.equal(pc, p0)
    got, ok = scene.volume()
    assert scene.n_views == len(E)
    assert torch.equal(ok, valid) and torch.equal(scene._count, count)
    vol_pc, valid_pc = ops.backproject_mean(pc, proj, no, crop, model.voxel_size, model.n_voxels)
    assert torch.equal(got, vol_pc) and torch.equal(ok, valid_pc), 'the session is not the one-shot lift of the features it was given'
    vol_equal = torch.equal(got, vol)
    assert vol_equal or not feats_equal
    d, scale = float((got.float() - vol.float()).abs().max()), float(vol.float().abs().max())
    scene.close()
    return d, scale, feats_equal, vol_equal


def test_session_chunked_within_volume_bar(ia, indoor):
    """Views added (1, 2, 1): mask and count are exactly the one-shot lift's (geometry does not depend on the features); the volume is
    bit for bit the one-shot lift of the features the trunk produced chunk by chunk, and equal to the one-shot run wherever those
    features are (_chunked_vs_one_shot).  Against the one-shot run of all four views the mean volume is within the bar of the
    full-size parity tests, atol = 2e-4 * max|ref|, rtol = 0: with the default fp16-pair trunk the per-tensor operand scales depend on
    which views share a call, so the features of a view need not be the one-shot run's bits.  No claim on kept boxes.  The figures
    (max |d|, its ratio to max|ref|, whether features and volume came out bit-equal) are printed before the bar is asserted."""
    d, scale, feats_equal, vol_equal = _chunked_vs_one_shot(indoor['model'], indoor['scene_meta'], indoor['E'], indoor['img'])
    print(f'chunked (1,2,1), fp16-pair trunk: max|d| {d:.3e} max|ref| {scale:.3e} ratio {d / scale:.3e} per-view features bit-equal {feats_equal} '
          f'volume bit-equal {vol_equal}')
    assert d <= 2e-4 * scale


def test_session_chunked_fp32_operand_trunk(ia):
    """The same with the trunk on fp32 MFMA operands (FusedConv.trunk_operands = 0): no per-tensor operand scale couples the views of a
    call, but the layer plans (tile, split-K, Winograd form) may still depend on the number of views.  The same rules: the exact ones of
    _chunked_vs_one_shot -- equality with the one-shot volume wherever the per-view features are bit-equal -- and the 2e-4 bar."""
    from imvoxelnet_amd.conv import FusedConv
    keep = FusedConv.trunk_operands
    FusedConv.trunk_operands = 0
    try:
        model, scene_meta, E, img = _indoor_small(ia)
        model.prepare(torch.device('cuda'))
        d, scale, feats_equal, vol_equal = _chunked_vs_one_shot(model, scene_meta, E, img)
    finally:
        FusedConv.trunk_operands = keep
    print(f'chunked (1,2,1), fp32-operand trunk: max|d| {d:.3e} max|ref| {scale:.3e} ratio {d / scale:.3e} per-view features bit-equal {feats_equal} '
          f'volume bit-equal {vol_equal}')
    assert d <= 2e-4 * scale


def test_add_views_u8_equals_add_views(ia, indoor):
    """Two uint8 frames through add_views_u8 == add_views on prepare_images_device's output (volume() bit for bit); the session's meta
    receives the shapes the pipeline produced."""
    from imvoxelnet_amd.data import prepare_images_device
    model, E = indoor['model'], indoor['E'][:2]
    rng = np.random.default_rng(70)
    frames = [rng.integers(0, 256, (190, 256, 3), dtype=np.uint8) for _ in range(2)]       # -> 95 x 128 in a 96 x 128 plane
    user = {k: v for k, v in indoor['scene_meta'].items() if k not in ('img_shape', 'ori_shape', 'pad_shape')}
    img, shapes = prepare_images_device([frames], (128, 96))
    assert img.shape == (1, 2, 3, 96, 128)
    a = model.open_scene(dict(user, **shapes[0]))
    a.add_views(img[0], E)
    b = model.open_scene(user)
    b.add_views_u8(frames, E, (128, 96))
    assert all(tuple(b.meta[k]) == tuple(shapes[0][k]) for k in ('img_shape', 'ori_shape', 'pad_shape')) and 'img_shape' not in user
    (va, oa), (vb, ob) = a.volume(), b.volume()
    assert torch.equal(va, vb) and torch.equal(oa, ob) and 0 < int(oa.sum())
    _same_results(b.detect(), a.detect())
