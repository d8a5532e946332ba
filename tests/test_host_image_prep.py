"""CPU-only tests of the device-side image pipeline's host surface (include/imvoxel.h ivx_rescale_size / ivx_image_prep_u8, csrc/image_prep.hip,
data.prepare_images_device): the size rule against data.rescale_size, argument validation before any launch, the ctypes layout, and the
batching logic of prepare_images_device with ops.image_prep_u8 replaced by a host stand-in built from data.prepare_image.  The library loads
without a device; nothing here launches a kernel."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from helpers import ROOT

# source (h, w) and img_scale of the four reference test pipelines
GEOMETRIES = {'kitti': ((375, 1242), (1280, 384)), 'nuscenes': ((900, 1600), (1600, 900)), 'scannet': ((968, 1296), (640, 480)),
              'sunrgbd': ((530, 730), (640, 480))}


def _rescale(L, h, w, a, b):
    dh, dw = C.c_int32(-1), C.c_int32(-1)
    assert L.ivx_rescale_size(h, w, a, b, C.byref(dh), C.byref(dw)) == 0, L.ivx_last_error()
    return dh.value, dw.value


def test_rescale_size_equals_data_rescale_size():
    from imvoxelnet_amd import _lib, data
    L = _lib.lib()
    cases = []
    for (h, w), (a, b) in GEOMETRIES.values():
        cases += [(h, w, a, b), (h, w, b, a), (w, h, a, b), (w, h, b, a)]          # both orders of the scale tuple, portrait frames
    cases += [(1, 1, 1, 1), (1, 4000, 640, 480), (4000, 1, 640, 480), (3, 5, 32768, 32768), (480, 640, 640, 480), (1080, 1920, 1333, 800)]
    rng = np.random.RandomState(20240)
    for _ in range(400):
        h, w = (int(v) for v in rng.randint(1, 4097, 2))
        a, b = (int(v) for v in rng.randint(1, 2049, 2))
        cases.append((h, w, a, b))
    for h, w, a, b in cases:
        assert _rescale(L, h, w, a, b) == data.rescale_size((h, w), (a, b)), (h, w, a, b)
    assert _rescale(L, 375, 1242, 1280, 384) == (384, 1272)                        # KITTI up-scales
    assert _rescale(L, 900, 1600, 1600, 900) == (900, 1600)
    assert _rescale(L, 968, 1296, 640, 480) == (478, 640)
    d = C.c_int32()
    assert L.ivx_rescale_size(0, 10, 640, 480, C.byref(d), C.byref(d)) == -1 and b'positive' in L.ivx_last_error()
    assert L.ivx_rescale_size(10, 10, 640, 0, C.byref(d), C.byref(d)) == -1 and b'positive' in L.ivx_last_error()
    assert L.ivx_rescale_size(10, 10, 640, 480, None, C.byref(d)) == -1 and b'null' in L.ivx_last_error()


def _desc(**kw):
    from imvoxelnet_amd import _lib
    v = dict(src_h=375, src_w=1242, src_row_bytes=3 * 1242, dst_h=384, dst_w=1272, pad_h=384, pad_w=1280, to_rgb=1)
    mean, std = kw.pop('mean', (123.675, 116.28, 103.53)), kw.pop('std', (58.395, 57.12, 57.375))
    v.update(kw)
    return _lib.ImagePrepDesc(mean=(C.c_float * 3)(*mean), std=(C.c_float * 3)(*std), **v)


def test_image_prep_argument_validation_without_gpu():
    """Every bad argument is rejected with status -1 and a message that names it, before any launch (dummy non-null pointers)."""
    from imvoxelnet_amd import _lib
    L = _lib.lib()
    dummy = C.c_void_p(64)
    img_bytes = 375 * 3 * 1242

    def call(d, src=dummy, sib=img_bytes, n=1, out=dummy):
        rc = L.ivx_image_prep_u8(C.byref(d) if d is not None else None, src, sib, n, out, None)
        return rc, L.ivx_last_error()

    for args in (dict(d=None), dict(d=_desc(), src=None), dict(d=_desc(), out=None)):
        rc, msg = call(**args)
        assert rc == -1 and b'null' in msg, (args, msg)
    for field in ('src_h', 'src_w', 'dst_h', 'dst_w'):
        for bad in (0, -3):
            rc, msg = call(_desc(**{field: bad}))
            assert rc == -1 and b'positive' in msg and str(bad).encode() in msg, (field, msg)
    rc, msg = call(_desc(pad_h=383))
    assert rc == -1 and b'pad 383 x 1280' in msg and b'dst 384 x 1272' in msg
    rc, msg = call(_desc(pad_w=1271))
    assert rc == -1 and b'pad 384 x 1271' in msg
    rc, msg = call(_desc(src_row_bytes=3 * 1242 - 1))
    assert rc == -1 and b'src_row_bytes 3725' in msg and b'3726' in msg
    for c in range(3):
        for bad in (0.0, float('inf'), float('nan'), -float('inf')):
            std = [58.395, 57.12, 57.375]
            std[c] = bad
            rc, msg = call(_desc(std=std))
            assert rc == -1 and f'std[{c}]'.encode() in msg, (c, bad, msg)
    for bad in (0, -1):
        rc, msg = call(_desc(), n=bad)
        assert rc == -1 and f'n = {bad}'.encode() in msg
    rc, msg = call(_desc(), n=2, sib=img_bytes - 1)
    assert rc == -1 and b'src_image_bytes' in msg and str(img_bytes - 1).encode() in msg
    # the limit of the index arithmetic the header states
    header = open(os.path.join(ROOT, 'include', 'imvoxel.h')).read()
    limit = int(re.search(r'#define IVX_IMAGE_PREP_MAX_DIM (\d+)', header).group(1))
    for field in ('src_h', 'src_w', 'pad_h', 'pad_w'):
        kw = {field: limit + 1}
        if field == 'src_w':
            kw['src_row_bytes'] = 3 * (limit + 1)
        rc, msg = call(_desc(**kw))
        assert rc == -1 and str(limit).encode() in msg and b'not supported' in msg, (field, msg)
    rc, msg = call(_desc(), n=(1 << 20) + 1, sib=img_bytes)
    assert rc == -1 and b'n = 1048577' in msg
    with pytest.raises(ValueError, match='pad 383'):
        _lib.check(call(_desc(pad_h=383))[0], 'ivx_image_prep_u8')


def test_image_prep_binding_matches_the_header():
    from imvoxelnet_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'imvoxel.h')).read()
    body = re.search(r'typedef struct ivx_image_prep_desc \{(.*?)\} ivx_image_prep_desc;', header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    n_fields = 0
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        assert decl.startswith(('int32_t ', 'float ')), decl
        for name in decl.split(' ', 1)[1].split(','):
            m = re.fullmatch(r'\s*\w+\s*(?:\[(\d+)\])?\s*', name)
            n_fields += int(m.group(1) or 1)
    assert n_fields == 14 and C.sizeof(_lib.ImagePrepDesc) == n_fields * 4
    assert [f[0] for f in _lib.ImagePrepDesc._fields_] == re.findall(r'(?:int32_t|float|,)\s*(\w+)(?=\s*[,;\[])', body)
    for name in ('ivx_rescale_size', 'ivx_image_prep_u8'):
        assert name in _lib.EXPORTS and re.search(r'\bint ' + name + r'\(', header) and hasattr(_lib.lib(), name)
    assert _lib.lib().ivx_version() >= 430
    import imvoxelnet_amd as ia
    assert ia.prepare_images_device is ia.data.prepare_images_device and ia.image_prep_u8 is ia.ops.image_prep_u8
    assert callable(ia.ImVoxelNet.simple_test_u8)


def test_ops_image_prep_u8_fails_loudly_on_host_tensors():
    from imvoxelnet_amd import ops
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.image_prep_u8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), (4, 4), (32, 32), (0, 0, 0), (1, 1, 1))


# ------------------------------------------------------------------ prepare_images_device with a host stand-in of the kernel
def _frame(rng, h, w):
    return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)


@pytest.fixture
def host_kernel(monkeypatch):
    """ops.image_prep_u8 served by data.prepare_image (keep_ratio=False at the requested size) + zero padding to the requested plane; records
    every call as (n, source shape, size_hw, pad_hw)."""
    from imvoxelnet_amd import data, ops
    calls = []

    def stand_in(src, size_hw, pad_hw, mean, std, to_rgb=True, out=None):
        assert isinstance(src, torch.Tensor) and src.dtype == torch.uint8 and src.dim() == 4 and src.shape[3] == 3
        n = src.shape[0]
        calls.append((n, tuple(src.shape[1:3]), tuple(size_hw), tuple(pad_hw)))
        res = torch.full((n, 3, pad_hw[0], pad_hw[1]), float('nan')) if out is None else out
        assert tuple(res.shape) == (n, 3, pad_hw[0], pad_hw[1]) and res.is_contiguous()
        for i in range(n):
            t, _ = data.prepare_image(src[i].numpy(), (size_hw[1], size_hw[0]), dict(mean=mean, std=std, to_rgb=to_rgb), size_divisor=1, keep_ratio=False)
            res[i] = 0
            res[i, :, :t.shape[1], :t.shape[2]] = t
        return res
    monkeypatch.setattr(ops, 'image_prep_u8', stand_in)
    return calls


def _expected(frames, img_scale, plane, **kw):
    from imvoxelnet_amd import data
    out = torch.zeros(len(frames), 3, *plane)
    metas = []
    for i, f in enumerate(frames):
        t, m = data.prepare_image(f, img_scale, **kw)
        out[i, :, :t.shape[1], :t.shape[2]] = t
        metas.append(m)
    return out, metas


def test_prepare_images_device_mixed_kitti_sizes(host_kernel):
    """375 x 1242 and 370 x 1224 frames in one batch: one stacked group per source shape, one common pad plane, per-sample dicts as prepare_image's."""
    from imvoxelnet_amd import data
    rng = np.random.RandomState(3)
    frames = [_frame(rng, 375, 1242), _frame(rng, 375, 1242), _frame(rng, 370, 1224), _frame(rng, 370, 1224), _frame(rng, 370, 1224)]
    img, metas = data.prepare_images_device(frames, (1280, 384), device='cpu')
    assert data.rescale_size((370, 1224), (1280, 384)) == (384, 1270)
    assert img.shape == (5, 3, 384, 1280) and img.dtype == torch.float32
    ref, ref_metas = _expected(frames, (1280, 384), (384, 1280))
    assert torch.equal(img, ref) and metas == ref_metas
    assert metas[0] == dict(img_shape=(384, 1272, 3), ori_shape=(375, 1242, 3), pad_shape=(384, 1280, 3))
    assert sorted(host_kernel) == sorted([(2, (375, 1242), (384, 1272), (384, 1280)), (3, (370, 1224), (384, 1270), (384, 1280))])
    # a batch whose pad shapes differ: every image lies in the largest plane, its own pad_shape stays in its dict
    del host_kernel[:]
    frames = [_frame(rng, 100, 160), _frame(rng, 60, 200)]
    img, metas = data.prepare_images_device(frames, (200, 120), device='cpu')
    assert [m['pad_shape'] for m in metas] == [(128, 192, 3), (64, 224, 3)] and img.shape == (2, 3, 128, 224)
    ref, ref_metas = _expected(frames, (200, 120), (128, 224))
    assert torch.equal(img, ref) and metas == ref_metas
    assert sorted(host_kernel) == [(1, (60, 200), (60, 200), (128, 224)), (1, (100, 160), (120, 192), (128, 224))]
    # frames of one shape that are not adjacent: still ONE stacked group (one host-to-device copy), a launch per run of adjacent frames
    del host_kernel[:]
    a, b, c = _frame(rng, 40, 64), _frame(rng, 32, 64), _frame(rng, 40, 64)
    img, metas = data.prepare_images_device([a, b, c], (64, 64), device='cpu', keep_ratio=False, size_divisor=16)
    ref, ref_metas = _expected([a, b, c], (64, 64), (64, 64), keep_ratio=False, size_divisor=16)
    assert torch.equal(img, ref) and metas == ref_metas and len(host_kernel) == 3


def test_prepare_images_device_input_forms(host_kernel):
    """A stacked [N,H,W,3] array or tensor is one group and one launch; a [B][V] input returns [B,V,3,Hp,Wp] and the dict of the LAST view."""
    from imvoxelnet_amd import data
    rng = np.random.RandomState(4)
    batch = rng.randint(0, 256, (4, 53, 73, 3)).astype(np.uint8)
    ref, ref_metas = _expected(list(batch), (64, 48), (64, 64))
    for form in (batch, torch.from_numpy(batch), list(batch), [torch.from_numpy(f) for f in batch]):
        del host_kernel[:]
        img, metas = data.prepare_images_device(form, (64, 48), device='cpu')
        assert torch.equal(img, ref) and metas == ref_metas
        assert host_kernel == [(4, (53, 73), (46, 64), (64, 64))]
    # [2][3] multi-view: the last view of sample 1 has another size, and its dict is the sample's
    views = [[_frame(rng, 53, 73), _frame(rng, 53, 73), _frame(rng, 53, 73)], [_frame(rng, 53, 73), _frame(rng, 53, 73), _frame(rng, 60, 60)]]
    del host_kernel[:]
    img, metas = data.prepare_images_device(views, (64, 48), device='cpu')
    flat = [f for s in views for f in s]
    ref, ref_metas = _expected(flat, (64, 48), (64, 64))
    assert img.shape == (2, 3, 3, 64, 64) and torch.equal(img, ref.view(2, 3, 3, 64, 64))
    assert metas == [ref_metas[2], ref_metas[5]] and metas[1]['ori_shape'] == (60, 60, 3) and metas[1]['img_shape'] == (48, 48, 3)
    assert sorted(host_kernel) == [(1, (60, 60), (48, 48), (64, 64)), (5, (53, 73), (46, 64), (64, 64))]
    with pytest.raises(ValueError):
        data.prepare_images_device([[flat[0]], [flat[1], flat[2]]], (64, 48), device='cpu')
    with pytest.raises(TypeError):
        data.prepare_images_device([flat[0].astype(np.float32)], (64, 48), device='cpu')


def test_simple_test_u8_fills_the_shape_keys(host_kernel, monkeypatch):
    """simple_test_u8 copies every meta, fills the three shape keys from the pipeline and hands a [B,V,3,Hp,Wp] tensor to simple_test."""
    import imvoxelnet_amd as ia
    from imvoxelnet_amd.workloads import kitti_model_cfg, KITTI_TEST_CFG
    model = ia.build_detector(kitti_model_cfg(n_voxels=(24, 28, 12), in_ch=16, out_ch=32), test_cfg=KITTI_TEST_CFG)
    seen = {}
    monkeypatch.setattr(model, 'simple_test', lambda img, metas: seen.update(img=img, metas=metas) or 'results')
    rng = np.random.RandomState(5)
    frames = [_frame(rng, 48, 160), _frame(rng, 48, 160)]
    user = [dict(lidar2img='L0', box_type_3d='T', img_shape='stale'), dict(lidar2img='L1', box_type_3d='T')]
    assert model.simple_test_u8(frames, user, (320, 96), device='cpu') == 'results'
    ref, ref_metas = _expected(frames, (320, 96), (96, 320))
    assert seen['img'].shape == (2, 1, 3, 96, 320) and torch.equal(seen['img'][:, 0], ref)
    assert seen['metas'] == [dict(lidar2img='L0', box_type_3d='T', **ref_metas[0]), dict(lidar2img='L1', box_type_3d='T', **ref_metas[1])]
    assert user[0]['img_shape'] == 'stale' and 'pad_shape' not in user[1]                # the caller's dicts are not written to
    with pytest.raises(ValueError):
        model.simple_test_u8(frames, user[:1], (320, 96), device='cpu')
