"""CPU-only tests of the lens-aware image pipeline's host surface (include/imvoxel.h ivx_lens / ivx_image_prep_lens_u8 / ivx_map_prep_lens,
csrc/image_prep.hip, data.Lens, data.prepare_images_device(lens=), the lens= / depth_frames= keywords of the scenes): argument validation before
any launch, the ctypes layout against the header text, the Lens record, the grouping and the launches of prepare_images_device with the ops
replaced by stand-ins built from tests/ref_lens.py, the scene logic with stubbed ops, and the sanity of the fp64 reference itself against
data.prepare_image.  The library loads without a device; nothing here launches a kernel."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import ref_lens as R
from helpers import ROOT

INF = float('inf')
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


def to_lens(L):
    """A ref_lens dict as a data.Lens."""
    from imvoxelnet_amd import data
    K = [[L['fx'], 0, L['cx']], [0, L['fy'], L['cy']], [0, 0, 1]]
    new_K = [[L['nfx'], 0, L['ncx']], [0, L['nfy'], L['ncy']], [0, 0, 1]]
    return data.Lens(L['model'], K, L['coef'] if L['model'] == 'brown' else L['coef'][:4], new_K, L['r2_max'])


def from_lens(lens):
    """A data.Lens as a ref_lens dict (for the stand-ins)."""
    (fx, fy, cx, cy), (nfx, nfy, ncx, ncy) = lens.key[1], lens.key[3]
    return R.lens(lens.model, fx, fy, cx, cy, list(lens.coef), new=(nfx, nfy, ncx, ncy), r2_max=lens.r2_max)


# ------------------------------------------------------------------ the C entries without a device
def _desc(**kw):
    from imvoxelnet_amd import _lib
    v = dict(src_h=37, src_w=53, src_row_bytes=3 * 53, dst_h=23, dst_w=31, pad_h=32, pad_w=32, to_rgb=1)
    mean, std = kw.pop('mean', MEAN), kw.pop('std', STD)
    v.update(kw)
    return _lib.ImagePrepDesc(mean=(C.c_float * 3)(*mean), std=(C.c_float * 3)(*std), **v)


def _lens(**kw):
    from imvoxelnet_amd import _lib
    v = dict(model=0, fx=40.0, fy=41.0, cx=26.0, cy=18.0, new_fx=38.0, new_fy=39.0, new_cx=26.5, new_cy=18.5, r2_max=INF)
    coef = kw.pop('coef', (-0.1, 0.01, 0.001, -0.001, 0.0))
    v.update(kw)
    return _lib.Lens(coef=(C.c_double * 5)(*coef), **v)


BAD_LENSES = [(dict(model=2), b'unknown lens model 2'), (dict(model=-1), b'unknown lens model -1')] + \
    [(dict(**{f: bad}), b'focal lengths') for f in ('fx', 'fy', 'new_fx', 'new_fy') for bad in (0.0, INF, float('nan'))] + \
    [(dict(**{f: bad}), b'principal points') for f in ('cx', 'cy', 'new_cx', 'new_cy') for bad in (INF, float('nan'))] + \
    [(dict(coef=tuple(bad if j == i else 0.0 for j in range(5))), f'coef[{i}]'.encode()) for i in range(5) for bad in (INF, float('nan'))] + \
    [(dict(r2_max=bad), b'r2_max') for bad in (0.0, -1.0, -INF, float('nan'))]


def test_image_entry_argument_validation_without_gpu():
    """Every bad argument is rejected with status -1 and a message that names it, before any launch (dummy non-null pointers)."""
    from imvoxelnet_amd import _lib
    L = _lib.lib()
    dummy, img_bytes = C.c_void_p(64), 37 * 3 * 53

    def call(d, lens='ok', src=dummy, sib=img_bytes, n=1, out=dummy):
        lens = _lens() if lens == 'ok' else lens
        rc = L.ivx_image_prep_lens_u8(C.byref(d) if d is not None else None, C.byref(lens) if lens is not None else None, src, sib, n, out, None)
        return rc, L.ivx_last_error()

    for args in (dict(d=None), dict(d=_desc(), lens=None), dict(d=_desc(), src=None), dict(d=_desc(), out=None)):
        rc, msg = call(**args)
        assert rc == -1 and b'null' in msg, (args, msg)
    for field in ('src_h', 'src_w', 'dst_h', 'dst_w'):
        for bad in (0, -3):
            rc, msg = call(_desc(**{field: bad}))
            assert rc == -1 and b'ivx_image_prep_lens_u8' in msg and b'positive' in msg and str(bad).encode() in msg, (field, msg)
    rc, msg = call(_desc(pad_h=22))
    assert rc == -1 and b'pad 22 x 32' in msg and b'dst 23 x 31' in msg
    rc, msg = call(_desc(src_row_bytes=3 * 53 - 1))
    assert rc == -1 and b'src_row_bytes 158' in msg and b'159' in msg
    for c in range(3):
        for bad in (0.0, INF, float('nan')):
            std = list(STD)
            std[c] = bad
            rc, msg = call(_desc(std=std))
            assert rc == -1 and f'std[{c}]'.encode() in msg, (c, bad, msg)
    for bad in (0, -1, (1 << 20) + 1):
        rc, msg = call(_desc(), n=bad)
        assert rc == -1 and f'n = {bad}'.encode() in msg
    rc, msg = call(_desc(), n=2, sib=img_bytes - 1)
    assert rc == -1 and b'src_image_bytes' in msg and str(img_bytes - 1).encode() in msg
    header = open(os.path.join(ROOT, 'include', 'imvoxel.h')).read()
    limit = int(re.search(r'#define IVX_IMAGE_PREP_MAX_DIM (\d+)', header).group(1))
    for field in ('src_h', 'src_w', 'pad_h', 'pad_w'):
        kw = {field: limit + 1}
        if field == 'src_w':
            kw['src_row_bytes'] = 3 * (limit + 1)
        rc, msg = call(_desc(**kw))
        assert rc == -1 and str(limit).encode() in msg and b'not supported' in msg, (field, msg)
    for kw, needle in BAD_LENSES:
        rc, msg = call(_desc(), lens=_lens(**kw))
        assert rc == -1 and b'ivx_image_prep_lens_u8' in msg and needle in msg, (kw, msg)
    with pytest.raises(ValueError, match='r2_max'):
        _lib.check(call(_desc(), lens=_lens(r2_max=0.0))[0], 'ivx_image_prep_lens_u8')


def test_map_entry_argument_validation_without_gpu():
    from imvoxelnet_amd import _lib
    L = _lib.lib()
    dummy = C.c_void_p(64)

    def call(d, lens=None, src=None, dt=0, row=4 * 53, plane=4 * 53 * 37, scale=1.0, stride=4, n=1, out=dummy):
        rc = L.ivx_map_prep_lens(C.byref(d) if d is not None else None, C.byref(lens) if lens is not None else None, src, dt, row, plane, scale, stride, n,
                                 out, None)
        return rc, L.ivx_last_error()

    for args in (dict(d=None), dict(d=_desc(), out=None)):
        rc, msg = call(**args)
        assert rc == -1 and b'null' in msg, (args, msg)
    for field in ('src_h', 'src_w', 'dst_h', 'dst_w'):
        rc, msg = call(_desc(**{field: 0}))
        assert rc == -1 and b'ivx_map_prep_lens' in msg and b'positive' in msg, (field, msg)
    rc, msg = call(_desc(pad_w=30))
    assert rc == -1 and b'pad 32 x 30' in msg
    for bad in (0, -4):
        rc, msg = call(_desc(), stride=bad)
        assert rc == -1 and f'stride = {bad}'.encode() in msg
    for bad in (0, -1):
        rc, msg = call(_desc(), n=bad)
        assert rc == -1 and f'n = {bad}'.encode() in msg
    for kw, needle in BAD_LENSES:
        rc, msg = call(_desc(), lens=_lens(**kw))
        assert rc == -1 and b'ivx_map_prep_lens' in msg and needle in msg, (kw, msg)
    # with a source map: the element type, the strides, the alignment, the scale
    for bad in (2, -1):
        rc, msg = call(_desc(), src=dummy, dt=bad)
        assert rc == -1 and f'unknown src_dtype {bad}'.encode() in msg
    rc, msg = call(_desc(), src=dummy, dt=0, row=4 * 53 - 4)
    assert rc == -1 and b'src_row_bytes 208' in msg and b'212' in msg
    rc, msg = call(_desc(), src=dummy, dt=0, row=4 * 53 + 2)
    assert rc == -1 and b'src_row_bytes 214' in msg and b'multiple of 4' in msg
    rc, msg = call(_desc(), src=dummy, dt=1, row=2 * 53 - 2)
    assert rc == -1 and b'src_row_bytes 104' in msg and b'106' in msg
    rc, msg = call(_desc(), src=C.c_void_p(66), dt=0)
    assert rc == -1 and b'not aligned' in msg
    rc, msg = call(_desc(), src=dummy, dt=0, n=2, plane=4 * 53 * 37 - 4)
    assert rc == -1 and b'src_map_bytes' in msg and str(4 * 53 * 37 - 4).encode() in msg
    for bad in (INF, float('nan')):
        rc, msg = call(_desc(), src=dummy, dt=1, row=2 * 53, scale=bad)
        assert rc == -1 and b'scale' in msg
    # the fields of the descriptor the map entry does not read are not judged: no row pitch of a uint8 image, no std
    rc, msg = call(_desc(src_row_bytes=0, std=(0.0, 0.0, 0.0), pad_h=22))
    assert rc == -1 and b'pad 22 x 32' in msg


def test_binding_matches_the_header():
    from imvoxelnet_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'imvoxel.h')).read()
    body = re.search(r'typedef struct ivx_lens \{(.*?)\} ivx_lens;', header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(' ', 1)
        assert ctype in ('int32_t', 'double'), decl
        for name in names.split(','):
            m = re.fullmatch(r'\s*(\w+)\s*(?:\[(\d+)\])?\s*', name)
            fields.append((m.group(1), ctype, int(m.group(2) or 1)))
    assert [f[0] for f in fields] == [f[0] for f in _lib.Lens._fields_] == ['model', 'fx', 'fy', 'cx', 'cy', 'coef', 'new_fx', 'new_fy', 'new_cx', 'new_cy', 'r2_max']
    for (name, ctype, count), (_, ct) in zip(fields, _lib.Lens._fields_):
        assert C.sizeof(ct) == count * (4 if ctype == 'int32_t' else 8), name
    assert C.sizeof(_lib.Lens) == 8 + 8 * sum(f[2] for f in fields[1:]) == 120 and _lib.Lens.fx.offset == 8        # the int32 is padded to the doubles
    for name, value in (('IVX_LENS_BROWN', _lib.LENS_BROWN), ('IVX_LENS_FISHEYE', _lib.LENS_FISHEYE), ('IVX_MAP_F32', _lib.MAP_F32), ('IVX_MAP_U16', _lib.MAP_U16)):
        assert int(re.search(r'#define ' + name + r' (\d+)', header).group(1)) == value
    L = _lib.lib()
    for name, n_args in (('ivx_image_prep_lens_u8', 7), ('ivx_map_prep_lens', 11)):
        decl = re.search(r'\bint ' + name + r'\((.*?)\);', header, re.S).group(1)
        assert name in _lib.EXPORTS and hasattr(L, name) and len(getattr(L, name).argtypes) == n_args == decl.count(',') + 1
    assert L.ivx_version() >= 502
    import imvoxelnet_amd as ia
    assert ia.image_prep_lens_u8 is ia.ops.image_prep_lens_u8 and ia.map_prep_lens is ia.ops.map_prep_lens and ia.Lens is ia.data.Lens


def test_ops_refuse_host_tensors_and_an_older_library(monkeypatch):
    from imvoxelnet_amd import _lib, ops
    lens = to_lens(R.case_lens('tangential', (4, 4)))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.image_prep_lens_u8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), lens, (4, 4), (32, 32), (0, 0, 0), (1, 1, 1))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.map_prep_lens((4, 4), (32, 32), (4, 4), lens, src=torch.zeros(1, 4, 4))
    with pytest.raises(TypeError, match='data.Lens'):
        ops.image_prep_lens_u8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), dict(k1=0), (4, 4), (32, 32), (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match='stride'):
        ops.map_prep_lens((4, 4), (32, 32), (4, 4), lens, stride=0)
    old = types.SimpleNamespace(ivx_version=lambda: 501)              # a build of the ABI from before 0.5.2: it loads, the ops refuse
    monkeypatch.setattr(_lib, 'lib', lambda: old)
    for call in (lambda: ops.image_prep_lens_u8(None, lens, (4, 4), (32, 32), (0, 0, 0), (1, 1, 1)), lambda: ops.map_prep_lens((4, 4), (32, 32), (4, 4))):
        with pytest.raises(_lib.IvxError, match='0.5.2'):
            call()


# ------------------------------------------------------------------ data.Lens
def test_lens_record():
    from imvoxelnet_amd import data, _lib
    K = np.array([[40., 0, 26, 0], [0, 41., 18, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)          # a 4x4 meta intrinsic is taken by its 3x3
    a = data.Lens('brown', K, [-0.1, 0.01, 0.001, -0.001])
    b = data.Lens('brown', K[:3, :3].astype(np.float64), (-0.1, 0.01, 0.001, -0.001, 0.0), new_K=K, r2_max=INF)
    assert a == b and hash(a) == hash(b) and a.key == b.key and {a: 1}[b] == 1 and a.coef == (-0.1, 0.01, 0.001, -0.001, 0.0)
    assert np.array_equal(a.new_K, a.K) and a.K.shape == (3, 3) and a.K[0, 0] == 40 and a.K[1, 2] == 18 and a.model == 'brown' and a.r2_max == INF
    c = data.Lens('fisheye', K, [0.1, 0.0, 0.0, 0.0], new_K=[[30, 0, 26], [0, 31, 18], [0, 0, 1]], r2_max=2.5)
    assert c != a and c.key != a.key and c.new_K[0, 0] == 30 and c.r2_max == 2.5
    s = c.struct()
    assert isinstance(s, _lib.Lens) and s.model == _lib.LENS_FISHEYE and (s.fx, s.fy, s.cx, s.cy) == (40.0, 41.0, 26.0, 18.0)
    assert list(s.coef) == [0.1, 0.0, 0.0, 0.0, 0.0] and (s.new_fx, s.new_fy, s.new_cx, s.new_cy, s.r2_max) == (30.0, 31.0, 26.0, 18.0, 2.5)
    assert a.struct().model == _lib.LENS_BROWN and a.struct().r2_max == INF
    for bad in (dict(model='pinhole'), dict(K=np.eye(2)), dict(K=[[0, 0, 1], [0, 1, 1], [0, 0, 1]]), dict(K=[[1, 0.1, 1], [0, 1, 1], [0, 0, 1]]),
                dict(K=[[float('nan'), 0, 1], [0, 1, 1], [0, 0, 1]]), dict(coef=[0.1] * 3), dict(coef=[0.1] * 6), dict(coef=[0.1, INF, 0, 0]),
                dict(new_K=[[1, 0, 1], [0, 0, 1], [0, 0, 1]]), dict(r2_max=0), dict(r2_max=-1), dict(r2_max=float('nan'))):
        kw = dict(dict(model='brown', K=K, coef=[0.0] * 5), **bad)
        with pytest.raises(ValueError):
            data.Lens(**kw)
    with pytest.raises(ValueError, match='4 coefficients'):
        data.Lens('fisheye', K, [0.0] * 5)


# ------------------------------------------------------------------ prepare_images_device with host stand-ins of both kernels
@pytest.fixture
def host_kernels(monkeypatch):
    """ops.image_prep_u8 served by data.prepare_image and ops.image_prep_lens_u8 by ref_lens.image (rounded to fp32); every call is recorded as
    (name, n, source shape, size_hw, pad_hw[, lens])."""
    from imvoxelnet_amd import data, ops
    calls = []

    def write(name, src, size_hw, pad_hw, out, one):
        assert isinstance(src, torch.Tensor) and src.dtype == torch.uint8 and src.dim() == 4 and src.shape[3] == 3
        n = src.shape[0]
        res = torch.full((n, 3, pad_hw[0], pad_hw[1]), float('nan')) if out is None else out
        assert tuple(res.shape) == (n, 3, pad_hw[0], pad_hw[1]) and res.is_contiguous()
        for i in range(n):
            res[i] = one(src[i].numpy())
        return res

    def plain(src, size_hw, pad_hw, mean, std, to_rgb=True, out=None):
        calls.append(('plain', src.shape[0], tuple(src.shape[1:3]), tuple(size_hw), tuple(pad_hw)))

        def one(f):
            t, _ = data.prepare_image(f, (size_hw[1], size_hw[0]), dict(mean=mean, std=std, to_rgb=to_rgb), size_divisor=1, keep_ratio=False)
            return torch.nn.functional.pad(t, (0, pad_hw[1] - t.shape[2], 0, pad_hw[0] - t.shape[1]))
        return write('plain', src, size_hw, pad_hw, out, one)

    def with_lens(src, lens, size_hw, pad_hw, mean, std, to_rgb=True, out=None):
        calls.append(('lens', src.shape[0], tuple(src.shape[1:3]), tuple(size_hw), tuple(pad_hw), lens))
        return write('lens', src, size_hw, pad_hw, out,
                     lambda f: torch.from_numpy(R.image(f, from_lens(lens), size_hw, pad_hw, mean, std, to_rgb)[0].astype(np.float32)))
    monkeypatch.setattr(ops, 'image_prep_u8', plain)
    monkeypatch.setattr(ops, 'image_prep_lens_u8', with_lens)
    return calls


def test_prepare_images_device_groups_by_shape_and_lens(host_kernels):
    from imvoxelnet_amd import data
    rng = np.random.default_rng(11)
    A, B = to_lens(R.case_lens('tangential', (37, 53))), to_lens(R.case_lens('fisheye', (37, 53)))
    A2 = to_lens(R.case_lens('tangential', (37, 53)))                # an equal lens is the same group
    f = [rng.integers(0, 256, (37, 53, 3), dtype=np.uint8) for _ in range(6)] + [rng.integers(0, 256, (30, 60, 3), dtype=np.uint8)]
    lenses = [A, A2, B, None, A, A, A]
    img, metas = data.prepare_images_device(f, (64, 48), device='cpu', lens=lenses)
    shp = data._pipeline_shapes((37, 53), (64, 48), 32, True)
    shp2 = data._pipeline_shapes((30, 60), (64, 48), 32, True)
    plane = (max(shp[1][0], shp2[1][0]), max(shp[1][1], shp2[1][1]))
    assert img.shape == (7, 3) + plane and not torch.isnan(img).any()
    # runs of adjacent frames of one (shape, lens) group take one launch each
    assert host_kernels == [('lens', 2, (37, 53), shp[0], plane, A), ('lens', 2, (37, 53), shp[0], plane, A), ('lens', 1, (37, 53), shp[0], plane, B),
                            ('plain', 1, (37, 53), shp[0], plane), ('lens', 1, (30, 60), shp2[0], plane, A)]
    for i, l in enumerate(lenses):
        hw = tuple(f[i].shape[:2])
        size = data._pipeline_shapes(hw, (64, 48), 32, True)[0]
        if l is None:
            t, m = data.prepare_image(f[i], (64, 48))
            want = torch.zeros(3, *plane)
            want[:, :t.shape[1], :t.shape[2]] = t
        else:
            want = torch.from_numpy(R.image(f[i], from_lens(l), size, plane, MEAN, STD, True)[0].astype(np.float32))
            m = data.prepare_image(f[i], (64, 48))[1]
        assert torch.equal(img[i], want) and metas[i] == m, i
    # one Lens for every frame; a stacked batch; a [B][V] sample
    del host_kernels[:]
    stacked = np.stack(f[:4])
    img1, _ = data.prepare_images_device(stacked, (64, 48), device='cpu', lens=A)
    assert host_kernels == [('lens', 4, (37, 53), shp[0], shp[1], A)]
    del host_kernels[:]
    img2, metas2 = data.prepare_images_device([f[:2], f[2:4]], (64, 48), device='cpu', lens=[A, A, B, B])
    assert img2.shape == (2, 2, 3) + shp[1] and torch.equal(img2[0], img1[:2]) and len(metas2) == 2
    assert host_kernels == [('lens', 2, (37, 53), shp[0], shp[1], A), ('lens', 2, (37, 53), shp[0], shp[1], B)]
    # a stacked batch with per-frame lenses splits into groups
    del host_kernels[:]
    img3, _ = data.prepare_images_device(stacked, (64, 48), device='cpu', lens=[A, B, A, A])
    assert [c[:2] + c[5:] for c in host_kernels] == [('lens', 1, A), ('lens', 2, A), ('lens', 1, B)] and torch.equal(img3[0], img1[0]) and torch.equal(img3[2:], img1[2:])
    with pytest.raises(ValueError, match='3 lenses for 4 frames'):
        data.prepare_images_device(stacked, (64, 48), device='cpu', lens=[A, B, A])
    with pytest.raises(TypeError, match='data.Lens or None'):
        data.prepare_images_device(stacked, (64, 48), device='cpu', lens=[A, B, A, 'brown'])


def test_prepare_images_device_without_a_lens_issues_the_calls_it_issued(host_kernels):
    """lens=None (and the keyword left out): the plain op only, one launch per run of adjacent frames of a source shape, the same pixels."""
    from imvoxelnet_amd import data
    rng = np.random.default_rng(12)
    f = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((40, 64), (32, 64), (40, 64), (40, 64))]
    want = [('plain', 1, (40, 64), (64, 64), (64, 64)), ('plain', 2, (40, 64), (64, 64), (64, 64)), ('plain', 1, (32, 64), (64, 64), (64, 64))]
    a, ma = data.prepare_images_device(f, (64, 64), device='cpu', keep_ratio=False, size_divisor=16)
    assert host_kernels == want
    del host_kernels[:]
    b, mb = data.prepare_images_device(f, (64, 64), device='cpu', keep_ratio=False, size_divisor=16, lens=None)
    assert host_kernels == want and torch.equal(a, b) and ma == mb
    for i, fr in enumerate(f):
        t, m = data.prepare_image(fr, (64, 64), keep_ratio=False, size_divisor=16)
        assert torch.equal(a[i], t) and ma[i] == m


def test_simple_test_u8_passes_the_lens_through(host_kernels, monkeypatch):
    import imvoxelnet_amd as ia
    from imvoxelnet_amd.workloads import kitti_model_cfg, KITTI_TEST_CFG
    model = ia.build_detector(kitti_model_cfg(n_voxels=(24, 28, 12), in_ch=16, out_ch=32), test_cfg=KITTI_TEST_CFG)
    seen = {}
    monkeypatch.setattr(model, 'simple_test', lambda img, metas: seen.update(img=img, metas=metas) or 'results')
    f = list(R.frames(5, 2, (48, 160)))
    A = to_lens(R.case_lens('tangential', (48, 160)))
    assert model.simple_test_u8(f, [dict(lidar2img='L0'), dict(lidar2img='L1')], (320, 96), lens=A, device='cpu') == 'results'
    assert host_kernels == [('lens', 2, (48, 160), (96, 320), (96, 320), A)] and seen['img'].shape == (2, 1, 3, 96, 320)
    del host_kernels[:]
    model.simple_test_u8(f, [dict(lidar2img='L0'), dict(lidar2img='L1')], (320, 96), device='cpu')
    assert host_kernels == [('plain', 2, (48, 160), (96, 320), (96, 320))]


# ------------------------------------------------------------------ the scenes with stubbed ops
VS = (0.16, 0.16, 0.2)
K4 = np.array([[90., 0, 63.5, 0], [0, 90., 47.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
META = dict(lidar2img=dict(intrinsic=K4, origin=np.array([0.37, -1.21, .5], np.float32)))
SRC, SIZE, PAD, FHW = (96, 128), (96, 128), (96, 128), (24, 32)
SHAPES = dict(img_shape=SIZE + (3,), ori_shape=SRC + (3,), pad_shape=PAD + (3,))
LENS = R.lens('brown', 84.0, 85.0, 65.1, 46.3, [0.19, 0.021, 0.0013, -0.0007, 0], new=(90.0, 90.0, 63.5, 47.5))       # pincushion: the corners are border


class _OnDevice(torch.Tensor):
    """A host tensor that says it lives on the device: enough for the argument checks of an add whose launches are all stubbed."""
    is_cuda = True


def _stubbed(monkeypatch, batch=False, counts=((10, 10),) * 8, **kw):
    """A SceneSession (or a SceneBatch of two) on a mock model; the pipeline, ops.map_prep_lens (served by ref_lens), the gate's count, the trunk and
    the lift are recorders.  log.order names what ran, in order."""
    from imvoxelnet_amd import SceneBatch, SceneSession, data, ops
    log = types.SimpleNamespace(order=[], pipeline=[], map_prep=[], coverage=[], lifts=[])
    model = types.SimpleNamespace(head_2d=None, voxel_size=VS, n_voxels=(40, 40, 16), _prepared_device=torch.device('cpu'), _native=None,
                                  _camera_setup=lambda metas, stride, dev: (torch.zeros(1, len(metas[0]['lidar2img']['extrinsic']), 3, 4), torch.zeros(1, 3),
                                                                            torch.zeros(1, 2, dtype=torch.int32)),
                                  _compute_projection=lambda meta, stride: torch.zeros(len(meta['lidar2img']['extrinsic']), 3, 4))
    s = SceneBatch(model, [META, META], **kw) if batch else SceneSession(model, META, **kw)

    def pipeline(frames, img_scale, **pkw):
        log.order.append('pipeline')
        log.pipeline.append(dict(pkw, n=len(frames[0])))
        return torch.zeros(1, len(frames[0]), 3, *PAD).as_subclass(_OnDevice), [dict(SHAPES)]

    def map_prep(size_hw, pad_hw, src_hw, lens=None, src=None, scale=1.0, stride=4, n=1, out=None, device=None):
        log.order.append('map_prep')
        log.map_prep.append(dict(lens=lens, src=None if src is None else tuple(src.shape), scale=scale, stride=stride, device=str(device)))
        L = None if lens is None else from_lens(lens)
        assert (tuple(size_hw), tuple(pad_hw), tuple(src_hw)) == (SIZE, PAD, SRC)
        if src is None:
            res = torch.from_numpy(R.cover(L, src_hw, size_hw, pad_hw, stride))[None].repeat(n, 1, 1)
        else:
            res = torch.stack([torch.from_numpy(R.picked(m.numpy(), L, size_hw, pad_hw, scale, stride)) for m in src])
        if out is not None:
            out.copy_(res)
        return res if out is None else out

    def coverage(E, *a, **k):
        log.order.append('coverage')
        log.coverage.append(a[1] if batch else a[0])                 # the maps the gate sees
        return np.asarray(counts[:len(E)], np.int64)

    def features(img):
        log.order.append('trunk')
        return torch.zeros(img.shape[0], 1, *FHW, 8)

    def lift_session(p0, proj, origin, crop, E, hw, weights, emit, maps=(None, None)):
        log.lifts.append(maps)
        s._grow(E, hw, stale=False)

    monkeypatch.setattr(data, 'prepare_images_device', pipeline)
    monkeypatch.setattr(ops, 'map_prep_lens', map_prep)
    s._coverage, s._features = coverage, features
    if batch:
        def lift_batch(p0, proj_h, groups, touched, cam, E, hw, weights, emit, maps=(None, None)):
            log.lifts.append(maps)
            for sc in touched:
                s._scenes[sc]._grow([E[t] for t in groups[sc]], hw, stale=False)
        s._add_unbounded = lift_batch
    else:
        s._add_unbounded = lift_session
    return s, log


def _frames(V):
    E = []
    for v in range(V):
        e = np.eye(4, dtype=np.float32)
        e[0, 3] = v
        E.append(e)
    return list(R.frames(3, V, SRC)), E


def test_scene_cover_multiplies_the_weights_is_cached_and_reaches_the_gate(monkeypatch):
    lens = to_lens(LENS)
    cover = torch.from_numpy(R.cover(LENS, SRC, SIZE, PAD, 4))
    assert cover.shape == FHW and 0 < cover.sum() < cover.numel() and cover[0, 0] == 0 and cover[12, 16] == 1
    s, log = _stubbed(monkeypatch, decay=1.0)
    f, E = _frames(2)
    pw = 0.25 + torch.rand(2, *FHW, generator=torch.Generator().manual_seed(1))
    s.add_views_u8(f, E, (128, 96), pixel_weights=pw, lens=lens, device='cpu')
    assert log.order == ['map_prep', 'pipeline', 'trunk'] and log.map_prep == [dict(lens=lens, src=None, scale=1.0, stride=4, device='cpu')]
    assert log.pipeline == [dict(device='cpu', lens=[lens, lens], n=2)]
    got = log.lifts[0]
    assert got[1] is None and torch.equal(got[0], pw * cover[None]) and (got[0][:, 0, 0] == 0).all(), 'the cover multiplies pixel_weights'
    # second call: the cover is cached (no map_prep), the cover alone is the confidence, and the gate -- before the pipeline -- sees it
    del log.order[:]
    s.add_views_u8(f[:1], E[:1], (128, 96), lens=to_lens(LENS), min_novelty=0.5, device='cpu')
    assert log.order == ['coverage', 'pipeline', 'trunk'] and len(log.map_prep) == 1 and len(s._covers) == 1
    assert torch.equal(log.coverage[0][0], cover[None]) and log.coverage[0][1] is None
    assert torch.equal(log.lifts[1][0], cover[None]) and s.last_admitted == [True] and s.n_views == 3
    # a rejected frame of a rig: its lens entry leaves with it
    s._coverage = lambda E, *a, **k: np.asarray([[10, 0], [10, 10]], np.int64)
    s.add_views_u8(f, E, (128, 96), lens=[None, lens], min_novelty=0.5, device='cpu')
    assert s.last_admitted == [False, True] and log.pipeline[-1] == dict(device='cpu', lens=[lens], n=1) and torch.equal(log.lifts[2][0], cover[None])
    # a frame without a lens in a rig keeps full confidence
    s.add_views_u8(f, E, (128, 96), lens=[None, lens], device='cpu')
    assert torch.equal(log.lifts[3][0], torch.stack([torch.ones(FHW), cover])) and len(log.map_prep) == 1


def test_scene_without_lens_calls_what_it_called(monkeypatch):
    s, log = _stubbed(monkeypatch, decay=1.0)
    f, E = _frames(2)
    s.add_views_u8(f, E, (128, 96), device='cpu')
    assert log.order == ['pipeline', 'trunk'] and log.pipeline == [dict(device='cpu', n=2)] and log.lifts == [(None, None)] and s._covers == {}
    # a plain session takes the lens for its image and no mask
    p, plog = _stubbed(monkeypatch)
    lens = to_lens(LENS)
    p.add_views_u8(f, E, (128, 96), lens=lens, device='cpu')
    assert plog.order == ['pipeline', 'trunk'] and plog.pipeline == [dict(device='cpu', lens=[lens, lens], n=2)] and plog.lifts == [(None, None)]
    with pytest.raises(ValueError, match='opened plain'):
        p.add_views_u8(f, E, (128, 96), lens=lens, depth_frames=np.zeros((2,) + SRC, np.uint16), device='cpu')


def test_scene_depth_frames(monkeypatch):
    lens = to_lens(LENS)
    f, E = _frames(2)
    depth = np.random.default_rng(4).integers(0, 5000, (2,) + SRC).astype(np.uint16)
    depth[:, ::7] = 0
    s, log = _stubbed(monkeypatch, decay=1.0)
    with pytest.raises(ValueError, match='opened without depth_gate'):
        s.add_views_u8(f, E, (128, 96), depth_frames=depth, device='cpu')
    assert log.order == [] and s.n_views == 0
    s, log = _stubbed(monkeypatch, window=4, depth_gate=(0.1, 0.2))
    s._add_windowed = lambda p0, proj, E, hw, weights, maps=(None, None): (log.lifts.append(maps), s._admit(*s._free_slots(len(E)), E, hw))
    with pytest.raises(ValueError, match='exclude each other'):
        s.add_views_u8(f, E, (128, 96), depth_frames=depth, depths=torch.zeros(2, *FHW), device='cpu')
    for bad, err in ((depth[:1], ValueError), (depth.astype(np.int32), TypeError), (depth[:, :50], ValueError), ([depth[0], depth[1]], TypeError)):
        with pytest.raises(err, match='depth_frames'):
            s.add_views_u8(f, E, (128, 96), depth_frames=bad, device='cpu')
    with pytest.raises(ValueError, match='depth_scale'):
        s.add_views_u8(f, E, (128, 96), depth_frames=depth, depth_scale=float('nan'), device='cpu')
    assert log.order == [] and s.n_views == 0
    # with a lens: the cover and the depth through the same geometry; without: the ideal camera, and no cover
    s.add_views_u8(f, E, (128, 96), lens=lens, depth_frames=depth, device='cpu')
    assert [m['src'] for m in log.map_prep] == [None, (2,) + SRC] and log.map_prep[1]['lens'] == lens and log.map_prep[1]['scale'] == 0.001
    want = torch.stack([torch.from_numpy(R.picked(d, LENS, SIZE, PAD, 0.001, 4)) for d in depth])
    assert torch.equal(log.lifts[0][1], want) and (want[:, 0, 0] == 0).all() and want.max() > 1.0 and torch.equal(log.lifts[0][0], torch.from_numpy(R.cover(LENS, SRC, SIZE, PAD, 4))[None].repeat(2, 1, 1))
    s.add_views_u8(f, E, (128, 96), depth_frames=torch.from_numpy(depth.astype(np.float32)), depth_scale=1.0, device='cpu')
    assert log.map_prep[2]['lens'] is None and log.pipeline[-1] == dict(device='cpu', n=2) and log.lifts[1][0] is None
    assert torch.equal(log.lifts[1][1], torch.stack([torch.from_numpy(R.picked(d.astype(np.float32), None, SIZE, PAD, 1.0, 4)) for d in depth]))
    # a rig: one launch per run of frames of one lens
    n = len(log.map_prep)
    s.add_views_u8(f, E, (128, 96), lens=[lens, None], depth_frames=depth, device='cpu')
    assert [(m['lens'], m['src']) for m in log.map_prep[n:]] == [(lens, (1,) + SRC), (None, (1,) + SRC)]


def test_scene_refuses_a_lens_that_is_not_the_metas_camera(monkeypatch):
    from imvoxelnet_amd import data
    s, log = _stubbed(monkeypatch, decay=1.0)
    f, E = _frames(1)
    wrong = data.Lens('brown', LENS_K(), LENS['coef'], new_K=[[90.001, 0, 63.5], [0, 90, 47.5], [0, 0, 1]])
    with pytest.raises(ValueError, match='new_K'):
        s.add_views_u8(f, E, (128, 96), lens=wrong, device='cpu')
    with pytest.raises(ValueError, match='new_K'):
        s.add_views_u8(f, E, (128, 96), lens=data.Lens('brown', LENS_K(), LENS['coef']), device='cpu')          # new_K defaults to K, which is another camera
    assert log.order == [] and s.n_views == 0
    close = data.Lens('brown', LENS_K(), LENS['coef'], new_K=[[90 * (1 + 5e-7), 0, 63.5], [0, 90, 47.5], [0, 0, 1]])
    s.add_views_u8(f, E, (128, 96), lens=close, device='cpu')
    assert s.n_views == 1
    # an identity intrinsic (the extrinsics carry the projection) is not judged
    from imvoxelnet_amd import scene
    scene._check_intrinsic(dict(lidar2img=dict(intrinsic=np.eye(4, dtype=np.float32))), wrong)
    with pytest.raises(ValueError, match='one source size'):
        s.add_views_u8([f[0], f[0][:50]], E * 2, (128, 96), lens=close, device='cpu')


def LENS_K():
    return [[LENS['fx'], 0, LENS['cx']], [0, LENS['fy'], LENS['cy']], [0, 0, 1]]


def test_batch_takes_lens_and_depth_frames(monkeypatch):
    lens = to_lens(LENS)
    cover = torch.from_numpy(R.cover(LENS, SRC, SIZE, PAD, 4))
    b, log = _stubbed(monkeypatch, batch=True, decay=1.0, depth_gate=(0.1, 0.1))
    f, E = _frames(3)
    depth = np.random.default_rng(5).integers(1, 4000, (3,) + SRC).astype(np.uint16)
    b.add_views_u8(f, E, [1, 0, 1], (128, 96), lens=lens, depth_frames=depth, device='cpu')
    assert log.order == ['map_prep', 'map_prep', 'pipeline', 'trunk'] and b.n_views == [1, 2] and log.pipeline == [dict(device='cpu', lens=[lens] * 3, n=3)]
    assert torch.equal(log.lifts[0][0], cover[None].repeat(3, 1, 1))
    assert torch.equal(log.lifts[0][1], torch.stack([torch.from_numpy(R.picked(d, LENS, SIZE, PAD, 0.001, 4)) for d in depth]))
    del log.order[:]
    b.add_views_u8(f[:2], E[:2], [0, 0], (128, 96), lens=lens, min_novelty=0.5, device='cpu')
    assert log.order == ['coverage', 'pipeline', 'trunk'] and torch.equal(log.coverage[0][0], cover[None].repeat(2, 1, 1)) and len(b._covers) == 1
    del log.order[:]
    b.add_views_u8(f[:1], E[:1], [0], (128, 96), device='cpu')
    assert log.order == ['pipeline', 'trunk'] and log.pipeline[-1] == dict(device='cpu', n=1) and log.lifts[-1] == (None, None)


# ------------------------------------------------------------------ the reference itself
def test_every_case_is_far_from_every_decision():
    """The decisions of the GPU tests are made robust by the reference alone: NO pixel of any case has u or v within 1e-6 px of an inside boundary,
    r2 within 1e-9 relative of r2_max or -- for the nearest pick -- a coordinate within 1e-6 of a half.  Zero, not merely few."""
    zero = dict(edge=0, ring=0, half=0)
    for name, (src, dst, pad, _) in R.SHAPES.items():
        for ln in R.LENSES:
            assert R.margins(R.case_lens(ln, src), src, dst) == zero, (name, ln)
    src, dst, _ = R.EQUAL
    assert R.margins(R.case_lens('zero', src), src, dst) == zero
    src, dst, _, _ = R.BIG
    assert R.margins(R.case_lens(R.BIG_LENS, src), src, dst) == zero
    for name, (src, dst, pad) in R.MAP_SHAPES.items():
        for ln in R.MAP_LENSES:
            for stride in R.STRIDES:
                assert R.margins(None if ln is None else R.case_lens(ln, src), src, dst, pick=True, stride=stride, pad_hw=pad) == zero, (name, ln, stride)
    assert R.margins(LENS, SRC, SIZE, pick=True, stride=4, pad_hw=PAD) == zero
    # what the case list promises about its lenses
    src, dst = R.SHAPES['vector'][:2]
    inside = {ln: R.G(R.case_lens(ln, src), src, dst, *R.grid(dst))[3] for ln in R.LENSES}
    assert not inside['barrel'][0, 0] and not inside['barrel'][-1, -1] and inside['barrel'][11, 15], 'the corners of the strong barrel are border'
    assert not inside['pincushion'][0, 0] and inside['tangential'].all() and 0 < inside['fisheye'].sum() < inside['fisheye'].size
    u, v, r2, ins = R.G(R.case_lens('ring', src), src, dst, *R.grid(dst))
    cut = r2 > 0.2317
    assert cut.any() and (~cut).any() and np.array_equal(ins, ~cut), 'the finite r2_max alone cuts the ring: every pixel it keeps is in the frame'


# the cv2 restatement against the exact blend, in grey levels: per axis two 11-bit weights, each within 0.5 / 2048 of its fraction, on values of at
# most 255: 0.5 * (S0 + S1) / 2048 <= 255 / 2048 per axis; the `>> 4` of the horizontal sums drops less than 1 / 128; the two `>> 16` of the vertical
# pass drop less than 1 / 4 each; the final `+ 2 >> 2` rounds to a grey level: at most 1 / 2.
CV2_QUANT = 2 * 255.0 / 2048 + 1.0 / 128 + 2 * 0.25 + 0.5            # = 1.2568 grey levels


@pytest.mark.parametrize('name,src,dst', [('down', (37, 53), (23, 31)), ('up', (9, 11), (20, 24)), ('equal', (21, 28), (21, 28)), ('half', (40, 56), (20, 28))])
def test_reference_agrees_with_prepare_image_for_an_ideal_camera(name, src, dst):
    """Reference sanity: with zero coefficients and new_K == K the map G is the resize's own pixel-centre rule, so the fp64 reference is exact bilinear
    resampling and must agree with data.prepare_image within the quantisation of the cv2 restatement.  In grey levels that is at most
    CV2_QUANT = 2 * 255 / 2048 (11-bit weights, both axes) + 1 / 128 (`>> 4`) + 2 / 4 (two `>> 16`) + 1 / 2 (the rounding to uint8) = 1.2568; the equal
    size is a copy (exact) and the exact half takes (a + b + c + d + 2) >> 2, the 2 x 2 mean rounded (bilinear at a 2 x 2 centre is the mean: 1 / 2).
    Divided by |std|, plus 1e-5 for the fp32 normalisation of prepare_image.  Measured worst |diff| * |std| / CV2_QUANT: down 0.601, up 0.593, equal
    5.5e-6 (the fp32 normalisation alone), half 0.398."""
    from imvoxelnet_amd import data
    f = R.frames(21, 1, src)[0]
    L = R.case_lens('zero', src)
    ref, mask = R.image(f, L, dst, dst, MEAN, STD, True)
    assert mask.all()
    t, _ = data.prepare_image(f, (dst[1], dst[0]), dict(mean=MEAN, std=STD, to_rgb=True), size_divisor=1, keep_ratio=False)
    sd = np.asarray(STD)[:, None, None]
    diff = np.abs(t.numpy().astype(np.float64) - ref)
    ratio = float((diff * sd / CV2_QUANT).max())
    print(f'{name}: worst |diff| * |std| / CV2_QUANT = {ratio:.3g}')
    bound = {'equal': 0.0, 'half': 0.5}.get(name, CV2_QUANT)
    assert (diff <= bound / sd + 1e-5).all(), ratio
    # and the ideal camera written as no lens at all is the same map
    u0, v0, _, in0 = R.G(None, src, dst, *R.grid(dst))
    u1, v1, _, in1 = R.G(L, src, dst, *R.grid(dst))
    assert in0.all() and in1.all() and np.abs(u0 - u1).max() < 1e-11 and np.abs(v0 - v1).max() < 1e-11
