"""CPU-only tests of the decoder pixel formats of the image pipeline (include/imvoxel.h 0.5.3: ivx_frame_format / ivx_yuv_matrix /
ivx_image_prep_fmt_u8, csrc/image_prep.hip, csrc/pixel_fetch.h; data.FrameFormat, data.to_bgr_u8, data.prepare_images_device(format=)): the host sibling of the
conversion against the independent restatement of tests/ref_pixfmt.py, the named matrices against Fraction arithmetic, the record, the
grouping with the op replaced by a host stand-in, the refusals of the Python layer and of the entry, and an older library.  The library loads
without a device; nothing here launches a kernel.  cv2 is not installed where this was written: parity with cv2.cvtColor is UNPINNED."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import ref_pixfmt as P
from helpers import ROOT

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
NAMED = [(s, f) for s in ('bt601', 'bt709') for f in (False, True)]


def _fmt_struct(layout=5, **kw):
    from imvoxelnet_amd import _lib
    v = dict(layout=layout, plane1_row_bytes=54, plane1_offset=37 * 53, y_off=16, cy=1220542, cub=2116026, cug=-409993, cvg=-852492, cvr=1673527)
    v.update(kw)
    return _lib.FrameFormat(**v)


# ------------------------------------------------------------------ the definition on the host
@pytest.mark.parametrize('layout', P.LAYOUTS)
def test_to_bgr_u8_equals_the_reference(layout):
    from imvoxelnet_amd import data
    rng = np.random.default_rng(3)
    mats = [P.matrix(*k) for k in NAMED] + [(255, P.COEF_MAX, P.COEF_MAX, -P.COEF_MAX, -P.COEF_MAX, P.COEF_MAX)] if layout in P.YUV else [None]
    for (h, w) in ((1, 1), (1, 2), (2, 1), (3, 3), (6, 8), (9, 13), (10, 14)):
        for m in mats:
            buf, g = P.surface(rng, layout, h, w)
            want = P.to_bgr(buf, layout, h, w, m=m, **g)
            if layout == 'nv12' and w % 2:                   # the stacked array has one pitch: rebuild the surface on the even width
                buf, g = P.surface(rng, layout, h, w, row_bytes=w + 1)
                want = P.to_bgr(buf, layout, h, w, m=m, **g)
                arr = np.concatenate([buf, np.zeros((h + (h + 1) // 2) * (w + 1) - buf.size, np.uint8)]).reshape(-1, w + 1)
            else:
                arr = P.tight(buf, layout, h, w, g)
            fmt = data.FrameFormat(layout, yuv=m) if m is not None else data.FrameFormat(layout)
            got = data.to_bgr_u8(arr, fmt, src_hw=(h, w))
            assert got.dtype == np.uint8 and got.shape == (h, w, 3) and np.array_equal(got, want), (layout, h, w, m)
            if w % 2 == 0:
                assert np.array_equal(data.to_bgr_u8(torch.from_numpy(arr), layout if m is None else fmt), want)
                assert fmt.frame_hw(arr.shape) == (h, w)
    if layout == 'gray':
        assert np.array_equal(data.to_bgr_u8(arr.reshape(h, w, 1), 'gray'), want)


def test_to_bgr_u8_refuses():
    from imvoxelnet_amd import data
    with pytest.raises(TypeError, match='uint8'):
        data.to_bgr_u8(np.zeros((4, 4, 3), np.float32), 'bgr')
    for layout, shape in (('bgr', (4, 4, 4)), ('bgra', (4, 4, 3)), ('gray', (4, 4, 3)), ('yuyv', (4, 3, 2)), ('yuyv', (4, 4, 3)), ('nv12', (6, 3)),
                          ('nv12', (4, 4)), ('nv12', (6, 4, 1)), ('rgb', (4, 4))):
        with pytest.raises(TypeError, match=layout):
            data.to_bgr_u8(np.zeros(shape, np.uint8), layout)
    with pytest.raises(ValueError, match='src_hw'):
        data.to_bgr_u8(np.zeros((6, 4), np.uint8), 'nv12', src_hw=(4, 5))
    with pytest.raises(ValueError, match='layout'):
        data.to_bgr_u8(np.zeros((6, 4), np.uint8), 'nv21')


# ------------------------------------------------------------------ ivx_yuv_matrix
def test_yuv_matrix_rows():
    from imvoxelnet_amd import _lib, data
    L = _lib.lib()
    rows = {}
    for si, std in enumerate(('bt601', 'bt709')):
        for full in (False, True):
            f = _lib.FrameFormat(layout=5, plane1_row_bytes=77, plane1_offset=99)
            assert L.ivx_yuv_matrix(si, int(full), C.byref(f)) == 0
            assert (f.layout, f.plane1_row_bytes, f.plane1_offset) == (5, 77, 99)                     # only the six integers are written
            rows[(std, full)] = (f.y_off, f.cy, f.cub, f.cug, f.cvg, f.cvr)
    assert rows[('bt601', False)] == (16, 1220542, 2116026, -409993, -852492, 1673527)               # OpenCV's table, by value
    for k in NAMED[1:]:
        assert rows[k] == P.matrix(*k), k                                                            # Fraction arithmetic, half to even
    for k, r in rows.items():
        assert 0 <= r[0] <= 255 and all(abs(v) <= 3 << 20 for v in r[1:]), k
        assert data.FrameFormat('nv12', k[0], k[1]).matrix == r and data.FrameFormat('yuyv', k[0], full_range=k[1]).struct().cy == r[1]
    assert rows[('bt601', True)][0] == 0 and rows[('bt601', True)][1] == 1 << 20
    # the exact BT.601 limited matrix differs from cv2's rounded decimals, which is why that row is listed by value
    from fractions import Fraction
    assert P.round_half_even(Fraction(255, 219) * 2 ** 20) != 1220542
    assert L.ivx_yuv_matrix(2, 0, C.byref(_lib.FrameFormat())) == -1 and b'unknown standard 2' in L.ivx_last_error()
    assert L.ivx_yuv_matrix(0, 0, None) == -1 and b'null' in L.ivx_last_error()


# ------------------------------------------------------------------ the record
def test_frame_format_record():
    from imvoxelnet_amd import data, _lib
    a, b = data.FrameFormat('nv12'), data.FrameFormat('nv12', 'bt601', False)
    assert a == b and hash(a) == hash(b) and a.key == b.key and {a: 1}[b] == 1 and a.layout == 'nv12' and a.matrix == P.BT601_LIMITED
    assert a == data.FrameFormat('nv12', yuv=P.BT601_LIMITED) and a == data.FrameFormat(a)
    assert a != data.FrameFormat('nv12', 'bt709') and a != data.FrameFormat('nv12', full_range=True) and a != data.FrameFormat('yuyv') and a != 'nv12'
    assert data.FrameFormat('bgra') == data.FrameFormat('bgra', 'bt709', True) and data.FrameFormat('bgra').matrix is None      # no matrix without YUV
    assert len({data.FrameFormat(l) for l in P.LAYOUTS}) == 7
    s = a.struct(plane1_offset=1 << 33, plane1_row_bytes=70)
    assert isinstance(s, _lib.FrameFormat) and (s.layout, s.plane1_row_bytes, s.plane1_offset) == (5, 70, 1 << 33)
    assert (s.y_off, s.cy, s.cub, s.cug, s.cvg, s.cvr) == P.BT601_LIMITED
    assert [data.FrameFormat(l).struct().layout for l in P.LAYOUTS] == list(range(7)) and tuple(data.FrameFormat.LAYOUTS) == P.LAYOUTS
    assert 'nv12' in repr(a)
    for bad in (dict(layout='nv21'), dict(layout=5), dict(layout='nv12', yuv='bt2020'), dict(layout='nv12', yuv=(16, 1, 2, 3, 4)),
                dict(layout='yuyv', yuv=(16, 1.5, 2, 3, 4, 5)), dict(layout='nv12', yuv=(256, 1, 2, 3, 4, 5)), dict(layout='nv12', yuv=(-1, 1, 2, 3, 4, 5)),
                dict(layout='nv12', yuv=(0, (3 << 20) + 1, 2, 3, 4, 5)), dict(layout='yuyv', yuv=(0, 1, 2, 3, 4, -(3 << 20) - 1))):
        with pytest.raises(ValueError):
            data.FrameFormat(**bad)
    data.FrameFormat('nv12', yuv=(255, 3 << 20, -(3 << 20), 3 << 20, -(3 << 20), 3 << 20))                    # the bound itself is legal


def test_binding_matches_the_header():
    from imvoxelnet_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'imvoxel.h')).read()
    body = re.search(r'typedef struct ivx_frame_format \{(.*?)\} ivx_frame_format;', header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = []
    for ctype, decl in re.findall(r'(int32_t|int64_t)\s+([^;]+);', body):
        names += [(n.strip(), ctype) for n in decl.split(',')]
    assert [(n, {C.c_int32: 'int32_t', C.c_int64: 'int64_t'}[t]) for n, t in _lib.FrameFormat._fields_] == names
    assert C.sizeof(_lib.FrameFormat) == 40 and _lib.FrameFormat.plane1_offset.offset == 8
    for i, name in enumerate(('BGR8', 'RGB8', 'BGRA8', 'RGBA8', 'GRAY8', 'NV12', 'YUYV')):
        assert re.search(rf'#define IVX_PIX_{name}\s+{i}\b', header), name
    assert re.search(r'#define IVX_YUV_BT601\s+0\b', header) and re.search(r'#define IVX_YUV_BT709\s+1\b', header)
    L = _lib.lib()
    assert L.ivx_version() >= 503 and len(L.ivx_image_prep_fmt_u8.argtypes) == 8 and len(L.ivx_yuv_matrix.argtypes) == 3
    assert {'ivx_image_prep_fmt_u8', 'ivx_yuv_matrix'} <= set(_lib.EXPORTS)
    import imvoxelnet_amd as ia
    assert ia.image_prep_fmt_u8 is ia.ops.image_prep_fmt_u8 and ia.FrameFormat is ia.data.FrameFormat and ia.to_bgr_u8 is ia.data.to_bgr_u8


# ------------------------------------------------------------------ the entry's refusals, without a device
def entry_call(src, out, d=None, f=None, lens=None, sib=1 << 20, n=1, null_d=False, null_f=False, null_src=False, null_out=False):
    """ivx_image_prep_fmt_u8 on a 37 x 53 NV12 frame (test_host_lens_prep._desc) with some arguments replaced -> (status, message)."""
    from imvoxelnet_amd import _lib
    import test_host_lens_prep as TL
    L = _lib.lib()
    d = TL._desc(src_row_bytes=53) if d is None else d
    f = _fmt_struct() if f is None else f
    rc = L.ivx_image_prep_fmt_u8(None if null_d else C.byref(d), None if null_f else C.byref(f), None if lens is None else C.byref(lens),
                                 None if null_src else src, sib, n, None if null_out else out, None)
    return rc, L.ivx_last_error()


def entry_cases():
    """Every IVX_ERR_INVALID_ARG of the entry: (keywords of entry_call, what the message must say)."""
    import test_host_lens_prep as TL
    cases = [(dict(null_d=True), b'null argument'), (dict(null_src=True), b'null argument'), (dict(null_out=True), b'null argument'),
             (dict(null_f=True), b'null frame format'),
             (dict(f=_fmt_struct(layout=7)), b'unknown layout 7'), (dict(f=_fmt_struct(layout=-1)), b'unknown layout -1'),
             (dict(d=TL._desc(src_row_bytes=52)), b'src_row_bytes 52 is below src_w = 53'),
             (dict(f=_fmt_struct(plane1_row_bytes=53)), b'plane1_row_bytes 53 is below 2 * ceil(src_w / 2) = 54'),
             (dict(f=_fmt_struct(plane1_offset=37 * 53 - 1)), b'plane1_offset 1960 is below src_h * src_row_bytes = 1961'),
             (dict(f=_fmt_struct(plane1_offset=(1 << 46) + 1)), b'plane1_offset 70368744177665 is above 2^46'),
             (dict(f=_fmt_struct(y_off=256)), b'y_off = 256'), (dict(f=_fmt_struct(y_off=-1)), b'y_off = -1'),
             (dict(n=2, sib=37 * 53 + 19 * 54 - 1), b'does not cover the last plane, which ends at byte 2987'),
             (dict(n=0), b'n = 0'), (dict(d=TL._desc(src_row_bytes=53, pad_h=22)), b'smaller than dst'),
             (dict(d=TL._desc(src_row_bytes=53, src_h=0)), b'positive'), (dict(d=TL._desc(src_row_bytes=53, std=(1, 0, 1))), b'std[1]'),
             (dict(d=TL._desc(src_row_bytes=53, pad_w=32769)), b'extents above'),
             (dict(lens=TL._lens(model=2)), b'unknown lens model 2'), (dict(lens=TL._lens(r2_max=0.0)), b'r2_max')]
    for c in ('cy', 'cub', 'cug', 'cvg', 'cvr'):
        for bad in ((3 << 20) + 1, -(3 << 20) - 1):
            cases.append((dict(f=_fmt_struct(**{c: bad})), f'coefficient {c} = {bad}'.encode()))
    # the row-bytes bound per layout: 3w, 3w, 4w, 4w, w, w, 4 * ceil(w / 2)
    for layout, need in enumerate((159, 159, 212, 212, 53, 53, 108)):
        cases.append((dict(d=TL._desc(src_row_bytes=need - 1), f=_fmt_struct(layout=layout, plane1_offset=1 << 20)),
                      f'src_row_bytes {need - 1} is below'.encode()))
    return cases


def test_entry_argument_validation_without_gpu():
    """Every bad argument is rejected with status -1 and a message that names it, before any launch (dummy non-null pointers)."""
    from imvoxelnet_amd import _lib
    import test_host_lens_prep as TL
    dummy = C.c_void_p(64)

    def call(**kw):
        return entry_call(dummy, dummy, **kw)
    for kw, needle in entry_cases():
        rc, msg = call(**kw)
        assert rc == -1 and b'ivx_image_prep_fmt_u8' in msg and needle in msg, (kw, msg)
    for layout, need in enumerate((159, 159, 212, 212, 53, 53, 108)):
        rc, msg = call(d=TL._desc(src_row_bytes=need - 1), f=_fmt_struct(layout=layout, plane1_offset=1 << 20))
        assert rc == -1 and msg.endswith(f'= {need}'.encode()), (layout, msg)
    # fields a layout does not use are not read: a wild matrix on BGRA, a wild plane on YUYV
    # (these calls would launch, so they are only shown to pass the checks up to an argument that fails later)
    rc, msg = call(d=TL._desc(src_row_bytes=212), f=_fmt_struct(layout=2, cy=1 << 30, y_off=999, plane1_row_bytes=0, plane1_offset=0), n=0)
    assert rc == -1 and b'n = 0' in msg
    with pytest.raises(ValueError, match='unknown layout'):
        _lib.check(call(f=_fmt_struct(layout=9))[0], 'ivx_image_prep_fmt_u8')


# ------------------------------------------------------------------ the Python layer's refusals and an older library
def test_ops_refuse_without_a_device_and_with_an_older_library(monkeypatch):
    from imvoxelnet_amd import _lib, ops, data
    z = lambda *s: torch.zeros(*s, dtype=torch.uint8)        # noqa: E731
    a = ((4, 4), (32, 32), (0, 0, 0), (1, 1, 1))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.image_prep_fmt_u8(z(1, 6, 4), 'nv12', *a)
    with pytest.raises(ValueError, match='layout'):
        ops.image_prep_fmt_u8(z(1, 6, 4), 'nv21', *a)
    with pytest.raises(TypeError, match='data.Lens'):
        ops.image_prep_fmt_u8(z(1, 6, 4), 'nv12', *a, lens=dict(k1=0))
    with pytest.raises(TypeError, match='torch.Tensor'):
        ops.image_prep_fmt_u8(np.zeros((1, 6, 4), np.uint8), 'nv12', *a)
    old = types.SimpleNamespace(ivx_version=lambda: 502)              # a build of the ABI from before 0.5.3: it loads, the op refuses
    monkeypatch.setattr(_lib, 'lib', lambda: old)
    with pytest.raises(_lib.IvxError, match='0.5.3'):
        ops.image_prep_fmt_u8(None, 'nv12', *a)
    with pytest.raises(_lib.IvxError, match='0.5.3'):
        data.prepare_images_device([np.zeros((6, 4), np.uint8)], (64, 48), device='cpu', format='nv12')
    assert data.FrameFormat('nv12').matrix == P.BT601_LIMITED          # the record itself needs no library


class _FakeCuda(torch.Tensor):
    """A host uint8 tensor that claims to be on the device: the shape / stride refusals of ops.image_prep_fmt_u8 come before any launch."""
    is_cuda = True


def test_ops_shape_and_geometry_refusals():
    from imvoxelnet_amd import ops

    def dev(*shape):
        return torch.zeros(*shape, dtype=torch.uint8).as_subclass(_FakeCuda)
    a = ((4, 4), (32, 32), (0, 0, 0), (1, 1, 1))
    bad = [((dev(1, 4, 4, 4), 'bgr'), {}, TypeError, r'\[n,H,W,3\]'), ((dev(1, 4, 4, 3), 'bgra'), {}, TypeError, r'\[n,H,W,4\]'),
           ((dev(1, 4, 4, 3), 'gray'), {}, TypeError, r'\[n,H,W,1\]'), ((dev(1, 4, 4, 3), 'yuyv'), {}, TypeError, r'\[n,H,W,2\]'),
           ((dev(1, 4, 3, 2), 'yuyv'), {}, ValueError, r'2 \* ceil'), ((dev(1, 6, 4, 1), 'nv12'), {}, TypeError, 'nv12'),
           ((dev(1, 6, 3), 'nv12'), {}, ValueError, 'even width'), ((dev(1, 4, 4), 'nv12'), {}, ValueError, 'even width'),
           ((dev(1, 6, 4), 'nv12'), dict(src_hw=(5, 4)), ValueError, 'src_hw'), ((dev(1, 4, 4, 2), 'yuyv'), dict(src_hw=(4, 5)), ValueError, 'src_hw'),
           ((dev(1, 4, 4, 4), 'bgra'), dict(src_hw=(4, 3)), ValueError, 'src_hw'), ((dev(1, 4, 4, 4), 'bgra'), dict(src_hw=(0, 4)), ValueError, 'positive'),
           ((dev(1, 6, 4), 'nv12'), dict(plane1_offset=16), ValueError, 'raw surface'),
           ((dev(1, 4, 8, 4)[:, :, ::2], 'bgra'), {}, ValueError, 'dense'), ((dev(1, 6, 8)[:, :, ::2], 'nv12'), {}, ValueError, 'dense'),
           ((dev(0, 4, 4, 3), 'rgb'), {}, ValueError, 'no frame'),
           # raw surfaces
           ((dev(64), 'nv12'), dict(row_bytes=4), ValueError, 'src_hw'), ((dev(2, 2, 32), 'bgra'), dict(row_bytes=16, src_hw=(4, 4)), TypeError, 'raw surface'),
           ((dev(64), 'bgra'), dict(row_bytes=15, src_hw=(4, 4)), ValueError, 'row_bytes 15'),
           ((dev(64), 'yuyv'), dict(row_bytes=11, src_hw=(4, 5)), ValueError, 'row_bytes 11'),
           ((dev(64), 'nv12'), dict(row_bytes=4, src_hw=(4, 4)), ValueError, 'plane1_offset= and plane1_row_bytes='),
           ((dev(64), 'nv12'), dict(row_bytes=5, src_hw=(4, 4), plane1_offset=19, plane1_row_bytes=4), ValueError, 'below'),
           ((dev(64), 'nv12'), dict(row_bytes=5, src_hw=(4, 5), plane1_offset=20, plane1_row_bytes=5), ValueError, 'below'),
           ((dev(64), 'bgra'), dict(row_bytes=16, src_hw=(4, 4), plane1_offset=64), ValueError, "belong to 'nv12'"),
           ((dev(63), 'bgra'), dict(row_bytes=16, src_hw=(4, 4)), ValueError, 'ends at byte 64'),
           ((dev(27), 'nv12'), dict(row_bytes=4, src_hw=(4, 4), plane1_offset=20, plane1_row_bytes=4), ValueError, 'ends at byte 28')]
    for (src, fmt), kw, exc, match in bad:
        with pytest.raises(exc, match=match):
            ops.image_prep_fmt_u8(src, fmt, *a, **kw)
    with pytest.raises(ValueError, match='out must be'):
        ops.image_prep_fmt_u8(dev(1, 4, 4, 4), 'bgra', *a, out=torch.zeros(1, 3, 32, 31).as_subclass(_FakeCuda))
    with pytest.raises(TypeError, match='uint8'):
        ops.image_prep_fmt_u8(torch.zeros(1, 4, 4, 4).as_subclass(_FakeCuda), 'bgra', *a)


# ------------------------------------------------------------------ prepare_images_device(format=) with a host stand-in of the op
@pytest.fixture
def host_op(monkeypatch):
    """ops.image_prep_fmt_u8 served by the reference conversion + data.prepare_image; ops.image_prep_u8 by data.prepare_image.  Calls are recorded
    as (name, n, frame array shape, format, lens, size_hw, pad_hw)."""
    from imvoxelnet_amd import data, ops
    calls = []

    def prep(f, size_hw, pad_hw, mean, std, to_rgb):
        t, _ = data.prepare_image(f, (size_hw[1], size_hw[0]), dict(mean=mean, std=std, to_rgb=to_rgb), size_divisor=1, keep_ratio=False)
        return torch.nn.functional.pad(t, (0, pad_hw[1] - t.shape[2], 0, pad_hw[0] - t.shape[1]))

    def ref_bgr(arr, fmt):
        h, w = fmt.frame_hw(arr.shape)
        g = dict(row_bytes=P.min_row_bytes(fmt.layout, w))
        if fmt.layout == 'nv12':
            g.update(plane1_offset=h * w, plane1_row_bytes=w)
        return P.to_bgr(arr.reshape(-1), fmt.layout, h, w, m=fmt.matrix, **g)

    def fmt_op(src, fmt, size_hw, pad_hw, mean, std, to_rgb=True, lens=None, out=None, **kw):
        assert isinstance(src, torch.Tensor) and src.dtype == torch.uint8 and not kw and isinstance(fmt, data.FrameFormat)
        calls.append(('fmt', src.shape[0], tuple(src.shape[1:]), fmt, lens, tuple(size_hw), tuple(pad_hw)))
        assert tuple(out.shape) == (src.shape[0], 3) + tuple(pad_hw) and out.is_contiguous()
        for i in range(src.shape[0]):
            out[i] = prep(ref_bgr(src[i].numpy(), fmt), size_hw, pad_hw, mean, std, to_rgb)
        return out

    def plain(src, size_hw, pad_hw, mean, std, to_rgb=True, out=None):
        calls.append(('plain', src.shape[0], tuple(src.shape[1:])))
        for i in range(src.shape[0]):
            out[i] = prep(src[i].numpy(), size_hw, pad_hw, mean, std, to_rgb)
        return out
    monkeypatch.setattr(ops, 'image_prep_fmt_u8', fmt_op)
    monkeypatch.setattr(ops, 'image_prep_u8', plain)
    return calls, ref_bgr


def test_prepare_images_device_groups_by_shape_format_and_lens(host_op):
    from imvoxelnet_amd import data
    import test_host_lens_prep as TL
    import ref_lens as RL
    calls, ref_bgr = host_op
    rng = np.random.default_rng(12)
    nv, nv709, yu, ga, bg = (data.FrameFormat('nv12'), data.FrameFormat('nv12', 'bt709'), data.FrameFormat('yuyv'), data.FrameFormat('gray'),
                             data.FrameFormat('bgra'))
    shapes = {'nv12': (54, 52), 'yuyv': (36, 52, 2), 'gray': (36, 52), 'bgra': (36, 52, 4), 'small': (30, 60)}     # all but `small` convert to 36 x 52
    fmts = [nv, data.FrameFormat('nv12'), nv709, nv, yu, ga, bg, bg, nv]
    keys = ['nv12', 'nv12', 'nv12', 'nv12', 'yuyv', 'gray', 'bgra', 'bgra', 'small']
    f = [rng.integers(0, 256, shapes[k], dtype=np.uint8) for k in keys]
    img, metas = data.prepare_images_device(f, (64, 48), device='cpu', format=fmts)
    shp, shp2 = data._pipeline_shapes((36, 52), (64, 48), 32, True), data._pipeline_shapes((20, 60), (64, 48), 32, True)
    plane = (max(shp[1][0], shp2[1][0]), max(shp[1][1], shp2[1][1]))
    assert [c[:5] for c in calls] == [('fmt', 2, (54, 52), nv, None), ('fmt', 1, (54, 52), nv, None), ('fmt', 1, (54, 52), nv709, None),
                                      ('fmt', 1, (36, 52, 2), yu, None), ('fmt', 1, (36, 52), ga, None), ('fmt', 2, (36, 52, 4), bg, None),
                                      ('fmt', 1, (30, 60), nv, None)]
    assert all(c[5:] == (shp[0], plane) for c in calls[:-1]) and calls[-1][5:] == (shp2[0], plane)
    # the call on the converted frames with format=None: same tensor, same shapes
    del calls[:]
    conv = [ref_bgr(f[i], fmts[i]) for i in range(len(f))]
    img0, metas0 = data.prepare_images_device(conv, (64, 48), device='cpu')
    assert torch.equal(img, img0) and metas == metas0 and metas[0]['ori_shape'] == (36, 52, 3) and metas[-1]['ori_shape'] == (20, 60, 3)
    assert {c[0] for c in calls} == {'plain'}
    # one format for all: a name, a stacked batch, a [B][V] sample, with a lens per frame
    del calls[:]
    stacked = np.stack(f[:4])
    img1, m1 = data.prepare_images_device(stacked, (64, 48), device='cpu', format='nv12')
    assert [c[:5] for c in calls] == [('fmt', 4, (54, 52), nv, None)] and img1.shape == (4, 3) + shp[1] and len(m1) == 4
    A, B = TL.to_lens(RL.case_lens('tangential', (36, 52))), TL.to_lens(RL.case_lens('fisheye', (36, 52)))
    del calls[:]
    img2, m2 = data.prepare_images_device([f[:2], [f[3], f[0]]], (64, 48), device='cpu', format=nv, lens=[A, A, B, None])
    assert [c[:5] for c in calls] == [('fmt', 2, (54, 52), nv, A), ('fmt', 1, (54, 52), nv, B), ('fmt', 1, (54, 52), nv, None)]
    assert img2.shape == (2, 2, 3) + shp[1] and len(m2) == 2
    # refusals: per-layout frame shapes, the count, the entries
    with pytest.raises(TypeError, match='nv12'):
        data.prepare_images_device([f[4]], (64, 48), device='cpu', format='nv12')
    with pytest.raises(TypeError, match="'bgr' frames must be"):
        data.prepare_images_device([f[0]], (64, 48), device='cpu', format='bgr')
    with pytest.raises(TypeError, match='uint8'):
        data.prepare_images_device([f[0].astype(np.float32)], (64, 48), device='cpu', format='nv12')
    with pytest.raises(ValueError, match='2 formats for 4 frames'):
        data.prepare_images_device(stacked, (64, 48), device='cpu', format=['nv12', 'nv12'])
    with pytest.raises(ValueError, match='layout'):
        data.prepare_images_device(stacked, (64, 48), device='cpu', format='p010')
    with pytest.raises(TypeError, match=r'\[N,H,W,3\]'):
        data.prepare_images_device(stacked, (64, 48), device='cpu')                 # without format= a 3-D stack is refused as before


def test_public_entries_pass_format_through(monkeypatch):
    """Every public entry has format=None by default, and simple_test_u8(format=) hands the format to prepare_images_device."""
    from imvoxelnet_amd import data, detector, scene
    import inspect
    for fn in (scene.SceneSession.add_views_u8, scene.SceneBatch.add_views_u8, detector.ImVoxelNet.simple_test_u8, data.prepare_images_device):
        assert inspect.signature(fn).parameters['format'].default is None
    seen = {}

    def fake(frames, img_scale, **kw):
        seen.update(kw)
        raise KeyboardInterrupt
    monkeypatch.setattr(data, 'prepare_images_device', fake)
    with pytest.raises(KeyboardInterrupt):
        detector.ImVoxelNet.simple_test_u8(None, [np.zeros((6, 4), np.uint8)], [{}], (64, 48), format='nv12')
    assert seen == dict(format='nv12')
    seen.clear()
    with pytest.raises(KeyboardInterrupt):
        detector.ImVoxelNet.simple_test_u8(None, [np.zeros((4, 4, 3), np.uint8)], [{}], (64, 48))
    assert seen == {}


def test_scene_lens_geometry_takes_the_converted_frames_size():
    """scene._lens_maps (what lens= / depth_frames= of add_views_u8 go through) sizes its maps by the CONVERTED frame: an NV12 array of 54 x 52,
    a YUYV array and a BGR frame of 36 x 52 share one source size; two NV12 arrays of different frames are told apart by their frame sizes."""
    from imvoxelnet_amd import data, scene
    rec = types.SimpleNamespace(_window=None, _decay=None, _gate=None, meta=dict(lidar2img=dict(intrinsic=np.eye(4, dtype=np.float32))))
    lens = data.Lens('brown', np.eye(3), [0.0] * 5)
    z = lambda *s: np.zeros(s, np.uint8)                     # noqa: E731
    frames, fmts = [z(54, 52), z(36, 52, 2), z(36, 52, 3)], ['nv12', 'yuyv', 'bgr']
    lenses, maps = scene._lens_maps([rec], {}, frames, (None, None), lens, None, 0.001, (64, 48), {}, 'session', fmts)
    assert lenses == [lens] * 3 and maps == (None, None)
    with pytest.raises(ValueError, match=r'share one source size in a call, got \[\(30, 60\), \(36, 52\)\]'):
        scene._lens_maps([rec], {}, [z(54, 52), z(45, 60)], (None, None), lens, None, 0.001, (64, 48), {}, 'session', 'nv12')
    with pytest.raises(ValueError, match=r'got \[\(36, 52\), \(54, 52\)\]'):                   # without format= the array shape is the frame's
        scene._lens_maps([rec], {}, frames[:2], (None, None), lens, None, 0.001, (64, 48), {}, 'session')
    with pytest.raises(TypeError, match='nv12'):
        scene._lens_maps([rec], {}, [z(36, 52, 3)], (None, None), lens, None, 0.001, (64, 48), {}, 'session', 'nv12')
