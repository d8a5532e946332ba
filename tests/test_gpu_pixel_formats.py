"""-m gpu: decoder pixel formats in the device image pipeline (include/imvoxel.h 0.5.3 ivx_image_prep_fmt_u8, csrc/image_prep.hip, csrc/pixel_fetch.h;
ops.image_prep_fmt_u8, data.prepare_images_device(format=), the format= keyword of simple_test_u8 and of the scenes).  A frame in any layout IS
a BGR frame through the header's integer rule (tests/ref_pixfmt.py restates it independently), and the result is the existing entry on that
BGR frame: every comparison is torch.equal / ==, there is NO tolerance.  All inputs are uniform random bytes from fixed seeds; surfaces are
handed over raw (flat bytes plus pitches and offsets, gaps filled with 0xFF) because that is the most general thing the entry takes, and every
case runs once from an aligned base pointer (the 2- / 4-byte loads of NV12 / YUYV / BGRA / RGBA, where pitch and offset allow them) and once
from a base one byte further (the byte-load fallback)."""
import ctypes as C

import numpy as np
import pytest
import torch

import ref_lens as RL
import ref_pixfmt as P
from test_host_lens_prep import to_lens

pytestmark = pytest.mark.gpu

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
CUSTOM = (255, P.COEF_MAX, P.COEF_MAX, -P.COEF_MAX, -P.COEF_MAX, P.COEF_MAX)          # every coefficient on the int32 bound, y_off at its top
CUSTOM_NEG = (0, P.COEF_MAX, -P.COEF_MAX, P.COEF_MAX, P.COEF_MAX, -P.COEF_MAX)       # ... and the largest yy the rule can form


@pytest.fixture(scope='module')
def ops():
    from imvoxelnet_amd import _lib, ops
    _lib.lib()
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    return ops


def _nan_out(n, pad, unaligned=False):
    """A NaN-filled fp32 [n,3,ph,pw] on the device; unaligned: 4 bytes past a 16-byte boundary (the scalar store path)."""
    numel = n * 3 * pad[0] * pad[1]
    base = torch.full((numel + 4,), float('nan'), device='cuda')
    assert base.data_ptr() % 16 == 0
    out = base[1:1 + numel].view(n, 3, *pad) if unaligned else base[:numel].view(n, 3, *pad)
    assert (out.data_ptr() % 16 != 0) == unaligned
    return out


def _fmt(layout, m):
    from imvoxelnet_amd import data
    return data.FrameFormat(layout, yuv=m) if layout in P.YUV else data.FrameFormat(layout)


def _device_surfaces(bufs, lead, gap):
    """n flat frames of one size as a device [n, size] view: frame stride size + gap, the first byte `lead` bytes past a 256-byte boundary;
    every byte outside the frames is 0xFF."""
    n, size = len(bufs), bufs[0].size
    step = size + gap
    host = np.full(lead + n * step, 0xFF, np.uint8)
    for i, b in enumerate(bufs):
        host[lead + i * step:lead + i * step + size] = b
    dev = torch.from_numpy(host).cuda()
    assert dev.data_ptr() % 256 == 0
    return dev[lead:].as_strided((n, size), (step, 1))


def _case(ops, layout, src, dst, pad, seed, n=3, m=P.BT601_LIMITED, pitch=None, p1_pitch=None, gap_rows=0, unaligned_out=False, lens=None, info=None,
          leads=(0, 1), to_rgbs=(1, 0), check_host=True):
    """n random surfaces of one geometry through ivx_image_prep_fmt_u8 == the BGR entry on the reference conversion (== data.prepare_image of it,
    without a lens), for both values of to_rgb, from an aligned and from a misaligned base pointer.  -> the reference BGR frames."""
    from imvoxelnet_amd import data
    rng = np.random.default_rng(seed)
    h, w = src
    made = [P.surface(rng, layout, h, w, row_bytes=pitch, plane1_row_bytes=p1_pitch, gap_rows=gap_rows) for _ in range(n)]
    geom = made[0][1]
    infos = [dict() for _ in range(n)]
    bgr = np.stack([P.to_bgr(b, layout, h, w, m=m, info=i, **geom) for (b, _), i in zip(made, infos)])
    if info is not None and layout in P.YUV:
        for k in infos[0]:
            info[k] = info.get(k, 0) + sum(i[k] for i in infos)
    ref_dev = torch.from_numpy(bgr).cuda()
    size = made[0][0].size
    for to_rgb in to_rgbs:
        if lens is None:
            want = ops.image_prep_u8(ref_dev, dst, pad, MEAN, STD, to_rgb)
        else:
            want = ops.image_prep_lens_u8(ref_dev, lens, dst, pad, MEAN, STD, to_rgb)
        assert not torch.isnan(want).any()
        if lens is None and check_host:
            for i in range(n):
                t, _ = data.prepare_image(bgr[i], (dst[1], dst[0]), dict(mean=MEAN, std=STD, to_rgb=bool(to_rgb)), size_divisor=1, keep_ratio=False)
                full = torch.zeros(3, *pad)
                full[:, :dst[0], :dst[1]] = t
                assert torch.equal(want[i].cpu(), full), (layout, src, dst, i)
        for lead in leads:
            gap = (-size) % 4 + 8                            # a frame stride that is a multiple of 4 and larger than the frame
            dev = _device_surfaces([b for b, _ in made], lead, gap)
            out = _nan_out(n, pad, unaligned_out)
            res = ops.image_prep_fmt_u8(dev if n > 1 else dev[0], _fmt(layout, m), dst, pad, MEAN, STD, to_rgb, lens=lens, out=out, src_hw=src, **geom)
            assert res is out and torch.equal(out.view(torch.int32), want.view(torch.int32)), (layout, src, dst, pad, to_rgb, lead)
    return bgr


def _assert_every_branch(info):
    """Uniform random bytes hit every branch of the YUV rule -- pixels clamped at 0, at 255, Y below y_off, exactly one channel saturating:
    keep that from silently stopping."""
    assert all(info[k] > 0 for k in ('clamped_0', 'clamped_255', 'y_below', 'one_saturates')), info


PLAIN = {                                                     # (source, dst, pad, unaligned out)
    'copy': ((5, 7), (5, 7), (32, 32), False),
    'half': ((10, 14), (5, 7), (32, 32), False),
    'down': ((9, 13), (5, 7), (32, 32), False),
    'up': ((5, 7), (11, 17), (32, 32), False),
    'scalar_store': ((9, 13), (5, 7), (32, 30), False),        # pad_w % 4 != 0: no 16-byte stores
    'scalar_store_copy': ((5, 7), (5, 7), (8, 30), False),
    'misaligned_out': ((10, 14), (5, 7), (32, 32), True),
    'wide_copy': ((6, 70), (6, 70), (32, 96), False),          # several work items per row, the last one ragged (70 = 17 * 4 + 2)
    'wide_half': ((12, 140), (6, 70), (32, 96), False),
}


@pytest.mark.parametrize('case', list(PLAIN))
@pytest.mark.parametrize('layout', P.LAYOUTS)
def test_plain_path_equals_the_bgr_entry_on_the_converted_frames(ops, layout, case):
    src, dst, pad, unaligned = PLAIN[case]
    info = {}
    _case(ops, layout, src, dst, pad, seed=100 + list(PLAIN).index(case), unaligned_out=unaligned, info=info)
    if layout in P.YUV:
        _assert_every_branch(info)


@pytest.mark.parametrize('layout', P.LAYOUTS)
def test_smallest_odd_sizes(ops, layout):
    """The last chroma row / column belongs to one pixel; copy mode and the linear mode (an up-scale), one frame and three."""
    for k, src in enumerate(((1, 1), (1, 2), (2, 1), (3, 3))):
        _case(ops, layout, src, src, (4, 4), seed=200 + k, n=1)
        _case(ops, layout, src, (4, 5), (32, 32), seed=210 + k, n=3)
    _case(ops, layout, (2, 2), (1, 1), (4, 4), seed=220, n=2)            # the smallest exact half


@pytest.mark.parametrize('layout,pitch,p1', [('nv12', 5, 3), ('nv12', 6, 4), ('yuyv', 3, None), ('yuyv', 4, None), ('bgra', 1, None), ('bgra', 4, None),
                                             ('rgba', 3, None), ('gray', 3, None), ('rgb', 2, None), ('bgr', 1, None)])
def test_pitch_and_plane_offset(ops, layout, pitch, p1):
    """Pitches above the row (odd ones: no wide load is aligned; multiples of the access size: they are), the UV plane two pitch-rows past the Y plane;
    the gaps hold 0xFF, so a wrong address shows."""
    for k, (src, dst) in enumerate((((9, 13), (9, 13)), ((10, 14), (5, 7)), ((9, 13), (5, 7)))):
        h, w = src
        kw = dict(pitch=P.min_row_bytes(layout, w) + pitch)
        if layout == 'nv12':
            kw.update(p1_pitch=2 * ((w + 1) // 2) + p1, gap_rows=2)
        info = {}
        _case(ops, layout, src, dst, (32, 32), seed=300 + k, info=info, **kw)
        if layout in P.YUV:
            _assert_every_branch(info)


def test_nv12_uv_plane_at_an_odd_address_takes_byte_loads(ops):
    """src + plane1_offset odd with an even UV pitch: only the host's alignment check keeps the 2-byte loads away."""
    rng = np.random.default_rng(310)
    h, w = 9, 13
    buf, geom = P.surface(rng, 'nv12', h, w, row_bytes=w + 2, plane1_row_bytes=14, gap_rows=1)
    assert geom['plane1_offset'] % 2 == 0 and geom['plane1_row_bytes'] % 2 == 0
    info = {}
    bgr = P.to_bgr(buf, 'nv12', h, w, m=P.BT601_LIMITED, info=info, **geom)
    _assert_every_branch(info)
    want = ops.image_prep_u8(torch.from_numpy(bgr)[None].cuda(), (9, 13), (32, 32), MEAN, STD, True)
    dev = _device_surfaces([buf], 1, 8)[0]
    assert (dev.data_ptr() + geom['plane1_offset']) % 2 == 1
    out = ops.image_prep_fmt_u8(dev, 'nv12', (9, 13), (32, 32), MEAN, STD, True, out=_nan_out(1, (32, 32)), src_hw=(h, w), **geom)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize('layout', P.YUV)
@pytest.mark.parametrize('name', ['bt601', 'bt601_full', 'bt709', 'bt709_full', 'custom', 'custom_neg'])
def test_coefficients(ops, layout, name):
    """The four named matrices (as ivx_yuv_matrix gives them) and custom ones with every coefficient at +-(3 << 20): the int32 bound itself;
    the reference asserts in Python ints that no intermediate reaches 2^31."""
    from imvoxelnet_amd import _lib
    if name.startswith('custom'):
        m = CUSTOM if name == 'custom' else CUSTOM_NEG
        assert P.assert_in_int32(m) > (2 ** 29 if name == 'custom' else 2 ** 30)       # (y_off = 255 leaves the chroma terms alone: 768 * 2^20)
    else:
        f = _lib.FrameFormat()
        assert _lib.lib().ivx_yuv_matrix(int(name.startswith('bt709')), int(name.endswith('full')), C.byref(f)) == 0
        m = (f.y_off, f.cy, f.cub, f.cug, f.cvg, f.cvr)
        assert m == P.matrix(name[:5], name.endswith('full'))
    info = {}
    for k, (src, dst) in enumerate((((9, 13), (9, 13)), ((10, 14), (5, 7)), ((9, 13), (5, 7)))):
        _case(ops, layout, src, dst, (32, 32), seed=400 + k, m=m, info=info, to_rgbs=(1,))
    assert info['clamped_0'] > 0 and info['clamped_255'] > 0 and info['one_saturates'] > 0, info
    assert info['y_below'] > 0 or m[0] == 0, info                      # (no byte is below a y_off of 0)


@pytest.mark.parametrize('lens_name', ['pincushion', 'barrel', 'tangential', 'fisheye'])
@pytest.mark.parametrize('layout', ['nv12', 'yuyv', 'bgra'])
def test_lens_path_equals_the_lens_entry_on_the_converted_frames(ops, layout, lens_name):
    src, dst, pad = (9, 13), (8, 12), (32, 32)
    L = RL.case_lens(lens_name, src)
    x, y = RL.grid(dst)
    inside = RL.G(L, src, dst, x, y)[3]
    if lens_name in ('pincushion', 'barrel'):                # strong enough that some pixels of the input are border
        assert 0 < int(inside.sum()) < inside.size
    info = {}
    _case(ops, layout, src, dst, pad, seed=500, lens=to_lens(L), info=info)
    _case(ops, layout, src, dst, (8, 14), seed=501, lens=to_lens(L), unaligned_out=True, n=1)          # scalar stores
    if layout in P.YUV:
        _assert_every_branch(info)


def test_capped_grid_writes_every_element(ops):
    """One NV12 frame of 1100 x 2000 copied: 1100 * 500 work items are more than the 2048 x 256 threads of the capped grid."""
    h, w = 1100, 2000
    assert h * (w // 4) > 2048 * 256
    buf, geom = P.surface(np.random.default_rng(600), 'nv12', h, w)
    info = {}
    bgr = P.to_bgr(buf, 'nv12', h, w, m=P.BT601_LIMITED, info=info, **geom)
    _assert_every_branch(info)
    want = ops.image_prep_u8(torch.from_numpy(bgr)[None].cuda(), (h, w), (h, w), MEAN, STD, True)
    stacked = torch.from_numpy(P.tight(buf, 'nv12', h, w, geom))[None].cuda()
    out = ops.image_prep_fmt_u8(stacked, 'nv12', (h, w), (h, w), MEAN, STD, True, out=_nan_out(1, (h, w)))
    assert not torch.isnan(out).any() and torch.equal(out.view(torch.int32), want.view(torch.int32))


def test_the_usual_arrays_equal_the_raw_surface(ops):
    """[n,H,W,C], [n,H,W] gray, the stacked NV12 array and [n,H,2*ceil(W/2),2] YUYV (with src_hw for an odd W), through a strided batch view."""
    rng = np.random.default_rng(610)
    for layout in P.LAYOUTS:
        for (h, w) in ((6, 8), (5, 7)):
            if layout == 'nv12' and w % 2:
                continue                                     # (an odd-width NV12 surface is a raw surface: its planes have different pitches)
            made = [P.surface(rng, layout, h, w) for _ in range(2)]
            infos = [dict(), dict()]
            bgr = np.stack([P.to_bgr(b, layout, h, w, m=P.BT601_LIMITED, info=i, **g) for (b, g), i in zip(made, infos)])
            if layout in P.YUV:                              # (over the two frames of the case: 35 .. 48 pixels each)
                _assert_every_branch({k: infos[0][k] + infos[1][k] for k in infos[0]})
            want = ops.image_prep_u8(torch.from_numpy(bgr).cuda(), (7, 9), (32, 32), MEAN, STD, True)
            arr = np.stack([P.tight(b, layout, h, w, g) for b, g in made])
            big = torch.zeros((3,) + arr.shape[1:], dtype=torch.uint8)
            big[::2] = torch.from_numpy(arr)
            out = ops.image_prep_fmt_u8(big.cuda()[::2], layout, (7, 9), (32, 32), MEAN, STD, True, out=_nan_out(2, (32, 32)), src_hw=(h, w))
            assert torch.equal(out.view(torch.int32), want.view(torch.int32)), (layout, h, w)


# ------------------------------------------------------------------ the BGR entries keep their bits
# Since 0.5.3 ivx_image_prep_u8 / ivx_image_prep_lens_u8 launch the BGR8 instantiation of the templated kernels.  Their outputs on seeded frames
# were recorded from the 0.5.2 kernels, on the device, before that change (tests/golden/image_prep_bgr_0_5_2.npz): the bits must stay.
GOLDEN = {'copy': ((5, 7), (5, 7), (32, 32), None), 'half': ((10, 14), (5, 7), (32, 32), None), 'down': ((9, 13), (5, 7), (32, 32), None),
          'up': ((5, 7), (11, 17), (32, 32), None), 'scalar': ((9, 13), (5, 7), (8, 30), None), 'big_down': ((37, 53), (23, 31), (32, 32), None),
          'lens_pincushion': ((9, 13), (8, 12), (32, 32), 'pincushion'), 'lens_fisheye': ((9, 13), (8, 12), (32, 32), 'fisheye'),
          'lens_tangential': ((37, 53), (23, 31), (32, 32), 'tangential'), 'lens_barrel_scalar': ((37, 53), (23, 31), (24, 34), 'barrel')}


def golden_outputs(ops):
    """{case: the BGR entry's output [2,3,ph,pw] as a numpy array, to_rgb on} on the seeded frames of ref_lens.frames."""
    res = {}
    for k, (name, (src, dst, pad, lens_name)) in enumerate(GOLDEN.items()):
        f = torch.from_numpy(RL.frames(800 + k, 2, src)).cuda()
        if lens_name is None:
            out = ops.image_prep_u8(f, dst, pad, MEAN, STD, True, out=_nan_out(2, pad))
        else:
            out = ops.image_prep_lens_u8(f, to_lens(RL.case_lens(lens_name, src)), dst, pad, MEAN, STD, True, out=_nan_out(2, pad))
        res[name] = out.cpu().numpy()
    return res


def test_bgr_entries_keep_the_bits_of_0_5_2(ops):
    import os
    from helpers import ROOT
    gold = np.load(os.path.join(ROOT, 'tests', 'golden', 'image_prep_bgr_0_5_2.npz'))
    got = golden_outputs(ops)
    assert sorted(gold.files) == sorted(got)
    for name, g in got.items():
        assert g.dtype == np.float32 and np.array_equal(g.view(np.int32), gold[name].view(np.int32)), name


# ------------------------------------------------------------------ refusals
def test_every_refusal_leaves_out_untouched(ops):
    from imvoxelnet_amd import _lib
    from test_host_pixel_formats import entry_call, entry_cases
    src = torch.zeros(1 << 16, dtype=torch.uint8, device='cuda')
    out = torch.full((2, 3, 32, 32), float('nan'), device='cuda')
    cases = entry_cases()
    assert len(cases) > 30
    for kw, needle in cases:
        rc, msg = entry_call(C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr()), **kw)
        assert rc == -1 and b'ivx_image_prep_fmt_u8' in msg and needle in msg, (kw, msg)
    # through the op: the library's refusal arrives as a ValueError with its message
    with pytest.raises(ValueError, match='plane1_offset 44 is below src_h'):
        _lib.check(entry_call(C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr()), f=_struct(plane1_offset=44))[0], 'ivx_image_prep_fmt_u8')
    with pytest.raises(ValueError, match='pad 4 x 4 is smaller than dst'):
        ops.image_prep_fmt_u8(src[:96].view(1, 12, 8), 'nv12', (8, 8), (4, 4), MEAN, STD, out=out[:1, :, :4, :4].contiguous())
    with pytest.raises(ValueError, match='std'):
        ops.image_prep_fmt_u8(src[:96].view(1, 12, 8), 'nv12', (8, 8), (32, 32), MEAN, (1, 0, 1), out=out[:1])
    with pytest.raises(ValueError, match='does not cover the last plane'):
        ops.image_prep_fmt_u8(src[:208].view(2, 104), 'nv12', (8, 8), (32, 32), MEAN, STD, out=out, src_hw=(8, 8), row_bytes=8, plane1_offset=66,
                              plane1_row_bytes=10)         # (the last UV row's payload ends at byte 104, the plane at 106)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


def _struct(**kw):
    from test_host_pixel_formats import _fmt_struct
    return _fmt_struct(**kw)


# ------------------------------------------------------------------ the public surface
SRC, SCALE, SIZE, PAD = (180, 250), (128, 96), (92, 128), (96, 128)


def _nv12_frames(seed, n, hw):
    """n stacked NV12 arrays of hw (even width) and the BGR frames they are."""
    rng = np.random.default_rng(seed)
    h, w = hw
    made = [P.surface(rng, 'nv12', h, w) for _ in range(n)]
    infos = [dict() for _ in made]
    bgr = [P.to_bgr(b, 'nv12', h, w, m=P.BT601_LIMITED, info=i, **g) for (b, g), i in zip(made, infos)]
    for i in infos:
        _assert_every_branch(i)
    return [P.tight(b, 'nv12', h, w, g) for b, g in made], bgr


def test_prepare_images_device_with_a_format_equals_the_call_on_the_converted_frames(ops):
    from imvoxelnet_amd import data
    a, a_bgr = _nv12_frames(700, 3, (36, 52))
    b, b_bgr = _nv12_frames(701, 2, (30, 60))
    mixed, conv = [a[0], b[0], a[1], a[2], b[1]], [a_bgr[0], b_bgr[0], a_bgr[1], a_bgr[2], b_bgr[1]]
    img, metas = data.prepare_images_device(mixed, (64, 48), format='nv12')
    img0, metas0 = data.prepare_images_device(conv, (64, 48))
    assert torch.equal(img.view(torch.int32), img0.view(torch.int32)) and metas == metas0
    # per-frame formats, device tensors, a lens per frame
    rng = np.random.default_rng(702)
    yb, yg = P.surface(rng, 'yuyv', 36, 52)
    gb, gg = P.surface(rng, 'gray', 36, 52)
    frames = [a[0], torch.from_numpy(P.tight(yb, 'yuyv', 36, 52, yg)).cuda(), P.tight(gb, 'gray', 36, 52, gg), a_bgr[1]]
    conv = [a_bgr[0], P.to_bgr(yb, 'yuyv', 36, 52, m=P.matrix('bt709', True), **yg), P.to_bgr(gb, 'gray', 36, 52, **gg), a_bgr[1]]
    fmts = ['nv12', data.FrameFormat('yuyv', 'bt709', full_range=True), 'gray', 'bgr']
    lens = [to_lens(RL.case_lens('pincushion', (36, 52))), None, to_lens(RL.case_lens('fisheye', (36, 52))), None]
    img, metas = data.prepare_images_device(frames, (64, 48), format=fmts, lens=lens)
    img0, metas0 = data.prepare_images_device(conv, (64, 48), lens=lens)
    assert torch.equal(img.view(torch.int32), img0.view(torch.int32)) and metas == metas0


@pytest.fixture(scope='module')
def z(ops):
    import imvoxelnet_amd
    from imvoxelnet_amd import data
    from test_gpu_scene_window import _family
    z = _family(imvoxelnet_amd, 'indoor')
    K = z['scene_meta']['lidar2img']['intrinsic']
    z['user'] = {k: v for k, v in z['scene_meta'].items() if k not in ('img_shape', 'ori_shape', 'pad_shape')}
    z['lens'] = data.Lens('brown', [[230.3, 0, 66.2], [0, 231.1, 45.1], [0, 0, 1]], [0.35, 0.012, 0.0011, -0.0006, 0], new_K=K[:3, :3])
    assert data._pipeline_shapes(SRC, SCALE, 32, True) == (SIZE, PAD)
    z['nv12'], z['bgr'] = _nv12_frames(710, 4, SRC)
    return z


def _same_results(res, ref):
    assert len(res) == len(ref)
    for a, b in zip(res, ref):
        assert torch.equal(a['scores_3d'], b['scores_3d']) and torch.equal(a['labels_3d'], b['labels_3d'])
        assert torch.equal(a['boxes_3d'].tensor, b['boxes_3d'].tensor) and type(a['boxes_3d']) is type(b['boxes_3d'])


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16) if t.dtype in (torch.bfloat16, torch.float16) else t


def _same_volume(a, b):
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1]) and 0 < int(a[1].sum()) < a[1].numel()


@pytest.mark.parametrize('with_lens', [False, True])
def test_simple_test_u8_with_a_format(z, with_lens):
    model, E = z['model'], z['E']
    meta = dict(z['user'], lidar2img=dict(z['user']['lidar2img'], extrinsic=list(E[:4])))
    kw = dict(lens=z['lens']) if with_lens else {}
    ref = model.simple_test_u8([z['bgr']], [meta], SCALE, **kw)
    res = model.simple_test_u8([z['nv12']], [meta], SCALE, format='nv12', **kw)
    _same_results(res, ref)
    res = model.simple_test_u8([[torch.from_numpy(f).cuda() for f in z['nv12']]], [meta], SCALE, format=['nv12'] * 4, **kw)
    _same_results(res, ref)


@pytest.mark.parametrize('with_lens', [False, True])
def test_session_add_views_u8_with_a_format(z, with_lens):
    model, E = z['model'], z['E']
    kw = dict(lens=z['lens']) if with_lens else {}
    open_kw = dict(decay=1.0) if with_lens else {}               # (a session that takes maps: the cover of the lens joins the weights)
    a, b = model.open_scene(z['user'], **open_kw), model.open_scene(z['user'], **open_kw)
    for lo, hi in ((0, 1), (1, 4)):
        a.add_views_u8(z['nv12'][lo:hi], E[lo:hi], SCALE, format='nv12', **kw)
        b.add_views_u8(z['bgr'][lo:hi], E[lo:hi], SCALE, **kw)
    _same_volume(a.volume(), b.volume())
    assert a.meta['ori_shape'] == SRC + (3,) == b.meta['ori_shape'] and a.meta['img_shape'] == b.meta['img_shape']
    _same_results(a.detect(), b.detect())
    a.close()
    b.close()


@pytest.mark.parametrize('with_lens', [False, True])
def test_batch_add_views_u8_with_a_format(z, with_lens):
    model, E = z['model'], z['E']
    kw = dict(lens=z['lens']) if with_lens else {}
    open_kw = dict(decay=1.0) if with_lens else {}
    a, b = model.open_scenes([z['user'], z['user']], **open_kw), model.open_scenes([z['user'], z['user']], **open_kw)
    scene = [1, 0, 1, 1]
    a.add_views_u8(z['nv12'], E[:4], scene, SCALE, format='nv12', **kw)
    b.add_views_u8(z['bgr'], E[:4], scene, SCALE, **kw)
    for s in (0, 1):
        _same_volume(a.volume(s), b.volume(s))
    res, ref = a.detect(), b.detect()
    assert len(ref) == 2
    _same_results(res, ref)
    a.close()
    b.close()
