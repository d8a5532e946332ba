"""-m gpu: the lens-aware image pipeline (ops.image_prep_lens_u8 / ops.map_prep_lens, csrc/image_prep.hip) against the numpy fp64 references of
tests/ref_lens.py, and the lens= / depth_frames= keywords of the streaming scenes against sessions that are handed the same images and maps.

The image bound.  The header fixes the blend: fu, fv are fractions rounded once to fp32 (|error| <= 2^-25 each); top = a + fu * (b - a), bot likewise,
val = top + fv * (bot - top), out = (val - mean) / std, every operation rounded to fp32 on its own.  With the unit U = 2^-24 * 255 (a half-ulp rounding
of a quantity of at most 255 grey levels): b - a is exact (integers); the rounding of fu moves top by at most U / 2, the product and the sum by U each:
top and bot are within 2.5 U.  val is a convex combination of them (2.5 U carried), plus the roundings of bot - top (U, times fv <= 1), of fv itself
(U / 2), of the product (U) and of the sum (U): 6 U.  val - mean rounds once more (|val - mean| <= 255): 7 U; K = 8 leaves one unit for magnitudes that
rounding pushed past 255.  The divide adds 2^-24 * |out|.  The fp64 coordinates of the kernel and of numpy follow one operation order; what remains
(atan, a few ulp) is below COORD_EPS = 1e-9 px, worth 2 * 255 * 1e-9 grey levels.  So
    |out - ref| <= (8 * 2^-24 * 255 + 2 * 255 * 1e-9) / |std| + 2^-24 * |ref|                                         (ref_lens.image_tolerance).
Every decision (inside / border, the nearest pixel) is far from its threshold in every case (tests/test_host_lens_prep.py asserts the margins), so
border pixels are compared exactly.  Worst measured |out - ref| / bound over all image cases on an MI355X: 0.263 (the 6 x 384 x 1280 case; the small
cases 0.12 .. 0.23), also recorded in profiles/image_prep_lens.md; every test prints its own figure before it asserts."""
import numpy as np
import pytest
import torch

import ref_lens as R
from test_host_lens_prep import from_lens, to_lens

pytestmark = pytest.mark.gpu

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
WORST = {'ratio': 0.0}


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


def _check_image(out, f, L, dst, pad, to_rgb, mean=MEAN, std=STD):
    """One frame of the device's output against the fp64 reference: the bound inside, +0.0f bits on border and pad, no NaN."""
    ref, mask = R.image(f, L, dst, pad, mean, std, to_rgb)
    got = out.cpu()
    assert not torch.isnan(got).any(), 'an element of out was not written'
    bits = got.view(torch.int32).numpy()
    assert (bits[:, ~mask] == 0).all(), 'border and pad pixels must be +0.0f'
    err = np.abs(got.numpy().astype(np.float64) - ref)
    ratio = float((err / R.image_tolerance(ref, std)).max())
    WORST['ratio'] = max(WORST['ratio'], ratio)
    print(f'worst |out - ref| / bound = {ratio:.3f}, inside {int(mask.sum())} of {dst[0] * dst[1]}')
    assert ratio <= 1.0, ratio
    return ratio, mask


@pytest.mark.parametrize('shape', list(R.SHAPES))
@pytest.mark.parametrize('lens_name', R.LENSES)
def test_image_entry_against_fp64(ops, shape, lens_name):
    src, dst, pad, unaligned = R.SHAPES[shape]
    L = R.case_lens(lens_name, src)
    f = R.frames(sorted(R.SHAPES).index(shape) * 10 + R.LENSES.index(lens_name), 1, src)
    masks = []
    for to_rgb in (True, False):
        out = _nan_out(1, pad, unaligned)
        res = ops.image_prep_lens_u8(torch.from_numpy(f).cuda(), to_lens(L), dst, pad, MEAN, STD, to_rgb, out=out)
        assert res is out
        ratio, mask = _check_image(out[0], f[0], L, dst, pad, to_rgb)
        masks.append(mask)
    if lens_name != 'tangential':
        assert 0 < masks[0].sum() < dst[0] * dst[1], 'the case has border pixels inside the resized region'


def test_image_entry_equal_size_with_a_zero_lens(ops):
    """The ideal camera written as a lens at the equal size: every pixel is its source pixel (fractions of 0 or 1 - 1e-14: the blend is continuous)."""
    src, dst, pad = R.EQUAL
    L = R.case_lens('zero', src)
    f = R.frames(77, 1, src)
    out = _nan_out(1, pad)
    ops.image_prep_lens_u8(torch.from_numpy(f).cuda(), to_lens(L), dst, pad, MEAN, STD, True, out=out)
    ratio, mask = _check_image(out[0], f[0], L, dst, pad, True)
    assert mask[:dst[0], :dst[1]].all()
    want = (torch.from_numpy(f[0][..., ::-1].copy()).float().permute(2, 0, 1) - torch.tensor(MEAN).view(3, 1, 1)) / torch.tensor(STD).view(3, 1, 1)
    assert (out[0, :, :dst[0], :dst[1]].cpu() - want).abs().max() <= 2.0 ** -22 * 255 / min(STD)


def test_image_entry_batch_through_a_strided_source_view(ops):
    """n = 3 frames read through a row-strided, frame-strided, non-contiguous view; the default output allocation."""
    src, dst, pad, _ = R.SHAPES['vector']
    L = R.case_lens('new_k', src)
    f = R.frames(78, 3, src)
    buf = torch.randint(0, 256, (3, src[0] + 2, src[1] + 5, 3), dtype=torch.uint8)
    buf[:, :src[0], :src[1]] = torch.from_numpy(f)
    view = buf.cuda()[:, :src[0], :src[1]]
    assert not view.is_contiguous()
    out = ops.image_prep_lens_u8(view, to_lens(L), dst, pad, MEAN, STD, True)
    assert out.shape == (3, 3) + pad
    for i in range(3):
        _check_image(out[i], f[i], L, dst, pad, True)


def test_image_entry_grid_stride_loop(ops):
    """6 frames at 384 x 1280: 6 * 384 * 320 work items, more than the capped grid of 2048 x 256 threads, so the loop strides.  The batch equals the
    per-frame calls bit for bit, and one frame meets the fp64 bound."""
    src, dst, pad, n = R.BIG
    assert n * pad[0] * (pad[1] // 4) > 2048 * 256
    L = R.case_lens(R.BIG_LENS, src)
    f = R.frames(79, n, src)
    dev = torch.from_numpy(f).cuda()
    out = _nan_out(n, pad)
    ops.image_prep_lens_u8(dev, to_lens(L), dst, pad, MEAN, STD, True, out=out)
    for i in range(n):
        assert torch.equal(ops.image_prep_lens_u8(dev[i:i + 1], to_lens(L), dst, pad, MEAN, STD, True)[0], out[i]), i
    _check_image(out[4], f[4], L, dst, pad, True)


def test_worst_measured_ratio_is_reported():
    print(f'worst |out - ref| / bound over the image cases of this run: {WORST["ratio"]:.3f}')
    assert WORST['ratio'] <= 1.0


# ------------------------------------------------------------------ the map entry: pinned with ==
@pytest.mark.parametrize('shape', list(R.MAP_SHAPES))
@pytest.mark.parametrize('lens_name', R.MAP_LENSES)
def test_map_entry_equals_the_reference(ops, shape, lens_name):
    src, dst, pad = R.MAP_SHAPES[shape]
    L = None if lens_name is None else R.case_lens(lens_name, src)
    lens = None if L is None else to_lens(L)
    rng = np.random.default_rng(5)
    d16 = rng.integers(0, 6000, (2,) + src).astype(np.uint16)
    d16[:, ::3, ::2] = 0                                             # no measurement: zeros stay zero
    d32 = rng.uniform(0.3, 5.0, (2,) + src).astype(np.float32)
    for stride in R.STRIDES:
        fhw = ((pad[0] - 1) // stride + 1, (pad[1] - 1) // stride + 1)
        want = R.cover(L, src, dst, pad, stride)
        assert want.shape == fhw
        out = torch.full((3,) + fhw, float('nan'), device='cuda')
        assert ops.map_prep_lens(dst, pad, src, lens, stride=stride, n=3, out=out) is out
        for i in range(3):
            assert np.array_equal(out[i].cpu().numpy(), want), (stride, i)
        got = ops.map_prep_lens(dst, pad, src, lens, src=torch.from_numpy(d16).cuda(), scale=0.001, stride=stride)
        assert got.shape == (2,) + fhw and got.dtype == torch.float32
        for i in range(2):
            ref = R.picked(d16[i], L, dst, pad, 0.001, stride)
            assert np.array_equal(got[i].cpu().numpy(), ref) and (ref[want == 0] == 0).all() and ref.max() > 1.0, (stride, i)
        # float32 maps through a row-strided, non-contiguous view, into a NaN-filled out
        buf = torch.zeros(2, src[0] + 1, src[1] + 3)
        buf[:, :src[0], :src[1]] = torch.from_numpy(d32)
        out = torch.full((2,) + fhw, float('nan'), device='cuda')
        ops.map_prep_lens(dst, pad, src, lens, src=buf.cuda()[:, :src[0], :src[1]], scale=1.7, stride=stride, out=out)
        for i in range(2):
            assert np.array_equal(out[i].cpu().numpy(), R.picked(d32[i], L, dst, pad, 1.7, stride)), (stride, i)


@pytest.mark.parametrize('lens_name', ['barrel', 'pincushion', 'ring', 'fisheye'])
def test_cover_is_where_the_image_entry_wrote_the_frame(ops, lens_name):
    """On a source without mean-coloured pixels (values 1 .. 255, mean 0) an inside pixel of the image entry is never 0, so the cover map equals
    (image != 0).any(channel)[::s, ::s] of the image entry's own output."""
    src, dst, pad = R.MAP_SHAPES['ragged']
    lens = to_lens(R.case_lens(lens_name, src))
    f = torch.from_numpy(np.random.default_rng(6).integers(1, 256, (1,) + src + (3,), dtype=np.uint8)).cuda()
    img = ops.image_prep_lens_u8(f, lens, dst, pad, (0, 0, 0), (1, 1, 1), True)[0]
    shown = (img != 0).any(0)
    assert 0 < int(shown.sum()) < dst[0] * dst[1]
    for stride in R.STRIDES:
        cover = ops.map_prep_lens(dst, pad, src, lens, stride=stride)[0]
        assert torch.equal(cover, shown[::stride, ::stride].float()), stride


# ------------------------------------------------------------------ the scenes
SRC, SCALE, SIZE, PAD = (180, 250), (128, 96), (92, 128), (96, 128)       # (no exact ratio: the nearest pick of an ideal camera at 2 : 1 would sit on ties)


@pytest.fixture(scope='module')
def z(ops):
    import imvoxelnet_amd
    from imvoxelnet_amd import data
    from test_gpu_scene_window import _family
    z = _family(imvoxelnet_amd, 'indoor')
    K = z['scene_meta']['lidar2img']['intrinsic']
    z['user'] = {k: v for k, v in z['scene_meta'].items() if k not in ('img_shape', 'ori_shape', 'pad_shape')}
    z['shapes'] = dict(img_shape=SIZE + (3,), ori_shape=SRC + (3,), pad_shape=PAD + (3,))
    # a pincushion lens whose ideal camera is the meta's intrinsic: the right and lower parts of the input are border
    z['lens'] = data.Lens('brown', [[230.3, 0, 66.2], [0, 231.1, 45.1], [0, 0, 1]], [0.35, 0.012, 0.0011, -0.0006, 0], new_K=K[:3, :3])
    assert data._pipeline_shapes(SRC, SCALE, 32, True) == (SIZE, PAD)
    z['frames'] = R.frames(90, 4, SRC)
    norm = data.IMG_NORM_CFG
    z['imgs'] = ops.image_prep_lens_u8(torch.from_numpy(z['frames']).cuda(), z['lens'], SIZE, PAD, norm['mean'], norm['std'], norm['to_rgb'])
    z['cover'] = ops.map_prep_lens(SIZE, PAD, SRC, z['lens'])[0]
    for L in (from_lens(z['lens']), None):
        assert R.margins(L, SRC, SIZE, pick=True, stride=4, pad_hw=PAD) == dict(edge=0, ring=0, half=0)
    assert np.array_equal(z['cover'].cpu().numpy(), R.cover(from_lens(z['lens']), SRC, SIZE, PAD, 4)) and 0.2 < float(z['cover'].mean()) < 0.9
    g = torch.Generator().manual_seed(91)
    z['pw'] = 0.25 + 1.5 * torch.rand(4, *z['cover'].shape, generator=g)
    z['depth'] = np.random.default_rng(92).integers(300, 4000, (4,) + SRC).astype(np.uint16)
    z['depth'][:, ::5, ::3] = 0
    return z


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16) if t.dtype in (torch.bfloat16, torch.float16) else t


def _same_scene(a, b):
    va, vb = a.volume(), b.volume()
    assert torch.equal(_bits(va[0]), _bits(vb[0])) and torch.equal(va[1], vb[1]) and 0 < int(va[1].sum()) < va[1].numel()
    for k in ('_sum', '_wsum', '_count'):
        ta, tb = getattr(a, k), getattr(b, k)
        assert (ta is None) == (tb is None) and (ta is None or torch.equal(_bits(ta), _bits(tb))), k
    assert a.n_views == b.n_views and a.view_ids == b.view_ids


@pytest.mark.parametrize('kw', [dict(decay=0.75, forget_below=0.3), dict(window=2)], ids=['fading', 'windowed'])
def test_scene_with_a_lens_holds_the_bits_of_a_scene_given_the_images_and_the_cover(z, kw):
    model, E, f, lens, cover = z['model'], z['E'], list(z['frames']), z['lens'], z['cover']
    a, b = model.open_scene(z['user'], **kw), model.open_scene(dict(z['user'], **z['shapes']), **kw)
    pw = z['pw'][1:3]
    a.add_views_u8(f[:1], E[:1], SCALE, lens=lens)
    a.add_views_u8(f[1:3], E[1:3], SCALE, lens=lens, pixel_weights=pw, weights=[0.5, 2.0])
    a.add_views_u8(f[3:], E[3:4], SCALE, lens=lens)
    b.add_views(z['imgs'][:1], E[:1], pixel_weights=cover[None])
    b.add_views(z['imgs'][1:3].contiguous(), E[1:3], pixel_weights=pw.cuda() * cover, weights=[0.5, 2.0])
    b.add_views(z['imgs'][3:], E[3:4], pixel_weights=cover[None])
    _same_scene(a, b)
    assert len(a._covers) == 1 and {k: a.meta[k] for k in z['shapes']} == z['shapes']
    # and the cover matters: without it the border's mean colour is fused too
    c = model.open_scene(dict(z['user'], **z['shapes']), **kw)
    for lo, hi in ((0, 1), (1, 3), (3, 4)):
        c.add_views(z['imgs'][lo:hi].contiguous(), E[lo:hi], **(dict(pixel_weights=pw.cuda(), weights=[0.5, 2.0]) if lo == 1 else {}))
    assert int(c.volume()[1].sum()) > int(a.volume()[1].sum())
    for s in (a, b, c):
        s.close()


@pytest.mark.parametrize('with_lens', [True, False])
def test_depth_frames_equal_depths_built_by_map_prep_lens(z, ops, with_lens):
    model, E, f, cover = z['model'], z['E'], list(z['frames']), z['cover']
    lens = z['lens'] if with_lens else None
    kw = dict(decay=1.0, depth_gate=(0.5, 0.75))
    depth = z['depth'] if with_lens else (z['depth'].astype(np.float32) * np.float32(0.001))
    scale = 0.001 if with_lens else 1.0
    dp = ops.map_prep_lens(SIZE, PAD, SRC, lens, src=torch.from_numpy(depth).cuda(), scale=scale)
    assert np.array_equal(dp[2].cpu().numpy(), R.picked(depth[2], None if lens is None else from_lens(lens), SIZE, PAD, scale, 4))
    a, b = model.open_scene(z['user'], **kw), model.open_scene(dict(z['user'], **z['shapes']), **kw)
    if with_lens:
        a.add_views_u8(f[:2], E[:2], SCALE, lens=lens, depth_frames=depth[:2])
        a.add_views_u8(f[2:], E[2:4], SCALE, lens=lens, depth_frames=torch.from_numpy(depth[2:]).cuda())
        imgs, maps = z['imgs'], [dict(pixel_weights=cover[None].repeat(2, 1, 1), depths=dp[:2]), dict(pixel_weights=cover[None].repeat(2, 1, 1), depths=dp[2:])]
    else:
        from imvoxelnet_amd import data
        a.add_views_u8(f[:2], E[:2], SCALE, depth_frames=depth[:2], depth_scale=1.0)
        a.add_views_u8(f[2:], E[2:4], SCALE, depth_frames=depth[2:], depth_scale=1.0)
        imgs, maps = data.prepare_images_device(f, SCALE)[0], [dict(depths=dp[:2]), dict(depths=dp[2:])]
    b.add_views(imgs[:2].contiguous(), E[:2], **maps[0])
    b.add_views(imgs[2:].contiguous(), E[2:4], **maps[1])
    _same_scene(a, b)
    ungated = model.open_scene(dict(z['user'], **z['shapes']), decay=1.0)
    ungated.add_views(imgs[:2].contiguous(), E[:2], **{k: v for k, v in maps[0].items() if k != 'depths'})
    ungated.add_views(imgs[2:].contiguous(), E[2:4], **{k: v for k, v in maps[1].items() if k != 'depths'})
    assert int(ungated.volume()[1].sum()) > int(a.volume()[1].sum()), 'the depth gate carved something'
    for s in (a, b, ungated):
        s.close()


def test_coverage_with_the_cover_equals_the_lifts_mask_and_the_gate_sees_it(z):
    model, E, f, lens, cover = z['model'], z['E'], list(z['frames']), z['lens'], z['cover']
    a = model.open_scene(z['user'], decay=1.0)
    a.add_views_u8(f[:1], E[:1], SCALE, lens=lens)
    lifted = int(a.volume()[1].sum())
    fresh = model.open_scene(dict(z['user'], **z['shapes']), decay=1.0)
    with_cover, without = fresh.coverage(E[:1], pixel_weights=cover[None]), fresh.coverage(E[:1])
    assert with_cover[0, 0] == lifted == with_cover[0, 1] and without[0, 0] > lifted
    # the same frame again is redundant UNDER the cover: the gate, before the pipeline, counts nothing fresh
    a.add_views_u8(f[:1], E[:1], SCALE, lens=lens, min_novelty=0.01)
    assert a.last_admitted == [False] and a.n_views == 1
    assert a.coverage(E[:1], pixel_weights=cover[None])[0].tolist() == [lifted, 0]
    # a batch of two takes the same keywords and holds the session's bits in its rows
    b = model.open_scenes([z['user'], z['user']], decay=1.0)
    b.add_views_u8(f[:2], E[:2], [1, 0], SCALE, lens=lens)
    s1 = model.open_scene(z['user'], decay=1.0)
    s1.add_views_u8(f[1:2], E[1:2], SCALE, lens=lens)
    assert torch.equal(b.volume(1)[1][0], a.volume()[1][0]) and torch.equal(b.volume(0)[1][0], s1.volume()[1][0])
    for s in (a, fresh, b, s1):
        s.close()


def test_plain_session_takes_the_lens_for_its_image_only(z):
    model, E, f, lens = z['model'], z['E'], list(z['frames']), z['lens']
    a, b = model.open_scene(z['user']), model.open_scene(dict(z['user'], **z['shapes']))
    a.add_views_u8(f[:2], E[:2], SCALE, lens=lens)
    b.add_views(z['imgs'][:2].contiguous(), E[:2])
    _same_scene(a, b)
    with pytest.raises(ValueError, match='opened plain'):
        a.add_views_u8(f[:1], E[:1], SCALE, lens=lens, depth_frames=z['depth'][:1])
    a.close()
    b.close()
