"""-m gpu: the small HIP kernels around the convolutions (csrc/dcn.hip, csrc/pool_layout.hip, ivx_amax_f32 of csrc/stem.hip), each against
the plain fp64 reference of the same operation in tests/ref_ops.py -- not against another kernel of the project -- at the shapes, storage
types, windows and launch forms where such kernels go wrong.  The error bounds are derived from the kernels' rounding counts
(ref_ops.dcn_bound: K = 17, ref_ops.trilinear_bound: K = 7, ref_ops.avgpool_bound); every test prints the worst measured ratio.
tests/test_host_ops_fp64.py proves the same references and bounds on the CPU restatement."""
import ctypes as C

import numpy as np
import pytest
import torch

import ref_ops as R

pytestmark = pytest.mark.gpu

SLOTS = 64


@pytest.fixture(scope='module')
def L():
    from imvoxelnet_amd import _lib
    lib = _lib.lib()
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    return lib


def _p(t):
    return C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(rc, what):
    from imvoxelnet_amd import _lib
    _lib.check(rc, what)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _slots_max(slots):
    return float(slots[:SLOTS].view(torch.float32).max())


def _map(seed, B, H, W, Cn):
    return (np.random.RandomState(seed).randn(B, H, W, Cn) * 1.7).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- DCNv2 columns
def _make_pair_map(x):
    """fp32 numpy map -> (device float16 pair data, device slots with the scale, scale, the exact decode of what the device holds)"""
    from imvoxelnet_amd import ops
    p = ops.pair_from_float(_dev(x))
    return p.data, p.slots, p.scale(), R.pair_decode(p.data.cpu().numpy(), p.scale())


def _run_dcn(L, kind, x, om, k, s, p, d, nan_map=None):
    """One launch of the column kernel of a storage type on a NaN-filled output tensor of the test's own.
    Returns (columns as fp32 device tensor [B*Ho*Wo, k*k, C], the exact fp32 decode of the map the kernel was given, scale, slots)."""
    B, H, W, Cn = x.shape
    _, Ho, Wo, omc = om.shape
    omd = _dev(om)
    scale = slots = None
    if kind == 'f32':
        xd, decoded = _dev(x), x
        col = torch.full((B, Ho, Wo, k * k * Cn), float('nan'), device='cuda', dtype=torch.float32)
        _ok(L.ivx_dcn_im2col_fwd(_p(xd), _p(omd), B, H, W, Cn, k, k, s, p, d, omc, _p(col), _st()), 'ivx_dcn_im2col_fwd')
        got = col
    elif kind == 'bf16':
        xd = _dev(x).to(torch.bfloat16)
        decoded = xd.float().cpu().numpy()
        col = torch.full((B, Ho, Wo, k * k * Cn), float('nan'), device='cuda', dtype=torch.bfloat16)
        _ok(L.ivx_dcn_im2col_fwd_bf16(_p(xd), _p(omd), B, H, W, Cn, k, k, s, p, d, omc, _p(col), _st()), 'ivx_dcn_im2col_fwd_bf16')
        got = col.float()
    else:
        from imvoxelnet_amd import ops
        data, in_slots, scale, decoded = _make_pair_map(np.nan_to_num(x, nan=0.0).reshape(B, 1, H, W, Cn))
        if nan_map is not None:             # the split clamps, so a NaN goes into the stored hi half directly
            for (b, h, w, c) in nan_map:
                data[b, 0, h, w, (c // 16) * 32 + c % 16] = float('nan')
                decoded[b, 0, h, w, c] = np.nan
        decoded = decoded.reshape(B, H, W, Cn)
        col = torch.full((B, Ho, Wo, 2 * k * k * Cn), float('nan'), device='cuda', dtype=torch.float16)
        slots = ops.new_slots('cuda')
        sc_in = C.c_void_p(in_slots.data_ptr() + 4 * SLOTS)
        sc_out = C.c_void_p(slots.data_ptr() + 4 * SLOTS)
        _ok(L.ivx_dcn_im2col_fwd_pair(_p(data), sc_in, _p(omd), B, H, W, Cn, k, k, s, p, d, omc, _p(col), sc_out, _p(slots), _st()),
            'ivx_dcn_im2col_fwd_pair')
        assert float(slots[SLOTS:SLOTS + 1].view(torch.float32)[0]) == scale, 'the columns keep the scale of the map'
        g = col.view(B * Ho * Wo, k * k * Cn // 16, 2, 16).float()
        got = (g[:, :, 0] + g[:, :, 1]) / scale                       # exact: hi + lo has 22 bits, the scale is a power of two
    torch.cuda.synchronize()
    return got.reshape(B * Ho * Wo, k * k, Cn), decoded, scale, slots


def _storage_term(kind, ref, scale):
    if kind == 'bf16':
        return 2.0 ** -8 * np.abs(ref) + R.BF16_TINY                 # one rounding to bf16
    if kind == 'pair':
        return 2.0 ** -21 * np.abs(ref) + 2.0 ** -24 / scale         # the split to 22 bits
    return None


@pytest.mark.parametrize('kind', ['f32', 'bf16', 'pair'])
def test_dcn_columns_vs_fp64(L, kind):
    """ivx_dcn_im2col_fwd / _bf16 / _pair against ref_ops.dcn_columns of the exact decode of the map: every window (k, stride, pad, dil) of
    ref_ops.DCN_PARAMS with every channel count, both om_channels, B 1 .. 3, the degenerate maps; offsets and masks built to drive the
    border branches (ref_ops.dcn_offsets_masks; the shares are asserted).  Bound: |got - ref| <= 17 * 2^-24 * A + 2^-126 for fp32
    (ref_ops.dcn_bound counts the roundings), plus 2^-8 |ref| + 2^-133 on bf16 storage, plus 2^-21 |ref| + 2^-24 / scale for pairs; exactly
    0 where the point or all corners are outside; the pair kernel keeps the map's scale and its recorded maximum, rounded as the split
    rounds, is max |decoded columns|."""
    worst = 0.0
    for seed, B, H, W, Cn, k, s, p, d, omc in R.dcn_small_cases(kind):
        x = _map(seed, B, H, W, Cn)
        om = R.dcn_offsets_masks(seed + 1, B, H, W, k, s, p, d, omc)
        got, decoded, scale, slots = _run_dcn(L, kind, x, om, k, s, p, d)
        ref, A = R.dcn_columns(decoded, om, k, s, p, d)
        name = f'dcn {kind} B{B} {H}x{W} C{Cn} k{k} s{s} p{p} d{d} omc{omc}'
        R.check_shares(name, om, ref, H, W, k, s, p, d)
        gv = got.cpu().numpy()
        worst = max(worst, R.check_dcn(name, gv, ref, A, _storage_term(kind, ref, scale)))
        if kind == 'pair':
            assert R.pair_round(_slots_max(slots), scale) == float(np.abs(gv).max()), name
    print(f'dcn {kind}: worst |got - ref| / (2^-24 A) over the cases = {worst:.3f} (fp32 bound: K = {R.K_DCN})')


@pytest.mark.parametrize('kind', ['f32', 'bf16', 'pair'])
def test_dcn_columns_nan_in_the_map(L, kind):
    """A NaN of the map shows in exactly the columns that have it among their in-map corners, whatever the weight (0 * NaN is NaN: an
    integer offset gives the high corner the weight 0), and nowhere else: a corner outside the map is replaced by 0, not multiplied by 0."""
    B, H, W, Cn, k = 2, 13, 17, 32, 3
    where = [(0, 0, 0, 1), (0, 12, 16, 31), (1, 6, 8, 16), (1, 0, 16, 5), (1, 12, 0, 20)]
    for s, p, d in ((1, 1, 1), (2, 1, 1), (1, 2, 2)):
        x = _map(77 + s + d, B, H, W, Cn)
        for b, h, w, c in where:
            x[b, h, w, c] = np.nan
        om = R.dcn_offsets_masks(78 + s + d, B, H, W, k, s, p, d, 27)
        got, decoded, scale, _ = _run_dcn(L, kind, x, om, k, s, p, d, nan_map=where)
        assert int(np.isnan(decoded).sum()) == len(where)
        ref, A = R.dcn_columns(decoded, om, k, s, p, d)
        assert 0 < int(np.isnan(ref).sum()) < ref.size // 8
        R.check_dcn(f'dcn {kind}, NaN in the map, s{s} p{p} d{d}', got.cpu().numpy(), ref, A, _storage_term(kind, np.nan_to_num(ref), scale))


@pytest.mark.parametrize('kind', ['f32', 'bf16', 'pair'])
def test_dcn_columns_capped_grid(L, kind):
    """The capped grid-stride form of every column kernel (fp32: more than 256 * 256 - 8 workgroups of 256 (pixel, tap, 4 channel) threads;
    bf16 / pair: more than 256 * 64 - 8 of 256 (pixel, 8 channel) threads): B 6, 116 x 200, C 256, stride 2 for fp32 (the nuScenes stage-3
    size) and 1 for bf16 / pair.  The output tensor is NaN before the launch and holds no NaN after it, anywhere; values are compared on a
    seeded sample of 4096 output pixels that holds the corners of the first image and the last pixel of the last, all taps, all channels."""
    B, H, W, Cn, k, p, d = 6, 116, 200, 256, 3, 1, 1
    s = 2 if kind == 'f32' else 1
    Ho, Wo = R.dcn_out_hw(H, W, k, s, p, d)
    threads = B * Ho * Wo * (k * k * Cn // 4 if kind == 'f32' else Cn // 8)
    assert (threads + 255) // 256 > (256 * 256 - 8 if kind == 'f32' else 256 * 64 - 8)
    x = torch.randn(B, H, W, Cn, generator=torch.Generator().manual_seed(41)).mul_(1.7).numpy()
    om = R.dcn_offsets_masks(42, B, H, W, k, s, p, d, 28)
    got, decoded, scale, slots = _run_dcn(L, kind, x, om, k, s, p, d)
    assert int(torch.isnan(got).sum()) == 0, 'an element of the output was not written'
    pix = R.sample_pixels(43, B, Ho, Wo, 4096)
    assert len(pix) >= 4096 and {0, Wo - 1, (Ho - 1) * Wo, Ho * Wo - 1, B * Ho * Wo - 1} <= set(pix.tolist())
    ref, A = R.dcn_columns(decoded, om, k, s, p, d, pixels=pix)
    R.check_shares(f'dcn {kind} capped grid', om, ref, H, W, k, s, p, d)
    gv = got[torch.from_numpy(pix).cuda()].cpu().numpy()
    R.check_dcn(f'dcn {kind} capped grid, B{B} {H}x{W} C{Cn} s{s}', gv, ref, A, _storage_term(kind, ref, scale))
    if kind == 'pair':
        assert R.pair_round(_slots_max(slots), scale) == float(got.abs().max())


# ---------------------------------------------------------------------------------------------------------------- max-pool
def _assert_same_bits(name, got, ref):
    """fp32 arrays: NaN in the same places, every other element the same bits"""
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), f'{name}: NaN in {int(np.isnan(got).sum())} elements, reference {int(nan.sum())}'
    assert np.array_equal(got.view(np.uint32)[~nan], ref.view(np.uint32)[~nan]), f'{name}: {int((got != ref)[~nan].sum())} elements differ'


def _pool_input(kind, seed, shape):
    """-> (device tensor in the storage type, its exact fp32 decode)"""
    if kind == 'fp8':            # random e4m3 bytes of both signs without the zeros; both NaN bytes, 0x7f and 0xff, at 1 % each
        rng = np.random.RandomState(seed)
        b = rng.randint(0, 256, size=shape).astype(np.uint8)
        b[(b & 0x7f) == 0] = 0x38
        b[(b & 0x7f) == 0x7f] ^= 0x01
        r = rng.rand(*shape)
        b[r < 0.01] = 0x7f
        b[(r >= 0.01) & (r < 0.02)] = 0xff
        t = torch.from_numpy(b).view(torch.float8_e4m3fn)
        return t.cuda(), t.float().numpy()
    x = R.pool_input(seed, shape)
    if kind == 'bf16':
        t = torch.from_numpy(x).to(torch.bfloat16)
        return t.cuda(), t.float().numpy()
    return _dev(x), x


POOL_CHANNELS = {'f32': (4, 16, 64, 100), 'bf16': (4, 16, 64, 100), 'fp8': (16, 64)}
# above the cap of 8192 workgroups (256 threads of 4 channels, e4m3: 16 channels): window (3, 1, 1) on 192 x 640 x 64, B 4 (e4m3: B 5)
POOL_LARGE = {'f32': (4, 192, 640, 64, 3, 1, 1), 'bf16': (4, 192, 640, 64, 3, 1, 1), 'fp8': (5, 192, 640, 64, 3, 1, 1)}


@pytest.mark.parametrize('kind', ['f32', 'bf16', 'fp8'])
def test_maxpool_exact(L, kind):
    """ivx_maxpool2d_fwd / _bf16 / _fp8 == F.max_pool2d of the decoded map, bit for bit: five windows, sizes with a partial last window,
    both signs, -inf / +inf / NaN in the input (e4m3: both NaN bytes; any NaN byte in the output), and one case above the block cap."""
    from imvoxelnet_amd import ops
    cases = R.pool_small_cases(POOL_CHANNELS[kind]) + [(3999,) + POOL_LARGE[kind]]
    for seed, B, H, W, Cn, k, s, p in cases:
        xd, decoded = _pool_input(kind, seed, (B, H, W, Cn))
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        if B * Ho * Wo * Cn > 10 ** 6:
            assert (B * Ho * Wo * (Cn // (16 if kind == 'fp8' else 4)) + 255) // 256 > 8192
        got = ops.maxpool2d(xd.view(B, 1, H, W, Cn), k, s, p)
        assert got.dtype == xd.dtype and tuple(got.shape) == (B, 1, Ho, Wo, Cn)
        ref = R.maxpool2d(decoded, k, s, p)
        assert np.isnan(ref).any() or H * W * Cn < 5000
        _assert_same_bits(f'maxpool {kind} B{B} {H}x{W} C{Cn} ({k},{s},{p})', got.cpu().float().numpy().reshape(ref.shape), ref)


def test_maxpool_pair_vs_reference(L):
    """ivx_maxpool2d_fwd_pair on inputs of both signs: the pool is exact and the split rounds to 22 bits; the scale is the one of the bound
    amax_in * wbound + sbound; the recorded maximum is max |pool| exactly.  One case above the block cap."""
    from imvoxelnet_amd import ops
    wb, sb, a_in = 7.5, 0.25, 2.0
    for seed, B, H, W, Cn, k, s, p in R.pool_small_cases((16, 64)) + [(3998, 4, 192, 640, 64, 3, 1, 1)]:
        x = R.pool_input(seed, (B, H, W, Cn), special=0.0)
        ref = R.maxpool2d(x, k, s, p)
        amax_in = ops.new_slots('cuda')
        amax_in[:SLOTS].view(torch.float32)[11] = a_in
        got = ops.maxpool2d_pair(_dev(x).view(B, 1, H, W, Cn), amax_in, wb, sb, k, s, p)
        scale = got.scale()
        assert scale == R.pow2_scale(np.float32(np.float32(a_in) * np.float32(wb) + np.float32(sb)) * np.float32(1.001))
        gv = R.pair_decode(got.data.cpu().numpy(), scale).reshape(ref.shape)
        assert float(np.abs(gv.astype(np.float64) - ref).max()) <= float(np.abs(ref).max()) * 2.0 ** -21 + 2.0 ** -24 / scale
        assert got.amax() == float(np.abs(ref).max())


# ---------------------------------------------------------------------------------------------------------------- trilinear x2
@pytest.mark.parametrize('kind', ['f32', 'bf16'])
def test_trilinear2x_vs_fp64(L, kind):
    """ivx_upsample_trilinear2x_fwd against the fp64 8-corner blend within 7 * 2^-24 * max |corner| (ref_ops.trilinear_bound); _bf16 against
    the fp64 blend of the decoded map within one rounding (2^-8 |ref| + 2^-133) plus that bound.  D, H, W equal to 1 in turn, odd sizes,
    C in {4, 12, 64}, one volume above the cap of 8192 workgroups."""
    from imvoxelnet_amd import ops
    worst = 0.0
    B, D, H, W, Cn = R.TRI_LARGE
    assert (B * 8 * D * H * W * (Cn // 4) + 255) // 256 > 8192
    for B, D, H, W, Cn in R.TRI_CASES + [R.TRI_LARGE]:
        x = (np.random.RandomState(D * 100 + H * 10 + W).randn(B, D, H, W, Cn) * 2).astype(np.float32)
        xd = _dev(x) if kind == 'f32' else _dev(x).to(torch.bfloat16)
        decoded = xd.float().cpu().numpy()
        got = ops.upsample_trilinear2x(xd)
        assert got.dtype == xd.dtype
        ref, M = R.trilinear2x(decoded)
        diff = np.abs(got.float().cpu().numpy() - ref)
        bound = R.trilinear_bound(M) + (2.0 ** -8 * np.abs(ref) + R.BF16_TINY if kind == 'bf16' else 0)
        worst = max(worst, float((diff / (R.U * M)).max()) if kind == 'f32' else float((diff / bound).max()))
        assert np.all(diff <= bound), (kind, B, D, H, W, Cn, float((diff / bound).max()))
    print(f'trilinear x2 {kind}: worst ' + (f'|got - ref| / (2^-24 max|corner|) = {worst:.3f} of K = {R.K_TRI}' if kind == 'f32' else f'|got - ref| / bound = {worst:.3f}'))


# ---------------------------------------------------------------------------------------------------------------- layout
def _layout_case(L, B, Cn, S, pad, misalign):
    from imvoxelnet_amd import ops
    cp = Cn if pad is None else (Cn + pad - 1) // pad * pad
    x = np.random.RandomState(Cn * 1000 + S).randn(B, Cn, S).astype(np.float32)
    x[B - 1, Cn - 1, S - 1] = -9.25
    ref = R.nchw_to_nhwc(x, cp)
    if misalign:                                    # a view that starts 4 bytes past a 16-byte boundary
        buf = torch.zeros(B * Cn * S + 1, device='cuda')
        buf[1:] = _dev(x).reshape(-1)
        xd = buf[1:].view(B, Cn, 1, S)
        assert xd.data_ptr() % 16 == 4 and xd.is_contiguous()
    else:
        xd = _dev(x).view(B, Cn, 1, S)
        assert xd.data_ptr() % 16 == 0
    name = f'layout B{B} C{Cn} S{S} pad{pad} misaligned {misalign}'
    out = ops.to_channels_last(xd, pad_to=pad)
    assert np.array_equal(out.cpu().numpy().reshape(ref.shape).view(np.uint32), ref.view(np.uint32)), name
    out2 = ops.to_channels_last_amax(xd, pad_to=pad)
    assert np.array_equal(out2.cpu().numpy().reshape(ref.shape).view(np.uint32), ref.view(np.uint32)), name + ' (amax form)'
    assert _slots_max(out2.ivx_slots) == R.amax(x) == 9.25, name
    back = ops.from_channels_last(out, ndim_spatial=2)
    bv = back.cpu().numpy().reshape(B, cp, S)
    assert np.array_equal(bv, R.nhwc_to_nchw(ref)) and np.array_equal(bv[:, :Cn], x) and not bv[:, Cn:].any(), name


def test_layout_exact(L):
    """ivx_nchw_to_nhwc, ivx_nchw_to_nhwc_amax and ivx_nhwc_to_nchw, exact: the 4-channel streaming kernel (C <= 4, pad_to 4, S % 4 == 0,
    aligned) and the 32 x 32 tile kernel everywhere else -- S % 4 in {1, 2, 3}, an input 4 bytes past a 16-byte boundary, C in
    {5, 31, 32, 33, 100} with and without padding to 8, S in {1, 31, 32, 33, 1000}; padded channels 0; the recorded maximum == max |in|."""
    for B, Cn, S in R.LAYOUT_IMAGE_CASES:
        for misalign in (False, True):
            _layout_case(L, B, Cn, S, 4, misalign)
    for B, Cn, S, pad in R.LAYOUT_TILE_CASES:
        _layout_case(L, B, Cn, S, pad, False)


def test_layout_amax_ignores_nan(L):
    """include/imvoxel.h: ivx_nchw_to_nhwc_amax takes the maximum over the non-NaN elements and an Inf counts (the bound built from it has
    to hold every finite value; a NaN stays a NaN under any scale) -- on both kernels."""
    from imvoxelnet_amd import ops
    for Cn, S, pad in ((3, 64, 4), (3, 66, 4), (33, 100, None)):
        x = np.random.RandomState(S).randn(2, Cn, S).astype(np.float32)
        x[1, 2, 5] = np.nan
        out = ops.to_channels_last_amax(_dev(x).view(2, Cn, 1, S), pad_to=pad)
        assert _slots_max(out.ivx_slots) == R.amax(x) and bool(torch.isnan(out[1, 0, 0, 5, 2]))
        x[0, 1, 7] = -np.inf
        out = ops.to_channels_last_amax(_dev(x).view(2, Cn, 1, S), pad_to=pad)
        assert _slots_max(out.ivx_slots) == float('inf')


# ---------------------------------------------------------------------------------------------------------------- maxima
def test_amax_f32(L):
    """ivx_amax_f32 == max |x| exactly for n in {0, 1, 2, 3, 5, 4096, 1027, 3 * 2^20 + 3} with the maximum in the first element, the last
    element and the n % 4 tail; a NaN anywhere gives +Inf (include/imvoxel.h); n = 0 leaves the slots untouched."""
    for n in R.AMAX_SIZES:
        for name, a in R.amax_inputs(n, n + 1).items():
            buf = torch.zeros(max(n, 4), device='cuda')
            buf[:n] = _dev(a)
            slots = torch.zeros(SLOTS, device='cuda', dtype=torch.int32)
            _ok(L.ivx_amax_f32(_p(buf), n, _p(slots), _st()), 'ivx_amax_f32')
            assert _slots_max(slots) == R.amax(a), (n, name)
            for pos in sorted({0, n - 1, n - (n % 4), n // 2}):
                if 0 <= pos < n:
                    b = buf.clone()
                    b[pos] = float('nan')
                    slots.zero_()
                    _ok(L.ivx_amax_f32(_p(b), n, _p(slots), _st()), 'ivx_amax_f32')
                    assert _slots_max(slots) == float('inf'), (n, name, pos)
    slots = torch.full((SLOTS,), 0x3f800000, device='cuda', dtype=torch.int32)
    _ok(L.ivx_amax_f32(_p(torch.ones(4, device='cuda')), 0, _p(slots), _st()), 'ivx_amax_f32')
    assert bool((slots == 0x3f800000).all())


def test_amax_bf16(L):
    """ivx_amax_bf16 == max |x| exactly for the same sizes and positions; the maximum is over the non-NaN elements and an Inf counts
    (include/imvoxel.h: the calibration needs a finite scale for the finite values); an all-NaN tensor and n = 0 leave *out untouched."""
    for n in R.AMAX_SIZES:
        for name, a in R.amax_inputs(n, n + 1).items():
            xb = torch.zeros(max(n, 4), device='cuda', dtype=torch.bfloat16)
            xb[:n] = _dev(a).to(torch.bfloat16)
            out = torch.zeros(1, device='cuda')
            _ok(L.ivx_amax_bf16(_p(xb), n, _p(out), _st()), 'ivx_amax_bf16')
            assert float(out[0]) == R.amax(xb[:n].float().cpu().numpy()), (n, name)
            if n >= 2:
                for pos in sorted({0, n - 1, n // 2}):
                    b = xb.clone()
                    b[pos] = float('nan')
                    out.zero_()
                    _ok(L.ivx_amax_bf16(_p(b), n, _p(out), _st()), 'ivx_amax_bf16')
                    assert float(out[0]) == R.amax(b[:n].float().cpu().numpy()), (n, name, pos)
                b[(pos + 1) % n] = float('-inf')
                out.zero_()
                _ok(L.ivx_amax_bf16(_p(b), n, _p(out), _st()), 'ivx_amax_bf16')
                assert float(out[0]) == float('inf'), (n, name)
    out = torch.full((1,), 1.5, device='cuda')
    _ok(L.ivx_amax_bf16(_p(torch.ones(4, device='cuda', dtype=torch.bfloat16)), 0, _p(out), _st()), 'ivx_amax_bf16')
    _ok(L.ivx_amax_bf16(_p(torch.full((8,), float('nan'), device='cuda', dtype=torch.bfloat16)), 8, _p(out), _st()), 'ivx_amax_bf16')
    assert float(out[0]) == 1.5


# ---------------------------------------------------------------------------------------------------------------- global mean
@pytest.mark.parametrize('kind', ['f32', 'bf16'])
def test_global_avgpool_vs_fp64(L, kind):
    """ivx_global_avgpool_fwd / _bf16 against the fp64 mean of the decoded map within (S/4 + 4) * 2^-24 * mean |x| (four sequential partial
    sums: ref_ops.avgpool_bound); S in {1, 3, 4, 35, 300}, C in {1, 63, 64, 65, 100, 2048}."""
    from imvoxelnet_amd import ops
    worst = 0.0
    for S in R.AVGPOOL_S:
        for Cn in R.AVGPOOL_C:
            B = 1 + (S + Cn) % 3
            x = (np.random.RandomState(S * 7 + Cn).randn(B, S, Cn) * 2 + 0.5).astype(np.float32)
            xd = _dev(x) if kind == 'f32' else _dev(x).to(torch.bfloat16)
            got = ops.global_avgpool(xd.view(B, 1, 1, S, Cn)).cpu().numpy().reshape(B, Cn)
            ref, mabs = R.global_mean(xd.float().cpu().numpy())
            ratio = float((np.abs(got - ref) / R.avgpool_bound(S, mabs)).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (kind, S, Cn, ratio)
    print(f'global mean {kind}: worst |got - ref| / ((S/4 + 4) 2^-24 mean|x|) = {worst:.3f}')
