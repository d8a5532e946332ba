"""-m gpu: the scale rule of the fp16-pair tensors at both ends of its contract (include/imvoxel.h "Chained fp16-pair activations"), the HIP
kernels against the fp64 references of tests/ref_pair.py -- the cases, drivers, conditions and derived bounds that
tests/test_host_pair_range.py proves on the CPU restatement.

Tight side: inputs that reach the bound max|in| * wbound + sbound + max|res| (L = bound / max|ref| <= 1.01, by the reference), with the
maximum solved so that the bound times 1.001 lies within 2^-12 below and, in a second run, above a power of two: every stored half finite,
s_out * max|ref| < 2^15, the stated scale, the recorded maximum, values within 2e-5 of the range.  Loose side: dead channels make the bound
loose by chosen factors L, and |out - ref| <= 2e-5 range + delta, delta(T) = max(2^-22, 2^-39 L) max|T| derived in ref_pair; pair inputs
written 2^20 and 2^26 below their ideal scale (subnormal halves) go through every consumer.  The Winograd forms on pair operands, which the
CPU restatement does not have, get the input that drives B^T d B to its largest gain.  Every test prints its worst error / bound."""
import ctypes as C

import numpy as np
import pytest
import torch

import ref_pair as P

pytestmark = pytest.mark.gpu
SIDES = ['below', 'above']


class GpuBackend:
    """ref_pair.HostBackend's twin on device memory; the structures are the library binding's own"""
    name = 'gpu'

    def __init__(self, L):
        from imvoxelnet_amd import _lib
        self.L = L
        self.ConvDesc, self.PairIO, self.BottleneckDesc, self.BottleneckIO = _lib.ConvDesc, _lib.PairIO, _lib.BottleneckDesc, _lib.BottleneckIO

    @property
    def stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def up(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def full(self, shape, dtype, fill):
        return torch.full(tuple(shape), fill, device='cuda', dtype=getattr(torch, np.dtype(dtype).name))

    def addr(self, h, byte_offset=0):
        return h.data_ptr() + byte_offset

    def get(self, h):
        torch.cuda.synchronize()
        return h.cpu().numpy()

    def ok(self, rc, what):
        from imvoxelnet_amd import _lib
        _lib.check(rc, what)


@pytest.fixture(scope='module')
def be():
    from imvoxelnet_amd import _lib
    lib = _lib.lib()
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    return GpuBackend(lib)


# ---------------------------------------------------------------------------------------------------------------- host-only packers
def test_pack_bounds_hip_library(be):
    """ivx_pair_pack_filters, ivx_bottleneck_proj_pack and the stem's bound terms as the HIP library computes them (host code): at least the
    exact fp64 value of their definition over the decoded packed filters, at most that times 1 + 2^-20; s_w puts max|w| into [2^14, 2^15);
    the decoded filters are within 2^-21 max|w| of the input.  Cin 32 .. 2048, taps 1 and 9, random and adversarial filters."""
    worst = 0.0
    for name, w, sc, sh in P.pack_cases():
        worst = max(worst, *P.check_pack(be, name, w, sc, sh))
    r = np.random.RandomState(3)
    (w3, s3, t3), (wd, sd, td) = P.tight_filters(r, 256, 1, 64, 0.75, 0.125), P.random_filters(r, 256, 1, 64)
    worst = max(worst, *P.check_pack_proj(be, 'proj', w3[:, 0], s3, t3, wd[:, 0], sd, td))
    w = (r.randn(64, 3, 7, 7) * (2.0 / 147) ** 0.5).astype(np.float32)
    worst = max(worst, *P.check_pack_stem(be, 'stem', w, (r.rand(64) + 0.5).astype(np.float32), (r.randn(64) * 0.1).astype(np.float32)))
    print(f'gpu library packers: bound term / exact - 1 <= {worst:.3e} (allowed 2^-20 = {2.0 ** -20:.3e})')


# ---------------------------------------------------------------------------------------------------------------- tight side
@pytest.mark.parametrize('side', SIDES)
@pytest.mark.parametrize('case', P.TIGHT_CONV, ids=lambda c: f'{c[0]}x{c[1][0]}x{c[1][1]}-{c[2]}-{c[3]}-k{c[4]}s{c[5]}{c[6]}')
def test_tight_conv_vs_fp64(be, case, side):
    """ivx_conv_fwd_pio on an input that reaches its bound: 1x1, 3x3, stride 2 with post_scale 0.5, split-K, pair / upsampled fp32 / upsampled
    pair residuals, fp32 and pair outputs, and filters, scales, shifts and inputs of both signs."""
    worst, L = P.run_tight_conv(be, case, side)
    print(f'gpu tight conv {case} {side}: worst error / bound = {worst:.3f}, L = {L:.5f}')


@pytest.mark.parametrize('side', SIDES)
@pytest.mark.parametrize('case', P.TIGHT_BOTTLENECK, ids=lambda c: f'{"proj" if c[0] else "identity"}-P{c[1]}-{c[2]}x{c[3]}x{c[4]}')
def test_tight_bottleneck_vs_fp64(be, case, side):
    """ivx_bottleneck_fwd_pio / ivx_bottleneck_proj_fwd_pio with b1, b2 and b3 (shortcut term included) attained at once"""
    worst, Ls = P.run_tight_bottleneck(be, case, side)
    print(f'gpu tight bottleneck {case} {side}: worst error / bound = {worst:.3f}, L1 L2 L3 = {Ls[0]:.5f} {Ls[1]:.5f} {Ls[2]:.5f}')


@pytest.mark.parametrize('side', SIDES)
@pytest.mark.parametrize('case', P.TIGHT_STEM, ids=lambda c: f'{c[0]}x{c[1]}x{c[2]}')
def test_tight_stem_vs_fp64(be, case, side):
    """ivx_stem_pool_fwd_pair and the three-launch head on an image that is +-a, sign-aligned with the filter of largest scale * L1 over one
    interior 7 x 7 window: the same, stated scale from both"""
    worst, L = P.run_tight_stem(be, case, side)
    print(f'gpu tight stem {case} {side}: worst error / bound = {worst:.3f}, L = {L:.5f}')


# ---------------------------------------------------------------------------------------------------------------- loose side
@pytest.mark.parametrize('how,target', P.LOOSE_TARGETS, ids=lambda v: v if isinstance(v, str) else f'L2^{int(np.log2(v))}')
@pytest.mark.parametrize('case', P.LOOSE_CONV, ids=lambda c: f'{c[0]}x{c[1][0]}x{c[1][1]}-k{c[4]}')
def test_loose_conv_vs_fp64(be, case, how, target):
    """a dead channel drives sbound (or wbound): |out - ref| <= 2e-5 range + max(2^-22, 2^-39 L) max|out|"""
    worst, L = P.run_loose_conv(be, case, how, target)
    print(f'gpu loose conv {case} {how}: worst error / bound = {worst:.3f}, L = 2^{np.log2(L):.2f}')


@pytest.mark.parametrize('target', [2.0 ** 10, 2.0 ** 18, 2.0 ** 24], ids=lambda v: f'L2^{int(np.log2(v))}')
def test_loose_stem_vs_fp64(be, target):
    worst, L = P.run_loose_stem(be, target)
    print(f'gpu loose stem: worst error / bound = {worst:.3f}, L = 2^{np.log2(L):.2f}')


@pytest.mark.parametrize('target', [2.0 ** 10, 2.0 ** 20], ids=lambda v: f'L2^{int(np.log2(v))}')
@pytest.mark.parametrize('case', P.LOOSE_BOTTLENECK, ids=lambda c: 'proj' if c[0] else 'identity')
def test_loose_bottleneck_vs_fp64(be, case, target):
    """the dead channel sits in conv1; bound 2e-5 range + wbound3 (wbound2 delta(mid1) + delta(mid2)) + delta(out); the layer-wise chain
    (three / four ivx_conv_fwd_pio launches, measured maxima) on the same data meets the plain 2e-5"""
    worst, chain, Ls = P.run_loose_bottleneck(be, case, target)
    print(f'gpu loose bottleneck {case}: worst error / bound = {worst:.3f}, layer-wise chain error / (2e-5 range) = {chain:.3f}, '
          f'L1 L2 L3 = 2^{np.log2(Ls[0]):.2f} 2^{np.log2(Ls[1]):.2f} 2^{np.log2(Ls[2]):.2f}')


@pytest.mark.parametrize('below', [20, 26])
def test_loosely_scaled_input_vs_fp64(be, below):
    """A pair input written 2^below under its ideal scale -- subnormal lo halves everywhere, at 2^26 subnormal hi halves too -- through
    ivx_conv_fwd_pio (1x1, 3x3), both bottlenecks and ivx_dcn_im2col_fwd_pair: a staging path that flushes fp16 subnormals fails here."""
    out = [P.run_loose_input_conv(be, 1, below), P.run_loose_input_conv(be, 3, below), P.run_loose_input_bottleneck(be, False, below),
           P.run_loose_input_bottleneck(be, True, below)]
    dcn = P.run_loose_input_dcn(be, below)
    print(f'gpu input scaled 2^{below} below: error / (2e-5 range) conv 1x1 {out[0]:.3f}, 3x3 {out[1]:.3f}, identity block {out[2]:.3f}, '
          f'projection block {out[3]:.3f}; dcn columns error / bound = {dcn:.3f}')


# ---------------------------------------------------------------------------------------------------------------- one model-level case
@pytest.mark.parametrize('name', P.MODEL_CASES)
def test_model_dead_channels_operand_modes(be, name):
    """The model handle on a trunk whose BatchNorms have 5 % dead channels (gamma = 0, beta = -50 max|beta|) and an image with a saturated
    16 x 16 block: default operand mode against trunk_operands = wino_operands = 0.  The second handle is the project's own code on other
    arithmetic (exact fp32 products), NOT an fp64 reference.  FPN level 0, the volume and the neck outputs are finite and within 2e-4 of the
    tensor's range, the valid mask is identical."""
    import plan_worker as W
    ratios = P.run_model_operand_modes(W.load_lib('hip'), 'cuda', name)
    print(f'gpu model {name}: error / (2e-4 range) ' + ', '.join(f'{k} {v:.3f}' for k, v in ratios.items()))


# ---------------------------------------------------------------------------------------------------------------- Winograd on pair operands
# B^T of F(4x4, 3x3) and F(6x6, 3x3) (Lavin & Gray, interpolation points 0, +-1, +-2 (, +-1/2), infinity): this test's own copy
BT = {4: np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], np.float64),
      6: np.array([[1, 0, -21 / 4, 0, 21 / 4, 0, -1, 0], [0, 1, 1, -17 / 4, -17 / 4, 1, 1, 0], [0, -1, 1, 17 / 4, -17 / 4, -1, 1, 0],
                   [0, 1 / 2, 1 / 4, -5 / 2, -5 / 4, 2, 1, 0], [0, -1 / 2, 1 / 4, 5 / 2, -5 / 4, -2, 1, 0], [0, 2, 4, -5 / 2, -5, 1 / 2, 1, 0],
                   [0, -2, 4, 5 / 2, -5, -1 / 2, 1, 0], [0, -1, 0, 21 / 4, 0, -21 / 4, 0, 1]], np.float64)}
GAIN = {4: (99.0, 100.0), 6: (222.0, 225.0)}                   # required, largest possible: (largest absolute row sum)^2
WINO_A = [float(np.nextafter(np.float32(2.0 ** e), np.float32(0))) for e in (-20, 0, 13)] + [2.0 ** e for e in (-20, 0, 13)]


def _wino_input(shape, tile, a, seed):
    """[B, X, Y, Z, C] fp32: uniform in [-a, a], and every channel and slice of the tile at tile index (1, 1) of sample 0 holds
    a * sigma_i * sigma_j, sigma the sign pattern (zeros count as +) of the row of B^T with the largest absolute row sum."""
    B, (X, Y, Z), ci = shape
    bt = BT[tile]
    sigma = np.where(bt[int(np.argmax(np.abs(bt).sum(1)))] < 0, -1.0, 1.0)
    x = np.random.RandomState(seed).uniform(-a, a, (B, X, Y, Z, ci)).astype(np.float32)
    x0 = tile - 1                                               # tile 1 reads positions tile - 1 .. 2 tile of the unpadded axis (padding 1)
    ix, iy = np.arange(x0, min(x0 + tile + 2, X)), np.arange(x0, min(x0 + tile + 2, Y))
    x[0, ix[:, None], iy[None, :]] = (a * sigma[ix - x0][:, None] * sigma[iy - x0][None, :]).astype(np.float32)[:, :, None, None]
    return x


def _wino_gain(x, tile):
    """max |B^T d B| / max|d| in fp64 over the tiles of sample 0, channel 0, slice 0 (padding 1)"""
    bt = BT[tile]
    d = np.pad(x[0, :, :, 0, 0].astype(np.float64), ((1, tile + 2), (1, tile + 2)))
    best = 0.0
    for tx in range((x.shape[1] + tile - 1) // tile):
        for ty in range((x.shape[2] + tile - 1) // tile):
            best = max(best, float(np.abs(bt @ d[tx * tile:tx * tile + tile + 2, ty * tile:ty * tile + tile + 2] @ bt.T).max()))
    return best / float(np.abs(x).max())


def _wino_check(name, x, w, scale, shift, tile, run_pair, run_f32):
    """finite, within 1e-4 of the fp64 range, rms error <= 1.5 x the fp32-operand form's + 2e-7 of the range: the bars of
    test_conv_winograd_f16_pair_operands.  The condition on the input: the test's own B^T d B reaches GAIN[tile][0]."""
    gain = _wino_gain(x.cpu().numpy(), tile)
    assert gain >= GAIN[tile][0], f'{name}: the input drives B^T d B only to {gain:.2f} of {GAIN[tile][1]}'
    ref = torch.nn.functional.conv3d(x.permute(0, 4, 1, 2, 3).cpu().double(), w.permute(0, 4, 1, 2, 3).cpu().double(), padding=1).permute(0, 2, 3, 4, 1)
    ref = (ref * scale.cpu().double() + shift.cpu().double()).clamp_min(0)
    rng = float(ref.abs().max())
    got, g32 = run_pair().cpu().double(), run_f32().cpu().double()
    assert bool(torch.isfinite(got).all()), f'{name}: the output is not finite'
    err = float((got - ref).abs().max())
    e_pair, e_f32 = float((got - ref).pow(2).mean().sqrt()), float((g32 - ref).pow(2).mean().sqrt())
    assert err <= 1e-4 * rng, f'{name}: max error {err:.3e} is {err / rng:.2e} of the range'
    assert e_pair <= 1.5 * e_f32 + 2e-7 * rng, f'{name}: rms error / range pair {e_pair / rng:.2e}, fp32 operands {e_f32 / rng:.2e}'
    return err / (1e-4 * rng), e_pair / (1.5 * e_f32 + 2e-7 * rng), gain


def _wino_layer(shape, co, a, seed):
    B, (X, Y, Z), ci = shape
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(co, 3, 3, 3, ci, generator=g) * (2.0 / (27 * ci)) ** 0.5).cuda()
    # shifts of the size of the response, so that the ReLU keeps about half of the outputs at every a
    return w, (torch.rand(co, generator=g) + 0.5).cuda(), (torch.randn(co, generator=g) * 0.1 * a).cuda()


@pytest.mark.parametrize('tile', [4, 6])
@pytest.mark.parametrize('shape', [(1, (12, 12, 3), 32), (2, (13, 14, 2), 64)], ids=['1x12x12x3-32', '2x13x14x2-64'])
def test_winograd_pair_operands_at_the_largest_gain(be, shape, tile):
    """The three-stage form and the chained form (amax_in = a producer's partial maxima) of the Winograd layers on fp16-pair operands, on
    an input whose B^T d B reaches the gain the operand scale allows for (100 of F(4,3), 225 of F(6,3), under the 2^8 of
    csrc/winograd.hip), with a = the largest fp32 below 2^e and 2^e itself, e = -20, 0, 13."""
    from imvoxelnet_amd import ops
    PAIR = ops.IVX_F16_PAIR
    ci = co = shape[2]
    worst = [0.0, 0.0, np.inf]
    eye = torch.zeros(ci, 3, 3, 3, ci)
    eye[torch.arange(ci), 1, 1, 1, torch.arange(ci)] = 1.0
    u_eye = ops.conv_winograd_weights(eye.cuda(), 1, tile)
    for i, a in enumerate(WINO_A):
        x = torch.from_numpy(_wino_input(shape, tile, a, 40 + i)).cuda()
        w, sc, sh = _wino_layer(shape, co, a, 60 + i)
        up, u32 = ops.conv_winograd_weights(w, 1, tile, operands=PAIR), ops.conv_winograd_weights(w, 1, tile)
        r = _wino_check(f'three-stage tile {tile} a {a!r}', x, w, sc, sh, tile,
                        lambda: ops.conv_winograd_fwd(x, up, sc, sh, 3, 1, (1, 1, 1), True, wgt_layout=1, operands=PAIR),
                        lambda: ops.conv_winograd_fwd(x, u32, sc, sh, 3, 1, (1, 1, 1), True, wgt_layout=1))
        # chained: a producer (the identity filter, fp32 operands) leaves y = x up to its own rounding and its per-workgroup maxima
        y, part = ops.conv_winograd_fwd(x, u_eye, None, None, 3, 1, (1, 1, 1), False, wgt_layout=1, want_amax=True)
        assert float(part.max()) == float(y.abs().max())
        r2 = _wino_check(f'chained tile {tile} a {a!r}', y, w, sc, sh, tile,
                         lambda: ops.conv_winograd_fwd(y, up, sc, sh, 3, 1, (1, 1, 1), True, wgt_layout=1, operands=PAIR, amax_in=part),
                         lambda: ops.conv_winograd_fwd(y, u32, sc, sh, 3, 1, (1, 1, 1), True, wgt_layout=1))
        worst = [max(worst[0], r[0], r2[0]), max(worst[1], r[1], r2[1]), min(worst[2], r[2], r2[2])]
    print(f'gpu winograd pair tile {tile} {shape}: worst max error / (1e-4 range) = {worst[0]:.3f}, rms / bar = {worst[1]:.3f}, smallest gain = {worst[2]:.2f}')


def test_winograd_fused_pair_operands_at_the_largest_gain(be):
    """ivx_conv_winograd_gemm_output_amax (F(4,3), GEMM + output transform in one launch) on the same kind of input"""
    from imvoxelnet_amd import ops
    PAIR = ops.IVX_F16_PAIR
    shape, tile = (1, (12, 8, 3), 64), 4
    worst = [0.0, 0.0, np.inf]
    for i, a in enumerate(WINO_A):
        x = torch.from_numpy(_wino_input(shape, tile, a, 80 + i)).cuda()
        w, sc, sh = _wino_layer(shape, 64, a, 90 + i)
        up, u32 = ops.conv_winograd_weights(w, 1, tile, operands=PAIR), ops.conv_winograd_weights(w, 1, tile)
        r = _wino_check(f'fused tile 4 a {a!r}', x, w, sc, sh, tile,
                        lambda: ops.conv_winograd_fwd(x, up, sc, sh, 3, 1, (1, 1, 1), True, wgt_layout=1, operands=PAIR, fused=True),
                        lambda: ops.conv_winograd_fwd(x, u32, sc, sh, 3, 1, (1, 1, 1), True, wgt_layout=1))
        worst = [max(worst[0], r[0]), max(worst[1], r[1]), min(worst[2], r[2])]
    print(f'gpu winograd fused pair {shape}: worst max error / (1e-4 range) = {worst[0]:.3f}, rms / bar = {worst[1]:.3f}, smallest gain = {worst[2]:.2f}')
