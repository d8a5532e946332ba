"""Plain fp64 references of the small operations around the convolutions (DCNv2 columns, max-pool, trilinear x2, layout changes,
global mean, max |x|), each written from the operation's definition with numpy / torch on the CPU: no device, no kernel of the
project.  tests/test_host_ops_fp64.py runs the CPU restatement of the C-ABI against them, tests/test_gpu_ops_fp64.py the HIP kernels."""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24            # relative error bound of one fp32 rounding (round to nearest)
K_DCN = 17                # roundings of dcn_im2col_kernel in units of U * A (counted in dcn_bound)
K_TRI = 7                 # roundings of upsample_trilinear2x_kernel in units of U * max |corner| (counted in trilinear_bound)
BF16_TINY = 2.0 ** -133   # the smallest bf16 denormal


# ---------------------------------------------------------------------------------------------------------------- storage formats
def bf16_round(x):
    """fp32 array -> the nearest bf16 value (ties to even), returned as fp32; NaN stays NaN."""
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).float().numpy()


def pair_decode(data, scale):
    """IVX_F16_PAIR storage, float16 [.., 2C] with [hi x16 | lo x16] per 16 channels, of scale * x -> fp32 [.., C].  hi + lo has at most 22
    significant bits and the scale is a power of two: both steps are exact in fp32."""
    d = np.asarray(data, np.float16)
    g = d.reshape(d.shape[:-1] + (d.shape[-1] // 32, 2, 16)).astype(np.float32)
    return ((g[..., 0, :] + g[..., 1, :]) / np.float32(scale)).reshape(d.shape[:-1] + (d.shape[-1] // 2,))


def pair_encode(x, scale):
    """fp32 [.., C] (C % 16 == 0) -> float16 [.., 2C]: hi = fp16(s x), lo = fp16(s x - hi), per 16 channels [hi x16 | lo x16]."""
    y = np.asarray(x, np.float32) * np.float32(scale)
    hi = y.astype(np.float16)
    lo = (y - hi.astype(np.float32)).astype(np.float16)
    g = np.stack([hi.reshape(y.shape[:-1] + (-1, 16)), lo.reshape(y.shape[:-1] + (-1, 16))], axis=-2)
    return np.ascontiguousarray(g.reshape(y.shape[:-1] + (2 * y.shape[-1],)))


def pair_round(v, scale):
    """The value an fp32 number has after the pair split with this scale (what pair_decode(pair_encode(v)) gives)."""
    return float(pair_decode(pair_encode(np.full((16,), v, np.float32), scale), scale)[0])


def pow2_scale(amax):
    """The scale rule of an IVX_F16_PAIR tensor: 2^k with amax * 2^k in [2^14, 2^15); 1 for a zero or non-finite maximum."""
    amax = float(np.float32(amax))
    if not (0.0 < amax < 3.0e38):
        return 1.0
    return 2.0 ** min(max(15 - int(np.frexp(amax)[1]), -120), 120)


# ---------------------------------------------------------------------------------------------------------------- DCNv2 columns
def dcn_out_hw(H, W, k, stride, pad, dil):
    return (H + 2 * pad - (dil * (k - 1) + 1)) // stride + 1, (W + 2 * pad - (dil * (k - 1) + 1)) // stride + 1


def dcn_coords(om, k, stride, pad, dil, pixels=None):
    """Sample coordinates (h_im, w_im), fp32 [P, k*k]: float32(ho * stride - pad + i * dil) + dh is ONE fp32 addition -- the coordinates
    are part of the operation's definition.  om [B,Ho,Wo,>=3k^2]; pixels: flat indices into (B, Ho, Wo), default all of them."""
    om = np.asarray(om, np.float32)
    B, Ho, Wo, _ = om.shape
    m = np.arange(B * Ho * Wo) if pixels is None else np.asarray(pixels, np.int64)
    rows = om.reshape(B * Ho * Wo, -1)[m]
    ho, wo = (m // Wo) % Ho, m % Wo
    i, j = np.divmod(np.arange(k * k), k)
    base_h = (ho[:, None] * stride - pad + i[None, :] * dil).astype(np.float32)
    base_w = (wo[:, None] * stride - pad + j[None, :] * dil).astype(np.float32)
    h = (base_h + rows[:, 0:2 * k * k:2]).astype(np.float32)
    w = (base_w + rows[:, 1:2 * k * k:2]).astype(np.float32)
    return h, w


def dcn_columns(x, om, k, stride, pad, dil, pixels=None):
    """Modulated deformable columns of a channels-last map x [B,H,W,C] (fp32: a map, or the exact decode of a bf16 / pair map) with the
    raw offset / mask channels om [B,Ho,Wo,>=3k^2] = [dh_0, dw_0, .., dh_{K-1}, dw_{K-1}, m_0 .. m_{K-1}, (unused)]:

        col[p, t, c] = sigmoid(m_t) * sum over the four corners of bilinear weight * x[b, corner, c]

    for a sample point with -1 < h_im < H and -1 < w_im < W, else 0; a corner outside the map is REPLACED by 0 (selected, not multiplied:
    0 * NaN is NaN, so a NaN of the map shows in exactly the columns that have it among their in-map corners).  Coordinates in fp32
    (dcn_coords); floor, fractions, weights, tests, blend, sigmoid and the product with it in fp64.
    Returns (col [P,k*k,C] fp64, A [P,k*k,C] fp64): A = sigmoid * max |in-map corner value|, the scale of the error bound (dcn_bound); A is
    0 exactly where the point or all four corners are outside (or every in-map corner is 0), NaN where col is."""
    x = np.asarray(x, np.float32)
    om = np.asarray(om, np.float32)
    B, H, W, C = x.shape
    _, Ho, Wo, _ = om.shape
    KK = k * k
    m = np.arange(B * Ho * Wo) if pixels is None else np.asarray(pixels, np.int64)
    b = m // (Ho * Wo)
    logits = om.reshape(B * Ho * Wo, -1)[m][:, 2 * KK:3 * KK].astype(np.float64)
    h32, w32 = dcn_coords(om, k, stride, pad, dil, pixels)
    col = np.zeros((len(m), KK, C))
    A = np.zeros((len(m), KK, C))
    for t in range(KK):
        h, w = h32[:, t].astype(np.float64), w32[:, t].astype(np.float64)
        inside = (h > -1) & (w > -1) & (h < H) & (w < W)
        hl, wl = np.floor(h), np.floor(w)
        lh, lw = h - hl, w - wl
        mask = 1.0 / (1.0 + np.exp(-logits[:, t]))
        acc = np.zeros((len(m), C))
        big = np.zeros((len(m), C))
        for hy, wx, wt in ((hl, wl, (1 - lh) * (1 - lw)), (hl, wl + 1, (1 - lh) * lw), (hl + 1, wl, lh * (1 - lw)), (hl + 1, wl + 1, lh * lw)):
            ok = inside & (hy >= 0) & (hy <= H - 1) & (wx >= 0) & (wx <= W - 1)
            v = x[b, np.clip(hy, 0, H - 1).astype(np.int64), np.clip(wx, 0, W - 1).astype(np.int64)].astype(np.float64)
            v = np.where(ok[:, None], v, 0.0)
            acc += wt[:, None] * v
            big = np.where(np.isnan(v) | np.isnan(big), np.nan, np.maximum(big, np.abs(v)))
        col[:, t] = acc * mask[:, None]
        A[:, t] = big * mask[:, None]
    return col, A


def dcn_bound(A):
    """|kernel - fp64| for the fp32 columns, first-order count of dcn_im2col_kernel's roundings in units of U = 2^-24 times
    A = mask * max |in-map corner|.  All weights lie in [0, 1] and the in-map weights sum to at most 1:
      lh = h_im - floor, lw               absolute error <= U/2 each (exact unless the point lies in (-1, 0))
      hh = 1 - lh, hw = 1 - lw            one more rounding: absolute error <= U each
      w1..w4 = products of two of them    carried error U+U, U+U/2, U/2+U, U/2+U/2 plus U/2 for the product: 2.5 + 2 + 2 + 1.5 = 8 U
      w_i * v_i                           one rounding each, relative: U * sum |w_i v_i| <= 1 U
      three additions                     3 U
      the product with the mask           1 U
      mask = 1 / (1 + expf(-m))           expf to 2 ulp, the addition, the division: 4 U relative
    K_DCN = 8 + 1 + 3 + 1 + 4 = 17 (fused multiply-adds only remove roundings).  The absolute term 2^-126 covers masks that underflow in
    fp32 (logits below -87: 0 or a denormal, where fp64 has a tiny non-zero value)."""
    return K_DCN * U * A + 2.0 ** -126


# ---------------------------------------------------------------------------------------------------------------- pools, resize
def maxpool2d(x, k, s, p):
    """nn.MaxPool2d(k, s, p) of a channels-last map [B,H,W,C] (fp32: a map or the exact decode of a bf16 / e4m3 map): F.max_pool2d on the
    CPU, which pads with -inf and propagates NaN.  Returns fp32 [B,Ho,Wo,C]."""
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32)).permute(0, 3, 1, 2)
    return F.max_pool2d(t, k, s, p).permute(0, 2, 3, 1).contiguous().numpy()


def _tri_axis(n):
    src = np.maximum(0.5 * (np.arange(2 * n) + 0.5) - 0.5, 0.0)
    i0 = np.floor(src).astype(np.int64)
    return i0, np.minimum(i0 + 1, n - 1), src - i0


def trilinear2x(x):
    """F.interpolate(scale_factor=2, mode='trilinear', align_corners=False) of a channels-last volume [B,D,H,W,C] in fp64: per axis the source
    coordinate max(0.5 * (o + 0.5) - 0.5, 0), neighbours i0 = floor and min(i0 + 1, n - 1), 8-corner blend.
    Returns (out [B,2D,2H,2W,C] fp64, M: max |corner| per output element, the scale of trilinear_bound)."""
    x = np.asarray(x, np.float64)
    B, D, H, W, C = x.shape
    (d0, d1, ld), (h0, h1, lh), (w0, w1, lw) = _tri_axis(D), _tri_axis(H), _tri_axis(W)
    out = np.zeros((B, 2 * D, 2 * H, 2 * W, C))
    M = np.zeros_like(out)
    for di, wd in ((d0, 1 - ld), (d1, ld)):
        for hi, wh in ((h0, 1 - lh), (h1, lh)):
            for wi, ww in ((w0, 1 - lw), (w1, lw)):
                v = x[:, di][:, :, hi][:, :, :, wi]
                out += (wd[:, None, None] * wh[None, :, None] * ww[None, None, :])[None, :, :, :, None] * v
                M = np.maximum(M, np.abs(v))
    return out, M


def trilinear_bound(M):
    """|kernel - fp64| of the fp32 resize: the weights 0, 0.25, 0.75, 1 are exact; the blend is a tree of three levels, each a pair of
    products and one addition of values bounded by M = max |corner| with weights that sum to 1: 2 U M per level, 6 U M in all; K_TRI = 7
    leaves one unit for the second-order terms; 2^-149 for a denormal result."""
    return K_TRI * U * M + 2.0 ** -149


# ---------------------------------------------------------------------------------------------------------------- layout, reductions
def nchw_to_nhwc(x, cpad=None):
    """[B,C,S] -> [B,S,Cpad], channels C .. Cpad-1 zero."""
    x = np.asarray(x)
    B, C, S = x.shape
    out = np.zeros((B, S, C if cpad is None else cpad), x.dtype)
    out[:, :, :C] = x.transpose(0, 2, 1)
    return out


def nhwc_to_nchw(x):
    """[B,S,C] -> [B,C,S]."""
    return np.ascontiguousarray(np.asarray(x).transpose(0, 2, 1))


def global_mean(x):
    """[B,S,C] -> ([B,C] fp64 mean over S, [B,C] fp64 mean |x|: the scale of avgpool_bound)."""
    x = np.asarray(x, np.float64)
    return x.mean(1), np.abs(x).mean(1)


def avgpool_bound(S, mean_abs):
    """global_avgpool_kernel: four sequential partial sums of ceil(S / 4) terms (each addition rounds a partial sum that is at most sum |x|),
    three additions of the partials and the division: (S/4 + 4) * U * mean |x|."""
    return (S / 4.0 + 4.0) * U * mean_abs


def amax(x):
    """max |x| in fp64 over the non-NaN elements (0 for an empty or all-NaN input)."""
    a = np.abs(np.asarray(x, np.float64)).ravel()
    a = a[~np.isnan(a)]
    return float(a.max()) if a.size else 0.0


# ---------------------------------------------------------------------------------------------------------------- inputs
def dcn_offsets_masks(seed, B, H, W, k, stride, pad, dil, om_channels):
    """Offsets and mask logits [B,Ho,Wo,om_channels] that drive every branch of the deformable sampling on purpose.  Per tap, by share:
      15 %  Gaussian offsets (sigma 2 pixels) rounded to integers: lh == 0 / lw == 0, the high corner has weight 0
      10 %  pushed far outside the map
       8 %  2 % for each band: h_im in (-1, 0), h_im in (H-1, H), w_im in (-1, 0), w_im in (W-1, W), the other coordinate inside the map:
            the point is inside, one corner row / column is not
       4 %  1 % each: h_im == -1, h_im == H, w_im == -1, w_im == W exactly (outside by the strict comparisons)
      rest  Gaussian offsets, sigma 2 pixels
    Mask logits: N(0, 2), 5 % -200 (fp32 sigmoid 0), 5 % -88 (denormal), 3 % +60 (1).  Channels beyond 3k^2 are NaN: nothing may read them."""
    rng = np.random.RandomState(seed)
    Ho, Wo = dcn_out_hw(H, W, k, stride, pad, dil)
    KK = k * k
    i, j = np.divmod(np.arange(KK), k)
    base_h = (np.arange(Ho)[:, None, None] * stride - pad + i[None, None, :] * dil + np.zeros((1, Wo, 1))).astype(np.float32)[None]
    base_w = (np.arange(Wo)[None, :, None] * stride - pad + j[None, None, :] * dil + np.zeros((Ho, 1, 1))).astype(np.float32)[None]
    dh = (rng.randn(B, Ho, Wo, KK) * 2).astype(np.float32)
    dw = (rng.randn(B, Ho, Wo, KK) * 2).astype(np.float32)
    r = rng.rand(B, Ho, Wo, KK)
    f = (0.01 + 0.98 * rng.rand(B, Ho, Wo, KK)).astype(np.float32)          # position inside a band
    in_h = (rng.rand(B, Ho, Wo, KK) * (H - 1)).astype(np.float32)           # a coordinate inside the map
    in_w = (rng.rand(B, Ho, Wo, KK) * (W - 1)).astype(np.float32)
    sgn = np.where(rng.rand(B, Ho, Wo, KK) < 0.5, -1.0, 1.0).astype(np.float32)
    s = r < 0.15
    dh[s], dw[s] = np.round(dh[s]), np.round(dw[s])
    s = (r >= 0.15) & (r < 0.25)
    dh[s] += (sgn * (max(H, W) + k * dil + 3))[s]
    bh, bw = np.broadcast_to(base_h, dh.shape), np.broadcast_to(base_w, dw.shape)
    for lo, target_h, target_w in ((0.25, -1 + f, in_w), (0.27, H - 1 + f, in_w), (0.29, in_h, -1 + f), (0.31, in_h, W - 1 + f),
                                   (0.33, np.full_like(f, -1), in_w), (0.34, np.full_like(f, H), in_w), (0.35, in_h, np.full_like(f, -1)),
                                   (0.36, in_h, np.full_like(f, W))):
        s = (r >= lo) & (r < lo + (0.02 if lo < 0.33 else 0.01))
        dh[s] = (target_h.astype(np.float32) - bh)[s]
        dw[s] = (target_w.astype(np.float32) - bw)[s]
    logit = (rng.randn(B, Ho, Wo, KK) * 2).astype(np.float32)
    rr = rng.rand(B, Ho, Wo, KK)
    logit[rr < 0.05] = -200.0
    logit[(rr >= 0.05) & (rr < 0.10)] = -88.0
    logit[rr > 0.97] = 60.0
    om = np.full((B, Ho, Wo, om_channels), np.nan, np.float32)
    om[..., 0:2 * KK:2], om[..., 1:2 * KK:2], om[..., 2 * KK:3 * KK] = dh, dw, logit
    return om


def dcn_shares(om, H, W, k, stride, pad, dil):
    """What an offset / mask map drives: the share of taps in each of the four half-outside bands (the point itself inside), of taps exactly
    on -1 / H / W, and of integer coordinates."""
    h, w = dcn_coords(om, k, stride, pad, dil)
    inside = (h > -1) & (w > -1) & (h < H) & (w < W)
    return dict(h_low=float((inside & (h < 0)).mean()), h_high=float((inside & (h > H - 1)).mean()),
                w_low=float((inside & (w < 0)).mean()), w_high=float((inside & (w > W - 1)).mean()),
                on_edge=float(((h == -1) | (h == H) | (w == -1) | (w == W)).mean()),
                integer=float((inside & (h == np.floor(h)) & (w == np.floor(w))).mean()))


def sample_pixels(seed, B, Ho, Wo, n):
    """n distinct flat pixel indices of (B, Ho, Wo), sorted: the four corners of the first image and the last pixel of the last image, the
    rest drawn with a fixed seed."""
    must = {0, Wo - 1, (Ho - 1) * Wo, Ho * Wo - 1, B * Ho * Wo - 1}
    rng = np.random.RandomState(seed)
    rest = rng.choice(B * Ho * Wo, size=min(n, B * Ho * Wo), replace=False)
    return np.array(sorted(must | set(rest.tolist())), np.int64)


# ---------------------------------------------------------------------------------------------------------------- checks
def check_dcn(name, got, ref, A, extra=None):
    """The assertions every column kernel has to meet: NaN exactly where the reference has it, exactly 0 where the point or all corners are
    outside, and |got - ref| <= dcn_bound(A) (+ extra: the storage rounding).  Returns the worst |got - ref| / (2^-24 A)."""
    got = np.asarray(got, np.float64).reshape(ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), f'{name}: NaN in {int(np.isnan(got).sum())} elements, reference {int(nan.sum())}'
    zero = (A == 0)
    assert np.all(got[zero] == 0), f'{name}: {int((got[zero] != 0).sum())} non-zero elements where the sample point or all corners are outside'
    fin = ~nan
    d = np.abs(got[fin] - ref[fin])
    bound = dcn_bound(A[fin]) + (0 if extra is None else extra[fin])
    pos = A[fin] > 2.0 ** -60            # (below: masks that underflow in fp32, covered by the absolute term)
    ratio = float((d[pos] / (U * A[fin][pos])).max()) if pos.any() else 0.0
    worst = float((d / bound).max()) if d.size else 0.0
    print(f'{name}: max |got - ref| / (2^-24 A) = {ratio:.3f}, / bound = {worst:.3f}, zero share {float((ref == 0).mean()):.3f}')
    assert worst <= 1.0, f'{name}: {int((d > bound).sum())} elements beyond the bound, worst {worst:.3f} x'
    return ratio


def check_shares(name, om, ref, H, W, k, s, p, d):
    """The inputs drive what they are meant to drive (maps with at least 2000 taps; a 1 x 1 map has 9)."""
    sh = dcn_shares(om, H, W, k, s, p, d)
    zero = float((ref == 0).mean())
    print(f'{name}: shares {sh}')
    if om.shape[0] * om.shape[1] * om.shape[2] * k * k >= 2000:
        assert 0.05 <= zero <= 0.6, (name, zero)
        assert min(sh['h_low'], sh['h_high'], sh['w_low'], sh['w_high']) >= 0.01 and sh['on_edge'] >= 0.01 and sh['integer'] >= 0.02, (name, sh)


# ---------------------------------------------------------------------------------------------------------------- cases
DCN_PARAMS = [(3, 1, 1, 1), (3, 2, 1, 1), (3, 1, 2, 2), (1, 1, 0, 1), (5, 2, 2, 1)]          # (k, stride, pad, dil)
DCN_CHANNELS = {'f32': (4, 8, 16, 64, 256), 'bf16': (8, 16, 64, 256), 'pair': (16, 64, 256)}


def dcn_small_cases(kind):
    """(seed, B, H, W, C, k, stride, pad, dil, om_channels): every window with every channel count of the storage type; the two map sizes,
    B in {1, 2, 3} and om_channels in {3k^2, 3k^2 + 1} alternate; then the degenerate maps 1 x 1, 1 x 2, 2 x 1."""
    cases, n = [], 0
    for pi, (k, s, p, d) in enumerate(DCN_PARAMS):
        for ci, C in enumerate(DCN_CHANNELS[kind]):
            H, W = ((23, 37), (29, 50))[(pi + ci) % 2]
            cases.append((1000 + n, 1 + n % 3, H, W, C, k, s, p, d, 3 * k * k + (n // 2 + pi) % 2))
            n += 1
    for H, W in ((1, 1), (1, 2), (2, 1)):
        for bi, (k, s, p, d) in enumerate(((3, 1, 1, 1), (1, 1, 0, 1), (5, 2, 2, 1))):
            cases.append((2000 + n, 1 + bi, H, W, 16, k, s, p, d, 3 * k * k + bi % 2))
            n += 1
    return cases


POOL_WINDOWS = [(3, 2, 1), (2, 2, 0), (3, 1, 1), (3, 3, 0), (1, 1, 0)]
POOL_SIZES = [(37, 53), (7, 9), (1, 1), (2, 3)]


def pool_small_cases(channels):
    """(seed, B, H, W, C, k, s, p) for every window x size that gives a non-empty output; C and B rotate."""
    cases, n = [], 0
    for k, s, p in POOL_WINDOWS:
        for H, W in POOL_SIZES:
            if H + 2 * p < k or W + 2 * p < k:
                continue
            cases.append((3000 + n, 1 + n % 3, H, W, channels[n % len(channels)], k, s, p))
            n += 1
    return cases


def pool_input(seed, shape, special=0.01):
    """fp32 values of both signs without zeros (the maximum of -0 and +0 has no defined sign), with -inf, +inf and NaN sprinkled in."""
    rng = np.random.RandomState(seed)
    x = (rng.randn(*shape) * 3).astype(np.float32)
    x[x == 0] = 1.0
    r = rng.rand(*shape)
    x[r < special] = -np.inf
    x[(r >= special) & (r < 2 * special)] = np.inf
    x[(r >= 2 * special) & (r < 3 * special)] = np.nan
    return x


TRI_CASES = [(1, 1, 5, 7, 4), (2, 3, 1, 6, 12), (1, 4, 5, 1, 64), (2, 3, 5, 7, 12), (1, 1, 1, 1, 4), (1, 2, 9, 11, 64)]      # B, D, H, W, C
TRI_LARGE = (1, 12, 40, 40, 64)            # 8 * 12 * 40 * 40 * 16 threads = 9600 blocks of 256: above the cap of 8192

LAYOUT_IMAGE_CASES = [(B, C, S) for C in (1, 2, 3, 4) for B, S in ((1, 64), (2, 65), (1, 130), (3, 31), (2, 1000))]          # pad_to = 4; S % 4 = 0, 1, 2, 3, 0
LAYOUT_TILE_CASES = [(1 + (C + S) % 2, C, S, pad) for C in (5, 31, 32, 33, 100) for S in (1, 31, 32, 33, 1000) for pad in (None, 8)]

AMAX_SIZES = [0, 1, 2, 3, 5, 4096, 1027, 3 * 2 ** 20 + 3]
AVGPOOL_S = [1, 3, 4, 35, 300]
AVGPOOL_C = [1, 63, 64, 65, 100, 2048]


def amax_inputs(n, seed):
    """Named inputs of n values in (-1, 1) with the maximum 7.5 (negative: the ABSOLUTE value counts) in the first element, the last
    element, and the first element of the n % 4 tail."""
    rng = np.random.RandomState(seed)
    base = (rng.rand(n) * 2 - 1).astype(np.float32)
    out = {'no peak': base}
    for name, pos in (('first', 0), ('last', n - 1), ('tail', n - (n % 4))):
        if 0 <= pos < n:
            a = base.copy()
            a[pos] = -7.5
            out[name] = a
    return out
