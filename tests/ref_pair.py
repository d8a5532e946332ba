"""The scale rule of the fp16 (hi, lo) pair tensors (include/imvoxel.h "Chained fp16-pair activations") at both ends of its contract,
against plain fp64: the formats, the fp64 references, the bound formulas of the header, the case builders, the drivers and the checkers
shared by tests/test_host_pair_range.py (the CPU restatement oracle/cpu_abi, no device) and tests/test_gpu_pair_range.py (the HIP library).

No kernel of the project is in here and no reference comes out of the library: the references take the values that the pair tensors and
the packed filters STAND FOR, decoded by this module's own decoder, so the quantisation of the operands is in no error budget.

Tight side: inputs built by the reference alone so that the output reaches the bound max|in| * wbound + sbound + max|res| (non-negative
filters with the same |scale| * L1 in every row, one positive shift, the input at its maximum on a block): the condition is
L = bound / max|ref| <= TIGHT_L, and the maximum `a` is solved so that the bound times 1.001 lies within 2^-12 below, or above, a power
of two.  Loose side: a dead channel (zero filters, a large negative shift: ReLU stores 0) makes the bound loose by a chosen factor L; the
storage term of a tensor T whose bound is loose by L is derived, not measured (storage_delta):

    the rule puts s * bound into [2^14, 2^15), so s * max|T| >= 2^14 / L; a value's pair is exact to 2^-22 of itself (22 significant bits)
    or, where its lo half is an fp16 subnormal (spacing 2^-24), to 2^-25 in scaled units, i.e. 2^-25 / s <= 2^-39 L max|T|:

    delta(T) = max(2^-22, 2^-39 L) * max|T|"""
import ctypes as C

import numpy as np

F32, PAIR = 0, 4                 # IVX_F32, IVX_F16_PAIR
SLOTS = 64                       # IVX_AMAX_SLOTS: the scale follows them in a tensor's scalar block
MARGIN = 1.001                   # the factor of the rule
TIGHT_L = 1.01
VALUE_TOL = 2e-5                 # of the reference's range: the bar of test_gpu_pair_chain / test_gpu_bottleneck / test_gpu_stem


# ------------------------------------------------------------------------------------------------------------------ formats
def pow2_scale(amax):
    """2^k with amax * 2^k in [2^14, 2^15); 1 for a zero or non-finite maximum"""
    amax = float(amax)
    if not (0.0 < amax < 3.0e38):
        return 1.0
    return 2.0 ** min(max(15 - int(np.frexp(amax)[1]), -120), 120)


def split(x, scale):
    """fp32 values -> (hi, lo) float16 of scale * x: hi = fp16(s x), lo = fp16(s x - hi), round to nearest even, subnormals kept"""
    y = np.asarray(x, np.float32) * np.float32(scale)
    hi = y.astype(np.float16)
    return hi, (y - hi.astype(np.float32)).astype(np.float16)


def pair_round(x, scale):
    """the values fp32 numbers stand for after the split (elementwise, any shape), fp64"""
    hi, lo = split(x, scale)
    return (hi.astype(np.float64) + lo.astype(np.float64)) / float(scale)


def pair_encode(x, scale):
    """fp32 [.., C] (C % 16 == 0) -> float16 [.., 2C], per 16 channels [hi x16 | lo x16]"""
    hi, lo = split(x, scale)
    g = np.stack([hi.reshape(hi.shape[:-1] + (-1, 16)), lo.reshape(lo.shape[:-1] + (-1, 16))], axis=-2)
    return np.ascontiguousarray(g.reshape(hi.shape[:-1] + (2 * hi.shape[-1],)))


def pair_decode(data, scale):
    """float16 [.., 2C] -> fp64 [.., C] = (hi + lo) / scale"""
    d = np.asarray(data, np.float16)
    g = d.reshape(d.shape[:-1] + (d.shape[-1] // 32, 2, 16)).astype(np.float64)
    return ((g[..., 0, :] + g[..., 1, :]) / float(scale)).reshape(d.shape[:-1] + (d.shape[-1] // 2,))


def filters_encode(w, s_w):
    """fp32 [Cout, taps, Cin] -> the layout of ivx_pair_pack_filters: float16 [Cout, Cin/32, taps, 64] = [hi16 | lo16 | hi16 | lo16] of s_w * w"""
    co, taps, ci = w.shape
    hi, lo = split(w, s_w)
    hi = hi.reshape(co, taps, ci // 32, 2, 16).transpose(0, 2, 1, 3, 4)
    lo = lo.reshape(co, taps, ci // 32, 2, 16).transpose(0, 2, 1, 3, 4)
    return np.ascontiguousarray(np.stack([hi, lo], axis=4).reshape(co, ci // 32, taps, 64))


def filters_decode(packed):
    """float16 [Cout, Cin/32, taps, 64] -> fp64 [Cout, taps, Cin]: the values s_w * w the pair filters stand for"""
    p = np.asarray(packed, np.float16)
    co, nch, taps, _ = p.shape
    g = p.reshape(co, nch, taps, 2, 2, 16).astype(np.float64)
    return (g[..., 0, :] + g[..., 1, :]).reshape(co, nch, taps, 32).transpose(0, 2, 1, 3).reshape(co, taps, nch * 32)


def stem_decode(frag):
    """the fragments of ivx_stem_pool_pack_filters, halves [column tile 2][step 11][hi, lo][lane 64][8]: lane = h * 32 + n_l holds output
    channel nt * 32 + n_l and the (channel, row) pair pq = 2 * step + h = c * 7 + ky, the 8 halves are the filter's columns -> fp64 [64, 3, 7, 7]"""
    f = np.frombuffer(np.ascontiguousarray(frag).tobytes(), np.float16).reshape(2, 11, 2, 64, 8).astype(np.float64)
    v = f[:, :, 0] + f[:, :, 1]
    w = np.zeros((64, 3, 7, 7))
    for nt in range(2):
        for kk in range(11):
            for lane in range(64):
                pq = 2 * kk + (lane >> 5)
                if pq < 21:
                    w[nt * 32 + (lane & 31), pq // 7, pq % 7] = v[nt, kk, lane, :7]
    return w


class PairT:
    """A pair tensor on the host: data float16 [B, H, W, 2C], its scale, and the true maximum of the values it stands for"""

    def __init__(self, data, scale, amax=None):
        self.data, self.scale = data, float(scale)
        self.value = pair_decode(data, scale)
        self.amax = float(np.abs(self.value).max()) if amax is None else float(amax)
        assert float(np.float32(self.amax)) == self.amax          # hi + lo has at most 22 bits


def make_pair(x, below=0):
    """fp32 [B, H, W, C] -> PairT with the scale the rule gives its maximum, divided by 2^below (a loosely scaled tensor)"""
    x = np.asarray(x, np.float32)
    return PairT(pair_encode(x, pow2_scale(np.abs(x).max()) / 2.0 ** below), pow2_scale(np.abs(x).max()) / 2.0 ** below)


def make_slots(amax=0.0, scale=None, slot=7):
    """the scalar block of a tensor: SLOTS words of max |tensor| (any slot: the readers take the maximum of all), then the scale"""
    s = np.zeros(SLOTS + 16, np.int32)
    s[:SLOTS].view(np.float32)[slot] = amax
    if scale is not None:
        s[SLOTS:SLOTS + 1].view(np.float32)[0] = scale
    return s


def slots_amax(s):
    return float(np.asarray(s)[:SLOTS].view(np.float32).max())


def slots_scale(s):
    return float(np.asarray(s)[SLOTS:SLOTS + 1].view(np.float32)[0])


# ------------------------------------------------------------------------------------------------------------------ fp64 references
def out_hw(H, W, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def conv2d(x, w, scale, shift, k, stride, pad, relu=True, res=None, res_mode=0, post_scale=1.0, res_after_act=False):
    """x [B, H, W, Cin], w [Cout, k*k, Cin] (tap-major), fp64.  v = acc * scale + shift; v += res (res_mode 1: the output's shape, 2: nearest
    neighbour from [B, h, w, Cout]); ReLU; (res_after_act: the residual is added here instead); v *= post_scale"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, H, W, ci = x.shape
    co = w.shape[0]
    Ho, Wo = out_hw(H, W, k, stride, pad)
    xp = np.zeros((B, H + 2 * pad, W + 2 * pad, ci))
    xp[:, pad:pad + H, pad:pad + W] = x
    acc = np.zeros((B * Ho * Wo, co))
    for ky in range(k):
        for kx in range(k):
            sl = xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]
            acc += sl.reshape(-1, ci) @ w[:, ky * k + kx].T
    v = acc.reshape(B, Ho, Wo, co) * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)
    r = None
    if res is not None:
        r = np.asarray(res, np.float64)
        if res_mode == 2:
            r = r[:, (np.arange(Ho) * r.shape[1]) // Ho][:, :, (np.arange(Wo) * r.shape[2]) // Wo]
    if r is not None and not res_after_act:
        v = v + r
    if relu:
        v = np.maximum(v, 0.0)
    if r is not None and res_after_act:
        v = v + r
    return v * float(post_scale)


def maxpool(x, k=3, s=2, p=1):
    """nn.MaxPool2d on [B, H, W, C]: padding counts as -inf"""
    B, H, W, Cn = x.shape
    Ho, Wo = out_hw(H, W, k, s, p)
    xp = np.full((B, H + 2 * p, W + 2 * p, Cn), -np.inf)
    xp[:, p:p + H, p:p + W] = x
    out = np.full((B, Ho, Wo, Cn), -np.inf)
    for e in range(k):
        for f in range(k):
            out = np.maximum(out, xp[:, e:e + (Ho - 1) * s + 1:s, f:f + (Wo - 1) * s + 1:s])
    return out


def bottleneck(x, layers, proj=None):
    """ResNet bottleneck, stride 1.  layers: three (w, scale, shift) with w [Cout, taps, Cin]; identity: out = relu(bn3(conv3(..)) + x).
    proj = (bank [4P, 1, Cin + P], scale, shift): the joint 1x1 over [x | mid2] (ivx_bottleneck_proj_pack), out = relu(that).
    Returns (mid1, mid2, out)."""
    (w1, s1, t1), (w2, s2, t2) = layers[0], layers[1]
    m1 = conv2d(x, w1, s1, t1, 1, 1, 0)
    m2 = conv2d(m1, w2, s2, t2, 3, 1, 1)
    if proj is None:
        w3, s3, t3 = layers[2]
        return m1, m2, conv2d(m2, w3, s3, t3, 1, 1, 0, res=x, res_mode=1)
    wb, sb, tb = proj
    return m1, m2, conv2d(np.concatenate([np.asarray(x, np.float64), m2], -1), wb, sb, tb, 1, 1, 0)


def stem_pool(img, w, scale, shift):
    """img [B, 3, H, W], w [64, 3, 7, 7]: conv 7x7 stride 2 pad 3 + affine + ReLU + MaxPool(3, 2, 1) -> [B, Hp, Wp, 64]"""
    x = np.asarray(img, np.float64).transpose(0, 2, 3, 1)
    wt = np.asarray(w, np.float64).transpose(0, 2, 3, 1).reshape(64, 49, 3)
    return maxpool(conv2d(x, wt, scale, shift, 7, 2, 3))


# ------------------------------------------------------------------------------------------------------------------ the bounds of the header
def conv_bound(a, wb, sb, r=0.0, post=1.0, f=np.float64):
    """(max|in| * wbound + sbound + max|res|) * |post_scale| * 1.001 in the precision f, in the order of csrc/conv_igemm.hip conv_pair_io"""
    a, wb, sb, r, post = f(a), f(wb), f(sb), f(r), f(abs(post) if post else 1.0)
    return (a * wb + sb + r) * post * f(MARGIN)


def bottleneck_bounds(a, wb, sb, wbd=None, f=np.float64):
    """b1, b2, b3 of csrc/bottleneck.hip (each times 1.001); wbd None: the identity shortcut (+ max|in|), else + max|in| * wboundd"""
    a, m = f(a), f(MARGIN)
    b1 = (a * f(wb[0]) + f(sb[0])) * m
    b2 = (b1 * f(wb[1]) + f(sb[1])) * m
    b3 = (b2 * f(wb[2]) + f(sb[2]) + a * f(1.0 if wbd is None else wbd)) * m
    return b1, b2, b3


def allowed_scales(b64, b32):
    """The scale the rule must choose for the bound b64 (fp64, margin included), and the neighbouring power of two only where the fp32
    evaluation b32 of the same bound lies within 2^-20 of the boundary."""
    s = pow2_scale(b64)
    ok = {s}
    m, _ = np.frexp(float(b32))                     # b32 = m 2^e, m in [0.5, 1)
    if 2 * m - 1 <= 2.0 ** -20:                     # just above a boundary: its own scale and the one of the values below
        ok |= {pow2_scale(float(b32)), pow2_scale(float(b32)) * 2}
    if 1 - m <= 2.0 ** -20:
        ok |= {pow2_scale(float(b32)), pow2_scale(float(b32)) / 2}
    return s, ok


def solve_amax(bound_of, nominal, side):
    """bound_of(a) is affine in a (fp64, margin included).  The a for which it lies 2^-13 below (side 'below') or above ('above') the power
    of two nearest to bound_of(nominal) in the logarithm; the caller rounds a into its tensor and asserts the side with side_ok."""
    T = 2.0 ** round(np.log2(float(bound_of(nominal))))
    f0, f1 = float(bound_of(0.0)), float(bound_of(1.0))
    a = (T * (1 - 2.0 ** -13 if side == 'below' else 1 + 2.0 ** -13) - f0) / (f1 - f0)
    assert a > 0, 'the constant terms alone exceed the target'
    return a, T


def side_ok(b64, T, side):
    return (T * (1 - 2.0 ** -12) < b64 < T) if side == 'below' else (T <= b64 < T * (1 + 2.0 ** -12))


def storage_delta(T, L):
    """the storage error of a pair tensor whose bound is loose by L (module docstring), absolute"""
    return max(2.0 ** -22, 2.0 ** -39 * L) * float(np.abs(T).max())


# ------------------------------------------------------------------------------------------------------------------ backends
class ConvDesc(C.Structure):                    # ivx_conv_desc
    _fields_ = [(n, C.c_int32) for n in ('B', 'D', 'H', 'W', 'Cin', 'Cout', 'KD', 'KH', 'KW', 'sd', 'sh', 'sw', 'pd', 'ph', 'pw', 'relu', 'res_mode',
                                         'res_h', 'res_w', 'wgt_layout', 'out_mode', 'res_after_act')] + \
        [('post_scale', C.c_float), ('in_dtype', C.c_int32), ('out_dtype', C.c_int32), ('res_scale', C.c_float), ('wino_operands', C.c_int32)]


class PairIO(C.Structure):                      # ivx_pair_io
    _fields_ = [('in_scale', C.c_void_p), ('res_scale', C.c_void_p), ('res_dtype', C.c_int32), ('out_scale', C.c_void_p), ('amax_in', C.c_void_p),
                ('amax_res', C.c_void_p), ('amax_out', C.c_void_p), ('wbound', C.c_float), ('sbound', C.c_float)]


class BottleneckDesc(C.Structure):              # ivx_bottleneck_desc
    _fields_ = [(n, C.c_int32) for n in ('B', 'H', 'W', 'P')]


class BottleneckIO(C.Structure):                # ivx_bottleneck_io
    _fields_ = [('in_scale', C.c_void_p), ('amax_in', C.c_void_p), ('out_scale', C.c_void_p), ('amax_out', C.c_void_p), ('wbound', C.c_float * 3),
                ('sbound', C.c_float * 3)]


def bind(L):
    """argument types of the entry points used here (include/imvoxel.h), for a library loaded without them"""
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    pf = C.POINTER(f32)
    L.ivx_last_error.restype = C.c_char_p
    for name, res, args in [
            ('ivx_pair_pack_filters', C.c_int, [vp, i32, i32, i32, vp, vp, vp, vp, pf, pf]),
            ('ivx_bottleneck_proj_pack', C.c_int, [vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, pf, pf, pf]),
            ('ivx_stem_pool_filter_bytes', i64, []),
            ('ivx_stem_pool_pack_filters', C.c_int, [vp, vp, vp, vp]),
            ('ivx_conv_pio_workspace_bytes', i64, [C.POINTER(ConvDesc), C.POINTER(PairIO)]),
            ('ivx_conv_fwd_pio', C.c_int, [C.POINTER(ConvDesc), C.POINTER(PairIO), vp, vp, vp, vp, vp, vp, vp, i64, vp]),
            ('ivx_conv_fwd', C.c_int, [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp]),
            ('ivx_bottleneck_fwd_pio', C.c_int, [C.POINTER(BottleneckDesc), C.POINTER(BottleneckIO)] + [vp] * 12),
            ('ivx_bottleneck_proj_fwd_pio', C.c_int, [C.POINTER(BottleneckDesc), i32, C.POINTER(BottleneckIO), f32] + [vp] * 12),
            ('ivx_amax_f32', C.c_int, [vp, i64, vp, vp]),
            ('ivx_stem_pool_fwd_pair', C.c_int, [vp, i32, i32, i32, vp, vp, vp, f32, f32, vp, vp, vp, vp, vp]),
            ('ivx_nchw_to_nhwc_amax', C.c_int, [vp, i32, i32, i64, i32, vp, vp, vp]),
            ('ivx_maxpool2d_fwd_pair', C.c_int, [vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, f32, f32, vp, vp, vp]),
            ('ivx_dcn_im2col_fwd_pair', C.c_int, [vp, vp, vp] + [i32] * 10 + [vp, vp, vp, vp])]:
        f = getattr(L, name)
        f.restype, f.argtypes = res, args


class HostBackend:
    """The entry points on host memory (the CPU restatement).  tests/test_gpu_pair_range.py has the device twin with the same methods."""
    name = 'cpu'
    ConvDesc, PairIO, BottleneckDesc, BottleneckIO = ConvDesc, PairIO, BottleneckDesc, BottleneckIO

    def __init__(self, L):
        self.L = L
        bind(L)
        self.stream = None

    def up(self, a):
        return np.ascontiguousarray(a).copy()

    def full(self, shape, dtype, fill):
        return np.full(shape, fill, dtype)

    def addr(self, h, byte_offset=0):
        return h.ctypes.data + byte_offset

    def get(self, h):
        return h

    def ok(self, rc, what):
        assert rc == 0, f'{what}: {self.L.ivx_last_error().decode()}'


def _p(be, h, off=0):
    return C.c_void_p(be.addr(h, off)) if h is not None else None


def _hp(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


# ------------------------------------------------------------------------------------------------------------------ the host-only packers
def pack_filters(be, w, scale, shift, packed=True):
    """ivx_pair_pack_filters on fp32 [Cout, taps, Cin] -> (float16 [Cout, Cin/32, taps, 64] or None, scale / s_w or None, wbound, sbound)"""
    w = np.ascontiguousarray(w, np.float32)
    co, taps, ci = w.shape
    sc = None if scale is None else np.ascontiguousarray(scale, np.float32)
    sf = None if shift is None else np.ascontiguousarray(shift, np.float32)
    out = np.full((co, ci // 32, taps, 64), np.nan, np.float16) if packed else None
    sp = np.full(co, np.nan, np.float32) if packed else None
    wb, sb = C.c_float(), C.c_float()
    be.ok(be.L.ivx_pair_pack_filters(_hp(w), co, taps, ci, _hp(sc), _hp(sf), _hp(out), _hp(sp), C.byref(wb), C.byref(sb)), 'ivx_pair_pack_filters')
    return out, sp, wb.value, sb.value


def pack_proj(be, w3, scale3, shift3, wd, scaled, shiftd):
    """ivx_bottleneck_proj_pack: w3 [4P, P], wd [4P, Cin] -> (bank float16 [4P, (Cin + P)/32, 1, 64], scale_out, shift_out, wbound3, sbound, wboundd)"""
    a = [np.ascontiguousarray(t, np.float32) for t in (w3, scale3, shift3, wd, scaled, shiftd)]
    C4, P = a[0].shape
    Cin = a[3].shape[1]
    out = np.full((C4, (Cin + P) // 32, 1, 64), np.nan, np.float16)
    sc, sf = np.full(C4, np.nan, np.float32), np.full(C4, np.nan, np.float32)
    wb3, sb, wbd = C.c_float(), C.c_float(), C.c_float()
    be.ok(be.L.ivx_bottleneck_proj_pack(*[_hp(t) for t in a], P, Cin, _hp(out), _hp(sc), _hp(sf), C.byref(wb3), C.byref(sb), C.byref(wbd)),
          'ivx_bottleneck_proj_pack')
    return out, sc, sf, wb3.value, sb.value, wbd.value


def pack_stem(be, w, scale, shift):
    """ivx_stem_pool_pack_filters + the bound terms as both hosts compute them: ivx_pair_pack_filters without a packed output on the
    tap-major filters [64, 49, 4] (three channels padded to four).  -> (fragments uint8, scale / s_w, wbound, sbound)"""
    w = np.ascontiguousarray(w, np.float32)
    sc = np.ascontiguousarray(scale, np.float32)
    frag = np.zeros(int(be.L.ivx_stem_pool_filter_bytes()), np.uint8)
    sp = np.full(64, np.nan, np.float32)
    be.ok(be.L.ivx_stem_pool_pack_filters(_hp(w), _hp(sc), _hp(frag), _hp(sp)), 'ivx_stem_pool_pack_filters')
    _, _, wb, sb = pack_filters(be, stem_taps(w), scale, shift, packed=False)
    return frag, sp, wb, sb


def stem_taps(w):
    """[64, 3, 7, 7] -> tap-major [64, 49, 4] fp32, the fourth channel zero"""
    t = np.zeros((64, 49, 4), np.float32)
    t[:, :, :3] = np.asarray(w, np.float32).transpose(0, 2, 3, 1).reshape(64, 49, 3)
    return t


def filter_scale(scale, scale_p):
    """s_w from the two scale vectors (scale_p = scale / s_w): a power of two, the same for every channel"""
    s_w = np.asarray(scale, np.float64) / np.asarray(scale_p, np.float64)
    assert np.all(s_w == s_w[0]) and np.log2(s_w[0]) == int(np.log2(s_w[0])), 's_w is not one power of two'
    return float(s_w[0])


def check_bound_term(name, got, exact):
    """exact <= got <= exact * (1 + 2^-20).  A term that is exactly 0 comes out as the smallest fp32 denormal (the packers step to the next
    float above the rounded value): that is allowed."""
    if exact == 0:
        assert 0 <= got <= 2.0 ** -149, f'{name}: {got!r} for a zero term'
        return 0.0
    assert exact <= got <= exact * (1 + 2.0 ** -20) + 1e-300, f'{name}: {got!r} against the exact {exact!r} (ratio - 1 = {got / max(exact, 1e-300) - 1:.3e})'
    return got / exact - 1 if exact > 0 else 0.0


def check_pack(be, name, w, scale, shift):
    """ivx_pair_pack_filters: the layout (bit-identical to filters_encode), the filter scale, the round trip, and the bound terms against
    their definition over the DECODED filters.  Returns (wbound / exact - 1, sbound / exact - 1)."""
    packed, sp, wb, sb = pack_filters(be, w, scale, shift)
    s_w = filter_scale(scale, sp)
    wmax = float(np.abs(w).max())
    assert 2.0 ** 14 <= s_w * wmax < 2.0 ** 15, f'{name}: s_w * max|w| = {s_w * wmax}'
    assert np.array_equal(packed.view(np.uint16), filters_encode(w, s_w).view(np.uint16)), f'{name}: packed halves differ from the stated layout'
    dec = filters_decode(packed) / s_w
    assert float(np.abs(dec - w.astype(np.float64)).max()) <= 2.0 ** -21 * wmax, f'{name}: round trip'
    e_w = float((np.abs(np.asarray(scale, np.float64)) * np.abs(dec).sum((1, 2))).max())
    e_s = float(np.abs(np.asarray(shift, np.float64)).max())
    return check_bound_term(f'{name} wbound', wb, e_w), check_bound_term(f'{name} sbound', sb, e_s)


def check_pack_proj(be, name, w3, scale3, shift3, wd, scaled, shiftd):
    """ivx_bottleneck_proj_pack: the joint bank [scaled * wd | scale3 * w3] * s_w, wbound3 / wboundd / sbound over the decoded bank"""
    bank, sc, sf, wb3, sb, wbd = pack_proj(be, w3, scale3, shift3, wd, scaled, shiftd)
    Cin = wd.shape[1]
    s_w = filter_scale(np.ones(len(sc)), sc)
    folded = np.concatenate([np.asarray(scaled, np.float64)[:, None] * wd, np.asarray(scale3, np.float64)[:, None] * w3], 1)
    fmax = float(np.abs(folded).max())
    assert 2.0 ** 14 <= s_w * float(np.float32(fmax)) < 2.0 ** 15, f'{name}: s_w * max|w| = {s_w * fmax}'
    dec = filters_decode(bank)[:, 0] / s_w
    assert float(np.abs(dec - folded).max()) <= 2.0 ** -21 * fmax, f'{name}: round trip'
    assert np.array_equal(sf, (np.asarray(shift3, np.float32) + np.asarray(shiftd, np.float32)).astype(np.float32))
    return (check_bound_term(f'{name} wbound3', wb3, float(np.abs(dec[:, Cin:]).sum(1).max())),
            check_bound_term(f'{name} wboundd', wbd, float(np.abs(dec[:, :Cin]).sum(1).max())),
            check_bound_term(f'{name} sbound', sb, float(np.abs(sf.astype(np.float64)).max())))


def check_pack_stem(be, name, w, scale, shift):
    """the stem's bound terms, as the hosts compute them, against the decoded fragments of ivx_stem_pool_pack_filters"""
    frag, sp, wb, sb = pack_stem(be, w, scale, shift)
    s_w = filter_scale(scale, sp)
    wmax = float(np.abs(w).max())
    assert 2.0 ** 14 <= s_w * wmax < 2.0 ** 15, f'{name}: s_w * max|w| = {s_w * wmax}'
    dec = stem_decode(frag) / s_w
    assert float(np.abs(dec - np.asarray(w, np.float64)).max()) <= 2.0 ** -21 * wmax, f'{name}: round trip'
    e_w = float((np.abs(np.asarray(scale, np.float64)) * np.abs(dec).sum((1, 2, 3))).max())
    return check_bound_term(f'{name} wbound', wb, e_w), check_bound_term(f'{name} sbound', sb, float(np.abs(np.asarray(shift, np.float64)).max()))


# ------------------------------------------------------------------------------------------------------------------ filters of the cases
def tight_filters(r, co, taps, ci, gain, shift):
    """non-negative filters, every row with the same scale * L1 = gain, one positive shift"""
    w = (r.uniform(0.2, 1.0, (co, taps, ci)) / (taps * ci)).astype(np.float32)
    scale = (gain / w.astype(np.float64).sum((1, 2))).astype(np.float32)
    return w, scale, np.full(co, shift, np.float32)


def mixed_filters(r, co, taps, ci, gain, shift):
    """filters, scales and shifts of both signs; the row of largest |scale| * L1 (returned) has the largest |shift|, of its scale's sign"""
    w = (r.randn(co, taps, ci) * (2.0 / (taps * ci)) ** 0.5).astype(np.float32)
    l1 = np.abs(w.astype(np.float64)).sum((1, 2))
    scale = (r.uniform(0.5, 1.0, co) * r.choice([-1.0, 1.0], co) * gain / l1.max()).astype(np.float32)
    row = int(np.argmax(np.abs(scale.astype(np.float64)) * l1))
    sh = r.uniform(-0.8, 0.8, co) * shift
    sh[row] = np.sign(scale[row]) * shift
    return w, scale, sh.astype(np.float32), row


def random_filters(r, co, taps, ci):
    """He-initialised filters with BatchNorm-like vectors, as the other pair tests draw them"""
    w = (r.randn(co, taps, ci) * (2.0 / (taps * ci)) ** 0.5).astype(np.float32)
    return w, (r.rand(co) + 0.5).astype(np.float32), (r.randn(co) * 0.1).astype(np.float32)


def pack_cases():
    """(name, w, scale, shift): Cin 32 .. 2048, taps 1 and 9, random and the filters of the tight and loose constructions"""
    out = []
    for ci, co, taps in [(32, 16, 1), (32, 64, 9), (64, 64, 9), (96, 32, 1), (256, 64, 1), (512, 64, 9), (2048, 64, 1), (2048, 16, 9)]:
        r = np.random.RandomState(ci + co + taps)
        out.append((f'random {ci}->{co} taps {taps}',) + random_filters(r, co, taps, ci))
        out.append((f'tight {ci}->{co} taps {taps}',) + tight_filters(r, co, taps, ci, 1.5, 0.25))
        out.append((f'mixed {ci}->{co} taps {taps}',) + mixed_filters(r, co, taps, ci, 1.5, 0.25)[:3])
        w, sc, sh = random_filters(r, co, taps, ci)
        w[3], sh[3] = 0.0, -2.0 ** 20                                   # a dead channel: sbound
        out.append((f'dead shift {ci}->{co} taps {taps}', w, sc, sh))
        w, sc, sh = random_filters(r, co, taps, ci)
        w[5], sh[5] = np.float32(37.3), -1e6                            # a dead channel with huge filters: wbound, and the others' lo halves go subnormal
        out.append((f'dead filters {ci}->{co} taps {taps}', w, sc, sh))
        w = np.full((co, taps, ci), np.float32(1.0 + 2.0 ** -11 + 2.0 ** -22), np.float32) / np.float32(ci)      # equal values
        out.append((f'equal {ci}->{co} taps {taps}', w, np.ones(co, np.float32), np.zeros(co, np.float32)))
    return out


# ------------------------------------------------------------------------------------------------------------------ ivx_conv_fwd_pio
def run_conv(be, x, packed, scale_p, shift, k, stride, pad, wb, sb, relu=True, res=None, res_mode=0, out_pair=True, post_scale=1.0, res_after_act=False):
    """One ivx_conv_fwd_pio call.  x: PairT [B, H, W, Cin]; res: None, a PairT or (fp32 array, its maximum).  The output is pre-filled with
    NaN.  Returns dict(data: float16 pairs or fp32 [B, Ho, Wo, .], scale, rec: the recorded maximum)."""
    L = be.L
    B, H, W, ci = x.value.shape
    co = packed.shape[0]
    Ho, Wo = out_hw(H, W, k, stride, pad)
    d = be.ConvDesc()
    d.B, d.D, d.H, d.W, d.Cin, d.Cout, d.KD, d.KH, d.KW = B, 1, H, W, ci, co, 1, k, k
    d.sd, d.sh, d.sw, d.pd, d.ph, d.pw, d.relu, d.wgt_layout = 1, stride, stride, 0, pad, pad, int(relu), 1
    d.post_scale, d.in_dtype, d.out_dtype, d.res_scale, d.res_after_act = post_scale, PAIR, PAIR if out_pair else F32, 1.0, int(res_after_act)
    io = be.PairIO()
    xin, sl_in = be.up(x.data), be.up(make_slots(x.amax, x.scale))
    io.in_scale, io.amax_in = be.addr(sl_in, 4 * SLOTS), be.addr(sl_in)
    rd = sl_res = None
    if res is not None:
        d.res_mode = res_mode or 1
        if isinstance(res, PairT):
            rd, sl_res = be.up(res.data), be.up(make_slots(res.amax, res.scale, slot=3))
            io.res_dtype, io.res_scale = PAIR, be.addr(sl_res, 4 * SLOTS)
            rshape = res.value.shape
        else:
            rd, sl_res = be.up(np.asarray(res[0], np.float32)), be.up(make_slots(res[1], slot=3))
            rshape = res[0].shape
        io.amax_res = be.addr(sl_res)
        if d.res_mode == 2:
            d.res_h, d.res_w = rshape[1], rshape[2]
    sl_out = be.up(make_slots())
    io.amax_out, io.out_scale = be.addr(sl_out), be.addr(sl_out, 4 * SLOTS)
    io.wbound, io.sbound = wb, sb
    out = be.full((B, Ho, Wo, 2 * co), np.float16, np.nan) if out_pair else be.full((B, Ho, Wo, co), np.float32, np.nan)
    wd, sd, fd = be.up(packed), be.up(np.asarray(scale_p, np.float32)), be.up(np.asarray(shift, np.float32))
    nb = L.ivx_conv_pio_workspace_bytes(C.byref(d), C.byref(io))
    assert nb >= 0, 'ivx_conv_pio_workspace_bytes'
    ws = be.full((max(int(nb), 256),), np.uint8, 0)
    be.ok(L.ivx_conv_fwd_pio(C.byref(d), C.byref(io), _p(be, xin), _p(be, wd), _p(be, sd), _p(be, fd), _p(be, rd), _p(be, out), _p(be, ws), int(nb),
                             be.stream), 'ivx_conv_fwd_pio')
    so = be.get(sl_out)
    return dict(data=be.get(out), scale=slots_scale(so), rec=slots_amax(so))


def check_pair_output(name, got, ref, allowed=None, extra=0.0, store=0.0, tol=VALUE_TOL):
    """got: dict(data, scale, rec) of a pair output; ref fp64.  Every stored half finite, s_out * max|ref| < 2^15, the scale among `allowed`
    (a pair (stated, set)), the recorded maximum (of the values before the split) = max|out| to 2^-20 of it plus `store`, the storage term
    of this tensor on the loose side, |out - ref| <= tol * range + extra.  Returns error / bound."""
    data = np.asarray(got['data'])
    assert np.isfinite(data.astype(np.float32)).all(), f'{name}: {int((~np.isfinite(data.astype(np.float32))).sum())} stored halves are not finite'
    s = got['scale']
    rng = float(np.abs(ref).max())
    assert s * rng < 2.0 ** 15, f'{name}: s_out * max|ref| = {s * rng} reaches 2^15'
    if allowed is not None:
        assert s in allowed[1], f'{name}: out_scale 2^{np.log2(s):.0f}, the rule must choose 2^{np.log2(allowed[0]):.0f}'
    gv = pair_decode(data, s)
    assert gv.shape == ref.shape, (name, gv.shape, ref.shape)
    assert abs(got['rec'] - float(np.abs(gv).max())) <= got['rec'] * 2.0 ** -20 + store, \
        f'{name}: recorded maximum {got["rec"]} against max|out| {np.abs(gv).max()}'
    return check_values(name, gv, ref, tol * rng + extra)


def check_values(name, gv, ref, bound):
    err = float(np.abs(gv - ref).max())
    assert err <= bound, f'{name}: |out - ref| = {err:.3e} is {err / bound:.2f} x the bound {bound:.3e}'
    return err / bound


def check_f32_output(name, got, ref):
    gv = np.asarray(got['data'], np.float64)
    assert np.isfinite(gv).all(), f'{name}: not finite'
    assert abs(got['rec'] - float(np.abs(gv).max())) <= got['rec'] * 2.0 ** -20, f'{name}: recorded maximum'
    return check_values(name, gv, ref, VALUE_TOL * float(np.abs(ref).max()))


def block_of(H, W, n=6):
    """an n x n block off the border and across an 8 x 16 tile edge where the map has one"""
    y0 = min(5, H - n - 1)
    x0 = min(13, W - n - 1)
    return slice(y0, y0 + n), slice(x0, x0 + n)


def covered_outputs(sl, k, stride, pad, n_out):
    """output indices whose whole window lies inside the input slice"""
    o = [i for i in range(n_out) if i * stride - pad >= sl.start and i * stride - pad + k - 1 < sl.stop]
    assert o, 'the block holds no whole window'
    return slice(o[0], o[-1] + 1)


#            B, (H, W), Cin, Cout, k, stride, residual, outputs,            post_scale
TIGHT_CONV = [(1, (9, 13), 64, 64, 1, 1, '', ('pair',), 1.0),
              (2, (17, 23), 64, 64, 3, 1, '', ('f32', 'pair'), 1.0),
              (1, (30, 44), 128, 128, 3, 2, '', ('pair',), 0.5),
              (1, (12, 40), 2048, 512, 1, 1, '', ('pair',), 1.0),                   # few rows, long K: split-K and its reduction kernel
              (2, (24, 40), 64, 256, 1, 1, 'pair', ('pair',), 1.0),
              (2, (24, 40), 512, 64, 1, 1, 'up_f32', ('pair',), 1.0),
              (2, (24, 40), 512, 64, 1, 1, 'up_pair', ('pair',), 1.0),
              (1, (9, 13), 64, 64, 1, 1, 'mixed', ('pair',), 1.0)]                  # filters, scales, shifts and input of both signs


# res_after_act (out = relu(v) + res: the same bound, and the construction still reaches it -- every term is non-negative): a 1x1 and a 3x3
# layer of the table above with a pair residual, and the split-K layer, whose reduction kernel has its own epilogue call
AFTER_ACT_CONV = [(2, (24, 40), 64, 256, 1, 1, 'pair', ('pair',), 1.0),
                  (2, (17, 23), 64, 64, 3, 1, 'pair', ('f32', 'pair'), 1.0),
                  (1, (12, 40), 2048, 512, 1, 1, 'pair', ('pair',), 0.5)]


def build_tight_conv(be, case, side, res_after_act=False):
    """The tensors of a tight conv case.  Everything is decided here, from the packed filters' decode and in fp64."""
    B, (H, W), ci, co, k, stride, kind, outs, post = case
    pad = k // 2
    r = np.random.RandomState(ci + 3 * co + k + (7 if side == 'above' else 0))
    row = None
    if kind == 'mixed':
        w, scale, shift, row = mixed_filters(r, co, k * k, ci, 1.5, 0.25)
    else:
        w, scale, shift = tight_filters(r, co, k * k, ci, 1.5, 0.25)
    packed, sp, wb, sb = pack_filters(be, w, scale, shift)
    wdec = filters_decode(packed)
    Ho, Wo = out_hw(H, W, k, stride, pad)
    by, bx = block_of(H, W)
    oy, ox = covered_outputs(by, k, stride, pad, Ho), covered_outputs(bx, k, stride, pad, Wo)
    res, rmax, res_mode = None, 0.0, 0
    if kind in ('pair', 'up_f32', 'up_pair'):
        up = kind.startswith('up')
        res_mode = 2 if up else 1
        rh, rw = (Ho // 2, Wo // 2) if up else (Ho, Wo)
        rv = r.uniform(0, 2.0, (B, rh, rw, co)).astype(np.float32)
        ry, rx = (slice(oy.start // 2, (oy.stop - 1) // 2 + 1), slice(ox.start // 2, (ox.stop - 1) // 2 + 1)) if up else (oy, ox)
        rv[:, ry, rx] = 2.0
        res = make_pair(rv) if kind.endswith('pair') else (rv, 2.0)
        rmax = res.amax if isinstance(res, PairT) else 2.0
    a, T = solve_amax(lambda t: conv_bound(t, wb, sb, rmax, post), 3.0, side)
    a = float(np.float32(a))
    sgn = np.ones(ci) if row is None else np.sign(wdec[row, 0]) * np.sign(float(scale[row]))
    xv = r.uniform(-a if row is not None else 0.0, a, (B, H, W, ci)).astype(np.float32)
    xv[:, by, bx] = (a * sgn).astype(np.float32)
    x = make_pair(xv)
    b64, b32 = conv_bound(x.amax, wb, sb, rmax, post), conv_bound(x.amax, wb, sb, rmax, post, np.float32)
    assert side_ok(b64, T, side), f'bound * 1.001 = {b64!r} is not 2^-12 {side} {T}'
    rval = None if res is None else (res.value if isinstance(res, PairT) else res[0])
    ref = conv2d(x.value, wdec, sp, shift, k, stride, pad, True, rval, res_mode, post, res_after_act)
    L = b64 / MARGIN / float(np.abs(ref).max())
    assert L <= TIGHT_L, f'the construction reaches the bound only to L = {L}'
    return dict(x=x, packed=packed, sp=sp, shift=shift, k=k, stride=stride, pad=pad, wb=wb, sb=sb, res=res, res_mode=res_mode, post=post,
                ref=ref, allowed=allowed_scales(b64, b32), L=L, outs=outs)


def run_tight_conv(be, case, side, res_after_act=False):
    """Returns (worst error / bound, L)."""
    c = build_tight_conv(be, case, side, res_after_act)
    name = f'{be.name} tight conv {case} {side}' + (' res_after_act' if res_after_act else '')
    worst = 0.0
    for o in c['outs']:
        got = run_conv(be, c['x'], c['packed'], c['sp'], c['shift'], c['k'], c['stride'], c['pad'], c['wb'], c['sb'], True, c['res'], c['res_mode'],
                       o == 'pair', c['post'], res_after_act)
        worst = max(worst, check_pair_output(name, got, c['ref'], c['allowed']) if o == 'pair' else check_f32_output(name, got, c['ref']))
    return worst, c['L']


def run_signed_after_act_conv(be, k, post=-1.25):
    """The tight cases are non-negative, so their ReLU is the identity and the side the residual is added on cannot show.  Here the input,
    the filters and the pair residual have both signs: out = (relu(v) + res) * post against the plain 2e-5 of the range, with the scale
    the rule gives the bound (max|in| wbound + sbound + max|res|) |post|.  Condition, by the reference alone: the other residual order
    and the multiplier before the ReLU each lie more than 100 x that tolerance away on at least 25 % of the elements."""
    B, H, W, ci, co = 2, 17, 23, 64, 64
    r = np.random.RandomState(100 + k)
    w, scale, shift = random_filters(r, co, k * k, ci)
    x, res = make_pair((r.randn(B, H, W, ci) * 1.5).astype(np.float32)), make_pair(r.randn(B, H, W, co).astype(np.float32))
    packed, sp, wb, sb = pack_filters(be, w, scale, shift)
    wdec = filters_decode(packed)
    ref = conv2d(x.value, wdec, sp, shift, k, 1, k // 2, True, res.value, 1, post, True)
    far = 100 * VALUE_TOL * float(np.abs(ref).max())
    swapped = conv2d(x.value, wdec, sp, shift, k, 1, k // 2, True, res.value, 1, post, False)
    early = conv2d(x.value, wdec, np.asarray(sp, np.float64) * post, np.asarray(shift, np.float64) * post, k, 1, k // 2, True, res.value, 1, 1.0, True)
    for what, other in (('the other residual order', swapped), ('scaling before the ReLU', early)):
        frac = float((np.abs(other - ref) > far).mean())
        assert frac >= 0.25, f'{what} is told apart on {frac:.3f} of the elements only'
    b64, b32 = conv_bound(x.amax, wb, sb, res.amax, post), conv_bound(x.amax, wb, sb, res.amax, post, np.float32)
    got = run_conv(be, x, packed, sp, shift, k, 1, k // 2, wb, sb, True, res, 1, True, post, True)
    return check_pair_output(f'{be.name} conv {k}x{k} res_after_act post_scale {post} on signed data', got, ref, allowed_scales(b64, b32))


# loose side: B, (H, W), Cin, Cout, k
LOOSE_CONV = [(1, (9, 13), 64, 64, 1), (2, (17, 23), 64, 64, 3)]
LOOSE_TARGETS = [('shift', 2.0 ** 10), ('shift', 2.0 ** 18), ('shift', 2.0 ** 24), ('filters', 2.0 ** 10)]


def run_loose_conv(be, case, how, target):
    """A dead output channel makes the bound loose by `target`: zero filters and a shift of -target x the response ('shift': sbound), or
    huge filters under a still larger negative shift ('filters': wbound).  |out - ref| <= 2e-5 range + delta(out).  Returns (ratio, L)."""
    B, (H, W), ci, co, k = case
    pad, dead = k // 2, 9
    r = np.random.RandomState(ci + co + k + int(np.log2(target)))
    w, scale, shift = random_filters(r, co, k * k, ci)
    x = make_pair(r.uniform(0, 3.0, (B, H, W, ci)).astype(np.float32))
    w[dead] = 0.0
    packed, sp, wb, sb = pack_filters(be, w, scale, shift)
    M = float(np.abs(conv2d(x.value, filters_decode(packed), sp, shift, k, 1, pad)).max())         # the live channels' maximum, by the reference
    if how == 'shift':
        shift[dead] = -(target * M - x.amax * wb)
    else:
        g = target * M / (3 * x.amax)                                   # the dead row's scale * L1: bound = a g + 2 a g
        w[dead], scale[dead], shift[dead] = g / (k * k * ci), 1.0, -2 * x.amax * g
    packed, sp, wb, sb = pack_filters(be, w, scale, shift)
    ref = conv2d(x.value, filters_decode(packed), sp, shift, k, 1, pad)
    assert not ref[..., dead].any() and float(np.abs(ref).max()) == M
    b64, b32 = conv_bound(x.amax, wb, sb), conv_bound(x.amax, wb, sb, f=np.float32)
    L = b64 / MARGIN / M
    assert target / 2 <= L <= target * 2, f'L = {L} is not within a factor 2 of {target}'
    got = run_conv(be, x, packed, sp, shift, k, 1, pad, wb, sb)
    return check_pair_output(f'{be.name} loose conv {case} {how} L = 2^{np.log2(L):.1f}', got, ref, allowed_scales(b64, b32), storage_delta(ref, L), storage_delta(ref, L)), L


def run_loose_input_conv(be, k, below):
    """The input pair tensor is written with a scale 2^below under the ideal one (subnormal lo halves everywhere, for 2^26 subnormal hi
    halves too); its slots hold the true maximum.  The reference takes the decoded values: plain 2e-5 of the range."""
    B, H, W, ci, co = 2, 17, 23, 64, 64
    r = np.random.RandomState(k + below)
    w, scale, shift = random_filters(r, co, k * k, ci)
    x = make_pair((r.randn(B, H, W, ci) * 1.5).astype(np.float32), below)
    assert x.amax * x.scale < 2.0 ** (15 - below)
    packed, sp, wb, sb = pack_filters(be, w, scale, shift)
    ref = conv2d(x.value, filters_decode(packed), sp, shift, k, 1, k // 2)
    b64, b32 = conv_bound(x.amax, wb, sb), conv_bound(x.amax, wb, sb, f=np.float32)
    got = run_conv(be, x, packed, sp, shift, k, 1, k // 2, wb, sb)
    return check_pair_output(f'{be.name} conv {k}x{k} on an input scaled 2^{below} below', got, ref, allowed_scales(b64, b32))


# ------------------------------------------------------------------------------------------------------------------ the bottlenecks
def run_bottleneck(be, x, lay, wbs, sbs, proj=None):
    """ivx_bottleneck_fwd_pio, or ivx_bottleneck_proj_fwd_pio with proj = (bank, scale, shift, wboundd).  lay: [(packed, scale_p, shift)] of
    conv1, conv2 (and conv3); wbs / sbs: the three bound terms.  Returns dict(data, scale, rec)."""
    L = be.L
    B, H, W, cin = x.value.shape
    P = lay[0][0].shape[0]
    d = be.BottleneckDesc(B, H, W, P)
    io = be.BottleneckIO()
    xin, sl_in, sl_out = be.up(x.data), be.up(make_slots(x.amax, x.scale)), be.up(make_slots())
    io.in_scale, io.amax_in = be.addr(sl_in, 4 * SLOTS), be.addr(sl_in)
    io.out_scale, io.amax_out = be.addr(sl_out, 4 * SLOTS), be.addr(sl_out)
    for i in range(3):
        io.wbound[i], io.sbound[i] = wbs[i], sbs[i]
    out = be.full((B, H, W, 8 * P), np.float16, np.nan)
    dev = [be.up(np.asarray(t)) for l in (list(lay[:2]) + [proj[:3] if proj is not None else lay[2]]) for t in l]
    ptrs = [_p(be, t) for t in dev]
    if proj is None:
        be.ok(L.ivx_bottleneck_fwd_pio(C.byref(d), C.byref(io), _p(be, xin), *ptrs, _p(be, out), be.stream), 'ivx_bottleneck_fwd_pio')
    else:
        be.ok(L.ivx_bottleneck_proj_fwd_pio(C.byref(d), cin, C.byref(io), proj[3], _p(be, xin), *ptrs, _p(be, out), be.stream),
              'ivx_bottleneck_proj_fwd_pio')
    so = be.get(sl_out)
    return dict(data=be.get(out), scale=slots_scale(so), rec=slots_amax(so))


def build_bottleneck(be, r, P, cin, proj, kind, dead_shift=None):
    """The packed layers of a block.  kind 'tight': non-negative filters with equal row sums; 'random': He-initialised.  dead_shift: channel 9
    of conv1 gets zero filters and this shift.  Returns dict(lay, proj, wbs, sbs, wbd, ref_layers, ref_proj)."""
    mk = (lambda co, t, ci, g: tight_filters(r, co, t, ci, g, 0.125)) if kind == 'tight' else (lambda co, t, ci, g: random_filters(r, co, t, ci))
    raw = [mk(P, 1, cin, 1.0), mk(P, 9, P, 1.25), mk(4 * P, 1, P, 0.75)]
    if dead_shift is not None:
        raw[0][0][9], raw[0][2][9] = 0.0, dead_shift
    lay, wbs, sbs, ref_layers = [], [], [], []
    for w, sc, sh in raw[:2] if proj else raw:
        packed, sp, wb, sb = pack_filters(be, w, sc, sh)
        lay.append((packed, sp, sh))
        ref_layers.append((filters_decode(packed), sp, sh))
        wbs.append(wb)
        sbs.append(sb)
    pj = ref_proj = wbd = raw_proj = None
    if proj:
        w3, s3, t3 = raw[2]
        wd, sd, td = mk(4 * P, 1, cin, 0.5)
        bank, sc, sf, wb3, sb, wbd = pack_proj(be, w3[:, 0], s3, t3, wd[:, 0], sd, td)
        pj, ref_proj, raw_proj = (bank, sc, sf, wbd), (filters_decode(bank), sc, sf), ((w3, s3, t3), (wd, sd, td))
        wbs.append(wb3)
        sbs.append(sb)
    return dict(lay=lay, proj=pj, wbs=wbs, sbs=sbs, wbd=wbd, ref_layers=ref_layers, ref_proj=ref_proj, raw_proj=raw_proj)


TIGHT_BOTTLENECK = [(False, 64, 1, 8, 16), (False, 64, 2, 13, 37), (False, 128, 1, 8, 16), (True, 64, 1, 8, 16), (True, 64, 2, 13, 37)]      # proj, P, B, H, W


def run_tight_bottleneck(be, case, side):
    """All three bounds (b1, b2, b3 with its shortcut term) are attained at once at the interior of the block.  Returns (ratio, (L1, L2, L3))."""
    proj, P, B, H, W = case
    cin = P if proj else 4 * P
    r = np.random.RandomState(P + B + H + (1 if proj else 0) + (7 if side == 'above' else 0))
    m = build_bottleneck(be, r, P, cin, proj, 'tight')
    a, T = solve_amax(lambda t: bottleneck_bounds(t, m['wbs'], m['sbs'], m['wbd'])[2], 3.0, side)
    a = float(np.float32(a))
    by, bx = block_of(H, W)
    xv = r.uniform(0, a, (B, H, W, cin)).astype(np.float32)
    xv[:, by, bx] = a
    x = make_pair(xv)
    b = bottleneck_bounds(x.amax, m['wbs'], m['sbs'], m['wbd'])
    b32 = bottleneck_bounds(x.amax, m['wbs'], m['sbs'], m['wbd'], np.float32)
    assert side_ok(b[2], T, side), f'b3 = {b[2]!r} is not 2^-12 {side} {T}'
    refs = bottleneck(x.value, m['ref_layers'], m['ref_proj'])
    Ls = tuple(float(bi) / MARGIN / float(np.abs(t).max()) for bi, t in zip(b, refs))
    assert max(Ls) <= TIGHT_L, f'the construction reaches the bounds only to L = {Ls}'
    got = run_bottleneck(be, x, m['lay'], m['wbs'], m['sbs'], m['proj'])
    return check_pair_output(f'{be.name} tight bottleneck {case} {side}', got, refs[2], allowed_scales(b[2], b32[2])), Ls


def run_chain(be, x, m):
    """The same block layer by layer: ivx_conv_fwd_pio per convolution, every scale from the MEASURED maximum of the layer's input (the
    slots its producer filled).  Projection form: four launches, the shortcut conv's fp32 output is the residual of conv3; conv3 and the
    shortcut conv are packed on their own here (BN scales in the epilogue), 2^-24-level apart from the joint bank the reference decodes."""
    def as_pair(g):
        return PairT(g['data'], g['scale'], g['rec'])
    (p1, s1, t1), (p2, s2, t2) = m['lay'][:2]
    m1 = as_pair(run_conv(be, x, p1, s1, t1, 1, 1, 0, m['wbs'][0], m['sbs'][0]))
    m2 = as_pair(run_conv(be, m1, p2, s2, t2, 3, 1, 1, m['wbs'][1], m['sbs'][1]))
    if m['proj'] is None:
        p3, s3, t3 = m['lay'][2]
        return run_conv(be, m2, p3, s3, t3, 1, 1, 0, m['wbs'][2], m['sbs'][2], res=x, res_mode=1)
    (w3, s3, t3), (wd, sd, td) = m['raw_proj']
    pd, spd, wbd, sbd = pack_filters(be, wd, sd, td)
    short = run_conv(be, x, pd, spd, td, 1, 1, 0, wbd, sbd, relu=False, out_pair=False)
    p3, sp3, wb3, sb3 = pack_filters(be, w3, s3, t3)
    return run_conv(be, m2, p3, sp3, t3, 1, 1, 0, wb3, sb3, res=(short['data'], short['rec']), res_mode=1)


LOOSE_BOTTLENECK = [(False, 64, 2, 13, 37), (True, 64, 2, 13, 37)]


def run_loose_bottleneck(be, case, target):
    """The dead channel sits in conv1 (L1 near `target`); the looseness carries through b2 and b3.  Bound, every term from the reference's
    fp64 tensors:  2e-5 range + wbound3 (wbound2 delta(mid1) + delta(mid2)) + delta(out).  The layer-wise chain on the same data, which
    measures its maxima, must meet the plain 2e-5.  Returns (ratio, chain ratio, (L1, L2, L3))."""
    proj, P, B, H, W = case
    cin = P if proj else 4 * P
    seed = P + H + (1 if proj else 0) + int(np.log2(target))
    xv = np.random.RandomState(seed).uniform(0, 3.0, (B, H, W, cin)).astype(np.float32)
    x = make_pair(xv)
    m0 = build_bottleneck(be, np.random.RandomState(seed + 1), P, cin, proj, 'random')
    M1 = float(np.abs(bottleneck(x.value, m0['ref_layers'], m0['ref_proj'])[0]).max())
    dead = -(target * M1 - x.amax * m0['wbs'][0])
    m = build_bottleneck(be, np.random.RandomState(seed + 1), P, cin, proj, 'random', dead_shift=dead)
    refs = bottleneck(x.value, m['ref_layers'], m['ref_proj'])
    assert not refs[0][..., 9].any()
    b = bottleneck_bounds(x.amax, m['wbs'], m['sbs'], m['wbd'])
    b32 = bottleneck_bounds(x.amax, m['wbs'], m['sbs'], m['wbd'], np.float32)
    Ls = tuple(float(bi) / MARGIN / float(np.abs(t).max()) for bi, t in zip(b, refs))
    assert target / 2 <= Ls[0] <= target * 2, f'L1 = {Ls[0]} is not within a factor 2 of {target}'
    extra = m['wbs'][2] * (m['wbs'][1] * storage_delta(refs[0], Ls[0]) + storage_delta(refs[1], Ls[1])) + storage_delta(refs[2], Ls[2])
    name = f'{be.name} loose bottleneck {case} L1 = 2^{np.log2(Ls[0]):.1f}'
    got = run_bottleneck(be, x, m['lay'], m['wbs'], m['sbs'], m['proj'])
    ratio = check_pair_output(name, got, refs[2], allowed_scales(b[2], b32[2]), extra, storage_delta(refs[2], Ls[2]))
    chain = run_chain(be, x, m)
    return ratio, check_pair_output(name + ' (layer-wise chain)', chain, refs[2]), Ls


def run_loose_input_bottleneck(be, proj, below):
    P, B, H, W = 64, 2, 13, 37
    cin = P if proj else 4 * P
    r = np.random.RandomState(below + (1 if proj else 0))
    x = make_pair(np.maximum(r.randn(B, H, W, cin) * 1.5, 0).astype(np.float32), below)
    m = build_bottleneck(be, r, P, cin, proj, 'random')
    refs = bottleneck(x.value, m['ref_layers'], m['ref_proj'])
    b = bottleneck_bounds(x.amax, m['wbs'], m['sbs'], m['wbd'])
    b32 = bottleneck_bounds(x.amax, m['wbs'], m['sbs'], m['wbd'], np.float32)
    got = run_bottleneck(be, x, m['lay'], m['wbs'], m['sbs'], m['proj'])
    return check_pair_output(f'{be.name} bottleneck proj={proj} on an input scaled 2^{below} below', got, refs[2], allowed_scales(b[2], b32[2]))


# ------------------------------------------------------------------------------------------------------------------ the stem
def run_stem_heads(be, img, w, scale, shift, frag, sp, wb, sb):
    """Both heads of the chain on one image: ivx_amax_f32 + ivx_stem_pool_fwd_pair, and ivx_nchw_to_nhwc_amax + the fp32 stem (ivx_conv_fwd) +
    ivx_maxpool2d_fwd_pair.  w: the fp32 filters the fragments stand for.  Returns two dict(data, scale, rec)."""
    L = be.L
    B, _, H, W = img.shape
    Hc, Wc = out_hw(H, W, 7, 2, 3)
    Hp, Wp = out_hw(Hc, Wc, 3, 2, 1)
    im = be.up(np.asarray(img, np.float32))
    fr, spd, shd = be.up(frag), be.up(np.asarray(sp, np.float32)), be.up(np.asarray(shift, np.float32))
    sl_img, sl_out = be.up(make_slots()), be.up(make_slots())
    be.ok(L.ivx_amax_f32(_p(be, im), img.size, _p(be, sl_img), be.stream), 'ivx_amax_f32')
    out = be.full((B, Hp, Wp, 128), np.float16, np.nan)
    be.ok(L.ivx_stem_pool_fwd_pair(_p(be, im), B, H, W, _p(be, fr), _p(be, spd), _p(be, shd), wb, sb, _p(be, sl_img), _p(be, out), _p(be, sl_out, 4 * SLOTS),
                                   _p(be, sl_out), be.stream), 'ivx_stem_pool_fwd_pair')
    so = be.get(sl_out)
    one = dict(data=be.get(out), scale=slots_scale(so), rec=slots_amax(so))
    assert slots_amax(be.get(sl_img)) == float(np.abs(img).max())
    # three launches
    sl_img2, sl_out2 = be.up(make_slots()), be.up(make_slots())
    x4 = be.full((B, H, W, 4), np.float32, np.nan)
    be.ok(L.ivx_nchw_to_nhwc_amax(_p(be, im), B, 3, H * W, 4, _p(be, x4), _p(be, sl_img2), be.stream), 'ivx_nchw_to_nhwc_amax')
    d = be.ConvDesc()
    d.B, d.D, d.H, d.W, d.Cin, d.Cout, d.KD, d.KH, d.KW = B, 1, H, W, 4, 64, 1, 7, 7
    d.sd, d.sh, d.sw, d.pd, d.ph, d.pw, d.relu, d.post_scale, d.res_scale = 1, 2, 2, 0, 3, 3, 1, 1.0, 1.0
    wt, scd = be.up(stem_taps(w).reshape(64, 7, 7, 4)), be.up(np.asarray(scale, np.float32))
    y = be.full((B, Hc, Wc, 64), np.float32, np.nan)
    be.ok(L.ivx_conv_fwd(C.byref(d), _p(be, x4), _p(be, wt), _p(be, scd), _p(be, shd), None, _p(be, y), be.stream), 'ivx_conv_fwd')
    out2 = be.full((B, Hp, Wp, 128), np.float16, np.nan)
    be.ok(L.ivx_maxpool2d_fwd_pair(_p(be, y), B, Hc, Wc, 64, 3, 2, 1, _p(be, out2), _p(be, sl_img2), wb, sb, _p(be, sl_out2, 4 * SLOTS), _p(be, sl_out2),
                                   be.stream), 'ivx_maxpool2d_fwd_pair')
    so2 = be.get(sl_out2)
    return one, dict(data=be.get(out2), scale=slots_scale(so2), rec=slots_amax(so2))


def stem_filters(be, r, dead_shift=None):
    """Random stem filters, made their own pair decode (so both heads see the same values), with positive scales; the row of largest
    scale * L1 carries the largest shift.  Returns (w fp32 [64,3,7,7], scale, shift, row, frag, sp, wbound, sbound)."""
    w = (r.randn(64, 3, 7, 7) * (2.0 / 147) ** 0.5).astype(np.float32)
    scale = (r.rand(64) + 0.5).astype(np.float32)
    shift = (r.uniform(-0.1, 0.1, 64)).astype(np.float32)
    frag, sp, _, _ = pack_stem(be, w, scale, shift)
    w = (stem_decode(frag) / filter_scale(scale, sp)).astype(np.float32)
    if dead_shift is not None:
        w[9], shift[9] = 0.0, dead_shift
    row = int(np.argmax(scale.astype(np.float64) * np.abs(w.astype(np.float64)).sum((1, 2, 3))))
    if dead_shift is None:
        shift[row] = 0.125
    frag, sp, wb, sb = pack_stem(be, w, scale, shift)
    assert np.array_equal(stem_decode(frag) / filter_scale(scale, sp), w.astype(np.float64)), 'the decoded filters are not a fixed point of the packer'
    return w, scale, shift, row, frag, sp, wb, sb


TIGHT_STEM = [(1, 32, 64), (2, 37, 53)]


def run_tight_stem(be, case, side):
    """The image is +-a, sign-aligned with the filter of largest scale * L1 over one interior 7 x 7 window, and uniform in [-a, a] on the pair
    grid elsewhere.  Both heads must give the stated scale and the values.  Returns (worst ratio, L)."""
    B, H, W = case
    r = np.random.RandomState(H + W + (7 if side == 'above' else 0))
    w, scale, shift, row, frag, sp, wb, sb = stem_filters(be, r)
    a, T = solve_amax(lambda t: conv_bound(t, wb, sb), 2.5, side)
    a = float(np.float32(a))
    a = float(pair_round(np.float32(a), pow2_scale(a)))
    img = pair_round(r.uniform(-a, a, (B, 3, H, W)).astype(np.float32), pow2_scale(a)).astype(np.float32)
    oy, ox = 5, 9                                                          # conv output pixel: window rows 2 oy - 3 .. 2 oy + 3
    img[:, :, 2 * oy - 3:2 * oy + 4, 2 * ox - 3:2 * ox + 4] = (a * np.sign(w[row]) + (w[row] == 0) * a).astype(np.float32)
    assert float(np.abs(img).max()) == a
    b64, b32 = conv_bound(a, wb, sb), conv_bound(a, wb, sb, f=np.float32)
    assert side_ok(b64, T, side), f'bound * 1.001 = {b64!r} is not 2^-12 {side} {T}'
    ref = stem_pool(img, w, scale, shift)
    L = b64 / MARGIN / float(np.abs(ref).max())
    assert L <= TIGHT_L, f'the construction reaches the bound only to L = {L}'
    one, three = run_stem_heads(be, img, w, scale, shift, frag, sp, wb, sb)
    al = allowed_scales(b64, b32)
    assert one['scale'] == three['scale'], 'the two heads chose different scales'
    return max(check_pair_output(f'{be.name} tight stem {case} {side} (one launch)', one, ref, al),
               check_pair_output(f'{be.name} tight stem {case} {side} (three launches)', three, ref, al)), L


def run_loose_stem(be, target):
    """a dead stem channel (zero filters, shift -target x the response): |out - ref| <= 2e-5 range + delta(out), both heads"""
    B, H, W = 2, 37, 53
    r = np.random.RandomState(int(np.log2(target)))
    a = 2.5
    img = pair_round(r.uniform(-a, a, (B, 3, H, W)).astype(np.float32), pow2_scale(a)).astype(np.float32)
    amax = float(np.abs(img).max())
    w, scale, shift, _, frag, sp, wb, sb = stem_filters(be, np.random.RandomState(5), dead_shift=0.0)
    M = float(np.abs(stem_pool(img, w, scale, shift)).max())
    w, scale, shift, _, frag, sp, wb, sb = stem_filters(be, np.random.RandomState(5), dead_shift=-(target * M - amax * wb))
    ref = stem_pool(img, w, scale, shift)
    assert not ref[..., 9].any() and float(np.abs(ref).max()) == M
    b64, b32 = conv_bound(amax, wb, sb), conv_bound(amax, wb, sb, f=np.float32)
    L = b64 / MARGIN / M
    assert target / 2 <= L <= target * 2, f'L = {L} is not within a factor 2 of {target}'
    one, three = run_stem_heads(be, img, w, scale, shift, frag, sp, wb, sb)
    al, extra = allowed_scales(b64, b32), storage_delta(ref, L)
    assert one['scale'] == three['scale'], 'the two heads chose different scales'
    return max(check_pair_output(f'{be.name} loose stem L = 2^{np.log2(L):.1f} (one launch)', one, ref, al, extra, extra),
               check_pair_output(f'{be.name} loose stem L = 2^{np.log2(L):.1f} (three launches)', three, ref, al, extra, extra)), L


# ------------------------------------------------------------------------------------------------------------------ DCNv2 columns
def run_loose_input_dcn(be, below):
    """ivx_dcn_im2col_fwd_pair on a map scaled 2^below under the ideal scale: the columns keep the map's scale; bound of
    tests/test_gpu_ops_fp64.py: 17 * 2^-24 A + 2^-126 + 2^-21 |ref| + 2^-24 / scale.  Returns the worst error / bound."""
    import ref_ops as R
    B, H, W, Cn, k, s, p, d, omc = 2, 11, 13, 64, 3, 1, 1, 1, 27
    r = np.random.RandomState(below)
    x = make_pair((r.randn(B, H, W, Cn) * 1.7).astype(np.float32), below)
    om = R.dcn_offsets_masks(below + 1, B, H, W, k, s, p, d, omc)
    Ho, Wo = R.dcn_out_hw(H, W, k, s, p, d)
    xin, sl_in, sl_out, omd = be.up(x.data), be.up(make_slots(x.amax, x.scale)), be.up(make_slots()), be.up(np.asarray(om, np.float32))
    col = be.full((B, Ho, Wo, 2 * k * k * Cn), np.float16, np.nan)
    be.ok(be.L.ivx_dcn_im2col_fwd_pair(_p(be, xin), _p(be, sl_in, 4 * SLOTS), _p(be, omd), B, H, W, Cn, k, k, s, p, d, omc, _p(be, col),
                                       _p(be, sl_out, 4 * SLOTS), _p(be, sl_out), be.stream), 'ivx_dcn_im2col_fwd_pair')
    so = be.get(sl_out)
    assert slots_scale(so) == x.scale, 'the columns keep the scale of the map'
    gv = pair_decode(be.get(col), x.scale).reshape(B * Ho * Wo, k * k, Cn)
    ref, A = R.dcn_columns(x.value.astype(np.float32), om, k, s, p, d)
    assert float(np.abs(ref).max()) > 0.25 * x.amax
    extra = 2.0 ** -21 * np.abs(ref) + 2.0 ** -24 / x.scale
    R.check_dcn(f'{be.name} dcn columns of a map scaled 2^{below} below', gv, ref, A, extra)
    return float((np.abs(gv - ref) / (R.dcn_bound(A) + extra)).max())


# ------------------------------------------------------------------------------------------------------------------ one model-level case
MODEL_TOL = 2e-4                 # the project's own bar between operand modes, of the tensor's range
MODEL_CASES = ['kitti_small', 'scannet_fast']


def model_case(name):
    """(module, family, image [B, V, 3, H, W], metas): plan_worker.family_model('kitti', (24, 28, 12), small_channels=True) or the scannet_fast
    run configuration, with 5 % of the channels of every BatchNorm of the 2-D trunk dead (gamma = 0, beta = -50 max|beta|: ReLU stores 0 and
    sbound is large) and a saturated 16 x 16 block of +-max|image| in every view."""
    import torch
    import plan_worker as W
    from imvoxelnet_amd.params import BNParams
    if name == 'kitti_small':
        fam, B, V, hw = 'kitti', 2, 1, (128, 224)
        model = W.family_model('kitti', (24, 28, 12), small_channels=True)
    else:
        fam, nv, small, B, V, hw = W.run_config(name)[:6]
        model = W.family_model(fam, n_voxels=nv, seed=3, small_channels=small)
    r = np.random.RandomState(0)
    n_bn = 0
    with torch.no_grad():
        for m in model.backbone.modules():
            if isinstance(m, BNParams):
                c = m.weight.numel()
                idx = torch.from_numpy(r.choice(c, max(1, int(round(0.05 * c))), replace=False))
                bmax = float(m.bias.abs().max())
                m.weight[idx] = 0.0
                m.bias[idx] = -50.0 * bmax
                n_bn += 1
    assert n_bn >= 50, n_bn
    img = torch.randn(B, V, 3, *hw, generator=torch.Generator().manual_seed(11))
    sign = torch.from_numpy(r.choice([-1.0, 1.0], (3, 16, 16)).astype(np.float32))
    img[:, :, :, 40:56, 60:76] = float(img.abs().max()) * sign
    return model, fam, img.contiguous(), W.metas_for(fam, B, V, hw)


def run_model_operand_modes(L, dev, name):
    """The model handle in the default operand mode (fp16-pair trunk and Winograd operands) and with trunk_operands = wino_operands = 0 (exact
    fp32 products) on model_case(name).  The second handle is the project's own code on other arithmetic, NOT an fp64 reference: this shows
    that the bounds of a whole trunk with dead channels and a saturated image neither overflow nor lose the small activations, nothing
    more.  FPN level 0, the volume and the neck outputs are finite and within MODEL_TOL of the tensor's range of the fp32-operand run; the
    valid mask is identical.  Returns {tensor: error / (MODEL_TOL range)}."""
    import torch
    import plan_worker as W
    model, fam, img, metas = model_case(name)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if dev != 'cpu' else None
    B = img.shape[0]
    outs = {}
    for mode in (PAIR, F32):
        hd = W.Handle(L, model, trunk_operands=mode, wino_operands=mode, stream=stream)
        try:
            cache = {}
            out = W.detect_once(hd, img.to(dev).contiguous(), metas, dev, cache)
        finally:
            hd.close()
        steps = list(cache['plan']['steps'].values())
        lift = [s for s in steps if s['kind'] == 4][0]                      # the unprojection: FPN level 0 -> volume, valid mask
        ids = {'fpn0': lift['in'], 'volume': lift['out'], 'valid': lift['out2']}
        for l, head in enumerate(s['in'] for s in steps if s['kind'] in (5, 10)):      # the anchor tail / every FCOS level reads a head conv's output
            ids[f'neck{l}'] = [s for s in steps if s['kind'] == 2 and s['out'] == head][0]['in']
        outs[mode] = {k: out[f'tensor{t}'] for k, t in ids.items()}
    assert outs[PAIR]['valid'].size == B * int(np.prod(model.n_voxels)), 'the valid mask is one byte per voxel'
    assert np.array_equal(outs[PAIR]['valid'], outs[F32]['valid']) and outs[PAIR]['valid'].any(), f'{name}: the valid masks differ'
    ratios = {}
    for k in outs[PAIR]:
        if k == 'valid':
            continue
        a, b = outs[PAIR][k].view(np.float32).astype(np.float64), outs[F32][k].view(np.float32).astype(np.float64)
        assert a.shape == b.shape and np.isfinite(a).all() and np.isfinite(b).all(), f'{name} {k}: not finite'
        rng = float(np.abs(b).max())
        assert rng > 0, f'{name} {k}: an all-zero tensor checks nothing'
        err = float(np.abs(a - b).max())
        assert err <= MODEL_TOL * rng, f'{name} {k}: default operands against fp32 operands {err:.3e} = {err / rng:.2e} of the range'
        ratios[k] = err / (MODEL_TOL * rng)
    assert 'neck0' in ratios
    return ratios
