"""The e4m3 forms of the direct convolution (include/imvoxel.h, ivx_conv_desc.res_scale: IVX_FP8 tensors are OCP e4m3 bytes with a scale
kept by the caller, who folds s_in * s_wgt[co] / s_out into scale[], 1 / s_out into shift[] and passes res_scale = s_res / s_out; the
store saturates at +-448 and rounds to nearest even) against plain fp64: the codec, the operation, the cases, the comparison rule and
the driver -- shared by tests/test_host_fp8_conv.py (no device: the codec against torch.float8_e4m3fn, the conditions on the cases) and
tests/test_gpu_fp8_conv.py (the HIP library through ops.conv_fwd and FusedConv).

No kernel of the project is in here and no reference comes out of the library.  The codec is written from the format's definition, the
sum and the clause order are ref_conv.accumulate / ref_conv.finish, the operands are the exact decodes of the bytes (or the bf16-rounded
values) the kernel reads.

The forms of the trunk:  a  bf16 in, e4m3 out (conv1; conv2 under variant='conv3');  b  e4m3 in, e4m3 out;  c  e4m3 in, bf16 out + bf16
shortcut (conv3 of the default variant);  d  e4m3 in, e4m3 out + e4m3 shortcut (residual='fp8');  f  e4m3 in, fp32 out (accepted by
ivx_conv_fwd; no layer of the trunk).

The comparison rule of an e4m3 output.  The kernel sums exact products in its own order and with the fp8 MFMA's internal precision, so
its v = acc*scale + shift may lie delta_v away from the fp64 one, with delta = 1e-4 max |pre-rounding reference| of the run (the
accumulation bar of test_conv_fp8_storage; tools/fp8_mfma_precision.py measured 3.7e-5) and delta_v = delta / |post_scale|.  The rest of
the epilogue is monotone in v, so the values the kernel may round lie between the reference at v - delta_v and at v + delta_v -- an
interval inside [u - delta, u + delta] around the reference u -- and the stored byte must be a code whose cell meets that interval:
  * no boundary inside the interval (and beyond +-448: one saturated code): the byte equals encode(reference) exactly;
  * one boundary inside: one of the two codes that meet there; among the subnormals, where a step (2^-9) is smaller than delta,
    every code the interval touches;
  * an output the ReLU set to zero from a v farther than delta_v below zero is exact (the interval is the point 0): such elements are
    not boundary elements although 0 lies within delta of the boundaries +-2^-10;
  * +0 and -0 are two codes with the boundary 0 between them (0 * -1.25 is -0: byte 0x80);
  * NaN: a NaN byte (0x7F / 0xFF); under the ReLU a NaN becomes 0 (v > 0 ? v : 0, the rule of every epilogue of the project).
Nothing is left out.  The share of elements whose interval holds a boundary is capped at 10 % per run (a condition on the inputs)."""
import numpy as np
import torch

import ref_conv as R

FMAX = 448.0
DELTA_REL = 1e-4                      # accumulation bar, a fraction of max |pre-rounding reference|
BOUNDARY_CAP = 0.10
FP8 = torch.float8_e4m3fn


# ------------------------------------------------------------------------------------------------------------------ the codec
def decode(b):
    """OCP e4m3 bytes -> fp64.  sign | 4 exponent bits, bias 7 | 3 mantissa bits; exponent 0: subnormals m * 2^-9; 0x7F / 0xFF: NaN;
    no infinities; the largest finite value is 0x7E = 1.75 * 2^8 = 448"""
    b = np.asarray(b, np.uint8)
    e, m = ((b >> 3) & 15).astype(np.float64), (b & 7).astype(np.float64)
    mag = np.where(e == 0, m * 2.0 ** -9, (8.0 + m) * np.exp2(e - 10.0))
    return np.where((b & 0x7F) == 0x7F, np.nan, np.where(b & 0x80, -mag, mag))


_POS = decode(np.arange(0x7F, dtype=np.uint8))          # the 127 non-negative finite values; the code is the index
_MID = (_POS[:-1] + _POS[1:]) / 2.0                    # exact in fp64


def encode(v):
    """fp64 -> bytes under the header's sentence: clamp to +-448 first (so +-inf saturates), then round to nearest, ties to the even
    mantissa; NaN -> 0x7F with the sign bit of the NaN"""
    v = np.asarray(v, np.float64)
    nan = np.isnan(v)
    a = np.where(nan, 0.0, np.minimum(np.abs(v), FMAX))
    lo, hi = np.searchsorted(_MID, a, 'left'), np.searchsorted(_MID, a, 'right')      # they differ on a midpoint only
    code = np.where(nan, 0x7F, np.where(lo % 2 == 0, lo, hi)).astype(np.uint8)
    return code | (np.signbit(v).astype(np.uint8) << 7)


def boundaries():
    """the sorted midpoints between adjacent finite values of the signed code line -448 .. -0, +0 .. 448: 253 of them, 0 (between the two
    zeros) among them"""
    return np.concatenate([-_MID[::-1], [0.0], _MID])


_BND = boundaries()
_CELL_LO, _CELL_HI = np.concatenate([[-np.inf], _BND]), np.concatenate([_BND, [np.inf]])      # by ordinal + 127


def ordinal(b):
    """position of a byte on the signed code line: -127 (-448) .. -1 (-0), 0 (+0) .. 126 (448); the NaN bytes fall outside (-128, 127)"""
    b = np.asarray(b, np.uint8).astype(np.int64)
    return np.where(b & 0x80, -1 - (b & 0x7F), b & 0x7F)


def steps(b):
    """signed count of code steps from zero (the two zeros are one value): what two encodings are apart by"""
    b = np.asarray(b, np.uint8).astype(np.int64)
    return np.where(b & 0x80, -(b & 0x7F), b & 0x7F)


def nearest_boundary(u):
    u = np.asarray(u, np.float64)
    i = np.clip(np.searchsorted(_BND, u), 1, len(_BND) - 1)
    return np.where(np.abs(_BND[i - 1] - u) <= np.abs(_BND[i] - u), _BND[i - 1], _BND[i])


# ------------------------------------------------------------------------------------------------------------------ the operation
def finish(v, r, relu, after, post, order='header'):
    """ref_conv.finish with the ReLU as the kernels spell it, v > 0 ? v : 0: a NaN that reaches the ReLU becomes 0 (np.maximum would
    keep it).  Stated here because the saturation case carries a NaN through a layer with a ReLU."""
    if relu:
        t = v + r if (r is not None and (after if order == 'swapped' else not after)) else v
        if order == 'scaled_early':
            t = t * post
        v = np.where(np.isnan(t), -np.inf, v)                # what the ReLU zeroes whatever the (finite) residual
    return R.finish(v, r, relu, after, post, order)


class Expect:
    """What one run must store.  u: the fp64 result before the storage rounding, in units of the output's scale; for an e4m3 output
    the interval of the comparison rule as code ordinals [olo, ohi] and the boundary flag"""

    def __init__(self, v, r, relu, after, post, out):
        self.out = out
        self.u = finish(v, r, relu, after, post)
        if out != 'e4m3':
            return
        fin = np.abs(self.u[np.isfinite(self.u)])
        self.delta = DELTA_REL * float(fin.max())
        dv = self.delta / abs(post)
        ua, ub = finish(v - dv, r, relu, after, post), finish(v + dv, r, relu, after, post)
        self.nan = np.isnan(self.u)
        self.want = encode(self.u)
        self.olo, self.ohi = ordinal(encode(np.fmin(ua, ub))), ordinal(encode(np.fmax(ua, ub)))
        self.boundary = (self.olo != self.ohi) & ~self.nan
        self.boundary_share = float(self.boundary.mean())
        self.saturated_share = float((np.abs(self.u) >= 464.0).mean())        # beyond where rounding alone still gives +-448


def check_bytes(name, got, ex):
    """The comparison rule on the stored bytes of one run; prints and returns (worst distance of the reference from the stored code's
    cell / delta, share of boundary elements).  A failure names the run, the element, the stored byte, the reference and the nearest
    boundary."""
    got = np.asarray(got, np.uint8)
    assert got.shape == ex.u.shape, f'{name}: shape {got.shape} against {ex.u.shape}'
    g = ordinal(got)
    ok = np.where(ex.nan, (got & 0x7F) == 0x7F, (g >= ex.olo) & (g <= ex.ohi))
    fin = ~ex.nan & ((got & 0x7F) != 0x7F)
    uc = np.clip(ex.u, -FMAX, FMAX)
    dist = np.where(fin, np.maximum(np.maximum(_CELL_LO[np.clip(g, -127, 126) + 127] - uc, uc - _CELL_HI[np.clip(g, -127, 126) + 127]), 0.0), 0.0)
    ratio = float(dist.max() / ex.delta)
    print(f'{name}: worst error / bound = {ratio:.3f}, boundary share {ex.boundary_share:.4f}, saturated {ex.saturated_share:.4f}, '
          f'{float((got != ex.want).mean()):.4f} of the bytes are the other code of a boundary')
    if not ok.all():
        i = np.unravel_index(int(np.argmin(ok)), ok.shape)
        raise AssertionError(f'{name}: {int((~ok).sum())} of {ok.size} bytes outside the rule; first at element {tuple(int(k) for k in i)}: stored byte '
                             f'0x{int(got[i]):02X} ({float(decode(got[i]))}), reference {float(ex.u[i])!r} -> 0x{int(ex.want[i]):02X}, nearest boundary '
                             f'{float(nearest_boundary(ex.u[i]))!r}, delta {ex.delta:.4g}, allowed ordinals [{int(ex.olo[i])}, {int(ex.ohi[i])}]')
    return ratio, ex.boundary_share


# ------------------------------------------------------------------------------------------------------------------ cases
FORMS = {'a': ('bf16', 'e4m3', None), 'b': ('e4m3', 'e4m3', None), 'c': ('e4m3', 'bf16', 'bf16'), 'd': ('e4m3', 'e4m3', 'e4m3'),
         'f': ('e4m3', 'f32', None)}
TORCH_DT = {'e4m3': FP8, 'bf16': torch.bfloat16, 'f32': torch.float32}
TOL = {'bf16': R.TOL_BF16_OUT, 'f32': R.TOL_BF16_IN}
CH_SCALE = (1.0, 8.0, 2.0, 0.5)         # filter magnitude of channel co % 4: neighbours co, co ^ 1 are 8 x and 4 x apart


def opt_id(o):
    return f'{o["res"] or "nores"}-post{o["post"]:g}-{"relu" if o["relu"] else "lin"}'


def options(with_res):
    """{ReLU on, off} x {post_scale 1, -1.25} [x {residual before, after the ReLU}]"""
    return [dict(relu=r, res=s, post=p) for s in (('before', 'after') if with_res else (None,)) for p in (1.0, -1.25) for r in (True, False)]


class Case:
    """One 2-D layer (D = 1) in one form, drawn once from a seed fixed by its name.  Real quantities: activations |N(0,1)| (signed=True:
    N(0,1); the trunk's e4m3 activations are post-ReLU), He-scaled filters times CH_SCALE[co % 4], a BN scale that undoes CH_SCALE (as a
    trained BN does) and leaves pre-activations of standard deviation 0.35 .. 0.7, a BN shift 0.2 + 0.2 N(0,1) (about two thirds of the
    pre-activations are positive), a signed residual of standard deviation res_std.  Quantised as the product does: s_in = max|x| / 448,
    s_w[co] = max|w[co]| / 448, s_res = max|r| / 448, s_out = max |result of the option| / 448 (out_cal 0.25: a quarter of it)."""

    def __init__(self, name, form, B, hw, cin, cout, k=1, stride=1, layout=0, signed=False, res_std=0.6, out_cal=1.0, shift_special=None, opts=None):
        self.name, self.form, self.B, self.hw, self.cin, self.cout = name, form, B, tuple(hw), cin, cout
        self.k, self.s, self.layout, self.signed, self.res_std, self.out_cal = k, stride, layout, signed, res_std, out_cal
        self.in_t, self.out_t, self.res_t = FORMS[form]
        self.shift_special = shift_special or {}          # {channel: value} written into the BN shift after the calibration
        self.kernel, self.stride, self.padding = (1, k, k), (1, stride, stride), (0, k // 2, k // 2)
        self._opts = opts
        self._made = False

    @property
    def has_res(self):
        return self.res_t is not None

    def options(self):
        return self._opts if self._opts is not None else options(self.has_res)

    def make(self):
        if self._made:
            return self
        r = np.random.RandomState(sum(map(ord, self.name)))
        taps = self.k * self.k
        x = r.randn(self.B, 1, *self.hw, self.cin)
        x = x if self.signed else np.abs(x)
        chs = np.array([CH_SCALE[c % 4] for c in range(self.cout)])
        w = r.randn(self.cout, 1, self.k, self.k, self.cin) * (2.0 / (taps * self.cin)) ** 0.5 * chs[:, None, None, None, None]
        if self.in_t == 'e4m3':
            self.s_in = float(np.abs(x).max()) / FMAX
            self.s_w = np.abs(w).reshape(self.cout, -1).max(1) / FMAX
            self.xb, self.wb = encode(x / self.s_in), encode(w / self.s_w[:, None, None, None, None])
            self.x_op, self.w_op = decode(self.xb), decode(self.wb)
        else:
            self.s_in, self.s_w = 1.0, np.ones(self.cout)
            self.x_op, self.w_op = R.bf16_round(x.astype(np.float32)).astype(np.float64), R.bf16_round(w.astype(np.float32)).astype(np.float64)
        self.bn_scale = r.uniform(0.25, 0.5, self.cout) / chs
        self.bn_shift = 0.2 + 0.2 * r.randn(self.cout)
        self.acc = R.accumulate(self.x_op, self.w_op, self.kernel, self.stride, self.padding)          # in units of s_in * s_w[co]
        self.oshape = self.acc.shape
        self.pre = self.acc * (self.s_in * self.s_w * self.bn_scale) + self.bn_shift                    # real units, before the options
        self.s_res, self.r_op, self.rb = 1.0, None, None
        if self.has_res:
            res = self.res_std * r.randn(*self.oshape)
            if self.res_t == 'e4m3':
                self.s_res = float(np.abs(res).max()) / FMAX
                self.rb = encode(res / self.s_res)
                self.r_op = decode(self.rb)
            else:
                self.r_op = R.bf16_round(res.astype(np.float32)).astype(np.float64)
        self._s_out = {}
        for o in self.options():
            real = finish(self.pre, None if self.r_op is None else self.r_op * self.s_res, o['relu'], o['res'] == 'after', o['post'])
            self._s_out[opt_id(o)] = self.out_cal * float(np.abs(real).max()) / FMAX if self.out_t == 'e4m3' else 1.0
        for c, val in self.shift_special.items():
            self.bn_shift[c] = val
        self._made = True
        return self

    def s_out(self, o):
        return self.make()._s_out[opt_id(o)]

    def fold(self, o, s_in=None, wrong=None):
        """The header's fold of the unfolded quantities (fp64): scale = bn_scale * s_in * s_w[co] / s_out, shift = bn_shift / s_out,
        res_scale = s_res / s_out.  wrong: one of the three folds a host could get wrong, for the discrimination condition only."""
        self.make()
        s_out = self.s_out(o)
        s_w = self.s_w[np.arange(self.cout) ^ 1] if wrong == 'sw_swapped' else self.s_w
        scale = self.bn_scale * (self.s_in if s_in is None else s_in) * s_w / s_out
        shift = self.bn_shift / (1.0 if wrong == 'shift_undivided' else s_out)
        return scale, shift, (1.0 if wrong == 'res_scale_1' else self.s_res / s_out)

    def value(self, o, scale, shift, res_scale, order='header'):
        """the operation on folded vectors, fp64, before the storage rounding"""
        self.make()
        v = self.acc * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)
        r = None if self.r_op is None else self.r_op * float(res_scale)
        return finish(v, r, o['relu'], o['res'] == 'after', o['post'], order)

    def expect(self, o, scale, shift, res_scale):
        """the folded driver: scale / shift / res_scale exactly as ops.conv_fwd takes them (the kernel's contract)"""
        self.make()
        v = self.acc * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)
        r = None if self.r_op is None else self.r_op * float(res_scale)
        return Expect(v, r, o['relu'], o['res'] == 'after', o['post'], self.out_t)

    def expect_unfolded(self, o, s_in=None):
        """the unfolded driver: BN scale and shift, s_in, s_w[co], s_out, s_res folded by the header's rule (FusedConv._call_quantized)"""
        return self.expect(o, *self.fold(o, s_in))


# name, B, (H, W), Cin, Cout, k, stride, layout.  M = 2*9*13 = 234: one full 128-row tile and a partial one (three full 64-row tiles and a
# partial one); M = 35: fewer rows than any tile; 144 channels: a second (third) column tile of 16 channels; 24: no multiple of 16 (8).
GEOM = [('k1_c16_n16', 2, (9, 13), 16, 16, 1, 1, 0),                  # K = 16: one partial chunk
        ('k1_c128_n144', 2, (9, 13), 128, 144, 1, 1, 1),
        ('k3_c48_n48', 2, (9, 13), 48, 48, 3, 1, 0),                  # K = 432: no multiple of the chunk
        ('k3_c128_n256', 2, (9, 13), 128, 256, 3, 1, 1),                # K = 1152: 18 slabs, split K on 234 rows
        ('k3s2_c48_n144', 2, (11, 14), 48, 144, 3, 2, 0),             # stride 2: 2 * 6 * 7 = 84 rows
        ('m35_c16_n24', 1, (5, 7), 16, 24, 1, 1, 0),                  # the one-byte-per-lane epilogue by rule; bf16 output: the & 7 rule
        ('m35_c512_n256', 1, (5, 7), 512, 256, 1, 1, 1),              # split K with bf16 operands (16 slabs of 32); 8 slabs of 64 bytes in e4m3: none
        ('m35_c1024_n256', 1, (5, 7), 1024, 256, 1, 1, 1)]            # split K with e4m3 operands (16 slabs)
# where plan_conv splits K under its own rule (S >= 16 slabs and too few tiles to fill the chip; asserted through ivx_conv_workspace_bytes)
SPLIT_K = {('k3_c128_n256', f) for f in 'abcd'} | {('m35_c1024_n256', f) for f in 'abcdf'} | {('m35_c512_n256', 'a')}
F_OPTS = [dict(relu=True, res=None, post=-1.25), dict(relu=False, res=None, post=1.0)]
ROUNDING = [Case(f'{g[0]}_{f}', f, *g[1:], opts=F_OPTS if f == 'f' else None, res_std=0.25 if f == 'd' else 0.6) for g in GEOM for f in 'abcdf'
            if not (f == 'f' and g[0] not in ('k1_c128_n144', 'm35_c16_n24', 'm35_c1024_n256'))]
ROUNDING.append(Case('k3_c48_n48_signed_a', 'a', 2, (9, 13), 48, 48, 3, 1, 0, signed=True))
# Saturation and non-finite values, derived from k1_c128_n144_b: s_out from a quarter of the true maximum, and a NaN, +inf and -inf in the
# shift of one channel each (first, second and third 64-column tile), without and with the ReLU.  They enter through the epilogue vector only.
SPECIAL = {5: np.nan, 70: np.inf, 130: -np.inf}
SATURATION = Case('k1_c128_n144_b', 'b', 2, (9, 13), 128, 144, 1, 1, 1, out_cal=0.25, shift_special=SPECIAL,
                  opts=[dict(relu=False, res=None, post=1.0), dict(relu=True, res=None, post=1.0)])
FUSED = ['k3_c48_n48_a', 'k1_c128_n144_b', 'k3_c128_n256_c', 'k1_c128_n144_d']           # one case per form through FusedConv
BY_NAME = {c.name: c for c in ROUNDING}


# ------------------------------------------------------------------------------------------------------------------ conditions on the cases
WRONG_FOLDS = ('res_scale_1', 'shift_undivided', 'sw_swapped', 'swapped', 'scaled_early')


def has_feature(case, o, wrong):
    if wrong == 'res_scale_1':
        return case.res_t == 'e4m3'
    if wrong == 'shift_undivided':
        return case.out_t == 'e4m3'
    if wrong == 'sw_swapped':
        return case.in_t == 'e4m3'
    if wrong == 'swapped':
        return case.has_res and o['relu']
    return o['post'] != 1.0 and ((o['relu'] and o['post'] < 0) or case.has_res)


def separated(case, o, wrong):
    """share of the elements at which a wrong fold (or a wrong order) lies more than two code steps (e4m3 output) or more than 4 x the
    bar (bf16 / fp32 output) away from the reference"""
    ref = case.value(o, *case.fold(o))
    bad = case.value(o, *case.fold(o), order=wrong) if wrong in ('swapped', 'scaled_early') else case.value(o, *case.fold(o, wrong=wrong))
    if case.out_t == 'e4m3':
        return float((np.abs(steps(encode(ref)) - steps(encode(bad))) > 2).mean())
    return float((np.abs(ref - bad) > 4.0 * R.bound_of(ref, TOL[case.out_t])).mean())


# ------------------------------------------------------------------------------------------------------------------ the device driver
def to_device(case):
    """the operands as ops.conv_fwd takes them: channels-last input, packed filters (layout 1: 128-byte channel chunks), residual"""
    case.make()
    ck = 128 if case.in_t == 'e4m3' else 64

    def up(a, kind):
        if kind == 'e4m3':
            return torch.from_numpy(np.ascontiguousarray(a, np.uint8)).cuda().view(FP8)
        return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda().to(TORCH_DT[kind])        # (exact: the values are bf16 already)
    w = case.wb if case.in_t == 'e4m3' else case.w_op
    w = up(R.pack_layout1(w, ck) if case.layout == 1 else w, case.in_t)
    x = up(case.xb if case.in_t == 'e4m3' else case.x_op, case.in_t)
    res = None if not case.has_res else up(case.rb if case.res_t == 'e4m3' else case.r_op, case.res_t)
    return x, w, res


def folded_f32(case, o, s_in=None):
    """the fold rounded to what the entry point takes: fp32 vectors and an fp32 res_scale"""
    scale, shift, rs = case.fold(o, s_in)
    return scale.astype(np.float32), shift.astype(np.float32), float(np.float32(rs))


def prefilled(case):
    """an output no kernel has written: byte 0x7F (an e4m3 NaN) or NaN"""
    if case.out_t == 'e4m3':
        return torch.full(case.oshape, 0x7F, device='cuda', dtype=torch.uint8).view(FP8)
    return torch.full(case.oshape, float('nan'), device='cuda', dtype=TORCH_DT[case.out_t])


def run(ops, case, o, dev, vec, naive=False):
    """one ops.conv_fwd call with hand-folded vectors on a pre-filled output; dev = to_device(case), vec = (scale, shift) device tensors
    and res_scale.  Returns the device tensor."""
    x, w, res = dev
    return ops.conv_fwd(x, w, vec[0], vec[1], case.kernel, case.stride, case.padding, o['relu'], res if o['res'] else None, 1 if o['res'] else 0, naive=naive,
                        out=prefilled(case), wgt_layout=case.layout, res_after_act=o['res'] == 'after', post_scale=o['post'], out_dtype=TORCH_DT[case.out_t],
                        res_scale=vec[2])


def to_host(case, y):
    return y.view(torch.uint8).cpu().numpy() if case.out_t == 'e4m3' else y.float().cpu().numpy()
