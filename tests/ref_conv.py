"""The conv epilogue (include/imvoxel.h: v = acc*scale + shift; [v += res]; [ReLU]; [v += res if res_after_act]; v *= post_scale) against
plain fp64: the reference, the cases, the option set, the tolerances, the condition that makes the cases able to tell a wrong order from
the right one, and the driver of the fp32 direct form -- shared by tests/test_host_conv_epilogue.py (the CPU restatement oracle/cpu_abi,
no device) and tests/test_gpu_conv_epilogue.py (the HIP library).

No kernel of the project is in here and no reference comes out of the library.  The reference is a sum of per-tap matrix products in
fp64 followed by the header's sentence, one numpy statement per clause; the two wrong orders a kernel could have (the residual on the
other side of the ReLU, the multiplier before the ReLU) exist here only to prove that the inputs separate them (discrimination)."""
import ctypes as C
import itertools

import numpy as np
import torch
import torch.nn.functional as F

from ref_pair import ConvDesc, _p

# |d| <= RTOL |ref| + ATOL max|ref|: the bars of test_conv_winograd_matches_direct / test_conv_winograd_f16_pair_operands (fp32 and pair
# operands), test_conv_bf16_storage (bf16 output: 2^-7 relative + 1e-3; fp32 output from bf16 operands 2e-4).  The options add one add and
# one multiply in fp32: two roundings of 2^-24, nothing widens.
# (rtol, atol, atol is a fraction of max|ref|): the two bf16 bars are assert_close's, whose atol is absolute
TOL_F32 = (1e-4, 1e-4, True)
TOL_BF16_OUT = (2.0 ** -7, 1e-3, False)
TOL_BF16_IN = (2e-4, 2e-4, False)
POST_SCALES = (1.0, 0.5, -1.25)


# ------------------------------------------------------------------------------------------------------------------ the option set
def options(with_res=True):
    """dict(after, post, relu): {res before act, res after act} x {post_scale 1, 0.5, -1.25} x {ReLU on, off}; without a residual the
    first factor is gone"""
    return [dict(after=a, post=p, relu=r) for a, p, r in itertools.product((False, True) if with_res else (False,), POST_SCALES, (True, False))]


def opt_id(o):
    return f'{"after" if o["after"] else "before"}-post{o["post"]:g}-{"relu" if o["relu"] else "lin"}'


# ------------------------------------------------------------------------------------------------------------------ the fp64 reference
def nearest_index(n_out, n_in):
    """source index of every output index under F.interpolate(mode='nearest'), read off an fp32 tensor of integer indices: the rule
    the product copies (res_mode 2)"""
    src = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1)
    return F.interpolate(src, size=(n_out, 1), mode='nearest').view(-1).numpy().astype(np.int64)


def nearest_index_exact(n_out, n_in):
    """floor(i * n_in / n_out) in integers"""
    return (np.arange(n_out, dtype=np.int64) * n_in) // n_out


def accumulate(x, w, kernel, stride, padding):
    """x [B,D,H,W,Cin], w [Cout,KD,KH,KW,Cin] -> fp64 [B,Do,Ho,Wo,Cout]: zero padding, one matrix product per tap"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, ci = x.shape[0], x.shape[4]
    co = w.shape[0]
    no = [(x.shape[1 + a] + 2 * padding[a] - kernel[a]) // stride[a] + 1 for a in range(3)]
    xp = np.zeros((B,) + tuple(x.shape[1 + a] + 2 * padding[a] for a in range(3)) + (ci,))
    xp[:, padding[0]:padding[0] + x.shape[1], padding[1]:padding[1] + x.shape[2], padding[2]:padding[2] + x.shape[3]] = x
    acc = np.zeros((B * no[0] * no[1] * no[2], co))
    for kd, kh, kw in itertools.product(range(kernel[0]), range(kernel[1]), range(kernel[2])):
        sl = xp[:, kd:kd + (no[0] - 1) * stride[0] + 1:stride[0], kh:kh + (no[1] - 1) * stride[1] + 1:stride[1],
                kw:kw + (no[2] - 1) * stride[2] + 1:stride[2]]
        acc += sl.reshape(-1, ci) @ w[:, kd, kh, kw].T
    return acc.reshape(B, no[0], no[1], no[2], co)


def scatter_up2(acc):
    """out_mode 1 (ConvTranspose3d kernel 2 stride 2 as a 1x1x1 GEMM): columns n = ((a*2+e)*2+f)*C + co of [B,D,H,W,8C] go to
    out[b, 2d+a, 2h+e, 2w+f, co]"""
    B, D, H, W, n = acc.shape
    c = n // 8
    return acc.reshape(B, D, H, W, 2, 2, 2, c).transpose(0, 1, 4, 2, 5, 3, 6, 7).reshape(B, 2 * D, 2 * H, 2 * W, c)


def residual_at_output(res, res_mode, oshape):
    """the residual every output element sees, fp64 in the output's shape: res_mode 1 as it is, res_mode 2 [B,1,h,w,C] nearest-upsampled"""
    r = np.asarray(res, np.float64)
    if res_mode == 2:
        r = r[:, :, nearest_index(oshape[2], r.shape[2])][:, :, :, nearest_index(oshape[3], r.shape[3])]
    assert r.shape == tuple(oshape), (r.shape, oshape)
    return r


def finish(v, r, relu, after, post, order='header'):
    """The header's sentence on v = acc*scale + shift (fp64) and the residual r (or None).  order 'swapped': the residual on the other
    side of the ReLU; 'scaled_early': the multiplier applied before the residual and the ReLU -- the two mistakes the cases must expose."""
    if order == 'swapped':
        after = not after
    if order == 'scaled_early':
        v = v * post
    if r is not None and not after:
        v = v + r
    if relu:
        v = np.maximum(v, 0.0)
    if r is not None and after:
        v = v + r
    return v if order == 'scaled_early' else v * post


def conv3d(x, w, scale, shift, kernel, stride=(1, 1, 1), padding=(0, 0, 0), relu=False, res=None, res_mode=0, res_after_act=False,
           post_scale=1.0, out_mode=0):
    """the whole operation of ivx_conv_desc in fp64, channels-last"""
    acc = accumulate(x, w, kernel, stride, padding)
    if out_mode == 1:
        acc = scatter_up2(acc)
    v = acc * (1.0 if scale is None else np.asarray(scale, np.float64)) + (0.0 if shift is None else np.asarray(shift, np.float64))
    r = None if res is None else residual_at_output(res, res_mode or 1, v.shape)
    return finish(v, r, relu, res_after_act, 1.0 if post_scale == 0 else float(post_scale))


# ------------------------------------------------------------------------------------------------------------------ cases
class Case:
    """One layer with its tensors (fp32, drawn once) and the fp64 pre-activation, computed once and left unchanged.
    randn input, He-scaled filters, scale in [0.5, 1.5], shift 0.1 randn: about half the pre-activations are negative."""

    def __init__(self, name, B, sp, cin, cout, kernel=(3, 3, 3), stride=(1, 1, 1), padding=None, res_mode=1, res_hw=None, out_mode=0,
                 rounding=None, res_std=1.0):
        self.name, self.B, self.sp, self.cin, self.cout = name, B, tuple(sp), cin, cout
        self.kernel, self.stride = tuple(kernel), tuple(stride)
        self.padding = tuple(k // 2 for k in kernel) if padding is None else tuple(padding)
        self.res_mode, self.res_hw, self.out_mode = res_mode, res_hw, out_mode
        self.rounding = rounding                  # a function fp32 array -> fp32 array: the storage rounding of operands and residual (bf16)
        # standard deviation of the residual.  The bf16 cases take 4: 100 x the bf16-output bar is 78 % of a value, and a unit residual moves
        # only 15 % of the outputs that far when it changes sides of the ReLU (4 does on a third: test_cases_tell_the_orders_apart)
        self.res_std = res_std
        self._made = False

    def make(self):
        if self._made:
            return self
        rd = self.rounding or (lambda a: a)
        r = np.random.RandomState(sum(map(ord, self.name)))
        taps = self.kernel[0] * self.kernel[1] * self.kernel[2]
        self.x = rd(r.randn(self.B, *self.sp, self.cin).astype(np.float32))
        self.w = rd((r.randn(self.cout, *self.kernel, self.cin) * (2.0 / (taps * self.cin)) ** 0.5).astype(np.float32))
        cr = self.cout // 8 if self.out_mode == 1 else self.cout
        self.scale = r.uniform(0.5, 1.5, cr).astype(np.float32)
        self.shift = (0.1 * r.randn(cr)).astype(np.float32)
        acc = accumulate(self.x, self.w, self.kernel, self.stride, self.padding)
        if self.out_mode == 1:
            acc = scatter_up2(acc)
        self.pre = acc * self.scale.astype(np.float64) + self.shift.astype(np.float64)
        self.oshape = self.pre.shape
        self.res = self.res_up = None
        if self.res_mode == 1:
            self.res = rd((self.res_std * r.randn(*self.oshape)).astype(np.float32))
        elif self.res_mode == 2:
            self.res = rd((self.res_std * r.randn(self.B, 1, self.res_hw[0], self.res_hw[1], self.cout)).astype(np.float32))
        if self.res is not None:
            self.res_up = residual_at_output(self.res, self.res_mode, self.oshape)
        self._made = True
        return self

    @property
    def has_res(self):
        return self.res_mode != 0

    def options(self):
        return options(self.has_res)

    def ref(self, o, order='header'):
        self.make()
        return finish(self.pre, self.res_up, o['relu'], o['after'], o['post'], order)


def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).float().numpy()


# fp32 direct form: name, B, (D,H,W), Cin, Cout, ...
DIRECT = [Case('d_8_20', 1, (5, 6, 7), 8, 20),
          Case('d_8_22_cout_not_4', 1, (5, 6, 7), 8, 22),                       # Cout % 4 != 0: the one-channel-per-lane epilogue by rule
          Case('d_64_72_s112', 2, (9, 11, 12), 64, 72, stride=(1, 1, 2))]
SPLITK = [Case('sk_256_192_3x3x3', 1, (5, 5, 2), 256, 192),
          Case('sk_fpn_lat_x2', 1, (1, 12, 40), 2048, 64, kernel=(1, 1, 1), res_mode=2, res_hw=(6, 20)),
          Case('sk_fpn_lat_7x21', 1, (1, 12, 40), 2048, 64, kernel=(1, 1, 1), res_mode=2, res_hw=(7, 21))]
RES2_SMALL = [Case('r2_13x21_from_7x11', 2, (1, 13, 21), 32, 16, kernel=(1, 1, 1), res_mode=2, res_hw=(7, 11)),
              Case('r2_equal', 2, (1, 12, 20), 32, 16, kernel=(1, 1, 1), res_mode=2, res_hw=(12, 20))]
UP2 = [Case(f'up2_{ci}_{co}', 2, (3, 5, 4), ci, 8 * co, kernel=(1, 1, 1), out_mode=1) for ci, co in ((8, 4), (64, 32), (36, 20), (32, 40))]
BF16 = [Case('bf_64_64_3x3x3', 1, (10, 12, 12), 64, 64, rounding=bf16_round, res_std=4.0),
        Case('bf_256_64_res2', 2, (1, 13, 21), 256, 64, kernel=(1, 1, 1), res_mode=2, res_hw=(7, 11), rounding=bf16_round, res_std=4.0)]
PAIR_SPLIT = [Case('pair_64_128_s2', 1, (8, 8, 4), 64, 128, stride=(2, 2, 2))]
WINO = [Case('w_16_12', 2, (9, 14, 5), 16, 12), Case('w_32_64_zs2', 1, (12, 10, 6), 32, 64, stride=(1, 1, 2)),
        Case('w_128_128', 3, (31, 17, 2), 128, 128)]
FUSED = [Case('f_64_64', 1, (5, 3, 2), 64, 64), Case('f_32_128', 1, (9, 14, 5), 32, 128), Case('f_128_96', 3, (12, 8, 3), 128, 96)]
ROUTE = [Case('route_64_64_wino', 1, (16, 16, 8), 64, 64), Case('route_64_128_s2_split', 1, (8, 8, 4), 64, 128, stride=(2, 2, 2))]
RES2_SIZES = [((12, 40), (6, 20)), ((12, 40), (7, 21)), ((13, 21), (7, 11)), ((12, 20), (12, 20))]      # exact x2, non-integer, non-integer, equal
HOST_CASES = DIRECT + SPLITK + RES2_SMALL + UP2                   # what the CPU restatement runs (fp32, no Winograd there)
ALL_CASES = HOST_CASES + BF16 + PAIR_SPLIT + WINO + FUSED + ROUTE


def tol_of(case):
    return TOL_BF16_IN if case.rounding is not None else TOL_F32


# ------------------------------------------------------------------------------------------------------------------ checks
def bound_of(ref, tol):
    return tol[0] * np.abs(ref) + tol[1] * (float(np.abs(ref).max()) if tol[2] else 1.0)


def check(name, got, ref, tol):
    """every element finite (the outputs are pre-filled with NaN) and |got - ref| <= rtol |ref| + atol (max|ref|); prints and returns the
    worst error / tolerance"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, f'{name}: shape {got.shape} against {ref.shape}'
    bad = int((~np.isfinite(got)).sum())
    assert bad == 0, f'{name}: {bad} elements were not written or are not finite'
    bound = bound_of(ref, tol)
    ratio = float((np.abs(got - ref) / bound).max())
    print(f'{name}: worst error / tolerance = {ratio:.3f}')
    assert ratio <= 1.0, f'{name}: |out - ref| is {ratio:.2f} x the tolerance at {np.unravel_index(int((np.abs(got - ref) / bound).argmax()), ref.shape)}'
    return ratio


def separated(a, b, tol):
    """fraction of the elements at which b lies more than 100 x the tolerance (taken at a) away from a"""
    return float((np.abs(a - b) > 100.0 * bound_of(a, tol)).mean())


def discrimination(case, tol=None):
    """A condition on the inputs, from the reference alone.  For every option of the case with a residual and the ReLU, the reference with
    the residual on the other side of the ReLU differs from the right one by more than 100 x the tolerance on at least 25 % of the
    elements; for every option with the ReLU and a negative post_scale, or with a residual and any post_scale, so does the reference that
    multiplies first.  (relu(0.5 v) == 0.5 relu(v): without a residual a positive multiplier commutes with the ReLU, and without the
    ReLU and the residual every multiplier does -- those options cannot tell the orders apart and 0.5 alone never could; -1.25 does.)
    Returns {option id: (fraction under the swapped residual or None, fraction under the early multiplier or None)} and asserts that
    the case has both kinds."""
    tol = tol or tol_of(case)
    out, kinds = {}, set()
    for o in case.options():
        ref = case.ref(o)
        f_res = f_post = None
        if case.has_res and o['relu']:
            f_res = separated(ref, case.ref(o, 'swapped'), tol)
            assert f_res >= 0.25, f'{case.name} {opt_id(o)}: the other residual order is told apart on {f_res:.3f} of the elements only'
            kinds.add('res')
        if o['post'] != 1.0 and ((o['relu'] and o['post'] < 0) or case.has_res):
            f_post = separated(ref, case.ref(o, 'scaled_early'), tol)
            assert f_post >= 0.25, f'{case.name} {opt_id(o)}: scaling before the ReLU is told apart on {f_post:.3f} of the elements only'
            kinds.add('post')
        out[opt_id(o)] = (f_res, f_post)
    assert 'post' in kinds and (not case.has_res or 'res' in kinds), (case.name, kinds)
    neg = float((case.pre < 0).mean())
    assert 0.3 < neg < 0.7, f'{case.name}: {neg:.2f} of the pre-activations are negative'
    return out


# ------------------------------------------------------------------------------------------------------------------ the fp32 direct driver
def pack_layout1(w, ck=32):
    """[Cout,KD,KH,KW,Cin] -> wgt_layout 1 [Cout, Cin/ck, KD,KH,KW, ck] (include/imvoxel.h)"""
    co, kd, kh, kw, ci = w.shape
    return np.ascontiguousarray(w.reshape(co, kd, kh, kw, ci // ck, ck).transpose(0, 4, 1, 2, 3, 5))


def bind(L):
    """argument types of the entry points used here, for a library loaded without them"""
    vp, i64 = C.c_void_p, C.c_int64
    L.ivx_last_error.restype = C.c_char_p
    L.ivx_conv_workspace_bytes.restype, L.ivx_conv_workspace_bytes.argtypes = i64, [C.POINTER(ConvDesc)]
    L.ivx_conv_fwd_ws.restype, L.ivx_conv_fwd_ws.argtypes = C.c_int, [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp, i64, vp]


class HostBackend:
    """The entry points on host memory (the CPU restatement); tests/test_gpu_conv_epilogue.py has the device twin."""
    name = 'cpu'
    ConvDesc = ConvDesc

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


def run_direct(be, case, o, layout=0):
    """One ivx_conv_fwd_ws call on fp32 tensors, the output pre-filled with NaN.  Returns (output as numpy, workspace bytes the library asked for)."""
    case.make()
    d = be.ConvDesc()
    d.B, (d.D, d.H, d.W), d.Cin, d.Cout = case.B, case.sp, case.cin, case.cout
    (d.KD, d.KH, d.KW), (d.sd, d.sh, d.sw), (d.pd, d.ph, d.pw) = case.kernel, case.stride, case.padding
    d.relu, d.res_mode, d.wgt_layout, d.out_mode, d.res_after_act = int(o['relu']), case.res_mode, layout, case.out_mode, int(o['after'])
    d.post_scale, d.in_dtype, d.out_dtype, d.res_scale = o['post'], 0, 0, 1.0
    if case.res_mode == 2:
        d.res_h, d.res_w = case.res_hw
    x, w = be.up(case.x), be.up(pack_layout1(case.w) if layout == 1 else case.w)
    sc, sf = be.up(case.scale), be.up(case.shift)
    res = None if case.res is None else be.up(case.res)
    out = be.full(case.oshape, np.float32, np.nan)
    nb = int(be.L.ivx_conv_workspace_bytes(C.byref(d)))
    assert nb >= 0, 'ivx_conv_workspace_bytes'
    ws = be.full((max(nb, 256),), np.uint8, 0)
    be.ok(be.L.ivx_conv_fwd_ws(C.byref(d), _p(be, x), _p(be, w), _p(be, sc), _p(be, sf), _p(be, res), _p(be, out), _p(be, ws), nb, be.stream),
          'ivx_conv_fwd_ws')
    return be.get(out), nb


def run_direct_options(be, case, layout=0, want_split=None):
    """every option of the case through run_direct against the fp64 reference; want_split: assert that the library did (True) or did
    not (False) plan split-K.  Returns the worst error / tolerance."""
    worst = 0.0
    for o in case.options():
        got, nb = run_direct(be, case, o, layout)
        if want_split is not None:
            assert (nb > 0) == want_split, f'{case.name}: ivx_conv_workspace_bytes = {nb}'
        worst = max(worst, check(f'{be.name} {case.name} layout {layout} {opt_id(o)}', got, case.ref(o), TOL_F32))
    return worst
