"""Tensor-level wrappers over the C-ABI.  torch tensors are containers only: every wrapper
checks device / dtype / contiguity (as CHECK_INPUT does for the reference's native op,
mmdet3d/ops/iou3d/src/iou3d.cpp:17-23), allocates the output with torch.empty and passes raw
pointers plus the current HIP stream to libimvoxel_hip.so.

Internal activation layout is channels-last: 5-D [B, D, H, W, C] (a 2-D map has D == 1).
"""
import ctypes as C
import math

import torch

from . import _lib
from ._lib import ConvDesc, AnchorHeadDesc, check


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


FP8 = torch.float8_e4m3fn      # OCP e4m3 bytes with a per-tensor scale kept by the caller (conv.QTensor)
_DT = {torch.float32: 0, torch.bfloat16: 1, FP8: 2}   # IVX_F32 / IVX_BF16 / IVX_FP8


def _chk(t, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f'{name} must be a torch.Tensor')
    if not t.is_cuda:
        raise RuntimeError(f'{name} must be a device (HIP) tensor; the MI355X path has no CPU fallback')
    if t.dtype != dtype:
        raise TypeError(f'{name} must be {dtype}, got {t.dtype}')
    if not t.is_contiguous():
        raise ValueError(f'{name} must be contiguous')
    return t


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ------------------------------------------------------------------ layout
def image_s2d_bf16(img):
    """bf16 mode: image [N,3,H,W] fp32 -> 2x2 space-to-depth blocks [N,1,H/2+1,W/2+1,16] bf16 (ivx_image_s2d_bf16): the input of
    the stem in its 4x4 stride-1 form (backbones.ResNet)."""
    _chk(img, 'img')
    N, Cn, H, W = img.shape
    if Cn != 3:
        raise ValueError('image_s2d_bf16 takes a 3-channel image')
    out = torch.empty((N, 1, H // 2 + 1, W // 2 + 1, 16), device=img.device, dtype=torch.bfloat16)
    check(_lib.lib().ivx_image_s2d_bf16(_ptr(img), N, H, W, _ptr(out), _stream()), 'ivx_image_s2d_bf16')
    return out


def _entry(name, version, what):
    """The entry `name` of the loaded library, which has it since `version`; an older build of the ABI refuses here."""
    L = _lib.lib()
    if not hasattr(L, name):
        raise _lib.IvxError(f'{name} is not in the loaded libimvoxel_hip.so (version {L.ivx_version()} < {version}): {what}')
    return getattr(L, name)


_LENS_ABI = (502, 'the lens-aware image pipeline needs 0.5.2')
_FMT_ABI = (503, 'decoder pixel formats in the image pipeline need 0.5.3')


def _bgr_frames(src):
    """The packed-BGR tensor rule of image_prep_u8 / image_prep_lens_u8 -> (n, H, W, row bytes)."""
    if not isinstance(src, torch.Tensor):
        raise TypeError('src must be a torch.Tensor')
    if not src.is_cuda:
        raise RuntimeError('src must be a device (HIP) tensor; the MI355X path has no CPU fallback')
    if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[3] != 3:
        raise TypeError(f'src must be uint8 [n,H,W,3], got {src.dtype} {tuple(src.shape)}')
    n, H, W, _ = src.shape
    if n < 1:
        raise ValueError('src holds no frame')
    row = src.stride(1) if H > 1 else 3 * W                  # (the stride of an extent-1 axis is arbitrary)
    if src.stride(3) != 1 or (W > 1 and src.stride(2) != 3) or row < 3 * W or (n > 1 and src.stride(0) < H * row):
        raise ValueError(f'src rows must be dense HWC (strides (>= H * row, >= 3 * W, 3, 1)), got {tuple(src.stride())}')
    return n, H, W, row


def _prep_out(out, shape, device, where=True):
    """The `out` argument of the image ops: a new fp32 tensor of `shape` on `device`, or the caller's, checked (where: the message names the
    device and the check asks for it)."""
    if out is None:
        return torch.empty(shape, device=device, dtype=torch.float32)
    _chk(out, 'out')
    if tuple(out.shape) != tuple(shape) or (where and out.device != device):
        want = f'[{",".join(str(v) for v in shape)}]' if len(shape) == 4 else f'{list(shape)}'
        raise ValueError(f'out must be {want}' + (f' on {device}' if where else '') + f', got {tuple(out.shape)} on {out.device}')
    return out


def _prep_desc(H, W, row, size_hw, pad_hw, to_rgb=False, mean=(0, 0, 0), std=(1, 1, 1)):
    return _lib.ImagePrepDesc(H, W, row, *size_hw, *pad_hw, int(bool(to_rgb)), (C.c_float * 3)(*[float(v) for v in mean]),
                              (C.c_float * 3)(*[float(v) for v in std]))


def image_prep_u8(src, size_hw, pad_hw, mean, std, to_rgb=True, out=None):
    """uint8 frames [n,H,W,3] (HWC, BGR as a decoder leaves them) -> Resize to size_hw -> Normalize -> zero Pad to pad_hw:
    [n,3,pad_h,pad_w] fp32 in one launch (ivx_image_prep_u8), bit-identical to data.prepare_image per frame.  The pixels of a row
    must be dense (strides (.., 3, 1)); a row stride above 3 * W (a decoder pitch) and any frame stride are passed through.
    mean / std in output-channel order; out: a contiguous fp32 [n,3,pad_h,pad_w] view to write into (a slice of a batch tensor)."""
    n, H, W, row = _bgr_frames(src)
    (nh, nw), (ph, pw) = (int(v) for v in size_hw), (int(v) for v in pad_hw)
    out = _prep_out(out, (n, 3, ph, pw), src.device)
    d = _prep_desc(H, W, row, (nh, nw), (ph, pw), to_rgb, mean, std)
    check(_lib.lib().ivx_image_prep_u8(C.byref(d), _ptr(src), src.stride(0), n, _ptr(out), _stream()), 'ivx_image_prep_u8')
    return out


def _lens_struct(lens, name='lens'):
    """A data.Lens (anything with .struct()) -> _lib.Lens."""
    if not hasattr(lens, 'struct'):
        raise TypeError(f'{name} must be a data.Lens, got {type(lens).__name__}')
    return lens.struct()


def image_prep_lens_u8(src, lens, size_hw, pad_hw, mean, std, to_rgb=True, out=None):
    """image_prep_u8 for the frames of a real camera: Undistort -> Resize -> Normalize -> zero Pad in one launch and ONE interpolation
    (ivx_image_prep_lens_u8; include/imvoxel.h has the definition of the map G and of the fp32 bilinear blend).  lens: a data.Lens, one for
    all n frames; the output shows the ideal camera lens.new_K (at the source size), and pixels that G sends outside the frame or beyond
    r2_max are border: +0.0f, like the pad.  Everything else as image_prep_u8."""
    fn = _entry('ivx_image_prep_lens_u8', *_LENS_ABI)
    ls = _lens_struct(lens)
    n, H, W, row = _bgr_frames(src)
    (nh, nw), (ph, pw) = (int(v) for v in size_hw), (int(v) for v in pad_hw)
    out = _prep_out(out, (n, 3, ph, pw), src.device)
    d = _prep_desc(H, W, row, (nh, nw), (ph, pw), to_rgb, mean, std)
    check(fn(C.byref(d), C.byref(ls), _ptr(src), src.stride(0), n, _ptr(out), _stream()), 'ivx_image_prep_lens_u8')
    return out


_PIX_BYTES = {'bgr': 3, 'rgb': 3, 'bgra': 4, 'rgba': 4, 'gray': 1}      # bytes per pixel of the packed one-sample-per-pixel layouts


def image_prep_fmt_u8(src, fmt, size_hw, pad_hw, mean, std, to_rgb=True, lens=None, out=None, src_hw=None, row_bytes=None, plane1_offset=None,
                      plane1_row_bytes=None):
    """image_prep_u8 / image_prep_lens_u8 on frames in a decoder's pixel format (ivx_image_prep_fmt_u8; include/imvoxel.h has the integer
    definition): the frame IS a BGR frame through data.to_bgr_u8's rule, converted inside the fetch of the same one launch, and the result
    equals the BGR entry on the converted frames bit for bit.  fmt: a data.FrameFormat or a layout name.  src, a device uint8 tensor:
      'bgr' | 'rgb' [n,H,W,3], 'bgra' | 'rgba' [n,H,W,4], 'gray' [n,H,W] or [n,H,W,1], 'yuyv' [n,H,2*ceil(W/2),2] -- pixels of a row
          dense, a row stride above the row's bytes (a decoder pitch) and any frame stride are passed through, as for image_prep_u8;
      'nv12' [n, H + ceil(H/2), 2*ceil(W/2)]: the usual stacked array, Y rows then UV rows at one pitch;
      any layout, a raw surface: a 1-D tensor (one frame) or 2-D [n, bytes] (bytes dense) with src_hw=(H, W), row_bytes= and for NV12
          plane1_offset= / plane1_row_bytes=: a decoder's pitched surface as it lies, without a copy.
    src_hw: the frame size where the array cannot tell it (an odd W of 'yuyv' / 'nv12'; required for a raw surface).  lens: a data.Lens
    (image_prep_lens_u8's rule) or None.  Everything else as image_prep_u8."""
    fn = _entry('ivx_image_prep_fmt_u8', *_FMT_ABI)
    from .data import FrameFormat
    if not isinstance(fmt, FrameFormat):
        fmt = FrameFormat(fmt)
    ls = None if lens is None else _lens_struct(lens)
    if not isinstance(src, torch.Tensor):
        raise TypeError('src must be a torch.Tensor')
    if not src.is_cuda:
        raise RuntimeError('src must be a device (HIP) tensor; the MI355X path has no CPU fallback')
    if src.dtype != torch.uint8:
        raise TypeError(f'src must be uint8, got {src.dtype}')
    lay = fmt.layout
    hw = None if src_hw is None else tuple(int(v) for v in src_hw)
    if hw is not None and (len(hw) != 2 or min(hw) < 1):
        raise ValueError(f'src_hw must be a positive (H, W), got {src_hw!r}')
    p1_off = p1_row = 0
    if row_bytes is not None:                                    # a raw surface: the geometry is the caller's
        if hw is None:
            raise ValueError('a raw surface (row_bytes=) needs src_hw=(H, W)')
        if src.dim() not in (1, 2) or src.stride(-1) != 1:
            raise TypeError(f'a raw surface must be a 1-D tensor or [n, bytes] with dense bytes, got {tuple(src.shape)} strides {tuple(src.stride())}')
        H, W = hw
        n, size = (1, src.shape[0]) if src.dim() == 1 else (int(src.shape[0]), int(src.shape[1]))
        step = src.stride(0) if src.dim() == 2 else size
        row = int(row_bytes)
        cw, ch = (W + 1) // 2, (H + 1) // 2
        tight = 4 * cw if lay == 'yuyv' else W if lay == 'nv12' else _PIX_BYTES[lay] * W
        if row < tight:
            raise ValueError(f'row_bytes {row} is below the {tight} bytes of a {lay} row of {W} pixels')
        end = (H - 1) * row + tight
        if lay == 'nv12':
            if plane1_offset is None or plane1_row_bytes is None:
                raise ValueError('a raw NV12 surface needs plane1_offset= and plane1_row_bytes=')
            p1_off, p1_row = int(plane1_offset), int(plane1_row_bytes)
            if p1_row < 2 * cw or p1_off < H * row:
                raise ValueError(f'plane1_row_bytes {p1_row} / plane1_offset {p1_off} are below 2 * ceil(W / 2) = {2 * cw} / H * row_bytes = {H * row}')
            end = p1_off + (ch - 1) * p1_row + 2 * cw
        elif plane1_offset is not None or plane1_row_bytes is not None:
            raise ValueError(f"plane1_offset / plane1_row_bytes belong to 'nv12', not to {lay!r}")
        if n < 1 or size < end:
            raise ValueError(f'the surface holds {n} x {size} bytes, a frame of this geometry ends at byte {end}')
    else:
        if plane1_offset is not None or plane1_row_bytes is not None:
            raise ValueError('plane1_offset / plane1_row_bytes describe a raw surface: pass row_bytes= and src_hw= with them')
        if lay == 'nv12':
            if src.dim() != 3:
                raise TypeError(f"'nv12' frames must be [n, H + ceil(H/2), W] uint8 (or a raw surface with row_bytes=), got {tuple(src.shape)}")
            n, R, We = (int(v) for v in src.shape)
            if We % 2 or R % 3 == 1 or R < 2:
                raise ValueError(f"a stacked 'nv12' array has an even width and H + ceil(H/2) rows, got {R} x {We}")
            H, W = (2 * R) // 3 if R % 3 == 0 else (2 * R - 1) // 3, We
            if hw is not None:
                if hw[0] != H or (hw[1] + 1) // 2 * 2 != We:
                    raise ValueError(f'src_hw {hw} does not fit a stacked nv12 array of {R} x {We}')
                W = hw[1]
            row = src.stride(1)
            if (We > 1 and src.stride(2) != 1) or row < We or (n > 1 and src.stride(0) < R * row):
                raise ValueError(f'src rows must be dense (strides (>= rows * row, >= W, 1)), got {tuple(src.stride())}')
            p1_off, p1_row = H * row, row
        else:
            if lay == 'gray' and src.dim() == 3:
                src = src.unsqueeze(3)
            Cb = 2 if lay == 'yuyv' else _PIX_BYTES[lay]
            if src.dim() != 4 or src.shape[3] != Cb:
                raise TypeError(f'{lay!r} frames must be uint8 [n,H,W,{Cb}], got {tuple(src.shape)}')
            n, H, We, _ = (int(v) for v in src.shape)
            W = We
            if lay == 'yuyv':
                if We % 2:
                    raise ValueError(f"a 'yuyv' array holds 2 * ceil(W/2) samples per row, got {We}")
                if hw is not None:
                    W = hw[1]
            if hw is not None and (hw[0] != H or (hw[1] != We if lay != 'yuyv' else (hw[1] + 1) // 2 * 2 != We)):
                raise ValueError(f'src_hw {hw} does not fit {lay!r} frames of shape {tuple(src.shape)}')
            row = src.stride(1) if H > 1 else Cb * We            # (the stride of an extent-1 axis is arbitrary)
            if (Cb > 1 and src.stride(3) != 1) or (We > 1 and src.stride(2) != Cb) or row < Cb * We or (n > 1 and src.stride(0) < H * row):
                raise ValueError(f'src rows must be dense (strides (>= H * row, >= {Cb} * W, {Cb}, 1)), got {tuple(src.stride())}')
        if n < 1:
            raise ValueError('src holds no frame')
        step = src.stride(0)
    (nh, nw), (ph, pw) = (int(v) for v in size_hw), (int(v) for v in pad_hw)
    out = _prep_out(out, (n, 3, ph, pw), src.device)
    d = _prep_desc(H, W, row, (nh, nw), (ph, pw), to_rgb, mean, std)
    fs = fmt.struct(plane1_offset=p1_off, plane1_row_bytes=p1_row)
    check(fn(C.byref(d), C.byref(fs), None if ls is None else C.byref(ls), _ptr(src), step, n, _ptr(out), _stream()), 'ivx_image_prep_fmt_u8')
    return out


_MAP_DT = {torch.float32: (_lib.MAP_F32, 4), torch.uint16: (_lib.MAP_U16, 2)}


def map_prep_lens(size_hw, pad_hw, src_hw, lens=None, src=None, scale=1.0, stride=4, n=1, out=None, device=None):
    """The feature-resolution maps of the geometry of image_prep_lens_u8 (ivx_map_prep_lens): [n, ceil(pad_h / stride), ceil(pad_w / stride)]
    fp32, feature pixel (i, j) being input pixel (stride * i, stride * j) of the pipeline src_hw -> size_hw -> pad_hw (scene.pick_map's rule).
    src=None: the cover map, 1 where that input pixel shows the frame and 0 where it is border (pad, outside the frame, beyond r2_max); n
    copies; on `device` (None: the current HIP device).  src: device maps [n,H,W] at the source size src_hw, float32 or uint16 (a depth
    frame), rows dense: scale * the value at the nearest source pixel, 0 at border pixels (the lifts' "no measurement").  lens=None is the
    ideal camera, which takes depth frames through the plain pipeline.  out: a contiguous fp32 tensor of the result's shape to write into."""
    fn = _entry('ivx_map_prep_lens', *_LENS_ABI)
    ls = None if lens is None else _lens_struct(lens)
    (nh, nw), (ph, pw), (H, W) = (int(v) for v in size_hw), (int(v) for v in pad_hw), (int(v) for v in src_hw)
    if isinstance(stride, bool) or not isinstance(stride, int) or stride < 1:
        raise ValueError(f'stride must be an integer >= 1, got {stride!r}')
    row = plane = dt = 0
    if src is not None:
        if not isinstance(src, torch.Tensor):
            raise TypeError('src must be None or a torch.Tensor')
        if not src.is_cuda:
            raise RuntimeError('src must be a device (HIP) tensor; the MI355X path has no CPU fallback')
        if src.dtype not in _MAP_DT or src.dim() != 3 or tuple(src.shape[1:]) != (H, W):
            raise TypeError(f'src must be float32 or uint16 [n,{H},{W}] at the source size, got {src.dtype} {tuple(src.shape)}')
        n = int(src.shape[0])
        if n < 1:
            raise ValueError('src holds no map')
        dt, es = _MAP_DT[src.dtype]
        rs = src.stride(1) if H > 1 else W
        if (W > 1 and src.stride(2) != 1) or rs < W or (n > 1 and src.stride(0) < H * rs):
            raise ValueError(f'src rows must be dense (strides (>= H * row, >= W, 1)), got {tuple(src.stride())}')
        row, plane = rs * es, src.stride(0) * es
        device = src.device
    elif isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f'n must be an integer >= 1, got {n!r}')
    if min(ph, pw) < 1:
        raise ValueError(f'pad_hw must be positive, got {(ph, pw)}')
    shape = (n, (ph - 1) // stride + 1, (pw - 1) // stride + 1)
    if out is None and device is None:
        device = torch.device('cuda', torch.cuda.current_device())
    out = _prep_out(out, shape, device, where=src is not None)
    d = _prep_desc(H, W, 3 * W, (nh, nw), (ph, pw))
    check(fn(C.byref(d), None if ls is None else C.byref(ls), _ptr(src), dt, row, plane, float(scale), stride, n, _ptr(out), _stream()),
          'ivx_map_prep_lens')
    return out


def to_channels_last(x, pad_to=None):
    """[B,C,*spatial] (reference layout) -> [B,D,H,W,Cpad] channels-last (D=1 for 2-D input)."""
    _chk(x, 'x')
    B, Cn = x.shape[0], x.shape[1]
    sp = list(x.shape[2:])
    if len(sp) == 2:
        sp = [1] + sp
    S = sp[0] * sp[1] * sp[2]
    Cp = Cn if pad_to is None else ((Cn + pad_to - 1) // pad_to) * pad_to
    out = torch.empty([B] + sp + [Cp], device=x.device, dtype=torch.float32)
    check(_lib.lib().ivx_nchw_to_nhwc(_ptr(x), B, Cn, S, Cp, _ptr(out), _stream()), 'ivx_nchw_to_nhwc')
    return out


def from_channels_last(x, ndim_spatial=3):
    """[B,D,H,W,C] -> [B,C,D,H,W] (or [B,C,H,W] when ndim_spatial == 2); the reference layout is always fp32."""
    if x.dtype == torch.bfloat16:
        x = x.float()
    _chk(x, 'x')
    B, D, H, W, Cn = x.shape
    S = D * H * W
    shape = [B, Cn, D, H, W] if ndim_spatial == 3 else [B, Cn, H, W]
    if ndim_spatial == 2 and D != 1:
        raise ValueError('2-D output requested but D != 1')
    out = torch.empty(shape, device=x.device, dtype=torch.float32)
    check(_lib.lib().ivx_nhwc_to_nchw(_ptr(x), B, S, Cn, _ptr(out), _stream()), 'ivx_nhwc_to_nchw')
    return out


# ------------------------------------------------------------------ conv
def conv_fwd(x, wgt, scale=None, shift=None, kernel=(1, 1, 1), stride=(1, 1, 1), padding=(0, 0, 0), relu=False,
             res=None, res_mode=0, naive=False, out=None, wgt_layout=0, out_mode=0, res_after_act=False, post_scale=1.0,
             out_dtype=None, res_scale=1.0, pair=False):
    """x [B,D,H,W,Cin], wgt [Cout,KD,KH,KW,Cin] (packed), scale/shift [Cout] -> [B,Do,Ho,Wo,Cout].
    x and wgt are fp32 (the reference's precision), both bf16, or both e4m3 bytes (torch.float8_e4m3fn; the caller folds the
    tensors' scales into scale / shift / res_scale, see ivx_conv_desc); out_dtype (default: x.dtype) is the storage type of
    the output and of the residual.  Accumulation and the epilogue are fp32 in every case.
    pair=True: x and wgt are IVX_BF16_PAIR operands (bf16_pair_split / conv.pack_pair_weights: bf16 tensors with 2*Cin stored
    elements per voxel / tap); the output defaults to fp32."""
    if pair:
        if x.dtype != torch.bfloat16 or x.shape[4] % 32:
            raise TypeError('pair=True takes the bf16 tensor made by bf16_pair_split (2 * Cin elements per voxel, Cin % 16 == 0)')
        out_dtype = torch.float32 if out_dtype is None else out_dtype
    if x.dtype not in _DT:
        raise TypeError(f'x must be float32, bfloat16 or float8_e4m3fn, got {x.dtype}')
    out_dtype = x.dtype if out_dtype is None else out_dtype
    if out_dtype not in _DT:
        raise TypeError(f'out_dtype must be float32, bfloat16 or float8_e4m3fn, got {out_dtype}')
    _chk(x, 'x', x.dtype)
    _chk(wgt, 'wgt', x.dtype)
    B, D, H, W, Cin = x.shape
    Cout = wgt.shape[0]
    ck = {torch.float32: 32, torch.bfloat16: 64, FP8: 128}[x.dtype]
    want = (kernel[0], kernel[1], kernel[2], Cin) if wgt_layout == 0 else (Cin // ck, kernel[0], kernel[1], kernel[2], ck)
    if tuple(wgt.shape[1:]) != want:
        raise ValueError(f'weight shape {tuple(wgt.shape)} does not match kernel {kernel} / Cin {Cin} / layout {wgt_layout}')
    d = ConvDesc(B, D, H, W, Cin // 2 if pair else Cin, Cout, kernel[0], kernel[1], kernel[2], stride[0], stride[1], stride[2],
                 padding[0], padding[1], padding[2], int(bool(relu)), 0, 0, 0, int(wgt_layout), int(out_mode), int(bool(res_after_act)), float(post_scale),
                 IVX_BF16_PAIR if pair else _DT[x.dtype], _DT[out_dtype], float(res_scale))
    do, ho, wo = C.c_int32(), C.c_int32(), C.c_int32()
    L = _lib.lib()
    check(L.ivx_conv_out_dims(C.byref(d), C.byref(do), C.byref(ho), C.byref(wo)), 'ivx_conv_out_dims')
    oshape = (B, do.value, ho.value, wo.value, Cout)
    if out_mode == 1:
        oshape = (B, 2 * D, 2 * H, 2 * W, Cout // 8)
    if res is not None:
        _chk(res, 'res', out_dtype)
        if res_mode == 0:
            res_mode = 1
        if res_mode == 1 and tuple(res.shape) != oshape:
            raise ValueError(f'residual shape {tuple(res.shape)} != output shape')
        if res_mode == 2:
            if res.shape[0] != B or res.shape[1] != 1 or res.shape[4] != Cout:
                raise ValueError('res_mode 2 residual must be [B,1,h,w,Cout]')
            d.res_h, d.res_w = res.shape[2], res.shape[3]
        d.res_mode = res_mode
    for t, n in ((scale, 'scale'), (shift, 'shift')):
        if t is not None:
            _chk(t, n)
            if t.numel() != oshape[-1]:
                raise ValueError(f'{n} must have {oshape[-1]} elements')
    if out is None:
        out = torch.empty(oshape, device=x.device, dtype=out_dtype)
    else:
        _chk(out, 'out', out_dtype)
    if naive:
        check(L.ivx_conv_fwd_naive(C.byref(d), _ptr(x), _ptr(wgt), _ptr(scale), _ptr(shift), _ptr(res), _ptr(out), _stream()),
              'ivx_conv_fwd_naive')
        return out
    wsb = L.ivx_conv_workspace_bytes(C.byref(d))
    ws = torch.empty((wsb,), device=x.device, dtype=torch.uint8) if wsb > 0 else None
    check(L.ivx_conv_fwd_ws(C.byref(d), _ptr(x), _ptr(wgt), _ptr(scale), _ptr(shift), _ptr(res), _ptr(out), _ptr(ws), max(wsb, 0),
                            _stream()), 'ivx_conv_fwd_ws')
    return out


IVX_BF16_PAIR = 3


def bf16_pair_split(x, out=None):
    """fp32 [..., C] (C % 16 == 0, contiguous) -> the IVX_BF16_PAIR operand: bf16 [..., 2C], per 16 channels [hi x16 | lo x16] with
    hi = bf16(x), lo = bf16(x - hi)  (ivx_bf16_pair_split)."""
    _chk(x, 'x')
    if x.shape[-1] % 16:
        raise ValueError('the channel count must be a multiple of 16')
    if out is None:
        out = torch.empty(x.shape[:-1] + (2 * x.shape[-1],), device=x.device, dtype=torch.bfloat16)
    else:
        _chk(out, 'out', torch.bfloat16)
    check(_lib.lib().ivx_bf16_pair_split(_ptr(x), x.numel(), _ptr(out), _stream()), 'ivx_bf16_pair_split')
    return out


def conv_pair_supported(x_shape, Cout, kernel, stride, padding, wgt_layout=1):
    """True when the fp32 convolution can run in the split-operand (bf16 pair) form: ivx_conv_pair_supported."""
    B, D, H, W, Cin = x_shape
    d = ConvDesc(B, D, H, W, Cin, Cout, kernel[0], kernel[1], kernel[2], stride[0], stride[1], stride[2], padding[0], padding[1], padding[2],
                 0, 0, 0, 0, int(wgt_layout), 0, 0, 1.0, 0, 0, 1.0)
    return bool(_lib.lib().ivx_conv_pair_supported(C.byref(d)))


IVX_F16_PAIR = 4


def _wino_desc(B, D, H, W, Cin, Cout, kw, stride_w, padding, relu, wgt_layout, res_mode=0, res_after_act=False, post_scale=1.0, operands=0):
    return ConvDesc(B, D, H, W, Cin, Cout, 3, 3, kw, 1, 1, stride_w, padding[0], padding[1], padding[2], int(bool(relu)),
                    int(res_mode), 0, 0, int(wgt_layout), 0, int(bool(res_after_act)), float(post_scale), 0, 0, 1.0, int(operands))


def conv_winograd_supported(x_shape, Cout, kernel, stride, padding, tile=2, operands=0):
    """True when ivx_conv_winograd_fwd can run this fp32 convolution (3x3xKW, stride 1 on the first two axes, planes < 2 GiB)."""
    if kernel[0] != 3 or kernel[1] != 3 or stride[0] != 1 or stride[1] != 1 or x_shape[4] % 4 or Cout % 4 or tile not in (2, 4, 6):
        return False
    B, D, H, W, Cin = x_shape
    d = _wino_desc(B, D, H, W, Cin, Cout, kernel[2], stride[2], padding, False, 0, operands=operands)
    return bool(_lib.lib().ivx_conv_winograd_supported(C.byref(d), tile))


def conv_winograd_weights(wgt, wgt_layout, tile=2, operands=0):
    """wgt [Cout,3,3,KW,Cin] fp32 (layout 0, on the device) -> transformed filters u [(tile+2)^2, Cout, KW*Cin] whose K order
    is `wgt_layout` (0: tap-major, 1: 32-channel chunks).  operands = IVX_F16_PAIR: the same bytes hold fp16 (hi, lo) pairs
    (ivx_conv_desc.wino_operands); pass the same value to conv_winograd_fwd."""
    _chk(wgt, 'wgt')
    Cout, kd, kh, kw, Cin = wgt.shape
    if kd != 3 or kh != 3:
        raise ValueError('Winograd F(m x m, 3x3) needs a 3x3 kernel on the first two axes')
    d = _wino_desc(1, 4, 4, max(kw, 1), Cin, Cout, kw, 1, (1, 1, kw // 2), False, wgt_layout, operands=operands)
    L = _lib.lib()
    n = L.ivx_conv_winograd_weight_elems(C.byref(d), tile)
    if n < 0:
        check(-1, 'ivx_conv_winograd_weight_elems')
    # pair operands: one more plane (it carries the filter scale); the same bytes then hold fp16 pairs
    u = torch.empty(((tile + 2) ** 2 + (1 if operands else 0), Cout, kw * Cin), device=wgt.device, dtype=torch.float32)
    assert u.numel() == n
    check(L.ivx_conv_winograd_weights(C.byref(d), tile, _ptr(wgt), _ptr(u), _stream()), 'ivx_conv_winograd_weights')
    return u


# optional stage timing of the Winograd path (bench.py): list of (stage, start_event, end_event, executed_flops)
winograd_trace = None


def winograd_bg_plan(valid, x_shape, Cout, out_slices, wgt_layout=1, operands=IVX_F16_PAIR):
    """Background plan of a chain of F(6x6,3x3) layers that starts at the unprojection's output (ivx_conv_winograd_bg_plan): valid
    [B,X,Y,Z] uint8 / bool, x_shape the volume's [B,X,Y,Z,C], out_slices the output z extent of every layer.  Returns (block, views):
    the device block (uint8) and per layer its int32 view {slots, GEMM rows, image-dependent tiles, keys, list[B TX TY], src[B TX TY]},
    to be handed to conv_winograd_fwd(bg=...)."""
    B, X, Y, Z, Cin = x_shape
    if tuple(valid.shape) != (B, X, Y, Z) or not valid.is_cuda or not valid.is_contiguous() or valid.element_size() != 1:
        raise ValueError('valid must be a contiguous [B,X,Y,Z] one-byte device tensor')
    d = _wino_desc(B, X, Y, Z, Cin, Cout, 3, 1, (1, 1, 1), False, wgt_layout, operands=operands)
    L = _lib.lib()
    nl = len(out_slices)
    nb = L.ivx_conv_winograd_bg_bytes(C.byref(d), nl)
    if nb < 0:
        check(-1, 'ivx_conv_winograd_bg_bytes')
    block = torch.zeros((nb,), device=valid.device, dtype=torch.uint8)
    zo = (C.c_int32 * nl)(*[int(z) for z in out_slices])
    check(L.ivx_conv_winograd_bg_plan(C.byref(d), _ptr(valid), nl, zo, _ptr(block), nb, _stream()), 'ivx_conv_winograd_bg_plan')
    n = B * ((X + 5) // 6) * ((Y + 5) // 6)
    views = []
    for l in range(nl):
        off = L.ivx_conv_winograd_bg_layer_offset(C.byref(d), l)
        views.append(block[off:off + 4 * (4 + 2 * n)].view(torch.int32))
    return block, views


def conv_winograd_fwd(x, u, scale=None, shift=None, kw=3, stride_w=1, padding=(1, 1, 1), relu=False, res=None, out=None,
                      wgt_layout=0, res_after_act=False, post_scale=1.0, operands=0, amax_in=None, want_amax=False, fused=False, bg=None):
    """Same result as conv_fwd for a 3x3xkw kernel with stride (1,1,stride_w), computed in the F(m x m, 3x3) minimal-filtering
    form (fp32).  x [B,D,H,W,Cin]; u from conv_winograd_weights (its first dimension, 16 / 36 / 64, selects m = 2 / 4 / 6)."""
    _chk(x, 'x')
    _chk(u, 'u')
    B, D, H, W, Cin = x.shape
    Cout = u.shape[1]
    tile = {16: 2, 36: 4, 64: 6}.get(u.shape[0] - (1 if operands else 0))
    if tile is None or tuple(u.shape[1:]) != (Cout, kw * Cin):
        raise ValueError(f'transformed filters {tuple(u.shape)} do not match kw {kw} / Cin {Cin}')
    d = _wino_desc(B, D, H, W, Cin, Cout, kw, stride_w, padding, relu, wgt_layout, 1 if res is not None else 0, res_after_act,
                   post_scale, operands)
    do, ho, wo = C.c_int32(), C.c_int32(), C.c_int32()
    L = _lib.lib()
    check(L.ivx_conv_out_dims(C.byref(d), C.byref(do), C.byref(ho), C.byref(wo)), 'ivx_conv_out_dims')
    oshape = (B, do.value, ho.value, wo.value, Cout)
    if res is not None:
        _chk(res, 'res')
        if tuple(res.shape) != oshape:
            raise ValueError(f'residual shape {tuple(res.shape)} != output shape')
    for t, n in ((scale, 'scale'), (shift, 'shift')):
        if t is not None:
            _chk(t, n)
            if t.numel() != Cout:
                raise ValueError(f'{n} must have {Cout} elements')
    if out is None:
        out = torch.empty(oshape, device=x.device, dtype=torch.float32)
    else:
        _chk(out, 'out')
    wsb = L.ivx_conv_winograd_workspace_bytes(C.byref(d), tile)
    if wsb < 0:
        check(-1, 'ivx_conv_winograd_workspace_bytes')
    ws = torch.empty((wsb,), device=x.device, dtype=torch.uint8)
    if fused:
        # F(4x4,3x3) pair operands: GEMM + output transform in one launch, M on chip (ivx_conv_winograd_gemm_output_amax)
        if not L.ivx_conv_winograd_fused_supported(C.byref(d), tile):
            raise ValueError('this layer does not take the fused GEMM + output form (ivx_conv_winograd_fused_supported)')
        part = None
        if want_amax:
            part = torch.empty((L.ivx_conv_winograd_fused_blocks(C.byref(d), tile),), device=x.device, dtype=torch.float32)
        if amax_in is not None:
            _chk(amax_in, 'amax_in')
        check(L.ivx_conv_winograd_input_amax(C.byref(d), tile, _ptr(x), _ptr(ws), wsb, _ptr(amax_in), 0 if amax_in is None else amax_in.numel(),
                                             _stream()), 'ivx_conv_winograd_input_amax')
        check(L.ivx_conv_winograd_gemm_output_amax(C.byref(d), tile, _ptr(u), _ptr(scale), _ptr(shift), _ptr(res), _ptr(out), _ptr(ws), wsb, _ptr(part),
                                                   _stream()), 'ivx_conv_winograd_gemm_output_amax')
        return (out, part) if want_amax else out
    if bg is not None:
        # a layer of a background chain (winograd_bg_plan): the three stages over the plan's slots; partial maxima as in the chained form
        if not L.ivx_conv_winograd_bg_supported(C.byref(d), tile):
            raise ValueError('this layer does not take the background form (ivx_conv_winograd_bg_supported)')
        part = None
        if want_amax:
            part = torch.empty((L.ivx_conv_winograd_output_blocks(C.byref(d), tile),), device=x.device, dtype=torch.float32)
        if amax_in is not None:
            _chk(amax_in, 'amax_in')
        check(L.ivx_conv_winograd_input_bg(C.byref(d), tile, _ptr(x), _ptr(ws), wsb, _ptr(amax_in), 0 if amax_in is None else amax_in.numel(),
                                           _ptr(bg), _stream()), 'ivx_conv_winograd_input_bg')
        check(L.ivx_conv_winograd_gemm_bg(C.byref(d), tile, _ptr(u), _ptr(ws), wsb, _ptr(bg), _stream()), 'ivx_conv_winograd_gemm_bg')
        check(L.ivx_conv_winograd_output_bg(C.byref(d), tile, _ptr(scale), _ptr(shift), _ptr(res), _ptr(out), _ptr(ws), wsb, _ptr(part),
                                            _ptr(bg), _stream()), 'ivx_conv_winograd_output_bg')
        return (out, part) if want_amax else out
    if amax_in is not None or want_amax:
        # chained layers (ivx_conv_winograd_output_amax / _input_amax): amax_in = the producer's per-workgroup maxima of x;
        # want_amax: also return this layer's own -> (out, partials)
        part = None
        if want_amax:
            nb = L.ivx_conv_winograd_output_blocks(C.byref(d), tile)
            if nb < 0:
                check(-1, 'ivx_conv_winograd_output_blocks')
            part = torch.empty((nb,), device=x.device, dtype=torch.float32)
        if amax_in is not None:
            _chk(amax_in, 'amax_in')
        check(L.ivx_conv_winograd_input_amax(C.byref(d), tile, _ptr(x), _ptr(ws), wsb, _ptr(amax_in), 0 if amax_in is None else amax_in.numel(),
                                             _stream()), 'ivx_conv_winograd_input_amax')
        check(L.ivx_conv_winograd_gemm(C.byref(d), tile, _ptr(u), _ptr(ws), wsb, _stream()), 'ivx_conv_winograd_gemm')
        check(L.ivx_conv_winograd_output_amax(C.byref(d), tile, _ptr(scale), _ptr(shift), _ptr(res), _ptr(out), _ptr(ws), wsb, _ptr(part),
                                              _stream()), 'ivx_conv_winograd_output_amax')
        return (out, part) if want_amax else out
    if winograd_trace is None:
        check(L.ivx_conv_winograd_fwd(C.byref(d), tile, _ptr(x), _ptr(u), _ptr(scale), _ptr(shift), _ptr(res), _ptr(out), _ptr(ws),
                                      wsb, _stream()), 'ivx_conv_winograd_fwd')
        return out
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record()
    check(L.ivx_conv_winograd_input(C.byref(d), tile, _ptr(x), _ptr(ws), wsb, _stream()), 'ivx_conv_winograd_input')
    ev[1].record()
    check(L.ivx_conv_winograd_gemm(C.byref(d), tile, _ptr(u), _ptr(ws), wsb, _stream()), 'ivx_conv_winograd_gemm')
    ev[2].record()
    check(L.ivx_conv_winograd_output(C.byref(d), tile, _ptr(scale), _ptr(shift), _ptr(res), _ptr(out), _ptr(ws), wsb, _stream()),
          'ivx_conv_winograd_output')
    ev[3].record()
    tiles = B * ((oshape[1] + tile - 1) // tile) * ((oshape[2] + tile - 1) // tile)
    winograd_trace.append(('input', ev[0], ev[1], 0.0))
    frac = float(L.ivx_conv_winograd_issued_fraction(C.byref(d)))      # the z-blocked tile skips the taps outside a 3-slice column
    winograd_trace.append(('gemm', ev[1], ev[2], (3.0 if operands else 1.0) * frac * 2.0 * (tile + 2) ** 2 * tiles * oshape[3] * Cout * kw * Cin))
    winograd_trace.append(('output', ev[2], ev[3], 0.0))
    return out


class WinogradLayerPlan:
    """One fp32 3x3xkw layer in the F(m x m, 3x3) form for a fixed input shape: descriptor, output shape and workspace
    size, with the three stages as separate calls on caller-owned buffers (tools/gemm_ab.py times them one by one)."""

    def __init__(self, x_shape, Cout, kw, stride_w, padding, relu, wgt_layout, tile, has_res=False, res_after_act=False,
                 post_scale=1.0, operands=0):
        B, D, H, W, Cin = x_shape
        self.tile = int(tile)
        self.d = _wino_desc(B, D, H, W, Cin, Cout, kw, stride_w, padding, relu, wgt_layout, 1 if has_res else 0, res_after_act,
                            post_scale, operands)
        do, ho, wo = C.c_int32(), C.c_int32(), C.c_int32()
        L = _lib.lib()
        check(L.ivx_conv_out_dims(C.byref(self.d), C.byref(do), C.byref(ho), C.byref(wo)), 'ivx_conv_out_dims')
        self.x_shape = tuple(x_shape)
        self.oshape = (B, do.value, ho.value, wo.value, Cout)
        self.ws_bytes = L.ivx_conv_winograd_workspace_bytes(C.byref(self.d), self.tile)
        if self.ws_bytes < 0:
            check(-1, 'ivx_conv_winograd_workspace_bytes')
        n2 = (self.tile + 2) ** 2
        tiles = B * ((self.oshape[1] + tile - 1) // tile) * ((self.oshape[2] + tile - 1) // tile)
        self.gemm_flops = 2.0 * n2 * tiles * self.oshape[3] * Cout * kw * Cin
        self.v_bytes = 4.0 * n2 * tiles * W * Cin
        self.m_bytes = 4.0 * n2 * tiles * self.oshape[3] * Cout

    def input(self, x, ws):
        check(_lib.lib().ivx_conv_winograd_input(C.byref(self.d), self.tile, _ptr(x), _ptr(ws), ws.numel(), _stream()),
              'ivx_conv_winograd_input')

    def gemm(self, u, ws):
        check(_lib.lib().ivx_conv_winograd_gemm(C.byref(self.d), self.tile, _ptr(u), _ptr(ws), ws.numel(), _stream()),
              'ivx_conv_winograd_gemm')

    def output(self, scale, shift, res, out, ws):
        check(_lib.lib().ivx_conv_winograd_output(C.byref(self.d), self.tile, _ptr(scale), _ptr(shift), _ptr(res), _ptr(out), _ptr(ws),
                                                  ws.numel(), _stream()), 'ivx_conv_winograd_output')


def maxpool2d(x, k=3, s=2, p=1):
    if x.dtype not in _DT:
        raise TypeError(f'x must be float32, bfloat16 or float8_e4m3fn, got {x.dtype}')
    _chk(x, 'x', x.dtype)
    B, D, H, W, Cn = x.shape
    if D != 1:
        raise ValueError('maxpool2d expects a 2-D map (D == 1)')
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    out = torch.empty((B, 1, Ho, Wo, Cn), device=x.device, dtype=x.dtype)
    L = _lib.lib()
    fn = {torch.float32: L.ivx_maxpool2d_fwd, torch.bfloat16: L.ivx_maxpool2d_fwd_bf16, FP8: L.ivx_maxpool2d_fwd_fp8}[x.dtype]
    check(fn(_ptr(x), B, H, W, Cn, k, s, p, _ptr(out), _stream()), 'ivx_maxpool2d_fwd')
    return out


# ------------------------------------------------------------------ chained fp16-pair activations (include/imvoxel.h, ivx_pair_io)
AMAX_SLOTS = 64


def new_slots(device):
    """Scalar block of one tensor of a pair chain: AMAX_SLOTS words of max |tensor| (float bits, accumulated by the producing kernel
    with atomic max: they start at zero) followed by the tensor's power-of-two scale."""
    return torch.zeros(AMAX_SLOTS + 16, device=device, dtype=torch.int32)


def _scale_ptr(slots):
    return C.c_void_p(slots.data_ptr() + 4 * AMAX_SLOTS)


class PairTensor:
    """An IVX_F16_PAIR activation: data = float16 [B,D,H,W,2C] (per 16 channels [hi x16 | lo x16]) of s * x, with the scalar block
    (amax slots, scale s) its producer filled on the device.  `shape` is the logical fp32 shape [B,D,H,W,C]."""
    __slots__ = ('data', 'slots')

    def __init__(self, data, slots):
        self.data, self.slots = data, slots

    shape = property(lambda self: tuple(self.data.shape[:4]) + (self.data.shape[4] // 2,))
    device = property(lambda self: self.data.device)
    dtype = property(lambda self: torch.float32)       # what the values are; the storage is fp16 pairs

    def numel(self):
        return self.data.numel() // 2

    def element_size(self):
        return 4

    def float(self):
        """fp32 values (hi + lo) / s (ivx_f16_pair_merge)."""
        out = torch.empty(self.shape, device=self.data.device, dtype=torch.float32)
        check(_lib.lib().ivx_f16_pair_merge(_ptr(self.data), out.numel(), _scale_ptr(self.slots), _ptr(out), _stream()), 'ivx_f16_pair_merge')
        return out

    def amax(self):
        """max |x| as the producer recorded it (host float; synchronises)."""
        return float(self.slots[:AMAX_SLOTS].view(torch.float32).max())

    def scale(self):
        return float(self.slots[AMAX_SLOTS:AMAX_SLOTS + 1].view(torch.float32)[0])


def pair_from_float(x):
    """fp32 device tensor [.., C] (C % 16 == 0) -> PairTensor, scaled by its exact maximum (one pass over the tensor + a host sync:
    for tools and tests; inside the model the producing kernels write pairs)."""
    import math
    _chk(x, 'x')
    amax = float(x.abs().max())
    s = 1.0
    if 0.0 < amax < 3e38:
        s = 2.0 ** (15 - math.frexp(amax)[1])
    data = torch.empty(tuple(x.shape[:-1]) + (2 * x.shape[-1],), device=x.device, dtype=torch.float16)
    check(_lib.lib().ivx_f16_pair_split(_ptr(x), x.numel(), C.c_float(s), _ptr(data), _stream()), 'ivx_f16_pair_split')
    slots = new_slots(x.device)
    slots[:1].view(torch.float32)[0] = amax
    slots[AMAX_SLOTS:AMAX_SLOTS + 1].view(torch.float32)[0] = s
    return PairTensor(data, slots)


def slots_of(t):
    """The scalar block a tensor of the chain carries (a PairTensor's, or the one attached to an fp32 tensor by its producer), or None."""
    return t.slots if isinstance(t, PairTensor) else getattr(t, 'ivx_slots', None)


def to_channels_last_amax(x, pad_to=None):
    """to_channels_last that also records max |x| in a scalar block attached to the result (out.ivx_slots): ivx_nchw_to_nhwc_amax."""
    _chk(x, 'x')
    B, Cn = x.shape[0], x.shape[1]
    sp = list(x.shape[2:])
    if len(sp) == 2:
        sp = [1] + sp
    S = sp[0] * sp[1] * sp[2]
    Cp = Cn if pad_to is None else ((Cn + pad_to - 1) // pad_to) * pad_to
    out = torch.empty([B] + sp + [Cp], device=x.device, dtype=torch.float32)
    slots = new_slots(x.device)
    check(_lib.lib().ivx_nchw_to_nhwc_amax(_ptr(x), B, Cn, S, Cp, _ptr(out), _ptr(slots), _stream()), 'ivx_nchw_to_nhwc_amax')
    out.ivx_slots = slots
    return out


def maxpool2d_pair(x, amax_in, wbound, sbound, k=3, s=2, p=1):
    """nn.MaxPool2d on an fp32 map -> PairTensor scaled by the bound amax_in * wbound + sbound of the input map (ivx_maxpool2d_fwd_pair);
    amax_in: the scalar block of the tensor the bound refers to (the image)."""
    _chk(x, 'x')
    B, D, H, W, Cn = x.shape
    if D != 1 or Cn % 16:
        raise ValueError('maxpool2d_pair expects a 2-D map with C % 16 == 0')
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    out = torch.empty((B, 1, Ho, Wo, 2 * Cn), device=x.device, dtype=torch.float16)
    slots = new_slots(x.device)
    check(_lib.lib().ivx_maxpool2d_fwd_pair(_ptr(x), B, H, W, Cn, k, s, p, _ptr(out), _ptr(amax_in), float(wbound), float(sbound),
                                            _scale_ptr(slots), _ptr(slots), _stream()), 'ivx_maxpool2d_fwd_pair')
    return PairTensor(out, slots)


def pair_pack_filters(w_tap, scale, shift, pack=True):
    """Host: fp32 filters [Cout, taps, Cin] (tap-major, CPU) + the epilogue vectors -> (pair filters float16 [Cout, Cin/32, taps, 64] or None,
    scale / s_w [Cout] or None, wbound, sbound) through ivx_pair_pack_filters (the native handle packs with the same function)."""
    w_tap = w_tap.detach().to(torch.float32).cpu().contiguous()
    co, taps, ci = w_tap.shape
    sc = None if scale is None else scale.detach().to(torch.float32).cpu().contiguous()
    sf = None if shift is None else shift.detach().to(torch.float32).cpu().contiguous()
    packed = torch.empty((co, ci // 32, taps, 64), dtype=torch.float16) if pack else None
    sp = torch.empty(co, dtype=torch.float32) if pack else None
    wb, sb = C.c_float(), C.c_float()
    check(_lib.lib().ivx_pair_pack_filters(_ptr_any(w_tap), co, taps, ci, _ptr_any(sc), _ptr_any(sf), _ptr_any(packed), _ptr_any(sp), C.byref(wb),
                                           C.byref(sb)), 'ivx_pair_pack_filters')
    return packed, sp, wb.value, sb.value


def _ptr_any(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def conv_fwd_pio(x, wgt, scale, shift, kernel, stride, padding, relu, wbound, sbound, res=None, res_mode=0, out_pair=False,
                 res_after_act=False, post_scale=1.0, naive=False):
    """Convolution on a PairTensor (ivx_conv_fwd_pio): wgt = pair filters of pair_pack_filters (device), scale = scale / s_w.
    res: None, an fp32 tensor or a PairTensor.  Returns a PairTensor (out_pair) or an fp32 tensor; either carries the scalar block with
    max |out| (result.slots / result.ivx_slots)."""
    if not isinstance(x, PairTensor):
        raise TypeError('conv_fwd_pio takes a PairTensor')
    _chk(x.data, 'x', torch.float16)
    _chk(wgt, 'wgt', torch.float16)
    B, D, H, W, Cin = x.shape
    Cout = wgt.shape[0]
    if tuple(wgt.shape[1:]) != (Cin // 32, kernel[0] * kernel[1] * kernel[2], 64):
        raise ValueError(f'pair filters {tuple(wgt.shape)} do not match kernel {kernel} / Cin {Cin}')
    d = ConvDesc(B, D, H, W, Cin, Cout, kernel[0], kernel[1], kernel[2], stride[0], stride[1], stride[2], padding[0], padding[1], padding[2],
                 int(bool(relu)), 0, 0, 0, 1, 0, int(bool(res_after_act)), float(post_scale), IVX_F16_PAIR, IVX_F16_PAIR if out_pair else 0, 1.0)
    do, ho, wo = C.c_int32(), C.c_int32(), C.c_int32()
    L = _lib.lib()
    check(L.ivx_conv_out_dims(C.byref(d), C.byref(do), C.byref(ho), C.byref(wo)), 'ivx_conv_out_dims')
    oshape = (B, do.value, ho.value, wo.value, Cout)
    out_pair = bool(out_pair) and Cout % 16 == 0 and B * do.value * ho.value * wo.value * Cout * 4 < 2 ** 31     # (as csrc/model.cpp wants_pair)
    io = _lib.PairIO()
    io.in_scale = _scale_ptr(x.slots)
    io.amax_in = _ptr(x.slots)
    rd = None
    if res is not None:
        res_mode = res_mode or 1
        rshape = tuple(res.shape)
        if res_mode == 1 and rshape != oshape:
            raise ValueError(f'residual shape {rshape} != output shape')
        if res_mode == 2:
            if rshape[0] != B or rshape[1] != 1 or rshape[4] != Cout:
                raise ValueError('res_mode 2 residual must be [B,1,h,w,Cout]')
            d.res_h, d.res_w = rshape[2], rshape[3]
        d.res_mode = res_mode
        if isinstance(res, PairTensor):
            rd = _chk(res.data, 'res', torch.float16)
            io.res_dtype, io.res_scale = IVX_F16_PAIR, _scale_ptr(res.slots)
        else:
            rd = _chk(res, 'res')
        rs = slots_of(res)
        io.amax_res = _ptr(rs)
        if out_pair and rs is None:
            raise ValueError('a pair output needs the scalar block (max |res|) of its residual')
    for t, n in ((scale, 'scale'), (shift, 'shift')):
        if t is not None:
            _chk(t, n)
            if t.numel() != Cout:
                raise ValueError(f'{n} must have {Cout} elements')
    slots = new_slots(x.device)
    io.amax_out = _ptr(slots)
    io.out_scale = _scale_ptr(slots)
    io.wbound, io.sbound = float(wbound), float(sbound)
    if out_pair:
        out = torch.empty(oshape[:4] + (2 * Cout,), device=x.device, dtype=torch.float16)
    else:
        out = torch.empty(oshape, device=x.device, dtype=torch.float32)
    if naive:
        check(L.ivx_conv_fwd_pio_naive(C.byref(d), C.byref(io), _ptr(x.data), _ptr(wgt), _ptr(scale), _ptr(shift), _ptr(rd), _ptr(out), _stream()),
              'ivx_conv_fwd_pio_naive')
    else:
        wsb = L.ivx_conv_pio_workspace_bytes(C.byref(d), C.byref(io))
        if wsb < 0:
            check(-1, 'ivx_conv_pio_workspace_bytes')
        ws = torch.empty((wsb,), device=x.device, dtype=torch.uint8) if wsb > 0 else None
        check(L.ivx_conv_fwd_pio(C.byref(d), C.byref(io), _ptr(x.data), _ptr(wgt), _ptr(scale), _ptr(shift), _ptr(rd), _ptr(out), _ptr(ws),
                                 max(wsb, 0), _stream()), 'ivx_conv_fwd_pio')
    if out_pair:
        return PairTensor(out, slots)
    out.ivx_slots = slots
    return out


def stem_pool_pack_filters(w, scale):
    """Host: [64,3,7,7] stem filters + BN scale [64] (CPU tensors) -> (fragment-ordered pair filters as a uint8 tensor, scale / s_w [64]) through
    ivx_stem_pool_pack_filters (the native handle packs with the same function)."""
    w = w.detach().to(torch.float32).cpu().contiguous()
    if tuple(w.shape) != (64, 3, 7, 7):
        raise ValueError('the one-launch stem is built for [64, 3, 7, 7] filters')
    sc = scale.detach().to(torch.float32).cpu().contiguous()
    L = _lib.lib()
    packed = torch.empty(int(L.ivx_stem_pool_filter_bytes()), dtype=torch.uint8)
    sp = torch.empty(64, dtype=torch.float32)
    check(L.ivx_stem_pool_pack_filters(_ptr_any(w), _ptr_any(sc), _ptr_any(packed), _ptr_any(sp)), 'ivx_stem_pool_pack_filters')
    return packed, sp


def stem_pool_pair(img, wfrag, scale_p, shift, wbound, sbound):
    """fp32 NCHW image [N,3,H,W] -> PairTensor [N,1,Hp,Wp,64]: conv 7x7 s2 p3 + BN + ReLU + MaxPool2d(3,2,1) in one launch (ivx_amax_f32 +
    ivx_stem_pool_fwd_pair, csrc/stem.hip).  wfrag / scale_p: device copies of stem_pool_pack_filters' outputs."""
    _chk(img, 'img')
    N, Cn, H, W = img.shape
    if Cn != 3:
        raise ValueError('stem_pool_pair takes a 3-channel image')
    L = _lib.lib()
    hp, wp = C.c_int32(), C.c_int32()
    check(L.ivx_stem_pool_out_dims(H, W, C.byref(hp), C.byref(wp)), 'ivx_stem_pool_out_dims')
    islots, slots = new_slots(img.device), new_slots(img.device)
    check(L.ivx_amax_f32(_ptr(img), img.numel(), _ptr(islots), _stream()), 'ivx_amax_f32')
    out = torch.empty((N, 1, hp.value, wp.value, 128), device=img.device, dtype=torch.float16)
    check(L.ivx_stem_pool_fwd_pair(_ptr(img), N, H, W, _ptr(wfrag), _ptr(scale_p), _ptr(shift), float(wbound), float(sbound), _ptr(islots), _ptr(out),
                                   _scale_ptr(slots), _ptr(slots), _stream()), 'ivx_stem_pool_fwd_pair')
    return PairTensor(out, slots)


def bottleneck_supported(B, H, W, planes):
    """ivx_bottleneck_supported: the one-launch form of an identity bottleneck exists for this map (csrc/bottleneck.hip)."""
    d = _lib.BottleneckDesc(int(B), int(H), int(W), int(planes))
    return bool(_lib.lib().ivx_bottleneck_supported(C.byref(d)))


def bottleneck_fwd_pio(x, f1, f2, f3):
    """One identity bottleneck (1x1 -> 3x3 -> 1x1 + shortcut, every BN / ReLU) in one launch on a PairTensor [B,1,H,W,4P] (ivx_bottleneck_fwd_pio).
    f1 / f2 / f3: the block's three layers, objects with wpair, scale_p, shift, wbound, sbound (conv.FusedConv(chain=True)).  -> PairTensor."""
    if not isinstance(x, PairTensor):
        raise TypeError('bottleneck_fwd_pio takes a PairTensor')
    _chk(x.data, 'x', torch.float16)
    B, D, H, W, Cn = x.shape
    P = Cn // 4
    if D != 1 or not bottleneck_supported(B, H, W, P) or Cn != 4 * P:
        raise ValueError(f'no fused bottleneck for an input of shape {x.shape}')
    want = ((P, Cn // 32, 1, 64), (P, P // 32, 9, 64), (Cn, P // 32, 1, 64))
    for f, shp in zip((f1, f2, f3), want):
        _chk(f.wpair, 'wpair', torch.float16)
        if tuple(f.wpair.shape) != shp:
            raise ValueError(f'pair filters {tuple(f.wpair.shape)} do not match the bottleneck ({shp})')
        _chk(f.scale_p, 'scale_p')
        _chk(f.shift, 'shift')
    d = _lib.BottleneckDesc(B, H, W, P)
    io = _lib.BottleneckIO()
    slots = new_slots(x.device)
    io.in_scale, io.amax_in = _scale_ptr(x.slots), _ptr(x.slots)
    io.out_scale, io.amax_out = _scale_ptr(slots), _ptr(slots)
    for i, f in enumerate((f1, f2, f3)):
        io.wbound[i], io.sbound[i] = float(f.wbound), float(f.sbound)
    out = torch.empty_like(x.data)
    check(_lib.lib().ivx_bottleneck_fwd_pio(C.byref(d), C.byref(io), _ptr(x.data), _ptr(f1.wpair), _ptr(f1.scale_p), _ptr(f1.shift), _ptr(f2.wpair),
                                            _ptr(f2.scale_p), _ptr(f2.shift), _ptr(f3.wpair), _ptr(f3.scale_p), _ptr(f3.shift), _ptr(out), _stream()),
          'ivx_bottleneck_fwd_pio')
    return PairTensor(out, slots)


def bottleneck_proj_supported(B, H, W, planes, cin):
    """ivx_bottleneck_proj_supported: the one-launch form of a stage's first block (shortcut conv, stride 1) exists for this map."""
    d = _lib.BottleneckDesc(int(B), int(H), int(W), int(planes))
    return bool(_lib.lib().ivx_bottleneck_proj_supported(C.byref(d), int(cin)))


class ProjBank:
    """the joint pair filter bank of conv3 and the shortcut conv (ivx_bottleneck_proj_pack) + its epilogue vectors and bound terms"""

    def __init__(self, f3, fd):
        P, cin = f3.cin, fd.cin
        if f3._w_tap_host is None or fd._w_tap_host is None or f3.cout != 4 * P or fd.cout != 4 * P:
            raise ValueError('bottleneck_proj_pack takes the 1x1 conv3 (P -> 4P) and the 1x1 shortcut conv (Cin -> 4P) of one block, built with chain=True')
        self.planes, self.cin = P, cin
        packed = torch.empty((4 * P, (cin + P) // 32, 1, 64), dtype=torch.float16)
        sc, sf = torch.empty(4 * P, dtype=torch.float32), torch.empty(4 * P, dtype=torch.float32)
        wb3, sb, wbd = C.c_float(), C.c_float(), C.c_float()
        check(_lib.lib().ivx_bottleneck_proj_pack(_ptr_any(f3._w_tap_host), _ptr_any(f3._scale_host), _ptr_any(f3._shift_host), _ptr_any(fd._w_tap_host),
                                                  _ptr_any(fd._scale_host), _ptr_any(fd._shift_host), P, cin, _ptr_any(packed), _ptr_any(sc), _ptr_any(sf),
                                                  C.byref(wb3), C.byref(sb), C.byref(wbd)), 'ivx_bottleneck_proj_pack')
        self._host = (packed, sc, sf)
        self.wbound3, self.sbound, self.wboundd = wb3.value, sb.value, wbd.value
        self.wpair = self.scale_p = self.shift = None

    def to(self, device):
        self.wpair, self.scale_p, self.shift = (t.to(device) for t in self._host)
        return self


def bottleneck_proj_fwd_pio(x, f1, f2, bank):
    """The first block of ResNet stage 1 (1x1 -> 3x3 -> 1x1 + the 1x1 shortcut conv of the input, every BN / ReLU) in one launch on a PairTensor
    [B,1,H,W,Cin] (ivx_bottleneck_proj_fwd_pio).  f1 / f2: conv.FusedConv(chain=True) of conv1 / conv2, bank: ProjBank(conv3, shortcut conv).to(device)
    -> PairTensor [B,1,H,W,4P]."""
    if not isinstance(x, PairTensor):
        raise TypeError('bottleneck_proj_fwd_pio takes a PairTensor')
    _chk(x.data, 'x', torch.float16)
    B, D, H, W, Cn = x.shape
    P = bank.planes
    if D != 1 or Cn != bank.cin or not bottleneck_proj_supported(B, H, W, P, Cn):
        raise ValueError(f'no fused projection bottleneck for an input of shape {x.shape} (planes {P})')
    want = ((P, Cn // 32, 1, 64), (P, P // 32, 9, 64), (4 * P, (Cn + P) // 32, 1, 64))
    for f, shp in zip((f1, f2, bank), want):
        _chk(f.wpair, 'wpair', torch.float16)
        if tuple(f.wpair.shape) != shp:
            raise ValueError(f'pair filters {tuple(f.wpair.shape)} do not match the bottleneck ({shp})')
        _chk(f.scale_p, 'scale_p')
        _chk(f.shift, 'shift')
    d = _lib.BottleneckDesc(B, H, W, P)
    io = _lib.BottleneckIO()
    slots = new_slots(x.device)
    io.in_scale, io.amax_in = _scale_ptr(x.slots), _ptr(x.slots)
    io.out_scale, io.amax_out = _scale_ptr(slots), _ptr(slots)
    for i, f in enumerate((f1, f2)):
        io.wbound[i], io.sbound[i] = float(f.wbound), float(f.sbound)
    io.wbound[2], io.sbound[2] = float(bank.wbound3), float(bank.sbound)
    out = torch.empty((B, 1, H, W, 8 * P), device=x.data.device, dtype=torch.float16)
    check(_lib.lib().ivx_bottleneck_proj_fwd_pio(C.byref(d), Cn, C.byref(io), float(bank.wboundd), _ptr(x.data), _ptr(f1.wpair), _ptr(f1.scale_p),
                                                 _ptr(f1.shift), _ptr(f2.wpair), _ptr(f2.scale_p), _ptr(f2.shift), _ptr(bank.wpair), _ptr(bank.scale_p),
                                                 _ptr(bank.shift), _ptr(out), _stream()), 'ivx_bottleneck_proj_fwd_pio')
    return PairTensor(out, slots)


def global_avgpool(x):
    """[B,D,H,W,C] channels-last fp32 or bf16 -> [B,1,1,1,C] fp32: mean over every spatial position (a bf16 map through
    ivx_global_avgpool_fwd_bf16: the same bits as the fp32 pool of x.float())."""
    bf16 = isinstance(x, torch.Tensor) and x.dtype == torch.bfloat16
    _chk(x, 'x', torch.bfloat16 if bf16 else torch.float32)
    B, Cn = x.shape[0], x.shape[-1]
    S = x.numel() // (B * Cn)
    out = torch.empty((B, 1, 1, 1, Cn), device=x.device, dtype=torch.float32)
    fn, name = (_lib.lib().ivx_global_avgpool_fwd_bf16, 'ivx_global_avgpool_fwd_bf16') if bf16 else (_lib.lib().ivx_global_avgpool_fwd, 'ivx_global_avgpool_fwd')
    check(fn(_ptr(x), B, S, Cn, _ptr(out), _stream()), name)
    return out


def dcn_im2col(x, offset_mask, kernel=3, stride=1, pad=1, dil=1):
    """x [B,1,H,W,C], offset_mask [B,1,Ho,Wo,>=3*k*k] fp32 -> modulated deformable columns [B,1,Ho,Wo,k*k*C] in x's dtype:
    fp32 (ivx_dcn_im2col_fwd) or, on bf16 storage, bf16 (ivx_dcn_im2col_fwd_bf16: fp32 blend, one rounding; C % 8 == 0)."""
    bf16 = isinstance(x, torch.Tensor) and x.dtype == torch.bfloat16
    _chk(x, 'x', torch.bfloat16 if bf16 else torch.float32)
    _chk(offset_mask, 'offset_mask')
    B, D, H, W, Cn = x.shape
    Ho = (H + 2 * pad - (dil * (kernel - 1) + 1)) // stride + 1
    Wo = (W + 2 * pad - (dil * (kernel - 1) + 1)) // stride + 1
    if D != 1 or tuple(offset_mask.shape[:4]) != (B, 1, Ho, Wo):
        raise ValueError('offset/mask map does not match the output size')
    col = torch.empty((B, 1, Ho, Wo, kernel * kernel * Cn), device=x.device, dtype=x.dtype)
    fn, name = (_lib.lib().ivx_dcn_im2col_fwd_bf16, 'ivx_dcn_im2col_fwd_bf16') if bf16 else (_lib.lib().ivx_dcn_im2col_fwd, 'ivx_dcn_im2col_fwd')
    check(fn(_ptr(x), _ptr(offset_mask), B, H, W, Cn, kernel, kernel, stride, pad, dil, offset_mask.shape[4], _ptr(col), _stream()), name)
    return col


def dcn_im2col_pair(x, offset_mask, kernel=3, stride=1, pad=1, dil=1):
    """The columns inside the pair chain (ivx_dcn_im2col_fwd_pair): x a PairTensor [B,1,H,W,2C], offset_mask fp32 [B,1,Ho,Wo,>=3*k*k] ->
    PairTensor [B,1,Ho,Wo,2*k*k*C] with x's scale and its own recorded maximum."""
    if not isinstance(x, PairTensor):
        raise TypeError('dcn_im2col_pair takes a PairTensor')
    _chk(offset_mask, 'offset_mask')
    B, D, H, W, C2 = x.data.shape
    Cn = C2 // 2
    Ho = (H + 2 * pad - (dil * (kernel - 1) + 1)) // stride + 1
    Wo = (W + 2 * pad - (dil * (kernel - 1) + 1)) // stride + 1
    if D != 1 or Cn % 16 or tuple(offset_mask.shape[:4]) != (B, 1, Ho, Wo):
        raise ValueError('offset/mask map does not match the output size (or C % 16 != 0)')
    col = torch.empty((B, 1, Ho, Wo, 2 * kernel * kernel * Cn), device=x.data.device, dtype=torch.float16)
    slots = new_slots(x.data.device)
    check(_lib.lib().ivx_dcn_im2col_fwd_pair(_ptr(x.data), _scale_ptr(x.slots), _ptr(offset_mask), B, H, W, Cn, kernel, kernel, stride, pad, dil,
                                             offset_mask.shape[4], _ptr(col), _scale_ptr(slots), _ptr(slots), _stream()), 'ivx_dcn_im2col_fwd_pair')
    return PairTensor(col, slots)


def upsample_trilinear2x(x):
    if x.dtype not in _DT:
        raise TypeError(f'x must be float32 or bfloat16, got {x.dtype}')
    _chk(x, 'x', x.dtype)
    B, D, H, W, Cn = x.shape
    out = torch.empty((B, 2 * D, 2 * H, 2 * W, Cn), device=x.device, dtype=x.dtype)
    fn = _lib.lib().ivx_upsample_trilinear2x_fwd if x.dtype == torch.float32 else _lib.lib().ivx_upsample_trilinear2x_fwd_bf16
    check(fn(_ptr(x), B, D, H, W, Cn, _ptr(out), _stream()), 'ivx_upsample_trilinear2x_fwd')
    return out


# ------------------------------------------------------------------ unprojection
# optional stage timing (bench.py): when a list, backproject_mean appends ('lift', start_event, end_event) around its launch
stage_trace = None

_LIFT_MEAN, _LIFT_SUM, _LIFT_ACCUM = 0, 1, 2
_F32_BF16 = (torch.float32, torch.bfloat16)
# the nearest rule goes to the entry points of the parity claims, called exactly as before ivx_backproject_fwd_ex existed (a library older than 0.4.4 serves it)
_LIFT_NEAREST = {(_LIFT_MEAN, torch.float32): 'ivx_backproject_mean_fwd', (_LIFT_MEAN, torch.bfloat16): 'ivx_backproject_mean_fwd_bf16',
                 (_LIFT_SUM, torch.float32): 'ivx_backproject_sum_fwd',
                 (_LIFT_ACCUM, torch.float32): 'ivx_backproject_accum_fwd', (_LIFT_ACCUM, torch.bfloat16): 'ivx_backproject_accum_fwd_bf16'}


def _lift(mode, sampling, feat, proj, new_origin, crop_hw, voxel_size, n_voxels=None, vol=None, count=None, mean_out=None, valid=None, first=False,
          feat_dtypes=(torch.float32,)):
    """The one checker and caller of the lifts of a view stack: feat [B*V,1,FH,FW,C] channels-last (one of feat_dtypes), proj [B,V,3,4],
    new_origin [B,3], crop_hw [B,2] int32, all on the device.  _LIFT_MEAN: allocates vol [B,X,Y,Z,C] (feat's dtype) and valid (uint8);
    _LIFT_SUM: vol (fp32) and count (int32); _LIFT_ACCUM: the caller's state vol / count, checked here, and its optional mean_out / valid.
    sampling 0: the older export of (mode, dtype); 1: ivx_backproject_fwd_ex.  Returns (vol, count, valid)."""
    dtype = getattr(feat, 'dtype', None)
    _chk(feat, 'feat', dtype if dtype in feat_dtypes else feat_dtypes[0])
    _chk(proj, 'proj')
    _chk(new_origin, 'new_origin')
    _chk(crop_hw, 'crop_hw', torch.int32)
    if mode == _LIFT_ACCUM:
        _chk(vol, 'vol_sum')
        _chk(count, 'count', torch.int32)
    B, V = proj.shape[0], proj.shape[1]
    BV, D, FH, FW, Cn = feat.shape
    if BV != B * V or D != 1 or tuple(proj.shape[2:]) != (3, 4):
        raise ValueError('feat / proj shapes do not agree')
    if mode == _LIFT_ACCUM:
        if vol.dim() != 5 or vol.shape[0] != B or vol.shape[-1] != Cn or tuple(count.shape) != tuple(vol.shape[:-1]):
            raise ValueError('vol_sum must be [B,X,Y,Z,C] and count [B,X,Y,Z] for the features\' B and C')
        if mean_out is not None:
            _chk(mean_out, 'mean_out', dtype)
            if tuple(mean_out.shape) != tuple(vol.shape):
                raise ValueError('mean_out must have the shape of vol_sum')
            _chk_mask(valid, 'valid_out', count.shape)
        X, Y, Z = (int(v) for v in vol.shape[1:4])
    else:
        X, Y, Z = (int(v) for v in n_voxels)
        vol = torch.empty((B, X, Y, Z, Cn), device=feat.device, dtype=dtype if mode == _LIFT_MEAN else torch.float32)
        if mode == _LIFT_MEAN:
            valid = torch.empty((B, X, Y, Z), device=feat.device, dtype=torch.uint8)
        else:
            count = torch.empty((B, X, Y, Z), device=feat.device, dtype=torch.int32)
    vs = (C.c_float * 3)(*[float(v) for v in voxel_size])
    if sampling:
        name = 'ivx_backproject_fwd_ex'
        fn = getattr(_lib.lib(), name, None)
        if fn is None:
            raise _lib.IvxError('this build of libimvoxel_hip.so has no ivx_backproject_fwd_ex (bilinear sampling needs version 0.4.4)')
        d = _lib.BackprojectDesc(B, V, FH, FW, Cn, X, Y, Z, vs, _DT[dtype], mode, int(sampling), int(bool(first)))
        rc = fn(C.byref(d), _ptr(feat), _ptr(proj), _ptr(new_origin), _ptr(crop_hw), _ptr(vol), _ptr(count), _ptr(mean_out), _ptr(valid), _stream())
    else:
        name = _LIFT_NEAREST[mode, dtype]
        outs = {_LIFT_MEAN: (_ptr(vol), _ptr(valid)), _LIFT_SUM: (_ptr(vol), _ptr(count)),
                _LIFT_ACCUM: (_ptr(vol), _ptr(count), int(bool(first)), _ptr(mean_out), _ptr(valid))}[mode]
        rc = getattr(_lib.lib(), name)(_ptr(feat), B, V, FH, FW, Cn, _ptr(proj), _ptr(new_origin), _ptr(crop_hw), vs, X, Y, Z, *outs, _stream())
    check(rc, name)
    return vol, count, valid


def backproject_mean(feat, proj, new_origin, crop_hw, voxel_size, n_voxels, sampling='nearest'):
    """feat [B*V,1,FH,FW,C] channels-last (fp32 or bf16), proj [B,V,3,4], new_origin [B,3], crop_hw [B,2] int32 (device)
    -> volume [B,X,Y,Z,C] (feat's dtype), valid [B,X,Y,Z] bool.
    sampling: 'nearest' (the reference's rule: the entry points of the parity claims, called exactly as before the option existed) or
    'bilinear' (optional extra mode, ivx_backproject_fwd_ex; include/imvoxel.h has the definition)."""
    sampling = _lib.sampling_id(sampling)
    if stage_trace is None:
        return _backproject_mean(feat, proj, new_origin, crop_hw, voxel_size, n_voxels, sampling)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = _backproject_mean(feat, proj, new_origin, crop_hw, voxel_size, n_voxels, sampling)
    e1.record()
    stage_trace.append(('lift', e0, e1))
    return out


def _backproject_mean(feat, proj, new_origin, crop_hw, voxel_size, n_voxels, sampling):
    if sampling and feat.dtype not in _F32_BF16:
        raise TypeError(f'feat must be float32 or bfloat16, got {feat.dtype}')
    if not sampling and feat.dtype == torch.bfloat16 and proj.shape[1] == 1 and feat.shape[-1] % 2 == 0:
        # bf16 storage (optional reduced-precision mode): with one view the nearest lift is a pure gather-copy (no arithmetic on the features,
        # imvoxelnet.py:75 divides by a count of 1), so a bf16 map with C channels is passed as C/2 32-bit words.  (The bilinear blend is
        # arithmetic: a single bf16 view goes through the one kernel template like any other.)
        vol, valid = _backproject_mean(feat.view(torch.float32), proj, new_origin, crop_hw, voxel_size, n_voxels, sampling)
        return vol.view(torch.bfloat16), valid
    vol, _, valid = _lift(_LIFT_MEAN, sampling, feat, proj, new_origin, crop_hw, voxel_size, n_voxels, feat_dtypes=_F32_BF16)
    return vol, valid.view(torch.bool)


def backproject_gather_mean(pool, proj_pool, view_slot, new_origin, crop_hw, voxel_size, n_voxels, sampling='nearest'):
    """backproject_mean over views listed by slot (ivx_backproject_gather_fwd): pool [S,1,FH,FW,C] (or [S,FH,FW,C]) fp32 or bf16 and
    proj_pool [S,3,4] hold one view per slot, view_slot [B,V] lists the views of every sample in the order they count.  The result is
    bit for bit backproject_mean over a contiguous copy of the listed views; slots may repeat, unlisted slots are never read.
    view_slot: a host sequence / CPU int32 tensor (range-checked here, then uploaded: a slot outside [0, S) raises ValueError) or a
    device int32 tensor, used as it is (the kernel treats an out-of-range slot as a view that sees nothing).
    -> volume [B,X,Y,Z,C] (pool's dtype), valid [B,X,Y,Z] bool."""
    vol, valid = _pooled_lift('gather', _LIFT_MEAN, pool, proj_pool, new_origin, crop_hw, voxel_size, None, None, sampling, view_slot=view_slot, n_voxels=n_voxels)
    return vol, valid.view(torch.bool)


def backproject_gather_mean_(pool, proj_pool, view_slot, new_origin, crop_hw, voxel_size, vol, valid, sampling='nearest'):
    """backproject_gather_mean into the caller's buffers (windowed scenes keep theirs): vol [B,X,Y,Z,C] (pool's dtype) and valid
    [B,X,Y,Z] uint8 / bool are overwritten.  Returns (vol, valid as bool)."""
    _pooled_lift('gather', _LIFT_MEAN, pool, proj_pool, new_origin, crop_hw, voxel_size, vol, valid, sampling, view_slot=view_slot)
    return vol, valid.view(torch.bool)


def backproject_lists_accum_(pool, proj_pool, lists, rows, first, new_origin, crop_hw, voxel_size, vol_sum, count, mean_out=None, valid_out=None,
                             sampling='nearest'):
    """backproject_accum_ for B samples that share pools and have RAGGED view lists (ivx_backproject_lists_fwd; scene batches): pool
    [S,1,FH,FW,C] (or [S,FH,FW,C]) fp32 or bf16 and proj_pool [S,3,4] hold one view per slot; lists: B host lists of slots, of differing
    lengths (an empty list adds nothing; -1 inside a list is padding, any other slot outside [0, S) raises ValueError); rows: a host list of
    B DISTINCT ints in [0, R): sample b reads and writes row rows[b] of vol_sum [R,X,Y,Z,C] fp32 / count [R,X,Y,Z] int32 (and of mean_out
    (pool's dtype) / valid_out, both or neither); first: a host list of B bools, sample b starts its row from zero without reading it.
    new_origin [B,3] and crop_hw [B,2] are per sample.  Row rows[b] afterwards is bit for bit backproject_accum_ at B = 1 over a contiguous
    copy of lists[b]'s views; rows named by no sample are neither read nor written.  The three lists go up in one copy; every argument
    error is raised before any launch.  Returns (vol_sum, count)."""
    if (mean_out is None) != (valid_out is None):
        raise ValueError('mean_out and valid_out must both be given or both be None')
    _pooled_lift('lists', _LIFT_ACCUM, pool, proj_pool, new_origin, crop_hw, voxel_size, vol_sum, valid_out, sampling, lists=lists, rows=rows, first=first,
                 count=count, mean_out=mean_out)
    return vol_sum, count


def backproject_lists_mean_(pool, proj_pool, lists, rows, new_origin, crop_hw, voxel_size, vol, valid, sampling='nearest'):
    """backproject_gather_mean_ with RAGGED host lists into rows of the caller's pools: sample b's mean / mask of the views lists[b] go to
    row rows[b] of vol [R,X,Y,Z,C] (pool's dtype) / valid [R,X,Y,Z] uint8 / bool; the other rows stay as they are.  lists, rows and the
    errors as for backproject_lists_accum_.  Row rows[b] is bit for bit backproject_mean over a contiguous copy of lists[b]'s views (an
    empty list: zeros, nothing valid).  Returns (vol, valid as bool)."""
    _pooled_lift('lists', _LIFT_MEAN, pool, proj_pool, new_origin, crop_hw, voxel_size, vol, valid, sampling, lists=lists, rows=rows)
    return vol, valid.view(torch.bool)


def backproject_weighted_accum_(pool, proj_pool, lists, weights, rows, first, decay, new_origin, crop_hw, voxel_size, vol_sum, wsum, count, mean_out=None,
                                valid_out=None, forget_below=0.0, sampling='nearest'):
    """backproject_lists_accum_ with per-view weights, a decay per sample and a forgetting threshold (ivx_backproject_weighted_fwd; fading scenes;
    include/imvoxel.h has the definition).  pool, proj_pool, lists, rows, first, new_origin, crop_hw, vol_sum, count, mean_out / valid_out: as for
    backproject_lists_accum_.  weights: the weight of every SLOT of the pool -- a host list of S finite floats >= 0 (0 makes the slot's view unseen;
    checked here, ValueError), None (1 for every slot), or a device float32 tensor [S], used as it is (the kernel treats NaN, 0, negative and inf as
    an unseen view).  decay: None (nothing fades) or a host list of B floats in (0, 1]: the state of sample b that is read (first[b] false) is
    multiplied by decay[b] before this call's views are added.  wsum [R,X,Y,Z] fp32: the running weight sums, in/out beside vol_sum and count.
    forget_below >= 0: a voxel whose faded weight sum is below it becomes unseen again (sum, weight sum and count zero); 0 forgets nothing.
    mean = wsum > 0 ? vol_sum / wsum : 0.  With unit weights, no decay and forget_below 0, vol_sum / count / mean_out / valid_out are bit for bit
    those of backproject_lists_accum_ and wsum == count.  The lists, the weights and the decays go up in one copy; every argument error is raised
    before any launch.  Returns (vol_sum, wsum, count)."""
    if (mean_out is None) != (valid_out is None):
        raise ValueError('mean_out and valid_out must both be given or both be None')
    _pooled_lift('weighted', _LIFT_ACCUM, pool, proj_pool, new_origin, crop_hw, voxel_size, vol_sum, valid_out, sampling, lists=lists, rows=rows, first=first,
                 count=count, mean_out=mean_out, weighted=dict(weights=weights, decay=decay, forget_below=forget_below, wsum=wsum))
    return vol_sum, wsum, count


def backproject_weighted_mean_(pool, proj_pool, lists, weights, rows, new_origin, crop_hw, voxel_size, vol, valid, sampling='nearest'):
    """backproject_lists_mean_ with per-view weights: row rows[b] of vol / valid becomes the weighted mean  sum(w * sample) / sum(w)  over the
    views of lists[b] that see the voxel and the mask sum(w) > 0.  weights as for backproject_weighted_accum_ (per slot).  With unit weights the
    bits are those of backproject_lists_mean_.  Returns (vol, valid as bool)."""
    _pooled_lift('weighted', _LIFT_MEAN, pool, proj_pool, new_origin, crop_hw, voxel_size, vol, valid, sampling, lists=lists, rows=rows,
                 weighted=dict(weights=weights, decay=None, forget_below=0.0, wsum=None))
    return vol, valid.view(torch.bool)


def backproject_mapped_accum_(pool, proj_pool, lists, weights, rows, first, decay, new_origin, crop_hw, voxel_size, vol_sum, wsum, count, mean_out=None,
                              valid_out=None, forget_below=0.0, sampling='nearest', pixel_weight=None, depth=None, gate=(math.inf, math.inf)):
    """backproject_weighted_accum_ whose views bring pixel maps (ivx_backproject_mapped_fwd; include/imvoxel.h has the definition).  pixel_weight: a
    device float32 tensor [S,FH,FW] (or [S,1,FH,FW]), one confidence map per SLOT of the pool at feature resolution, or None (1 everywhere): the
    weight of a view at a voxel is weights[slot] * pixel_weight[slot, y, x] at the nearest pixel the voxel projects to (one rounded product), and
    the view counts there only if the product passes  w > 0 && w < inf.  depth: a device float32 tensor of the same shape, the measured depth per
    pixel in the units of the projection's third coordinate, or None (no gate); gate = (behind, front), two numbers >= 0 (inf: no limit on that
    side, the default): where the pixel has a measurement D (D > 0 && D < inf; 0, negative, NaN and inf are holes and gate nothing) the view counts
    only at voxels of depth d with  D - front <= d <= D + behind.  The maps are used as they are (no copy; unlisted slots are never read); under the
    bilinear rule they are read at the nearest pixel too.  With both maps None this is backproject_weighted_accum_ (the same launch; the gate is
    still checked).  Everything else, and the returns, as there; every argument error is raised before any launch."""
    if (mean_out is None) != (valid_out is None):
        raise ValueError('mean_out and valid_out must both be given or both be None')
    _pooled_lift('mapped', _LIFT_ACCUM, pool, proj_pool, new_origin, crop_hw, voxel_size, vol_sum, valid_out, sampling, lists=lists, rows=rows, first=first,
                 count=count, mean_out=mean_out, weighted=dict(weights=weights, decay=decay, forget_below=forget_below, wsum=wsum),
                 maps=dict(pixel_weight=pixel_weight, depth=depth, gate=gate))
    return vol_sum, wsum, count


def backproject_mapped_mean_(pool, proj_pool, lists, weights, rows, new_origin, crop_hw, voxel_size, vol, valid, sampling='nearest', pixel_weight=None,
                             depth=None, gate=(math.inf, math.inf)):
    """backproject_weighted_mean_ with the pixel maps of backproject_mapped_accum_: row rows[b] of vol / valid becomes  sum(w * sample) / sum(w)  over
    the views of lists[b] that count at the voxel (seen, inside the gate of their depth map, w = weight * pixel weight valid) and the mask
    sum(w) > 0.  Returns (vol, valid as bool)."""
    _pooled_lift('mapped', _LIFT_MEAN, pool, proj_pool, new_origin, crop_hw, voxel_size, vol, valid, sampling, lists=lists, rows=rows,
                 weighted=dict(weights=weights, decay=None, forget_below=0.0, wsum=None), maps=dict(pixel_weight=pixel_weight, depth=depth, gate=gate))
    return vol, valid.view(torch.bool)


def check_gate(gate):
    """gate = (behind, front) of a depth map: two real numbers >= 0, +inf allowed (no limit on that side), never NaN -> (float, float)."""
    if isinstance(gate, (torch.Tensor, str, bytes)) or not hasattr(gate, '__len__') or len(gate) != 2:
        raise TypeError(f'gate must be (behind, front), two numbers >= 0, got {gate!r}')
    g = []
    for v in gate:
        if isinstance(v, bool) or not hasattr(v, '__float__'):
            raise TypeError(f'gate must hold two real numbers, got {v!r}')
        g.append(float(v))
    if any(not v >= 0 for v in g):
        raise ValueError(f'gate (behind, front) must be >= 0 (inf: no limit on that side) and not NaN, got {tuple(g)}')
    return g[0], g[1]


def _host_floats(x, name, n):
    """A host sequence of n Python / numpy real numbers (no bools, no tensors) -> list of float."""
    if isinstance(x, torch.Tensor) or isinstance(x, (str, bytes)) or not hasattr(x, '__len__'):
        raise TypeError(f'{name} must be a host list of floats')
    out = []
    for v in x:
        if isinstance(v, bool) or not hasattr(v, '__float__'):
            raise TypeError(f'{name} must hold real numbers, got {v!r}')
        out.append(float(v))
    if len(out) != n:
        raise ValueError(f'{name} has {len(out)} entries, expected {n}')
    return out


def _host_ints(x, name, n=None):
    """A host sequence of Python / numpy integers (no bools, no tensors) -> list of int."""
    if isinstance(x, torch.Tensor) or isinstance(x, (str, bytes)) or not hasattr(x, '__len__'):
        raise TypeError(f'{name} must be a host list of integers')
    out = []
    for v in x:
        if isinstance(v, bool) or not hasattr(v, '__index__'):
            raise TypeError(f'{name} must hold integers, got {v!r}')
        out.append(int(v))
    if n is not None and len(out) != n:
        raise ValueError(f'{name} has {len(out)} entries for {n} samples')
    return out


# the three lifts that read their views from a pool by slot: the export of each form and the library version that brought it
_POOLED = {'gather': ('ivx_backproject_gather_fwd', '0.4.6'), 'lists': ('ivx_backproject_lists_fwd', '0.4.7'),
           'weighted': ('ivx_backproject_weighted_fwd', '0.4.8'), 'mapped': ('ivx_backproject_mapped_fwd', '0.5.0')}


def _pooled_lift(form, mode, pool, proj_pool, new_origin, crop_hw, voxel_size, vol, valid, sampling, view_slot=None, n_voxels=None, lists=None, rows=None,
                 first=None, count=None, mean_out=None, weighted=None, maps=None):
    """The one checker and caller of the lifts over pool [S,1,FH,FW,C] / proj_pool [S,3,4]; form is a key of _POOLED.
    'gather' (_LIFT_MEAN only): view_slot [B,V], sample b writes row b.  A host list / CPU tensor is range-checked and uploaded; a device
      int32 tensor is used as it is (no copy).  n_voxels given: vol / valid are allocated here; else the caller's, with B rows.
    'lists': B ragged host lists, rows [B] and (accumulate mode) first [B] into the caller's vol [R,X,Y,Z,C] / count / mean_out / valid.
    'weighted': the same with weighted = dict(weights, decay, forget_below, wsum); host weights [S] and decays [B] travel in the same upload
      (as bits behind the integers).
    'mapped': 'weighted' with maps = dict(pixel_weight, depth, gate): device fp32 maps [S,FH,FW] (or [S,1,FH,FW]) or None, used as they are, and the
      host gate (behind, front); with both maps None the call goes out as 'weighted'.
    The host lists are checked first (against shapes only), then the tensors; then ONE upload of view_slot [B,V] (-1 padded), row [B] and
    first [B], and the launch.  Returns (vol, valid)."""
    sampling = _lib.sampling_id(sampling)
    alloc = n_voxels is not None
    for t, name in ((pool, 'pool'), (proj_pool, 'proj_pool')) + (() if alloc else ((vol, 'vol_sum' if mode == _LIFT_ACCUM else 'vol'),)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f'{name} must be a torch.Tensor')
    if pool.dtype not in _F32_BF16:
        raise TypeError(f'pool must be float32 or bfloat16, got {pool.dtype}')
    if pool.dim() == 5 and pool.shape[1] == 1:
        pool = pool[:, 0]
    if pool.dim() != 4 or tuple(proj_pool.shape) != (pool.shape[0], 3, 4):
        raise ValueError(f'pool must be [S,FH,FW,C] (or [S,1,FH,FW,C]) and proj_pool [S,3,4], got {tuple(pool.shape)} and {tuple(proj_pool.shape)}')
    S, FH, FW, Cn = (int(v) for v in pool.shape)
    if alloc:
        X, Y, Z = (int(v) for v in n_voxels)
    elif vol.dim() != 5 or vol.shape[-1] != Cn:
        raise ValueError('the state / output volume must be [R,X,Y,Z,C] with the pool\'s C')
    else:
        R, X, Y, Z = (int(v) for v in vol.shape[:4])
    host, hostf = [], []                           # what goes up: the integers (view_slot, then row and first), the floats behind them
    if form != 'gather':
        if isinstance(lists, torch.Tensor) or not hasattr(lists, '__len__') or len(lists) < 1:
            raise TypeError('lists must be a host list of B >= 1 lists of slots')
        lists = [_host_ints(l, f'lists[{b}]') for b, l in enumerate(lists)]
        B = len(lists)
        bad = sorted({v for l in lists for v in l if v != -1 and not 0 <= v < S})
        if bad:
            raise ValueError(f'lists hold slots outside [0, {S}) other than the padding -1: {bad}')
        rows = _host_ints(rows, 'rows', B)
        if len(set(rows)) != B:
            raise ValueError(f'rows must be distinct (two samples on one row race), got {rows}')
        if any(not 0 <= r < R for r in rows):
            raise ValueError(f'rows must be in [0, {R}), got {rows}')
        if mode == _LIFT_ACCUM:
            if isinstance(first, torch.Tensor) or not hasattr(first, '__len__') or len(first) != B:
                raise ValueError(f'first must be a host list of {B} bools')
            first = [int(bool(f)) for f in first]
        V = max(1, max(len(l) for l in lists))
        host = [v for l in lists for v in l + [-1] * (V - len(l))] + rows + (first if mode == _LIFT_ACCUM else [])
    elif not (isinstance(view_slot, torch.Tensor) and view_slot.is_cuda):       # a host list: checked here, uploaded once the pools have passed
        slots = view_slot if isinstance(view_slot, torch.Tensor) else torch.as_tensor(view_slot)
        if slots.dtype not in (torch.int32, torch.int64) or slots.dim() != 2 or slots.numel() == 0:
            raise ValueError('a host view_slot must be a [B,V] list / tensor of integers with B, V >= 1')
        (B, V), host = (int(v) for v in slots.shape), slots.flatten().tolist()
        bad = sorted({v for v in host if not 0 <= v < S})
        if bad:
            raise ValueError(f'view_slot holds slots outside [0, {S}): {bad}')
    wdev = decay = None
    if weighted is not None:
        wts, decay, forget_below, wsum = weighted['weights'], weighted['decay'], weighted['forget_below'], weighted['wsum']
        if isinstance(wts, torch.Tensor) and wts.is_cuda:
            wdev = wts                                                                # a device list: used as it is, the kernel guards it
        elif wts is not None:
            wts = _host_floats(wts, 'weights', S)
            if any(not (math.isfinite(w) and w >= 0) for w in wts):
                raise ValueError(f'weights must be finite and >= 0, got {wts}')
            hostf += wts
        if decay is not None:
            if mode != _LIFT_ACCUM:
                raise ValueError('the mean mode takes no decay')
            decay = _host_floats(decay, 'decay', B)
            if any(not 0 < lam <= 1 for lam in decay):
                raise ValueError(f'decay must be in (0, 1], got {decay}')
            hostf += decay
        if isinstance(forget_below, bool) or not isinstance(forget_below, (int, float)) or not (math.isfinite(forget_below) and forget_below >= 0):
            raise ValueError(f'forget_below must be a finite number >= 0, got {forget_below!r}')
    mdev = {}
    if maps is not None:                           # the gate and the maps' shapes are host rules; device, dtype and layout come with the other tensors
        gate = check_gate(maps['gate'])
        for name in ('pixel_weight', 'depth'):
            t = maps[name]
            if t is None:
                continue
            if not isinstance(t, torch.Tensor):
                raise TypeError(f'{name} must be None or a torch.Tensor [S,FH,FW]')
            if t.dim() == 4 and t.shape[1] == 1:
                t = t[:, 0]
            if tuple(t.shape) != (S, FH, FW):
                raise ValueError(f'{name} must be [S,FH,FW] = [{S},{FH},{FW}] (or [S,1,FH,FW]) for this pool, got {tuple(maps[name].shape)}')
            mdev[name] = t
        if not mdev:
            form = 'weighted'
    _chk(pool, 'pool', pool.dtype)
    _chk(proj_pool, 'proj_pool')
    for name, t in mdev.items():
        _chk(t, name)
    if form == 'gather' and not host:                                             # a device list: used as it is, the kernel guards it
        _chk(view_slot, 'view_slot', torch.int32)
        if view_slot.dim() != 2 or view_slot.shape[0] < 1 or view_slot.shape[1] < 1:
            raise ValueError(f'view_slot must be [B,V] with B, V >= 1, got {tuple(view_slot.shape)}')
        B, V = (int(v) for v in view_slot.shape)
    _chk(new_origin, 'new_origin')
    _chk(crop_hw, 'crop_hw', torch.int32)
    if tuple(new_origin.shape) != (B, 3) or tuple(crop_hw.shape) != (B, 2):
        raise ValueError(f'new_origin must be [B,3] and crop_hw [B,2] for the B {"rows of view_slot" if form == "gather" else "lists"}')
    if alloc:
        vol = torch.empty((B, X, Y, Z, Cn), device=pool.device, dtype=pool.dtype)
        valid = torch.empty((B, X, Y, Z), device=pool.device, dtype=torch.uint8)
    elif mode == _LIFT_ACCUM:
        _chk(vol, 'vol_sum')
        _chk(count, 'count', torch.int32)
        if tuple(count.shape) != (R, X, Y, Z):
            raise ValueError('count must be [R,X,Y,Z] for vol_sum [R,X,Y,Z,C]')
        if mean_out is not None:
            _chk(mean_out, 'mean_out', pool.dtype)
            if tuple(mean_out.shape) != tuple(vol.shape):
                raise ValueError('mean_out must have the shape of vol_sum')
            _chk_mask(valid, 'valid_out', count.shape)
    else:
        _chk(vol, 'vol', pool.dtype)
        if form == 'gather' and R != B:
            raise ValueError('vol must be [B,X,Y,Z,C] for the B rows of view_slot and the pool\'s C')
        _chk_mask(valid, 'valid', vol.shape[:-1])
    if weighted is not None:
        if wdev is not None and tuple(_chk(wdev, 'weights').shape) != (S,):
            raise ValueError(f'device weights must be [S] = [{S}], got {tuple(wdev.shape)}')
        if mode == _LIFT_ACCUM:
            if not isinstance(wsum, torch.Tensor):
                raise TypeError('wsum must be a torch.Tensor')
            if tuple(_chk(wsum, 'wsum').shape) != (R, X, Y, Z):
                raise ValueError('wsum must be [R,X,Y,Z] for vol_sum [R,X,Y,Z,C]')
    export, since = _POOLED[form]
    fn = getattr(_lib.lib(), export, None)
    if fn is None:
        raise _lib.IvxError(f'this build of libimvoxel_hip.so has no {export} (needs version {since})')
    if host:                                       # the one upload (`dev` is released in stream order: the allocator reuses it after this launch)
        ints = torch.tensor(host, dtype=torch.int32)
        dev = (torch.cat([ints, torch.tensor(hostf, dtype=torch.float32).view(torch.int32)]) if hostf else ints).to(pool.device)
        p0, n_vs = dev.data_ptr(), B * V
    d = _lib.BackprojectDesc(B, V, FH, FW, Cn, X, Y, Z, (C.c_float * 3)(*[float(v) for v in voxel_size]), _DT[pool.dtype], mode, sampling, 0)
    if form == 'gather':
        rc = fn(C.byref(d), S, _ptr(pool), _ptr(proj_pool), C.c_void_p(p0) if host else _ptr(view_slot), _ptr(new_origin), _ptr(crop_hw), _ptr(vol),
                _ptr(valid), _stream())
    else:
        l = _lib.LiftLists(S, R, p0, p0 + 4 * n_vs, (p0 + 4 * (n_vs + B)) if mode == _LIFT_ACCUM else None)
        tensors = (_ptr(pool), _ptr(proj_pool), _ptr(new_origin), _ptr(crop_hw), _ptr(vol), _ptr(count), _ptr(mean_out), _ptr(valid), _stream())
        if form == 'lists':
            rc = fn(C.byref(d), C.byref(l), *tensors)
        else:
            extra = (C.byref(_lib.LiftMaps(_ptr(mdev.get('pixel_weight')), _ptr(mdev.get('depth')), *gate)),) if form == 'mapped' else ()
            pf = p0 + 4 * len(host)                                                # the floats: weights [S] (when they came as a host list), then decay [B]
            n_w = S if (wdev is None and wts is not None) else 0
            w = _lib.LiftWeights(_ptr(wdev) if wdev is not None else (pf if n_w else None), (pf + 4 * n_w) if decay is not None else None,
                                 float(forget_below), _ptr(wsum) if mode == _LIFT_ACCUM else None)
            rc = fn(C.byref(d), C.byref(l), C.byref(w), *extra, *tensors)
    check(rc, export)
    return vol, valid


def backproject_sum(feat, proj, new_origin, crop_hw, voxel_size, n_voxels, sampling='nearest'):
    """View-sharded mode: like backproject_mean but returns the raw view sum [B,X,Y,Z,C] and the int32 view count
    [B,X,Y,Z] of THIS rank's views (to be all-reduced, then volume_normalize_).  sampling as for backproject_mean."""
    vol, cnt, _ = _lift(_LIFT_SUM, _lib.sampling_id(sampling), feat, proj, new_origin, crop_hw, voxel_size, n_voxels)
    return vol, cnt


def volume_normalize_(vol_sum, count):
    """In place: vol = count ? vol / count : 0; returns (vol, valid bool [B,X,Y,Z])."""
    _chk(vol_sum, 'vol_sum')
    _chk(count, 'count', torch.int32)
    if tuple(count.shape) != tuple(vol_sum.shape[:-1]):
        raise ValueError('count must have the spatial shape of the volume')
    valid = torch.empty(count.shape, device=vol_sum.device, dtype=torch.uint8)
    check(_lib.lib().ivx_volume_normalize_fwd(_ptr(vol_sum), _ptr(count), count.numel(), vol_sum.shape[-1], _ptr(valid), _stream()),
          'ivx_volume_normalize_fwd')
    return vol_sum, valid.view(torch.bool)


def _chk_mask(t, name, shape):
    if t.dtype not in (torch.uint8, torch.bool):
        raise TypeError(f'{name} must be uint8 or bool, got {t.dtype}')
    _chk(t, name, t.dtype)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f'{name} must have the spatial shape of the volume')
    return t


def backproject_accum_(feat, proj, new_origin, crop_hw, voxel_size, vol_sum, count, first, mean_out=None, valid_out=None, sampling='nearest'):
    """Streaming scenes: add the V views of `feat` ([B*V,1,FH,FW,C] fp32 or bf16) to the running state vol_sum [B,X,Y,Z,C] fp32 /
    count [B,X,Y,Z] int32, in place and in view order (ivx_backproject_accum_fwd: after the last chunk the state holds what ONE
    backproject_mean over all the views computes, bit for bit).  first: start the state from zero without reading it.
    mean_out [B,X,Y,Z,C] (feat's dtype) + valid_out [B,X,Y,Z] uint8 / bool: the same pass also writes the mean and the mask; both or
    neither.  sampling as for backproject_mean (one rule per running volume).  Returns (vol_sum, count)."""
    sampling = _lib.sampling_id(sampling)
    if feat.dtype not in _F32_BF16:
        raise TypeError(f'feat must be float32 or bfloat16, got {feat.dtype}')
    if (mean_out is None) != (valid_out is None):
        raise ValueError('mean_out and valid_out must both be given or both be None')
    _lift(_LIFT_ACCUM, sampling, feat, proj, new_origin, crop_hw, voxel_size, vol=vol_sum, count=count, mean_out=mean_out, valid=valid_out, first=first,
          feat_dtypes=_F32_BF16)
    return vol_sum, count


def volume_mean(vol_sum, count, dtype=torch.float32, out=None, valid_out=None):
    """Out of place: mean = count ? vol_sum / count : 0 in `dtype` (float32 or bfloat16), valid = count > 0; vol_sum and count stay
    as they are.  out / valid_out: buffers to write into (allocated when None).  Returns (mean, valid bool [B,X,Y,Z])."""
    return _mean_of_state('ivx_volume_mean_fwd', None, vol_sum, count, 'count', torch.int32, dtype, out, valid_out)


def _mean_of_state(export, since, vol_sum, den, den_name, den_dtype, dtype, out, valid_out):
    """The one body of volume_mean (den: the int32 count) and volume_wmean (den: the fp32 weight sum); since: the library version that brought
    the export, when an older library may lack it."""
    _chk(vol_sum, 'vol_sum')
    _chk(den, den_name, den_dtype)
    if dtype not in _F32_BF16:
        raise TypeError(f'dtype must be float32 or bfloat16, got {dtype}')
    if tuple(den.shape) != tuple(vol_sum.shape[:-1]):
        raise ValueError(f'{den_name} must have the spatial shape of the volume')
    if out is None:
        out = torch.empty(vol_sum.shape, device=vol_sum.device, dtype=dtype)
    elif tuple(_chk(out, 'out', dtype).shape) != tuple(vol_sum.shape):
        raise ValueError('out must have the shape of vol_sum')
    if valid_out is None:
        valid_out = torch.empty(den.shape, device=vol_sum.device, dtype=torch.uint8)
    else:
        _chk_mask(valid_out, 'valid_out', den.shape)
    fn = getattr(_lib.lib(), export) if since is None else getattr(_lib.lib(), export, None)
    if fn is None:
        raise _lib.IvxError(f'this build of libimvoxel_hip.so has no {export} (needs version {since})')
    check(fn(_ptr(vol_sum), _ptr(den), den.numel(), vol_sum.shape[-1], _ptr(out), _DT[dtype], _ptr(valid_out), _stream()), export)
    return out, valid_out.view(torch.bool)


def volume_wmean(vol_sum, wsum, dtype=torch.float32, out=None, valid_out=None):
    """volume_mean for a weighted state (ivx_volume_wmean_fwd): mean = wsum > 0 ? vol_sum / wsum : 0 in `dtype` (float32 or bfloat16), valid =
    wsum > 0 -- the mean_out / valid_out of backproject_weighted_accum_ on the same state, bit for bit; vol_sum and wsum stay as they are.
    Returns (mean, valid bool [R,X,Y,Z])."""
    return _mean_of_state('ivx_volume_wmean_fwd', '0.4.8', vol_sum, wsum, 'wsum', torch.float32, dtype, out, valid_out)


def volume_scroll_(vol_sum, count, rows, shifts, wsum=None):
    """Scrolling scenes: move rows of the state pools vol_sum [R,X,Y,Z,C] fp32 / count [R,X,Y,Z] int32 (/ wsum [R,X,Y,Z] fp32) by whole voxels,
    in place (ivx_volume_scroll_fwd): for sample b, row rows[b] becomes new[i,j,k] = old[i+sx, j+sy, k+sz] with (sx, sy, sz) = shifts[b] where that
    source lies inside the grid and an unseen voxel (all bits zero) elsewhere -- a pure move of bits, NaN payloads, -0 and denormals included.
    rows: B distinct host integers in [0, R); shifts: B host triples of integers (one triple alone for B = 1).  Rows not named are neither read
    nor written.  Every check comes before the one C call, so a call that raises changes nothing.  Returns (vol_sum, count)."""
    for t, name in ((vol_sum, 'vol_sum'), (count, 'count')) + (((wsum, 'wsum'),) if wsum is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f'{name} must be a torch.Tensor')
    if vol_sum.dim() != 5:
        raise ValueError(f'vol_sum must be [R,X,Y,Z,C], got {tuple(vol_sum.shape)}')
    R, X, Y, Z, Cn = (int(v) for v in vol_sum.shape)
    rows = _host_ints(rows, 'rows')
    if not rows:
        raise ValueError('rows must name at least one row')
    if isinstance(shifts, torch.Tensor) or isinstance(shifts, (str, bytes)) or not hasattr(shifts, '__len__'):
        raise TypeError('shifts must be a host list of (sx, sy, sz) integer triples')
    if len(rows) == 1 and len(shifts) == 3 and not any(hasattr(s, '__len__') for s in shifts):
        shifts = [shifts]
    shifts = [_host_ints(s, f'shifts[{b}]') for b, s in enumerate(shifts)]
    if len(shifts) != len(rows) or any(len(s) != 3 for s in shifts):
        raise ValueError(f'shifts must hold one (sx, sy, sz) triple per row: {len(rows)} rows, got {shifts}')
    if any(not -2 ** 31 <= v < 2 ** 31 for s in shifts for v in s):
        raise ValueError(f'shifts must fit int32, got {shifts}')
    if len(set(rows)) != len(rows):
        raise ValueError(f'rows must be distinct (two samples on one row race), got {rows}')
    if any(not 0 <= r < R for r in rows):
        raise ValueError(f'rows must be in [0, {R}), got {rows}')
    if Cn % 4:
        raise ValueError(f'vol_sum must have C % 4 == 0, got C = {Cn}')
    if tuple(count.shape) != (R, X, Y, Z):
        raise ValueError('count must be [R,X,Y,Z] for vol_sum [R,X,Y,Z,C]')
    if wsum is not None and tuple(wsum.shape) != (R, X, Y, Z):
        raise ValueError('wsum must be [R,X,Y,Z] for vol_sum [R,X,Y,Z,C]')
    _chk(vol_sum, 'vol_sum')
    _chk(count, 'count', torch.int32)
    if wsum is not None:
        _chk(wsum, 'wsum')
        if wsum.device != vol_sum.device:
            raise ValueError('wsum must be on the device of vol_sum')
    if count.device != vol_sum.device:
        raise ValueError('count must be on the device of vol_sum')
    fn = getattr(_lib.lib(), 'ivx_volume_scroll_fwd', None)
    if fn is None:
        raise _lib.IvxError('this build of libimvoxel_hip.so has no ivx_volume_scroll_fwd (needs version 0.4.9)')
    B = len(rows)
    check(fn(B, (C.c_int32 * B)(*rows), (C.c_int32 * (3 * B))(*[v for s in shifts for v in s]), R, X, Y, Z, Cn, _ptr(vol_sum), _ptr(count), _ptr(wsum),
             _stream()), 'ivx_volume_scroll_fwd')
    return vol_sum, count


RIGID_TOL = 1e-4             # a transform of volume_warp is rigid when max |R^T R - I| <= RIGID_TOL and det R > 0, in float64 (a float32 rotation: ~1e-7)


def check_rigid(T, name='transform'):
    """A rigid transform as a host 4x4 or 3x4 array (numpy, a host tensor, nested lists) -> float32 array [3,4].  Finite; a 4x4 must have the
    last row (0, 0, 0, 1); R = T[:3,:3] must satisfy max |R^T R - I| <= RIGID_TOL and det R > 0, computed in float64: a scale, a shear and a
    reflection raise ValueError."""
    import numpy as np
    if isinstance(T, torch.Tensor):
        if T.is_cuda:
            raise TypeError(f'{name} must be a host matrix (the transforms of a warp are checked and passed by value), got a device tensor')
        T = T.detach().numpy()
    try:
        A = np.asarray(T, np.float64)
    except (TypeError, ValueError):
        raise TypeError(f'{name} must be a 4x4 or 3x4 matrix of numbers, got {type(T).__name__}') from None
    if A.shape not in ((4, 4), (3, 4)):
        raise ValueError(f'{name} must be 4x4 or 3x4, got {A.shape}')
    if not np.isfinite(A).all():
        raise ValueError(f'{name} must be finite')
    if A.shape == (4, 4) and not np.array_equal(A[3], [0, 0, 0, 1]):
        raise ValueError(f'{name}: the last row of a 4x4 must be (0, 0, 0, 1), got {A[3].tolist()}')
    R = A[:3, :3]
    off = float(np.abs(R.T @ R - np.eye(3)).max())
    if not off <= RIGID_TOL:
        raise ValueError(f'{name} is not rigid: max |R^T R - I| = {off:.3g} > {RIGID_TOL} (a scale or a shear would not keep the voxel size)')
    if not np.linalg.det(R) > 0:
        raise ValueError(f'{name} is not rigid: det R < 0 (a reflection)')
    return np.ascontiguousarray(A[:3], np.float32)


def _rigid_list(transforms, B):
    """The transforms of a resample of B rows: a host list of B 4x4 or 3x4 matrices, or one matrix alone for one row -> B float32 [3,4] arrays
    through check_rigid."""
    if isinstance(transforms, (str, bytes)) or not hasattr(transforms, '__len__'):
        raise TypeError('transforms must be a host list of 4x4 or 3x4 matrices')
    if B == 1 and (transforms.dim() == 2 if isinstance(transforms, torch.Tensor) else
                   len(transforms) in (3, 4) and all(hasattr(r, '__len__') and len(r) == 4 and not any(hasattr(v, '__len__') for v in r) for r in transforms)):
        transforms = [transforms]                               # one matrix alone for one row
    if len(transforms) != B:
        raise ValueError(f'transforms must hold one matrix per row: {B} rows, got {len(transforms)}')
    return [check_rigid(T, f'transforms[{b}]') for b, T in enumerate(transforms)]


def _grid_floats(B, voxel_size, **origins):
    """The host grid arguments of a resample of B rows: every named origin as host floats [B,3] (or [3] for all) and voxel_size as three numbers,
    finite, voxel_size > 0 -> ([float32 [B,3] per origin], float32 [3])."""
    import numpy as np
    names = ' and '.join(origins)
    for name, o in origins.items():
        if isinstance(o, torch.Tensor):
            if o.is_cuda:
                raise TypeError(f'{name} must be host floats [B,3] (it is checked and passed by value), got a device tensor')
            origins[name] = o.detach().numpy()
    try:
        os_ = [np.asarray(o, np.float32) for o in origins.values()]
        vs = np.asarray([float(v) for v in voxel_size], np.float32)
    except (TypeError, ValueError):
        raise TypeError(f'{names} must be host floats [B,3] and voxel_size three numbers') from None
    os_ = [np.broadcast_to(o, (B, 3)) if o.shape == (3,) else o for o in os_]
    if any(o.shape != (B, 3) for o in os_) or vs.shape != (3,):
        raise ValueError(f'{names} must be [B,3] (or [3]) for {B} rows and voxel_size three numbers, got {", ".join(str(o.shape) for o in os_)} and {vs.shape}')
    if not (all(np.isfinite(o).all() for o in os_) and np.isfinite(vs).all() and (vs > 0).all()):
        raise ValueError(f'{names} must be finite and voxel_size finite and > 0, got {", ".join(str(o.tolist()) for o in os_)} and {vs.tolist()}')
    return os_, vs


def _check_forget(forget_below):
    if isinstance(forget_below, bool) or not isinstance(forget_below, (int, float)) or not (math.isfinite(forget_below) and forget_below >= 0):
        raise ValueError(f'forget_below must be a finite number >= 0, got {forget_below!r}')


def volume_warp(vol_sum, wsum, count, rows, transforms, new_origin, voxel_size, out, out_rows=None, forget_below=0.0):
    """Scenes that turn with their platform: resample rows of the state pools vol_sum [R,X,Y,Z,C] fp32 / wsum [R,X,Y,Z] fp32 / count [R,X,Y,Z]
    int32 under rigid transforms into the pools out = (sum, wsum, count) of the same X, Y, Z, C (ivx_volume_warp_fwd; include/imvoxel.h has the
    definition).  For sample b, row out_rows[b] of `out` (None: rows[b]) becomes the trilinear read of row rows[b] at x_old = T x_new with
    T = transforms[b], a host 4x4 or 3x4 matrix (check_rigid; one matrix alone for one row) that maps a point of the NEW grid frame to the OLD one;
    the grid itself -- new_origin [B,3] (or [3] for all; host floats, the device new_origin of the lifts) and voxel_size -- stays.  Sums and
    weight sum take the same weights, count the maximum over the corners read; a voxel whose source lies outside the grid is unseen, and with
    forget_below > 0 so is one whose new weight sum is below it.  Out of place: `out` must not share memory with the inputs.  rows: B host
    integers in [0, R); out_rows: B distinct host integers.  Rows not named are neither read nor written.  Every check comes before the one C
    call, so a call that raises changes nothing.  Returns out."""
    import numpy as np
    for t, name in ((vol_sum, 'vol_sum'), (wsum, 'wsum'), (count, 'count')):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f'{name} must be a torch.Tensor')
    if not isinstance(out, (tuple, list)) or len(out) != 3 or any(not isinstance(t, torch.Tensor) for t in out):
        raise TypeError('out must be a (sum, wsum, count) triple of torch.Tensors: the warp is out of place')
    osum, owsum, ocount = out
    if vol_sum.dim() != 5:
        raise ValueError(f'vol_sum must be [R,X,Y,Z,C], got {tuple(vol_sum.shape)}')
    R, X, Y, Z, Cn = (int(v) for v in vol_sum.shape)
    rows = _host_ints(rows, 'rows')
    if not rows:
        raise ValueError('rows must name at least one row')
    B = len(rows)
    out_rows = list(rows) if out_rows is None else _host_ints(out_rows, 'out_rows', B)
    M = _rigid_list(transforms, B)
    (o,), vs = _grid_floats(B, voxel_size, new_origin=new_origin)
    _check_forget(forget_below)
    if any(not 0 <= r < R for r in rows):
        raise ValueError(f'rows must be in [0, {R}), got {rows}')
    if osum.dim() != 5 or tuple(osum.shape[1:]) != (X, Y, Z, Cn):
        raise ValueError(f'out[0] must be [R_out,{X},{Y},{Z},{Cn}] like vol_sum, got {tuple(osum.shape)}')
    Ro = int(osum.shape[0])
    if len(set(out_rows)) != B:
        raise ValueError(f'out_rows must be distinct (two samples on one row race), got {out_rows}')
    if any(not 0 <= r < Ro for r in out_rows):
        raise ValueError(f'out_rows must be in [0, {Ro}), got {out_rows}')
    if Cn % 4:
        raise ValueError(f'vol_sum must have C % 4 == 0, got C = {Cn}')
    for t, name, shape in ((wsum, 'wsum', (R, X, Y, Z)), (count, 'count', (R, X, Y, Z)), (owsum, 'out[1]', (Ro, X, Y, Z)), (ocount, 'out[2]', (Ro, X, Y, Z))):
        if tuple(t.shape) != shape:
            raise ValueError(f'{name} must be {list(shape)} beside its sums, got {tuple(t.shape)}')
    for t, name, dt in ((vol_sum, 'vol_sum', torch.float32), (wsum, 'wsum', torch.float32), (count, 'count', torch.int32), (osum, 'out[0]', torch.float32),
                        (owsum, 'out[1]', torch.float32), (ocount, 'out[2]', torch.int32)):
        _chk(t, name, dt)
        if t.device != vol_sum.device:
            raise ValueError(f'{name} must be on the device of vol_sum')
    for a, an in ((vol_sum, 'vol_sum'), (wsum, 'wsum'), (count, 'count')):
        for t, tn in ((osum, 'out[0]'), (owsum, 'out[1]'), (ocount, 'out[2]')):
            a0, t0 = a.data_ptr(), t.data_ptr()
            if a0 < t0 + t.numel() * 4 and t0 < a0 + a.numel() * 4:
                raise ValueError(f'{tn} shares memory with {an}: a resample cannot run in place')
    fn = getattr(_lib.lib(), 'ivx_volume_warp_fwd', None)
    if fn is None:
        raise _lib.IvxError('this build of libimvoxel_hip.so has no ivx_volume_warp_fwd (needs version 0.5.4)')
    flat = lambda a: (C.c_float * a.size)(*np.ascontiguousarray(a, np.float32).reshape(-1).tolist())     # noqa: E731
    check(fn(B, (C.c_int32 * B)(*rows), (C.c_int32 * B)(*out_rows), flat(np.stack(M)), flat(o), flat(vs), float(forget_below), R, Ro, X, Y, Z, Cn,
             _ptr(vol_sum), _ptr(wsum), _ptr(count), _ptr(osum), _ptr(owsum), _ptr(ocount), _stream()), 'ivx_volume_warp_fwd')
    return out


def volume_merge_(vol_sum, wsum, count, rows, src, src_rows, transforms, new_origin, src_origin, voxel_size, alpha=1.0, forget_below=0.0):
    """Scenes that become one: add rows of the state pools src = (sum, wsum, count) into rows of the pools vol_sum [R,X,Y,Z,C] fp32 / wsum [R,X,Y,Z]
    fp32 / count [R,X,Y,Z] int32 of the same X, Y, Z, C under rigid transforms, in place (ivx_volume_merge_fwd; include/imvoxel.h has the
    definition).  For sample b, row rows[b] takes  S += alpha * S_s, W += alpha * W_s, count += count_s  where (S_s, W_s, count_s) is the trilinear
    read of row src_rows[b] of `src` at x_src = T x_dst, T = transforms[b] a host 4x4 or 3x4 matrix (check_rigid; one matrix alone for one row)
    that maps a point of the destination grid's frame to the source grid's -- at the voxels where the source holds evidence (inside its grid,
    W_s > 0); no other voxel is written.  new_origin / src_origin: the two grids' corner terms, host floats [B,3] (or [3] for all), which may
    differ (a scrolled scene); voxel_size is common.  alpha: one float or B floats, finite and > 0.  forget_below > 0: a merged voxel whose new
    weight sum is below it becomes unseen.  rows: B distinct host integers in [0, R); src_rows: B host integers (a source row may repeat).  `src`
    may be the same pools (rows of one batch) as long as no row is both a source and a destination; any other shared memory raises.  Rows not
    named are neither read nor written, and the source pools are read only.  Every check comes before the one C call, so a call that raises
    changes nothing.  Returns (vol_sum, wsum, count)."""
    import numpy as np
    for t, name in ((vol_sum, 'vol_sum'), (wsum, 'wsum'), (count, 'count')):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f'{name} must be a torch.Tensor')
    if not isinstance(src, (tuple, list)) or len(src) != 3 or any(not isinstance(t, torch.Tensor) for t in src):
        raise TypeError('src must be a (sum, wsum, count) triple of torch.Tensors')
    ssum, swsum, scount = src
    if vol_sum.dim() != 5:
        raise ValueError(f'vol_sum must be [R,X,Y,Z,C], got {tuple(vol_sum.shape)}')
    R, X, Y, Z, Cn = (int(v) for v in vol_sum.shape)
    rows = _host_ints(rows, 'rows')
    if not rows:
        raise ValueError('rows must name at least one row')
    B = len(rows)
    src_rows = _host_ints(src_rows, 'src_rows', B)
    M = _rigid_list(transforms, B)
    (o, so), vs = _grid_floats(B, voxel_size, new_origin=new_origin, src_origin=src_origin)
    try:
        al = np.asarray(alpha.tolist() if isinstance(alpha, torch.Tensor) else alpha, np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise TypeError(f'alpha must be one number or {B} numbers, got {alpha!r}') from None
    if isinstance(alpha, bool) or al.shape not in ((1,), (B,)) or (al.shape == (1,) and hasattr(alpha, '__len__') and B != 1):
        raise ValueError(f'alpha must be one number or {B} numbers (one per row), got {alpha!r}')
    al = np.broadcast_to(al, (B,)).astype(np.float32)
    if not (np.isfinite(al).all() and (al > 0).all()):
        raise ValueError(f'alpha must be finite and > 0 (after rounding to float32), got {al.tolist()}')
    _check_forget(forget_below)
    if len(set(rows)) != B:
        raise ValueError(f'rows must be distinct (two samples on one destination row race), got {rows}')
    if any(not 0 <= r < R for r in rows):
        raise ValueError(f'rows must be in [0, {R}), got {rows}')
    if ssum.dim() != 5 or tuple(ssum.shape[1:]) != (X, Y, Z, Cn):
        raise ValueError(f'src[0] must be [R_src,{X},{Y},{Z},{Cn}] like vol_sum, got {tuple(ssum.shape)}')
    Rs = int(ssum.shape[0])
    if any(not 0 <= r < Rs for r in src_rows):
        raise ValueError(f'src_rows must be in [0, {Rs}), got {src_rows}')
    if Cn % 4:
        raise ValueError(f'vol_sum must have C % 4 == 0, got C = {Cn}')
    for t, name, shape in ((wsum, 'wsum', (R, X, Y, Z)), (count, 'count', (R, X, Y, Z)), (swsum, 'src[1]', (Rs, X, Y, Z)), (scount, 'src[2]', (Rs, X, Y, Z))):
        if tuple(t.shape) != shape:
            raise ValueError(f'{name} must be {list(shape)} beside its sums, got {tuple(t.shape)}')
    for t, name, dt in ((vol_sum, 'vol_sum', torch.float32), (wsum, 'wsum', torch.float32), (count, 'count', torch.int32), (ssum, 'src[0]', torch.float32),
                        (swsum, 'src[1]', torch.float32), (scount, 'src[2]', torch.int32)):
        _chk(t, name, dt)
        if t.device != vol_sum.device:
            raise ValueError(f'{name} must be on the device of vol_sum')
    dst = (vol_sum, wsum, count)
    same = all(a.data_ptr() == t.data_ptr() for a, t in zip(dst, src)) and Rs == R
    if same:
        both = sorted(set(rows) & set(src_rows))
        if both:
            raise ValueError(f'with the same pools as source and destination, rows {both} are named both as a source and as a destination')
    else:
        for a, an in zip(dst, ('vol_sum', 'wsum', 'count')):
            for t, tn in zip(src, ('src[0]', 'src[1]', 'src[2]')):
                a0, t0 = a.data_ptr(), t.data_ptr()
                if a0 < t0 + t.numel() * 4 and t0 < a0 + a.numel() * 4:
                    raise ValueError(f'{tn} shares memory with {an} without src being the same pools: a merge reads its source while it writes')
    fn = getattr(_lib.lib(), 'ivx_volume_merge_fwd', None)
    if fn is None:
        raise _lib.IvxError('this build of libimvoxel_hip.so has no ivx_volume_merge_fwd (needs version 0.5.5)')
    flat = lambda a: (C.c_float * a.size)(*np.ascontiguousarray(a, np.float32).reshape(-1).tolist())     # noqa: E731
    check(fn(B, (C.c_int32 * B)(*src_rows), (C.c_int32 * B)(*rows), flat(np.stack(M)), flat(o), flat(so), flat(al), flat(vs), float(forget_below), Rs, R,
             X, Y, Z, Cn, _ptr(ssum), _ptr(swsum), _ptr(scount), _ptr(vol_sum), _ptr(wsum), _ptr(count), _stream()), 'ivx_volume_merge_fwd')
    return vol_sum, wsum, count


def _match_step(step):
    """The lattice step of a match: one integer for all axes or three -> [px, py, pz], each >= 1 and an int32."""
    if hasattr(step, '__index__') and not isinstance(step, (bool, torch.Tensor)) and not hasattr(step, '__len__'):
        step = (step,) * 3
    try:
        p = _host_ints(step, 'step')
    except TypeError:
        raise ValueError(f'step must be one integer >= 1 or three (px, py, pz), got {step!r}') from None
    if len(p) != 3 or any(not 1 <= v < 2 ** 31 for v in p):
        raise ValueError(f'step must be one integer >= 1 or three (px, py, pz), each >= 1, got {step!r}')
    return p


def volume_match(vol_sum, wsum, rows, src, src_rows, transforms, new_origin, src_origin, voxel_size, step=(1, 1, 1)):
    """Matching scenes: score candidate rigid transforms between rows of the state pools vol_sum [R,X,Y,Z,C] fp32 / wsum [R,X,Y,Z] fp32 and rows of
    the pools src = (sum, wsum) of the same X, Y, Z, C (ivx_volume_match_fwd; include/imvoxel.h has the definition).  For sample b, row rows[b]
    (the destination: its voxels are visited) is compared with the trilinear read of row src_rows[b] of `src` at x_src = T x_dst for each of the
    K candidates T of transforms[b] -- a host list of K 4x4 or 3x4 matrices per sample (check_rigid each), the same K for every sample.  Over the
    voxels both hold evidence for ("paired": own W_d > 0, inside the source grid, sampled W_s > 0) and all channels, with the means a = S_d / W_d
    and b = S_s / W_s:  dot = sum a b, na = sum a a, nb = sum b b.  new_origin / src_origin: the two grids' corner terms, host floats [B,3] (or [3]
    for all); voxel_size is common.  step: the lattice step, one integer or (px, py, pz), each >= 1: only voxels with i % px == j % py == k % pz
    == 0 are visited.  rows and src_rows: B host integers each; rows may repeat, `src` may be the same pools and a row may be matched against
    itself: everything is read only.  Every check comes before the one C call.  The sums are deterministic: the same two states give the same
    bits in any rows of any pools.
    -> (pairs [B,K] int64, own [B] int64, stats [B,K,3] float64 = (dot, na, nb)) as device tensors; the score is the caller's:
    ncc = dot / sqrt(na * nb), overlap = pairs / own."""
    return _match_call(vol_sum, wsum, rows, src, src_rows, transforms, new_origin, src_origin, voxel_size, step)


def _match_call(vol_sum, wsum, rows, src, src_rows, transforms, new_origin, src_origin, voxel_size, step, about=None):
    """The one path of volume_match (about None) and volume_align: every host check, the scratch, the outputs and the one C call."""
    import numpy as np
    for t, name in ((vol_sum, 'vol_sum'), (wsum, 'wsum')):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f'{name} must be a torch.Tensor')
    if not isinstance(src, (tuple, list)) or len(src) not in (2, 3) or any(not isinstance(t, torch.Tensor) for t in src):
        raise TypeError('src must be a (sum, wsum) pair of torch.Tensors (a (sum, wsum, count) triple is taken too; the count is not read)')
    ssum, swsum = src[:2]
    if vol_sum.dim() != 5:
        raise ValueError(f'vol_sum must be [R,X,Y,Z,C], got {tuple(vol_sum.shape)}')
    R, X, Y, Z, Cn = (int(v) for v in vol_sum.shape)
    rows = _host_ints(rows, 'rows')
    if not rows:
        raise ValueError('rows must name at least one row')
    B = len(rows)
    src_rows = _host_ints(src_rows, 'src_rows', B)
    if isinstance(transforms, (str, bytes, torch.Tensor)) or not hasattr(transforms, '__len__') or len(transforms) != B or \
            any(isinstance(c, (str, bytes)) or not hasattr(c, '__len__') for c in transforms):
        raise TypeError(f'transforms must be a host list of {B} lists (one per row) of 4x4 or 3x4 matrices')
    K = len(transforms[0])
    if K == 0 or any(len(c) != K for c in transforms):
        raise ValueError(f'transforms must hold the same number K >= 1 of candidates for every row, got {[len(c) for c in transforms]}')
    M = [check_rigid(T, f'transforms[{b}][{k}]') for b, cands in enumerate(transforms) for k, T in enumerate(cands)]
    origins, vs = _grid_floats(B, voxel_size, new_origin=new_origin, src_origin=src_origin, **({} if about is None else {'about': about}))
    o, so = origins[:2]
    step = _match_step(step)
    if any(not 0 <= r < R for r in rows):
        raise ValueError(f'rows must be in [0, {R}), got {rows}')
    if ssum.dim() != 5 or tuple(ssum.shape[1:]) != (X, Y, Z, Cn):
        raise ValueError(f'src[0] must be [R_src,{X},{Y},{Z},{Cn}] like vol_sum, got {tuple(ssum.shape)}')
    Rs = int(ssum.shape[0])
    if any(not 0 <= r < Rs for r in src_rows):
        raise ValueError(f'src_rows must be in [0, {Rs}), got {src_rows}')
    if Cn % 4:
        raise ValueError(f'vol_sum must have C % 4 == 0, got C = {Cn}')
    for t, name, shape in ((wsum, 'wsum', (R, X, Y, Z)), (swsum, 'src[1]', (Rs, X, Y, Z))):
        if tuple(t.shape) != shape:
            raise ValueError(f'{name} must be {list(shape)} beside its sums, got {tuple(t.shape)}')
    for t, name in ((vol_sum, 'vol_sum'), (wsum, 'wsum'), (ssum, 'src[0]'), (swsum, 'src[1]')):
        _chk(t, name)
        if t.device != vol_sum.device:
            raise ValueError(f'{name} must be on the device of vol_sum')
    L = _lib.lib()
    align = about is not None
    entry, version = ('ivx_volume_align', '0.5.8') if align else ('ivx_volume_match', '0.5.7')
    fn = getattr(L, entry + '_fwd', None)
    if fn is None:
        raise _lib.IvxError(f'this build of libimvoxel_hip.so has no {entry}_fwd (needs version {version})')
    nbytes = getattr(L, entry + '_scratch_bytes')(B, K, X, Y, Z, Cn)
    if nbytes < 0:
        raise ValueError(f'{entry}_scratch_bytes refuses B = {B}, K = {K}, grid {X} x {Y} x {Z}, C = {Cn}')
    dev = vol_sum.device
    scratch = torch.empty((nbytes // 8,), device=dev, dtype=torch.int64)
    pairs, own = torch.empty((B, K), device=dev, dtype=torch.int64), torch.empty((B,), device=dev, dtype=torch.int64)
    stats = torch.empty((B, K, 31 if align else 3), device=dev, dtype=torch.float64)
    flat = lambda a: (C.c_float * a.size)(*np.ascontiguousarray(a, np.float32).reshape(-1).tolist())     # noqa: E731
    lists = (B, K, (C.c_int32 * B)(*src_rows), (C.c_int32 * B)(*rows), flat(np.stack(M))) + ((flat(origins[2]),) if align else ()) + \
        (flat(o), flat(so), flat(vs), (C.c_int32 * 3)(*step), Rs, R, X, Y, Z, Cn, _ptr(ssum), _ptr(swsum), _ptr(vol_sum), _ptr(wsum))
    if align:
        used = torch.empty((B, K), device=dev, dtype=torch.int64)
        check(fn(*lists, _ptr(pairs), _ptr(used), _ptr(own), _ptr(stats), _ptr(scratch), _stream()), entry + '_fwd')
        return pairs, used, own, stats
    check(fn(*lists, _ptr(pairs), _ptr(own), _ptr(stats), _ptr(scratch), _stream()), entry + '_fwd')
    return pairs, own, stats


def volume_align(vol_sum, wsum, rows, src, src_rows, transforms, about, new_origin, src_origin, voxel_size, step=(1, 1, 1)):
    """Aligning scenes: the Gauss-Newton normal equations of the six degrees of freedom of a pose between rows of the state pools
    (ivx_volume_align_fwd, the ALIGN instantiation of the match kernel; include/imvoxel.h has the definition).  The arguments are volume_match's
    and go through the same checks; `about`, host floats [B,3] (or [3] for all), finite, is the point the rotation increments go through.  For
    sample b and candidate T (x_src = T x_dst), over the USED voxels -- paired, all eight corners of the sample inside the source grid and of
    positive weight sum -- and all channels, with r = b - a and J the derivative of b by a small motion (v, w) of the destination point,
    p -> p + v + w x (p - about):  e = sum r^2,  g = sum J r,  H = sum J J^T.
    -> (pairs [B,K] int64, used [B,K] int64, own [B] int64, stats [B,K,31] float64 = (dot, na, nb, e, g[6], H upper triangle row-major [21])) as
    device tensors; pairs, own, dot, na, nb are volume_match's bit for bit.  The step is the caller's (scene.solve_align):
    (H + damping diag H) delta = -g, the trial pose T @ scene.rigid_increment(delta, about)."""
    if about is None:
        raise TypeError('about must be host floats [B,3] (or [3] for all): the point the rotation increments go through')
    return _match_call(vol_sum, wsum, rows, src, src_rows, transforms, new_origin, src_origin, voxel_size, step, about)


_PACK_DT = {torch.float32: 0, torch.bfloat16: 1}     # the payload of a packed state: IVX_F32 (the sums, as words) | IVX_BF16 (the mean)


def _pack_pools(vol_sum, count, rows, wsum):
    """The checks the pack and the unpack share: pools vol_sum [R,X,Y,Z,C] fp32 / count [R,X,Y,Z] int32 (/ wsum [R,X,Y,Z] fp32) on one device, rows a
    non-empty host list of distinct integers in [0, R) -> (rows, (R, X, Y, Z, C))."""
    for t, name in ((vol_sum, 'vol_sum'), (count, 'count')) + (((wsum, 'wsum'),) if wsum is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f'{name} must be a torch.Tensor')
    if vol_sum.dim() != 5:
        raise ValueError(f'vol_sum must be [R,X,Y,Z,C], got {tuple(vol_sum.shape)}')
    R, X, Y, Z, Cn = (int(v) for v in vol_sum.shape)
    rows = _host_ints(rows, 'rows')
    if not rows:
        raise ValueError('rows must name at least one row')
    if len(set(rows)) != len(rows):
        raise ValueError(f'rows must be distinct, got {rows}')
    if any(not 0 <= r < R for r in rows):
        raise ValueError(f'rows must be in [0, {R}), got {rows}')
    if Cn % 4:
        raise ValueError(f'vol_sum must have C % 4 == 0, got C = {Cn}')
    if X * Y * Z >= 2 ** 31:
        raise ValueError(f'X*Y*Z must be below 2^31, got {X * Y * Z}')
    if tuple(count.shape) != (R, X, Y, Z):
        raise ValueError('count must be [R,X,Y,Z] for vol_sum [R,X,Y,Z,C]')
    if wsum is not None and tuple(wsum.shape) != (R, X, Y, Z):
        raise ValueError('wsum must be [R,X,Y,Z] for vol_sum [R,X,Y,Z,C]')
    return rows, (R, X, Y, Z, Cn)


def _pack_on_device(vol_sum, count, wsum):
    """... and the checks that end them: fp32 / int32, contiguous, on one HIP device."""
    _chk(vol_sum, 'vol_sum')
    _chk(count, 'count', torch.int32)
    if count.device != vol_sum.device:
        raise ValueError('count must be on the device of vol_sum')
    if wsum is not None:
        _chk(wsum, 'wsum')
        if wsum.device != vol_sum.device:
            raise ValueError('wsum must be on the device of vol_sum')


def _pack_call(vol_sum, count, rows, wsum, dims, dt, cap, outs):
    """One ivx_volume_pack_fwd; outs: (index, payload, wsum, count) device tensors or four Nones (cap == 0, the count-only form) -> n per row,
    read back (the one host sync of a pack)."""
    L = _lib.lib()
    fn = getattr(L, 'ivx_volume_pack_fwd', None)
    if fn is None:
        raise _lib.IvxError('this build of libimvoxel_hip.so has no ivx_volume_pack_fwd (needs version 0.5.6)')
    R, X, Y, Z, Cn = dims
    B, dev = len(rows), vol_sum.device
    nbytes = L.ivx_volume_pack_scratch_bytes(B, X, Y, Z)
    if nbytes < 0:
        raise ValueError(f'ivx_volume_pack_scratch_bytes refuses B = {B}, grid {X} x {Y} x {Z}')
    scratch = torch.empty((nbytes // 4,), device=dev, dtype=torch.int32)
    n_out = torch.empty((B,), device=dev, dtype=torch.int32)
    check(fn(B, (C.c_int32 * B)(*rows), R, X, Y, Z, Cn, _ptr(vol_sum), _ptr(count), _ptr(wsum), dt, cap, *(_ptr(t) for t in outs), _ptr(n_out), _ptr(scratch),
             _stream()), 'ivx_volume_pack_fwd')
    return [int(v) for v in n_out.tolist()]


def volume_pack_count(vol_sum, count, rows, wsum=None):
    """Scene snapshots: how many voxels of rows of the state pools hold evidence (the count-only form of ivx_volume_pack_fwd; include/imvoxel.h has
    the definition).  A voxel is kept iff its count word or its wsum word is non-zero, as raw 32-bit words.  rows: distinct host integers in [0, R).
    Only the two counting launches run; the pools are read only.  -> list of ints, one per row."""
    rows, dims = _pack_pools(vol_sum, count, rows, wsum)
    _pack_on_device(vol_sum, count, wsum)
    return _pack_call(vol_sum, count, rows, wsum, dims, 0, 0, (None,) * 4)


def volume_pack(vol_sum, count, rows, wsum=None, dtype=torch.float32):
    """Scene snapshots: the kept voxels of rows of the state pools vol_sum [R,X,Y,Z,C] fp32 / count [R,X,Y,Z] int32 (/ wsum [R,X,Y,Z] fp32) as
    records in ascending flat voxel index (ivx_volume_pack_fwd; include/imvoxel.h has the definition).  It counts, reads the counts back (the one
    host sync), allocates exactly max(n) records per row and packs.  dtype=torch.float32: the payload is the C sums, moved as words -- every bit
    pattern survives; torch.bfloat16: the payload is the mean S / den (den the weight sum, or the count without wsum), rounded once.  rows:
    distinct host integers in [0, R); rows not named are not read and the pools are read only.  -> per row (index int32 [n], payload [n,C], wsum
    fp32 [n] or None, count int32 [n]) as device tensors (views of the call's buffers); a call whose rows are all unseen returns empty tensors
    without a second call.  Every check comes before the C calls, so a call that raises changes nothing."""
    rows, dims = _pack_pools(vol_sum, count, rows, wsum)
    if dtype not in _PACK_DT:
        raise TypeError(f'dtype must be torch.float32 (the sums as words) or torch.bfloat16 (the mean), got {dtype!r}')
    _pack_on_device(vol_sum, count, wsum)
    n = _pack_call(vol_sum, count, rows, wsum, dims, _PACK_DT[dtype], 0, (None,) * 4)
    B, Cn, dev, cap = len(rows), dims[4], vol_sum.device, max(n)
    outs = (torch.empty((B, cap), device=dev, dtype=torch.int32), torch.empty((B, cap, Cn), device=dev, dtype=dtype),
            torch.empty((B, cap), device=dev, dtype=torch.float32) if wsum is not None else None, torch.empty((B, cap), device=dev, dtype=torch.int32))
    if cap:
        n2 = _pack_call(vol_sum, count, rows, wsum, dims, _PACK_DT[dtype], cap, outs)
        if n2 != n:
            raise _lib.IvxError(f'ivx_volume_pack_fwd: the pools changed between the count and the pack ({n} then {n2} kept voxels)')
    return [tuple(None if t is None else t[b, :n[b]] for t in outs) for b in range(B)]


def volume_unpack_(vol_sum, count, rows, records, wsum=None):
    """Scene snapshots: write rows of the state pools from packed records (ivx_volume_unpack_fwd; include/imvoxel.h has the definition): for sample b,
    voxel index[q] of row rows[b] takes record q of records[b] = (index int32 [n], payload [n,C] fp32 or bf16, wsum fp32 [n] or None, count int32
    [n]) -- what volume_pack returns, as device tensors or host tensors / numpy arrays (a bf16 payload on the host may be its uint16 words) -- and
    every other voxel of that row becomes unseen, all bits zero.  A bf16 payload restores S = float(m) * den.  The records carry a weight sum iff
    the pools have one.  Checked on the host before the one C call: each index list is strictly ascending and inside [0, X*Y*Z) (device lists are
    read back for it), dtypes, shapes and devices agree; a call that raises changes nothing.  Rows not named are neither read nor written.
    Returns (vol_sum, count) or (vol_sum, wsum, count)."""
    import numpy as np
    rows, (R, X, Y, Z, Cn) = _pack_pools(vol_sum, count, rows, wsum)
    if isinstance(records, torch.Tensor) or not hasattr(records, '__len__') or len(records) != len(rows):
        raise ValueError(f'records must hold one (index, payload, wsum, count) per row: {len(rows)} rows')
    B, dev, nvox = len(rows), vol_sum.device, X * Y * Z
    recs, dtype = [], None
    for b, rec in enumerate(records):
        if isinstance(rec, torch.Tensor) or not hasattr(rec, '__len__') or len(rec) != 4:
            raise ValueError(f'records[{b}] must be (index, payload, wsum or None, count)')
        idx, pay, ws, cnt = (None if t is None else t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t)) for t in rec)
        if idx is None or pay is None or cnt is None:
            raise ValueError(f'records[{b}]: index, payload and count are required')
        if pay.dtype == torch.uint16:
            pay = pay.view(torch.bfloat16)
        if idx.dtype != torch.int32 or cnt.dtype != torch.int32 or pay.dtype not in _PACK_DT or (ws is not None and ws.dtype != torch.float32):
            raise TypeError(f'records[{b}] must be (int32, float32 or bfloat16, float32 or None, int32), got ({idx.dtype}, {pay.dtype}, '
                            f'{None if ws is None else ws.dtype}, {cnt.dtype})')
        if dtype is not None and pay.dtype != dtype:
            raise TypeError(f'the payloads of one call must share a dtype, got {dtype} and {pay.dtype}')
        dtype = pay.dtype
        n = int(idx.shape[0]) if idx.dim() == 1 else -1
        if n < 0 or tuple(pay.shape) != (n, Cn) or tuple(cnt.shape) != (n,) or (ws is not None and tuple(ws.shape) != (n,)):
            raise ValueError(f'records[{b}] must be index [n], payload [n,{Cn}], wsum [n] or None, count [n], got {tuple(idx.shape)}, {tuple(pay.shape)}, '
                             f'{None if ws is None else tuple(ws.shape)}, {tuple(cnt.shape)}')
        if (ws is None) != (wsum is None):
            raise ValueError(f'records[{b}]: the records must carry a weight sum iff the pools have one (wsum=)')
        for t in (idx, pay, ws, cnt):
            if t is not None and t.is_cuda and t.device != dev:
                raise ValueError(f'records[{b}] lies on {t.device}, the pools on {dev}')
        if n:
            host = idx.cpu().numpy().astype(np.int64)
            if host[0] < 0 or host[-1] >= nvox or (np.diff(host) <= 0).any():
                raise ValueError(f'records[{b}]: the indices must be strictly ascending inside [0, {nvox})')
        recs.append((idx, pay, ws, cnt, n))
    _pack_on_device(vol_sum, count, wsum)
    fn = getattr(_lib.lib(), 'ivx_volume_unpack_fwd', None)
    if fn is None:
        raise _lib.IvxError('this build of libimvoxel_hip.so has no ivx_volume_unpack_fwd (needs version 0.5.6)')
    ns = [r[4] for r in recs]
    cap = max(ns)
    bufs = (None,) * 4
    if cap:
        if B == 1 and all(t is None or (t.is_cuda and t.is_contiguous()) for t in recs[0][:4]):
            bufs = recs[0][:4]                    # one row whose records are on the device already: they are the call's lists
        else:                                     # [B,cap] lists, filled per row (host records: one upload each)
            bufs = (torch.empty((B, cap), device=dev, dtype=torch.int32), torch.empty((B, cap, Cn), device=dev, dtype=dtype),
                    torch.empty((B, cap), device=dev, dtype=torch.float32) if wsum is not None else None, torch.empty((B, cap), device=dev, dtype=torch.int32))
            for b, rec in enumerate(recs):
                for buf, t in zip(bufs, rec[:4]):
                    if buf is not None and rec[4]:
                        buf[b, :rec[4]].copy_(t)
    check(fn(B, (C.c_int32 * B)(*rows), (C.c_int32 * B)(*ns), cap, _ptr(bufs[0]), _ptr(bufs[1]), _ptr(bufs[2]), _ptr(bufs[3]), _PACK_DT[dtype or torch.float32],
             R, X, Y, Z, Cn, _ptr(vol_sum), _ptr(count), _ptr(wsum), _stream()), 'ivx_volume_unpack_fwd')
    return (vol_sum, count) if wsum is None else (vol_sum, wsum, count)


_STATE_KIND = {torch.int32: _lib.STATE_COUNT, torch.float32: _lib.STATE_WSUM, torch.uint8: _lib.STATE_MASK, torch.bool: _lib.STATE_MASK}
MAX_COVERAGE_VIEWS = 256      # candidates per sample of one view_coverage call (the kernel's counters live in LDS)


def view_coverage(proj_pool, lists, rows, new_origin, crop_hw, voxel_size, n_voxels, fhw, state=None, fresh_below=1.0, pixel_weight=None, depth=None,
                  gate=None, out=None):
    """View coverage (ivx_view_coverage_fwd; include/imvoxel.h has the definition): for sample b (a scene) and each candidate view of lists[b] --
    slots of proj_pool [S,3,4], -1 pads -- the number of voxels of the grid n_voxels = (X, Y, Z) at (new_origin[b], crop_hw[b], voxel_size) the
    lift would count the view at, and how many of those hold less than fresh_below of evidence in row rows[b] of `state`.  The decision is the
    lift's own, bit for bit, with the maps pixel_weight / depth [S,FH,FW] (or [S,1,FH,FW]; None: no map) and gate = (behind, front) (None: no
    limit) of backproject_mapped_accum_; fhw = (FH, FW) is the feature-map size the crop is clamped to.  state: None (an empty scene: every seen
    voxel is fresh; R = max(rows) + 1), or a device tensor [R,X,Y,Z]: int32 view counts, float32 weight sums, or uint8 / bool valid mask.  fresh =
    not (evidence >= fresh_below); fresh_below finite and > 0.  lists and rows are host lists, checked as the listed lifts check them (rows
    distinct and in range) and uploaded in ONE copy; nothing but the result is written.  out: a device int32 tensor [B,V,2] to write into (V = the
    longest list), zeroed by the call.  Returns out [B,V,2] int32 on the device: (seen, fresh) per candidate, (0, 0) for padding.  Integer
    counting: the result does not depend on the order of arrival.  Every argument error is raised before any launch."""
    if not isinstance(proj_pool, torch.Tensor):
        raise TypeError('proj_pool must be a torch.Tensor')
    if proj_pool.dim() != 3 or tuple(proj_pool.shape[1:]) != (3, 4) or proj_pool.shape[0] < 1:
        raise ValueError(f'proj_pool must be [S,3,4] with S >= 1, got {tuple(proj_pool.shape)}')
    S = int(proj_pool.shape[0])
    if isinstance(lists, torch.Tensor) or not hasattr(lists, '__len__') or len(lists) < 1:
        raise TypeError('lists must be a host list of B >= 1 lists of slots')
    lists = [_host_ints(l, f'lists[{b}]') for b, l in enumerate(lists)]
    B = len(lists)
    bad = sorted({v for l in lists for v in l if v != -1 and not 0 <= v < S})
    if bad:
        raise ValueError(f'lists hold slots outside [0, {S}) other than the padding -1: {bad}')
    V = max(1, max(len(l) for l in lists))
    if V > MAX_COVERAGE_VIEWS:
        raise ValueError(f'{V} candidate views for one sample (at most {MAX_COVERAGE_VIEWS} per call)')
    rows = _host_ints(rows, 'rows', B)
    if len(set(rows)) != B:
        raise ValueError(f'rows must be distinct (two samples on one row race), got {rows}')
    X, Y, Z = _host_ints(n_voxels, 'n_voxels', 3)
    FH, FW = _host_ints(fhw, 'fhw', 2)
    if min(X, Y, Z, FH, FW) < 1:
        raise ValueError(f'n_voxels and fhw must be positive, got {(X, Y, Z)} and {(FH, FW)}')
    if state is None:
        kind, R = _lib.STATE_NONE, max(rows) + 1
    else:
        if not isinstance(state, torch.Tensor):
            raise TypeError('state must be None or a torch.Tensor [R,X,Y,Z]')
        if state.dtype not in _STATE_KIND:
            raise TypeError(f'state must be int32 (counts), float32 (weight sums) or uint8 / bool (valid mask), got {state.dtype}')
        if state.dim() != 4 or tuple(state.shape[1:]) != (X, Y, Z):
            raise ValueError(f'state must be [R,X,Y,Z] = [R,{X},{Y},{Z}] for this grid, got {tuple(state.shape)}')
        kind, R = _STATE_KIND[state.dtype], int(state.shape[0])
    if any(not 0 <= r < R for r in rows):
        raise ValueError(f'rows must be in [0, {R}), got {rows}' if state is not None else f'rows must be >= 0, got {rows}')
    if isinstance(fresh_below, bool) or not hasattr(fresh_below, '__float__') or isinstance(fresh_below, torch.Tensor) \
            or not (math.isfinite(float(fresh_below)) and float(fresh_below) > 0):
        raise ValueError(f'fresh_below must be a finite number > 0, got {fresh_below!r}')
    gate = check_gate(gate) if gate is not None else (math.inf, math.inf)
    mdev = {}
    for name, t in (('pixel_weight', pixel_weight), ('depth', depth)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f'{name} must be None or a torch.Tensor [S,FH,FW]')
        if t.dim() == 4 and t.shape[1] == 1:
            t = t[:, 0]
        if tuple(t.shape) != (S, FH, FW):
            raise ValueError(f'{name} must be [S,FH,FW] = [{S},{FH},{FW}] (or [S,1,FH,FW]) for this pool, got {tuple(t.shape)}')
        mdev[name] = t
    if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != (B, V, 2)):
        raise ValueError(f'out must be an int32 tensor [B,V,2] = [{B},{V},2]')
    _chk(proj_pool, 'proj_pool')
    for name, t in mdev.items():
        _chk(t, name)
    _chk(new_origin, 'new_origin')
    _chk(crop_hw, 'crop_hw', torch.int32)
    if tuple(new_origin.shape) != (B, 3) or tuple(crop_hw.shape) != (B, 2):
        raise ValueError('new_origin must be [B,3] and crop_hw [B,2] for the B lists')
    if state is not None:
        _chk(state, 'state', state.dtype)
    if out is None:
        out = torch.empty((B, V, 2), device=proj_pool.device, dtype=torch.int32)
    else:
        _chk(out, 'out', torch.int32)
    fn = getattr(_lib.lib(), 'ivx_view_coverage_fwd', None)
    if fn is None:
        raise _lib.IvxError('this build of libimvoxel_hip.so has no ivx_view_coverage_fwd (needs version 0.5.1)')
    # the one upload: view_slot [B,V] (-1 padded), then row [B] (`dev` is released in stream order: the allocator reuses it after this launch)
    dev = torch.tensor([v for l in lists for v in l + [-1] * (V - len(l))] + rows, dtype=torch.int32).to(proj_pool.device)
    p0 = dev.data_ptr()
    d = _lib.BackprojectDesc(B, V, FH, FW, 0, X, Y, Z, (C.c_float * 3)(*[float(v) for v in voxel_size]), 0, 0, 0, 0)
    l = _lib.LiftLists(S, R, p0, p0 + 4 * B * V, None)
    m = _lib.LiftMaps(_ptr(mdev.get('pixel_weight')), _ptr(mdev.get('depth')), *gate)
    check(fn(C.byref(d), C.byref(l), C.byref(m), _ptr(proj_pool), _ptr(new_origin), _ptr(crop_hw), _ptr(state), kind, float(fresh_below), _ptr(out), _stream()),
          'ivx_view_coverage_fwd')
    return out


# ------------------------------------------------------------------ detection tail
def anchor_head_get_bboxes(head_out, anchors, H, W, num_anchors, num_classes, offs, cfg, dir_offset=0.0,
                           dir_limit_offset=1.0, hw_transposed=False, want_candidates=False):
    """head_out [B,*,*,CH] channels-last map of the fused head conv; anchors [H*W*A,7].
    Returns (boxes [B,max_num,7], scores [B,max_num], labels [B,max_num] int64, count [B] int32[, cands])."""
    _chk(head_out, 'head_out')
    _chk(anchors, 'anchors')
    B, CH = head_out.shape[0], head_out.shape[-1]
    if head_out.numel() != B * H * W * CH:
        raise ValueError('head_out does not hold B*H*W*CH values')
    if anchors.shape[0] != H * W * num_anchors or anchors.shape[1] != 7:
        raise ValueError('anchors must be [H*W*A, 7]')
    nms_pre, max_num = int(cfg['nms_pre']), int(cfg['max_num'])
    d = AnchorHeadDesc(B, H, W, CH, num_anchors, num_classes, offs[0], offs[1], offs[2], nms_pre, max_num,
                       int(bool(cfg['use_rotate_nms'])), int(bool(hw_transposed)), float(cfg.get('score_thr', 0)),
                       float(cfg['nms_thr']), float(dir_offset), float(dir_limit_offset))
    L = _lib.lib()
    ws_bytes = L.ivx_anchor_head_workspace_bytes(C.byref(d))
    if ws_bytes < 0:
        check(-1, 'ivx_anchor_head_workspace_bytes')
    ws = torch.empty((ws_bytes,), device=head_out.device, dtype=torch.uint8)
    boxes = torch.empty((B, max_num, 7), device=head_out.device, dtype=torch.float32)
    scores = torch.empty((B, max_num), device=head_out.device, dtype=torch.float32)
    labels = torch.empty((B, max_num), device=head_out.device, dtype=torch.int64)
    count = torch.empty((B,), device=head_out.device, dtype=torch.int32)
    ci = cb = cs = None
    if want_candidates:
        ci = torch.empty((B, nms_pre), device=head_out.device, dtype=torch.int64)
        cb = torch.empty((B, nms_pre, 7), device=head_out.device, dtype=torch.float32)
        cs = torch.empty((B, nms_pre), device=head_out.device, dtype=torch.float32)
    check(L.ivx_anchor_head_get_bboxes(C.byref(d), _ptr(head_out), _ptr(anchors), _ptr(ws), ws_bytes, _ptr(boxes),
                                       _ptr(scores), _ptr(labels), _ptr(count), _ptr(ci), _ptr(cb), _ptr(cs), _stream()),
          'ivx_anchor_head_get_bboxes')
    if want_candidates:
        return boxes, scores, labels, count, (ci, cb, cs)
    return boxes, scores, labels, count


def nms_bev_sorted(boxes_sorted, thresh, rotated=True):
    """boxes [n,5] sorted by descending score -> (keep [n] int64, num [1] int32) device tensors."""
    _chk(boxes_sorted, 'boxes')
    n = boxes_sorted.shape[0]
    L = _lib.lib()
    ws_bytes = L.ivx_nms_workspace_bytes(n)
    ws = torch.empty((max(int(ws_bytes), 256),), device=boxes_sorted.device, dtype=torch.uint8)
    keep = torch.empty((max(n, 1),), device=boxes_sorted.device, dtype=torch.int64)
    num = torch.empty((1,), device=boxes_sorted.device, dtype=torch.int32)
    check(L.ivx_nms_bev(_ptr(boxes_sorted), n, float(thresh), int(bool(rotated)), _ptr(ws), ws.numel(), _ptr(keep),
                        _ptr(num), _stream()), 'ivx_nms_bev')
    return keep, num


def multiclass_nms_bev(boxes, scores, num_classes, score_thr, nms_thr, rotated, max_num):
    """boxes [n,5] BEV (x1,y1,x2,y2,ry), scores [n, >= num_classes] -> (idx [m] int64 into the n candidates,
    labels [m] int64, count [1] int32), all on the device; m = min(max_num, n * num_classes) slots, `count` valid."""
    _chk(boxes, 'boxes')
    _chk(scores, 'scores')
    n = boxes.shape[0]
    if scores.shape[0] != n or scores.shape[1] < num_classes or boxes.shape[1] != 5:
        raise ValueError('boxes must be [n,5] and scores [n, >= num_classes]')
    L = _lib.lib()
    wsb = L.ivx_multiclass_nms_workspace_bytes(n, int(num_classes))
    if wsb < 0:
        check(-1, 'ivx_multiclass_nms_workspace_bytes')
    ws = torch.empty((max(int(wsb), 256),), device=boxes.device, dtype=torch.uint8)
    m = max(1, min(int(max_num), n * int(num_classes)))
    idx = torch.empty((m,), device=boxes.device, dtype=torch.int64)
    lab = torch.empty((m,), device=boxes.device, dtype=torch.int64)
    cnt = torch.empty((1,), device=boxes.device, dtype=torch.int32)
    check(L.ivx_multiclass_nms_bev(_ptr(boxes), _ptr(scores), n, scores.shape[1], int(num_classes), float(score_thr), float(nms_thr),
                                   int(bool(rotated)), int(max_num), _ptr(ws), ws.numel(), _ptr(idx), _ptr(lab), _ptr(cnt), _stream()),
          'ivx_multiclass_nms_bev')
    return idx, lab, cnt


def indoor_tail(cand_boxes, cand_scores, n_classes, score_thr, nms_thr, use_rotate_nms=False, max_num=None):
    """Cross-level tail of the anchor-free indoor heads (ivx_indoor_tail_get_bboxes): cand_boxes / cand_scores = per-level lists of
    [B, k_l, R] / [B, k_l, n_classes] device tensors (R = 6 ScanNet corners, 7 SUN RGB-D boxes) -> (boxes [B,M,7] rows of the box
    object's tensor (bottom-face z), scores [B,M], labels int64 [B,M], count int32 [B]); M = sum(k_l) for ScanNet, max_num (the
    reference passes test_cfg.nms_pre) capped at sum(k_l) * n_classes for SUN RGB-D."""
    from ._lib import IndoorTailDesc
    L = _lib.lib()
    B, R = cand_boxes[0].shape[0], cand_boxes[0].shape[2]
    d = IndoorTailDesc()
    d.B, d.n_levels, d.n_classes, d.n_reg = B, len(cand_boxes), int(n_classes), R
    K = 0
    for l, (cb, cs) in enumerate(zip(cand_boxes, cand_scores)):
        _chk(cb, 'cand_boxes')
        _chk(cs, 'cand_scores')
        if cb.shape[0] != B or cs.shape[:2] != cb.shape[:2] or cs.shape[2] != n_classes or cb.shape[2] != R:
            raise ValueError('candidate lists must be [B, k, R] / [B, k, n_classes] per level')
        d.k[l] = cb.shape[1]
        K += cb.shape[1]
    M = K if R == 6 else max(1, min(int(max_num if max_num is not None else K), K * int(n_classes)))
    d.use_rotate_nms, d.max_num, d.score_thr, d.nms_thr = int(bool(use_rotate_nms)), M, float(score_thr), float(nms_thr)
    wsb = L.ivx_indoor_tail_workspace_bytes(C.byref(d))
    if wsb < 0:
        check(-1, 'ivx_indoor_tail_workspace_bytes')
    dev = cand_boxes[0].device
    ws = torch.empty((max(int(wsb), 256),), device=dev, dtype=torch.uint8)
    boxes, scores = torch.empty((B, M, 7), device=dev, dtype=torch.float32), torch.empty((B, M), device=dev, dtype=torch.float32)
    labels, count = torch.empty((B, M), device=dev, dtype=torch.int64), torch.empty((B,), device=dev, dtype=torch.int32)
    pb = (C.c_void_p * 4)(*([t.data_ptr() for t in cand_boxes] + [None] * (4 - len(cand_boxes))))
    ps = (C.c_void_p * 4)(*([t.data_ptr() for t in cand_scores] + [None] * (4 - len(cand_scores))))
    check(L.ivx_indoor_tail_get_bboxes(C.byref(d), pb, ps, _ptr(ws), ws.numel(), _ptr(boxes), _ptr(scores), _ptr(labels), _ptr(count), _stream()),
          'ivx_indoor_tail_get_bboxes')
    return boxes, scores, labels, count


def boxes_overlap_bev(a, b, iou=False):
    _chk(a, 'a')
    _chk(b, 'b')
    out = torch.zeros((a.shape[0], b.shape[0]), device=a.device, dtype=torch.float32)
    check(_lib.lib().ivx_boxes_overlap_bev(_ptr(a), a.shape[0], _ptr(b), b.shape[0], int(bool(iou)), _ptr(out), _stream()),
          'ivx_boxes_overlap_bev')
    return out


def aligned_3d_nms_dev(boxes, scores, classes, thresh, single_workgroup=False):
    _chk(boxes, 'boxes')
    _chk(scores, 'scores')
    _chk(classes, 'classes', torch.int64)
    n = boxes.shape[0]
    pick = torch.empty((max(n, 1),), device=boxes.device, dtype=torch.int64)
    num = torch.empty((1,), device=boxes.device, dtype=torch.int32)
    L = _lib.lib()
    if single_workgroup:
        check(L.ivx_aligned_3d_nms(_ptr(boxes), _ptr(scores), _ptr(classes), n, float(thresh), _ptr(pick), _ptr(num), _stream()),
              'ivx_aligned_3d_nms')
        return pick, num
    wsb = L.ivx_aligned_3d_nms_workspace_bytes(n)
    if wsb < 0:
        raise ValueError(f'ivx_aligned_3d_nms_ws: at most 65536 boxes (got {n})')
    ws = torch.empty((wsb,), device=boxes.device, dtype=torch.uint8)
    check(L.ivx_aligned_3d_nms_ws(_ptr(boxes), _ptr(scores), _ptr(classes), n, float(thresh), _ptr(ws), wsb, _ptr(pick), _ptr(num),
                                  _stream()), 'ivx_aligned_3d_nms_ws')
    return pick, num
