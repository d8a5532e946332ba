"""Input side of the path: checkpoint loading, the test-time image pipeline and the
on-disk calibration -> `lidar2img` adapters.  Host-side numpy/torch, except prepare_images_device, which runs the image pipeline
of prepare_image on the device (ops.image_prep_u8) and is held to prepare_image bit for bit; with lens= (a Lens record: a real camera's
intrinsic and distortion) it undistorts in the same launch (ops.image_prep_lens_u8), held to an fp64 reference within a derived bound.

Reference: configs/imvoxelnet/imvoxelnet_kitti.py:66,94-105 (Resize keep_ratio -> Normalize -> Pad(size_divisor=32)),
mmdet3d/datasets/{kitti,nuscenes,scannet,sunrgbd}_monocular_dataset.py (lidar2img), pipelines/multi_view.py:45-53
(KittiSetOrigin, SunRgbdSetOrigin), pipelines/multi_view.py:7-31 (MultiViewPipeline view sampling).
mmcv / cv2 are not installed here: the resize restates cv2.resize(INTER_LINEAR) on uint8 images -- the 11-bit fixed-point
coefficient tables, the int32 horizontal pass, the `>> 4 ... >> 16 ... + 2 >> 2` vertical pass and the exact-half
INTER_AREA shortcut -- from OpenCV's published algorithm (imgproc/resize.cpp); it is checked against hand-derived vectors
(tests/test_host_cpu.py), not against cv2 itself: parity of the resize stays UNPINNED.
"""
import numpy as np
import torch
import torch.nn.functional as F

IMG_NORM_CFG = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)


# ------------------------------------------------------------------ checkpoints
def torch_load_trusted(filename, map_location='cpu', trusted=None):
    """torch.load for mmcv-style .pth files: `weights_only=True` first (tensors, dicts, strings and numbers -- what a released
    ImVoxelNet checkpoint holds -- load under it; nothing in the file is executed).  Files that carry other pickled objects
    (an optimizer's param-group classes, numpy scalars in 'meta') need the full unpickler, which can run arbitrary code from
    the file: that fallback is taken only when the caller vouches for the file -- `trusted=True`, or IVX_TRUST_CHECKPOINT=1
    in the environment (what mmcv.runner.load_checkpoint does unconditionally)."""
    import os
    import pickle
    try:
        return torch.load(filename, map_location=map_location, weights_only=True)
    except TypeError:           # torch < 1.13: no weights_only argument
        return torch.load(filename, map_location=map_location)
    except (pickle.UnpicklingError, RuntimeError) as e:
        if trusted is None:
            trusted = os.environ.get('IVX_TRUST_CHECKPOINT', '0') == '1'
        if not trusted:
            raise RuntimeError(f'{filename}: not loadable with weights_only=True ({str(e).splitlines()[0][:160]}); if you trust the '
                               'file, pass trusted=True (or set IVX_TRUST_CHECKPOINT=1) to unpickle it fully') from e
        return torch.load(filename, map_location=map_location, weights_only=False)


def load_checkpoint(model, filename, map_location='cpu', strict=False, trusted=None):
    """mmcv.runner.load_checkpoint for the released ImVoxelNet .pth files: a dict with 'state_dict' (and 'meta'),
    keys optionally prefixed with 'module.'.  Returns the checkpoint dict.  A model that was already prepared is re-packed for
    the device by its load_state_dict hook; otherwise call model.prepare(device) (or just run it).  trusted: see torch_load_trusted."""
    ckpt = torch_load_trusted(filename, map_location=map_location, trusted=trusted)
    sd = ckpt.get('state_dict', ckpt) if isinstance(ckpt, dict) else ckpt
    sd = {(k[7:] if k.startswith('module.') else k): v for k, v in sd.items()}
    res = model.load_state_dict(sd, strict=False)
    missing = [k for k in res.missing_keys if not k.endswith('num_batches_tracked')]
    if strict and (missing or res.unexpected_keys):
        raise RuntimeError(f'checkpoint mismatch: missing {missing[:8]}, unexpected {list(res.unexpected_keys)[:8]}')
    if isinstance(ckpt, dict) and 'meta' in ckpt and 'CLASSES' in ckpt['meta']:
        model.CLASSES = ckpt['meta']['CLASSES']          # tools/test.py:122-125
    ckpt['_missing_keys'], ckpt['_unexpected_keys'] = missing, list(res.unexpected_keys)
    return ckpt


# ------------------------------------------------------------------ image pipeline
def rescale_size(old_hw, scale):
    """mmcv.rescale_size for a (w, h) tuple scale: largest size keeping the aspect ratio inside `scale`."""
    h, w = old_hw
    max_long, max_short = max(scale), min(scale)
    f = min(max_long / max(h, w), max_short / min(h, w))
    return int(h * float(f) + 0.5), int(w * float(f) + 0.5)


def _linear_tables(src, dst):
    """cv2 resize.cpp, INTER_LINEAR coefficient tables for one axis: source index and the two 11-bit weights per output
    position.  fx = (d + 0.5) * (src / dst) - 0.5 in FLOAT, sx = floor(fx); clamped at both borders; weights =
    round((1 - fx, fx) * 2048) as int16."""
    scale = float(src) / float(dst)
    d = np.arange(dst, dtype=np.float64)
    fx = ((d + 0.5) * scale - 0.5).astype(np.float32)
    sx = np.floor(fx).astype(np.int64)
    fx = (fx - sx.astype(np.float32)).astype(np.float32)
    lo = sx < 0
    sx[lo], fx[lo] = 0, 0.0
    hi = sx >= src - 1
    sx[hi], fx[hi] = src - 1, 0.0
    a1 = np.rint(fx * np.float32(2048.0)).astype(np.int64)           # cvRound: round half to even
    a0 = np.rint((np.float32(1.0) - fx) * np.float32(2048.0)).astype(np.int64)
    return sx, np.minimum(sx + 1, src - 1), a0, a1


def imresize_cv2_linear(img_u8, size_hw):
    """cv2.resize(img, (w, h), interpolation=cv2.INTER_LINEAR) for an (H, W, C) uint8 image (what mmcv.imresize runs inside
    mmdet's Resize: imvoxelnet_kitti.py:98), in integer arithmetic:
      horizontal: D[x] = S[sx] * a0 + S[sx+1] * a1                                  (int32, weights sum to 2048)
      vertical:   dst  = (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2
    An exact 2x down-scale on both axes takes OpenCV's INTER_AREA shortcut: (a + b + c + d + 2) >> 2."""
    img = np.ascontiguousarray(img_u8)
    if img.dtype != np.uint8 or img.ndim != 3:
        raise TypeError('imresize_cv2_linear expects an (H, W, C) uint8 image')
    h, w = img.shape[:2]
    nh, nw = int(size_hw[0]), int(size_hw[1])
    if (nh, nw) == (h, w):
        return img.copy()
    if h == 2 * nh and w == 2 * nw:
        q = img.astype(np.int64).reshape(nh, 2, nw, 2, img.shape[2])
        return ((q.sum(axis=(1, 3)) + 2) >> 2).astype(np.uint8)
    sx, sx1, a0, a1 = _linear_tables(w, nw)
    sy, sy1, b0, b1 = _linear_tables(h, nh)
    src = img.astype(np.int64)
    rows = src[:, sx] * a0[None, :, None] + src[:, sx1] * a1[None, :, None]        # [h, nw, C], up to 255 * 2048
    d0, d1 = rows[sy] >> 4, rows[sy1] >> 4
    out = (((b0[:, None, None] * d0) >> 16) + ((b1[:, None, None] * d1) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def prepare_image(img_bgr_u8, img_scale, img_norm_cfg=IMG_NORM_CFG, size_divisor=32, keep_ratio=True):
    """LoadImageFromFile -> Resize -> Normalize -> Pad for ONE image (H,W,3 uint8, BGR as cv2 loads it).
    Returns (tensor [3,Hp,Wp] fp32, meta dict with img_shape / ori_shape / pad_shape as the mmdet pipeline sets them)."""
    ori_shape = tuple(img_bgr_u8.shape)
    if keep_ratio:
        nh, nw = rescale_size(ori_shape[:2], img_scale)
    else:
        nw, nh = img_scale
    resized = imresize_cv2_linear(img_bgr_u8, (nh, nw))                    # uint8 in, uint8 out, as mmcv.imresize
    img = torch.from_numpy(resized).float().permute(2, 0, 1)[None]
    mean = torch.tensor(img_norm_cfg['mean'], dtype=torch.float32).view(1, 3, 1, 1)
    std = torch.tensor(img_norm_cfg['std'], dtype=torch.float32).view(1, 3, 1, 1)
    if img_norm_cfg.get('to_rgb', True):
        img = img[:, [2, 1, 0]]
    img = (img - mean) / std
    ph = (nh + size_divisor - 1) // size_divisor * size_divisor
    pw = (nw + size_divisor - 1) // size_divisor * size_divisor
    img = F.pad(img, (0, pw - nw, 0, ph - nh))
    return img[0], dict(img_shape=(nh, nw, 3), ori_shape=ori_shape, pad_shape=(ph, pw, 3))


def _pipeline_shapes(ori_hw, img_scale, size_divisor, keep_ratio):
    """(resized (h, w), own padded (h, w)) of one frame, as prepare_image computes them."""
    if keep_ratio:
        nh, nw = rescale_size(ori_hw, img_scale)
    else:
        nw, nh = img_scale
    return (nh, nw), ((nh + size_divisor - 1) // size_divisor * size_divisor, (nw + size_divisor - 1) // size_divisor * size_divisor)


class Lens:
    """A real camera and the ideal one its undistorted image shows (include/imvoxel.h, ivx_lens): a small checked record.
    model: 'brown' (OpenCV's 5-coefficient model, coef = (k1, k2, p1, p2, k3); four coefficients mean k3 = 0) or 'fisheye' (OpenCV's
    equidistant model, coef = (k1, k2, k3, k4)).  K: the real camera's intrinsic, at least 3x3, zero skew, in pixels of the SOURCE frame.
    new_K: the ideal pinhole camera of the undistorted image at the source size (None: K) -- what the lidar2img intrinsic of the metas must
    describe.  r2_max: the normalised radius squared beyond which the polynomial is not trusted (> 0; inf: no limit); pixels beyond it are
    border.  Immutable; `key` is hashable and equal for equal lenses, so frames group by it and scenes cache by it."""
    MODELS = {'brown': 0, 'fisheye': 1}

    def __init__(self, model, K, coef, new_K=None, r2_max=float('inf')):
        if model not in self.MODELS:
            raise ValueError(f"model must be 'brown' or 'fisheye', got {model!r}")
        cams = []
        for name, M in (('K', K), ('new_K', K if new_K is None else new_K)):
            M = np.asarray(M, np.float64)
            if M.ndim != 2 or M.shape[0] < 3 or M.shape[1] < 3:
                raise ValueError(f'{name} must be at least 3x3, got {M.shape}')
            fx, fy, cx, cy = float(M[0, 0]), float(M[1, 1]), float(M[0, 2]), float(M[1, 2])
            if not all(np.isfinite(v) for v in (fx, fy, cx, cy)) or fx == 0 or fy == 0:
                raise ValueError(f'{name} must hold finite entries and non-zero focal lengths, got fx {fx}, fy {fy}, cx {cx}, cy {cy}')
            if M[0, 1] != 0 or M[1, 0] != 0 or M[2, 0] != 0 or M[2, 1] != 0 or M[2, 2] != 1:
                raise ValueError(f'{name} must be a pinhole intrinsic without skew ([[fx,0,cx],[0,fy,cy],[0,0,1]])')
            cams.append((fx, fy, cx, cy))
        c = [float(v) for v in np.asarray(coef, np.float64).reshape(-1)]
        want = (4, 5) if model == 'brown' else (4,)
        if len(c) not in want:
            raise ValueError(f'a {model} lens takes {" or ".join(str(n) for n in want)} coefficients, got {len(c)}')
        if not all(np.isfinite(v) for v in c):
            raise ValueError(f'coefficients must be finite, got {c}')
        r2_max = float(r2_max)
        if not r2_max > 0:
            raise ValueError(f'r2_max must be > 0 (inf: no limit), got {r2_max}')
        self._key = (model, cams[0], tuple(c + [0.0] * (5 - len(c))), cams[1], r2_max)

    model = property(lambda self: self._key[0])
    coef = property(lambda self: self._key[2])
    r2_max = property(lambda self: self._key[4])
    key = property(lambda self: self._key)

    @staticmethod
    def _matrix(cam):
        fx, fy, cx, cy = cam
        return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)

    K = property(lambda self: self._matrix(self._key[1]))
    new_K = property(lambda self: self._matrix(self._key[3]))

    def __eq__(self, other):
        return isinstance(other, Lens) and self._key == other._key

    def __hash__(self):
        return hash(self._key)

    def __repr__(self):
        return f'Lens{self._key!r}'

    def struct(self):
        """The ivx_lens of this record."""
        import ctypes
        from ._lib import Lens as CLens
        model, k, c, nk, r2 = self._key
        return CLens(self.MODELS[model], *k, (ctypes.c_double * 5)(*c), *nk, r2)


def _check_lenses(lens, n):
    """lens of prepare_images_device -> None (no lens anywhere) or a list of n entries, each a Lens or None."""
    if lens is None:
        return None
    if isinstance(lens, Lens):
        return [lens] * n
    lens = list(lens)
    if len(lens) != n:
        raise ValueError(f'{len(lens)} lenses for {n} frames (one Lens for all, or one entry per frame)')
    for l in lens:
        if l is not None and not isinstance(l, Lens):
            raise TypeError(f'every lens entry must be a data.Lens or None, got {type(l).__name__}')
    return lens


def _yuv_rows():
    """The named integer matrices of ivx_yuv_matrix (include/imvoxel.h): (y_off, cy, cub, cug, cvg, cvr) by (standard, full_range).  BT.601
    limited range is OpenCV's table by value; the others are the exact matrix times 2^20 rounded half to even (Fraction arithmetic;
    Python's round() on a Fraction rounds half to even)."""
    from fractions import Fraction as Fr
    rows = {}
    for std, (kr, kb) in (('bt601', (Fr(299, 1000), Fr(114, 1000))), ('bt709', (Fr(2126, 10000), Fr(722, 10000)))):
        kg = 1 - kr - kb
        for full in (False, True):
            cy, s, y_off = (Fr(1), Fr(1), 0) if full else (Fr(255, 219), Fr(255, 224), 16)
            m = (cy, 2 * s * (1 - kb), -2 * s * kb * (1 - kb) / kg, -2 * s * kr * (1 - kr) / kg, 2 * s * (1 - kr))
            rows[(std, full)] = (y_off,) + tuple(int(round(v * (1 << 20))) for v in m)
    rows[('bt601', False)] = (16, 1220542, 2116026, -409993, -852492, 1673527)
    return rows


class FrameFormat:
    """The pixel format of a source frame (include/imvoxel.h, ivx_frame_format): a small checked record.
    layout: 'bgr' | 'rgb' (3 bytes / pixel), 'bgra' | 'rgba' (4 bytes, byte 3 ignored), 'gray' (1 byte), 'nv12' (a Y plane and an interleaved
    half-resolution UV plane), 'yuyv' (packed 4:2:2).  yuv (YUV layouts only): 'bt601' | 'bt709' with full_range, or the six integers
    (y_off, cy, cub, cug, cvg, cvr) of another standard, 20 fractional bits, |coefficient| <= 3 << 20 and 0 <= y_off <= 255.
    Immutable; `key` is hashable and equal for equal formats, so frames group by it.  The frame arrays of each layout: (H,W,3), (H,W,4),
    (H,W) or (H,W,1), (H + ceil(H/2), W) with even W (the stacked NV12 array), (H,W,2) with even W."""
    LAYOUTS = {'bgr': 0, 'rgb': 1, 'bgra': 2, 'rgba': 3, 'gray': 4, 'nv12': 5, 'yuyv': 6}
    COEF_MAX = 3 << 20
    _rows = None

    def __init__(self, layout, yuv='bt601', full_range=False):
        if isinstance(layout, FrameFormat):
            layout, yuv = layout.layout, layout.matrix
        if not isinstance(layout, str) or layout not in self.LAYOUTS:
            raise ValueError(f'layout must be one of {sorted(self.LAYOUTS, key=self.LAYOUTS.get)}, got {layout!r}')
        m = None
        if layout in ('nv12', 'yuyv'):
            if isinstance(yuv, str):
                if FrameFormat._rows is None:
                    FrameFormat._rows = _yuv_rows()
                if (yuv, bool(full_range)) not in FrameFormat._rows:
                    raise ValueError(f"yuv must be 'bt601', 'bt709' or six integers, got {yuv!r}")
                m = FrameFormat._rows[(yuv, bool(full_range))]
            else:
                m = tuple(yuv)
                if len(m) != 6 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in m):
                    raise ValueError(f'a custom yuv matrix is six integers (y_off, cy, cub, cug, cvg, cvr), got {yuv!r}')
                m = tuple(int(v) for v in m)
                if not 0 <= m[0] <= 255:
                    raise ValueError(f'y_off must be in 0 .. 255, got {m[0]}')
                if any(abs(v) > self.COEF_MAX for v in m[1:]):
                    raise ValueError(f'every coefficient magnitude must be <= 3 << 20 = {self.COEF_MAX}, got {m[1:]}')
        self._key = (layout, m)

    layout = property(lambda self: self._key[0])
    matrix = property(lambda self: self._key[1])
    key = property(lambda self: self._key)

    def __eq__(self, other):
        return isinstance(other, FrameFormat) and self._key == other._key

    def __hash__(self):
        return hash(self._key)

    def __repr__(self):
        return f'FrameFormat{self._key!r}'

    def struct(self, plane1_offset=0, plane1_row_bytes=0):
        """The ivx_frame_format of this record (the plane geometry of an NV12 surface is the call's, not the format's)."""
        from ._lib import FrameFormat as CFormat
        return CFormat(self.LAYOUTS[self.layout], int(plane1_row_bytes), int(plane1_offset), *(self.matrix or (0,) * 6))

    def frame_hw(self, shape):
        """(H, W) of the converted BGR frame of a frame array of this layout; TypeError when the shape is not the layout's."""
        shape, lay = tuple(int(v) for v in shape), self.layout
        if lay in ('bgr', 'rgb', 'bgra', 'rgba'):
            ok = len(shape) == 3 and shape[2] == (3 if lay in ('bgr', 'rgb') else 4)
        elif lay == 'gray':
            ok = len(shape) == 2 or (len(shape) == 3 and shape[2] == 1)
        elif lay == 'yuyv':
            ok = len(shape) == 3 and shape[2] == 2 and shape[1] % 2 == 0
        else:
            ok = len(shape) == 2 and shape[1] % 2 == 0 and shape[0] % 3 != 1
        if not ok or min(shape) < 1:
            want = {'bgr': '(H,W,3)', 'rgb': '(H,W,3)', 'bgra': '(H,W,4)', 'rgba': '(H,W,4)', 'gray': '(H,W) or (H,W,1)', 'yuyv': '(H,W,2) with even W',
                    'nv12': '(H + ceil(H/2), W) with even W'}[lay]
            raise TypeError(f'{lay!r} frames must be {want} uint8, got {shape}')
        if lay == 'nv12':
            return ((2 * shape[0]) // 3 if shape[0] % 3 == 0 else (2 * shape[0] - 1) // 3), shape[1]
        return shape[0], shape[1]


def to_bgr_u8(frame, fmt, src_hw=None):
    """The BGR frame that a frame in format `fmt` IS (include/imvoxel.h, the 0.5.3 definition), in numpy on the host: (H,W,3) uint8.  The host
    sibling of the conversion inside ops.image_prep_fmt_u8, as prepare_image is of ops.image_prep_u8.  frame: the layout's array (see
    FrameFormat); src_hw=(H, W) names an odd width, which the arrays of 'nv12' / 'yuyv' (2 * ceil(W/2) samples per row) cannot tell.
    Chroma is the nearest sample (replicated); YUV -> BGR is the header's integer rule, every shift a floor."""
    if not isinstance(fmt, FrameFormat):
        fmt = FrameFormat(fmt)
    a = frame.cpu().numpy() if isinstance(frame, torch.Tensor) else np.asarray(frame)
    if a.dtype != np.uint8:
        raise TypeError(f'frames must be uint8, got {a.dtype}')
    H, W = fmt.frame_hw(a.shape)
    if src_hw is not None:
        h, w = (int(v) for v in src_hw)
        if h != H or ((w + 1) // 2 * 2 != W if fmt.layout in ('nv12', 'yuyv') else w != W):
            raise ValueError(f'src_hw {(h, w)} does not fit a {fmt.layout!r} frame of shape {a.shape}')
        W = w
    lay = fmt.layout
    if lay == 'bgr':
        return a.copy()
    if lay == 'rgb':
        return a[:, :, ::-1].copy()
    if lay == 'bgra':
        return a[:, :, :3].copy()
    if lay == 'rgba':
        return a[:, :, 2::-1].copy()
    if lay == 'gray':
        return np.repeat(a.reshape(H, W, 1), 3, axis=2)
    xs = np.arange(W)
    if lay == 'nv12':
        Y = a[:H, :W].astype(np.int64)
        uv = a[H:].reshape(-1, a.shape[1] // 2, 2).astype(np.int64)[np.arange(H) >> 1][:, xs >> 1]
    else:
        Y = a.reshape(H, -1)[:, 0::2][:, :W].astype(np.int64)
        uv = a.reshape(H, -1, 4)[:, :, 1::2].astype(np.int64)[:, xs >> 1]
    y_off, cy, cub, cug, cvg, cvr = fmt.matrix
    yy = np.maximum(0, Y - y_off) * cy + (1 << 19)
    u, v = uv[..., 0] - 128, uv[..., 1] - 128
    bgr = np.stack([(yy + cub * u) >> 20, (yy + cvg * v + cug * u) >> 20, (yy + cvr * v) >> 20], axis=2)
    return np.clip(bgr, 0, 255).astype(np.uint8)


def _check_formats(format, n):
    """format of prepare_images_device -> None (packed BGR everywhere: the call as it was) or a list of n FrameFormat."""
    if format is None:
        return None
    if isinstance(format, (str, FrameFormat)):
        return [FrameFormat(format)] * n
    format = list(format)
    if len(format) != n:
        raise ValueError(f'{len(format)} formats for {n} frames (one format for all, or one entry per frame)')
    return [FrameFormat(f) for f in format]


def prepare_images_device(frames, img_scale, img_norm_cfg=IMG_NORM_CFG, size_divisor=32, keep_ratio=True, device='cuda', lens=None, format=None):
    """prepare_image for a whole batch on the device (ops.image_prep_u8, csrc/image_prep.hip): the uint8 frames cross to the
    device as they are (a quarter of the bytes of the fp32 tensor) and ONE launch per group of same-sized frames resizes, normalises
    and pads them -- bit-identical to prepare_image per frame.
    frames: a list of (H,W,3) uint8 BGR arrays / tensors; one [N,H,W,3] uint8 array or tensor (host or device); or a list of B
    lists of V frames (multi-view samples).  Frames are grouped by source shape; a group of host frames is stacked and copied in one
    host-to-device copy, device tensors are used where they are.  Every group is written into its slices of one output tensor
    whose plane is the LARGEST pad shape of the batch (zero filled below / right of each image, what mmdet's collate does); a
    group whose frames are not adjacent in the batch takes one launch per run of adjacent frames.
    Returns (img [N,3,Hp,Wp] or [B,V,3,Hp,Wp] fp32 on `device`, list of per-sample dicts img_shape / ori_shape / pad_shape equal to
    prepare_image's; for a multi-view sample the dict of its LAST view, as MultiViewPipeline).
    lens: None (ideal cameras: the call as it was), one Lens for every frame, or a list with one entry per frame in batch order, each a
    Lens or None (a rig).  Frames with a lens go through ops.image_prep_lens_u8 (the lens sampler of csrc/image_prep.hip: undistortion in the same launch, ONE
    bilinear interpolation in fp32 instead of cv2's integer resize, border pixels zero); frames are then grouped by (source shape, lens),
    a run of adjacent frames of one group still taking one launch.  The image shows the lens's new_K scaled by the resize.
    format: None (packed BGR frames: the call as it was), one FrameFormat or layout name for every frame, or one per frame: the frames are
    a decoder's -- 'rgb', 'bgra', 'rgba', 'gray', 'nv12', 'yuyv'; FrameFormat lists the array of each layout -- and are converted inside the
    same launch (ops.image_prep_fmt_u8), the result being the format=None call on to_bgr_u8 of each frame, bit for bit, with or without a
    lens.  Frames are then grouped by (source shape, format, lens), and the returned shapes are those of the converted frame."""
    from . import ops
    device = torch.device(device)
    views = None
    if isinstance(frames, (np.ndarray, torch.Tensor)):
        if frames.ndim != 4 and (format is None or frames.ndim != 3):
            raise TypeError(f'a stacked batch must be [N,H,W,3] uint8, got {tuple(frames.shape)}')
        flat = list(frames)
        stacked = frames
    else:
        frames, stacked = list(frames), None
        if frames and isinstance(frames[0], (list, tuple)):
            views = len(frames[0])
            if any(len(s) != views for s in frames) or views == 0:
                raise ValueError('every multi-view sample must hold the same number of views')
            flat = [f for s in frames for f in s]
        else:
            flat = frames
    if not flat:
        raise ValueError('no frames')
    formats = _check_formats(format, len(flat))
    if formats is not None:
        lenses = _check_lenses(lens, len(flat))
    groups, hws = {}, []                                         # (array shape, format or None, lens or None) -> indices, in batch order
    for i, f in enumerate(flat):
        if formats is None:
            if f.ndim != 3 or f.shape[2] != 3 or f.dtype not in (np.uint8, torch.uint8):
                raise TypeError(f'frames must be (H,W,3) uint8, got {tuple(f.shape)} {f.dtype}')
            hws.append((int(f.shape[0]), int(f.shape[1])))
        else:                                                    # the frame-shape checks are the layout's
            if f.dtype not in (np.uint8, torch.uint8):
                raise TypeError(f'frames must be uint8, got {f.dtype}')
            hws.append(formats[i].frame_hw(f.shape))
    if formats is None:
        lenses = _check_lenses(lens, len(flat))
    for i, f in enumerate(flat):
        key = (tuple(int(v) for v in f.shape), None if formats is None else formats[i], None if lenses is None else lenses[i])
        groups.setdefault(key, []).append(i)
    shapes = {k: _pipeline_shapes(hws[idx[0]], img_scale, size_divisor, keep_ratio) for k, idx in groups.items()}
    Hp, Wp = max(s[1][0] for s in shapes.values()), max(s[1][1] for s in shapes.values())
    out = torch.empty((len(flat), 3, Hp, Wp), device=device, dtype=torch.float32)
    mean, std, to_rgb = img_norm_cfg['mean'], img_norm_cfg['std'], img_norm_cfg.get('to_rgb', True)
    for k, idx in groups.items():
        if stacked is not None and len(groups) == 1:             # one group: the batch as it is
            src = torch.from_numpy(np.ascontiguousarray(stacked)) if isinstance(stacked, np.ndarray) else stacked
        elif all(isinstance(flat[i], np.ndarray) for i in idx):
            src = torch.from_numpy(np.stack([flat[i] for i in idx]))
        else:
            fs = [torch.from_numpy(flat[i]) if isinstance(flat[i], np.ndarray) else flat[i] for i in idx]
            src = torch.stack([f.to(device) for f in fs] if any(f.is_cuda for f in fs) else fs)
        src = src.to(device)                                     # the one host-to-device copy of the group (no-op for device tensors)
        a = 0
        while a < len(idx):                                      # runs of adjacent frames: one launch each (one per group when sorted)
            b = a + 1
            while b < len(idx) and idx[b] == idx[b - 1] + 1:
                b += 1
            o = out[idx[a]:idx[a] + b - a]
            if k[1] is not None:
                ops.image_prep_fmt_u8(src[a:b], k[1], shapes[k][0], (Hp, Wp), mean, std, to_rgb, lens=k[2], out=o)
            elif k[2] is not None:
                ops.image_prep_lens_u8(src[a:b], k[2], shapes[k][0], (Hp, Wp), mean, std, to_rgb, out=o)
            else:
                ops.image_prep_u8(src[a:b], shapes[k][0], (Hp, Wp), mean, std, to_rgb, out=o)
            a = b
    metas = []
    for hw in hws:
        (nh, nw), (ph, pw) = _pipeline_shapes(hw, img_scale, size_divisor, keep_ratio)
        metas.append(dict(img_shape=(nh, nw, 3), ori_shape=(hw[0], hw[1], 3), pad_shape=(ph, pw, 3)))
    if views is not None:
        return out.view(len(flat) // views, views, 3, Hp, Wp), metas[views - 1::views]
    return out, metas


# ------------------------------------------------------------------ multi-view pipeline
class MultiViewPipeline:
    """pipelines/multi_view.py:7-31: draw `n_images` of the scene's views with np.random.choice (with replacement only when
    the scene has fewer views), run the per-view transforms on each drawn view, and re-order the extrinsics to the drawn
    order.  `transforms`: one callable or a list of callables dict -> dict (mmdet's Compose of LoadImageFromFile / Resize /
    Normalize / Pad; view_transform() below is that chain for an in-memory image).  Seed numpy's global generator as
    the reference's training / test scripts do to reproduce a draw."""

    def __init__(self, transforms, n_images):
        self.transforms = list(transforms) if isinstance(transforms, (list, tuple)) else [transforms]
        self.n_images = n_images

    def _apply(self, res):
        for t in self.transforms:
            res = t(res)
        return res

    def __call__(self, results):
        ids = np.arange(len(results['img_info']))
        ids = np.random.choice(ids, self.n_images, replace=self.n_images > len(ids))
        imgs, extrinsics, last = [], [], None
        for i in ids.tolist():
            last = self._apply({key: results[key][i] for key in ('img_prefix', 'img_info')})
            imgs.append(last['img'])
            extrinsics.append(results['lidar2img']['extrinsic'][i])
        for key, val in last.items():          # per-view meta of the LAST drawn view becomes the sample's (img_shape, ...)
            if key not in ('img', 'img_prefix', 'img_info'):
                results[key] = val
        results['img'] = imgs
        results['lidar2img']['extrinsic'] = extrinsics
        return results


def view_transform(img_scale, img_norm_cfg=IMG_NORM_CFG, size_divisor=32, keep_ratio=True, loader=None):
    """The per-view transform chain of the reference test pipelines (imvoxelnet_kitti.py:94-105) for MultiViewPipeline:
    img_info['filename'] is loaded with `loader` (default: img_info['array'], an in-memory BGR uint8 image)."""
    def run(res):
        arr = loader(res['img_info']['filename']) if loader is not None else res['img_info']['array']
        img, meta = prepare_image(arr, img_scale, img_norm_cfg, size_divisor, keep_ratio)
        out = dict(res)
        out.update(meta)
        out['img'] = img
        return out
    return run


class KittiSetOrigin:
    """multi_view.py:45-53 (also the nuScenes configs): origin = centre of point_cloud_range, fp32."""

    def __init__(self, point_cloud_range):
        pcr = np.array(point_cloud_range, dtype=np.float32)
        self.origin = (pcr[:3] + pcr[3:]) / 2.

    def __call__(self, results):
        results['lidar2img']['origin'] = self.origin.copy()
        return results


class SunRgbdSetOrigin:
    """multi_view.py:84-94 (Total3D configs): the point 3 m along the ray through the image centre."""

    def __call__(self, results):
        l2i = results['lidar2img']
        projection = l2i['intrinsic'][:3, :3] @ l2i['extrinsic'][0][:3, :3]
        h, w, _ = results['ori_shape']
        centre = np.array([w / 2, h / 2, 1], dtype=np.float32)
        centre *= 3
        l2i['origin'] = np.linalg.inv(projection) @ centre
        return results


# ------------------------------------------------------------------ calibration -> lidar2img
def kitti_lidar2img(P2, R0_rect, Tr_velo_to_cam, point_cloud_range=(0, -39.68, -3, 69.12, 39.68, 1)):
    """kitti_monocular_dataset.py:16-22 + KittiSetOrigin (multi_view.py:45-53).  4x4 calibration matrices."""
    rect, trv2c, p2 = (np.asarray(m).astype(np.float32) for m in (R0_rect, Tr_velo_to_cam, P2))
    extrinsic = rect @ trv2c
    extrinsic[:3, 3] += np.linalg.inv(p2[:3, :3]) @ p2[:3, 3]
    intrinsic = np.copy(p2)
    intrinsic[:3, 3] = 0
    pcr = np.array(point_cloud_range, dtype=np.float32)
    return dict(extrinsic=[extrinsic], intrinsic=intrinsic, origin=(pcr[:3] + pcr[3:]) / 2.)


def nuscenes_lidar2img(lidar2img_per_camera, point_cloud_range=(-49.92, -49.92, -2.92, 49.92, 49.92, 0.92)):
    """nuscenes_monocular_dataset.py:15-22: K is already folded into every camera's lidar2img, intrinsic = eye(4)."""
    pcr = np.array(point_cloud_range, dtype=np.float32)
    return dict(extrinsic=[np.asarray(x).astype(np.float32) for x in lidar2img_per_camera], intrinsic=np.eye(4, dtype=np.float32),
                origin=(pcr[:3] + pcr[3:]) / 2.)


def scannet_lidar2img(axis_align_matrix, camera_extrinsics, intrinsics):
    """scannet_monocular_dataset.py:19-32: extrinsic_v = inv(axis_align @ cam2world_v), origin (0, 0, .5)."""
    aam = np.asarray(axis_align_matrix).astype(np.float32)
    ext = [np.linalg.inv(aam @ np.asarray(e)).astype(np.float32) for e in camera_extrinsics]
    return dict(extrinsic=ext, intrinsic=np.asarray(intrinsics).astype(np.float32), origin=np.array([.0, .0, .5], np.float32))


def sunrgbd_lidar2img(K, Rt):
    """sunrgbd_monocular_dataset.py:29-73: K stored column-major (reshape(3,3).T), Rt with y/z swapped and y negated,
    extrinsic rotation = Rt^T, origin (0, 3, -1)."""
    intrinsic = np.eye(4)
    intrinsic[:3, :3] = np.asarray(K).copy().reshape(3, 3).T
    rt = np.asarray(Rt).copy()
    rt[:, [1, 2]] = rt[:, [2, 1]]
    rt[:, 1] = -1 * rt[:, 1]
    extrinsic = np.eye(4)
    extrinsic[:3, :3] = rt.T
    return dict(extrinsic=[extrinsic.astype(np.float32)], intrinsic=intrinsic.astype(np.float32), origin=np.array([0, 3, -1], np.float32))
