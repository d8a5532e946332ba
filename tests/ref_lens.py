"""numpy fp64 references of the lens-aware image pipeline (include/imvoxel.h: the map G, ivx_image_prep_lens_u8, ivx_map_prep_lens), the case
list of its tests and the margin checker.  No project kernel is a reference: everything here is numpy on the host.

A lens is a plain dict here (model 'brown' | 'fisheye', fx, fy, cx, cy, coef[5], nfx, nfy, ncx, ncy, r2_max), independent of data.Lens; None
is the ideal camera.  G is written in the header's operation order (numpy rounds every operation on its own, as the kernel built with
-ffp-contract=off does), so device and reference coordinates agree to a few ulp of fp64; the DECISIONS (inside / border, the nearest pixel)
are made robust by `margins`, which counts the pixels of a case that lie near one -- the tests assert that the count is zero for every case.
"""
import numpy as np

INF = float('inf')


def lens(model, fx, fy, cx, cy, coef, new=None, r2_max=INF):
    coef = list(coef) + [0.0] * (5 - len(coef))
    nfx, nfy, ncx, ncy = (fx, fy, cx, cy) if new is None else new
    return dict(model=model, fx=fx, fy=fy, cx=cx, cy=cy, coef=coef, nfx=nfx, nfy=nfy, ncx=ncx, ncy=ncy, r2_max=r2_max)


def G(L, src_hw, dst_hw, x, y):
    """The map G for input pixels (x, y) (integer arrays, broadcast together): (u, v, r2, inside), fp64, the header's order."""
    (sh, sw), (dh, dw) = src_hw, dst_hw
    x, y = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64))
    px = (x + 0.5) * (np.float64(sw) / np.float64(dw)) - 0.5
    py = (y + 0.5) * (np.float64(sh) / np.float64(dh)) - 0.5
    with np.errstate(all='ignore'):
        if L is None:
            u, v, r2 = px, py, np.zeros_like(px)
            r2_max = INF
        else:
            xn = (px - L['ncx']) / L['nfx']
            yn = (py - L['ncy']) / L['nfy']
            r2 = xn * xn + yn * yn
            c = L['coef']
            if L['model'] == 'brown':
                k1, k2, p1, p2, k3 = c
                rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
                xd = (xn * rad + ((2.0 * p1) * xn) * yn) + p2 * (r2 + (2.0 * xn) * xn)
                yd = (yn * rad + p1 * (r2 + (2.0 * yn) * yn)) + ((2.0 * p2) * xn) * yn
            else:
                r = np.sqrt(r2)
                th = np.arctan(r)
                t2 = th * th
                thd = th * (1.0 + t2 * (c[0] + t2 * (c[1] + t2 * (c[2] + t2 * c[3]))))
                s = np.where(r > 0, thd / np.where(r > 0, r, 1.0), 1.0)
                xd, yd = xn * s, yn * s
            u = L['fx'] * xd + L['cx']
            v = L['fy'] * yd + L['cy']
            r2_max = L['r2_max']
        inside = (r2 <= r2_max) & (u >= -0.5) & (u <= sw - 0.5) & (v >= -0.5) & (v <= sh - 0.5)
    return u, v, r2, inside


def grid(dst_hw, stride=1, pad_hw=None):
    """Input pixel coordinates (x [1,w], y [h,1]) of the dst region, or of the strided feature pixels of the pad plane."""
    h, w = dst_hw if pad_hw is None else pad_hw
    return np.arange(0, w, stride)[None, :], np.arange(0, h, stride)[:, None]


def image(src, L, dst_hw, pad_hw, mean, std, to_rgb=True):
    """ivx_image_prep_lens_u8 for one frame src [H,W,3] uint8 in fp64: the EXACT bilinear blend at the fp64 (u, v), normalised with the fp32 mean / std
    taken as exact numbers -> (out [3,ph,pw] float64 with border and pad 0, mask [ph,pw] bool of the inside pixels)."""
    sh, sw = src.shape[:2]
    (dh, dw), (ph, pw) = dst_hw, pad_hw
    x, y = grid(dst_hw)
    u, v, _, inside = G(L, (sh, sw), dst_hw, x, y)
    u, v = np.where(inside, u, 0.0), np.where(inside, v, 0.0)
    iu, iv = np.floor(u), np.floor(v)
    fu, fv = (u - iu)[..., None], (v - iv)[..., None]
    x0, x1 = np.maximum(iu, 0).astype(np.int64), np.minimum(iu + 1, sw - 1).astype(np.int64)
    y0, y1 = np.maximum(iv, 0).astype(np.int64), np.minimum(iv + 1, sh - 1).astype(np.int64)
    S = src.astype(np.float64)
    if to_rgb:
        S = S[..., ::-1]
    top = S[y0, x0] + fu * (S[y0, x1] - S[y0, x0])
    bot = S[y1, x0] + fu * (S[y1, x1] - S[y1, x0])
    val = top + fv * (bot - top)                                   # [dh,dw,3]
    m, sd = np.asarray(mean, np.float32).astype(np.float64), np.asarray(std, np.float32).astype(np.float64)
    out = np.zeros((3, ph, pw), np.float64)
    out[:, :dh, :dw] = np.where(inside[None], ((val - m) / sd).transpose(2, 0, 1), 0.0)
    mask = np.zeros((ph, pw), bool)
    mask[:dh, :dw] = inside
    return out, mask


def feature_inside(L, src_hw, dst_hw, pad_hw, stride):
    """(u, v, inside) at the feature pixels (i, j) = input pixels (stride * i, stride * j) of the pad plane; pad pixels are not inside."""
    x, y = grid(dst_hw, stride, pad_hw)
    u, v, _, inside = G(L, src_hw, dst_hw, x, y)
    inside = inside & (x < dst_hw[1]) & (y < dst_hw[0])
    return u, v, inside


def cover(L, src_hw, dst_hw, pad_hw, stride):
    """ivx_map_prep_lens with src == NULL: float32 [ceil(ph / stride), ceil(pw / stride)]."""
    return feature_inside(L, src_hw, dst_hw, pad_hw, stride)[2].astype(np.float32)


def picked(src_map, L, dst_hw, pad_hw, scale, stride):
    """ivx_map_prep_lens with a source map [H,W] (float32 or uint16): float32(scale) * float32(nearest source value), 0 at border pixels."""
    sh, sw = src_map.shape
    u, v, inside = feature_inside(L, (sh, sw), dst_hw, pad_hw, stride)
    u, v = np.where(inside, u, 0.0), np.where(inside, v, 0.0)
    sx = np.clip(np.floor(u + 0.5), 0, sw - 1).astype(np.int64)
    sy = np.clip(np.floor(v + 0.5), 0, sh - 1).astype(np.int64)
    val = np.float32(scale) * src_map[sy, sx].astype(np.float32)
    return np.where(inside, val, np.float32(0.0)).astype(np.float32)


def margins(L, src_hw, dst_hw, pick=False, stride=1, pad_hw=None):
    """How many pixels of a case lie near a decision: u or v within 1e-6 px of an inside boundary (-0.5, src - 0.5), r2 within 1e-9 relative of
    r2_max, and -- pick=True, among the inside pixels -- u or v within 1e-6 of a half (the nearest pick's tie).  NaN coordinates count as near.
    -> dict of counts; the tests need every one to be zero."""
    sh, sw = src_hw
    x, y = grid(dst_hw, stride, pad_hw if stride > 1 else None)
    if stride > 1:
        keep_x, keep_y = x[x < dst_hw[1]][None, :], y[y < dst_hw[0]][:, None]
        x, y = keep_x, keep_y
    u, v, r2, inside = G(L, src_hw, dst_hw, x, y)
    eps = 1e-6
    near = lambda a, b: ~(np.abs(a - b) > eps)                       # noqa: E731   (NaN: near)
    edge = near(u, -0.5) | near(u, sw - 0.5) | near(v, -0.5) | near(v, sh - 0.5)
    ring = np.zeros_like(edge)
    if L is not None and np.isfinite(L['r2_max']):
        ring = ~(np.abs(r2 - L['r2_max']) > 1e-9 * L['r2_max'])
    out = dict(edge=int(edge.sum()), ring=int(ring.sum()), half=0)
    if pick:
        fu, fv = u - np.floor(u), v - np.floor(v)
        out['half'] = int((inside & (near(fu, 0.5) | near(fv, 0.5))).sum())
    return out


# ------------------------------------------------------------------ the cases
def case_lens(name, src_hw):
    """The lenses of the tests, scaled to a source frame of src_hw = (h, w).  Parameters are deliberately not round numbers: no pixel of any case
    lies near a decision (margins, asserted by the tests)."""
    h, w = src_hw
    fx, fy, cx, cy = 0.77 * w + 0.113, 0.79 * w + 0.071, 0.49 * w + 0.137, 0.51 * h - 0.093
    if name == 'zero':                    # the ideal camera written as a lens: G is the resize's own rule
        return lens('brown', fx, fy, cx, cy, [0, 0, 0, 0, 0])
    if name == 'barrel':                  # strong barrel seen through a wider ideal camera; the polynomial is trusted up to its fold: corners are border
        return lens('brown', fx, fy, cx, cy, [-0.3, 0.04137, 0, 0, 0], new=(0.55 * fx, 0.55 * fy, cx, cy), r2_max=0.9731)
    if name == 'pincushion':              # corners map outside the frame
        return lens('brown', fx, fy, cx, cy, [0.21, 0.033, 0, 0, 0])
    if name == 'tangential':
        return lens('brown', fx, fy, cx, cy, [-0.11, 0.0171, 0.013, -0.009, 0.002])
    if name == 'new_k':                   # another ideal camera: zoomed out and shifted
        return lens('brown', fx, fy, cx, cy, [-0.17, 0.023, 0.0007, -0.0004, 0], new=(0.83 * fx, 0.81 * fy, cx + 1.37, cy - 0.71))
    if name == 'ring':                    # a finite r2_max inside the frame cuts a disc out of it
        return lens('brown', fx, fy, cx, cy, [-0.05, 0.003, 0, 0, 0], r2_max=0.2317)
    if name == 'fisheye':
        return lens('fisheye', fx, fy, cx, cy, [-0.031, 0.0127, -0.0043, 0.0011], new=(0.7 * fx, 0.7 * fy, cx - 0.41, cy + 0.29))
    raise KeyError(name)


LENSES = ('barrel', 'pincushion', 'tangential', 'new_k', 'ring', 'fisheye')
# (source hw, dst hw, pad hw, unaligned out): the vector path; an unaligned `out` pointer and pad_w % 4 != 0 (scalar path); an up-scale (the -0.5 edge
# band and replicated taps).  The scalar case pads to 24 x 34: a pad of 24 x 30 cannot hold a 23 x 31 image; 34 keeps pad_w % 4 == 2.
SHAPES = {'vector': ((37, 53), (23, 31), (32, 32), False), 'scalar': ((37, 53), (23, 31), (24, 34), True), 'upscale': ((9, 11), (20, 24), (20, 24), False)}
EQUAL = ((21, 28), (21, 28), (32, 32))                              # equal size with the zero lens
BIG = ((480, 1600), (384, 1280), (384, 1280), 6)                    # more than 2048 x 256 work items: 6 * 384 * 320
BIG_LENS = 'tangential'
# the map entry: (source hw, dst hw, pad hw) with pad sizes that are and are not multiples of the strides 4 and 1
MAP_SHAPES = {'multiple': ((37, 53), (23, 31), (32, 32)), 'ragged': ((37, 53), (23, 31), (27, 34)), 'upscale': ((9, 11), (20, 24), (22, 25))}
MAP_LENSES = (None, 'barrel', 'pincushion', 'ring', 'fisheye')
STRIDES = (4, 1)

# the image bound (tests/test_gpu_lens_prep.py derives it): K fp32 roundings of quantities of at most 255 grey levels, the coordinates' fp64 noise
K_IMAGE = 8
COORD_EPS = 1e-9                                                    # px: fp64 disagreement of the coordinates (about 50 roundings at 1.1e-16 of <= 4e4 px)


def image_tolerance(ref, std):
    """|out - ref| <= (K * 2^-24 * 255 + 2 * 255 * COORD_EPS) / |std[c]| + 2^-24 * |ref|   per element of ref [3,h,w] (the last term: the divide)."""
    sd = np.abs(np.asarray(std, np.float32).astype(np.float64))[:, None, None]
    return (K_IMAGE * 2.0 ** -24 * 255.0 + 2 * 255.0 * COORD_EPS) / sd + 2.0 ** -24 * np.abs(ref)


def frames(seed, n, hw):
    return np.random.default_rng(seed).integers(0, 256, (n,) + tuple(hw) + (3,), dtype=np.uint8)
