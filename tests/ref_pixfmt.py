"""An independent numpy / int64 restatement of the decoder pixel formats of include/imvoxel.h (0.5.3, ivx_frame_format): a frame in any layout
IS a BGR uint8 frame through the header's integer rule.  It calls neither data.to_bgr_u8 nor any kernel; the tests of the host sibling and of
the device path are both held to it.  Frames are raw surfaces here -- a flat uint8 buffer plus the geometry a decoder would hand over (pitch
of plane 0, offset and pitch of the NV12 UV plane) -- because that is the most general thing the entry accepts; tight() gives the usual arrays."""
from fractions import Fraction

import numpy as np

LAYOUTS = ('bgr', 'rgb', 'bgra', 'rgba', 'gray', 'nv12', 'yuyv')          # IVX_PIX_* by value
YUV = ('nv12', 'yuyv')
COEF_MAX = 3 << 20
BT601_LIMITED = (16, 1220542, 2116026, -409993, -852492, 1673527)       # (y_off, cy, cub, cug, cvg, cvr): OpenCV's table, listed by value


def round_half_even(q):
    """A Fraction to the nearest integer, ties to even, in integers."""
    fl = q.numerator // q.denominator
    r = q - fl
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and fl % 2):
        fl += 1
    return fl


def matrix(standard, full_range):
    """The named rows of ivx_yuv_matrix from the header's text: the exact real matrix times 2^20 rounded half to even, except BT.601 limited."""
    if standard == 'bt601' and not full_range:
        return BT601_LIMITED
    kr, kb = {'bt601': (Fraction(299, 1000), Fraction(114, 1000)), 'bt709': (Fraction(2126, 10000), Fraction(722, 10000))}[standard]
    kg = 1 - kr - kb
    cy, s, y_off = (Fraction(1), Fraction(1), 0) if full_range else (Fraction(255, 219), Fraction(255, 224), 16)
    cvr, cub = 2 * s * (1 - kr), 2 * s * (1 - kb)
    cug, cvg = -2 * s * kb * (1 - kb) / kg, -2 * s * kr * (1 - kr) / kg
    return (y_off,) + tuple(round_half_even(v * 2 ** 20) for v in (cy, cub, cug, cvg, cvr))


def min_row_bytes(layout, w):
    return {'bgr': 3 * w, 'rgb': 3 * w, 'bgra': 4 * w, 'rgba': 4 * w, 'gray': w, 'nv12': w, 'yuyv': 4 * ((w + 1) // 2)}[layout]


def assert_in_int32(m):
    """In Python ints: with matrix m no intermediate of the rule reaches 2^31 for any bytes (the extremes of every term are at the ends of
    the byte range, the terms are linear in each byte)."""
    y_off, cy, cub, cug, cvg, cvr = (int(v) for v in m)
    worst = 0
    for Y in (0, 255):
        yy = max(0, Y - y_off) * cy
        for u in (-128, 127):
            for v in (-128, 127):
                for t in (yy, yy + (1 << 19), cvr * v, cvg * v, cug * u, cub * u, yy + (1 << 19) + cvr * v, yy + (1 << 19) + cvg * v,
                          yy + (1 << 19) + cvg * v + cug * u, cvg * v + cug * u, yy + (1 << 19) + cub * u):
                    worst = max(worst, abs(t))
    assert worst < 2 ** 31, (m, worst)
    return worst


def yuv_pre(Y, U, V, m):
    """The three values of the rule BEFORE the clamp, (B, G, R) int64 arrays, and Y - y_off."""
    y_off, cy, cub, cug, cvg, cvr = (int(v) for v in m)
    Y, U, V = Y.astype(np.int64), U.astype(np.int64), V.astype(np.int64)
    yy = np.maximum(0, Y - y_off) * cy
    u, v = U - 128, V - 128
    R = (yy + (1 << 19) + cvr * v) >> 20
    G = (yy + (1 << 19) + cvg * v + cug * u) >> 20
    B = (yy + (1 << 19) + cub * u) >> 20
    return np.stack([B, G, R], axis=-1), Y - y_off


def samples(buf, layout, h, w, row_bytes, plane1_offset=0, plane1_row_bytes=0):
    """(Y, U, V) [h, w] of a YUV surface: chroma at the nearest sample, replicated."""
    buf = np.asarray(buf, np.uint8).reshape(-1)
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    if layout == 'nv12':
        Y = buf[ys * row_bytes + xs]
        c = plane1_offset + (ys >> 1) * plane1_row_bytes + 2 * (xs >> 1)
        return Y, buf[c], buf[c + 1]
    assert layout == 'yuyv'
    mp = ys * row_bytes + 4 * (xs >> 1)
    return buf[mp + 2 * (xs & 1)], buf[mp + 1], buf[mp + 3]


def to_bgr(buf, layout, h, w, row_bytes, plane1_offset=0, plane1_row_bytes=0, m=None, info=None):
    """The BGR frame [h, w, 3] uint8 that the surface IS.  info: a dict that receives, for a YUV layout, the counts the tests assert on."""
    buf = np.asarray(buf, np.uint8).reshape(-1)
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    if layout in ('bgr', 'rgb', 'bgra', 'rgba'):
        bpp = 3 if layout in ('bgr', 'rgb') else 4
        base = ys * row_bytes + bpp * xs
        order = (0, 1, 2) if layout in ('bgr', 'bgra') else (2, 1, 0)
        return np.stack([buf[base + k] for k in order], axis=-1)
    if layout == 'gray':
        g = buf[ys * row_bytes + xs]
        return np.stack([g, g, g], axis=-1)
    Y, U, V = samples(buf, layout, h, w, row_bytes, plane1_offset, plane1_row_bytes)
    assert_in_int32(m)
    pre, yd = yuv_pre(Y, U, V, m)
    if info is not None:
        lo, hi = pre < 0, pre > 255
        info.update(clamped_0=int(lo.sum()), clamped_255=int(hi.sum()), y_below=int((yd < 0).sum()),
                    one_saturates=int(((lo | hi).sum(axis=-1) == 1).sum()))
    return np.clip(pre, 0, 255).astype(np.uint8)


def surface(rng, layout, h, w, row_bytes=None, plane1_row_bytes=None, gap_rows=0, lead=0, fill=0xFF):
    """A random surface of the layout: -> (flat uint8 buffer, geometry dict for to_bgr / the op).  Payload bytes are uniform random, every
    other byte (pitch gaps, the rows between the planes, `lead` bytes in front -- the frame starts at buf[lead]) is `fill`, so a wrong
    address shows.  The buffer ends with the last payload byte."""
    tight = min_row_bytes(layout, w)
    rb = tight if row_bytes is None else row_bytes
    assert rb >= tight
    cw, ch = (w + 1) // 2, (h + 1) // 2
    geom = dict(row_bytes=rb)
    if layout == 'nv12':
        p1 = 2 * cw if plane1_row_bytes is None else plane1_row_bytes
        off = (h + gap_rows) * rb
        size = off + (ch - 1) * p1 + 2 * cw
        geom.update(plane1_offset=off, plane1_row_bytes=p1)
    else:
        size = (h - 1) * rb + tight
    buf = np.full(lead + size, fill, np.uint8)
    f = buf[lead:]
    for y in range(h):
        f[y * rb:y * rb + tight] = rng.integers(0, 256, tight, dtype=np.uint8)
    if layout == 'nv12':
        for y in range(ch):
            f[off + y * p1:off + y * p1 + 2 * cw] = rng.integers(0, 256, 2 * cw, dtype=np.uint8)
    return buf, geom


def tight(buf, layout, h, w, geom):
    """The usual array of a surface made with the default pitches: (H,W,3) / (H,W,4) / (H,W) / (H + ceil(H/2), 2*ceil(W/2)) / (H, 2*ceil(W/2), 2).
    A stacked NV12 array needs an even w (its Y rows and UV rows share one pitch)."""
    buf = np.asarray(buf, np.uint8).reshape(-1)
    assert geom['row_bytes'] == min_row_bytes(layout, w)
    if layout in ('bgr', 'rgb'):
        return buf.reshape(h, w, 3)
    if layout in ('bgra', 'rgba'):
        return buf.reshape(h, w, 4)
    if layout == 'gray':
        return buf.reshape(h, w)
    if layout == 'yuyv':
        return buf.reshape(h, 2 * ((w + 1) // 2), 2)
    assert w % 2 == 0 and geom['plane1_offset'] == h * w and geom['plane1_row_bytes'] == w
    return buf.reshape(h + (h + 1) // 2, w)
