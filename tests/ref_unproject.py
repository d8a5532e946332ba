"""fp64 reference of the image-to-voxel unprojection with the BILINEAR sampling rule, written from its definition in include/imvoxel.h
(ivx_backproject_fwd_ex), and the error bound of the fp32 kernel against it.  Plain numpy; there is deliberately no other restatement of this mode.

The reference takes the fp32 quotients xf = u / d, yf = v / d and the depth d as INPUTS, so that no floor / rint decision can differ between it
and the kernel.  `project` computes them with the kernel's own fp32 operation chain (correctly rounded products, fused multiply-adds and
divisions, emulated exactly in fp64); on the dyadic scene below every one of those operations is exact, which `dyadic_scene` asserts.
"""
import numpy as np

U = 2.0 ** -24            # unit roundoff of fp32
TINY = 2.0 ** -126        # absolute slack: one subnormal-range rounding
U_BF16 = 2.0 ** -8        # unit roundoff of bf16 (one rounding at the store)
TINY_BF16 = 2.0 ** -133


def k_bilinear(V):
    """Roundings between the fp64 value and the fp32 kernel, counted from the fixed order of include/imvoxel.h:
      weights   bx = 1 - ax (1), the product bx * by etc. (1)   (ax, ay themselves are the reference's inputs)          2
      blend     w00 * f00 (1), three fused multiply-adds (3): a term passes through at most these four                  4
      view sum  V - 1 additions (the first one adds to 0 and is exact)                                                  V - 1
      mean      one division by the count (the count is exact)                                                          1
    Every term is bounded by its share of A = mean over the valid views of sum_i w_i |f_i|, so |got - ref| <= K * 2^-24 * A to first order."""
    return 2 + 4 + (V - 1) + 1


def _round_sum_f32(p, c):
    """float32(p + c) with ONE rounding, for fp64 arrays p (an exact product of two fp32 numbers) and c (an fp32 number): the fp64 sum s may be
    inexact; where s sits exactly half-way between two fp32 numbers the sign of the fp64 rounding error decides (TwoSum), as the fused
    multiply-add decides on the exact value."""
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                 # exact: p + c = s + e
    r = s.astype(np.float32)
    d = s - r.astype(np.float64)
    away = np.nextafter(r, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    tie = (d != 0) & ((r.astype(np.float64) + away.astype(np.float64)) / 2 == s)
    return np.where(tie & (e != 0) & (np.sign(e) == np.sign(d)), away, r).astype(np.float32)


def fma32(a, b, c):
    """fmaf(a, b, c) for fp32 arrays (the product of two fp32 numbers is exact in fp64)."""
    return _round_sum_f32(a.astype(np.float64) * b.astype(np.float64), np.asarray(c, np.float32).astype(np.float64))


def points(n_voxels, voxel_size, new_origin):
    """[N, 3] fp32 voxel centres, n = (i*Y + j)*Z + k: float(idx) * voxel_size + new_origin, an fp32 product and an fp32 sum."""
    X, Y, Z = n_voxels
    idx = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing='ij'), -1).reshape(-1, 3).astype(np.float32)
    return (idx * np.asarray(voxel_size, np.float32)[None]) + np.asarray(new_origin, np.float32)[None]


def project(proj, pts):
    """proj [V, 3, 4] fp32, pts [N, 3] fp32 -> (xf, yf, d) [V, N] fp32 by the kernel's chain: row . (x, y, z, 1) as P0 * x, then
    fma(P1, y, .), fma(P2, z, .), fma(P3, 1, .); xf = u / d, yf = v / d (IEEE division: fp64 quotient of fp32 numbers rounds once)."""
    proj, pts = np.asarray(proj, np.float32), np.asarray(pts, np.float32)
    x, y, z = (pts[None, :, a] for a in range(3))
    rows = []
    for r in range(3):
        P = [proj[:, r, c][:, None] for c in range(4)]
        acc = (P[0].astype(np.float64) * x.astype(np.float64)).astype(np.float32)
        acc = fma32(P[1], y, acc)
        acc = fma32(P[2], z, acc)
        acc = fma32(P[3], np.ones_like(z), acc)
        rows.append(acc)
    u, v, d = rows
    with np.errstate(divide='ignore', invalid='ignore'):
        xf = (u.astype(np.float64) / d.astype(np.float64)).astype(np.float32)
        yf = (v.astype(np.float64) / d.astype(np.float64)).astype(np.float32)
    return xf, yf, d


def valid_views(xf, yf, d, hc, wc):
    """The validity rule, shared by both sampling rules: rint(xf), rint(yf) inside the crop and d > 0 (NaN / inf fail)."""
    with np.errstate(invalid='ignore'):
        xr, yr = np.rint(xf), np.rint(yf)
        return (xr >= 0) & (yr >= 0) & (xr < wc) & (yr < hc) & (d > 0)


def nearest_reference(feat, xf, yf, d, hc, wc):
    """feat [V, FH, FW, C]; xf, yf, d [V, N] fp32 -> (fp64 mean [N, C], valid [N] bool, count [N]) by the reference's nearest rule."""
    feat = np.asarray(feat, np.float64)
    V, N = xf.shape
    ok = valid_views(xf, yf, d, hc, wc)
    tot = np.zeros((N, feat.shape[-1]))
    for v in range(V):
        n = np.nonzero(ok[v])[0]
        tot[n] += feat[v, np.rint(yf[v, n]).astype(np.int64), np.rint(xf[v, n]).astype(np.int64)]
    cnt = ok.sum(0)
    return np.where(cnt[:, None] > 0, tot / np.maximum(cnt, 1)[:, None], 0.0), cnt > 0, cnt


def corners(xf, yf, hc, wc):
    """(x0, x1, y0, y1 clamped ints, ax, ay fp32) of VALID samples: floor, + 1, border clamp; the fractions by one fp32 subtraction."""
    fx, fy = np.floor(xf), np.floor(yf)
    ax, ay = (xf - fx).astype(np.float32), (yf - fy).astype(np.float32)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    cl = lambda a, n: np.clip(a, 0, n - 1)         # noqa: E731
    return cl(x0, wc), cl(x0 + 1, wc), cl(y0, hc), cl(y0 + 1, hc), ax, ay


def bilinear_reference(feat, xf, yf, d, hc, wc):
    """feat [V, FH, FW, C]; xf, yf, d [V, N] fp32; hc, wc: the crop clamped to the map.
    -> (fp64 mean [N, C], valid [N] bool, count [N], A [N, C]): the mean over the valid views of the four-corner blend with weights
    (1-ax)(1-ay), ax(1-ay), (1-ax)ay, ax*ay in fp64 (ax, ay the fp32 fractions), 0 where no view is valid; A = the same mean of sum_i w_i |f_i|."""
    feat = np.asarray(feat, np.float64)
    V, N = xf.shape
    ok = valid_views(xf, yf, d, hc, wc)
    tot, mag = np.zeros((N, feat.shape[-1])), np.zeros((N, feat.shape[-1]))
    for v in range(V):
        n = np.nonzero(ok[v])[0]
        x0, x1, y0, y1, ax, ay = corners(xf[v, n], yf[v, n], hc, wc)
        ax, ay = ax.astype(np.float64)[:, None], ay.astype(np.float64)[:, None]
        for w, yy, xx in (((1 - ax) * (1 - ay), y0, x0), (ax * (1 - ay), y0, x1), ((1 - ax) * ay, y1, x0), (ax * ay, y1, x1)):
            f = feat[v, yy, xx]
            tot[n] += w * f
            mag[n] += w * np.abs(f)
    cnt = ok.sum(0)
    den = np.maximum(cnt, 1)[:, None]
    return np.where(cnt[:, None] > 0, tot / den, 0.0), cnt > 0, cnt, np.where(cnt[:, None] > 0, mag / den, 0.0)


def bound(A, V, ref=None, bf16=False):
    """|got - ref| <= K * 2^-24 * A + 2^-126; bf16 storage: one more rounding of the result (relative 2^-8 of what is rounded)."""
    b = k_bilinear(V) * U * A + TINY
    if bf16:
        b = b + U_BF16 * (np.abs(ref) + b) + TINY_BF16
    return b


# ------------------------------------------------------------------ the dyadic scene
N_VOXELS = (7, 6, 5)
VOXEL_SIZE = (0.25, 0.25, 0.25)
ORIGIN, ORIGIN_2 = (1.5, 0.0, 0.25), (1.25, 0.25, 0.5)       # the second sample of the batch: another origin, the whole map as crop


def new_origin_of(origin):
    """origin - n_voxels / 2 * voxel_size (detectors/imvoxelnet.py:139); exact here."""
    return tuple(float(o) - n / 2.0 * v for o, n, v in zip(origin, N_VOXELS, VOXEL_SIZE))


NEW_ORIGIN, NEW_ORIGIN_2 = new_origin_of(ORIGIN), new_origin_of(ORIGIN_2)
FH, FW = 6, 9
CROP, CROP_2 = (5, 8), (6, 9)
K = np.array([[4, 0, 3.5], [0, 4, 2.5], [0, 0, 1]], np.float64)
_R0 = np.array([[0, -1, 0], [0, 0, -1], [1, 0, 0]], np.float64)
_R1 = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], np.float64)
EXTRINSICS = ((_R0, (0.125, 0.25, 0.5)), (_R1, (-1.0, 0.5, 0.75)), (_R0, (0.5, 0.0, -1.25)))


def dyadic_proj():
    """[3, 3, 4] fp32: K @ [R | t] of the three views (exact: small dyadic numbers)."""
    P = np.stack([K @ np.concatenate([R, np.asarray(t, np.float64)[:, None]], 1) for R, t in EXTRINSICS])
    assert np.array_equal(P.astype(np.float32).astype(np.float64), P)
    return P.astype(np.float32)


def dyadic_scene(new_origin=NEW_ORIGIN, crop=CROP):
    """dict(proj [3,3,4], pts [N,3], xf, yf, d [3,N], hc, wc) of the scene of the bilinear tests: grid 7x6x5, voxel size 0.25, a 6x9 map.
    Every number is dyadic, so points, u, v and d are exact in fp32 (asserted against fp64) and xf, yf are the correctly rounded quotients."""
    proj, pts = dyadic_proj(), points(N_VOXELS, VOXEL_SIZE, new_origin)
    xf, yf, d = project(proj, pts)
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in N_VOXELS], indexing='ij'), -1).reshape(-1, 3).astype(np.float64)
    p64 = idx * np.asarray(VOXEL_SIZE, np.float64) + np.asarray(new_origin, np.float64)
    assert np.array_equal(pts.astype(np.float64), p64), 'the points are not exact in fp32'
    h = np.concatenate([p64, np.ones((len(p64), 1))], 1)
    uvd = np.einsum('vrc,nc->vrn', proj.astype(np.float64), h)
    assert np.array_equal(uvd.astype(np.float32).astype(np.float64), uvd), 'u, v, d are not exact in fp32'
    with np.errstate(divide='ignore', invalid='ignore'):
        assert np.array_equal(d.astype(np.float64), uvd[:, 2]) and np.array_equal(xf, (uvd[:, 0] / uvd[:, 2]).astype(np.float32), equal_nan=True)
        assert np.array_equal(yf, (uvd[:, 1] / uvd[:, 2]).astype(np.float32), equal_nan=True)
    hc, wc = min(crop[0], FH), min(crop[1], FW)
    return dict(proj=proj, pts=pts, xf=xf, yf=yf, d=d, hc=hc, wc=wc, new_origin=np.asarray(new_origin, np.float32), crop=np.asarray(crop, np.int32))


def scene_classes(sc):
    """Per view: the counts of the classes the tests must cover (valid, behind the camera, valid in the clamped border band, exact-integer hits,
    exact half-pixel ties), and the histogram of per-voxel view counts."""
    xf, yf, d, hc, wc = sc['xf'], sc['yf'], sc['d'], sc['hc'], sc['wc']
    ok = valid_views(xf, yf, d, hc, wc)
    with np.errstate(invalid='ignore'):
        band = ok & ((xf < 0) | (xf > wc - 1) | (yf < 0) | (yf > hc - 1))
        integer = ok & (xf == np.floor(xf)) & (yf == np.floor(yf))
        tie = ok & ((np.abs(xf - np.floor(xf)) == 0.5) | (np.abs(yf - np.floor(yf)) == 0.5))
    cnt = ok.sum(0)
    return dict(valid=ok.sum(1).tolist(), behind=(d <= 0).sum(1).tolist(), band=band.sum(1).tolist(), integer=integer.sum(1).tolist(),
                tie=tie.sum(1).tolist(), counts=[int((cnt == c).sum()) for c in range(xf.shape[0] + 1)])
