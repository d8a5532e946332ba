"""The numpy reference of the rigid resample of the scene state (include/imvoxel.h, ivx_volume_warp_fwd), written from the definition, and the
error bound of the fp32 kernel against it.

Steps 1 - 3 (centre, source point, grid coordinate, floor and fraction) run bit-exactly in fp32 -- correctly rounded numpy float32 products, sums and
divisions, and fma32 of tests/ref_unproject.py for the fused multiply-adds -- so that i0 and f are the device's: no floor decision can differ.  The
fp32 corner weights are formed the same way, because they decide which corners are READ (a corner of weight exactly 0 is not) and so which counts
enter the maximum.  Steps 4 - 5, the values, run in float64 with the exact weights of the same f.

The bound.  Between the float64 value and the kernel's lie, per term w * S_corner of a sum:
    1 - f           one rounding per axis, and an axis weight enters a corner weight once          1
    (wx * wy) * wz  two rounded products                                                           2
    fma chain       a term passes through at most eight roundings of the running sum               8
so K = 11 and, to first order,  |got - ref| <= K * 2^-24 * sum_corners |w * S_corner| + 2^-126  (the last term: one rounding in the subnormal range).
The same bound holds for W'.  count is an integer and must be equal."""
import numpy as np

from ref_unproject import fma32, points, U, TINY

K_WARP = 1 + 2 + 8
FORGET_MARGIN = 1e-3       # the forget decision is only tested where every W' lies at least this far (relative) from forget_below


def grid_coords(dims, voxel_size, new_origin, M):
    """Steps 1 - 3 in fp32 for every voxel n = (i*Y + j)*Z + k -> (inside [N] bool, i0 [N,3] int64, f [N,3] float32); i0 and f are 0 where outside."""
    vs, o, M = np.asarray(voxel_size, np.float32), np.asarray(new_origin, np.float32), np.asarray(M, np.float32)[:3]
    p = points(dims, vs, o)
    x, y, z = (np.ascontiguousarray(p[:, a]) for a in range(3))
    inside, i0, f = np.ones(len(p), bool), np.zeros((len(p), 3), np.int64), np.zeros((len(p), 3), np.float32)
    for a in range(3):
        full = lambda v: np.full_like(x, v)                                   # noqa: E731
        q = full(M[a, 0]) * x                                                 # one rounded fp32 product
        q = fma32(full(M[a, 1]), y, q)
        q = fma32(full(M[a, 2]), z, q)
        q = fma32(full(M[a, 3]), np.ones_like(x), q)
        with np.errstate(invalid='ignore', over='ignore'):
            g = (q - o[a]) / vs[a]                                            # a rounded fp32 difference, an IEEE fp32 division
            ok = (g > np.float32(-1)) & (g < np.float32(dims[a]))
        assert g.dtype == np.float32
        fl = np.floor(np.where(ok, g, np.float32(0)))
        inside &= ok
        i0[:, a], f[:, a] = fl.astype(np.int64), np.where(ok, g, np.float32(0)) - fl
    i0[~inside], f[~inside] = 0, 0
    return inside, i0, f


def corner_weights(f):
    """f [N,3] float32 -> (w32 [N,8] float32: the device's corner weights, bit for bit; w64 [N,8]: the exact products of the exact axis weights),
    corners in the order dx, dy, dz with dz fastest."""
    one = np.float32(1)
    ax32 = [(one - f[:, a], f[:, a]) for a in range(3)]
    ax64 = [(1.0 - f[:, a].astype(np.float64), f[:, a].astype(np.float64)) for a in range(3)]
    w32, w64 = np.empty((len(f), 8), np.float32), np.empty((len(f), 8))
    for c in range(8):
        dx, dy, dz = c >> 2, (c >> 1) & 1, c & 1
        w32[:, c] = (ax32[0][dx] * ax32[1][dy]) * ax32[2][dz]
        w64[:, c] = (ax64[0][dx] * ax64[1][dy]) * ax64[2][dz]
    return w32, w64


def warp_grid(S, W, cnt, voxel_size, new_origin, M, forget_below=0.0):
    """One row: S [X,Y,Z,C] fp32, W [X,Y,Z] fp32, cnt [X,Y,Z] int32 -> dict(S, W: float64; cnt: int32; bound_S, bound_W: the error bounds; read:
    [X,Y,Z,8] bool, the corners that are read).  Asserts that the forget decision is robust."""
    dims = tuple(S.shape[:3])
    Cn, N = S.shape[3], int(np.prod(dims))
    inside, i0, f = grid_coords(dims, voxel_size, new_origin, M)
    w32, w64 = corner_weights(f)
    Sf, Wf, cf = S.reshape(N, Cn), W.reshape(N), cnt.reshape(N)
    outS, outW, outc = np.zeros((N, Cn)), np.zeros(N), np.zeros(N, np.int32)
    absS, absW, read = np.zeros((N, Cn)), np.zeros(N), np.zeros((N, 8), bool)
    for c in range(8):
        idx = i0 + np.array([c >> 2, (c >> 1) & 1, c & 1])
        rd = inside & (w32[:, c] != 0) & np.all((idx >= 0) & (idx < np.array(dims)), axis=1)
        flat = ((idx[rd, 0] * dims[1]) + idx[rd, 1]) * dims[2] + idx[rd, 2]
        w = w64[rd, c]
        with np.errstate(invalid='ignore', over='ignore'):
            outS[rd] += w[:, None] * Sf[flat].astype(np.float64)
            outW[rd] += w * Wf[flat].astype(np.float64)
            absS[rd] += np.abs(w[:, None] * Sf[flat].astype(np.float64))
            absW[rd] += np.abs(w * Wf[flat].astype(np.float64))
        outc[rd] = np.maximum(outc[rd], cf[flat])
        read[:, c] = rd
    if forget_below > 0:
        with np.errstate(invalid='ignore'):
            assert np.all(np.abs(outW - forget_below) >= FORGET_MARGIN * forget_below), 'the forget decision must be robust: a W\' too near forget_below'
            gone = ~(outW >= forget_below)
        outS[gone], outW[gone], outc[gone] = 0, 0, 0
    return dict(S=outS.reshape(dims + (Cn,)), W=outW.reshape(dims), cnt=outc.reshape(dims), read=read.reshape(dims + (8,)),
                bound_S=(K_WARP * U * absS + TINY).reshape(dims + (Cn,)), bound_W=(K_WARP * U * absW + TINY).reshape(dims))


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the finite entries of the reference; where the reference is not finite `got` must be non-finite in the same way."""
    got, fin = np.asarray(got, np.float64), np.isfinite(ref)
    assert np.array_equal(np.isnan(got[~fin]), np.isnan(ref[~fin])) and np.array_equal(got[~fin][~np.isnan(got[~fin])], ref[~fin][~np.isnan(ref[~fin])])
    return float((np.abs(got[fin] - ref[fin]) / bound[fin]).max()) if fin.any() else 0.0


def rigid(yaw=0.0, pitch=0.0, roll=0.0, t=(0, 0, 0), about=(0, 0, 0)):
    """A float64 4x4 rigid transform: rotation Rz(yaw) Ry(pitch) Rx(roll) about the point `about`, then the translation t."""
    cz, sz, cy, sy, cx, sx = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = np.asarray(about, np.float64) - R @ np.asarray(about, np.float64) + np.asarray(t, np.float64)
    return T


def quarter_yaw(about):
    """The exact quarter turn about the vertical through `about` (entries 0 and +-1, no cos(pi/2) residue)."""
    T = np.eye(4)
    T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    T[:3, 3] = np.asarray(about, np.float64) - T[:3, :3] @ np.asarray(about, np.float64)
    return T
