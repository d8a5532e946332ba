"""The numpy reference of the rigid merge of the scene state (include/imvoxel.h, ivx_volume_merge_fwd), written from the definition, and the error
bound of the fp32 kernel against it.

Steps 1 - 3 (centre from the DESTINATION origin, source point, grid coordinate against the SOURCE origin, floor and fraction) run bit-exactly in
fp32, as in tests/ref_volume_warp.py, so that i0 and f are the device's; the fp32 corner weights decide which corners are read.  The values -- the
sample of step 4 and the add of step 6 -- run in float64 with the exact weights of the same f and the float32 value of alpha.

The bound.  The sample carries the warp's K = 11 roundings per term (tests/ref_volume_warp.py derives it) and is then scaled by alpha; the final
fma(alpha, sample, destination) rounds once:
    |got - exact| <= |alpha| * 11 * 2^-24 * sum_corners |w * S_corner| + 2^-24 * |exact| + 2^-126
and the same for W'.  count is an integer and must be equal.

Decisions must be robust, or fp32 and float64 could disagree on WHICH voxels are written: every positive reference W_s is at least MIN_WS (so that
W_s > 0 is the same statement in both), and the forget decision keeps the warp reference's FORGET_MARGIN."""
import numpy as np

from ref_unproject import fma32, points, U, TINY
from ref_volume_warp import corner_weights, rigid, worst_ratio, K_WARP, FORGET_MARGIN      # noqa: F401  (rigid, worst_ratio: for the tests)

MIN_WS = 1e-6
COUNT_MAX = 2 ** 31 - 1


def grid_coords(dims, voxel_size, origin_dst, origin_src, M):
    """Steps 1 - 3 in fp32 for every destination voxel n = (i*Y + j)*Z + k -> (inside [N] bool, i0 [N,3] int64, f [N,3] float32) in the SOURCE grid;
    i0 and f are 0 where outside."""
    vs, od, os_, M = np.asarray(voxel_size, np.float32), np.asarray(origin_dst, np.float32), np.asarray(origin_src, np.float32), np.asarray(M, np.float32)[:3]
    p = points(dims, vs, od)
    x, y, z = (np.ascontiguousarray(p[:, a]) for a in range(3))
    inside, i0, f = np.ones(len(p), bool), np.zeros((len(p), 3), np.int64), np.zeros((len(p), 3), np.float32)
    for a in range(3):
        full = lambda v: np.full_like(x, v)                                   # noqa: E731
        q = full(M[a, 0]) * x                                                 # one rounded fp32 product
        q = fma32(full(M[a, 1]), y, q)
        q = fma32(full(M[a, 2]), z, q)
        q = fma32(full(M[a, 3]), np.ones_like(x), q)
        with np.errstate(invalid='ignore', over='ignore'):
            g = (q - os_[a]) / vs[a]                                          # a rounded fp32 difference, an IEEE fp32 division
            ok = (g > np.float32(-1)) & (g < np.float32(dims[a]))
        assert g.dtype == np.float32
        fl = np.floor(np.where(ok, g, np.float32(0)))
        inside &= ok
        i0[:, a], f[:, a] = fl.astype(np.int64), np.where(ok, g, np.float32(0)) - fl
    i0[~inside], f[~inside] = 0, 0
    return inside, i0, f


def merge_grid(dst, src, voxel_size, origin_dst, origin_src, M, alpha=1.0, forget_below=0.0):
    """One pair of rows: dst = (S_d [X,Y,Z,C] fp32, W_d [X,Y,Z] fp32, cnt_d [X,Y,Z] int32), src the same for the source row -> dict(S, W: float64, the
    destination after the merge -- the destination's own values where it is not merged; cnt: int32; merged [X,Y,Z] bool; inside [X,Y,Z] bool;
    read [X,Y,Z,8] bool: the corners read; Ws: the float64 sample of the weight sum; bound_S, bound_W: the error bounds on the merged voxels).
    Asserts that the merged and the forget decisions are robust."""
    Sd, Wd, cd = dst
    Ss, Ws, cs = src
    dims = tuple(Sd.shape[:3])
    Cn, N = Sd.shape[3], int(np.prod(dims))
    al = float(np.float32(alpha))
    inside, i0, f = grid_coords(dims, voxel_size, origin_dst, origin_src, M)
    w32, w64 = corner_weights(f)
    Sf, Wf, cf = Ss.reshape(N, Cn), Ws.reshape(N), cs.reshape(N)
    smpS, smpW, smpc = np.zeros((N, Cn)), np.zeros(N), np.zeros(N, np.int64)
    absS, absW, read = np.zeros((N, Cn)), np.zeros(N), np.zeros((N, 8), bool)
    for c in range(8):
        idx = i0 + np.array([c >> 2, (c >> 1) & 1, c & 1])
        rd = inside & (w32[:, c] != 0) & np.all((idx >= 0) & (idx < np.array(dims)), axis=1)
        flat = ((idx[rd, 0] * dims[1]) + idx[rd, 1]) * dims[2] + idx[rd, 2]
        w = w64[rd, c]
        with np.errstate(invalid='ignore', over='ignore'):
            smpS[rd] += w[:, None] * Sf[flat].astype(np.float64)
            smpW[rd] += w * Wf[flat].astype(np.float64)
            absS[rd] += np.abs(w[:, None] * Sf[flat].astype(np.float64))
            absW[rd] += np.abs(w * Wf[flat].astype(np.float64))
        smpc[rd] = np.maximum(smpc[rd], cf[flat])
        read[:, c] = rd
    with np.errstate(invalid='ignore'):
        merged = inside & (smpW > 0)
    assert (smpW[merged] >= MIN_WS).all(), 'the merged decision must be robust: a positive W_s too near 0'
    outS, outW, outc = Sd.reshape(N, Cn).astype(np.float64), Wd.reshape(N).astype(np.float64), cd.reshape(N).astype(np.int64)
    with np.errstate(invalid='ignore', over='ignore'):
        outS[merged] = al * smpS[merged] + outS[merged]
        outW[merged] = al * smpW[merged] + outW[merged]
    outc[merged] = np.minimum(outc[merged] + smpc[merged], COUNT_MAX)
    with np.errstate(invalid='ignore'):
        bound_S, bound_W = abs(al) * K_WARP * U * absS + U * np.abs(outS) + TINY, abs(al) * K_WARP * U * absW + U * np.abs(outW) + TINY
    if forget_below > 0:
        with np.errstate(invalid='ignore'):
            assert np.all(np.abs(outW[merged] - forget_below) >= FORGET_MARGIN * forget_below), 'the forget decision must be robust: a W\' too near forget_below'
            gone = merged & ~(outW >= forget_below)
        outS[gone], outW[gone], outc[gone] = 0, 0, 0
    return dict(S=outS.reshape(dims + (Cn,)), W=outW.reshape(dims), cnt=outc.astype(np.int32).reshape(dims), merged=merged.reshape(dims),
                inside=inside.reshape(dims), read=read.reshape(dims + (8,)), Ws=smpW.reshape(dims),
                bound_S=bound_S.reshape(dims + (Cn,)), bound_W=bound_W.reshape(dims))


def check_row(got, ref, dst, what=''):
    """A destination row after the device's merge, got = (S, W, cnt) host arrays, against the reference `ref` of merge_grid and the row before,
    dst: merged voxels within the bound and counts equal, every other voxel with the bits it had.  -> the worst ratios (sums, weight sum)."""
    m = ref['merged']
    for g, d, name in zip(got, dst, ('sum', 'wsum', 'count')):
        assert np.array_equal(g[~m].view(np.int32), d[~m].view(np.int32)), f'{what}: {name} of an unmerged voxel changed'
    rs, rw = worst_ratio(got[0][m], ref['S'][m], ref['bound_S'][m]), worst_ratio(got[1][m], ref['W'][m], ref['bound_W'][m])
    print(f'{what}: worst |got - ref| / bound  sums {rs:.3f}  weight sum {rw:.3f}; merged {int(m.sum())} of {m.size}')
    assert np.array_equal(got[2][m], ref['cnt'][m]), (what, int((got[2][m] != ref['cnt'][m]).sum()))
    assert rs <= 1 and rw <= 1, (what, rs, rw)
    return rs, rw
