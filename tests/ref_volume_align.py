"""The numpy reference of the Gauss-Newton normal equations of a pose between two rows of the scene state (include/imvoxel.h, ivx_volume_align_fwd),
written from the definition, and the error bound of the fp32 kernel against it.

Steps 1 - 3 of the sample run bit-exactly in fp32 (tests/ref_volume_merge.grid_coords, tests/ref_unproject.points), so i0, f, the voxel centre p
and d = p - about (one rounded fp32 difference) are the device's; the fp32 corner weights decide which corners the sample reads.  Values run in
float64 with the exact weights of the same f.  geometry='float64' runs the geometry in float64 too: the cost is then a smooth function of the
pose (between cell changes) and its gradient can be checked against finite differences -- that switch serves the finite-difference test alone.

    a_c = S_d[c] / W_d,  b_c = S_s[c] / W_s,  r_c = b_c - a_c
    grad_c[A] = (D_A S_s[c] - b_c D_A W_s) / (W_s voxel_size[A]),  D_A V = sum over the four corner pairs of axis A of (w_p w_q) (V[+1] - V[0])
    u_c = R^T grad_c,  d = p - about,  J_c = (u_c, d x u_c)
    e = sum r_c^2,  g = sum J_c r_c,  H = sum J_c J_c^T        over the USED voxels and all channels
    dot, na, nb, pairs, own: ref_volume_match's, over the paired voxels.

Counts are integers and must be EQUAL, so every decision must be robust, or the reference refuses the input: wherever a corner's weight sum or a
sampled W_s is positive it is at least MIN_WS, and no visited own point lies so close to a cell face that the fp32 chain and the exact chain on
the same inputs pick different cells (or differ on inside).

The bound, from the operation order the header fixes (u = 2^-24, first order).  Every difference adds the magnitudes of both terms.
    b_c   24 u B_c,  a_c   2 u A_c         (ref_volume_match: B_c = sum_corners |w S_corner| / W_s, A_c = |a_c|);  r_s = 1 / W_s   12 u
    r_c   one rounded difference: 24 B + 2 A + (A + B) <= 25 u Rm_c,  Rm_c = A_c + B_c
    D_A V two axis weights (1 - f: 1 each), their product (1), the corner difference (1, on |V[+1]| + |V[0]|), a chain of four fma (4):
          8 u MV,  MV = sum_pairs w_p w_q (|V[+1]| + |V[0]|);  MN over the sums, MD over the weight sums
    b dD  24 + 8 + 1 = 33 u B MD;   dN - b dD   8 MN + 33 B MD + 1 (MN + B MD) <= 34 u Ms,  Ms = MN + B MD
    grad  * r_s: 34 + 12 + 1 = 47;  / voxel_size: + 1 = 48 u Gm,  Gm[A] = Ms / (W_s voxel_size[A])
    u     a product and two fma, a term passes through at most three roundings: 48 + 3 = 51 u Um,  Um[j] = sum_i |R[i][j]| Gm[i]
    d x u a product (1) and the difference (1): 53 u Cm,  Cm[0] = |d_1| Um[2] + |d_2| Um[1], ..    (d itself is the device's, bit for bit)
    per sum: the two factors' errors add, the product rounds once (1), the four-term chain (3), every fp64 sum together (1: below 2^29 terms)
    K_E = 25 + 25 + 5 = 55;   K_G = K_J + 25 + 5 = 81 (translations), 83 (rotations);   K_H = K_Ji + K_Jj + 5 = 107, 109, 111
    |got - ref| <= K * 2^-24 * sum |terms| + 2^-126 * (number of terms)
with sum |terms| = sum Rm^2, sum Jm[i] Rm, sum Jm[i] Jm[j].  The bound is derived, never fitted to what the device gives; the GPU tests print
the worst ratio."""
import numpy as np

from ref_unproject import U, TINY, points
from ref_volume_merge import grid_coords, MIN_WS
from ref_volume_warp import corner_weights, rigid, warp_grid      # noqa: F401  (rigid, warp_grid: for the tests)
from ref_volume_match import K_DOT, K_NA, K_NB, lattice, match_grid, smooth_state      # noqa: F401  (smooth_state: for the tests)

K_R, K_DIFF, K_GRAD = 24 + 1, 2 + 1 + 1 + 4, (24 + 8 + 1) + 1 + 12 + 1 + 1
K_JT, K_JR = K_GRAD + 3, K_GRAD + 3 + 2
K_J = np.array([K_JT] * 3 + [K_JR] * 3)
K_E = K_R + K_R + 1 + 3 + 1
K_G = K_J + K_R + 1 + 3 + 1
TRIU = [(i, j) for i in range(6) for j in range(i, 6)]          # the upper triangle, row-major: the order of stats[10:31]
K_H = np.array([K_J[i] + K_J[j] + 1 + 3 + 1 for i, j in TRIU])
K_ALIGN = np.concatenate([[K_DOT, K_NA, K_NB, K_E], K_G, K_H]).astype(np.float64)
N_STATS = 31
assert (K_E, K_G.tolist(), sorted(set(K_H.tolist()))) == (55, [81] * 3 + [83] * 3, [107, 109, 111]) and len(K_ALIGN) == N_STATS


def full_H(tri):
    """The 21 numbers of the upper triangle, row-major -> the symmetric [6,6]."""
    H = np.zeros((6, 6))
    for n, (i, j) in enumerate(TRIU):
        H[i, j] = H[j, i] = tri[n]
    return H


def _coords(dims, vs, od, os_, M, geometry, own, robust):
    """-> (inside [N] bool, i0 [N,3] int64, f [N,3] float64, p [N,3] float64: the voxel centres, fp32 values unless geometry == 'float64')."""
    idx = np.stack(np.meshgrid(*(np.arange(d) for d in dims), indexing='ij'), -1).reshape(-1, 3).astype(np.float64)
    if geometry == 'float64':
        vs, od, os_, M = (np.asarray(v, np.float64) for v in (vs, od, os_, M))
        p = idx * vs + od
        g = ((p @ M[:3, :3].T + M[:3, 3]) - os_) / vs
        inside = np.all((g > -1) & (g < np.array(dims)), axis=1)
        fl = np.floor(np.where(inside[:, None], g, 0.0))
        return inside, fl.astype(np.int64), np.where(inside[:, None], g, 0.0) - fl, p
    assert geometry == 'float32', geometry
    inside, i0, f = grid_coords(dims, vs, od, os_, M)
    p = points(dims, np.asarray(vs, np.float32), np.asarray(od, np.float32))
    if robust:                                     # the exact chain on the same fp32 inputs picks the same cells
        v64, M64 = np.asarray(vs, np.float32).astype(np.float64), np.asarray(M, np.float32).astype(np.float64)
        g = ((p.astype(np.float64) @ M64[:3, :3].T + M64[:3, 3]) - np.asarray(os_, np.float32).astype(np.float64)) / v64
        in64 = np.all((g > -1) & (g < np.array(dims)), axis=1)
        assert np.array_equal(in64[own], inside[own]), 'a visited point too near the border of the source grid: fp32 and exact geometry differ on inside'
        sel = own & inside
        assert np.array_equal(np.floor(g[sel]).astype(np.int64), i0[sel]), 'a visited point too near a cell face: fp32 and exact geometry pick different cells'
    return inside, i0, f.astype(np.float64), p.astype(np.float64)


def align_grid(dst, src, voxel_size, origin_dst, origin_src, M, about, step=(1, 1, 1), robust=True, geometry='float32'):
    """One pair of rows and ONE candidate: dst = (S_d [X,Y,Z,C] fp32, W_d [X,Y,Z] fp32), src the same for the source row, about [3]
    -> dict(pairs, used, own: int; stats [31] float64 = (dot, na, nb, e, g[6], H upper triangle [21]); bound [31]; e, g [6], H [6,6];
    used_mask, paired [X,Y,Z] bool).  robust=False asserts nothing about decisions (a search that runs on this reference alone)."""
    Sd, Wd = dst[:2]
    Ss, Ws = src[:2]
    dims = tuple(Sd.shape[:3])
    Cn, N = Sd.shape[3], int(np.prod(dims))
    f32 = geometry == 'float32'
    vs = np.asarray(voxel_size, np.float32 if f32 else np.float64)
    visited = lattice(dims, step)
    with np.errstate(invalid='ignore'):
        own = visited & (Wd.reshape(N) > 0)
    inside, i0, f, p = _coords(dims, voxel_size, origin_dst, origin_src, M, geometry, own, robust)
    sel = np.flatnonzero(own & inside)                                          # everything below runs on these voxels only
    i0, f, p = i0[sel], f[sel], p[sel]
    if f32:
        w32, w64 = corner_weights(f.astype(np.float32))
    else:
        w64 = np.stack([np.where(c & 4, f[:, 0], 1 - f[:, 0]) * np.where(c & 2, f[:, 1], 1 - f[:, 1]) * np.where(c & 1, f[:, 2], 1 - f[:, 2]) for c in range(8)], 1)
        w32 = w64
    Sf, Wf = Ss.reshape(N, Cn), Ws.reshape(N)
    n = len(sel)
    Sc, Wc, inb = np.zeros((n, 8, Cn)), np.zeros((n, 8)), np.zeros((n, 8), bool)
    for c in range(8):
        idx = i0 + np.array([c >> 2, (c >> 1) & 1, c & 1])
        inb[:, c] = np.all((idx >= 0) & (idx < np.array(dims)), axis=1)
        flat = ((idx[inb[:, c], 0] * dims[1]) + idx[inb[:, c], 1]) * dims[2] + idx[inb[:, c], 2]
        Sc[inb[:, c], c], Wc[inb[:, c], c] = Sf[flat].astype(np.float64), Wf[flat].astype(np.float64)
    read = inb & (w32 != 0)                                                     # the corners the sample folds: the match's
    with np.errstate(invalid='ignore', over='ignore'):
        wr = np.where(read, w64, 0.0)
        smpW = np.where(read, wr * np.where(read, Wc, 0.0), 0.0).sum(1)
        paired = smpW > 0
        used = paired & inb.all(1) & (Wc > 0).all(1)
    if robust:
        assert (smpW[paired] >= MIN_WS).all(), 'the paired decision must be robust: a positive W_s too near 0'
        with np.errstate(invalid='ignore'):
            assert (Wc[inb & (Wc > 0)] >= MIN_WS).all(), 'the used decision must be robust: a positive corner weight sum too near 0'
    # ---- the match's three statistics over the paired voxels
    if f32:
        mg = match_grid(dst, src, voxel_size, origin_dst, origin_src, M, step, robust)
        assert mg['pairs'] == int(paired.sum()) and mg['own'] == int(own.sum())
        stats3, bound3 = mg['stats'], mg['bound']
    else:
        sp = np.flatnonzero(paired)
        a_ = Sd.reshape(N, Cn)[sel[sp]].astype(np.float64) / Wd.reshape(N)[sel[sp]].astype(np.float64)[:, None]
        b_ = np.einsum('nc,nck->nk', wr[sp], np.where(read[sp][:, :, None], Sc[sp], 0.0)) / smpW[sp][:, None]
        stats3, bound3 = np.array([(a_ * b_).sum(), (a_ * a_).sum(), (b_ * b_).sum()]), np.zeros(3)
    # ---- the used voxels
    su = np.flatnonzero(used)
    Sc, Wc, f, p, W_s, wr = Sc[su], Wc[su], f[su], p[su], smpW[su], wr[su]
    a = Sd.reshape(N, Cn)[sel[su]].astype(np.float64) / Wd.reshape(N)[sel[su]].astype(np.float64)[:, None]
    b = np.einsum('nc,nck->nk', wr, Sc) / W_s[:, None]                         # (a used voxel: every corner in the grid; weight 0 adds 0)
    B = np.einsum('nc,nck->nk', wr, np.abs(Sc)) / W_s[:, None]
    ax = [(1.0 - f[:, d], f[:, d]) for d in range(3)]
    grad, Gm = np.zeros((3, len(su), Cn)), np.zeros((3, len(su), Cn))
    for A in range(3):
        bit, (pa, P), (qa, Q) = 4 >> A, ((1, 2) if A == 0 else (0, 4)), ((1, 2) if A == 2 else (2, 1))
        dN, MN, dD, MD = np.zeros((len(su), Cn)), np.zeros((len(su), Cn)), np.zeros(len(su)), np.zeros(len(su))
        for pp in range(2):
            for qq in range(2):
                c0, w2 = pp * P + qq * Q, ax[pa][pp] * ax[qa][qq]
                dN += w2[:, None] * (Sc[:, c0 + bit] - Sc[:, c0])
                MN += w2[:, None] * (np.abs(Sc[:, c0 + bit]) + np.abs(Sc[:, c0]))
                dD += w2 * (Wc[:, c0 + bit] - Wc[:, c0])
                MD += w2 * (np.abs(Wc[:, c0 + bit]) + np.abs(Wc[:, c0]))
        grad[A] = (dN - b * dD[:, None]) / W_s[:, None] / float(vs[A])
        Gm[A] = (MN + B * MD[:, None]) / W_s[:, None] / float(vs[A])
    Rot = (np.asarray(M, np.float32).astype(np.float64) if f32 else np.asarray(M, np.float64))[:3, :3]
    u = np.einsum('ij,inc->jnc', Rot, grad)                                      # u = R^T grad
    Um = np.einsum('ij,inc->jnc', np.abs(Rot), Gm)
    if f32:
        d = (p.astype(np.float32) - np.asarray(about, np.float32)[None]).astype(np.float64)        # one rounded fp32 difference: the device's
    else:
        d = p - np.asarray(about, np.float64)[None]
    d, D = d.T[:, :, None], np.abs(d).T[:, :, None]
    J = np.stack([u[0], u[1], u[2], d[1] * u[2] - d[2] * u[1], d[2] * u[0] - d[0] * u[2], d[0] * u[1] - d[1] * u[0]])
    Jm = np.stack([Um[0], Um[1], Um[2], D[1] * Um[2] + D[2] * Um[1], D[2] * Um[0] + D[0] * Um[2], D[0] * Um[1] + D[1] * Um[0]])
    r, Rmag = b - a, np.abs(a) + B
    e, g = float((r * r).sum()), (J * r[None]).sum((1, 2))
    tri = np.array([(J[i] * J[j]).sum() for i, j in TRIU])
    mags = np.concatenate([[(Rmag * Rmag).sum()], (Jm * Rmag[None]).sum((1, 2)), [(Jm[i] * Jm[j]).sum() for i, j in TRIU]])
    stats = np.concatenate([stats3, [e], g, tri])
    bound = np.concatenate([bound3, K_ALIGN[3:] * U * mags + TINY * max(1, a.size)])
    def mask(m):
        out = np.zeros(N, bool)
        out[sel[m]] = True
        return out.reshape(dims)
    return dict(pairs=int(paired.sum()), used=int(used.sum()), own=int(own.sum()), stats=stats, bound=bound, e=e, g=g, H=full_H(tri),
                paired=mask(paired), used_mask=mask(used))


def align_rows(dst, src, voxel_size, origin_dst, origin_src, Ms, about, step=(1, 1, 1)):
    """... and K candidates -> dict(pairs [K], used [K] int64, own int, stats [K,31], bound [K,31], refs: the K dicts of align_grid)."""
    refs = [align_grid(dst, src, voxel_size, origin_dst, origin_src, M, about, step) for M in Ms]
    assert len({r['own'] for r in refs}) == 1, 'own does not depend on the candidate'
    return dict(pairs=np.array([r['pairs'] for r in refs], np.int64), used=np.array([r['used'] for r in refs], np.int64), own=refs[0]['own'],
                stats=np.stack([r['stats'] for r in refs]), bound=np.stack([r['bound'] for r in refs]), refs=refs)


def check(got, ref, what=''):
    """The device's (pairs [K], used [K], own, stats [K,31]) host arrays against align_rows' reference: counts equal, statistics within the bound.
    Prints and returns the worst ratios (match's three, e, g, H)."""
    pairs, used, own, stats = got
    assert int(own) == ref['own'], (what, int(own), ref['own'])
    assert np.array_equal(np.asarray(pairs, np.int64), ref['pairs']), (what, np.asarray(pairs).tolist(), ref['pairs'].tolist())
    assert np.array_equal(np.asarray(used, np.int64), ref['used']), (what, np.asarray(used).tolist(), ref['used'].tolist())
    ratio = np.abs(np.asarray(stats, np.float64) - ref['stats']) / ref['bound']
    worst = [float(ratio[:, :3].max()), float(ratio[:, 3].max()), float(ratio[:, 4:10].max()), float(ratio[:, 10:].max())]
    print(f'{what}: worst |got - ref| / bound  dot,na,nb {worst[0]:.3f}  e {worst[1]:.3f}  g {worst[2]:.3f}  H {worst[3]:.3f}  '
          f'(K_E = {K_E}, K_G = {K_G.min()} .. {K_G.max()}, K_H = {K_H.min()} .. {K_H.max()}); own {ref["own"]}, pairs {ref["pairs"].min()} .. '
          f'{ref["pairs"].max()}, used {ref["used"].min()} .. {ref["used"].max()}')
    assert max(worst) <= 1, (what, ratio.max(axis=0).tolist())
    return worst
