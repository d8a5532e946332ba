"""The numpy reference of the scoring of candidate poses between two rows of the scene state (include/imvoxel.h, ivx_volume_match_fwd), written from
the definition, and the error bound of the fp32 kernel against it.

Steps 1 - 3 of the sample (centre from the DESTINATION origin, source point, grid coordinate against the SOURCE origin, floor and fraction) run
bit-exactly in fp32 -- tests/ref_volume_merge.grid_coords -- so that i0 and f are the device's, and the fp32 corner weights of
tests/ref_volume_warp.corner_weights decide which corners are read.  Values and sums run in float64 with the exact weights of the same f:
    a_c = S_d[c] / W_d,   b_c = S_s[c] / W_s,   dot = sum a_c b_c,   na = sum a_c^2,   nb = sum b_c^2   over the paired voxels and all channels.
pairs and own are integers and must be EQUAL, so every paired decision must be robust: wherever the float64 W_s is positive it is at least MIN_WS
(the rule of ref_volume_merge.merge_grid), or the reference refuses the input.

The bound, derived from the operation order the header fixes (u = 2^-24, first order).  Write A_c = |a_c| and B_c = sum_corners |w S_corner[c]| / W_s,
the magnitude sum of the sample over its weight (B_c >= |b_c|, with equality when the corner values of a channel share a sign).
    the sample          S_s carries the warp's K = 11 roundings per term (ref_volume_warp derives it): |S_s - exact| <= 11 u sum |w S_corner|.
                        W_s is the same chain over positive terms: a relative error of 11 u.
    the reciprocals     r = 1 / W is one IEEE division: r_d has 1 u, r_s has 11 u (from W_s) + 1 u.
    the means           a_c = S_d[c] * r_d, one rounded product:  1 + 1 = 2 u relative.
                        b_c = S_s[c] * r_s, one rounded product:  |b_c - exact| <= (11 + 12 + 1) u B_c = 24 u B_c.
    the product         a_c * b_c, a_c * a_c, b_c * b_c: the two factors' errors add and the product rounds once:
                        dot  24 + 2 + 1 = 27,   na  2 + 2 + 1 = 5,   nb  24 + 24 + 1 = 49   (in units of u A_c B_c, u A_c^2, u B_c^2).
    a lane's fp32 chain four products, three rounded sums in channel order: a term passes through at most three roundings of a running sum
                        whose magnitude the sum of the |terms| bounds:  + 3.  The chain is never longer: every four-term sum is widened to fp64.
    the trees           everything after that is fp64 -- the lane's walk, the tree over the lanes, the waves, the workgroups' partials: N terms
                        cost at most N 2^-53 relative to the sum of the |terms|, below 2^-24 for N < 2^29:  + 1.
    K_DOT = 31,  K_NA = 9,  K_NB = 53,   |got - ref| <= K * 2^-24 * sum |terms| + 2^-126 * (number of terms)
with sum |terms| = sum A_c B_c, sum A_c^2, sum B_c^2.  The bound is derived, never fitted to what the device gives; the GPU tests print the worst
ratio."""
import numpy as np

from ref_unproject import U, TINY
from ref_volume_merge import grid_coords, MIN_WS
from ref_volume_warp import corner_weights, rigid, warp_grid      # noqa: F401  (rigid, warp_grid: for the tests)

K_DOT, K_NA, K_NB = 24 + 2 + 1 + 3 + 1, 2 + 2 + 1 + 3 + 1, 24 + 24 + 1 + 3 + 1
K_MATCH = np.array([K_DOT, K_NA, K_NB], np.float64)


def lattice(dims, step=(1, 1, 1)):
    """[N] bool: the voxels n = (i*Y + j)*Z + k a lattice step visits, i % px == 0 && j % py == 0 && k % pz == 0."""
    i, j, k = np.meshgrid(*(np.arange(d) for d in dims), indexing='ij')
    return ((i % step[0] == 0) & (j % step[1] == 0) & (k % step[2] == 0)).reshape(-1)


def match_grid(dst, src, voxel_size, origin_dst, origin_src, M, step=(1, 1, 1), robust=True):
    """One pair of rows and ONE candidate: dst = (S_d [X,Y,Z,C] fp32, W_d [X,Y,Z] fp32), src the same for the source row (a third entry, the counts,
    is ignored) -> dict(pairs, own: int; stats [3] float64 = (dot, na, nb); bound [3]: the error bounds; visited, own_mask, inside, paired [X,Y,Z]
    bool; read [X,Y,Z,8] bool: the corners read; Ws: the float64 sample of the weight sum).  Asserts that the paired decision is robust (robust=False: does not -- only
    for a search that runs on this reference alone and is compared with no device)."""
    Sd, Wd = dst[:2]
    Ss, Ws = src[:2]
    dims = tuple(Sd.shape[:3])
    Cn, N = Sd.shape[3], int(np.prod(dims))
    visited = lattice(dims, step)
    with np.errstate(invalid='ignore'):
        own = visited & (Wd.reshape(N) > 0)
    inside, i0, f = grid_coords(dims, voxel_size, origin_dst, origin_src, M)
    w32, w64 = corner_weights(f)
    Sf, Wf = Ss.reshape(N, Cn), Ws.reshape(N)
    smpS, smpW, absS, read = np.zeros((N, Cn)), np.zeros(N), np.zeros((N, Cn)), np.zeros((N, 8), bool)
    for c in range(8):
        idx = i0 + np.array([c >> 2, (c >> 1) & 1, c & 1])
        rd = own & inside & (w32[:, c] != 0) & np.all((idx >= 0) & (idx < np.array(dims)), axis=1)
        flat = ((idx[rd, 0] * dims[1]) + idx[rd, 1]) * dims[2] + idx[rd, 2]
        w = w64[rd, c]
        with np.errstate(invalid='ignore', over='ignore'):
            smpS[rd] += w[:, None] * Sf[flat].astype(np.float64)
            smpW[rd] += w * Wf[flat].astype(np.float64)
            absS[rd] += np.abs(w[:, None] * Sf[flat].astype(np.float64))
        read[:, c] = rd
    with np.errstate(invalid='ignore'):
        paired = own & inside & (smpW > 0)
    assert not robust or (smpW[paired] >= MIN_WS).all(), 'the paired decision must be robust: a positive W_s too near 0'
    a = Sd.reshape(N, Cn)[paired].astype(np.float64) / Wd.reshape(N)[paired].astype(np.float64)[:, None]
    b, B = smpS[paired] / smpW[paired][:, None], absS[paired] / smpW[paired][:, None]
    stats = np.array([(a * b).sum(), (a * a).sum(), (b * b).sum()])
    mags = np.array([(np.abs(a) * B).sum(), (a * a).sum(), (B * B).sum()])
    sh = lambda m: m.reshape(dims)                                            # noqa: E731
    return dict(pairs=int(paired.sum()), own=int(own.sum()), stats=stats, bound=K_MATCH * U * mags + TINY * max(1, a.size),
                visited=sh(visited), own_mask=sh(own), inside=sh(inside), paired=sh(paired), read=read.reshape(dims + (8,)), Ws=sh(smpW))


def match_rows(dst, src, voxel_size, origin_dst, origin_src, Ms, step=(1, 1, 1)):
    """... and K candidates -> dict(pairs [K] int64, own int, stats [K,3], bound [K,3], refs: the K dicts of match_grid)."""
    refs = [match_grid(dst, src, voxel_size, origin_dst, origin_src, M, step) for M in Ms]
    assert len({r['own'] for r in refs}) == 1, 'own does not depend on the candidate'
    return dict(pairs=np.array([r['pairs'] for r in refs], np.int64), own=refs[0]['own'], stats=np.stack([r['stats'] for r in refs]),
                bound=np.stack([r['bound'] for r in refs]), refs=refs)


def score(pairs, own, stats, min_overlap=0.3):
    """The host's score of K candidates from the device's or the reference's outputs: ncc = dot / sqrt(na * nb), -inf where pairs == 0, overlap =
    pairs / own < min_overlap or a norm is not positive.  -> (score [K], overlap [K])."""
    pairs, stats = np.asarray(pairs, np.float64).reshape(-1), np.asarray(stats, np.float64).reshape(-1, 3)
    overlap = pairs / own if own > 0 else np.zeros(len(pairs))
    den = stats[:, 1] * stats[:, 2]
    ok = (pairs > 0) & (overlap >= min_overlap) & (den > 0)
    return np.where(ok, stats[:, 0] / np.sqrt(np.where(ok, den, 1.0)), -np.inf), overlap


def check(got, ref, what=''):
    """The device's (pairs [K], own, stats [K,3]) host arrays against match_rows' reference: counts equal, statistics within the bound.  Prints
    and returns the worst ratio."""
    pairs, own, stats = got
    assert int(own) == ref['own'], (what, int(own), ref['own'])
    assert np.array_equal(np.asarray(pairs, np.int64), ref['pairs']), (what, np.asarray(pairs).tolist(), ref['pairs'].tolist())
    ratio = np.abs(np.asarray(stats, np.float64) - ref['stats']) / ref['bound']
    worst = float(ratio.max())
    print(f'{what}: worst |got - ref| / bound  dot {ratio[:, 0].max():.3f}  na {ratio[:, 1].max():.3f}  nb {ratio[:, 2].max():.3f}  '
          f'(K = {K_DOT}, {K_NA}, {K_NB}); own {ref["own"]}, pairs {ref["pairs"].min()} .. {ref["pairs"].max()}')
    assert worst <= 1, (what, ratio.max(axis=0).tolist())
    return worst


def smooth_state(dims, C, seed, unseen=0.1, voxel_size=(0.16, 0.16, 0.2)):
    """A smooth source row (S, W, cnt): per channel the mean is a sum of 6 cosines with wavelengths between 0.5 and 2 grid extents, weights in
    [0.5, 4), counts in 1 .. 8, and `unseen` of the voxels unseen -- as one slab at the low-x end, so no seen voxel sits alone among unseen ones."""
    rng = np.random.default_rng(seed)
    ext = np.asarray(dims) * np.asarray(voxel_size)
    p = np.stack(np.meshgrid(*(np.arange(d) * v for d, v in zip(dims, voxel_size)), indexing='ij'), -1)           # [X,Y,Z,3]
    mean = np.zeros(dims + (C,))
    for c in range(C):
        for _ in range(6):
            d = rng.standard_normal(3)
            k = d / np.linalg.norm(d) / (rng.uniform(0.5, 2.0) * ext)         # cycles per metre along each axis: a wavelength of 0.5 .. 2 extents
            mean[..., c] += rng.uniform(0.5, 1.5) * np.cos(2 * np.pi * (p @ k) + rng.uniform(0, 2 * np.pi))
    W = rng.uniform(0.5, 4.0, dims).astype(np.float32)
    S, cnt = (mean * W[..., None]).astype(np.float32), rng.integers(1, 9, dims).astype(np.int32)
    gone = np.zeros(dims, bool)
    gone[:max(1, int(round(unseen * dims[0])))] = True
    S[gone], W[gone], cnt[gone] = 0, 0, 0
    return S, W, cnt
