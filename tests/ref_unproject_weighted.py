"""fp64 reference of the WEIGHTED listed lift (ivx_backproject_weighted_fwd), written from its definition in include/imvoxel.h, for both sampling
rules, and the error bound of the fp32 kernel against it.  Plain numpy on top of ref_unproject (projection inputs, validity rule, corners).

Like ref_unproject it takes the fp32 quotients xf, yf and the depth d as inputs, so no floor / rint decision can differ from the kernel's.  The
weights and the decays are the fp32 numbers the kernel reads, used exactly (as fp64).  The state is carried in fp64 from tick to tick:
  start   S, W, cnt from the previous tick (zero with `first`)
  fade    S *= lambda, W *= lambda; then, if !(W >= forget_below): S = W = cnt = 0
  add     every listed view whose weight passes w > 0 && w < inf and that sees the voxel: S += w * sample, W += w, ++cnt
  store   mean = W > 0 ? S / W : 0, valid = W > 0
"""
import numpy as np

import ref_unproject as R

U, TINY, U_BF16, TINY_BF16 = R.U, R.TINY, R.U_BF16, R.TINY_BF16


def k_weighted(n_views, n_fades, bilinear):
    """Roundings between the fp64 value and the fp32 kernel, counted from the fixed order of include/imvoxel.h as ref_unproject.k_bilinear counts:
      view sum    one rounding per counted view: S = fma(w, sample, S)                                                   n_views
      weight sum  one rounding per addition into W                                                                       n_views
      mean        one division                                                                                           1
      fade        two per fading tick: lambda * S and lambda * W                                                         2 * n_fades
      sample      the six of the bilinear sample (2 for its weights, 4 through its blend); the nearest sample is exact   6 | 0
    n_views: the most views any voxel can have counted since the state was started; n_fades: the ticks that multiplied it by lambda != 1.
    Every term is bounded by its share of A = sum_v w_eff,v sum_i b_i |f_i| / W (w_eff: the weight times the decays applied since; b_i: the
    bilinear corner weights), so |got - ref| <= K * 2^-24 * A to first order; an error of W moves the mean by that fraction of |mean| <= A."""
    return 2 * n_views + 1 + 2 * n_fades + (6 if bilinear else 0)


def _samples(feat_v, xf, yf, n, hc, wc, bilinear):
    """The fp64 sample of view map feat_v [FH, FW, C] at the voxels n, and its magnitude sum_i b_i |f_i|."""
    if not bilinear:
        f = feat_v[np.rint(yf[n]).astype(np.int64), np.rint(xf[n]).astype(np.int64)]
        return f, np.abs(f)
    x0, x1, y0, y1, ax, ay = R.corners(xf[n], yf[n], hc, wc)
    ax, ay = ax.astype(np.float64)[:, None], ay.astype(np.float64)[:, None]
    val, mag = 0.0, 0.0
    for b, yy, xx in (((1 - ax) * (1 - ay), y0, x0), (ax * (1 - ay), y0, x1), ((1 - ax) * ay, y1, x0), (ax * ay, y1, x1)):
        f = feat_v[yy, xx]
        val, mag = val + b * f, mag + b * np.abs(f)
    return val, mag


class WeightedReference:
    """The running fp64 state of ONE sample.  feat [V, FH, FW, C] (the maps of all its views), xf, yf, d [V, N] fp32, hc, wc: the clamped crop."""

    def __init__(self, feat, xf, yf, d, hc, wc, bilinear=False, forget_below=0.0):
        self.feat, self.xf, self.yf, self.hc, self.wc, self.bilinear = np.asarray(feat, np.float64), xf, yf, hc, wc, bool(bilinear)
        self.ok = R.valid_views(xf, yf, d, hc, wc)
        self.fb = float(np.float32(forget_below))
        N, Cn = xf.shape[1], self.feat.shape[-1]
        self.S, self.M, self.W, self.cnt = np.zeros((N, Cn)), np.zeros((N, Cn)), np.zeros(N), np.zeros(N, np.int64)

    def tick(self, views, weights, decay=1.0, first=False):
        """One call: fade the state (unless first), then add `views` (indices into feat) with `weights` (one per listed view).  Returns result()."""
        lam = float(np.float32(decay))
        if first:
            self.S[:], self.M[:], self.W[:], self.cnt[:] = 0, 0, 0, 0
        else:
            if lam != 1.0:
                self.S *= lam
                self.M *= lam
                self.W *= lam
            gone = ~(self.W >= self.fb)
            self.S[gone], self.M[gone], self.W[gone], self.cnt[gone] = 0, 0, 0, 0
        for v, w in zip(views, weights):
            w = float(np.float32(w))
            if not (w > 0 and w < np.inf):
                continue
            n = np.nonzero(self.ok[v])[0]
            val, mag = _samples(self.feat[v], self.xf[v], self.yf[v], n, self.hc, self.wc, self.bilinear)
            self.S[n] += w * val
            self.M[n] += w * mag
            self.W[n] += w
            self.cnt[n] += 1
        return self.result()

    def result(self):
        """dict(mean [N,C], valid [N], count [N], W [N], A [N,C], S [N,C], M [N,C]): M = sum w_eff |sample|, A = M / W (0 where W == 0)."""
        seen = self.W > 0
        den = np.where(seen, self.W, 1.0)[:, None]
        return dict(mean=np.where(seen[:, None], self.S / den, 0.0), valid=seen.copy(), count=self.cnt.copy(), W=self.W.copy(),
                    A=np.where(seen[:, None], self.M / den, 0.0), S=self.S.copy(), M=self.M.copy())


def weighted_mean_reference(feat, xf, yf, d, hc, wc, views, weights, bilinear=False):
    """The mean mode: one tick from zero."""
    return WeightedReference(feat, xf, yf, d, hc, wc, bilinear).tick(views, weights, first=True)


def bound(A, K, ref=None, bf16=False):
    """|got - ref| <= K * 2^-24 * A + 2^-126; bf16 storage: one more rounding of the result (ref_unproject.bound's store term).  For the sums pass
    M in place of A (no division: the bound is then one rounding generous)."""
    b = K * U * A + TINY
    if bf16:
        b = b + U_BF16 * (np.abs(ref) + b) + TINY_BF16
    return b
