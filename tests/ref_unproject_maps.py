"""fp64 reference of the weighted listed lift WITH PIXEL MAPS (ivx_backproject_mapped_fwd), written from its definition in include/imvoxel.h on top
of ref_unproject_weighted (start, fade, forget, store, the sample functions) and ref_unproject (projection inputs, validity rule).

Only step 3 of the weighted definition, "a view counts", changes.  Both new tests are DECISIONS, and they are restated here in fp32 exactly as the
kernel makes them, so that none can differ from the kernel's: the nearest pixel (xr, yr) = (rint(xf), rint(yf)) of the fp32 quotients the
reference takes as inputs; the gate  d <= float32(D + behind)  and  d >= float32(D - front)  on a measured D (D > 0 && D < inf), one np.float32
sum and one np.float32 difference; the weight test  w > 0 && w < inf  on the np.float32 product  w = wv * pixel_weight[yr, xr].  The VALUES are
fp64: a counted view enters with the exact product  float64(wv) * float64(pixel_weight)  -- the kernel's rounded product is one of the roundings
the bound counts.
"""
import numpy as np

import ref_unproject as R
import ref_unproject_weighted as RW

INF = float('inf')


def k_mapped(n_views, n_fades, bilinear, weight_map=True):
    """Roundings between the fp64 value and the fp32 kernel: those of ref_unproject_weighted.k_weighted, plus
      effective weight   one rounding per counted view: w = wv * pixel_weight                                            n_views
    (none without a pixel_weight map: w = wv is the number the reference uses).  Why one unit of 2^-24 * A per counted view covers it: the
    kernel's w_i is the exact product times (1 + e_i), |e_i| <= 2^-24.  The sums move by sum_i e_i w_i f_i, at most 2^-24 * M in all -- not per
    view -- and the mean  sum w_i (1 + e_i) f_i / sum w_i (1 + e_i)  moves, to first order, by  sum_i e_i w_i (f_i - mean) / W, at most
    2^-24 * (A + |mean|) <= 2 * 2^-24 * A in all.  n_views units cover both whenever two or more views were counted; with one counted view
    and no earlier state the factor cancels in S / W and the mean does not move at all.  (The roundings of the later fma chain act on the
    perturbed numbers: second order.)  The count is arithmetic, not a measurement.  n_views, n_fades, bilinear: as for k_weighted."""
    return RW.k_weighted(n_views, n_fades, bilinear) + (n_views if weight_map else 0)


def _f32(a):
    return np.asarray(a, np.float32)


class MappedReference(RW.WeightedReference):
    """The running fp64 state of ONE sample whose views bring maps.  feat [V,FH,FW,C], xf, yf, d [V,N] fp32, hc, wc as for WeightedReference;
    pixel_weight, depth: [V,FH,FW] fp32 (indexed by the view's index into feat) or None; gate = (behind, front)."""

    def __init__(self, feat, xf, yf, d, hc, wc, bilinear=False, forget_below=0.0, pixel_weight=None, depth=None, gate=(INF, INF)):
        super().__init__(feat, xf, yf, d, hc, wc, bilinear, forget_below)
        self.d = _f32(d)
        self.pw = None if pixel_weight is None else _f32(pixel_weight)
        self.D = None if depth is None else _f32(depth)
        self.behind, self.front = np.float32(gate[0]), np.float32(gate[1])

    def classes(self, v):
        """The (view, voxel) pairs of view v that pass validity, split by the gate alone: (holes, too far, too near, pass) as index arrays into
        the voxels.  Without a depth map every pair is a hole."""
        n = np.nonzero(self.ok[v])[0]
        if self.D is None:
            return n, n[:0], n[:0], n[:0]
        yr, xr = np.rint(self.yf[v, n]).astype(np.int64), np.rint(self.xf[v, n]).astype(np.int64)
        D, dd = self.D[v, yr, xr], self.d[v, n]
        with np.errstate(invalid='ignore'):
            meas = (D > 0) & (D < np.float32(INF))
            far = meas & ~(dd <= (D + self.behind).astype(np.float32))          # one fp32 sum
            near = meas & ~far & ~(dd >= (D - self.front).astype(np.float32))    # one fp32 difference
        return n[~meas], n[far], n[near], n[meas & ~far & ~near]

    def counted(self, v, wv):
        """(voxels at which view v of weight wv counts, its fp64 weight at each of them)."""
        wv = np.float32(wv)
        if not (wv > 0 and wv < INF):
            return np.zeros(0, np.int64), np.zeros(0)
        holes, _, _, passed = self.classes(v)
        n = np.sort(np.concatenate([holes, passed]))
        if self.pw is None:
            return n, np.full(len(n), float(wv))
        pw = self.pw[v, np.rint(self.yf[v, n]).astype(np.int64), np.rint(self.xf[v, n]).astype(np.int64)]
        with np.errstate(invalid='ignore', over='ignore'):
            w32 = (wv * pw).astype(np.float32)                                   # the kernel's rounded product decides
            keep = (w32 > 0) & (w32 < np.float32(INF))
        return n[keep], float(wv) * pw[keep].astype(np.float64)                  # the exact product is the value

    def tick(self, views, weights, decay=1.0, first=False):
        """One call: start / fade / forget as WeightedReference (a tick of no views), then the views that count, each with its per-voxel weight."""
        super().tick([], [], decay, first)
        for v, wv in zip(views, weights):
            n, w = self.counted(v, wv)
            val, mag = RW._samples(self.feat[v], self.xf[v], self.yf[v], n, self.hc, self.wc, self.bilinear)
            self.S[n] += w[:, None] * val
            self.M[n] += w[:, None] * mag
            self.W[n] += w
            self.cnt[n] += 1
        return self.result()


def mapped_mean_reference(feat, xf, yf, d, hc, wc, views, weights, bilinear=False, pixel_weight=None, depth=None, gate=(INF, INF)):
    """The mean mode: one tick from zero."""
    return MappedReference(feat, xf, yf, d, hc, wc, bilinear, 0.0, pixel_weight, depth, gate).tick(views, weights, first=True)


bound = RW.bound


# ------------------------------------------------------------------ the maps of the tests, on the dyadic scene of ref_unproject
GATE = (0.25, 0.5)
HOLES = (0.0, float('nan'), -1.0, INF)      # how a pixel says "no measurement"


def dyadic_depth(V=3):
    """[V,FH,FW] fp32: D[v,y,x] = 1 + 0.25 * ((x + 2y + v) mod 5), dyadic, so that every D + behind and D - front with a dyadic gate is exact;
    holes where (x + y) mod 4 == 0, written as 0, NaN, -1 and +inf in turn (by (x + v) mod 4)."""
    v, y, x = np.meshgrid(np.arange(V), np.arange(R.FH), np.arange(R.FW), indexing='ij')
    D = (1 + 0.25 * ((x + 2 * y + v) % 5)).astype(np.float32)
    hole = (x + y) % 4 == 0
    D[hole] = np.asarray(HOLES, np.float32)[(x + v) % 4][hole]
    return D


def general_weight_map(V=3, seed=11):
    """[V,FH,FW] fp32 confidences in [0.25, 1.75) with no structure, and a sprinkling of pixels that block their view: 0, NaN, a negative value
    and +inf where (2x + 3y + v) mod 7 == 0."""
    pw = (0.25 + 1.5 * np.random.default_rng(seed).random((V, R.FH, R.FW))).astype(np.float32)
    v, y, x = np.meshgrid(np.arange(V), np.arange(R.FH), np.arange(R.FW), indexing='ij')
    bad = (2 * x + 3 * y + v) % 7 == 0
    pw[bad] = np.asarray([0.0, float('nan'), -0.5, INF], np.float32)[(x + y + v) % 4][bad]
    return pw
