"""numpy restatement of ivx_volume_pack_fwd / ivx_volume_unpack_fwd (include/imvoxel.h): the ordered compaction of the kept voxels of one row of the
scene state and its inverse.  Written from the definition, not from the kernel.

Kept.     Voxel n of a row (flat index (i*Y + j)*Z + k) is kept iff its count word or its wsum word is non-zero, as raw 32-bit words:
          np.flatnonzero((count != 0) | (wsum.view(int32) != 0)).  A -0 or NaN weight sum is kept.
F32.      A record is the voxel's words: nothing is computed, so the comparison with the device is == on the bits.
BF16.     The payload is the mean m = den > 0 ? S / den : 0 (den the weight sum, or the count as a float) rounded to bf16, and the restore is
          S' = m * den.  Here both are computed in fp64 from the fp32 inputs, so the reference carries ONE rounding, the one to 8 significant bits.

The bound of the bf16 round trip on the device, for |S / den| in bf16's normal range and S, S' normal fp32 numbers:
    q  = fl32(S / den)   = (S / den)(1 + e1)     |e1| <= 2^-24     one IEEE division
    m  = bf16(q)         = q (1 + e2)            |e2| <= 2^-8      8 significant bits, round to nearest even: half an ulp of 2^-7
    S' = fl32(m * den)   = m den (1 + e3)        |e3| <= 2^-24     one rounded product
    S' = S (1 + e1)(1 + e2)(1 + e3),  so  |S' - S| / |S| <= 2^-8 + 2^-23 + (terms below 2^-31)  <=  2^-8 + 2^-22.
The fp64 reference itself lies within 2^-8 |S| (+ fp64 rounding) of S, inside the same bound."""
import numpy as np

BF16_BOUND = 2.0 ** -8 + 2.0 ** -22
BF16_MIN_NORMAL, BF16_MAX = 2.0 ** -126, (2.0 - 2.0 ** -7) * 2.0 ** 127


def words(a):
    """A float32 / int32 array as its raw 32-bit words."""
    return np.ascontiguousarray(a).view(np.int32)


def kept(count, wsum=None):
    """Ascending flat indices of the kept voxels of one row: count [...] int32, wsum [...] float32 or None."""
    k = np.ascontiguousarray(count).reshape(-1) != 0
    if wsum is not None:
        k = k | (words(wsum).reshape(-1) != 0)
    return np.flatnonzero(k).astype(np.int32)


def bf16_round(x):
    """float64 -> the nearest bf16 value (ties to even) as its uint16 word; x finite, |x| zero or in bf16's normal range."""
    x = np.asarray(x, np.float64)
    out = np.zeros(x.shape, np.uint16)
    nz = x != 0
    mant, exp = np.frexp(np.abs(x[nz]))           # |x| = mant * 2^exp, mant in [0.5, 1)
    sig = np.rint(mant * 256.0)                   # 8 significant bits; np.rint rounds half to even; 256 means the next binade
    bump = sig == 256
    sig, exp = np.where(bump, 128, sig), exp + bump
    biased = exp - 1 + 127                        # value = (sig / 128) * 2^(exp - 1)
    assert ((biased >= 1) & (biased <= 254)).all(), 'outside the normal range of bf16'
    w = (biased.astype(np.uint32) << 7) | (sig.astype(np.uint32) - 128) | np.where(np.signbit(x[nz]), 0x8000, 0).astype(np.uint32)
    out[nz] = w.astype(np.uint16)
    out[np.signbit(x) & ~nz] = 0x8000
    return out


def bf16_value(w):
    """uint16 bf16 words -> float64 values."""
    return (np.asarray(w, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def den_of(count_rec, wsum_rec):
    return (np.asarray(count_rec).astype(np.float32) if wsum_rec is None else np.asarray(wsum_rec, np.float32)).astype(np.float64)


def pack(vol_sum, count, wsum=None, bf16=False):
    """One row: vol_sum [X,Y,Z,C] float32, count [X,Y,Z] int32, wsum [X,Y,Z] float32 or None ->
    (index int32 [n], payload [n,C] float32 words or uint16 bf16 words, wsum [n] or None, count int32 [n])."""
    C = vol_sum.shape[-1]
    idx = kept(count, wsum)
    S = np.ascontiguousarray(vol_sum).reshape(-1, C)[idx]
    cnt = np.ascontiguousarray(count).reshape(-1)[idx]
    ws = None if wsum is None else np.ascontiguousarray(wsum).reshape(-1)[idx]
    if not bf16:
        return idx, S.copy(), ws, cnt
    den = den_of(cnt, ws)[:, None]
    mean = np.where(den > 0, S.astype(np.float64) / np.where(den > 0, den, 1.0), 0.0)
    return idx, bf16_round(mean), ws, cnt


def unpack(dims, C, records):
    """records (index, payload, wsum or None, count) -> one row (vol_sum [X,Y,Z,C], count [X,Y,Z], wsum [X,Y,Z] or None): listed voxels take their
    record, every other voxel is unseen, all bits zero.  A uint16 payload restores S = m * den in float64 (returned as float64)."""
    idx, pay, ws, cnt = records
    nvox = int(np.prod(dims))
    idx = np.asarray(idx, np.int64)
    assert (np.diff(idx) > 0).all() and (idx.size == 0 or (idx[0] >= 0 and idx[-1] < nvox)), 'indices strictly ascending inside the grid'
    bf16 = np.asarray(pay).dtype == np.uint16
    S = np.zeros((nvox, C), np.float64 if bf16 else np.float32)
    count, wsum = np.zeros(nvox, np.int32), (None if ws is None else np.zeros(nvox, np.float32))
    S[idx] = bf16_value(pay) * den_of(cnt, ws)[:, None] if bf16 else pay
    count[idx] = cnt
    if ws is not None:
        wsum[idx] = ws
    return S.reshape(tuple(dims) + (C,)), count.reshape(dims), (None if ws is None else wsum.reshape(dims))


def random_state(rng, dims, C, pattern='third', wsum=True, R=1, raw=True):
    """R rows of a state that meets the precondition (all-zero sums at unseen voxels): vol_sum [R,X,Y,Z,C] float32, count [R,X,Y,Z] int32, wsum
    [R,X,Y,Z] float32 or None.  raw: the sums of kept voxels are random bit patterns (NaNs, infs, -0 and denormals among them), else normal
    values.  pattern: which voxels are kept -- 'none', 'all', 'first', 'last', 'alternate', 'third' (a random third), 'chunks' (whole runs of 256
    voxels kept, whole runs empty, with ragged edges), 'mixed' (kept by count alone, by wsum alone, by a -0 wsum word, by a NaN wsum)."""
    nvox = int(np.prod(dims))
    keep = np.zeros((R, nvox), bool)
    if pattern == 'all':
        keep[:] = True
    elif pattern == 'first':
        keep[:, 0] = True
    elif pattern == 'last':
        keep[:, -1] = True
    elif pattern == 'alternate':
        keep[:, ::2] = True
    elif pattern in ('third', 'mixed'):
        keep = rng.random((R, nvox)) < 1 / 3
    elif pattern == 'chunks':
        run = (np.arange(nvox) + 37) // 256
        keep[:] = (run % 3 != 1) & ~((run % 3 == 2) & (np.arange(nvox) % 256 > 200))
    else:
        assert pattern == 'none', pattern
    count = np.where(keep, rng.integers(1, 9, (R, nvox)), 0).astype(np.int32)
    ws = np.where(keep, rng.uniform(0.25, 6.0, (R, nvox)), 0).astype(np.float32)
    if pattern == 'mixed':
        how = rng.integers(0, 4, (R, nvox))
        ws[keep & (how == 0)] = 0.0                                            # kept by count alone
        count[keep & (how >= 1)] = 0                                           # kept by the wsum word alone ...
        ws[keep & (how == 2)] = -0.0                                           # ... a -0 among them (the word is 0x80000000)
        ws[keep & (how == 3)] = np.nan
    if raw:
        S = rng.integers(-2 ** 31, 2 ** 31, (R, nvox, C), dtype=np.int64).astype(np.int32).view(np.float32)
        S[:, ::7, 0], S[:, ::11, 1 % C] = -0.0, np.float32(1e-41)
    else:
        S = (rng.uniform(0.5, 2.0, (R, nvox, C)) * rng.choice([-1.0, 1.0], (R, nvox, C))).astype(np.float32) * ws[..., None]
    S = np.where(keep[..., None], words(S), 0).astype(np.int32).view(np.float32)
    shape = (R,) + tuple(dims)
    return S.reshape(shape + (C,)), count.reshape(shape), (ws.reshape(shape) if wsum else None)
