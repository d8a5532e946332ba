"""numpy reference of the view coverage counts (ivx_view_coverage_fwd), written from the definition in include/imvoxel.h on top of ref_unproject:
`points`, `project` and `valid_views` restate the lift's fp32 chain exactly (every rounding emulated), so every decision here is the kernel's
decision and the counts are compared with ==.  The two tests the pixel maps add are restated in fp32 as in ref_unproject_maps: the gate
d <= float32(D + behind) and d >= float32(D - front) on a measured D (D > 0 && D < inf), and w > 0 && w < inf on the map's value (the view
weight is 1, and 1 * w is w).  The evidence rule is fresh = !(den >= fresh_below) with den in fp32.  Counts are int64.
"""
import numpy as np

import ref_unproject as R

NONE, COUNT, WSUM, MASK = 0, 1, 2, 3
INF = np.float32(np.inf)


def den_of(state_row, kind, n):
    """The evidence [n] fp32 of one state row (any shape of n elements), by kind."""
    if kind == NONE:
        return np.zeros(n, np.float32)
    s = np.asarray(state_row).reshape(-1)
    assert s.shape == (n,)
    if kind == COUNT:
        return s.astype(np.int32).astype(np.float32)
    if kind == WSUM:
        return s.astype(np.float32)
    assert kind == MASK
    return (s != 0).astype(np.float32)


def fresh_of(den, fresh_below):
    """!(den >= fresh_below) in fp32: a NaN evidence is fresh, equality is not."""
    with np.errstate(invalid='ignore'):
        return ~(np.asarray(den, np.float32) >= np.float32(fresh_below))


def sees(proj, n_voxels, voxel_size, new_origin, crop, fhw, pixel_weight=None, depth=None, gate=(np.inf, np.inf)):
    """proj [V,3,4] fp32 (the candidates' rows); pixel_weight, depth: [V,FH,FW] fp32 or None (indexed like proj) -> bool [V,N]: candidate v
    counts at voxel n."""
    pts = R.points(n_voxels, voxel_size, new_origin)
    xf, yf, d = R.project(np.asarray(proj, np.float32), pts)
    hc, wc = min(int(crop[0]), int(fhw[0])), min(int(crop[1]), int(fhw[1]))
    ok = R.valid_views(xf, yf, d, hc, wc)
    behind, front = np.float32(gate[0]), np.float32(gate[1])
    for v in range(ok.shape[0]):
        n = np.nonzero(ok[v])[0]                       # the maps are read only where the validity test has passed
        yr, xr = np.rint(yf[v, n]).astype(np.int64), np.rint(xf[v, n]).astype(np.int64)
        keep = np.ones(len(n), bool)
        with np.errstate(invalid='ignore'):
            if depth is not None:
                D, dd = np.asarray(depth, np.float32)[v, yr, xr], d[v, n]
                meas = (D > 0) & (D < INF)
                inside = (dd <= (D + behind).astype(np.float32)) & (dd >= (D - front).astype(np.float32))     # one fp32 sum, one fp32 difference
                keep &= ~meas | inside
            if pixel_weight is not None:
                w = np.asarray(pixel_weight, np.float32)[v, yr, xr]
                keep &= (w > 0) & (w < INF)
        ok[v, n] = keep
    return ok


def coverage(proj, n_voxels, voxel_size, new_origin, crop, fhw, state_row=None, kind=NONE, fresh_below=1.0, pixel_weight=None, depth=None,
             gate=(np.inf, np.inf)):
    """One sample: -> int64 [V,2], columns (seen, fresh)."""
    ok = sees(proj, n_voxels, voxel_size, new_origin, crop, fhw, pixel_weight, depth, gate)
    fresh = fresh_of(den_of(state_row, kind, ok.shape[1]), fresh_below)
    return np.stack([ok.sum(1), (ok & fresh[None]).sum(1)], 1).astype(np.int64)


def coverage_lists(proj_pool, lists, rows, n_voxels, voxel_size, new_origin, crop, fhw, state=None, kind=NONE, fresh_below=1.0, pixel_weight=None,
                   depth=None, gate=(np.inf, np.inf)):
    """The whole call: proj_pool [S,3,4]; lists: B ragged lists of slots (-1 and slots outside [0, S) see nothing); rows [B]; new_origin [B,3];
    crop [B,2]; state [R,...] or None; the maps [S,FH,FW] indexed by slot -> int64 [B,V,2], V the longest list, padding (0, 0)."""
    proj_pool = np.asarray(proj_pool, np.float32)
    S, V = len(proj_pool), max(1, max(len(l) for l in lists))
    out = np.zeros((len(lists), V, 2), np.int64)
    for b, l in enumerate(lists):
        at = [(i, s) for i, s in enumerate(l) if 0 <= s < S]
        if not at:
            continue
        slots = [s for _, s in at]
        c = coverage(proj_pool[slots], n_voxels, voxel_size, new_origin[b], crop[b], fhw, None if state is None else state[rows[b]], kind, fresh_below,
                     None if pixel_weight is None else np.asarray(pixel_weight)[slots], None if depth is None else np.asarray(depth)[slots], gate)
        out[b, [i for i, _ in at]] = c
    return out
