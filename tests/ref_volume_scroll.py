"""The numpy reference of the voxel scroll (include/imvoxel.h, ivx_volume_scroll_fwd), written from the definition:

    new[i,j,k] = old[i+sx, j+sy, k+sz]   where that source lies inside [0,X) x [0,Y) x [0,Z),   all bits zero elsewhere,

as ONE slice copy into a zero array, on integer views of the data so that no float operation can touch a bit pattern -- and the numpy statement
of the origin rule of a scrolling scene (imvoxelnet_amd.scene.scrolled_origin)."""
import numpy as np


def _as_words(a):
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4, a.dtype
    return a.view(np.int32)


def _span(L, s):
    """The destination and source slices of one axis of length L under shift s (empty when |s| >= L)."""
    lo, hi = max(0, -s), min(L, L - s)
    return (slice(lo, max(lo, hi)), slice(lo + s, max(lo, hi) + s))


def scroll_grid(a, shift):
    """a [X,Y,Z] or [X,Y,Z,C], any 4-byte dtype -> the scrolled array of the same dtype, bit for bit."""
    w = _as_words(a)
    out = np.zeros_like(w)
    dst, src = zip(*(_span(L, int(s)) for L, s in zip(w.shape[:3], shift)))
    out[dst] = w[src]
    return out.view(a.dtype)


def scroll_rows(pool, rows, shifts):
    """pool [R,X,Y,Z(,C)] -> a copy in which row rows[b] is scrolled by shifts[b]; every other row keeps its bits."""
    out = np.ascontiguousarray(pool).copy()
    for r, s in zip(rows, shifts):
        out[r] = scroll_grid(pool[r], s)
    return out


def stayed_inside(shape, shift):
    """bool [X,Y,Z]: the voxels of the scrolled grid whose source lay inside the grid (the others entered and are unseen)."""
    m = np.zeros(shape, bool)
    m[tuple(_span(L, int(s))[0] for L, s in zip(shape, shift))] = True
    return m


def scrolled_origin(origin, voxels, voxel_size):
    """float32(origin) + float32(voxels) * float32(voxel_size), per component: the product is rounded to fp32, then the sum."""
    out = np.empty(3, np.float32)
    for a in range(3):
        p = np.float32(np.float32(voxels[a]) * np.float32(voxel_size[a]))
        out[a] = np.float32(np.float32(origin[a]) + p)
    return out
