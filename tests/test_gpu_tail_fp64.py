"""-m gpu: the detection tail (csrc/anchor_tail.hip) through its public entry points, each against the plain fp64 reference of the same
operation in tests/ref_tail.py -- not against the C oracle, which restates the kernels in fp32 in their own operation order, and not
against another form of the same code.  The cases, drivers, bounds and decision margins are those of tests/test_host_tail_fp64.py, which
proves them on the CPU restatement: sizes below, at and above one 64-lane mask word, nms_pre below, at and above n, 1 to 3 anchors per
location, both memory orders, padded channel blocks, B = 3, a score exactly at score_thr, empty results, max_num = 1,
dir_limit_offset = 0.5, FCOS grids with three extents, per-sample level geometry, the 4-of-8 / 5-of-8 rule of the pooled mask,
suppression chains across mask words, and either side of n = 16384 where the chip-wide top-k takes over.

Outputs are pre-filled with NaN (floats) or -7 (integers): an unwritten row shows.  Kept indices, labels, counts and order must be
identical to the reference's in every case; continuous outputs stay within the derived bounds; every test prints its worst ratio."""
import ctypes as C

import numpy as np
import pytest
import torch

import ref_tail as T

pytestmark = pytest.mark.gpu


class GpuBackend:
    """ref_tail.HostBackend's twin on device memory"""
    name = 'gpu'

    def __init__(self, L):
        from imvoxelnet_amd import _lib
        self.L = L
        self.AnchorHeadDesc, self.IndoorTailDesc = _lib.AnchorHeadDesc, _lib.IndoorTailDesc

    @property
    def stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def up(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def full(self, shape, dtype, fill):
        return torch.full(tuple(shape), fill, device='cuda', dtype=getattr(torch, np.dtype(dtype).name))

    def ptr(self, h, byte_offset=0):
        return C.c_void_p(h.data_ptr() + byte_offset) if h is not None else None

    def get(self, h):
        torch.cuda.synchronize()
        return h.cpu().numpy()

    def ok(self, rc, what):
        from imvoxelnet_amd import _lib
        _lib.check(rc, what)

    def workspace(self, nbytes):
        raw = torch.zeros(int(nbytes) + 512, device='cuda', dtype=torch.uint8)
        return raw, C.c_void_p(raw.data_ptr() + (-raw.data_ptr() % 256))


@pytest.fixture(scope='module')
def be():
    from imvoxelnet_amd import _lib
    lib = _lib.lib()
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    return GpuBackend(lib)


@pytest.mark.parametrize('cls', T.OVERLAP_CLASSES)
def test_boxes_overlap_bev_vs_fp64(be, cls):
    """ivx_boxes_overlap_bev, overlap and IoU, 1x1, 1x65, 63x64, 65x3, both argument orders, per configuration class within
    ref_tail.OVERLAP_SLACK x the C oracle's measured error of that class (ref_tail.OVERLAP_MEASURED); shared edges and touching corners are
    0 in fp64, identical boxes give the area."""
    print(f'gpu overlap {cls}: worst error / ({T.OVERLAP_SLACK} x measured bound {T.OVERLAP_MEASURED[cls]:.1e}) = {T.run_overlap(be, cls):.3f}')


@pytest.mark.parametrize('rotated', [0, 1])
def test_nms_bev_vs_fp64(be, rotated):
    """ivx_nms_bev at n = 0, 1, 2, 63, 64, 65, 128, 129, 300, thresholds 0.1 and 0.7: identical boxes keep 1, disjoint boxes keep n, chains
    across the word boundaries 63 | 64 | 65 and 127 | 128 | 129 keep the third box, a box that overlaps only a box of lower score; axis-aligned
    also n = 4097 (the removal words in LDS).  The kept list is identical to greedy_nms in fp64, whose decision margin is asserted >= 1e-3."""
    print(f'gpu nms rotated={rotated}: smallest decision margin |IoU - thr| of the reference = {T.run_nms(be, bool(rotated)):.3e} (required {T.IOU_MARGIN})')


def test_anchor_head_vs_fp64(be):
    """ivx_anchor_head_get_bboxes with the candidate outputs on, ref_tail.anchor_cases(): candidate indices identical, candidate boxes and scores
    within the rounding counts K_XY = 7, K_Z = 9, K_SIZE = 5, K_ROT = 1, K_SIGMOID = 6, kept boxes (yaw: K_YAW = 6), scores, labels, count and the
    zero rows beyond count."""
    worst, marg = T.run_anchor_head(be)
    print(f'gpu anchor head: worst error / bound = {worst:.3f}; reference margins {marg}')


@pytest.mark.parametrize('grid', T.TOPK_GRIDS)
def test_fcos_topk_forms_vs_fp64(be, grid):
    """The top-k forms through ivx_fcos_head_level_candidates at n = 16383 (one-workgroup select) and n = 16384 (histogram form), k = 1, 64,
    1000: spread scores, all scores inside one first-level radix bin, a bit-equal block straddling the cut, more than 8192 bit-equal scores
    at the cut (the fallback).  The reference order is one np.lexsort; the boxes identify the voxels."""
    worst, margin = T.run_fcos_topk(be, grid)
    print(f'gpu fcos top-k grid {grid}: worst error / bound = {worst:.3f}; smallest relative score gap that decides = {margin:.2e}')


def test_fcos_levels_vs_fp64(be):
    """ivx_fcos_head_level_candidates on grids with three different extents at levels 0, 1, 2, R = 6 and 7, CH above 1 + R + ncls, scale != 1,
    level geometry that differs between the two samples, a level-0 mask whose pooled cells see 0, 3, 4, 5, 6 and 8 set voxels, nms_pre below and
    above n.  Scores within K_FCOS_SCORE = 13, boxes within the propagated bound of ref_tail.fcos_level_candidates."""
    worst, margin = T.run_fcos_levels(be)
    print(f'gpu fcos levels: worst error / bound = {worst:.3f}; smallest relative score gap that decides = {margin:.2e}')


def test_multiclass_nms_vs_fp64(be):
    """ivx_multiclass_nms_bev: 1, 2, 3, 64 classes, n = 1, 64, 65, 200, score_stride = num_classes (+ 1), a class without and a class with one
    candidate, a score exactly at score_thr, max_num on both sides of the cut and between equal scores of two classes, rotated and axis-aligned."""
    print(f'gpu multi-class nms: smallest decision margin = {T.run_multiclass(be):.3e}')


def test_aligned_3d_nms_vs_fp64(be):
    """ivx_aligned_3d_nms and _ws at n = 1, 2, 64, 65, 300: touching and identical boxes in one class and in two, class ids below 0 and from 64
    up, bit-equal scores, zero-volume and NaN-corner boxes (a NaN IoU removes across classes: ref_tail.aligned_3d_nms states the rule)."""
    print(f'gpu aligned 3-D nms: smallest decision margin = {T.run_aligned(be):.3e}')


def test_indoor_tail_vs_fp64(be):
    """ivx_indoor_tail_get_bboxes, B = 2, 1 / 3 / 4 levels with unequal k: ScanNet with a best score equal to score_thr, all candidates below
    it, max_num below the picks, a label tie; SUN RGB-D with 1, 2, 3, 10 classes."""
    worst, margin = T.run_indoor(be)
    print(f'gpu indoor tails: worst error / bound = {worst:.3f}; smallest decision margin = {margin:.3e}')
