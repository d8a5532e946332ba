"""The CPU restatement of the detection tail (oracle/cpu_abi: ivx_boxes_overlap_bev, ivx_nms_bev, ivx_anchor_head_get_bboxes,
ivx_fcos_head_level_candidates, ivx_indoor_tail_get_bboxes, ivx_multiclass_nms_bev, ivx_aligned_3d_nms / _ws) against the plain fp64
references of tests/ref_tail.py, on the cases, with the drivers, the bounds and the decision margins of tests/test_gpu_tail_fp64.py.
No device: this proves the references, the construction of the cases and the bounds before a GPU is involved, and it measures the
per-class error of the C oracle's rotated overlap, which is the bound of that kernel (ref_tail.OVERLAP_MEASURED)."""
import importlib.util
import os

import numpy as np
import pytest

import ref_tail as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def be():
    spec = importlib.util.spec_from_file_location('ivx_cpu_abi_host', os.path.join(ROOT, 'oracle', 'cpu_abi', 'host.py'))
    host = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(host)
    return T.HostBackend(host.load())


# ---------------------------------------------------------------------------------------------------------------- the references themselves
def test_rect_overlap_known_answers():
    """the clipping reference against areas known in closed form"""
    sq = [0, 0, 2, 2, 0.0]
    assert T.rect_overlap(sq, sq) == 4.0
    assert T.rect_overlap(sq, [1, 1, 3, 3, 0.0]) == 1.0
    assert T.rect_overlap(sq, [2, 0, 4, 2, 0.0]) == 0.0 and T.rect_overlap(sq, [2, 2, 4, 4, 0.0]) == 0.0
    assert T.rect_overlap(sq, [10, 10, 11, 11, 0.3]) == 0.0
    # a square turned by 45 degrees about the same centre: the octagon of area 8 (sqrt 2 - 1) s^2 with s = 1 the half side ... = 4 * 2 (sqrt 2 - 1)
    assert abs(T.rect_overlap(sq, [0, 0, 2, 2, np.pi / 4]) - 8 * (np.sqrt(2) - 1)) < 1e-14
    # a 4 x 1 box and its quarter turn share the central 1 x 1 square; any common turn changes nothing
    for t in (0.0, 0.3, -2.0):
        assert abs(T.rect_overlap([-2, -0.5, 2, 0.5, t], [-2, -0.5, 2, 0.5, t + np.pi / 2]) - 1.0) < 1e-14
    # the corner convention: x' = dx cos a + dy sin a, y' = -dx sin a + dy cos a turns the long axis of a 4 x 1 box at angle a towards -a
    a = 0.5
    tip = np.array([1.8 * np.cos(a), -1.8 * np.sin(a)])
    probe = [tip[0] - 0.05, tip[1] - 0.05, tip[0] + 0.05, tip[1] + 0.05, 0.0]
    assert abs(T.rect_overlap([-2, -0.5, 2, 0.5, a], probe) - 0.01) < 1e-14 and T.rect_overlap([-2, -0.5, 2, 0.5, -a], probe) == 0.0
    # symmetric, contained
    r = np.random.RandomState(0)
    A, B = T._rand_boxes(r, 40, 2.0), T._rand_boxes(r, 30, 2.0)
    M = T.overlap_matrix(A, B)
    assert np.abs(M - T.overlap_matrix(B, A).T).max() < 1e-13 and (M > 0.01).sum() > 100
    assert np.all(M <= np.minimum(T.areas(A)[:, None], T.areas(B)[None, :]) + 1e-12)
    assert T.iou_bev(sq, [1, 1, 3, 3, 0.0]) == 1 / 7 and T.iou_axis(sq, [1, 1, 3, 3, 1.0]) == 1 / 7 and T.iou_bev([0, 0, 0, 0, 0], [0, 0, 0, 0, 0]) == 0.0


def test_reference_rules():
    idx, m = T.topk(np.array([0.5, 0.9, 0.5, 0.1, 0.9]), 3)
    assert idx.tolist() == [1, 4, 0] and abs(m - 0.4 / 0.9) < 1e-15
    assert T.topk(np.array([0.5, 0.5]), 5)[0].tolist() == [0, 1]
    v = np.zeros((4, 4, 4), np.uint8)
    v[1:3, 1:3, 1] = 1                       # 4 of the 8 voxels of the one level-2 cell
    assert not T.pooled_valid(v, 2)[0, 0, 0]
    v[1, 1, 2] = 1                           # 5 of 8
    assert T.pooled_valid(v, 2)[0, 0, 0] and T.pooled_valid(v, 1).shape == (2, 2, 2) and T.pooled_valid(v, 1).sum() == 0
    keep, margin = T.greedy_nms(np.array([[0, 0, 2, 2, 0], [0.2, 0, 2.2, 2, 0], [0.4, 0, 2.4, 2, 0]], np.float32), 0.7, False)
    assert keep.tolist() == [0, 2] and abs(margin - abs(1.6 / 2.4 - np.float32(0.7))) < 1e-6       # 1 falls to 0; 2 is decided by 0 alone (0.667)
    # multi-class: class-major when it fits, otherwise by score with ties to the lower class
    boxes = np.array([[0, 0, 1, 1, 0], [5, 5, 6, 6, 0], [9, 9, 10, 10, 0]], np.float32)
    sc = np.array([[0.9, 0.6], [0.6, 0.8], [0.1, 0.6]], np.float32)
    idx, lab, _ = T.multiclass_nms(boxes, sc, 2, 0.3, 0.5, True, 10)
    assert idx.tolist() == [0, 1, 1, 0, 2] and lab.tolist() == [0, 0, 1, 1, 1]
    idx, lab, _ = T.multiclass_nms(boxes, sc, 2, 0.3, 0.5, True, 3)
    assert idx.tolist() == [0, 1, 1] and lab.tolist() == [0, 1, 0]


# ---------------------------------------------------------------------------------------------------------------- rotated overlap
def test_overlap_oracle_measured():
    """Measures the C oracle's rotated overlap against fp64 per configuration class (both argument orders) and prints it; the recorded
    constants of ref_tail.OVERLAP_MEASURED must be what is measured here, rounded up: measured <= constant <= max(2 x measured, 2^-22)."""
    from oracle import c_oracle as co
    bad = []
    for cls in T.OVERLAP_CLASSES:
        worst, pairs = 0.0, 0
        for seed in T.OVERLAP_SEEDS:
            for na, nb in T.OVERLAP_SHAPES:
                e, _, _, (i, _) = T.overlap_measure(co.boxes_overlap_bev, cls, seed, na, nb)
                worst, pairs = max(worst, e), pairs + len(i)
        const = T.OVERLAP_MEASURED.get(cls)
        print(f'overlap class {cls:22s} {pairs} pairs: worst |C oracle - fp64| / min area = {worst:.3e}   recorded {const}')
        if const is None or not (worst <= const <= max(2 * worst, 2.0 ** -22)):
            bad.append((cls, worst, const))
    assert not bad, f'ref_tail.OVERLAP_MEASURED does not match the measurement: {bad}'


@pytest.mark.parametrize('cls', T.OVERLAP_CLASSES)
def test_overlap_cpu(be, cls):
    print(f'cpu overlap {cls}: worst error / (4 x measured bound) = {T.run_overlap(be, cls):.3f}')


# ---------------------------------------------------------------------------------------------------------------- the entry points
@pytest.mark.parametrize('rotated', [0, 1])
def test_nms_bev_cpu(be, rotated):
    print(f'cpu nms rotated={rotated}: smallest decision margin |IoU - thr| of the reference = {T.run_nms(be, bool(rotated)):.3e} (required {T.IOU_MARGIN})')


def test_anchor_head_cpu(be):
    worst, marg = T.run_anchor_head(be)
    print(f'cpu anchor head: worst error / bound = {worst:.3f}; reference margins {marg}')


@pytest.mark.parametrize('grid', T.TOPK_GRIDS)
def test_fcos_topk_cpu(be, grid):
    worst, margin = T.run_fcos_topk(be, grid)
    print(f'cpu fcos top-k grid {grid}: worst error / bound = {worst:.3f}; smallest relative score gap that decides = {margin:.2e}')


def test_fcos_levels_cpu(be):
    worst, margin = T.run_fcos_levels(be)
    print(f'cpu fcos levels: worst error / bound = {worst:.3f}; smallest relative score gap that decides = {margin:.2e}')


def test_multiclass_nms_cpu(be):
    print(f'cpu multi-class nms: smallest decision margin = {T.run_multiclass(be):.3e}')


def test_aligned_3d_nms_cpu(be):
    print(f'cpu aligned 3-D nms: smallest decision margin = {T.run_aligned(be):.3e}')


def test_indoor_tail_cpu(be):
    worst, margin = T.run_indoor(be)
    print(f'cpu indoor tails: worst error / bound = {worst:.3f}; smallest decision margin = {margin:.3e}')
