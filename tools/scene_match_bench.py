"""Measure matching scenes (ivx_volume_match_fwd, ops.volume_match, SceneSession.register's search) on the GPU box.
python tools/scene_match_bench.py [--md profiles/scene_match.md]

Method of tools/scene_warp_bench.py: HIP events around 20 back-to-back calls, the forms alternating in one process, median (min .. max) of --kreps
batches.  Three grids, one row of fp32 state each on either side: scannet_fast 40 x 40 x 16, C = 256; scannet_v1 80 x 80 x 32, C = 64; kitti
216 x 248 x 12, C = 64.  The source state has a fifth of its voxels unseen; the destination is the warp of the source under the warp bench's
motion (2 degrees of yaw, 0.5 of pitch, (1.3, 0.4, 0.1) voxels), so that motion is the truth; the candidates are pose_candidates around it
(1 degree, one voxel), the truth first.
  (a) match        ops.volume_match with K = 1, 32 and 81 candidates, step 1: us per call and per candidate (the checks of the op, the scratch
                   allocation and the launches; no read-back).
  (b) step 2       the same with step = 2 (an eighth of the voxels visited).
  (c) composition  what the parent commit offers for ONE candidate: zero a scratch row, ops.volume_merge_ of the source into it, ops.volume_wmean of
                   it, and torch reductions of the products with the destination's mean over the voxels both have seen (the destination's mean is
                   computed once, outside the timed region; no read-back, though a search would need one per candidate to choose).
  (d) register     one search of 6 levels x 81 candidates through the op (scene._register, what SceneSession.register runs), from a start 3 degrees
                   and half a voxel off: ms on the host clock, read-backs included; step 1, and step 2 on the first three levels.
The candidates ride on blockIdx.y, 32 per launch; the other arrangement (a loop over the candidates inside the workgroup) was not built.
The tool writes tables and no interpretation: profiles/scene_match.md ends in a '## Reading' written by hand, which --md keeps and marks as older.
Not part of bench.py.  Needs a device: there is no fallback.  A figure that could not be taken is written as "not measured"."""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from scene_window_bench import BATCH, fmt, host_ms            # noqa: E402
from scene_scroll_bench import many_us                        # noqa: E402
from scene_warp_bench import GRIDS, motion, state             # noqa: E402

# From `hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -Rpass-analysis=kernel-resource-usage` on csrc/volume_match.hip (a compile, not a run)
RESOURCES = '''| kernel | VGPRs | SGPRs | scratch B/lane | LDS B | waves/SIMD |
|---|---|---|---|---|---|
| volume_match_kernel (256 lanes per workgroup) | 86 | 104 | 0 | 128 | 5 |
| volume_match_sum_kernel (64 lanes) | 28 | 30 | 0 | 0 | 8 |

Kernel arguments: 168 bytes of pools, grid, walk and one sample plus 32 candidates of 12 words = 1704 bytes, under the 4 KB limit.'''

KEPT = 'The reading below was written by hand for the tables of an earlier run and is kept as it was: check it against the tables above.'


def setup(name):
    from imvoxelnet_amd import ops, pose_candidates
    dims, Cn, vs = GRIDS[name]
    o = (-np.asarray(dims) / 2 * np.asarray(vs)).astype(np.float32)
    T = motion(dims, vs)
    src = state(dims, Cn, 7)
    gone = torch.rand(src[1].shape, generator=torch.Generator().manual_seed(9)).cuda() < 0.2
    for t in src:
        t[gone] = 0
    dst = [torch.zeros_like(t) for t in src]
    ops.volume_warp(*src, [0], [T], o[None], vs, out=dst)
    cands = pose_candidates(T, math.radians(1.0), vs, (0, 0, 0))
    cands = [cands[40]] + cands[:40] + cands[41:]
    return ops, dims, Cn, vs, o, T, src, dst, cands


def kernel_rows(name, kreps):
    ops, dims, Cn, vs, o, T, src, dst, cands = setup(name)
    row_bytes = sum(t.numel() * 4 for t in src[:2])
    match = lambda K, step: (lambda: ops.volume_match(dst[0], dst[1], [0], src, [0], [cands[:K]], o, o, vs, step))      # noqa: E731
    scratch = [torch.empty_like(t) for t in src]
    a_mean, a_ok = ops.volume_wmean(dst[0], dst[1])

    def composition():
        for t in scratch:
            t.zero_()
        ops.volume_merge_(*scratch, [0], src, [0], [cands[0]], o, o, vs)
        b_mean, b_ok = ops.volume_wmean(scratch[0], scratch[1])
        m = (a_ok & b_ok).to(torch.float32)[..., None]
        bm = b_mean * m
        return (a_mean * bm).sum(), (a_mean * a_mean * m).sum(), (bm * bm).sum(), m.sum()

    ts = many_us([match(1, 1), match(32, 1), match(81, 1), match(1, 2), match(32, 2), match(81, 2), composition], kreps)
    torch.cuda.synchronize()
    med = statistics.median
    pairs, own, stats = ops.volume_match(dst[0], dst[1], [0], src, [0], [cands[:2]], o, o, vs)
    s = stats[0].cpu().numpy()
    ncc = s[:, 0] / np.sqrt(s[:, 1] * s[:, 2])
    c = [float(v) for v in composition()]
    head = f'| {name} | {"x".join(map(str, dims))} x {Cn} | {2 * row_bytes / 1e6:.1f} |'
    a = [f'{head} {fmt(ts[0], 1)} | {fmt(ts[1], 1)} | {med(ts[1]) / 32:.1f} | {fmt(ts[2], 1)} | {med(ts[2]) / 81:.1f} | {fmt(ts[6], 1)} | {med(ts[6]) / (med(ts[2]) / 81):.1f} | '
         f'{med(ts[6]) / med(ts[0]):.2f} |']
    b = [f'{head} {fmt(ts[3], 1)} | {fmt(ts[4], 1)} | {med(ts[4]) / 32:.1f} | {fmt(ts[5], 1)} | {med(ts[5]) / 81:.1f} | {med(ts[2]) / med(ts[5]):.2f} |']
    chk = [f'| {name} | {ncc[0]:.6f} | {ncc[1]:.6f} | {int(pairs[0, 0])} | {int(own[0])} | {c[0] / math.sqrt(c[1] * c[2]):.6f} | {int(c[3])} |']
    return a, b, chk


def register_rows(name, passes):
    from imvoxelnet_amd import MatchResult
    from imvoxelnet_amd.scene import _register
    ops, dims, Cn, vs, o, T, src, dst, cands = setup(name)
    c, s, z = math.cos(math.radians(3)), math.sin(math.radians(3)), np.asarray(vs)
    off = np.array([[c, -s, 0, 0.5 * z[0]], [s, c, 0, -0.5 * z[1]], [0, 0, 1, 0.25 * z[2]], [0, 0, 0, 1]])

    def play(Ts, step):
        pairs, own, stats = ops.volume_match(dst[0], dst[1], [0], src, [0], [Ts], o, o, vs, step)
        return MatchResult(pairs[0].cpu().numpy(), int(own[0]), stats[0].cpu().numpy(), Ts, 0.3)

    out = []
    for steps in (1, [2, 2, 2, 1, 1, 1]):
        run = lambda: _register(play, T @ off, math.radians(8), None, 6, steps, 0.3, np.zeros(3), vs)      # noqa: E731
        run()
        ts = [host_ms(run) for _ in range(passes)]
        Tf, res = run()
        E = np.linalg.inv(T) @ Tf
        out.append(f'{fmt(ts)} | {math.degrees(abs(math.atan2(E[1, 0], E[0, 0]))):.3f} | {(np.abs(E[:3, 3]) / z).max():.3f}')
    return [f'| {name} | {out[0]} | {out[1]} |']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    ap.add_argument('--kreps', type=int, default=10)
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--grids', default='scannet_fast,scannet_v1,kitti')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('scene_match_bench needs a HIP device: nothing is measured without one')
    grids = a.grids.split(',')
    ra, rb, rc, rd = [], [], [], []
    for name in grids:
        x, y, z = kernel_rows(name, a.kreps)
        ra, rb, rc = ra + x, rb + y, rc + z
        torch.cuda.empty_cache()
        rd += register_rows(name, a.passes)
        torch.cuda.empty_cache()
    lines = ['# Matching scenes: scoring candidate poses in one call against merge-into-scratch plus torch reductions per candidate', '',
             f'Device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}.  Written by tools/scene_match_bench.py.', '',
             '## (a), (c) ops.volume_match at K = 1, 32 and 81 candidates, step 1, and the composition of the parent commit for one candidate', '',
             f'us per call; HIP events around {BATCH} back-to-back calls, all forms alternating in one process; median (min .. max) of {a.kreps} batches each.  A figure holds '
             'the kernels of the call, the gaps between them and the host side of the call (the checks of the op and the scratch allocation); no read-back in any form.  '
             'The composition is: zero a scratch row, ops.volume_merge_ into it, ops.volume_wmean of it, torch reductions of the products with the destination\'s mean.  '
             '`state MB` is the two rows (sums and weight sum) a candidate reads at most.', '',
             '| grid | voxels x C | state MB | K = 1 us | K = 32 us | per candidate | K = 81 us | per candidate | composition, one candidate us | composition / per candidate at K = 81 | composition / K = 1 |',
             '|---|---|---|---|---|---|---|---|---|---|---|'] + ra
    lines += ['', '## (b) The same with step = 2 (every second voxel per axis: an eighth of the voxels)', '',
              '| grid | voxels x C | state MB | K = 1 us | K = 32 us | per candidate | K = 81 us | per candidate | step 1 / step 2 at K = 81 |', '|---|---|---|---|---|---|---|---|---|'] + rb
    lines += ['', '## What the two forms computed (a check, not a timing)', '',
              'ncc of the truth and of its first neighbour from ops.volume_match; the truth\'s ncc and pairs from the composition (fp32 torch reductions).', '',
              '| grid | ncc at the truth | ncc at the neighbour | pairs | own | composition: ncc at the truth | pairs |', '|---|---|---|---|---|---|---|'] + rc
    lines += ['', '## (d) One register search: 6 levels x 81 candidates, from 3 degrees and (0.5, -0.5, 0.25) voxels off', '',
              f'ms on the host clock around the whole search, the read-back of every level included; one warm run, then median (min .. max) of {a.passes}.  The error is the '
              'found transform against the truth: yaw in degrees, the largest translation component in voxels.', '',
              '| grid | step 1: ms | yaw error | shift error | step 2 on levels 1 - 3: ms | yaw error | shift error |', '|---|---|---|---|---|---|---|'] + rd
    lines += ['', '## Kernel resources (compile-time, gfx950)', '', RESOURCES]
    print('\n'.join(lines), flush=True)
    if a.md:                                   # the tables are this run's; what a reader made of them ('## Reading' and below) is prose, not output
        tail = ''
        if os.path.exists(a.md):
            old = open(a.md).read()
            if '## Reading' in old:
                tail = f'\n{KEPT}\n\n' + old[old.index('## Reading'):]
        with open(a.md, 'w') as fo:
            fo.write('\n'.join(lines) + '\n' + tail)


if __name__ == '__main__':
    main()
