"""Measure aligning scenes (ivx_volume_align_fwd, ops.volume_align, SceneSession.refine's loop) on the GPU box.
python tools/scene_align_bench.py [--md profiles/scene_align.md]

Method of tools/scene_match_bench.py: HIP events around 20 back-to-back calls, the forms alternating in one process, median (min .. max) of --kreps
batches; host-clock figures are one warm run, then median (min .. max) of --passes.  Three grids, one row of fp32 state each on either side:
scannet_fast 40 x 40 x 16, C = 256; scannet_v1 80 x 80 x 32, C = 64; kitti 216 x 248 x 12, C = 64.
  (a) one call     ops.volume_align against ops.volume_match at K = 1, the same pose, the same pools, step 1 and step 2: us per call (the checks of
                   the op, the scratch allocation and the launches; no read-back).  The state is the match bench's: random sums, a fifth of the
                   voxels unseen, the destination the warp of the source under the warp bench's motion; the pose is that motion.  (a') repeats
                   step 1 on the smooth state of (c), where most paired voxels are used.
  (b) read-back    one evaluation as refine runs it -- the op and the read-back of 31 doubles and three counts per pair -- on the host clock, against
                   the op alone followed by a synchronize: the difference is what the read-back costs.
  (c) refine       refine (scene._refine through the op, what SceneSession.refine runs, its defaults) against the six-level register (scene._register,
                   486 candidates) from the same start, 3 degrees of yaw and (0.5, -0.5, 0.25) voxels off, on a SMOOTH state and its warp: every
                   channel a sum of six cosines with wavelengths between six voxels and the grid's extent (a gradient method needs a field with a
                   gradient: on the random state of (a) neighbouring voxels are unrelated and refine's basin is a fraction of a voxel).  ms on the
                   host clock with every read-back, the final pose errors against the truth (rotation angle in degrees, largest translation
                   component in voxels) and the evaluations each spent.
The tool writes tables and no interpretation: profiles/scene_align.md ends in a '## Reading' written by hand, which --md keeps and marks as older.
Not part of bench.py.  Needs a device: there is no fallback."""
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
from scene_warp_bench import GRIDS, motion                    # noqa: E402
from scene_match_bench import setup, KEPT                     # noqa: E402

# From `hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -Rpass-analysis=kernel-resource-usage` on csrc/volume_match.hip (a compile, not a run)
RESOURCES = '''| kernel | VGPRs | AGPRs | SGPRs | scratch B/lane | LDS B | waves/SIMD |
|---|---|---|---|---|---|---|
| volume_match_kernel<false> (the match; 256 lanes per workgroup) | 86 | 0 | 104 | 0 | 128 | 5 |
| volume_match_kernel<true> (the align) | 221 | 0 | 106 | 0 | 1040 | 2 |
| volume_match_sum_kernel<false> (64 lanes) | 28 | 0 | 30 | 0 | 0 | 8 |
| volume_match_sum_kernel<true> | 146 | 0 | 26 | 0 | 0 | 3 |

The match instantiation is what it was before the template (86 VGPRs, 104 SGPRs, no scratch).  The align keeps 31 fp64 accumulators per sums lane
(the direct arrangement, 62 VGPRs), the eight corner words (32) and the Jacobian rows of a word (24 + 4), without scratch.'''


def smooth_pair(name, seed=11):
    """A smooth source row on the device and its warp under the warp bench's motion -> (ops, dims, Cn, vs, o, T, src, dst)."""
    from imvoxelnet_amd import ops
    dims, Cn, vs = GRIDS[name]
    o = (-np.asarray(dims) / 2 * np.asarray(vs)).astype(np.float32)
    T = motion(dims, vs)
    g = torch.Generator().manual_seed(seed)
    idx = torch.stack(torch.meshgrid(*(torch.arange(d, dtype=torch.float32) for d in dims), indexing='ij'), -1).cuda()        # [X,Y,Z,3] in voxels
    mean = torch.zeros(dims + (Cn,), device='cuda')
    for _ in range(6):
        d = torch.randn(Cn, 3, generator=g)
        lam = 6.0 + torch.rand(Cn, generator=g) * (max(dims) - 6.0)                                                            # wavelength in voxels
        k = (d / d.norm(dim=1, keepdim=True) / lam[:, None]).cuda()
        mean += (0.5 + torch.rand(Cn, generator=g)).cuda() * torch.cos(2 * math.pi * (idx @ k.T) + (2 * math.pi * torch.rand(Cn, generator=g)).cuda())
    W = (torch.rand(dims, generator=g) * 3.5 + 0.5).cuda()
    gone = torch.zeros(dims, dtype=torch.bool, device='cuda')
    gone[:max(1, dims[0] // 10)] = True
    S = mean * W[..., None]
    S[gone], W[gone] = 0, 0
    src = [S[None].contiguous(), W[None].contiguous(), torch.ones((1,) + dims, dtype=torch.int32, device='cuda')]
    dst = [torch.zeros_like(t) for t in src]
    ops.volume_warp(*src, [0], [T], o[None], vs, out=dst)
    return ops, dims, Cn, vs, o, T, src, dst


def call_rows(name, kreps, passes):
    from imvoxelnet_amd.scene import _align_host
    ops, dims, Cn, vs, o, T, src, dst, cands = setup(name)
    about = np.zeros(3)
    match = lambda step: (lambda: ops.volume_match(dst[0], dst[1], [0], src, [0], [[T]], o, o, vs, step))                   # noqa: E731
    align = lambda step: (lambda: ops.volume_align(dst[0], dst[1], [0], src, [0], [[T]], about, o, o, vs, step))            # noqa: E731
    ts = many_us([match(1), align(1), match(2), align(2)], kreps)
    torch.cuda.synchronize()
    med = statistics.median
    pairs, used, own, stats = (t.cpu().numpy() for t in align(1)())
    m = [t.cpu().numpy() for t in match(1)()]
    same = np.array_equal(pairs, m[0]) and np.array_equal(own, m[1]) and stats[..., :3].tobytes() == m[2].tobytes()
    head = f'| {name} | {"x".join(map(str, dims))} x {Cn} |'
    a = [f'{head} {fmt(ts[0], 1)} | {fmt(ts[1], 1)} | {med(ts[1]) / med(ts[0]):.2f} | {fmt(ts[2], 1)} | {fmt(ts[3], 1)} | {med(ts[3]) / med(ts[2]):.2f} | '
         f'{int(pairs[0, 0])} | {int(used[0, 0])} | {int(own[0])} | {"yes" if same else "NO"} |']
    run = align(1)
    alone = [host_ms(run) for _ in range(passes + 1)][1:]
    full = [host_ms(lambda: _align_host(run(), 1)) for _ in range(passes + 1)][1:]
    b = [f'{head} {fmt([t * 1e3 for t in alone], 1)} | {fmt([t * 1e3 for t in full], 1)} | {(med(full) - med(alone)) * 1e3:.1f} |']
    return a, b


def refine_rows(name, passes, kreps):
    from imvoxelnet_amd import MatchResult
    from imvoxelnet_amd.scene import _register, _refine, _check_refine, _align_host, ALIGN_DOF
    ops, dims, Cn, vs, o, T, src, dst = smooth_pair(name)
    c, s, z = math.cos(math.radians(3)), math.sin(math.radians(3)), np.asarray(vs)
    off = np.array([[c, -s, 0, 0.5 * z[0]], [s, c, 0, -0.5 * z[1]], [0, 0, 1, 0.25 * z[2]], [0, 0, 0, 1]])
    about = np.zeros(3)

    def play_match(Ts, step):
        pairs, own, stats = ops.volume_match(dst[0], dst[1], [0], src, [0], [Ts], o, o, vs, step)
        return MatchResult(pairs[0].cpu().numpy(), int(own[0]), stats[0].cpu().numpy(), Ts, 0.3)

    def play_align(idx, Ts):
        return _align_host(ops.volume_align(dst[0], dst[1], [0] * len(Ts), src[:2], [0] * len(Ts), [[M] for M in Ts], about, o, o, vs, (1, 1, 1)), len(Ts))

    args = _check_refine(12, ALIGN_DOF, 0.3, 1e-3, None, 1e-5, vs)
    reg = lambda: _register(play_match, T @ off, math.radians(8), None, 6, 1, 0.3, about, vs)                                # noqa: E731
    ref = lambda: _refine(play_align, [T @ off], [about], Cn, *args)[0]                                                      # noqa: E731

    def err(Tf):
        E = np.linalg.inv(T) @ Tf
        return math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(E[:3, :3]) - 1) / 2)))), float((np.abs(E[:3, 3]) / z).max())

    one = many_us([lambda: ops.volume_match(dst[0], dst[1], [0], src, [0], [[T]], o, o, vs), lambda: ops.volume_align(dst[0], dst[1], [0], src, [0], [[T]], about, o, o, vs)], kreps)
    torch.cuda.synchronize()
    pairs, used, own, _ = (t.cpu().numpy() for t in ops.volume_align(dst[0], dst[1], [0], src, [0], [[T]], about, o, o, vs))
    smooth = [f'| {name} | {fmt(one[0], 1)} | {fmt(one[1], 1)} | {statistics.median(one[1]) / statistics.median(one[0]):.2f} | {int(pairs[0, 0])} | {int(used[0, 0])} | {int(own[0])} |']
    reg(), ref()
    t_reg, t_ref = [host_ms(reg) for _ in range(passes)], [host_ms(ref) for _ in range(passes)]
    (T1, r1), (T2, r2) = reg(), ref()
    e1, e2 = err(T1), err(T2)
    return smooth, [f'| {name} | {fmt(t_reg)} | 486 | {e1[0]:.4f} | {e1[1]:.4f} | {fmt(t_ref)} | {r2.evaluations} ({r2.accepted} accepted{", converged" if r2.converged else ""}) | '
            f'{e2[0]:.5f} | {e2[1]:.5f} | {r2.history[0]:.3g} -> {r2.cost:.3g} | {r2.overlap:.2f} | {statistics.median(t_reg) / statistics.median(t_ref):.1f} |']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    ap.add_argument('--kreps', type=int, default=10)
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--grids', default='scannet_fast,scannet_v1,kitti')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('scene_align_bench needs a HIP device: nothing is measured without one')
    ra, rb, rc, rs = [], [], [], []
    for name in a.grids.split(','):
        x, y = call_rows(name, a.kreps, a.passes)
        ra, rb = ra + x, rb + y
        torch.cuda.empty_cache()
        x, y = refine_rows(name, a.passes, a.kreps)
        rs, rc = rs + x, rc + y
        torch.cuda.empty_cache()
    lines = ['# Aligning scenes: the normal equations of a six-DoF pose in one call, and refine against the six-level register', '',
             f'Device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}.  Written by tools/scene_align_bench.py.', '',
             '## (a) One ops.volume_align against one ops.volume_match at K = 1, the same pose and pools', '',
             f'us per call; HIP events around {BATCH} back-to-back calls, the four forms alternating in one process; median (min .. max) of {a.kreps} batches each.  A figure '
             'holds the kernels of the call, the gaps between them and the host side of the call (the checks of the op and the scratch allocation); no read-back.  Random '
             'state, a fifth unseen; the pose is the motion the destination was warped by.  The last column: pairs, own, dot, na, nb of the align equal the match\'s with ==.', '',
             '| grid | voxels x C | match us | align us | align / match | step 2: match us | align us | align / match | pairs | used | own | match parity |',
             '|---|---|---|---|---|---|---|---|---|---|---|---|'] + ra
    lines += ['', '## (a\') The same on the smooth state of (c), where most paired voxels are used', '',
              'The random state of (a) leaves a fifth of the voxels unseen at random, so only 0.8^8 of the paired voxels have eight seen corners and carry the 28 extra sums; '
              'the smooth state loses one slab.  us per call, as in (a), step 1.', '',
              '| grid | match us | align us | align / match | pairs | used | own |', '|---|---|---|---|---|---|---|'] + rs
    lines += ['', '## (b) The read-back of one evaluation (31 doubles and three counts for one pair)', '',
              f'us on the host clock: the op followed by a synchronize, and the op followed by the read-back refine makes; one warm run, then median (min .. max) of {a.passes}.', '',
              '| grid | voxels x C | op and synchronize us | op and read-back us | difference us |', '|---|---|---|---|---|'] + rb
    lines += ['', '## (c) refine against the six-level register, from 3 degrees of yaw and (0.5, -0.5, 0.25) voxels off, on a smooth state and its warp', '',
              f'ms on the host clock around the whole search, every read-back included; one warm run, then median (min .. max) of {a.passes}.  Errors are the found pose '
              'against the truth: the rotation angle in degrees and the largest translation component in voxels.  register: 6 levels x 81 candidates, step 1; refine: its '
              'defaults (12 evaluations at most, all six degrees of freedom, damping 1e-3, tol_shift 1e-3 of a voxel edge, tol_rot 1e-5 rad).', '',
              '| grid | register ms | evaluations | rotation error | shift error | refine ms | evaluations | rotation error | shift error | cost | used / own | register / refine |',
              '|---|---|---|---|---|---|---|---|---|---|---|---|'] + rc
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
