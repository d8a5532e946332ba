"""Measure merging scenes (ivx_volume_merge_fwd, SceneSession.merge) on the GPU box.  python tools/scene_merge_bench.py [--md profiles/scene_merge.md]

Method of tools/scene_warp_bench.py: HIP events around 20 back-to-back calls, the forms alternating in one process, median (min .. max) of --kreps
batches.  Three grids, one row of fp32 state each (sums, weight sum, count): scannet_fast 40 x 40 x 16, C = 256; scannet_v1 80 x 80 x 32, C = 64;
kitti 216 x 248 x 12, C = 64.  The motion is the warp bench's: 2 degrees of yaw, 0.5 degrees of pitch and a translation of (1.3, 0.4, 0.1) voxels;
the source state has a fifth of its voxels unseen and the source grid's origin differs by one voxel along x, as after a scroll.
  (a) entry        ivx_volume_merge_fwd alone: the bare C call through ctypes, no argument checks of the op around it.
  (b) composition  what the parent commit offers for the same job: ops.volume_warp of the source row into a scratch row, then three torch adds
                   (sums and weight sum with alpha, count) into the destination.  It writes and re-reads a whole row, rewrites every voxel, has no
                   forget rule and cannot read a source whose origin differs -- so it is timed with the destination's origin; the bytes are the same.
  (c) floor        a device add_ over the same bytes (two rows read, one written): dst.add_(src, alpha=) for sums and weight sum, dst.add_(src) for count.
  (d) op           the same merge through ops.volume_merge_ (the checks of the op and the ctypes marshalling on top of (a)).
  (e) per arrival  add_views(1 view) + merge(other) + detect() against add_views + detect() on a second fading session (decay=0.9); `other` is a
                   session of two views; host clock around calls that end in the detections' device-to-host copy; one warm pass, then the median
                   over --passes.  The merging session is reset every --views arrivals, like the other.
The destination accumulates over the repetitions (sums grow, nothing overflows in fp32 at these counts; the count saturates by definition), which
changes no address and no branch: which voxels are merged depends on the source alone.
  --only-kernel N runs N op calls per grid and nothing else: the body of a counter run of its own (rocprofv3 --pmc ... -- python
  tools/scene_merge_bench.py --only-kernel 3).
The tool writes tables and no interpretation: profiles/scene_merge.md ends in a '## Reading' written by hand, which --md keeps and marks as older.
Not part of bench.py.  Needs a device: there is no fallback.  A figure that could not be taken is written as "not measured"."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from scene_window_bench import BATCH, build, fmt, host_ms      # noqa: E402
from scene_scroll_bench import many_us                        # noqa: E402
from scene_warp_bench import GRIDS, motion, state             # noqa: E402

ALPHA = 0.5

# From `hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -Rpass-analysis=kernel-resource-usage` on csrc/volume_warp.hip (a compile, not a run)
RESOURCES = '''| kernel | VGPRs | SGPRs | scratch B/lane | LDS B | waves/SIMD |
|---|---|---|---|---|---|
| volume_warp_kernel at the parent commit (0.5.4, not a template) | 58 | 48 | 0 | 0 | 8 |
| volume_warp_kernel<false>, the warp instantiation | 58 | 48 | 0 | 0 | 8 |
| volume_warp_kernel<true>, the merge instantiation | 62 | 50 | 0 | 0 | 8 |

Kernel arguments: 96 bytes of pools, grid and threshold plus 32 samples of 21 words (rows, M, the two origins, alpha) = 2784 bytes, under the 4 KB
limit, so both instantiations carry 32 samples per launch.'''


KEPT = 'The reading below was written by hand for the tables of an earlier run and is kept as it was: check it against the tables above.'


def c_merge():
    """ivx_volume_merge_fwd of the product build through ctypes, with no checks of the op around it."""
    from imvoxelnet_amd import _lib
    fn = _lib.lib().ivx_volume_merge_fwd

    def merge(dst, src, T, od, os_, vs):
        X, Y, Z, Cn = dst[0].shape[1:]
        f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])     # noqa: E731
        rc = fn(1, (C.c_int32 * 1)(0), (C.c_int32 * 1)(0), (C.c_float * 12)(*T[:3].reshape(-1).tolist()), f3(od), f3(os_), (C.c_float * 1)(ALPHA), f3(vs), 0.0,
                1, 1, X, Y, Z, Cn, *[t.data_ptr() for t in src], *[t.data_ptr() for t in dst], C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
    return merge


def kernel_rows(name, kreps, only=0):
    from imvoxelnet_amd import ops
    dims, Cn, vs = GRIDS[name]
    od = (-np.asarray(dims) / 2 * np.asarray(vs)).astype(np.float32)
    os_ = od + np.asarray([vs[0], 0, 0], np.float32)
    T = motion(dims, vs)
    src, dst = state(dims, Cn, 7), state(dims, Cn, 8)
    gone = torch.rand(src[1].shape, generator=torch.Generator().manual_seed(9)).cuda() < 0.2
    for t in src:
        t[gone] = 0
    op = lambda: ops.volume_merge_(*dst, [0], src, [0], [T], od, os_, vs, alpha=ALPHA)      # noqa: E731
    if only:
        for _ in range(only):
            op()
        torch.cuda.synchronize()
        return []
    row_bytes = sum(t.numel() * 4 for t in src)
    scratch = [torch.empty_like(t) for t in src]
    bare = c_merge()

    def composition():
        ops.volume_warp(*src, [0], [T], od[None], vs, out=scratch)
        dst[0].add_(scratch[0], alpha=ALPHA)
        dst[1].add_(scratch[1], alpha=ALPHA)
        dst[2].add_(scratch[2])

    def floor():
        dst[0].add_(src[0], alpha=ALPHA)
        dst[1].add_(src[1], alpha=ALPHA)
        dst[2].add_(src[2])

    ta, tb, tc, td = many_us([lambda: bare(dst, src, T, od, os_, vs), composition, floor, op], kreps)
    torch.cuda.synchronize()
    med = statistics.median
    gbs = lambda t: 3 * row_bytes / (med(t) * 1e-6) / 1e9      # noqa: E731
    for t in scratch:                                             # the share of voxels the merge writes: what it leaves in an all-zero row
        t.zero_()
    merged = float((ops.volume_merge_(*scratch, [0], src, [0], [T], od, os_, vs, alpha=ALPHA)[1] > 0).float().mean())
    return [f'| {name} | {"x".join(map(str, dims))} x {Cn} | {row_bytes / 1e6:.1f} | {fmt(ta, 1)} | {gbs(ta):.0f} | {fmt(tb, 1)} | {fmt(tc, 1)} | {gbs(tc):.0f} | {fmt(td, 1)} | '
            f'{med(ta) / med(tc):.2f} | {med(ta) / med(tb):.2f} | {merged:.2f} |']


def arrivals(ia, name, a):
    from imvoxelnet_amd.workloads import indoor_meta
    model = build(ia, name)
    model.prepare(torch.device('cuda'))
    n = a.views
    meta = indoor_meta(n, box_type=ia.DepthInstance3DBoxes)
    E = meta['lidar2img']['extrinsic']
    scene_meta = dict(meta, lidar2img={k: v for k, v in meta['lidar2img'].items() if k != 'extrinsic'})
    img = torch.randn(n, 3, 480, 640, generator=torch.Generator().manual_seed(13)).cuda()
    alone, merging, other = (model.open_scene(scene_meta, decay=0.9) for _ in range(3))
    other.add_views(img[:2], E[:2])
    T = motion(model.n_voxels, model.voxel_size)
    ts, tm = [], []
    for p in range(a.passes + 1):                                 # pass 0 warms every shape up
        alone.reset()
        merging.reset()
        for k in range(n):
            t = host_ms(lambda: alone.add_views(img[k:k + 1], E[k:k + 1]).detect())
            u = host_ms(lambda: merging.add_views(img[k:k + 1], E[k:k + 1]).merge(other, T, ALPHA).detect())
            if p:
                ts.append(t)
                tm.append(u)
    for s in (alone, merging, other):
        s.close()
    return ts, tm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    ap.add_argument('--kreps', type=int, default=20)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--views', type=int, default=8)
    ap.add_argument('--grids', default='scannet_fast,scannet_v1,kitti')
    ap.add_argument('--workloads', default='scannet_fast,scannet_v1')
    ap.add_argument('--skip-arrivals', action='store_true')
    ap.add_argument('--only-kernel', type=int, default=0, help='run this many op calls per grid and nothing else (the body of a counter run)')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('scene_merge_bench needs a HIP device: nothing is measured without one')
    import imvoxelnet_amd as ia
    grids = a.grids.split(',')
    if a.only_kernel:
        for name in grids:
            kernel_rows(name, 0, a.only_kernel)
        return
    lines = ['# Merging scenes: the rigid in-place merge of the state against warp-into-scratch plus adds and against a device add_', '',
             f'Device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}.  Written by tools/scene_merge_bench.py.', '',
             f'## (a) - (d) One row of fp32 state merged into another under 2 degrees of yaw, 0.5 of pitch and (1.3, 0.4, 0.1) voxels, alpha = {ALPHA}', '',
             f'us per call; HIP events around {BATCH} back-to-back calls, the four forms alternating in one process; median (min .. max) of {a.kreps} batches each.  A figure '
             'holds the kernels of the call, the gaps between them and the host side of the call.  (a) is the bare C entry, (d) the same through ops.volume_merge_; '
             '(b) is the composition of the parent commit (ops.volume_warp into a scratch row, then three torch adds); (c), a device add_ of the three fields, is '
             'the floor: two rows read, one written.  GB/s counts those three rows for (a) and (c) alike.  Rows of 26 / 54 / 168 MB fit the 256 MB Infinity Cache, so '
             'rates above the HBM bandwidth are cache rates, for every form alike.  `merged` is the share of the destination voxels the merge writes.', '',
             '| grid | voxels x C | state MB | (a) entry us | GB/s | (b) warp + adds us | (c) add_ us | GB/s | (d) ops.volume_merge_ us | (a) / (c) | (a) / (b) | merged |',
             '|---|---|---|---|---|---|---|---|---|---|---|---|']
    for name in grids:
        lines += kernel_rows(name, a.kreps)
        torch.cuda.empty_cache()
    lines += ['', 'Read as: the merge takes `(a) / (c)` times the floor and `(a) / (b)` times the composition.']
    lines += ['', f'## (e) One arrival + detect() with and without a merge (arrivals 1 .. {a.views}, decay=0.9, fp32 storage, 480 x 640)', '',
              'ms, host clock around add_views(1 view) [+ merge of a two-view session under the motion above] + detect(), which ends in the detections\' device-to-host '
              f'copy; the two sessions alternate arrival by arrival in one process; one warm pass, then median (min .. max) over {a.passes} passes.  The merging session '
              'also recomputes the mean from the merged state (the existing refresh), which the other session gets from its lift.', '',
              '| workload | add_views + detect() | add_views + merge + detect() | difference of the medians |', '|---|---|---|---|']
    for name in a.workloads.split(','):
        if a.skip_arrivals:
            lines.append(f'| {name} | not measured | not measured | |')
            continue
        try:
            ts, tm = arrivals(ia, name, a)
            lines.append(f'| {name} | {fmt(ts)} | {fmt(tm)} | {statistics.median(tm) - statistics.median(ts):+.2f} ms |')
        except torch.cuda.OutOfMemoryError as exc:
            print(f'{name}: {exc}', flush=True)
            lines.append(f'| {name} | not measured (out of device memory) | not measured | |')
        torch.cuda.empty_cache()
    lines += ['', '## Kernel resources (compile-time, gfx950)', '', RESOURCES]
    print('\n'.join(lines), flush=True)
    if a.md:                                   # the tables are this run's; what a reader made of them ('## Reading' and below) is prose, not output:
        tail = ''                              # an existing note keeps it, marked as older than the tables
        if os.path.exists(a.md):
            old = open(a.md).read()
            if '## Reading' in old:
                tail = f'\n{KEPT}\n\n' + old[old.index('## Reading'):]
        with open(a.md, 'w') as fo:
            fo.write('\n'.join(lines) + '\n' + tail)


if __name__ == '__main__':
    main()
