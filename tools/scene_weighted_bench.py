"""Measure fading scenes (ivx_backproject_weighted_fwd, open_scene(meta, decay=...)) on the GPU box.  python tools/scene_weighted_bench.py [--md profiles/scene_weighted.md]

Method of tools/scene_window_bench.py: HIP events around 20 back-to-back launches, the two forms alternating in one process, median (min .. max) of
--kreps batches, the bit-equality column checked in the same run.
  (a) kernel      one view into each of N = 1, 4, 8 rows of a state pool: ops.backproject_weighted_accum_ (unit weights as a device list, decay 1 as a
                  list: what a session opened with decay=1.0 launches) against ops.backproject_lists_accum_ (the unweighted listed kernel, unchanged),
                  both emitting the mean.  scannet_v1 (204 800 voxels x 64) and scannet_fast (25 600 x 256) geometry, 120 x 160 maps of random
                  features, fp32 and bf16.  Both forms make the same calls, so their states must be bit-equal at the end and wsum == count.
  (b) per arrival add_views(1 view) + detect() on a session opened with decay=0.9 against a plain session, arrivals 1 .. --views, host clock around
                  calls that end in the detections' device-to-host copy; one warm pass, then the median over --passes passes.
Not part of bench.py.  Needs a device: there is no fallback.  A figure that could not be taken is written as "not measured"."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from scene_window_bench import BATCH, build, fmt, host_ms, kernel_pair_us      # noqa: E402

# From `hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -S` on csrc/backproject.hip, the kernel descriptors' .vgpr_count / .sgpr_count /
# .private_segment_fixed_size / .group_segment_fixed_size (a compile, not a run): backproject_mean_kernel<4, MODE, T, SAMP, true, true, WEIGHTED>
RESOURCES = '''| instantiation (VEC 4, listed) | VGPRs | SGPRs | scratch B/lane | LDS B | waves/SIMD |
|---|---|---|---|---|---|
| accumulate fp32 nearest | 56 | 58 | 0 | 0 | 8 |
| accumulate fp32 nearest, weighted | 60 | 64 | 0 | 0 | 8 |
| accumulate bf16 nearest | 56 | 58 | 0 | 0 | 8 |
| accumulate bf16 nearest, weighted | 60 | 64 | 0 | 0 | 8 |
| accumulate fp32 bilinear | 74 | 61 | 0 | 0 | 6 |
| accumulate fp32 bilinear, weighted | 78 | 67 | 0 | 0 | 6 |
| accumulate bf16 bilinear | 76 | 61 | 0 | 0 | 6 |
| accumulate bf16 bilinear, weighted | 80 | 67 | 0 | 0 | 6 |
| mean fp32 nearest | 56 | 51 | 0 | 0 | 8 |
| mean fp32 nearest, weighted | 60 | 54 | 0 | 0 | 8 |
| mean bf16 nearest | 56 | 51 | 0 | 0 | 8 |
| mean bf16 nearest, weighted | 60 | 54 | 0 | 0 | 8 |
| mean fp32 bilinear | 74 | 53 | 0 | 0 | 6 |
| mean fp32 bilinear, weighted | 78 | 57 | 0 | 0 | 6 |
| mean bf16 bilinear | 76 | 53 | 0 | 0 | 6 |
| mean bf16 bilinear, weighted | 80 | 57 | 0 | 0 | 6 |

No scratch and no LDS in any of them (the gate).  A weighted form carries 4 more VGPRs than its listed form (the view's weight on the projecting
lane, its broadcast copy, the weight sum) and 3 - 6 more SGPRs (the three pointers, the threshold, the decay), and keeps its occupancy (waves/SIMD =
floor(512 / VGPRs rounded up to 8), at most 8).  volume_wmean_kernel: 19 (fp32) / 21 (bf16) VGPRs, no scratch, no LDS.  The instruction
streams of the 28 kernels that existed before are unchanged by the new template parameter (compared line by line in the compiler's assembly
output, labels and symbol names aside).'''


def lift_pair(ia, name, N, dtype, kreps):
    """(us weighted, us listed, bit-equal) for one view into each of N rows."""
    from imvoxelnet_amd import ops
    from imvoxelnet_amd.workloads import indoor_meta
    model = build(ia, name)
    meta = indoor_meta(N, box_type=ia.DepthInstance3DBoxes)
    meta = dict(meta, img_shape=(480, 640, 3), ori_shape=(480, 640, 3), pad_shape=(480, 640, 3))
    proj, no, crop = model._camera_setup([meta], 4, torch.device('cuda'))
    Cn = {'scannet_v1': 64, 'scannet_fast': 256}[name]
    X, Y, Z = model.n_voxels
    pool = torch.randn(N, 1, 120, 160, Cn, generator=torch.Generator().manual_seed(21)).to(dtype).cuda()
    ppool, no, crop = proj[0].contiguous(), no.repeat(N, 1).contiguous(), crop.repeat(N, 1).contiguous()
    lists, rows, first = [[i] for i in range(N)], list(range(N)), [False] * N
    mk = lambda: dict(sum=torch.zeros((N, X, Y, Z, Cn), device='cuda'), count=torch.zeros((N, X, Y, Z), device='cuda', dtype=torch.int32),          # noqa: E731
                      mean=torch.empty((N, X, Y, Z, Cn), device='cuda', dtype=dtype), valid=torch.empty((N, X, Y, Z), device='cuda', dtype=torch.uint8))
    a, b = mk(), mk()
    a['wsum'] = torch.zeros((N, X, Y, Z), device='cuda')
    ones, decay = torch.ones(N, device='cuda'), [1.0] * N

    def weighted():
        ops.backproject_weighted_accum_(pool, ppool, lists, ones, rows, first, decay, no, crop, model.voxel_size, a['sum'], a['wsum'], a['count'], a['mean'], a['valid'])

    def listed():
        ops.backproject_lists_accum_(pool, ppool, lists, rows, first, no, crop, model.voxel_size, b['sum'], b['count'], b['mean'], b['valid'])

    tw, tl = kernel_pair_us(weighted, listed, kreps)
    torch.cuda.synchronize()               # both forms have made the same calls: the states must be equal now
    equal = all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in b) and torch.equal(a['wsum'], a['count'].float()) and int(a['count'].max()) > 0
    c = mk()
    c['wsum'] = torch.zeros((N, X, Y, Z), device='cuda')

    def bare():                # NULL weights and NULL decay: the weighted kernel without its two extra input loads, with the weight sums
        ops.backproject_weighted_accum_(pool, ppool, lists, None, rows, first, None, no, crop, model.voxel_size, c['sum'], c['wsum'], c['count'], c['mean'], c['valid'])

    tb, _ = kernel_pair_us(bare, listed, kreps)
    torch.cuda.synchronize()
    return tw, tl, bool(equal), X * Y * Z, Cn, tb


def arrivals(ia, name, a):
    from imvoxelnet_amd.workloads import indoor_meta
    model = build(ia, name)
    model.prepare(torch.device('cuda'))
    n = a.views
    meta = indoor_meta(n, box_type=ia.DepthInstance3DBoxes)
    E = meta['lidar2img']['extrinsic']
    scene_meta = dict(meta, lidar2img={k: v for k, v in meta['lidar2img'].items() if k != 'extrinsic'})
    img = torch.randn(n, 3, 480, 640, generator=torch.Generator().manual_seed(13)).cuda()
    plain, fading = model.open_scene(scene_meta), model.open_scene(scene_meta, decay=0.9)
    tp, tf, n_det = [], [], [0, 0]
    for p in range(a.passes + 1):                                 # pass 0 warms every shape up
        plain.reset()
        fading.reset()
        for k in range(n):
            for i, (s, ts) in enumerate(((plain, tp), (fading, tf))):
                out = []
                t = host_ms(lambda: out.append(s.add_views(img[k:k + 1], E[k:k + 1]).detect()))
                if p:
                    ts.append(t)
                n_det[i] = len(out[0][0]['scores_3d'])
    plain.close()
    fading.close()
    return tp, tf, n_det


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    ap.add_argument('--kreps', type=int, default=30)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--views', type=int, default=8)
    ap.add_argument('--workloads', default='scannet_v1,scannet_fast')
    ap.add_argument('--skip-arrivals', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('scene_weighted_bench needs a HIP device: nothing is measured without one')
    import imvoxelnet_amd as ia
    names = a.workloads.split(',')
    lines = ['# Fading scenes: the weighted listed lift against the unweighted one, and one arrival on a fading session', '',
             f'Device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}.  Random weights and features.  Written by tools/scene_weighted_bench.py.', '',
             '## (a) One view into each of N rows: weighted accumulate against the listed accumulate', '',
             f'us per launch; HIP events around {BATCH} back-to-back launches, the two forms alternating in one process; median (min .. max) of {a.kreps} batches each.  '
             'A figure holds the kernel, the gap to the next dispatch and the host side of the op (list checks, the one packed upload), which for the weighted op '
             'also packs the decays.  Unit weights (a device list) and decay 1 (a list), so both forms compute the same bits; both emit the mean.', '',
             '| workload | voxels x C | storage | N | listed (ops.backproject_lists_accum_) | weighted (ops.backproject_weighted_accum_) | weighted / listed | derived from bytes | states bit-equal, wsum == count |',
             '|---|---|---|---|---|---|---|---|---|']
    notes = []
    for name in names:
        for dtype in (torch.float32, torch.bfloat16):
            for N in (1, 4, 8):
                try:
                    tw, tl, equal, nvox, Cn, tb = lift_pair(ia, name, N, dtype, a.kreps)
                except torch.cuda.OutOfMemoryError as exc:
                    print(f'{name} N={N}: {exc}', flush=True)
                    lines.append(f'| {name} | | {str(dtype).split(".")[1]} | {N} | not measured (out of device memory) | not measured | | | |')
                    continue
                torch.cuda.empty_cache()
                esz = 4 if dtype == torch.float32 else 2
                derived = 1 + 8 / (Cn * (8 + esz) + 9)          # per voxel: sums in and out (8 C), the mean (esz C), count in and out + valid (9); weighted: + wsum in and out (8)
                d, spread = statistics.median(tw) - statistics.median(tl), max(tl) - min(tl)
                st = str(dtype).split('.')[1]
                lines.append(f'| {name} | {nvox} x {Cn} | {st} | {N} | {fmt(tl, 1)} | {fmt(tw, 1)} | {statistics.median(tw) / statistics.median(tl):.3f} | {derived:.3f} | {equal} |')
                allowed = (derived - 1) * statistics.median(tl) + spread
                notes.append(f'{name} {st} N={N}: weighted - listed = {d:+.1f} us at the median, {min(tw) - min(tl):+.1f} us between the minima (with NULL weights and NULL '
                             f'decay, measured after it against the same listed calls: {statistics.median(tb):.1f} us); the bytes allow '
                             f'{(derived - 1) * statistics.median(tl):+.1f} us and the listed form alone spreads over {spread:.1f} us (max - min): '
                             + ('within the two.' if d <= allowed else 'BEYOND the two.'))
    lines += [''] + notes
    lines += ['', 'The "derived from bytes" column is derived, not measured: the weighted form moves 8 more bytes per voxel (wsum in and out) beside the sums in and '
              'out, the mean, the counts and the mask.', '',
              'Reading.  The weighted form costs more than its bytes.  Two things were looked at.  (1) The weight of a view used to be loaded and tested BEFORE the '
              'projection rows were loaded, one more dependent memory round trip in front of every projection round; in that form the N = 8 ratios were 1.15 '
              '(scannet_v1 fp32), 1.23 (bf16), 1.17 and 1.17 (scannet_fast).  The kernel now loads the weight beside the projection rows (both addresses need '
              'the slot only) and tests it with the validity; the table above is that kernel.  (2) With NULL weights and NULL decay (no weight load, no decay '
              'load; the figure in the lines above) the time does not move, so what remains is not the two input loads: it comes with the weight sums, which add '
              'one 4-byte load per lane and one 4-byte store per voxel from a single lane of the group -- partial-wave accesses of the kind the count and the '
              'mask already make, whose cost is per memory instruction and per partly written line, not per byte.  At N = 1 the figures of both forms also hold '
              'the host side of the op, which is larger for the weighted one (it packs floats behind the integers of the one upload).  Where the time goes has '
              'NOT been confirmed with counters: no counter run was made.']
    lines += ['', f'## (b) One arrival + detect(): a session opened with decay=0.9 against a plain session (arrivals 1 .. {a.views}, fp32 storage)', '',
              f'ms, host clock around add_views(1 view) + detect(), which ends in the detections\' device-to-host copy; the two sessions alternate arrival by arrival in one '
              f'process; one warm pass, then median (min .. max) over {a.passes} passes.', '',
              '| workload | plain session | decay=0.9 session | fading / plain | detections at the last arrival (plain, fading) |', '|---|---|---|---|---|']
    for name in names:
        if a.skip_arrivals:
            lines.append(f'| {name} | not measured | not measured | | |')
            continue
        try:
            tp, tf, n_det = arrivals(ia, name, a)
            lines.append(f'| {name} | {fmt(tp)} | {fmt(tf)} | {statistics.median(tf) / statistics.median(tp):.3f} | {n_det[0]}, {n_det[1]} |')
        except torch.cuda.OutOfMemoryError as exc:
            print(f'{name}: {exc}', flush=True)
            lines.append(f'| {name} | not measured (out of device memory) | not measured | | |')
        torch.cuda.empty_cache()
    lines += ['', 'Both sessions run the same trunk call, neck and head per arrival; they differ in the lift (a B = 1 accumulate launch against the weighted listed '
              'launch with its packed upload of list, weights and decay) and in the 4 bytes per voxel of the weight sum.  The volumes differ (the fading one '
              'weighs older views less), so the detections need not be the same.', '',
              '## Kernel resources (compile-time, gfx950)', '', RESOURCES]
    print('\n'.join(lines), flush=True)
    if a.md:
        with open(a.md, 'w') as fo:
            fo.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
