"""Measure pixel maps (ivx_backproject_mapped_fwd, add_views(..., pixel_weights=, depths=)) on the GPU box.  python tools/scene_maps_bench.py [--md profiles/scene_maps.md]

Method of tools/scene_weighted_bench.py: HIP events around 20 back-to-back launches, two forms alternating in one process, median (min .. max) of
--kreps batches, the bit-equality column checked in the same run.
  (a) kernel      one view into each of N = 4, 8 rows of a state pool, fp32: ops.backproject_mapped_accum_ against ops.backproject_weighted_accum_ on the
                  same lists, both emitting the mean.  Two sets of maps: NEUTRAL (a weight map of ones, a depth map of zeros = no measurement, gate
                  (0.1, 0.3)): the two dependent loads on the projecting lane and nothing else -- the states must be bit-equal to the weighted form's;
                  and GENERAL (confidences in [0.5, 1.5), depths in [0.5, 4) m with one pixel in ten a hole, gate (0.1, 0.3)): what a caller runs; the
                  gate then drops most (view, voxel) pairs and their feature loads with them.  scannet_v1 (204 800 voxels x 64) and scannet_fast
                  (25 600 x 256) geometry, 120 x 160 maps of random features.
  (b) per arrival add_views(1 view) + detect() on a session opened with decay=0.9, depth_gate=(0.1, 0.3) that is given both maps at feature resolution
                  against the same session without maps, arrivals 1 .. --views, host clock around calls that end in the detections' device-to-host
                  copy; one warm pass, then the median over --passes passes.
Not part of bench.py.  Needs a device: there is no fallback.  A figure that could not be taken is written as "not measured"."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from scene_window_bench import BATCH, build, fmt, host_ms, kernel_pair_us      # noqa: E402

GATE = (0.1, 0.3)

# What the committed profile's figures say; rewrite it when a new run says something else.
READING = ('Reading (run of the committed profile).  With neutral maps the mapped form takes 1.02 - 1.09 times the weighted form\'s time (+3 to +16 us per launch), more than the 0.2 - 0.8 % its bytes allow: the two map loads sit on the projecting lane between the projection and the broadcast of the pixel offset, one more dependent memory round trip per projection round, as the weight load was before it was moved beside the projection rows (profiles/scene_weighted.md).  With general maps and a 0.4 m gate only 14 % of the (view, voxel) pairs count, their feature loads fall away, and the launch takes 0.91 - 1.01 times the weighted one.  Per arrival the maps cost nothing measurable at ScanNet v1 (0.997); at ScanNet fast the session with maps is 0.3 ms slower (1.08), far more than the lift\'s few us: the two sessions hold different volumes and return different numbers of detections, and the tail\'s time depends on them; which part of the 0.3 ms is the host side of the map arguments has NOT been separated, and no counter run was made.')

# From `hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -Rpass-analysis=kernel-resource-usage` on csrc/backproject.hip (a compile, not a run):
# backproject_mean_kernel<4, MODE, T, SAMP, true, true, true, MAPPED>
RESOURCES = '''| instantiation (VEC 4, weighted) | VGPRs | SGPRs | scratch B/lane | LDS B | waves/SIMD |
|---|---|---|---|---|---|
| accumulate fp32 nearest | 60 | 64 | 0 | 0 | 8 |
| accumulate fp32 nearest, mapped | 62 | 76 | 0 | 0 | 8 |
| accumulate bf16 nearest | 60 | 64 | 0 | 0 | 8 |
| accumulate bf16 nearest, mapped | 62 | 76 | 0 | 0 | 8 |
| accumulate fp32 bilinear | 78 | 67 | 0 | 0 | 6 |
| accumulate fp32 bilinear, mapped | 78 | 79 | 0 | 0 | 6 |
| accumulate bf16 bilinear | 80 | 67 | 0 | 0 | 6 |
| accumulate bf16 bilinear, mapped | 80 | 79 | 0 | 0 | 6 |
| mean fp32 nearest | 60 | 54 | 0 | 0 | 8 |
| mean fp32 nearest, mapped | 58 | 66 | 0 | 0 | 8 |
| mean bf16 nearest | 60 | 54 | 0 | 0 | 8 |
| mean bf16 nearest, mapped | 58 | 66 | 0 | 0 | 8 |
| mean fp32 bilinear | 78 | 57 | 0 | 0 | 6 |
| mean fp32 bilinear, mapped | 78 | 69 | 0 | 0 | 6 |
| mean bf16 bilinear | 80 | 57 | 0 | 0 | 6 |
| mean bf16 bilinear, mapped | 80 | 69 | 0 | 0 | 6 |

No scratch and no LDS in any of them.  A mapped form carries at most 2 more VGPRs than its weighted form and 12 more SGPRs (the two map pointers, the
gate) and keeps its occupancy (waves/SIMD = floor(512 / VGPRs rounded up to 8), at most 8).  The instruction streams of the 36 lift kernels that
existed before are unchanged by the new template parameter (compared line by line in the compiler's assembly output, labels and symbol names
aside).'''


def lift_triple(ia, name, N, kreps):
    """(us weighted, us mapped with neutral maps, us weighted again, us mapped with general maps, neutral states bit-equal, share of pairs the general
    maps keep) for one view into each of N rows, fp32."""
    from imvoxelnet_amd import ops
    from imvoxelnet_amd.workloads import indoor_meta
    model = build(ia, name)
    meta = indoor_meta(N, box_type=ia.DepthInstance3DBoxes)
    meta = dict(meta, img_shape=(480, 640, 3), ori_shape=(480, 640, 3), pad_shape=(480, 640, 3))
    proj, no, crop = model._camera_setup([meta], 4, torch.device('cuda'))
    Cn = {'scannet_v1': 64, 'scannet_fast': 256}[name]
    X, Y, Z = model.n_voxels
    g = torch.Generator().manual_seed(21)
    pool = torch.randn(N, 1, 120, 160, Cn, generator=g).cuda()
    ppool, no, crop = proj[0].contiguous(), no.repeat(N, 1).contiguous(), crop.repeat(N, 1).contiguous()
    lists, rows, first = [[i] for i in range(N)], list(range(N)), [False] * N
    mk = lambda: dict(sum=torch.zeros((N, X, Y, Z, Cn), device='cuda'), wsum=torch.zeros((N, X, Y, Z), device='cuda'),          # noqa: E731
                      count=torch.zeros((N, X, Y, Z), device='cuda', dtype=torch.int32), mean=torch.empty((N, X, Y, Z, Cn), device='cuda'),
                      valid=torch.empty((N, X, Y, Z), device='cuda', dtype=torch.uint8))
    ones, decay = torch.ones(N, device='cuda'), [1.0] * N
    neutral = dict(pixel_weight=torch.ones(N, 120, 160, device='cuda'), depth=torch.zeros(N, 120, 160, device='cuda'), gate=GATE)
    depth = 0.5 + 3.5 * torch.rand(N, 120, 160, generator=g)
    depth[torch.rand(N, 120, 160, generator=g) < 0.1] = 0.0
    general = dict(pixel_weight=(0.5 + torch.rand(N, 120, 160, generator=g)).cuda(), depth=depth.cuda(), gate=GATE)

    def weighted(st):
        return lambda: ops.backproject_weighted_accum_(pool, ppool, lists, ones, rows, first, decay, no, crop, model.voxel_size, st['sum'], st['wsum'], st['count'],
                                                       st['mean'], st['valid'])

    def mapped(st, maps):
        return lambda: ops.backproject_mapped_accum_(pool, ppool, lists, ones, rows, first, decay, no, crop, model.voxel_size, st['sum'], st['wsum'], st['count'],
                                                     st['mean'], st['valid'], **maps)

    a, b = mk(), mk()
    tn, tw = kernel_pair_us(mapped(a, neutral), weighted(b), kreps)
    torch.cuda.synchronize()               # both forms have made the same calls: the states must be equal now
    equal = all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in b) and int(a['count'].max()) > 0
    c, d = mk(), mk()
    tg, tw2 = kernel_pair_us(mapped(c, general), weighted(d), kreps)
    torch.cuda.synchronize()
    kept = float(c['count'].sum()) / max(1.0, float(d['count'].sum()))
    return tw, tn, tw2, tg, bool(equal), kept, X * Y * Z, Cn


def arrivals(ia, name, a):
    from imvoxelnet_amd.workloads import indoor_meta
    model = build(ia, name)
    model.prepare(torch.device('cuda'))
    n = a.views
    meta = indoor_meta(n, box_type=ia.DepthInstance3DBoxes)
    E = meta['lidar2img']['extrinsic']
    scene_meta = dict(meta, lidar2img={k: v for k, v in meta['lidar2img'].items() if k != 'extrinsic'})
    g = torch.Generator().manual_seed(13)
    img = torch.randn(n, 3, 480, 640, generator=g).cuda()
    pw = (0.5 + torch.rand(n, 120, 160, generator=g)).cuda()
    dp = 0.5 + 3.5 * torch.rand(n, 120, 160, generator=g)
    dp[torch.rand(n, 120, 160, generator=g) < 0.1] = 0.0
    dp = dp.cuda()
    bare, maps = (model.open_scene(scene_meta, decay=0.9, depth_gate=GATE) for _ in range(2))
    tb, tm, n_det = [], [], [0, 0]
    for p in range(a.passes + 1):                                 # pass 0 warms every shape up
        bare.reset()
        maps.reset()
        for k in range(n):
            for i, (s, ts, kw) in enumerate(((bare, tb, {}), (maps, tm, dict(pixel_weights=pw[k:k + 1], depths=dp[k:k + 1])))):
                out = []
                t = host_ms(lambda: out.append(s.add_views(img[k:k + 1], E[k:k + 1], **kw).detect()))
                if p:
                    ts.append(t)
                n_det[i] = len(out[0][0]['scores_3d'])
    bare.close()
    maps.close()
    return tb, tm, n_det


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
        raise SystemExit('scene_maps_bench needs a HIP device: nothing is measured without one')
    import imvoxelnet_amd as ia
    names = a.workloads.split(',')
    lines = ['# Pixel maps: the mapped lift against the weighted lift, and one arrival with and without maps', '',
             f'Device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}.  Random maps and features.  Written by tools/scene_maps_bench.py.', '',
             '## (a) One view into each of N rows, fp32: mapped accumulate against the weighted accumulate on the same lists', '',
             f'us per launch; HIP events around {BATCH} back-to-back launches, the two forms alternating in one process; median (min .. max) of {a.kreps} batches each.  '
             'A figure holds the kernel, the gap to the next dispatch and the host side of the op.  Neutral maps (ones, no measurement) compute the weighted '
             f'form\'s bits, so that pair differs by the two map loads on the projecting lane alone; general maps (gate {GATE}) also drop the pairs outside the gate '
             'and their feature loads.  Each mapped column stands beside the weighted figure taken in the same alternation.', '',
             '| workload | voxels x C | N | weighted | mapped, neutral maps | neutral / weighted | derived from bytes | states bit-equal | weighted (2nd run) | mapped, general maps '
             '| general / weighted | pairs the general maps keep |',
             '|---|---|---|---|---|---|---|---|---|---|---|---|']
    for name in names:
        for N in (4, 8):
            try:
                tw, tn, tw2, tg, equal, kept, nvox, Cn = lift_triple(ia, name, N, a.kreps)
            except torch.cuda.OutOfMemoryError as exc:
                print(f'{name} N={N}: {exc}', flush=True)
                lines.append(f'| {name} | | {N} | not measured (out of device memory) | not measured | | | | not measured | not measured | | |')
                continue
            torch.cuda.empty_cache()
            # per voxel the weighted form moves sums in and out (8 C), the mean (4 C), count and wsum in and out + valid (17) and the sampled pixel (4 C);
            # the maps add at most 8 bytes per (view, voxel) pair, less where neighbouring voxels share a pixel
            derived = 1 + 8 / (Cn * 16 + 17)
            med = statistics.median
            lines.append(f'| {name} | {nvox} x {Cn} | {N} | {fmt(tw, 1)} | {fmt(tn, 1)} | {med(tn) / med(tw):.3f} | <= {derived:.3f} | {equal} | {fmt(tw2, 1)} | {fmt(tg, 1)} | '
                         f'{med(tg) / med(tw2):.3f} | {kept:.2f} |')
    lines += ['', 'The "derived from bytes" column is derived, not measured: the maps add 8 bytes per (view, voxel) pair at most, against the 16 C + 17 bytes per voxel '
              'of sums, mean, counts, mask and the sampled pixel.  What the neutral column measures beyond that is latency: the projecting lane waits for its '
              'two map loads, which depend on the projection, before it can broadcast the pixel offset.', '', READING, '',
              f'## (b) One arrival + detect(): a decay=0.9 session given both maps against the same session without maps (arrivals 1 .. {a.views}, fp32 storage)', '',
              'ms, host clock around add_views(1 view) + detect(), which ends in the detections\' device-to-host copy; the two sessions alternate arrival by arrival in one '
              f'process; one warm pass, then median (min .. max) over {a.passes} passes.  The maps are device tensors at feature resolution.', '',
              '| workload | without maps | with both maps | with / without | detections at the last arrival (without, with) |', '|---|---|---|---|---|']
    for name in names:
        if a.skip_arrivals:
            lines.append(f'| {name} | not measured | not measured | | |')
            continue
        try:
            tb, tm, n_det = arrivals(ia, name, a)
            lines.append(f'| {name} | {fmt(tb)} | {fmt(tm)} | {statistics.median(tm) / statistics.median(tb):.3f} | {n_det[0]}, {n_det[1]} |')
        except torch.cuda.OutOfMemoryError as exc:
            print(f'{name}: {exc}', flush=True)
            lines.append(f'| {name} | not measured (out of device memory) | not measured | | |')
        torch.cuda.empty_cache()
    lines += ['', 'Both sessions run the same trunk call, neck and head per arrival and the same op-level checks; they differ in the lift\'s instantiation, the two maps '
              'it reads and the map checks of add_views.  The volumes differ (the maps drop pixels and gate views), so the detections need not be the same.', '',
              '## Kernel resources (compile-time, gfx950)', '', RESOURCES]
    print('\n'.join(lines), flush=True)
    if a.md:
        with open(a.md, 'w') as fo:
            fo.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
