"""Measure scene batches (SceneBatch, ivx_backproject_lists_fwd) on the GPU box.  python tools/scene_batch_bench.py [--md profiles/scene_batch.md]

Workloads: scannet_fast and scannet_v1 of workloads.py, synthetic 480 x 640 views; N scenes in {1, 4, 8}.
  (a) kernel      ops.backproject_lists_accum_ adding ONE view to each of N rows of the state pools (one launch, one upload of the lists) against N
                  calls of ops.backproject_accum_ at B = 1 (ivx_backproject_accum_fwd) doing the same: same process, alternating, HIP events around
                  10 repetitions enqueued back to back, divided by 10; warm-up, then median (min .. max) of --kreps such batches each.  At N = 1 that
                  is the listed accumulate against the plain one.  The two results are compared with torch.equal (from a zeroed state, first = 1).
  (b) per tick    one arrival on each of N scenes + detect() of all on a SceneBatch, against N SceneSessions doing add_views(1 view) + detect() one
                  after the other (what a caller has without batches), alternating tick by tick in the same process; unbounded and window = W.  Host
                  clock around calls that end in the device-to-host copy of the detections; W + 2 warm ticks (the windows are full afterwards), then
                  the median over --ticks ticks.
Not part of bench.py.  Needs a device: there is no fallback.  A figure that could not be taken is written as "not measured"."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from scene_window_bench import build, fmt, host_ms      # noqa: E402  (the same models and clocks as the window measurement)

BATCH = 10      # repetitions between one pair of events

# From `hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -Rpass-analysis=kernel-resource-usage` on csrc/backproject.hip (a compile, not a run):
# backproject_mean_kernel<4, MODE, T, SAMP, GATHER, ROWS>
RESOURCES = '''| instantiation (VEC 4) | VGPRs | SGPRs | scratch B/lane | LDS B | waves/SIMD |
|---|---|---|---|---|---|
| accumulate fp32 nearest | 58 | 58 | 0 | 0 | 8 |
| accumulate fp32 nearest, listed rows | 56 | 58 | 0 | 0 | 8 |
| accumulate bf16 nearest | 58 | 58 | 0 | 0 | 8 |
| accumulate bf16 nearest, listed rows | 56 | 58 | 0 | 0 | 8 |
| accumulate fp32 bilinear | 74 | 58 | 0 | 0 | 6 |
| accumulate fp32 bilinear, listed rows | 74 | 61 | 0 | 0 | 6 |
| accumulate bf16 bilinear | 76 | 58 | 0 | 0 | 6 |
| accumulate bf16 bilinear, listed rows | 76 | 61 | 0 | 0 | 6 |
| mean fp32 nearest: plain / gathered | 56 / 56 | 50 / 50 | 0 | 0 | 8 |
| mean fp32 nearest, listed rows | 56 | 51 | 0 | 0 | 8 |
| mean bf16 nearest: plain / gathered | 56 / 56 | 50 / 50 | 0 | 0 | 8 |
| mean bf16 nearest, listed rows | 56 | 51 | 0 | 0 | 8 |
| mean fp32 bilinear: plain / gathered | 74 / 74 | 50 / 53 | 0 | 0 | 6 |
| mean fp32 bilinear, listed rows | 74 | 53 | 0 | 0 | 6 |
| mean bf16 bilinear: plain / gathered | 76 / 76 | 50 / 53 | 0 | 0 | 6 |
| mean bf16 bilinear, listed rows | 76 | 53 | 0 | 0 | 6 |

No scratch and no LDS in any of the eight new instantiations; each keeps the occupancy of its plain form and is within 2 VGPRs and 3 SGPRs of it
(the row, the pool size and the two list pointers).  The instruction streams of the twenty kernels that existed before (sixteen of the lift
template, the two single-view kernels, the two normalisers) are unchanged by the new template parameter: the compiler's assembly of
csrc/backproject.hip at the parent commit and at this one was compared kernel by kernel, instruction by instruction (12 090 instructions, all
equal; only the mangled names carry the extra template argument).'''


def kernel_pair_us(fa, fb, reps, warmup=3):
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ts = ([], [])
    for _ in range(reps):
        for t, fn in zip(ts, (fa, fb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(BATCH):
                fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) * 1e3 / BATCH)
    return ts


def _state(N, nv, C, dtype, dev):
    X, Y, Z = nv
    return dict(sum=torch.zeros((N, X, Y, Z, C), device=dev), count=torch.zeros((N, X, Y, Z), device=dev, dtype=torch.int32),
                mean=torch.zeros((N, X, Y, Z, C), device=dev, dtype=dtype), valid=torch.zeros((N, X, Y, Z), device=dev, dtype=torch.uint8))


def measure_kernel(model, meta, img, N, kreps):
    """One view into each of N rows: the listed launch against N plain B = 1 launches."""
    from imvoxelnet_amd import ops
    dev = img.device
    E = meta['lidar2img']['extrinsic']
    p0 = model.features_2d_cl(img[:N][None].contiguous())                        # [N,1,FH,FW,C]
    cams = [model._camera_setup([dict(meta, lidar2img=dict(meta['lidar2img'], extrinsic=[E[i]]))], 4, dev) for i in range(N)]
    proj = torch.cat([c[0][0] for c in cams]).contiguous()                       # [N,3,4]
    origin, crop = torch.cat([c[1] for c in cams]).contiguous(), torch.cat([c[2] for c in cams]).contiguous()
    a, b = _state(N, model.n_voxels, p0.shape[-1], p0.dtype, dev), _state(N, model.n_voxels, p0.shape[-1], p0.dtype, dev)
    sampling = getattr(model, 'sampling', 'nearest')
    lists, rows = [[i] for i in range(N)], list(range(N))
    one = [(p0[i:i + 1], proj[i:i + 1][None].contiguous(), origin[i:i + 1], crop[i:i + 1]) for i in range(N)]

    def listed(first=False):
        ops.backproject_lists_accum_(p0, proj, lists, rows, [first] * N, origin, crop, model.voxel_size, a['sum'], a['count'], a['mean'], a['valid'], sampling=sampling)

    def plain(first=False):
        for i, (f, P, o, c) in enumerate(one):
            ops.backproject_accum_(f, P, o, c, model.voxel_size, b['sum'][i:i + 1], b['count'][i:i + 1], first, b['mean'][i:i + 1], b['valid'][i:i + 1], sampling=sampling)

    listed(True), plain(True)
    listed(), plain()
    equal = all(bool(torch.equal(a[k], b[k])) for k in a)
    tl, tp = kernel_pair_us(listed, plain, kreps)
    return dict(N=N, tl=tl, tp=tp, equal=equal)


def measure_ticks(model, meta, img, N, window, ticks):
    E = meta['lidar2img']['extrinsic']
    scene_meta = dict(meta, lidar2img={k: v for k, v in meta['lidar2img'].items() if k != 'extrinsic'})
    batch = model.open_scenes([scene_meta] * N, window=window)
    sessions = [model.open_scene(scene_meta, window=window) for _ in range(N)]
    n, scene = img.shape[0], list(range(N))
    tb, ts, n_det = [], [], 0
    warm = (window or 0) + 2
    for t in range(warm + ticks):
        vs = [(t * N + s) % n for s in range(N)]
        x = img[torch.tensor(vs, device=img.device)].contiguous()
        Ev = [E[v] for v in vs]
        out = []
        dt_b = host_ms(lambda: out.append(batch.add_views(x, Ev, scene).detect()))

        def sequential():
            for s in range(N):
                out.append(sessions[s].add_views(x[s:s + 1], Ev[s:s + 1]).detect())
        dt_s = host_ms(sequential)
        if t >= warm:
            tb.append(dt_b)
            ts.append(dt_s)
        n_det = sum(len(r['scores_3d']) for r in out[0])
    batch.close()
    for s in sessions:
        s.close()
    return dict(N=N, window=window, tb=tb, ts=ts, n_det=n_det)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    ap.add_argument('--window', type=int, default=20)
    ap.add_argument('--ticks', type=int, default=10)
    ap.add_argument('--kreps', type=int, default=20)
    ap.add_argument('--scenes', default='1,4,8')
    ap.add_argument('--storage', choices=['fp32', 'bf16'], default='fp32')
    ap.add_argument('--workloads', default='scannet_fast,scannet_v1')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('scene_batch_bench needs a HIP device: nothing is measured without one')
    import imvoxelnet_amd as ia
    from imvoxelnet_amd.workloads import indoor_meta
    Ns = [int(v) for v in a.scenes.split(',')]
    res = {}
    for name in a.workloads.split(','):
        model = build(ia, name)
        model.prepare(torch.device('cuda'), dtype=torch.bfloat16 if a.storage == 'bf16' else torch.float32)
        meta = indoor_meta(32, box_type=ia.DepthInstance3DBoxes)
        img = torch.randn(32, 3, 480, 640, generator=torch.Generator().manual_seed(13)).cuda()
        r = dict(kernel=[], ticks=[])
        for N in Ns:
            try:
                r['kernel'].append(measure_kernel(model, meta, img, N, a.kreps))
            except torch.cuda.OutOfMemoryError as exc:
                print(f'{name} kernel N={N}: {exc}', flush=True)
                r['kernel'].append(dict(N=N, failed='out of device memory'))
            for window in (None, a.window):
                try:
                    r['ticks'].append(measure_ticks(model, meta, img, N, window, a.ticks))
                except torch.cuda.OutOfMemoryError as exc:
                    print(f'{name} ticks N={N} window={window}: {exc}', flush=True)
                    r['ticks'].append(dict(N=N, window=window, failed='out of device memory'))
                torch.cuda.empty_cache()
                print(f'{name} N={N} window={window} done', flush=True)
        res[name] = r
        del model, img
        torch.cuda.empty_cache()
    lines = [f'# Scene batches: N streaming scenes per launch, 480 x 640 views ({a.storage} storage)', '',
             f'Device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}.  Random weights.  Written by tools/scene_batch_bench.py.', '',
             '## (a) One view into each of N rows: the listed accumulate against N plain B = 1 accumulates', '',
             f'us per N views; HIP events around {BATCH} back-to-back repetitions, the two forms alternating in one process; median (min .. max) of {a.kreps} batches each.  '
             'A figure holds the kernels, the gaps between dispatches and the host side of the ops (the listed form uploads its three lists in one copy per call).', '',
             '| workload | N | plain: N x ops.backproject_accum_ (B = 1) | listed: 1 x ops.backproject_lists_accum_ | plain / listed | results bit-equal |',
             '|---|---|---|---|---|---|']
    for name, r in res.items():
        for k in r['kernel']:
            if 'failed' in k:
                lines.append(f'| {name} | {k["N"]} | not measured ({k["failed"]}) | not measured | | |')
                continue
            lines.append(f'| {name} | {k["N"]} | {fmt(k["tp"], 1)} | {fmt(k["tl"], 1)} | {statistics.median(k["tp"]) / statistics.median(k["tl"]):.2f} | {k["equal"]} |')
    lines += ['']
    for name, r in res.items():
        k1 = [k for k in r['kernel'] if k['N'] == 1 and 'failed' not in k]
        if k1:
            lines.append(f'{name}: at N = 1 the listed form takes {statistics.median(k1[0]["tl"]) - statistics.median(k1[0]["tp"]):+.1f} us against the plain one (medians; '
                         f'{min(k1[0]["tl"]) - min(k1[0]["tp"]):+.1f} us between the minima).')
    lines += ['', 'Reading: per call the listed op checks three host lists and uploads them in one copy before its launch, which the plain op does not; the kernels differ '
              'by the loads of the row and the first flag.  The difference at N = 1 is that cost once; N plain calls pay their own dispatch N times, which is what the '
              'listed form saves as N grows.  How the difference splits between the host side and the kernel has NOT been measured: no trace was taken.']
    lines += ['', f'## (b) One tick: one arrival on each of N scenes + detect() of all', '',
              f'ms per tick, host clock around calls that end in the detections\' device-to-host copy; W + 2 warm ticks, then median (min .. max) over {a.ticks} ticks, the two '
              'forms alternating tick by tick.  "sessions" is what the parent commit offers: N SceneSessions, each add_views(1 view) + detect(), one after the other.', '',
              '| workload | N | window | N sessions, sequential | SceneBatch | sessions / batch | detections at the last tick (batch) |',
              '|---|---|---|---|---|---|---|']
    for name, r in res.items():
        for k in r['ticks']:
            w = 'none' if k['window'] is None else str(k['window'])
            if 'failed' in k:
                lines.append(f'| {name} | {k["N"]} | {w} | not measured ({k["failed"]}) | not measured | | |')
                continue
            lines.append(f'| {name} | {k["N"]} | {w} | {fmt(k["ts"])} | {fmt(k["tb"])} | {statistics.median(k["ts"]) / statistics.median(k["tb"]):.2f} | {k["n_det"]} |')
    lines += ['', 'The two columns are the same work, not the same bits: the features of a view and the batched neck depend on what shares a call (scene.py, SceneBatch); '
              'every scene\'s volume is the exact lift of the features it was given (tests/test_gpu_scene_batch.py).  Where the ratio is below 1 the batch does not win at '
              'that N; no threshold is set and the feature does not depend on one.  Where the time of a tick goes has NOT been split by stage: no trace was taken.', '',
              '## Kernel resources (compile-time, gfx950)', '', RESOURCES]
    print('\n'.join(lines), flush=True)
    if a.md:
        with open(a.md, 'w') as fo:
            fo.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
