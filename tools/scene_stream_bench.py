"""Measure streaming scenes (SceneSession, ivx_backproject_accum_fwd) on the GPU box.  python tools/scene_stream_bench.py [--md profiles/scene_stream.md]

Workload: scannet_v1 of workloads.py (ResNet-50 + FPN 64, Atlas neck, 80 x 80 x 32 voxels), 50 synthetic 480 x 640 views arriving one at a time.
  per arrival   for arrival k: add_views(1 view) + detect() -- host clock around the pair, which ends in the device-to-host copy of the detections;
                one whole pass over the 50 arrivals warms every shape up, then --passes timed passes; median over the passes at k = 1, 10, 25, 50
                and the mean over all 50 arrivals;
  one shot      what a caller without sessions runs at arrival k: simple_test over all k views so far (same process, alternating with nothing else:
                warm-up 2, median of --reps calls, same clock);
  kernel        the accumulate launch alone for one new view (HIP events around 20 launches enqueued back to back, divided by 20; warm-up,
                median of --kreps such batches), with and without the mean store;
                bytes from the shapes: N*C*(4 read + 4 written [+ 4 or 2 mean]) + count read and written + mask + the new views' feature maps counted
                once; next to it the one-shot lift of all 50 views (ops.backproject_mean) in the same process.
Not part of bench.py.  Needs a device: there is no fallback."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

ARRIVALS = (1, 10, 25, 50)


BATCH = 20      # launches between one pair of events


def kernel_us(fn, reps, warmup=5):
    """us per launch: BATCH launches enqueued back to back between two events, divided by BATCH, so the host's way to the first launch
    (argument checks, ctypes) is paid once per pair and not per launch; what stays in the figure is the gap between two dispatches."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(BATCH):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / BATCH)
    return statistics.median(ts), min(ts), max(ts)


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def fmt(ts):
    return f'{statistics.median(ts):.2f} ({min(ts):.2f} .. {max(ts):.2f})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    ap.add_argument('--views', type=int, default=50)
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--kreps', type=int, default=50)
    ap.add_argument('--storage', choices=['fp32', 'bf16'], default='fp32')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('scene_stream_bench needs a HIP device: nothing is measured without one')
    import imvoxelnet_amd as ia
    from imvoxelnet_amd import ops
    from imvoxelnet_amd.workloads import scannet_v1_model_cfg, SCANNET_V1_TEST_CFG, indoor_meta
    V = a.views
    model = ia.build_detector(scannet_v1_model_cfg(), test_cfg=dict(SCANNET_V1_TEST_CFG))
    ia.randomize_(model, 78)
    with torch.no_grad():
        g = torch.Generator().manual_seed(5)
        model.bbox_head.cls_conv.weight.normal_(0, 0.01, generator=g)
        model.bbox_head.cls_conv.bias.fill_(-2.0)
        model.bbox_head.centerness_conv.weight.normal_(0, 0.005, generator=g)
        model.bbox_head.reg_conv.weight.normal_(0, 0.002, generator=g)
    dtype = torch.bfloat16 if a.storage == 'bf16' else torch.float32
    model.prepare(torch.device('cuda'), dtype=dtype)
    meta = indoor_meta(V, box_type=ia.DepthInstance3DBoxes)
    E = meta['lidar2img']['extrinsic']
    scene_meta = dict(meta, lidar2img={k: v for k, v in meta['lidar2img'].items() if k != 'extrinsic'})
    img = torch.randn(V, 3, 480, 640, generator=torch.Generator().manual_seed(13)).cuda()
    marks = [k for k in ARRIVALS if k <= V]

    # ---- per arrival: add_views(1) + detect()
    scene = model.open_scene(scene_meta)
    per_k = {k: [] for k in range(1, V + 1)}
    n_det = 0
    for p in range(a.passes + 1):                        # pass 0 warms every shape up
        scene.reset()
        for k in range(1, V + 1):
            out = []
            t = host_ms(lambda: out.append(scene.add_views(img[k - 1:k], E[k - 1:k]).detect()))
            if p:
                per_k[k].append(t)
            n_det = len(out[0][0]['scores_3d'])
    # the scene after the last pass against the one-shot lift of the same views
    p0 = model.features_2d_cl(img[None])
    vol, valid = model.lift_cl(p0, [meta])
    sv, sok = scene.volume()
    mask_equal = bool(torch.equal(sok, valid))
    dmax, scale = float((sv.float() - vol.float()).abs().max()), float(vol.float().abs().max())

    # ---- one shot over the k views so far
    one = {}
    for k in marks:
        mk = dict(meta, lidar2img=dict(meta['lidar2img'], extrinsic=E[:k]))
        x = img[:k][None].contiguous()
        for _ in range(2):
            model.simple_test(x, [mk])
        one[k] = [host_ms(lambda: model.simple_test(x, [mk])) for _ in range(a.reps)]

    # ---- the accumulate launch alone, one new view
    proj, no, crop = model._camera_setup([meta], 4, img.device)
    X, Y, Z = model.n_voxels
    Cn, FH, FW = p0.shape[-1], p0.shape[2], p0.shape[3]
    N, esz = X * Y * Z, p0.element_size()
    s = torch.zeros((1, X, Y, Z, Cn), device='cuda')
    c = torch.zeros((1, X, Y, Z), device='cuda', dtype=torch.int32)
    m = torch.empty((1, X, Y, Z, Cn), device='cuda', dtype=p0.dtype)
    ok = torch.empty((1, X, Y, Z), device='cuda', dtype=torch.uint8)
    f1, P1 = p0[:1].contiguous(), proj[:, :1].contiguous()
    t_emit = kernel_us(lambda: ops.backproject_accum_(f1, P1, no, crop, model.voxel_size, s, c, False, m, ok), a.kreps)
    t_plain = kernel_us(lambda: ops.backproject_accum_(f1, P1, no, crop, model.voxel_size, s, c, False), a.kreps)
    t_mean = kernel_us(lambda: ops.volume_mean(s, c, p0.dtype, out=m, valid_out=ok), a.kreps)
    t_lift = kernel_us(lambda: ops.backproject_mean(p0, proj, no, crop, model.voxel_size, model.n_voxels), a.kreps)
    feat_b = FH * FW * Cn * esz
    b_plain = N * Cn * 8 + N * 8 + feat_b
    b_emit = b_plain + N * Cn * esz + N
    b_mean = N * Cn * (4 + esz) + N * 5
    b_lift = N * Cn * esz + N + V * feat_b

    def rate(b, t):
        return f'{b / 1e6:.1f} | {t[0]:.1f} ({t[1]:.1f} .. {t[2]:.1f}) | {b / t[0] / 1e3:.0f}'

    all_k = [statistics.median(per_k[k]) for k in range(1, V + 1)]
    lines = [f'# Streaming scenes: scannet_v1, {V} views of 480 x 640 arriving one at a time ({a.storage} storage)', '',
             f'Device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}.  Random weights, {n_det} detections at the last arrival.', '',
             f'## Latency at arrival k (ms, host clock around calls that end in the detections\' device-to-host copy; median (min .. max))', '',
             f'| arrival k | add_views(1 view) + detect(), {a.passes} passes | simple_test over the k views so far, {a.reps} calls | ratio |', '|---|---|---|---|']
    for k in marks:
        lines.append(f'| {k} | {fmt(per_k[k])} | {fmt(one[k])} | {statistics.median(one[k]) / statistics.median(per_k[k]):.2f} |')
    lines += ['', f'Mean over all {V} arrivals of the per-arrival median: {statistics.mean(all_k):.2f} ms (min {min(all_k):.2f}, max {max(all_k):.2f}).',
              'The two columns do not differ in the trunk alone: detect() runs neck and head layer by layer from Python (detect_indoor_cl), simple_test runs '
              'the native handle, one C call for the whole step.  The ratio therefore holds the saving in the trunk MINUS the host launch overhead of the '
              'volume stages on the session\'s side; it is not the kernel-side gain.',
              f'After the last arrival: valid mask equal to the one-shot lift: {mask_equal}; max |volume - one-shot| = {dmax:.3e} = {dmax / scale:.2e} of max |one-shot| '
              '(the trunk saw the views one per call).', '',
              f'## Kernels ({N} voxels x {Cn} channels, one new view {FH} x {FW}; HIP events around {BATCH} back-to-back launches, per launch; median (min .. max) of {a.kreps} batches)', '',
             'A figure holds the kernel and the gap to the next dispatch, not the host\'s way to the first launch; it is an upper bound of the kernel time, the GB/s a lower bound.', '',
              'The state (sum + mean) is smaller than the 256 MiB Infinity Cache and the same buffers are re-used by every timed launch, so these rates are not HBM rates.', '',
              '| launch | MB from the shapes | us | GB/s |', '|---|---|---|---|',
              f'| accumulate 1 view, mean + mask stored | {rate(b_emit, t_emit)} |',
              f'| accumulate 1 view, no mean | {rate(b_plain, t_plain)} |',
              f'| volume_mean (sums -> mean + mask) | {rate(b_mean, t_mean)} |',
              f'| one-shot lift of all {V} views (ops.backproject_mean; feature maps counted once) | {rate(b_lift, t_lift)} |']
    print('\n'.join(lines), flush=True)
    if a.md:
        with open(a.md, 'w') as fo:
            fo.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
