"""Measure the device-side image pipeline (ivx_image_prep_u8, csrc/image_prep.hip) on the GPU box.  python tools/image_prep_bench.py [--md out.md]

Per geometry (the four reference test pipelines at their benchmark batch sizes):
  kernel time    HIP events around one launch, warm-up first, median of --reps launches;
  rate           (source bytes + output bytes) / kernel time, next to ivx_ubench_copy moving the same byte total in this process
                 (the yardstick: the streaming copy rate of this box at this size; small totals stay inside the Infinity Cache for both);
  host time      data.prepare_image per frame on this machine's CPU (median of 3).
For KITTI batch 4: simple_test_u8 from host uint8 frames (H2D of the uint8 frames + the kernel + the model) against simple_test on an fp32
tensor that is already on the device (the model alone), host clock around calls that end in the result's device-to-host copy.
Not part of bench.py.  Needs a device: there is no fallback."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

GEOMETRIES = [('KITTI', (375, 1242), (1280, 384), 4), ('nuScenes', (900, 1600), (1600, 900), 6), ('ScanNet', (968, 1296), (640, 480), 50),
              ('SUN RGB-D', (530, 730), (640, 480), 1)]


def kernel_us(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def copy_gbps(total_bytes):
    """ivx_ubench_copy moving `total_bytes` in all (read + written)."""
    from imvoxelnet_amd import _lib
    n = max(16, total_bytes // 2 // 16 * 16)
    a, b = torch.empty(n, dtype=torch.uint8, device='cuda'), torch.empty(n, dtype=torch.uint8, device='cuda')
    a.zero_()
    v = C.c_double()
    _lib.check(_lib.lib().ivx_ubench_copy(C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), n, C.byref(v),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'ivx_ubench_copy')
    return v.value


def host_clock_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--no-e2e', action='store_true')
    a = ap.parse_args()
    assert a.reps >= 20
    if not torch.cuda.is_available():
        raise SystemExit('image_prep_bench needs a HIP device: nothing is measured without one')
    import imvoxelnet_amd as ia
    from imvoxelnet_amd import data, ops
    cfg = data.IMG_NORM_CFG
    lines = ['| geometry | n | resized -> plane | kernel us (median; min .. max) | bytes moved (MB) | kernel GB/s | copy GB/s, same bytes | kernel / copy | '
             'host prepare_image ms / frame |', '|---|---|---|---|---|---|---|---|---|']
    for name, (h, w), scale, n in GEOMETRIES:
        nh, nw = data.rescale_size((h, w), scale)
        ph, pw = (nh + 31) // 32 * 32, (nw + 31) // 32 * 32
        frames = np.random.RandomState(1).randint(0, 256, (n, h, w, 3)).astype(np.uint8)
        src = torch.from_numpy(frames).cuda()
        out = torch.empty(n, 3, ph, pw, device='cuda')
        med, lo, hi = kernel_us(lambda: ops.image_prep_u8(src, (nh, nw), (ph, pw), cfg['mean'], cfg['std'], True, out=out), a.reps)
        moved = src.numel() + out.numel() * 4
        rate, copy = moved / med / 1e3, copy_gbps(moved)
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            ref, _ = data.prepare_image(frames[0], scale)
            host.append((time.perf_counter() - t0) * 1e3)
        assert torch.equal(out[0].cpu(), ref), f'{name}: the kernel output is not prepare_image\'s'
        lines.append(f'| {name} {h} x {w} -> {scale} | {n} | {nh} x {nw} -> {ph} x {pw} | {med:.1f} ({lo:.1f} .. {hi:.1f}) | {moved / 1e6:.1f} | {rate:.0f} | {copy:.0f} | '
                     f'{rate / copy:.2f} | {statistics.median(host):.0f} |')
        print(lines[-1], flush=True)
        del src, out
    if not a.no_e2e:
        from imvoxelnet_amd.workloads import kitti_model_cfg, kitti_meta, KITTI_TEST_CFG
        model = ia.build_detector(kitti_model_cfg(), test_cfg=KITTI_TEST_CFG)
        ia.randomize_(model, 7)
        frames = [np.random.RandomState(10 + i).randint(0, 256, (375, 1242, 3)).astype(np.uint8) for i in range(4)]
        user = [{k: v for k, v in kitti_meta(box_type=ia.LiDARInstance3DBoxes).items() if k not in ('img_shape', 'ori_shape')} for _ in range(4)]
        prepared = [data.prepare_image(f, (1280, 384)) for f in frames]
        img = torch.stack([t for t, _ in prepared])[:, None].cuda()
        metas = [dict(u, **m) for u, (_, m) in zip(user, prepared)]
        t_f32 = host_clock_ms(lambda: model.simple_test(img, metas), 20)
        t_u8 = host_clock_ms(lambda: model.simple_test_u8(frames, user, (1280, 384)), 20)
        t_h2d = host_clock_ms(lambda: torch.from_numpy(np.stack(frames)).cuda(), 20)
        lines += ['', '| KITTI batch 4, end to end (host clock, median; min .. max of 20) | ms |', '|---|---|',
                  f'| simple_test, fp32 [4,1,3,384,1280] already on the device | {t_f32[0]:.2f} ({t_f32[1]:.2f} .. {t_f32[2]:.2f}) |',
                  f'| simple_test_u8 from 4 host uint8 frames 375 x 1242 (stack + H2D + kernel + model) | {t_u8[0]:.2f} ({t_u8[1]:.2f} .. {t_u8[2]:.2f}) |',
                  f'| of which: np.stack + H2D copy of the 4 uint8 frames alone | {t_h2d[0]:.2f} ({t_h2d[1]:.2f} .. {t_h2d[2]:.2f}) |']
        print('\n'.join(lines[-5:]), flush=True)
    if a.md:
        with open(a.md, 'w') as fo:
            fo.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
