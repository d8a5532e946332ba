"""Measure the lens-aware image pipeline (ivx_image_prep_lens_u8 / ivx_map_prep_lens, csrc/image_prep.hip) beside the plain entry
(ivx_image_prep_u8, csrc/image_prep.hip) on the GPU box.  python tools/image_prep_lens_bench.py [--md out.md]

Per geometry (network input 480 x 640, 384 x 1280, 928 x 1600 from the frames of the ScanNet, KITTI and nuScenes pipelines), in ONE process, the
three kernels alternating:
  kernel time    HIP events around --batch back-to-back launches, warm-up first, median of --reps such windows, divided by --batch (one launch of
                 these sizes takes tens of microseconds: a window of one would time the event pair);
  rate           (source bytes + output bytes) / kernel time -- the bytes the algorithm needs, the same count for all three;
  ratio          lens time / plain time.  The plain entry is the yardstick: it is the code as it was.
The map entry: the cover map and a uint16 depth frame to feature resolution (stride 4), per launch, same clock.
An arrival: SceneSession.add_views_u8 of one 968 x 1296 frame on a fading ScanNet-fast session with lens= (and with depth_frames=) against one
without, host clock around calls that end in a device synchronise, the three alternating.
Not part of bench.py.  Needs a device: there is no fallback."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

GEOMETRIES = [('ScanNet', (968, 1296), (640, 480), 8), ('KITTI', (375, 1242), (1280, 384), 4), ('nuScenes', (900, 1600), (1600, 900), 6)]


def lenses(hw):
    """A Brown and a fisheye lens of moderate distortion for a frame of hw; the ideal camera keeps the focal length."""
    from imvoxelnet_amd import data
    h, w = hw
    K = [[0.9 * w, 0, 0.5 * w - 0.3], [0, 0.9 * w, 0.5 * h + 0.2], [0, 0, 1]]
    return dict(Brown=data.Lens('brown', K, [-0.12, 0.02, 0.0008, -0.0005, 0.001]), fisheye=data.Lens('fisheye', K, [-0.03, 0.012, -0.004, 0.001]))


def windows_us(fns, reps, batch, warmup=3):
    """{name: (median, min, max) us per launch}: the functions take turns, each window is `batch` launches between two events."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(batch):
                fn()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1e3 / batch)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def host_clock_ms(fns, reps, warmup=3):
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--batch', type=int, default=20)
    ap.add_argument('--no-e2e', action='store_true')
    a = ap.parse_args()
    assert a.reps >= 20 and a.batch >= 1
    if not torch.cuda.is_available():
        raise SystemExit('image_prep_lens_bench needs a HIP device: nothing is measured without one')
    import imvoxelnet_amd as ia
    from imvoxelnet_amd import data, ops
    cfg = data.IMG_NORM_CFG
    fmt = lambda t: f'{t[0]:.1f} ({t[1]:.1f} .. {t[2]:.1f})'                      # noqa: E731
    lines = ['| geometry | n | resized -> plane | bytes moved (MB) | plain us (median; min .. max) | plain GB/s | Brown us | Brown GB/s | Brown / plain | '
             'fisheye us | fisheye GB/s | fisheye / plain | inside (Brown) |', '|---|---|---|---|---|---|---|---|---|---|---|---|---|']
    maps = ['', '| map entry (stride 4) | n | out | cover us (median; min .. max) | uint16 depth us | depth, no lens us |', '|---|---|---|---|---|---|']
    for name, (h, w), scale, n in GEOMETRIES:
        (nh, nw), (ph, pw) = data._pipeline_shapes((h, w), scale, 32, True)
        src = torch.from_numpy(np.random.RandomState(1).randint(0, 256, (n, h, w, 3)).astype(np.uint8)).cuda()
        out = torch.empty(n, 3, ph, pw, device='cuda')
        ls = lenses((h, w))
        fns = {'plain': lambda: ops.image_prep_u8(src, (nh, nw), (ph, pw), cfg['mean'], cfg['std'], True, out=out)}
        for k, l in ls.items():
            fns[k] = lambda l=l: ops.image_prep_lens_u8(src, l, (nh, nw), (ph, pw), cfg['mean'], cfg['std'], True, out=out)
        t = windows_us(fns, a.reps, a.batch)
        moved = src.numel() + out.numel() * 4
        inside = float(ops.map_prep_lens((nh, nw), (ph, pw), (h, w), ls['Brown'], stride=1)[0][:nh, :nw].mean())
        gbs = {k: moved / v[0] / 1e3 for k, v in t.items()}
        lines.append(f'| {name} {h} x {w} -> {scale} | {n} | {nh} x {nw} -> {ph} x {pw} | {moved / 1e6:.1f} | {fmt(t["plain"])} | {gbs["plain"]:.0f} | {fmt(t["Brown"])} | '
                     f'{gbs["Brown"]:.0f} | {t["Brown"][0] / t["plain"][0]:.2f} | {fmt(t["fisheye"])} | {gbs["fisheye"]:.0f} | {t["fisheye"][0] / t["plain"][0]:.2f} | {inside:.3f} |')
        print(lines[-1], flush=True)
        depth = torch.from_numpy(np.random.RandomState(2).randint(0, 6000, (n, h, w)).astype(np.uint16)).cuda()
        mout = torch.empty(n, ph // 4, pw // 4, device='cuda')
        m = windows_us({'cover': lambda: ops.map_prep_lens((nh, nw), (ph, pw), (h, w), ls['Brown'], n=n, out=mout),
                        'depth': lambda: ops.map_prep_lens((nh, nw), (ph, pw), (h, w), ls['Brown'], src=depth, scale=0.001, out=mout),
                        'ideal': lambda: ops.map_prep_lens((nh, nw), (ph, pw), (h, w), None, src=depth, scale=0.001, out=mout)}, a.reps, a.batch)
        maps.append(f'| {name} {h} x {w} | {n} | {ph // 4} x {pw // 4} | {fmt(m["cover"])} | {fmt(m["depth"])} | {fmt(m["ideal"])} |')
        print(maps[-1], flush=True)
        del src, out, depth, mout
    lines += maps
    if not a.no_e2e:
        from imvoxelnet_amd.workloads import indoor_meta, scannet_fast_model_cfg, SCANNET_FAST_TEST_CFG
        model = ia.build_detector(scannet_fast_model_cfg(), test_cfg=dict(SCANNET_FAST_TEST_CFG))
        ia.randomize_(model, 7)
        model.prepare(torch.device('cuda'))
        meta = indoor_meta(8, box_type=ia.DepthInstance3DBoxes)
        E = meta['lidar2img']['extrinsic']
        K = np.array([[1170., 0, 647.5, 0], [0, 1170., 483.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)      # the ideal camera at the source size
        user = dict(box_type_3d=ia.DepthInstance3DBoxes, lidar2img=dict(intrinsic=K, origin=meta['lidar2img']['origin']))
        h, w = 968, 1296
        lens = data.Lens('brown', [[1150.0, 0, 651.0], [0, 1151.0, 480.0], [0, 0, 1]], [0.09, 0.01, 0.0008, -0.0005, 0], new_K=K[:3, :3])
        frames = [np.random.RandomState(20 + i).randint(0, 256, (h, w, 3)).astype(np.uint8) for i in range(8)]
        depth = np.random.RandomState(30).randint(300, 5000, (1, h, w)).astype(np.uint16)
        kw = dict(decay=0.9, depth_gate=(0.5, 0.5))
        s = {k: model.open_scene(user, **kw) for k in ('plain', 'lens', 'lens+depth')}
        i = [0]

        def arrive(k, **extra):
            i[0] += 1
            s[k].add_views_u8([frames[i[0] % 8]], [E[i[0] % 8]], (640, 480), emit=False, **extra)
        t = host_clock_ms({'plain': lambda: arrive('plain'), 'lens': lambda: arrive('lens', lens=lens),
                           'lens+depth': lambda: arrive('lens+depth', lens=lens, depth_frames=depth)}, 30)
        fm = lambda v: f'{v[0]:.2f} ({v[1]:.2f} .. {v[2]:.2f})'                   # noqa: E731
        lines += ['', '| one arrival on a fading ScanNet-fast session, 968 x 1296 host frame -> 480 x 640 (host clock, median; min .. max of 30) | ms |', '|---|---|',
                  f'| add_views_u8, no lens | {fm(t["plain"])} |', f'| add_views_u8, lens= (cover cached after the first call) | {fm(t["lens"])} |',
                  f'| add_views_u8, lens= and depth_frames= (uint16 host frame) | {fm(t["lens+depth"])} |']
        print('\n'.join(lines[-6:]), flush=True)
    if a.md:
        with open(a.md, 'w') as fo:
            fo.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
