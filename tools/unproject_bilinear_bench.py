"""Measure the unprojection alone with both sampling rules on the GPU box.  python tools/unproject_bilinear_bench.py [--md profiles/unproject_bilinear.md]

Shapes: the lift of KITTI at batch 4 (one view, 216 x 248 x 12 voxels, 64 channels, 96 x 320 maps), of ScanNet fast with 20 views (40 x 40 x 16, 256 channels,
120 x 160 maps) and of ScanNet v1 with 50 views (80 x 80 x 32, 64 channels), fp32 and bf16 maps, cameras of workloads.py, seeded random features.
Both rules run in ONE process on the same inputs, alternating: for every repetition HIP events around BATCH back-to-back launches of the nearest lift, then
around BATCH launches of the bilinear lift (ops.backproject_mean, sampling='nearest' / 'bilinear'); per launch = the event time / BATCH; median (min .. max)
over --reps repetitions after a warm-up of both.  A figure holds the kernel and the gap to the next dispatch, not the host's way to the first launch.
GB/s: the algorithmic bytes of SURVEY.md section 8d -- the volume and the mask written once, every feature map read once -- over that time; the bilinear rule
reads up to four pixels per sample, so its real traffic through L2 is larger than the bytes it is rated with, which are the same for both rules.
Not part of bench.py.  Needs a device: there is no fallback."""
import argparse
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

BATCH = 20      # launches between one pair of events


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(BATCH):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / BATCH


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    ap.add_argument('--reps', type=int, default=15)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('unproject_bilinear_bench needs a HIP device: nothing is measured without one')
    import imvoxelnet_amd as ia
    from imvoxelnet_amd import ops
    from imvoxelnet_amd.workloads import kitti_meta, indoor_meta
    shapes = [('KITTI, batch 4, 1 view', (216, 248, 12), (.32, .32, .32), 64, (384, 1280), [kitti_meta(t=(0.02 * b, 0.01 * b, 0.0)) for b in range(4)]),
              ('ScanNet fast, 20 views', (40, 40, 16), (.16, .16, .16), 256, (480, 640), [indoor_meta(20)]),
              ('ScanNet v1, 50 views', (80, 80, 32), (.08, .08, .08), 64, (480, 640), [indoor_meta(50)])]
    rows, notes = [], []
    for name, nv, vs, Cn, hw, metas in shapes:
        cam = types.SimpleNamespace(n_voxels=nv, voxel_size=vs, _compute_projection=ia.ImVoxelNet._compute_projection)
        cam._new_origin = lambda origin, cam=cam: ia.ImVoxelNet._new_origin(cam, origin)      # the camera set-up asks its model for the grid's corner
        proj, no, crop = ia.ImVoxelNet._camera_setup(cam, metas, 4, 'cuda')
        B, V = proj.shape[0], proj.shape[1]
        FH, FW = hw[0] // 4, hw[1] // 4
        N = nv[0] * nv[1] * nv[2]
        for dtype in (torch.float32, torch.bfloat16):
            feat = torch.randn(B * V, 1, FH, FW, Cn, generator=torch.Generator().manual_seed(3)).to(dtype).cuda()
            run = {s: (lambda s=s: ops.backproject_mean(feat, proj, no, crop, vs, nv, sampling=s)) for s in ('nearest', 'bilinear')}
            (vn, okn), (vb, okb) = run['nearest'](), run['bilinear']()
            same_mask, seen = bool(torch.equal(okn, okb)), float(okn.float().mean())
            dmax = float((vn.float() - vb.float()).abs().max())
            del vn, vb
            for _ in range(2):                               # warm-up of both rules (code objects, the allocator's blocks)
                for s in run:
                    timed(run[s])
            ts = {s: [] for s in run}
            for _ in range(a.reps):                          # alternating: a drift of the box hits both alike
                for s in run:
                    ts[s].append(timed(run[s]))
            esz = feat.element_size()
            nbytes = B * N * Cn * esz + B * N + B * V * FH * FW * Cn * esz
            med = {s: statistics.median(ts[s]) for s in run}
            cell = lambda s: f'{med[s]:.3f} ({min(ts[s]):.3f} .. {max(ts[s]):.3f}) | {nbytes / med[s] / 1e6:.0f}'       # noqa: E731
            rows.append(f'| {name} | {"bf16" if esz == 2 else "fp32"} | {nbytes / 1e6:.1f} | {cell("nearest")} | {cell("bilinear")} | {med["bilinear"] / med["nearest"]:.2f} |')
            notes.append(f'{name}, {"bf16" if esz == 2 else "fp32"}: {seen:.1%} of the voxels seen, masks equal: {same_mask}, max |bilinear - nearest| = {dmax:.3f}')
            del feat
            torch.cuda.empty_cache()
    lines = ['# Unprojection alone: nearest and bilinear sampling', '',
             f'Device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}.  tools/unproject_bilinear_bench.py: one process, both rules on the same inputs, '
             f'alternating; HIP events around {BATCH} back-to-back launches, per launch; median (min .. max) of {a.reps} repetitions.', '',
             'MB and GB/s: the algorithmic bytes of SURVEY.md section 8d (volume + mask written once, every feature map read once), the same for both rules; '
             'a figure holds the kernel and the gap to the next dispatch, so the times are upper bounds of the kernel time and the rates lower bounds.', '',
             '| lift | maps | MB | nearest ms | GB/s | bilinear ms | GB/s | bilinear / nearest |', '|---|---|---|---|---|---|---|---|'] + rows + [''] + [f'- {n}' for n in notes]
    print('\n'.join(lines), flush=True)
    if a.md:
        with open(a.md, 'w') as fo:
            fo.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
