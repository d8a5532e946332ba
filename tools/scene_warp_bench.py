"""Measure warping scenes (ivx_volume_warp_fwd, SceneSession.warp) on the GPU box.  python tools/scene_warp_bench.py [--md profiles/scene_warp.md]

Method of tools/scene_scroll_bench.py: HIP events around 20 back-to-back calls, the forms alternating in one process, median (min .. max) of --kreps
batches.  Three grids, one row of fp32 state each (sums, weight sum, count): scannet_fast 40 x 40 x 16, C = 256; scannet_v1 80 x 80 x 32, C = 64;
kitti 216 x 248 x 12, C = 64.  The motion is a vehicle's tick: 2 degrees of yaw, 0.5 degrees of pitch and a translation of (1.3, 0.4, 0.1) voxels.
  (a) kernel      ops.volume_warp of one row into a second pool, against
                  - a device-to-device copy_ of the same state bytes (three copy_ calls: the floor, one read and one write of the row), and
                  - the torch formulation a user could write today: F.grid_sample (trilinear, zeros outside, align_corners) on the sums permuted to
                    [1,C,X,Y,Z] and on the weight sum, the result permuted back to channels-last; its sampling grid is built once, outside the timing,
                    and it forms no count.  Its border rule differs (it blends with zeros up to one voxel beyond the grid on both sides, the entry
                    stops at g < N), so the two are compared on the voxels whose eight corners lie inside.
                  GB/s counts one read and one write of the row.
  (b) tiling      with --variants NAME=LIB,...: the same call through other builds of csrc/volume_warp.hip alone (-DIVX_WARP_VW=64: 64 voxels per
                  wave whatever C; -DIVX_WARP_WG=64: 64 lanes per workgroup), in the same process, alternating with the product build, all through
                  the bare C call.  A variant is built with
                  hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC -ffp-contract=off -DIVX_WARP_VW=64 imvoxelnet_amd/csrc/volume_warp.hip \
                        -Limvoxelnet_amd/csrc -l:libimvoxel_hip.so -Wl,-rpath,<dir of libimvoxel_hip.so> -o LIB
  (c) per arrival add_views(1 view) + warp + detect() against add_views + detect() on a second fading session (decay=0.9), host clock around calls
                  that end in the detections' device-to-host copy; one warm pass, then the median over --passes.
  --only-kernel N runs N product calls per grid and nothing else: the body of a counter run of its own (rocprofv3 --pmc ... -- python
  tools/scene_warp_bench.py --only-kernel 3); profiles/scene_warp.md, section (d), has what such a run said.
Not part of bench.py.  Needs a device: there is no fallback.  A figure that could not be taken is written as "not measured"."""
import argparse
import ctypes as C
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from scene_window_bench import BATCH, build, fmt, host_ms      # noqa: E402
from scene_scroll_bench import many_us                        # noqa: E402

GRIDS = {'scannet_fast': ((40, 40, 16), 256, (0.16, 0.16, 0.16)), 'scannet_v1': ((80, 80, 32), 64, (0.08, 0.08, 0.08)),
         'kitti': ((216, 248, 12), 64, (0.32, 0.32, 0.32))}

# From `hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -Rpass-analysis=kernel-resource-usage` on csrc/volume_warp.hip (a compile, not a run)
RESOURCES = '''| kernel | VGPRs | SGPRs | scratch B/lane | LDS B | waves/SIMD |
|---|---|---|---|---|---|
| volume_warp_kernel (256 lanes per workgroup) | 58 | 48 | 0 | 0 | 8 |'''


READING = '''## (d) Counters of the kernel alone

rocprofv3 --pmc in a run of its own (counters only, no tracing), two passes of `python tools/scene_warp_bench.py --only-kernel 2`, per dispatch of volume_warp_kernel; the
two dispatches of a grid agree within 2 %.  Taken on the build with 16 voxels per wave for every C (the product's tiling at C = 64; at C = 256 the product now has 4).

| grid | state MB | TCC_REQ_sum | TCC_HIT_sum | TCC_MISS_sum | L2 hit rate | FETCH_SIZE MB | WRITE_SIZE MB |
|---|---|---|---|---|---|---|---|
| scannet_fast | 26.4 | 1 207 691 | 503 644 | 705 562 | 42 % | 31.2 | 25.8 |
| scannet_v1 | 54.1 | 2 494 417 | 1 436 876 | 1 057 951 | 58 % | 39.6 | 52.8 |
| kitti | 169.7 | 8 604 334 | 3 228 768 | 5 372 041 | 38 % | 253.6 | 166.0 |

WRITE_SIZE is the row, as it must be.  The eight corner reads of every destination voxel are up to 1.6 / 3.3 / 10.3 million 128-byte requests of the sums alone; the L2 sees
1.2 / 2.5 / 8.6 million requests in all, stores included, so the vector L1 absorbs most of the eightfold re-read, not the L2.  Of what reaches the L2, 42 / 58 / 38 % hits.
FETCH_SIZE is known to report half the bytes of 16-byte-per-lane streaming reads on gfx950 (it is below the row size on scannet_v1, which cannot be); doubled, the fabric
side -- Infinity Cache hits included -- fetches 2.4 / 1.5 / 3.0 times the row where the floor is 1.0.  The expectation that most corner reads hit L2 or the Infinity Cache holds
in the sense that 8 reads per cell become 1.5 - 3 fetches, and not in the sense of one: neighbouring workgroups run on different XCDs, each with its own L2, and fetch
their shared corners once each.  Re-dealing the workgroup ids so that an XCD walks a contiguous eighth of the row did not change the time (section (b) of an earlier run of
this tool, in one alternation with the 16-voxel build: 22.8 / 28.9 / 109.1 us against 23.7 / 28.9 / 105.9 us) and is not in the code; its counters were not taken.

## Worst error against the fp64 reference

tests/test_gpu_volume_warp.py and tests/test_gpu_scene_warp.py print, per case, the worst |got - ref| / bound with bound = 11 * 2^-24 * sum |w S_corner| + 2^-126
(tests/ref_volume_warp.py).  On the MI355X, over all cases: sums 0.503 (a row of a fading batch, 4608 voxels x 64 channels), weight sum 0.373; the kernel cases alone
0.453 and 0.348.  count was equal everywhere.  A constant mean departed from its value by at most 3.7e-07 relative (allowed 1.4e-06).

## Reading

Of the run this file was written from (MI355X).  The entry alone (bare C call) takes 18.5 us on a row of ScanNet fast, 29.1 us on ScanNet v1 and 107 us on the KITTI
grid: 1.5, 1.4 and 1.5 times the device copy_ of the same bytes (12.0 / 21.0 / 73.1 us), which is the floor of one read and one write of the row, and 29, 25 and 25 times
faster than F.grid_sample on the permuted sums and the weight sum (534 / 726 / 2672 us, sampling grid not counted, no count formed).  Through ops.volume_warp a call
takes 40 / 42 / 115 us back to back: on the two ScanNet grids the host side of the op (the rigidity check in float64, the lists built for ctypes) takes longer than the
kernel, so back-to-back calls are host bound there; a scene makes one call per tick.  Voxels per wave: both channel counts are fastest where a wave has four
steps (4 voxels at C = 256, 16 at C = 64); one voxel per wave leaves one lane in the geometry part and costs 5 times as much at C = 64, 64 voxels per wave makes a
ScanNet-fast row 400 waves of 64 steps.  256 lanes per workgroup beat 64 on the KITTI grid and tie elsewhere.  A warp per arrival costs a fading session 0.15 / 0.17 ms,
which includes recomputing the mean from the resampled state.'''


def motion(dims, vs):
    """float64 4x4, x_old = T x_new: the rotation about the grid's centre (the grid is centred on the origin here), then the translation."""
    yaw, pitch = math.radians(2.0), math.radians(0.5)
    Rz = np.array([[math.cos(yaw), -math.sin(yaw), 0], [math.sin(yaw), math.cos(yaw), 0], [0, 0, 1]])
    Ry = np.array([[math.cos(pitch), 0, math.sin(pitch)], [0, 1, 0], [-math.sin(pitch), 0, math.cos(pitch)]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry
    T[:3, 3] = np.array([1.3, 0.4, 0.1]) * np.asarray(vs)
    return T


def state(dims, Cn, seed):
    g = torch.Generator().manual_seed(seed)
    W = torch.rand((1,) + dims, generator=g) * 3.5 + 0.5
    S = torch.randn((1,) + dims + (Cn,), generator=g) * W[..., None]
    return [S.cuda(), W.cuda(), torch.randint(1, 9, (1,) + dims, generator=g, dtype=torch.int32).cuda()]


def torch_grid(dims, vs, origin, T):
    """The sampling grid of F.grid_sample for the same motion, [1,X,Y,Z,3] in (z, y, x) order, normalised with align_corners=True; fp32 like the entry's
    coordinates, built from float64 on the host once."""
    X, Y, Z = dims
    idx = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing='ij'), -1).astype(np.float64)
    p = idx * np.asarray(vs) + np.asarray(origin, np.float64)
    g = ((p @ T[:3, :3].T + T[:3, 3]) - np.asarray(origin, np.float64)) / np.asarray(vs)
    norm = 2 * g / (np.asarray(dims) - 1) - 1
    return torch.from_numpy(norm[..., ::-1].astype(np.float32).copy())[None].cuda(), g


def torch_warp(f, grid):
    import torch.nn.functional as F
    S = F.grid_sample(f[0].permute(0, 4, 1, 2, 3), grid, mode='bilinear', padding_mode='zeros', align_corners=True).permute(0, 2, 3, 4, 1).contiguous()
    W = F.grid_sample(f[1][:, None], grid, mode='bilinear', padding_mode='zeros', align_corners=True)[:, 0]
    return S, W


def c_call(path):
    """ivx_volume_warp_fwd of a build of csrc/volume_warp.hip through ctypes, with no checks of the op around it."""
    L = C.CDLL(os.path.abspath(path))
    fn = L.ivx_volume_warp_fwd
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    fn.argtypes = [C.c_int32, i32p, i32p, f32p, f32p, f32p, C.c_float] + [C.c_int32] * 6 + [C.c_void_p] * 7

    def warp(f, out, T, origin, vs):
        X, Y, Z, Cn = f[0].shape[1:]
        rc = fn(1, (C.c_int32 * 1)(0), (C.c_int32 * 1)(0), (C.c_float * 12)(*T[:3].reshape(-1).tolist()), (C.c_float * 3)(*[float(v) for v in origin]),
                (C.c_float * 3)(*vs), 0.0, 1, 1, X, Y, Z, Cn, *[t.data_ptr() for t in f], *[t.data_ptr() for t in out], C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
    return warp


def kernel_rows(name, kreps, variants, only=0):
    from imvoxelnet_amd import ops
    dims, Cn, vs = GRIDS[name]
    origin = (-np.asarray(dims) / 2 * np.asarray(vs)).astype(np.float32)
    T = motion(dims, vs)
    f = state(dims, Cn, 7)
    out = [torch.empty_like(t) for t in f]
    call = lambda: ops.volume_warp(*f, [0], [T], origin[None], vs, out=out)      # noqa: E731
    if only:
        for _ in range(only):
            call()
        torch.cuda.synchronize()
        return [], [], ''
    row_bytes = sum(t.numel() * 4 for t in f)
    grid, g = torch_grid(dims, vs, origin, T)
    call()
    tS, tW = torch_warp(f, grid)
    inner = torch.from_numpy(np.all((g >= 0) & (g <= np.asarray(dims) - 1), axis=-1))[None].cuda()       # all eight corners inside: the two border rules agree
    scale = float(f[0].abs().max())
    agree = (f'largest difference between ops.volume_warp and the torch formulation on the {int(inner.sum())} of {inner.numel()} voxels whose eight corners lie inside: '
             f'sums {float((out[0] - tS)[inner].abs().max()):.2e} (largest |sum| {scale:.1f}), weight sum {float((out[1] - tW)[inner].abs().max()):.2e}')
    del tS, tW

    def copy():
        for d, s in zip(out, f):
            d.copy_(s)

    vfns = [(vn, (lambda vw=vw: vw(f, out, T, origin, vs))) for vn, vw in variants]
    ts = many_us([copy, call, lambda: torch_warp(f, grid)] + [v[1] for v in vfns], kreps)
    torch.cuda.synchronize()
    tc, tk, tt, tv = ts[0], ts[1], ts[2], ts[3:]
    gbs = lambda t: 2 * row_bytes / (statistics.median(t) * 1e-6) / 1e9      # noqa: E731
    lines = [f'| {name} | {"x".join(map(str, dims))} x {Cn} | {row_bytes / 1e6:.1f} | {fmt(tc, 1)} | {gbs(tc):.0f} | {fmt(tk, 1)} | {gbs(tk):.0f} | '
             f'{statistics.median(tk) / statistics.median(tc):.2f} | {fmt(tt, 1)} | {statistics.median(tt) / statistics.median(tk):.2f} |']
    vrows = [f'| {name} | {vn} | {fmt(t, 1)} |' for (vn, _), t in zip(vfns, tv)]
    return lines, vrows, f'{name}: {agree}.'


def arrivals(ia, name, a):
    from imvoxelnet_amd.workloads import indoor_meta
    model = build(ia, name)
    model.prepare(torch.device('cuda'))
    n = a.views
    meta = indoor_meta(n, box_type=ia.DepthInstance3DBoxes)
    E = meta['lidar2img']['extrinsic']
    scene_meta = dict(meta, lidar2img={k: v for k, v in meta['lidar2img'].items() if k != 'extrinsic'})
    img = torch.randn(n, 3, 480, 640, generator=torch.Generator().manual_seed(13)).cuda()
    still, moving = model.open_scene(scene_meta, decay=0.9), model.open_scene(scene_meta, decay=0.9)
    T = motion(model.n_voxels, model.voxel_size)
    Tinv = np.linalg.inv(T)
    ts, tm = [], []
    for p in range(a.passes + 1):                                 # pass 0 warms every shape up
        still.reset()
        moving.reset()
        for k in range(n):
            t = host_ms(lambda: still.add_views(img[k:k + 1], E[k:k + 1]).detect())
            u = host_ms(lambda: moving.add_views(img[k:k + 1], E[k:k + 1]).warp(T if k % 2 == 0 else Tinv).detect())
            if p:
                ts.append(t)
                tm.append(u)
    still.close()
    moving.close()
    return ts, tm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    ap.add_argument('--kreps', type=int, default=20)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--views', type=int, default=8)
    ap.add_argument('--grids', default='scannet_fast,scannet_v1,kitti')
    ap.add_argument('--workloads', default='scannet_fast,scannet_v1')
    ap.add_argument('--variants', default='', help='NAME=LIB,...: other builds of csrc/volume_warp.hip to time beside the product build')
    ap.add_argument('--skip-arrivals', action='store_true')
    ap.add_argument('--only-kernel', type=int, default=0, help='run this many product calls per grid and nothing else (the body of a counter run)')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('scene_warp_bench needs a HIP device: nothing is measured without one')
    import imvoxelnet_amd as ia
    grids = a.grids.split(',')
    if a.only_kernel:
        for name in grids:
            kernel_rows(name, 0, [], a.only_kernel)
        return
    variants = [(v.rsplit('=', 1)[0], c_call(v.rsplit('=', 1)[1])) for v in a.variants.split(',') if v]
    if variants:                               # the product build through the same bare C call, to compare like with like
        from imvoxelnet_amd import _lib
        variants.insert(0, ('product (256 / G voxels per wave, 256 lanes per workgroup), bare C call', c_call(_lib.LIB_PATH)))
    lines = ['# Warping scenes: the rigid resample of the state against a device copy and against F.grid_sample', '',
             f'Device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}.  Written by tools/scene_warp_bench.py.', '',
             '## (a) One row of fp32 state (sums, weight sum, count) resampled under 2 degrees of yaw, 0.5 of pitch and (1.3, 0.4, 0.1) voxels', '',
             f'us per call; HIP events around {BATCH} back-to-back calls, the forms alternating in one process; median (min .. max) of {a.kreps} batches each.  A figure holds '
             'the kernels of the call, the gaps between them and the host side of the op.  GB/s counts one read and one write of the row, for every form.  '
             'The copy_ (three calls, one per field) is the floor: the entry reads every source cell up to eight times, from cache if the expectation of '
             'csrc/volume_warp.hip holds.  The torch formulation permutes the sums to channels-first, calls F.grid_sample on sums and weight sum with a '
             'sampling grid built outside the timing, permutes back, and forms no count.  Rows of 26 / 54 / 168 MB fit the 256 MB Infinity Cache, so rates '
             'above the HBM bandwidth are cache rates, for every form alike.', '',
             '| grid | voxels x C | state MB | copy_ us | GB/s | ops.volume_warp us | GB/s | warp / copy_ | torch formulation us | torch / warp |', '|---|---|---|---|---|---|---|---|---|---|']
    vrows, notes = [], []
    for name in grids:
        rows, v, note = kernel_rows(name, a.kreps, variants)
        lines += rows
        vrows += v
        notes.append(note)
        torch.cuda.empty_cache()
    lines += [''] + notes
    lines += ['', '## (b) Voxels per wave and workgroup size: other builds of the kernel in the same process', '']
    if vrows:
        lines += ['us per call as in (a), measured in the same alternation.  Every row here is the bare C call (ctypes, no argument checks of the op around it), so '
                  'the rows compare with each other and not with (a).', '', '| grid | build | us |', '|---|---|---|'] + vrows
    else:
        lines += ['not measured in this run (no --variants given).']
    lines += ['', f'## (c) One arrival + detect() with and without a warp (arrivals 1 .. {a.views}, decay=0.9, fp32 storage, 480 x 640)', '',
              'ms, host clock around add_views(1 view) [+ warp by the motion of (a), or by its inverse on every second arrival] + detect(), which ends in the '
              f'detections\' device-to-host copy; the two sessions alternate arrival by arrival in one process; one warm pass, then median (min .. max) over {a.passes} '
              'passes.  The warping session also recomputes the mean from the resampled state (the existing refresh), which the other session gets from its lift.', '',
              '| workload | add_views + detect() | add_views + warp + detect() | difference of the medians |', '|---|---|---|---|']
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
    lines += ['', READING]
    lines += ['', '## Kernel resources (compile-time, gfx950)', '', RESOURCES]
    print('\n'.join(lines), flush=True)
    if a.md:
        with open(a.md, 'w') as fo:
            fo.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
