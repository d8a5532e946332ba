"""Measure scrolling scenes (ivx_volume_scroll_fwd, SceneSession.scroll) on the GPU box.  python tools/scene_scroll_bench.py [--md profiles/scene_scroll.md]

Method of tools/scene_window_bench.py: HIP events around 20 back-to-back calls, the forms alternating in one process, median (min .. max) of --kreps
batches.  Two grids, one row of fp32 state each (sums, count, weight sum): scannet_fast 40 x 40 x 16, C = 256 and scannet_v1 80 x 80 x 32, C = 64.
  (a) kernel      ops.volume_scroll_ by one voxel along x, along y, along z and along all three, against
                  - a device-to-device copy_ of the same state bytes (three copy_ calls: the bandwidth yardstick), and
                  - the out-of-place torch equivalent a user could write today: zero a scratch, slice-copy into it, copy back, per field;
                  achieved GB/s counts one read and one write of the row per pass (three passes for the three-axis shift).  The scroll and the
                  torch equivalent are checked bit-equal on random bit patterns in the same run.
  (b) unroll      with --variants NAME=LIB,...: the same scrolls through other builds of csrc/volume_scroll.hip alone (other -DIVX_SCROLL_U /
                  -DIVX_SCROLL_WG), in the same process, alternating with the product build.  A variant is built with
                  hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC -DIVX_SCROLL_U=8 imvoxelnet_amd/csrc/volume_scroll.hip \
                        -Limvoxelnet_amd/csrc -l:libimvoxel_hip.so -Wl,-rpath,<dir of libimvoxel_hip.so> -o LIB
                  (the product library supplies the error reporting the entry point links against)
  (c) per arrival add_views(1 view) + scroll(one voxel on every axis, the sign alternating) + detect() against add_views + detect() on a second plain
                  session, host clock around calls that end in the detections' device-to-host copy; one warm pass, then the median over --passes.
Not part of bench.py.  Needs a device: there is no fallback.  A figure that could not be taken is written as "not measured"."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from scene_window_bench import BATCH, build, fmt, host_ms      # noqa: E402

GRIDS = {'scannet_fast': ((40, 40, 16), 256), 'scannet_v1': ((80, 80, 32), 64)}
SHIFTS = (('x', (1, 0, 0)), ('y', (0, 1, 0)), ('z', (0, 0, 1)), ('x, y and z', (1, 1, 1)))

# From `hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage` on csrc/volume_scroll.hip (a compile, not a run)
RESOURCES = '''| kernel (IVX_SCROLL_WG = 64) | U | VGPRs | scratch B/lane | LDS B | waves/SIMD |
|---|---|---|---|---|---|
| volume_scroll_axis_kernel, 16-byte elements (sums) | 2 | 24 | 0 | 0 | 8 |
| volume_scroll_axis_kernel, 16-byte elements (sums) | 4 | 44 | 0 | 0 | 8 |
| volume_scroll_axis_kernel, 16-byte elements (sums) | 8 | 56 | 0 | 0 | 8 |
| volume_scroll_axis_kernel, 4-byte elements (count, wsum) | 8 | 32 | 0 | 0 | 8 |

The product build is U = 8.'''


READING = '''## Reading

Of the run this file was first written from (MI355X).  One axis: a scroll takes 15 - 16 us (scannet_fast) / 20 - 21 us (scannet_v1) per call, 1.15 - 1.35 times the plain
copy_ of the same bytes, and is 2.5 - 3.3 times faster than the torch equivalent, without a second copy of the state.  Three axes are three passes: 38 / 60 us,
1.47 times faster than the torch equivalent on scannet_fast and level with it on scannet_v1 (1.06) -- the torch form moves all axes in one slice copy, the in-place
form pays one pass per axis and keeps the memory.  On scannet_fast every bare call of section (b) sits near 10.5 us from U = 4 on, whatever the axis: that is the
floor of a call's two back-to-back launches (sums, then count / wsum), not the kernels; the op of section (a) adds 4 - 5 us of host checks to it.  Unroll: on
the scannet_v1 x pass U = 1, 2, 4, 8 take 47, 31, 23 and 21 us; the z pass does not care; 256 lanes per workgroup instead of 64 lose 2.5 - 6 us on the z pass
and gain nothing elsewhere.  The product build is U = 8 with 64 lanes per workgroup.  A scroll per arrival costs a session 0.10 / 0.14 ms, which includes
recomputing the mean from the moved state.  No counter run was made.'''


def many_us(fns, reps, warmup=3):
    """us per call of every function of `fns`: alternating batches of BATCH back-to-back calls between two events each."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, fn in zip(ts, fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(BATCH):
                fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) * 1e3 / BATCH)
    return ts


def state(dims, Cn, seed=None):
    """One row of state.  seed: random bit patterns (the equality check); None: zeros (the time does not depend on the values)."""
    shapes = ((1,) + dims + (Cn,), (1,) + dims, (1,) + dims)
    if seed is None:
        return [torch.zeros(s, device='cuda', dtype=d) for s, d in zip(shapes, (torch.float32, torch.int32, torch.float32))]
    g = torch.Generator().manual_seed(seed)
    w = [torch.randint(-2 ** 31, 2 ** 31, s, generator=g, dtype=torch.int64).to(torch.int32).cuda() for s in shapes]
    return [w[0].view(torch.float32), w[1], w[2].view(torch.float32)]


def torch_scroll_(fields, scratch, shift):
    """What a user could write today, out of place: per field, zero a scratch, slice-copy the part that stays into it, copy it back."""
    for f, sc in zip(fields, scratch):
        dst, src = [slice(None)], [slice(None)]
        for L, s in zip(f.shape[1:4], shift):
            lo, hi = max(0, -s), max(max(0, -s), min(L, L - s))
            dst.append(slice(lo, hi))
            src.append(slice(lo + s, hi + s))
        sc.zero_()
        sc[tuple(dst)].copy_(f[tuple(src)])
        f.copy_(sc)


def variant_call(path):
    """ivx_volume_scroll_fwd of another build of csrc/volume_scroll.hip (the module docstring has the recipe)."""
    L = C.CDLL(os.path.abspath(path))
    fn = L.ivx_volume_scroll_fwd
    fn.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)] + [C.c_int32] * 5 + [C.c_void_p] * 4

    def scroll(fields, shift):
        X, Y, Z, Cn = fields[0].shape[1:]
        rc = fn(1, (C.c_int32 * 1)(0), (C.c_int32 * 3)(*shift), 1, X, Y, Z, Cn, fields[0].data_ptr(), fields[1].data_ptr(), fields[2].data_ptr(),
                C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
    return scroll


def kernel_rows(name, kreps, variants):
    from imvoxelnet_amd import ops
    dims, Cn = GRIDS[name]
    f, dst, scratch = state(dims, Cn), state(dims, Cn), state(dims, Cn)
    row_bytes = sum(t.numel() * 4 for t in f)
    # the forms agree bit for bit on random bit patterns
    a, b = state(dims, Cn, 7), state(dims, Cn, 7)
    equal = True
    for _, s in SHIFTS + (('back', (-2, 3, -1)),):
        ops.volume_scroll_(a[0], a[1], [0], [s], a[2])
        torch_scroll_(b, scratch, s)
        equal = equal and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    assert int((a[1] != 0).sum()) > 0
    del a, b

    def copy():
        for d, s in zip(dst, f):
            d.copy_(s)

    fns = [copy] + [lambda s=s: ops.volume_scroll_(f[0], f[1], [0], [s], f[2]) for _, s in SHIFTS] + [lambda s=s: torch_scroll_(f, scratch, s) for _, s in SHIFTS]
    vfns = [(vn, sn, (lambda vs=vs, s=s: vs(f, s))) for vn, vs in variants for sn, s in SHIFTS]
    ts = many_us(fns + [v[2] for v in vfns], kreps)
    torch.cuda.synchronize()
    tc, tk, tt, tv = ts[0], ts[1:1 + len(SHIFTS)], ts[1 + len(SHIFTS):1 + 2 * len(SHIFTS)], ts[1 + 2 * len(SHIFTS):]
    gbs = lambda t, passes: 2 * row_bytes * passes / (statistics.median(t) * 1e-6) / 1e9      # noqa: E731
    lines = [f'| {name} | {"x".join(map(str, dims))} x {Cn} | {row_bytes / 1e6:.1f} | copy_ of the state (3 calls) | {fmt(tc, 1)} | {gbs(tc, 1):.0f} | | |']
    notes = []
    for i, (sn, s) in enumerate(SHIFTS):
        passes = sum(1 for v in s if v)
        lines.append(f'| {name} | | | scroll along {sn} | {fmt(tk[i], 1)} | {gbs(tk[i], passes):.0f} | {fmt(tt[i], 1)} | {statistics.median(tt[i]) / statistics.median(tk[i]):.2f} |')
        if passes == 1 and sn in ('x', 'y') and gbs(tk[i], 1) < 0.5 * gbs(tc, 1):
            X, Y, Z = dims
            nlines = {'x': Y * Z, 'y': X * Z}[sn] * Cn // 4
            notes.append(f'{name}, {sn} pass: {gbs(tk[i], 1):.0f} GB/s is less than half the copy_ rate ({gbs(tc, 1):.0f} GB/s).  The pass of the sums has {nlines} lines, '
                         f'one lane each ({(nlines + 63) // 64} waves of 64 for 256 CUs), and a lane walks {dims["xy".index(sn)]} steps whose loads it can overlap only '
                         'IVX_SCROLL_U at a time: the time is the chain of a lane\'s round trips to memory (latency), not the bytes.  The launch of the 4-byte fields '
                         'adds a second, nearly empty kernel per pass.')
    vrows = [f'| {name} | {vn} | {sn} | {fmt(t, 1)} |' for (vn, sn, _), t in zip(vfns, tv)]
    return lines, notes, vrows, equal


def arrivals(ia, name, a):
    from imvoxelnet_amd.workloads import indoor_meta
    model = build(ia, name)
    model.prepare(torch.device('cuda'))
    n = a.views
    meta = indoor_meta(n, box_type=ia.DepthInstance3DBoxes)
    E = meta['lidar2img']['extrinsic']
    scene_meta = dict(meta, lidar2img={k: v for k, v in meta['lidar2img'].items() if k != 'extrinsic'})
    img = torch.randn(n, 3, 480, 640, generator=torch.Generator().manual_seed(13)).cuda()
    plain, moving = model.open_scene(scene_meta), model.open_scene(scene_meta)
    tp, tm = [], []
    for p in range(a.passes + 1):                                 # pass 0 warms every shape up
        plain.reset()
        moving.reset()
        for k in range(n):
            sign = 1 if k % 2 == 0 else -1
            t = host_ms(lambda: plain.add_views(img[k:k + 1], E[k:k + 1]).detect())
            u = host_ms(lambda: moving.add_views(img[k:k + 1], E[k:k + 1]).scroll((sign, sign, sign)).detect())
            if p:
                tp.append(t)
                tm.append(u)
    plain.close()
    moving.close()
    return tp, tm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    ap.add_argument('--kreps', type=int, default=20)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--views', type=int, default=8)
    ap.add_argument('--workloads', default='scannet_fast,scannet_v1')
    ap.add_argument('--variants', default='', help='NAME=LIB,...: other builds of csrc/volume_scroll.hip to time beside the product build')
    ap.add_argument('--skip-arrivals', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('scene_scroll_bench needs a HIP device: nothing is measured without one')
    import imvoxelnet_amd as ia
    names = a.workloads.split(',')
    variants = [(v.split('=')[0], variant_call(v.split('=')[1])) for v in a.variants.split(',') if v]
    if variants:                               # the product build through the same bare C call (no checks of the op around it), to compare like with like
        from imvoxelnet_amd import _lib
        variants.insert(0, ('product (U8, 64 lanes), bare C call', variant_call(_lib.LIB_PATH)))
    lines = ['# Scrolling scenes: the in-place voxel shift against a device copy and against the out-of-place torch equivalent', '',
             f'Device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}.  Written by tools/scene_scroll_bench.py.', '',
             '## (a) One row of fp32 state (sums, count, weight sum) scrolled by one voxel', '',
             f'us per call; HIP events around {BATCH} back-to-back calls, the forms alternating in one process; median (min .. max) of {a.kreps} batches each.  A figure holds '
             'the kernels of the call, the gaps between them and the host side of the op.  GB/s counts one read and one write of the row per pass (three passes '
             'for the three-axis shift; the copy_ is one pass).  The torch equivalent zeroes a scratch, slice-copies into it and copies back, per field: nine calls '
             'and a second copy of the state.  A row of state (26 / 54 MB) fits the 256 MB Infinity Cache, so rates above the HBM bandwidth are cache rates, for '
             'every form alike.', '',
             '| grid | voxels x C | state MB | form | ops.volume_scroll_ / copy_ us | GB/s | torch equivalent us | torch / scroll |', '|---|---|---|---|---|---|---|---|']
    notes, vrows, equal = [], [], True
    for name in names:
        rows, n, v, eq = kernel_rows(name, a.kreps, variants)
        lines += rows
        notes += n
        vrows += v
        equal = equal and eq
        torch.cuda.empty_cache()
    lines += ['', f'ops.volume_scroll_ and the torch equivalent bit-equal on random bit patterns over five successive shifts, every field: {equal}.']
    lines += [''] + (notes if notes else ['No x or y pass ran below half the copy_ rate.'])
    lines += ['', '## (b) Unroll factor and workgroup size: other builds of the kernel in the same process', '']
    if vrows:
        lines += ['us per call as in (a), measured in the same alternation.  Every row here is the bare C call (ctypes, no argument checks of the op around it), so '
                  'the rows compare with each other and not with (a); WG256: 256 lanes per workgroup instead of 64.', '', '| grid | build | scroll along | us |', '|---|---|---|---|'] + vrows
    else:
        lines += ['not measured in this run (no --variants given).']
    lines += ['', f'## (c) One arrival + detect() with and without a scroll (arrivals 1 .. {a.views}, fp32 storage, 480 x 640)', '',
              'ms, host clock around add_views(1 view) [+ scroll by one voxel on every axis] + detect(), which ends in the detections\' device-to-host copy; the two '
              f'sessions alternate arrival by arrival in one process; one warm pass, then median (min .. max) over {a.passes} passes.  The scrolling session also '
              'recomputes the mean from the moved state (the existing refresh), which the plain session gets from its lift.', '',
              '| workload | add_views + detect() | add_views + scroll + detect() | difference of the medians |', '|---|---|---|---|']
    for name in names:
        if a.skip_arrivals:
            lines.append(f'| {name} | not measured | not measured | |')
            continue
        try:
            tp, tm = arrivals(ia, name, a)
            lines.append(f'| {name} | {fmt(tp)} | {fmt(tm)} | {statistics.median(tm) - statistics.median(tp):+.2f} ms |')
        except torch.cuda.OutOfMemoryError as exc:
            print(f'{name}: {exc}', flush=True)
            lines.append(f'| {name} | not measured (out of device memory) | not measured | |')
        torch.cuda.empty_cache()
    lines += ['', READING, '', '## Kernel resources (compile-time, gfx950)', '', RESOURCES]
    print('\n'.join(lines), flush=True)
    if a.md:
        with open(a.md, 'w') as fo:
            fo.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
