"""Measure scene snapshots (ivx_volume_pack_fwd / ivx_volume_unpack_fwd, SceneSession.snapshot) on the GPU box.
python tools/scene_snapshot_bench.py [--md profiles/scene_snapshot.md]

Method of tools/scene_merge_bench.py: HIP events around 20 back-to-back calls, the forms alternating in one process, median (min .. max) of --kreps
batches; host-clock figures end in a device synchronise.  One row of fp32 state (sums, weight sum, count) at three grids: scannet_fast 40 x 40 x 16,
C = 256; scannet_v1 80 x 80 x 32, C = 64; kitti 216 x 248 x 12, C = 64.  The states are made by real lifts of a fading session (decay=0.9) of the
workload's model on random images: `1 view`, `20 views` (for kitti: the one camera at 20 positions along x, 0.5 m apart), and `moved`: the
20-view scene with forget_below=0.3 after two more ticks and a scroll by a quarter of the grid along x (kitti, whose anchor head refuses a scroll:
a warp by 8 voxels forward and 3 degrees of yaw).
  (a) pack         ivx_volume_pack_fwd alone at cap = n: the bare C call (count, scan and write launches), no readback.
  (b) count        its count-only form (cap = 0): the two counting launches.
  (c) unpack       ivx_volume_unpack_fwd alone from those records.
  (d) copy_        a device copy_ of the dense row (three fields) into a twin: the floor of pack or unpack when everything is seen.
  (e) torch pack   what torch offers for the same job: nonzero of the kept mask (a host sync inside), index_select on the [X*Y*Z, C] view and the
                   gathers of count, weight sum and the int32 index.
  (f) op           ops.volume_pack: count, read n back, allocate, pack (two C calls, one host sync).
  (g) snapshot()   end to end on the host clock, against .cpu() of the three dense fields; and the bytes of the saved files.
  (h) per arrival  add_views(1 view) + snapshot() + detect() against add_views + detect() on a second fading session.
The tool writes tables and no interpretation: profiles/scene_snapshot.md ends in a '## Reading' written by hand, which --md keeps and marks as older.
Not part of bench.py.  Needs a device: there is no fallback.  A figure that could not be taken is written as "not measured yet"."""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from scene_window_bench import BATCH, build, fmt, host_ms      # noqa: E402
from scene_scroll_bench import many_us                        # noqa: E402

# From `hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -Rpass-analysis=kernel-resource-usage` on csrc/volume_pack.hip (a compile, not a run)
RESOURCES = '''| kernel | VGPRs | scratch B/lane | LDS B | waves/SIMD |
|---|---|---|---|---|
| volume_pack_count_kernel | 6 | 0 | 16 | 8 |
| volume_pack_scan_kernel | 22 | 0 | 16 | 8 |
| volume_pack_write_kernel<false> (F32 payload) | 26 | 0 | 1040 | 8 |
| volume_pack_write_kernel<true> (bf16 payload) | 33 | 0 | 2064 | 8 |
| volume_unpack_kernel<false> | 24 | 0 | 1032 | 8 |
| volume_unpack_kernel<true> | 28 | 0 | 2056 | 8 |

256 lanes per workgroup, one chunk of 256 voxels per workgroup, 4 payload elements of 16 bytes in flight per lane.'''

KEPT = 'The reading below was written by hand for the tables of an earlier run and is kept as it was: check it against the tables above.'
NOT = 'not measured yet'


def make_model(ia, name):
    if name != 'kitti':
        return build(ia, name)
    from imvoxelnet_amd import workloads as wl
    model = ia.build_detector(wl.kitti_model_cfg(), test_cfg=dict(wl.KITTI_TEST_CFG))
    ia.randomize_(model, 0)
    return model


def views_of(ia, name, n):
    """(scene meta, n extrinsics, n images) of a workload."""
    from imvoxelnet_amd import workloads as wl
    g = torch.Generator().manual_seed(13)
    if name == 'kitti':
        meta = wl.kitti_meta(box_type=ia.LiDARInstance3DBoxes)
        E = [wl.kitti_meta(t=(0.0, 0.0, -0.5 * i))['lidar2img']['extrinsic'][0] for i in range(n)]
        img = torch.randn(n, 3, 384, 1280, generator=g).cuda()
    else:
        meta = wl.indoor_meta(n, box_type=ia.DepthInstance3DBoxes)
        E = meta['lidar2img']['extrinsic']
        img = torch.randn(n, 3, 480, 640, generator=g).cuda()
    return dict(meta, lidar2img={k: v for k, v in meta['lidar2img'].items() if k != 'extrinsic'}), E, img


def scenes_of(ia, name, model, n):
    """The three states: {label: session}."""
    meta, E, img = views_of(ia, name, n)
    one = model.open_scene(meta, decay=0.9)
    one.add_views(img[:1], E[:1])
    many, moved = model.open_scene(meta, decay=0.9), model.open_scene(meta, decay=0.9, forget_below=0.3)
    for s in (many, moved):
        for k in range(0, n, 4):
            s.add_views(img[k:k + 4], E[k:k + 4], emit=False)
    for k in (0, 1):
        moved.add_views(img[k:k + 1], E[k:k + 1], emit=False)
    if name == 'kitti':
        T = np.eye(4)
        a = np.deg2rad(3.0)
        T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        T[0, 3] = 8 * model.voxel_size[0]
        moved.warp(T)
    else:
        moved.scroll((model.n_voxels[0] // 4, 0, 0))
    return {'1 view': one, f'{n} views': many, 'moved': moved}


def c_entries():
    """The two entries of the product build through ctypes, with no checks of the ops around them."""
    from imvoxelnet_amd import _lib
    L = _lib.lib()
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)     # noqa: E731
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())       # noqa: E731
    row = (C.c_int32 * 1)(0)

    def pack(state, cap, outs, n_out, scratch):
        _, X, Y, Z, Cn = state[0].shape
        rc = L.ivx_volume_pack_fwd(1, row, 1, X, Y, Z, Cn, p(state[0]), p(state[2]), p(state[1]), 0, cap, *(p(t) for t in outs), p(n_out), p(scratch), st())
        assert rc == 0, L.ivx_last_error()

    def unpack(state, n, recs):
        _, X, Y, Z, Cn = state[0].shape
        rc = L.ivx_volume_unpack_fwd(1, row, (C.c_int32 * 1)(n), n, *(p(t) for t in recs), 0, 1, X, Y, Z, Cn, p(state[0]), p(state[2]), p(state[1]), st())
        assert rc == 0, L.ivx_last_error()
    return L, pack, unpack


def torch_pack(state):
    S, W, cnt = state
    nz = torch.nonzero((cnt.view(-1) != 0) | (W.view(-1).view(torch.int32) != 0)).view(-1)
    return nz.to(torch.int32), S.view(-1, S.shape[-1]).index_select(0, nz), W.view(-1).index_select(0, nz), cnt.view(-1).index_select(0, nz)


def kernel_row(name, label, s, kreps):
    from imvoxelnet_amd import ops
    L, pack, unpack = c_entries()
    state = (s._sum, s._wsum, s._count)
    _, X, Y, Z, Cn = s._sum.shape
    nvox = X * Y * Z
    n = ops.volume_pack_count(s._sum, s._count, [0], s._wsum)[0]
    dev = s._sum.device
    outs = (torch.empty((1, n), device=dev, dtype=torch.int32), torch.empty((1, n, Cn), device=dev, dtype=torch.float32),
            torch.empty((1, n), device=dev, dtype=torch.float32), torch.empty((1, n), device=dev, dtype=torch.int32))
    n_out = torch.empty((1,), device=dev, dtype=torch.int32)
    scratch = torch.empty((L.ivx_volume_pack_scratch_bytes(1, X, Y, Z) // 4,), device=dev, dtype=torch.int32)
    twin = tuple(torch.empty_like(t) for t in state)
    pack(state, n, outs, n_out, scratch)
    fns = [lambda: pack(state, n, outs, n_out, scratch), lambda: pack(state, 0, (None,) * 4, n_out, scratch), lambda: unpack(twin, n, outs),
           lambda: [t.copy_(q) for t, q in zip(twin, state)], lambda: torch_pack(state), lambda: ops.volume_pack(s._sum, s._count, [0], s._wsum)]
    ta, tb, tc, td, te, tf = many_us(fns, kreps)
    unpack(twin, n, outs)
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(twin, state)), 'the round trip is not exact'
    ref = torch_pack(state)
    assert all(torch.equal(a.view(torch.int32), b.reshape(a.shape).view(torch.int32)) for a, b in zip(ref, outs)), 'the pack differs from the torch form'
    med = statistics.median
    row_mb, rec_mb = nvox * (Cn + 2) * 4 / 1e6, n * (Cn + 3) * 4 / 1e6
    return (f'| {name} | {label} | {n / nvox:.3f} | {row_mb:.1f} | {rec_mb:.1f} | {fmt(ta, 1)} | {fmt(tb, 1)} | {fmt(tc, 1)} | {fmt(td, 1)} | {fmt(te, 1)} | {fmt(tf, 1)} | '
            f'{med(ta) / med(td):.2f} | {med(tc) / med(td):.2f} | {med(ta) / med(te):.2f} |')


def host_row(ia, name, label, s, passes, tmp):
    dense = lambda: [t.cpu() for t in (s._sum, s._wsum, s._count)]     # noqa: E731
    for fn in (s.snapshot, dense):
        fn()
    t_snap, t_bf16, t_dense = [], [], []
    for _ in range(passes):
        t_snap.append(host_ms(s.snapshot))
        t_bf16.append(host_ms(lambda: s.snapshot(torch.bfloat16)))
        t_dense.append(host_ms(dense))
    sizes = []
    for dt in (torch.float32, torch.bfloat16):
        path = os.path.join(tmp, 'snap.npz')
        s.snapshot(dt).save(path)
        sizes.append(os.path.getsize(path) / 1e6)
    path = os.path.join(tmp, 'dense.npz')
    with open(path, 'wb') as f:
        np.savez(f, **{k: t.cpu().numpy() for k, t in zip(('sum', 'wsum', 'count'), (s._sum, s._wsum, s._count))})
    dense_mb = os.path.getsize(path) / 1e6
    os.remove(path)
    return (f'| {name} | {label} | {s.snapshot().seen_fraction:.3f} | {fmt(t_snap)} | {fmt(t_bf16)} | {fmt(t_dense)} | {statistics.median(t_snap) / statistics.median(t_dense):.2f} | '
            f'{sizes[0]:.1f} | {sizes[1]:.1f} | {dense_mb:.1f} |')


def arrivals(ia, name, model, a):
    n = a.arrival_views
    meta, E, img = views_of(ia, name, n)
    alone, snapping = (model.open_scene(meta, decay=0.9) for _ in range(2))
    ts, tm = [], []
    for p in range(a.passes + 1):                                 # pass 0 warms every shape up
        alone.reset()
        snapping.reset()
        for k in range(n):
            t = host_ms(lambda: alone.add_views(img[k:k + 1], E[k:k + 1]).detect())
            u = host_ms(lambda: (snapping.add_views(img[k:k + 1], E[k:k + 1]).snapshot(), snapping.detect()))
            if p:
                ts.append(t)
                tm.append(u)
    for s in (alone, snapping):
        s.close()
    return ts, tm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    ap.add_argument('--kreps', type=int, default=10)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--views', type=int, default=20)
    ap.add_argument('--arrival-views', type=int, default=6)
    ap.add_argument('--workloads', default='scannet_fast,scannet_v1,kitti')
    ap.add_argument('--skip-arrivals', action='store_true')
    ap.add_argument('--bf16-worst', default=NOT, help='the worst measured fraction of the bf16 bound, as the GPU tests printed it')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('scene_snapshot_bench needs a HIP device: nothing is measured without one')
    import imvoxelnet_amd as ia
    k_rows, h_rows, a_rows = [], [], []
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.workloads.split(','):
            try:
                model = make_model(ia, name)
                model.prepare(torch.device('cuda'))
                scenes = scenes_of(ia, name, model, a.views)
                for label, s in scenes.items():
                    k_rows.append(kernel_row(name, label, s, a.kreps))
                    h_rows.append(host_row(ia, name, label, s, a.passes, tmp))
                    print(k_rows[-1], h_rows[-1], sep='\n', flush=True)
                for s in scenes.values():
                    s.close()
                torch.cuda.empty_cache()
                if a.skip_arrivals:
                    a_rows.append(f'| {name} | {NOT} | {NOT} | |')
                else:
                    ts, tm = arrivals(ia, name, model, a)
                    a_rows.append(f'| {name} | {fmt(ts)} | {fmt(tm)} | {statistics.median(tm) - statistics.median(ts):+.2f} ms |')
                    print(a_rows[-1], flush=True)
            except torch.cuda.OutOfMemoryError as exc:
                print(f'{name}: {exc}', flush=True)
                k_rows.append(f'| {name} | {NOT} (out of device memory) |')
            del model
            torch.cuda.empty_cache()
    lines = ['# Scene snapshots: packing the seen voxels of a state against a dense copy and against the torch form', '',
             f'Device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}.  Written by tools/scene_snapshot_bench.py.', '',
             '## (a) - (f) One row of fp32 state: seen fraction, pack, unpack, the dense copy_, the torch form', '',
             f'us per call; HIP events around {BATCH} back-to-back calls, the six forms alternating in one process; median (min .. max) of {a.kreps} batches each.  A figure '
             'holds the kernels of the call, the gaps between them and the host side of the call.  (a) is the bare C pack at cap = n (count, scan, write), (b) its '
             'count-only form, (c) the bare C unpack of those records into a twin row, (d) a device copy_ of the three dense fields into the twin -- the floor when '
             'everything is seen -- (e) nonzero + index_select + three gathers, which syncs the host inside nonzero, (f) ops.volume_pack (count, read n back, allocate, '
             'pack).  `seen` is n / (X*Y*Z); `records MB` is n * (C + 3) * 4 bytes.  Rows of 26 / 54 / 170 MB fit the 256 MB Infinity Cache, so copy rates above the '
             'HBM bandwidth are cache rates, for every form alike.  Each row ends with a check that unpack(pack(row)) == row on the words and that the pack equals (e).', '',
             '| workload | state | seen | row MB | records MB | (a) pack us | (b) count us | (c) unpack us | (d) copy_ us | (e) torch pack us | (f) ops.volume_pack us | (a) / (d) | '
             '(c) / (d) | (a) / (e) |', '|---|---|---|---|---|---|---|---|---|---|---|---|---|---|'] + k_rows
    lines += ['', '## (g) snapshot() end to end against .cpu() of the three dense fields, and the files', '',
              f'ms, host clock around calls that end in a device synchronise, median (min .. max) of {a.passes} passes after one warm call; pageable host memory on both '
              'sides.  snapshot() is one ops.volume_pack, the copy of n records to the host and the host record; the dense form is sum.cpu(), wsum.cpu(), count.cpu().  Files: '
              'SceneSnapshot.save of the F32 and of the bf16 snapshot, and np.savez of the three dense fields, MB on disk (uncompressed).', '',
              '| workload | state | seen | snapshot() ms | snapshot(bf16) ms | dense .cpu() ms | snapshot / dense | F32 file MB | bf16 file MB | dense file MB |',
              '|---|---|---|---|---|---|---|---|---|---|'] + h_rows
    lines += ['', f'## (h) One arrival + detect() with and without a snapshot (arrivals 1 .. {a.arrival_views}, decay=0.9, fp32 storage)', '',
              'ms, host clock around add_views(1 view) [+ snapshot()] + detect(), which ends in the detections\' device-to-host copy; the two sessions alternate arrival by '
              f'arrival in one process; one warm pass, then median (min .. max) over {a.passes} passes.  The session without a snapshot runs the parent commit\'s code.', '',
              '| workload | add_views + detect() | add_views + snapshot() + detect() | difference of the medians |', '|---|---|---|---|'] + a_rows
    lines += ['', '## bf16 payload: worst measured fraction of the bound', '',
              f'|S\' - S| / ((2^-8 + 2^-22) |S|) over the bf16 cases of tests/test_gpu_volume_pack.py and tests/test_gpu_scene_snapshot.py on the MI355X: {a.bf16_worst}.']
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
