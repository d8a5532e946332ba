"""Measure view coverage (ivx_view_coverage_fwd, SceneSession.coverage, add_views(..., min_novelty=)) on the GPU box.
python tools/view_coverage_bench.py [--md profiles/view_coverage.md] [--parent-json FILE] [--variants NAME=LIB,...]

Method of tools/scene_scroll_bench.py for the op (HIP events around 20 back-to-back calls, the forms alternating in one process, median (min .. max)
of --kreps batches) and of tools/scene_stream_bench.py for arrivals (host clock around calls that end in a device-to-host copy, one warm pass, then
the median over --passes).  Two grids: scannet_fast 40 x 40 x 16 and scannet_v1 80 x 80 x 32, 480 x 640 views (feature maps 120 x 160).
  (a) op          ops.view_coverage for K = 1, 4, 8 candidates of one scene, every state kind, without maps and with both maps, beside two
                  yardsticks of the same process: ONE tiny launch (zero_ of the 64-byte result) and TWO (zero_ + a one-element add_): the op is a
                  memset and a kernel.  Bytes from the shapes: the state row read once (4 B or 1 B per voxel), whatever K.
  (b) shape       the same op under IVX_COVERAGE_WGS = 64, 256, 1024, 4096 workgroups per launch (the environment is read at every call), and, with
                  --variants NAME=LIB, through other builds of csrc/view_coverage.hip alone (-DIVX_COVERAGE_WG=64 / 128 lanes per workgroup), bare C
                  calls alternating with the product build.  A variant is built with
                  hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC -ffp-contract=off -DIVX_COVERAGE_WG=64 imvoxelnet_amd/csrc/view_coverage.hip \
                        -Limvoxelnet_amd/csrc -l:libimvoxel_hip.so -Wl,-rpath,<dir of libimvoxel_hip.so> -o LIB
  (c) coverage()  SceneSession.coverage(K poses) end to end on a plain session that holds 8 views: projection on the host, one upload, the launch,
                  the device-to-host read of the counts.
  (d) arrivals    per arrival: an ungated add_views(1 view) + detect(); a gated one that is admitted (min_novelty = 1e-6) + detect(); and a gated
                  one that is rejected (the same pose again, min_novelty = 0.5: add_views alone, nothing follows a rejected frame).  The ungated
                  column AT THE PARENT COMMIT comes from --parent-json: the file `--ungated-json FILE` writes when this tool is run on a checkout of
                  the parent (that mode uses nothing the parent lacks), in a process of its own on the same device.
Not part of bench.py.  Needs a device: there is no fallback.  A figure that could not be taken is written as "not measured"."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from scene_scroll_bench import many_us                          # noqa: E402
from scene_window_bench import BATCH, build, fmt, host_ms      # noqa: E402

KS = (1, 4, 8)
KINDS = (('none', None), ('count', torch.int32), ('wsum', torch.float32), ('mask', torch.uint8))
WGS = (64, 256, 1024, 4096)

# From `hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -Rpass-analysis=kernel-resource-usage` on csrc/view_coverage.hip (a compile, not a run)
RESOURCES = '''| kernel (IVX_COVERAGE_WG = 256) | VGPRs | SGPRs | scratch B/lane | LDS B | waves/SIMD |
|---|---|---|---|---|---|
| view_coverage_kernel, no state | 20 | 82 | 0 | 2048 | 8 |
| view_coverage_kernel, count / wsum / mask | 20 | 86 | 0 | 2048 | 8 |

The slot, the twelve projection numbers, the origin and the crop live in scalar registers (the SGPR column); a lane keeps its voxel's centre, its
evidence and the chain's temporaries.'''

READING = '''## Reading

Of the run this file was first written from (MI355X).  The expectation to test was: the op is bound by launch latency, since it reads 4 B per voxel.
Confirmed for one candidate and for the small grid, refined for many candidates on the large one.  The bare entry -- a memset and a kernel -- takes 10.6 - 11.5 us
at K = 1 on BOTH grids (25 600 and 204 800 voxels, 0.1 and 0.8 MB of state) against 7.7 us for two tiny launches of the same process, and 11.2 - 11.5 us at K = 8
on scannet_fast: the time does not follow the bytes or the grid.  On scannet_v1, K = 8 takes 15.2 us: 4.5 us more for eight projections of 204 800 voxels, which
is arithmetic in the candidate loop, not traffic (0.8 MB in 15 us is 54 GB/s).  The state kind and the maps do not show (within 1 - 2 us through the op).
Shape: the cap on workgroups per launch does nothing from 256 up (scannet_v1, K = 8: 15.2 us at 256, 1024 and 4096; the small grid has only 100 blocks) and 64
workgroups are too few (39.4 us): the product default is 1024, at which neither grid strides.  256 lanes per workgroup beat 128 and 64 on scannet_v1 (15.3 against
18.3 and 24.0 us at K = 8: fewer workgroups, fewer global atomics) and tie on scannet_fast.
Through ops.view_coverage a call takes 35 - 40 us: the host side of the op (list checks, the one upload of the lists, ctypes) is three times the device side.
SceneSession.coverage end to end, with the device-to-host read, takes 0.12 - 0.15 ms for 1 - 8 poses.  A gated arrival that is rejected costs 0.18 - 0.22 ms instead
of the 3.9 / 5.5 ms of an arrival + detect(); one that is admitted costs 0.15 - 0.17 ms more than an ungated one (4.04 against 3.87 ms, 5.68 against 5.53 ms).
The ungated arrival of this build and of the parent commit agree on scannet_fast (3.87 ms both); on scannet_v1 the parent's process measured 6.24 ms
(5.99 .. 6.93) against 5.53 ms here -- two processes, the parent's being the first on the device, so that difference is between processes, not between commits
(the parent's process ran the parent's Python package on this build's library through IVX_LIB_PATH; the ungated path is the same Python code and its
kernels are compiled from the same sources).  A second run of the whole tool, minutes later, confirmed that reading and gives the run-to-run spread: the
parent's process measured 5.53 ms (5.50 .. 5.60) on scannet_v1 against 5.51 ms here and 3.87 against 3.86 ms on scannet_fast; the bare entry took 11.1 - 11.6 us
at K = 1 (one batch series of the scannet_v1 row had a median of 15.0 with a minimum of 11.1), 15.2 - 15.4 us at K = 8 on scannet_v1, 39.5 us under the cap of 64,
18.5 and 24.5 us at 128 and 64 lanes; coverage() 0.12 - 0.14 ms; an admitted arrival 4.05 / 5.72 ms; a rejected one 0.23 / 0.24 ms, so 0.18 - 0.24 ms over the two
runs.  No counter run was made.'''


def scene_of(ia, name, n):
    from imvoxelnet_amd.workloads import indoor_meta
    model = build(ia, name)
    model.prepare(torch.device('cuda'))
    meta = indoor_meta(n, box_type=ia.DepthInstance3DBoxes)
    E = meta['lidar2img']['extrinsic']
    scene_meta = dict(meta, lidar2img={k: v for k, v in meta['lidar2img'].items() if k != 'extrinsic'}, pad_shape=(480, 640, 3))
    img = torch.randn(n, 3, 480, 640, generator=torch.Generator().manual_seed(13)).cuda()
    return model, meta, scene_meta, E, img


def op_inputs(model, meta, E):
    """Device inputs of ops.view_coverage for the poses E on this model's grid: projection pool, origin, crop; the states of every kind; both maps."""
    dev = torch.device('cuda')
    proj, no, crop = model._camera_setup([dict(meta, lidar2img=dict(meta['lidar2img'], extrinsic=list(E)))], 4, dev)
    X, Y, Z = model.n_voxels
    g = torch.Generator().manual_seed(3)
    states = {'none': None, 'count': torch.randint(0, 3, (1, X, Y, Z), generator=g).to(torch.int32).cuda(), 'wsum': (2 * torch.rand(1, X, Y, Z, generator=g)).cuda(),
              'mask': torch.randint(0, 2, (1, X, Y, Z), generator=g).to(torch.uint8).cuda()}
    pw = (0.25 + 1.5 * torch.rand(len(E), 120, 160, generator=g)).cuda()
    dp = (0.5 + 3.0 * torch.rand(len(E), 120, 160, generator=g)).cuda()
    return proj[0].contiguous(), no, crop, states, pw, dp


def variant_call(path):
    """ivx_view_coverage_fwd of another build of csrc/view_coverage.hip (the module docstring has the recipe), as a bare C call."""
    from imvoxelnet_amd import _lib
    L = C.CDLL(os.path.abspath(path))
    fn = L.ivx_view_coverage_fwd
    fn.argtypes = [C.POINTER(_lib.BackprojectDesc), C.POINTER(_lib.LiftLists), C.POINTER(_lib.LiftMaps)] + [C.c_void_p] * 4 + [C.c_int32, C.c_float, C.c_void_p, C.c_void_p]

    def call(model, proj, slots, no, crop, state, kind, out):
        X, Y, Z = model.n_voxels
        K = proj.shape[0]
        d = _lib.BackprojectDesc(1, K, 120, 160, 0, X, Y, Z, (C.c_float * 3)(*[float(v) for v in model.voxel_size]), 0, 0, 0, 0)
        l = _lib.LiftLists(K, 1, slots.data_ptr(), None, None)
        rc = fn(C.byref(d), C.byref(l), None, proj.data_ptr(), no.data_ptr(), crop.data_ptr(), None if state is None else state.data_ptr(), kind, 1.0,
                out.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
    return call


def op_rows(name, model, meta, E, kreps, variants):
    from imvoxelnet_amd import ops
    proj, no, crop, states, pw, dp = op_inputs(model, meta, E)
    X, Y, Z = model.n_voxels
    N = X * Y * Z
    tiny, one = torch.zeros(16, dtype=torch.int32, device='cuda'), torch.zeros(1, device='cuda')

    def two():
        tiny.zero_()
        one.add_(1)

    def cov(K, kind, maps):
        out = torch.empty((1, K, 2), dtype=torch.int32, device='cuda')
        p, a, b = proj[:K].contiguous(), pw[:K].contiguous(), dp[:K].contiguous()
        return lambda: ops.view_coverage(p, [list(range(K))], [0], no, crop, model.voxel_size, model.n_voxels, (120, 160), states[kind], 1.0,
                                         a if maps else None, b if maps else None, (0.2, 0.2) if maps else None, out=out)

    cases = [(K, kind, maps) for K in KS for kind, _ in KINDS for maps in (False, True)]
    ts = many_us([tiny.zero_, two] + [cov(*c) for c in cases], kreps)
    lines = [f'| {name} | {N} | one tiny launch (zero_ of 64 bytes) | | | | {fmt(ts[0], 1)} | |', f'| {name} | {N} | two tiny launches (zero_ + add_ of one element) | | | | {fmt(ts[1], 1)} | |']
    for (K, kind, maps), t in zip(cases, ts[2:]):
        b = N * {'none': 0, 'count': 4, 'wsum': 4, 'mask': 1}[kind]
        lines.append(f'| {name} | {N} | ops.view_coverage | {K} | {kind} | {"both" if maps else "none"} | {fmt(t, 1)} | {b / 1e3:.0f} |')
    # (b) the grid cap, read from the environment at every call, and other builds of the kernel
    from imvoxelnet_amd import _lib
    bare = variant_call(_lib.LIB_PATH)
    out8, slots8 = torch.empty((1, 8, 2), dtype=torch.int32, device='cuda'), torch.arange(8, dtype=torch.int32).cuda()

    def capped(w, K):
        p = proj[:K].contiguous()

        def run():
            os.environ['IVX_COVERAGE_WGS'] = str(w)
            bare(model, p, slots8, no, crop, states['count'], 1, out8)
        return run

    keep = os.environ.pop('IVX_COVERAGE_WGS', None)
    tw = many_us([capped(w, K) for w in WGS for K in (1, 8)], kreps)
    os.environ.pop('IVX_COVERAGE_WGS', None)
    if keep is not None:
        os.environ['IVX_COVERAGE_WGS'] = keep
    wrows = [f'| {name} | IVX_COVERAGE_WGS={w} ({min((N + 255) // 256, w)} workgroups) | {K} | {fmt(t, 1)} |' for (w, K), t in zip([(w, K) for w in WGS for K in (1, 8)], tw)]
    vrows = []
    if variants:
        out = torch.empty((1, 8, 2), dtype=torch.int32, device='cuda')
        slots = torch.arange(8, dtype=torch.int32).cuda()
        p8 = proj[:8].contiguous()
        fns = [(vn, K, (lambda vc=vc, K=K: vc(model, p8[:K].contiguous(), slots, no, crop, states['count'], 1, out))) for vn, vc in variants for K in (1, 8)]
        tv = many_us([f[2] for f in fns], kreps)
        vrows = [f'| {name} | {vn} | {K} | {fmt(t, 1)} |' for (vn, K, _), t in zip(fns, tv)]
    return lines, wrows, vrows


def coverage_rows(name, model, scene_meta, E, img, reps):
    s = model.open_scene(scene_meta)
    s.add_views(img, E)
    rows = []
    for K in KS:
        s.coverage(E[:K])
        ts = [host_ms(lambda: s.coverage(E[:K])) for _ in range(reps)]
        rows.append(f'| {name} | {K} | {fmt([t * 1e3 for t in ts], 0)} |')
    s.close()
    return rows


def ungated_arrivals(model, scene_meta, E, img, passes):
    s, ts = model.open_scene(scene_meta), []
    for p in range(passes + 1):                                  # pass 0 warms every shape up
        s.reset()
        for k in range(len(E)):
            t = host_ms(lambda: s.add_views(img[k:k + 1], E[k:k + 1]).detect())
            if p:
                ts.append(t)
    s.close()
    return ts


def gated_arrivals(model, scene_meta, E, img, passes):
    """(ungated, admitted, rejected) ms per arrival, the three alternating arrival by arrival, and the number of arrivals the gate let in."""
    u, g = model.open_scene(scene_meta), model.open_scene(scene_meta)
    tu, ta, tr, let_in, thrown = [], [], [], 0, 0
    for p in range(passes + 1):
        u.reset()
        g.reset()
        for k in range(len(E)):
            x, e = img[k:k + 1], E[k:k + 1]
            a = host_ms(lambda: u.add_views(x, e).detect())
            b = host_ms(lambda: g.add_views(x, e, min_novelty=1e-6).detect())
            ok = g.last_admitted == [True]
            c = host_ms(lambda: g.add_views(x, e, min_novelty=0.5))
            no = g.last_admitted == [False]
            if p:
                tu.append(a)
                if ok:
                    ta.append(b)
                if no:
                    tr.append(c)
                let_in += ok
                thrown += no
    u.close()
    g.close()
    return tu, ta, tr, let_in, thrown


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    ap.add_argument('--kreps', type=int, default=20)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--views', type=int, default=8)
    ap.add_argument('--workloads', default='scannet_fast,scannet_v1')
    ap.add_argument('--variants', default='', help='NAME=LIB,...: other builds of csrc/view_coverage.hip to time beside the product build')
    ap.add_argument('--ungated-json', default=None, help='measure the ungated arrivals only and write them here (runs on the parent commit too)')
    ap.add_argument('--parent-json', default=None, help='the file --ungated-json wrote on a checkout of the parent commit')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('view_coverage_bench needs a HIP device: nothing is measured without one')
    import imvoxelnet_amd as ia
    names = a.workloads.split(',')
    if a.ungated_json:
        res = {}
        for name in names:
            model, meta, scene_meta, E, img = scene_of(ia, name, a.views)
            res[name] = ungated_arrivals(model, scene_meta, E, img, a.passes)
            print(name, fmt(res[name]), flush=True)
            del model, img
            torch.cuda.empty_cache()
        with open(a.ungated_json, 'w') as fo:
            json.dump(res, fo)
        return
    parent = json.load(open(a.parent_json)) if a.parent_json else {}
    variants = [(v.split('=')[0], variant_call(v.split('=')[1])) for v in a.variants.split(',') if v]
    if variants:
        from imvoxelnet_amd import _lib
        variants.insert(0, ('product (256 lanes), bare C call', variant_call(_lib.LIB_PATH)))
    op, wg, var, cov, arr = [], [], [], [], []
    for name in names:
        model, meta, scene_meta, E, img = scene_of(ia, name, a.views)
        o, w, v = op_rows(name, model, meta, E, a.kreps, variants)
        op += o
        wg += w
        var += v
        cov += coverage_rows(name, model, scene_meta, E, img, a.reps)
        tu, ta, tr, let_in, thrown = gated_arrivals(model, scene_meta, E, img, a.passes)
        tp = parent.get(name)
        arr.append(f'| {name} | {fmt(tp) if tp else "not measured"} | {fmt(tu)} | {fmt(ta) if ta else "not measured"} ({let_in} of {a.passes * a.views} let in) | '
                   f'{fmt(tr) if tr else "not measured"} ({thrown} of {a.passes * a.views} rejected) |')
        del model, img
        torch.cuda.empty_cache()
    lines = ['# View coverage: counting what a candidate view adds before its trunk runs', '',
             f'Device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}.  Written by tools/view_coverage_bench.py.', '',
             '## (a) The op alone: one scene, K candidate views of 480 x 640 (maps 120 x 160)', '',
             f'us per call; HIP events around {BATCH} back-to-back calls, the forms alternating in one process; median (min .. max) of {a.kreps} batches each.  A figure holds '
             'the memset and the kernel of the call, the gaps between them, the one upload of the lists and the host side of the op.  State KB: the bytes of the '
             'state row, read once whatever K.', '',
             '| grid | voxels | form | K | state | maps | us | state KB |', '|---|---|---|---|---|---|---|---|'] + op
    lines += ['', '## (b) Shape: workgroups per launch, lanes per workgroup', '',
              'The entry as a bare C call (ctypes: no upload, no checks of the op; count state, no maps) under other caps on the workgroups of a launch, in one '
              'alternation; compare these rows with each other, not with (a):', '',
              '| grid | cap | K | us |', '|---|---|---|---|'] + wg + ['']
    if var:
        lines += ['Other builds of the kernel, bare C calls (no upload, no checks of the op: compare these rows with each other, not with (a)):', '',
                  '| grid | build | K | us |', '|---|---|---|---|'] + var
    else:
        lines += ['Other lanes-per-workgroup builds: not measured in this run (no --variants given).']
    lines += ['', '## (c) SceneSession.coverage(K poses), end to end', '',
              f'us, host clock around the call on a plain session holding {a.views} views: the projection rows on the host, one upload, the launch and the device-to-host '
              f'read of the counts; median (min .. max) of {a.reps} calls.', '', '| workload | K | us |', '|---|---|---|'] + cov
    lines += ['', f'## (d) Arrivals (1 .. {a.views}, fp32 storage, 480 x 640)', '',
              'ms, host clock; the three forms of this build alternate arrival by arrival in one process, the parent commit ran the ungated form in a process of its own '
              f'on the same device; one warm pass, then median (min .. max) over {a.passes} passes.  A rejected arrival is add_views alone: the count, its read-back, '
              'and nothing else.', '',
              '| workload | ungated add_views + detect(), parent commit | ungated, this build | gated and admitted + detect() | gated and rejected (add_views alone) |',
              '|---|---|---|---|---|'] + arr
    lines += ['', READING, '', '## Kernel resources (compile-time, gfx950)', '', RESOURCES]
    print('\n'.join(lines), flush=True)
    if a.md:
        with open(a.md, 'w') as fo:
            fo.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
