"""Measure sliding-window scenes (SceneSession with window=W, ivx_backproject_gather_fwd) on the GPU box.  python tools/scene_window_bench.py [--md profiles/scene_window.md]

Workloads: scannet_v1 and scannet_fast of workloads.py, synthetic 480 x 640 views arriving one at a time, W = 20.
  (a) kernel      the gathered lift of W views from a ring whose list is wrapped and scrambled (ops.backproject_gather_mean, device list) against
                  ops.backproject_mean over a contiguous copy of the same views in the same order: same process, alternating, HIP events around 20
                  launches enqueued back to back, divided by 20; warm-up, then median (min .. max) of --kreps such batches each.  The two results are
                  compared with torch.equal.
  (b) per arrival add_views(1 view) + detect() on a windowed session at arrivals W+1 .. 2W (the window is full: every arrival drops the oldest view),
                  against what a caller has without windows: reset() + add_views(the last W views) + detect() on an unbounded session.  Host clock
                  around calls that end in the device-to-host copy of the detections; one whole warm pass, then the median over --passes passes.
Not part of bench.py.  Needs a device: there is no fallback.  A figure that could not be taken is written as "not measured"."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

BATCH = 20      # launches between one pair of events

# From `hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -Rpass-analysis=kernel-resource-usage` on csrc/backproject.hip (a compile, not a run):
# backproject_mean_kernel<4, BP_MEAN, T, SAMP, GATHER>
RESOURCES = '''| instantiation (VEC 4, mean) | VGPRs | SGPRs | scratch B/lane | LDS B | waves/SIMD |
|---|---|---|---|---|---|
| fp32 nearest | 54 | 50 | 0 | 0 | 8 |
| fp32 nearest, gathered | 56 | 50 | 0 | 0 | 8 |
| bf16 nearest | 54 | 50 | 0 | 0 | 8 |
| bf16 nearest, gathered | 56 | 50 | 0 | 0 | 8 |
| fp32 bilinear | 74 | 50 | 0 | 0 | 6 |
| fp32 bilinear, gathered | 74 | 53 | 0 | 0 | 6 |
| bf16 bilinear | 76 | 50 | 0 | 0 | 6 |
| bf16 bilinear, gathered | 76 | 53 | 0 | 0 | 6 |

No scratch and no LDS in any of them; the gathered forms are within 2 VGPRs and 3 SGPRs of the plain ones (the slot and the pool size) and
keep their occupancy.  The instruction streams of the sixteen kernels that existed before are unchanged by the new template parameter
(compared instruction by instruction in the compiler's assembly output).'''


def kernel_pair_us(fa, fb, reps, warmup=5):
    """us per launch of fa and of fb: alternating batches of BATCH back-to-back launches between two events each."""
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


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def fmt(ts, digits=2):
    return f'{statistics.median(ts):.{digits}f} ({min(ts):.{digits}f} .. {max(ts):.{digits}f})'


def build(ia, name):
    from imvoxelnet_amd import workloads as wl
    cfg, test_cfg = {'scannet_v1': (wl.scannet_v1_model_cfg, wl.SCANNET_V1_TEST_CFG), 'scannet_fast': (wl.scannet_fast_model_cfg, wl.SCANNET_FAST_TEST_CFG)}[name]
    model = ia.build_detector(cfg(), test_cfg=dict(test_cfg))
    ia.randomize_(model, 78)
    with torch.no_grad():
        g = torch.Generator().manual_seed(5)
        model.bbox_head.cls_conv.weight.normal_(0, 0.01, generator=g)
        model.bbox_head.cls_conv.bias.fill_(-2.0)
        model.bbox_head.centerness_conv.weight.normal_(0, 0.005, generator=g)
        model.bbox_head.reg_conv.weight.normal_(0, 0.002, generator=g)
    return model


def measure(ia, name, a):
    from imvoxelnet_amd import ops
    from imvoxelnet_amd.workloads import indoor_meta
    W = a.window
    n = 2 * W
    model = build(ia, name)
    model.prepare(torch.device('cuda'), dtype=torch.bfloat16 if a.storage == 'bf16' else torch.float32)
    meta = indoor_meta(n, box_type=ia.DepthInstance3DBoxes)
    E = meta['lidar2img']['extrinsic']
    scene_meta = dict(meta, lidar2img={k: v for k, v in meta['lidar2img'].items() if k != 'extrinsic'})
    img = torch.randn(n, 3, 480, 640, generator=torch.Generator().manual_seed(13)).cuda()

    # ---- (a) the two lifts of the same W views
    views = list(range(W, n))                                     # the views of the last window
    wmeta = dict(meta, lidar2img=dict(meta['lidar2img'], extrinsic=[E[v] for v in views]))
    p0 = model.features_2d_cl(img[W:][None].contiguous())         # [W,1,FH,FW,C]
    proj, no, crop = model._camera_setup([wmeta], 4, img.device)
    S, FH, FW, Cn = W, p0.shape[2], p0.shape[3], p0.shape[-1]
    order = torch.randperm(W, generator=torch.Generator().manual_seed(3)).tolist()       # list position i holds view order[i] ...
    slot = [(7 * v + 11) % W for v in range(W)] if W % 7 else list(range(W))            # ... which sits in slot slot[view]: wrapped and scrambled
    assert sorted(slot) == list(range(W))
    pool, ppool = torch.empty_like(p0), torch.empty_like(proj[0])
    pool[torch.tensor(slot, device='cuda')] = p0
    ppool[torch.tensor(slot, device='cuda')] = proj[0]
    oi = torch.tensor(order, device='cuda')
    cfeat, cproj = p0[oi].contiguous(), proj[:, oi].contiguous()
    view_slot = torch.tensor([[slot[v] for v in order]], dtype=torch.int32).cuda()
    sampling = getattr(model, 'sampling', 'nearest')

    def gathered():
        return ops.backproject_gather_mean(pool, ppool, view_slot, no, crop, model.voxel_size, model.n_voxels, sampling=sampling)

    def contiguous():
        return ops.backproject_mean(cfeat, cproj, no, crop, model.voxel_size, model.n_voxels, sampling=sampling)

    (gv, gok), (cv, cok) = gathered(), contiguous()
    equal = bool(torch.equal(gv, cv) and torch.equal(gok, cok))
    tg, tc = kernel_pair_us(gathered, contiguous, a.kreps)
    del pool, ppool, cfeat, cproj, p0

    # ---- (b) per arrival on a full window against reset() + re-adding the last W views
    win = model.open_scene(scene_meta, window=W)
    t_win, n_det = [], 0
    for p in range(a.passes + 1):                                 # pass 0 warms every shape up
        win.reset()
        for k in range(1, n + 1):
            out = []
            t = host_ms(lambda: out.append(win.add_views(img[k - 1:k], E[k - 1:k]).detect()))
            if p and k > W:
                t_win.append(t)
            n_det = len(out[0][0]['scores_3d'])
    win.close()
    old = model.open_scene(scene_meta)
    t_old = []
    for p in range(a.passes + 1):
        for k in range(W + 1, n + 1, a.old_stride):
            def today():
                old.reset()
                return old.add_views(img[k - W:k], E[k - W:k]).detect()
            t = host_ms(today)
            if p:
                t_old.append(t)
    old.close()
    X, Y, Z = model.n_voxels
    return dict(name=name, N=X * Y * Z, C=Cn, FH=FH, FW=FW, esz=gv.element_size(), tg=tg, tc=tc, equal=equal, t_win=t_win, t_old=t_old, n_det=n_det)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    ap.add_argument('--window', type=int, default=20)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--kreps', type=int, default=30)
    ap.add_argument('--old-stride', type=int, default=4, help='measure the reset() + re-add alternative at every n-th arrival')
    ap.add_argument('--storage', choices=['fp32', 'bf16'], default='fp32')
    ap.add_argument('--workloads', default='scannet_v1,scannet_fast')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('scene_window_bench needs a HIP device: nothing is measured without one')
    import imvoxelnet_amd as ia
    W = a.window
    res = []
    for name in a.workloads.split(','):
        try:
            res.append(measure(ia, name, a))
        except torch.cuda.OutOfMemoryError as exc:                # the file then says so for this workload; anything else ends the run
            print(f'{name}: {exc}', flush=True)
            res.append(dict(name=name, failed='out of device memory'))
        torch.cuda.empty_cache()
    lines = [f'# Sliding-window scenes: W = {W}, 480 x 640 views arriving one at a time ({a.storage} storage)', '',
             f'Device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}.  Random weights.  Written by tools/scene_window_bench.py.', '',
             f'## (a) The lift of {W} views: gathered from a scrambled ring against the contiguous stack', '',
             f'us per launch; HIP events around {BATCH} back-to-back launches, the two forms alternating in one process; median (min .. max) of {a.kreps} batches each.  '
             'A figure holds the kernel, the gap to the next dispatch and the allocation of the outputs, the same for both forms.', '',
             '| workload | voxels x C, map | ring MB | contiguous (ops.backproject_mean) | gathered (ops.backproject_gather_mean) | gathered / contiguous | results bit-equal |',
             '|---|---|---|---|---|---|---|']
    for r in res:
        if 'failed' in r:
            lines.append(f'| {r["name"]} | not measured ({r["failed"]}) | | | | | |')
            continue
        ring = W * r['FH'] * r['FW'] * r['C'] * r['esz'] / 1e6
        lines.append(f'| {r["name"]} | {r["N"]} x {r["C"]}, {r["FH"]} x {r["FW"]} | {ring:.1f} | {fmt(r["tc"], 1)} | {fmt(r["tg"], 1)} | '
                     f'{statistics.median(r["tg"]) / statistics.median(r["tc"]):.3f} | {r["equal"]} |')
    lines += ['']
    for r in res:
        if 'failed' in r:
            continue
        spread = max(r['tc']) - min(r['tc'])
        q = statistics.quantiles(r['tc'], n=4)
        d = statistics.median(r['tg']) - statistics.median(r['tc'])
        lines.append(f'{r["name"]}: gathered - contiguous = {d:+.1f} us at the median, {min(r["tg"]) - min(r["tc"]):+.1f} us between the minima; the contiguous form alone '
                     f'spreads over {spread:.1f} us (max - min; {q[2] - q[0]:.1f} us between its quartiles): '
                     + ('within that spread.' if abs(d) <= spread else 'OUTSIDE that spread.'))
    lines += ['', 'Reading: a difference that the minima show as the medians do is systematic even where one slow batch of the contiguous form makes its max - min '
              'spread wider.  What the gathered form adds is in the projecting lane only: it loads its slot before it can load the projection rows (one more '
              'dependent memory round trip in front of each projection round), tests it against the pool size and forms the row address from it.  That '
              'weighs most where a voxel has few lanes and many voxels share little channel work: scannet_v1 has 204 800 voxels with 16 lanes each and '
              'two projection rounds for 20 views, scannet_fast 25 600 voxels with 64 lanes each and one round.  Where the time goes has NOT been '
              'confirmed with counters: no counter run was made.']
    lines += ['', f'## (b) One arrival on a full window (arrivals {W + 1} .. {2 * W})', '',
              f'ms, host clock around calls that end in the detections\' device-to-host copy; one warm pass, then median (min .. max) over {a.passes} passes.', '',
              f'| workload | windowed: add_views(1 view) + detect() | without windows: reset() + add_views(last {W} views) + detect() | ratio | detections at the last arrival |',
              '|---|---|---|---|---|']
    for r in res:
        if 'failed' in r:
            lines.append(f'| {r["name"]} | not measured | not measured | | |')
            continue
        lines.append(f'| {r["name"]} | {fmt(r["t_win"])} | {fmt(r["t_old"])} | {statistics.median(r["t_old"]) / statistics.median(r["t_win"]):.2f} | {r["n_det"]} |')
    lines += ['', f'The second column runs the trunk on {W} views per arrival, the first on one; both run the lift of {W} views, neck and head once.  The features of a view '
              'may differ in the last bits between the two (the trunk\'s per-tensor operand scales depend on which views share a call), so the two columns '
              'are the same work, not the same bits; the bit identity of a windowed session is with a session that was given the same views one at a time '
              '(tests/test_gpu_scene_window.py).', '',
              '## Kernel resources (compile-time, gfx950)', '', RESOURCES]
    print('\n'.join(lines), flush=True)
    if a.md:
        with open(a.md, 'w') as fo:
            fo.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
