"""Measure the image pipeline on decoder pixel formats (ivx_image_prep_fmt_u8, csrc/image_prep.hip, csrc/pixel_fetch.h) beside the unchanged BGR entries
(ivx_image_prep_u8 / ivx_image_prep_lens_u8) on the GPU box.  python tools/image_prep_fmt_bench.py [--md out.md]

Per geometry (KITTI 375 x 1242 -> 384 x 1280, ScanNet 968 x 1296 -> 480 x 640, a 1080 x 1920 decoder frame -> the ScanNet input), plain and
through a Brown lens, in ONE process with all candidates taking turns in a shuffled order (the clock of tools/image_prep_lens_bench.py: HIP
events around --batch back-to-back launches, warm-up first, median; min .. max of --reps windows, per launch):
  BGR entry      ivx_image_prep_u8 / ivx_image_prep_lens_u8 on packed BGR frames of the same size: the yardstick.  Since 0.5.3 these entries
                 launch the BGR8 instantiation of the templated kernels, so on this tree `BGR entry` and `fmt bgr` time the same kernel
                 (section B of profiles/image_prep_fmt.md).  Section A of that profile, on which the reuse decision of DESIGN.md rests,
                 was taken with this tool while the entries still launched the 0.5.2 kernels and CANNOT be reproduced from this tree;
  fmt <layout>   ivx_image_prep_fmt_u8 on the layout's usual array (the stacked NV12 array, [n,H,W,2] YUYV, [n,H,W,4], [n,H,W] gray);
  two-pass       what a caller does without the entry: NV12 -> BGR written in torch (integer rule, same bytes), then the BGR entry.
bytes: source bytes + output bytes, the bytes the algorithm needs; the rate is bytes / time.  The outputs of all candidates are checked
to be equal before anything is timed.  Not part of bench.py.  Needs a device: there is no fallback."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

GEOMETRIES = [('KITTI', (375, 1242), (1280, 384), 4), ('ScanNet', (968, 1296), (640, 480), 8), ('1080p', (1080, 1920), (640, 480), 8)]
LAYOUTS = ('bgr', 'rgb', 'bgra', 'rgba', 'gray', 'nv12', 'yuyv')


def torch_nv12_to_bgr(st, H, W, m):
    """The header's integer rule in torch ops on a stacked NV12 batch [n, H + ceil(H/2), W] -> [n,H,W,3] uint8 (a handful of launches and
    several full-size int32 intermediates: what a caller writes without a kernel of their own)."""
    y_off, cy, cub, cug, cvg, cvr = m
    n = st.shape[0]
    Y = st[:, :H].to(torch.int32)
    uv = st[:, H:].reshape(n, -1, W // 2, 2).to(torch.int32) - 128
    uv = uv.repeat_interleave(2, dim=1)[:, :H].repeat_interleave(2, dim=2)
    u, v = uv[..., 0], uv[..., 1]
    yy = (Y - y_off).clamp_(min=0) * cy + (1 << 19)
    bgr = torch.stack([(yy + cub * u) >> 20, (yy + cvg * v + cug * u) >> 20, (yy + cvr * v) >> 20], dim=3)
    return bgr.clamp_(0, 255).to(torch.uint8)


def shuffled_windows_us(fns, reps, batch, warmup=3):
    """windows_us of tools/image_prep_lens_bench.py with the order of the candidates shuffled (seeded) every round: a candidate that reads the
    buffer its predecessor has just read finds it in the Infinity Cache, and one that follows the two-pass candidate finds the cache full of
    torch's intermediates; a window of `batch` launches bounds that bias by 1 / batch of a cold pass, the shuffle spreads the rest evenly.
    -> {name: (median, min, max)}."""
    import random
    import statistics
    names, rnd = list(fns), random.Random(0)
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in names}
    for r in range(reps):
        for k in rnd.sample(names, len(names)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(batch):
                fns[k]()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1e3 / batch)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def source(layout, n, h, w, rng):
    shape = {'bgr': (n, h, w, 3), 'rgb': (n, h, w, 3), 'bgra': (n, h, w, 4), 'rgba': (n, h, w, 4), 'gray': (n, h, w), 'nv12': (n, h + (h + 1) // 2, w),
             'yuyv': (n, h, w, 2)}[layout]
    return torch.from_numpy(rng.randint(0, 256, shape).astype(np.uint8)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--batch', type=int, default=20)
    a = ap.parse_args()
    assert a.reps >= 20 and a.batch >= 1
    if not torch.cuda.is_available():
        raise SystemExit('image_prep_fmt_bench needs a HIP device: nothing is measured without one')
    from image_prep_lens_bench import lenses
    from imvoxelnet_amd import data, ops
    cfg = data.IMG_NORM_CFG
    mean, std = cfg['mean'], cfg['std']
    m = data.FrameFormat('nv12').matrix
    cell = lambda t: f'{t[0]:.1f} ({t[1]:.1f} .. {t[2]:.1f})'                     # noqa: E731
    lines = []
    for name, (h, w), scale, n in GEOMETRIES:
        (nh, nw), (ph, pw) = data._pipeline_shapes((h, w), scale, 32, True)
        rng = np.random.RandomState(1)
        srcs = {l: source(l, n, h, w, rng) for l in LAYOUTS}
        outs = {k: torch.empty(n, 3, ph, pw, device='cuda') for k in ('a', 'b')}
        brown = lenses((h, w))['Brown']
        for lens_name, lens in (('plain', None), ('Brown lens', brown)):
            def bgr_entry(src, out):
                if lens is None:
                    return ops.image_prep_u8(src, (nh, nw), (ph, pw), mean, std, True, out=out)
                return ops.image_prep_lens_u8(src, lens, (nh, nw), (ph, pw), mean, std, True, out=out)

            def fmt_entry(l, out):
                return ops.image_prep_fmt_u8(srcs[l], l, (nh, nw), (ph, pw), mean, std, True, lens=lens, out=out)
            # the candidates agree before they are timed
            assert torch.equal(fmt_entry('bgr', outs['a']), bgr_entry(srcs['bgr'], outs['b']))
            assert torch.equal(fmt_entry('nv12', outs['a']), bgr_entry(torch_nv12_to_bgr(srcs['nv12'], h, w, m), outs['b']))
            fns = {'BGR entry': lambda: bgr_entry(srcs['bgr'], outs['a'])}
            for l in LAYOUTS:
                fns[f'fmt {l}'] = lambda l=l: fmt_entry(l, outs['a'])
            fns['two-pass nv12'] = lambda: bgr_entry(torch_nv12_to_bgr(srcs['nv12'], h, w, m), outs['a'])
            t = shuffled_windows_us(fns, a.reps, a.batch)
            lines += ['', f'### {name} {h} x {w} -> {nh} x {nw} in {ph} x {pw}, n = {n}, {lens_name}', '',
                      '| candidate | source bytes / pixel | us per launch (median; min .. max) | / BGR entry | bytes moved (MB) | GB/s |', '|---|---|---|---|---|---|']
            for k, v in t.items():
                l = k.split()[-1] if k != 'BGR entry' else 'bgr'
                sb = srcs[l].numel()
                moved = sb + outs['a'].numel() * 4
                lines.append(f'| {k} | {sb / (n * h * w):.2f} | {cell(v)} | {v[0] / t["BGR entry"][0]:.2f} | {moved / 1e6:.1f} | {moved / v[0] / 1e3:.0f} |')
            print('\n'.join(lines[-(len(t) + 4):]), flush=True)
        del srcs, outs
    if a.md:
        with open(a.md, 'w') as fo:
            fo.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
