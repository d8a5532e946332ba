"""Worker of tests/test_host_plan.py and tests/test_gpu_plan_switches.py (also imported by them for the in-process checks).

The planner reads IVX_SIDE_STREAM, IVX_FUSE_BOTTLENECK and IVX_FUSE_STEM once per process, so the other setting of a switch needs a fresh
process: the calling test starts this script with the switch in the environment.  Three jobs, on libimvoxel_hip.so (--lib hip) or on the CPU
restatement of the same ABI (--lib cpu):

  plans  build one handle per family, plan one shape each through the *_workspace_bytes queries, read the plans back through the view of
         include/imvoxel_lab.h and run tests/plan_check.py on them; one JSON line with what was seen (sites, fuse values) and any defect.
  run    build a seeded model, run four steps alternating two seeded inputs (A, B, A, B) through ivx_model_detect and save, per step, every
         boundary tensor of the plan (FPN level 0, volume, valid mask, neck output or levels, head output) read out of the arena plus the
         detections to an .npz; --phases runs the four steps once per trace level in the SAME process (prefix t<level>_).
  routes record tests/golden/conv_routes.json: which form every convolution takes (direct, Winograd with which tile and operands, split-operand).
         Section `layers` (no GPU) asks the FusedConv queries on a grid of layers, shapes and switches; section `plans` (GPU, planning only)
         reads the conv steps of every family's detect plan at the BASELINE shapes.  Run it at the commit whose rule is to be the reference,
         BEFORE the rule is touched: tests/test_conv_route.py and tests/test_gpu_plan_switches.py hold every later commit to the file.
  convplans record tests/golden/conv_plans.json: what the conv planner answers one level below the route (ivx_conv_plan_query: tile, K split,
         grid-tail plan, workspace, batch slices; for the grouped launches the z-halo / z-blocked config or the tile) on the grids below, under
         every lab knob, and -- one child process per switch, since they are read once -- under every environment switch.  No GPU.  Run it on a
         library built from the commit whose rules are the reference (IVX_LIB_PATH): tests/test_host_conv_plan.py holds later commits to the file."""
import argparse
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

FAMILIES = ('kitti', 'nuscenes', 'nuscenes_dcn', 'scannet_fast', 'sunrgbd_fast', 'scannet_v1', 'sunrgbd_total')
# BASELINE shapes (B, V, H, W) per family: KITTI batch 4, nuScenes 6 cameras, ScanNet 50 (and 20) views, SUN RGB-D one view
FULL_SHAPES = {'kitti': [(4, 1, 384, 1280)], 'nuscenes': [(1, 6, 928, 1600)], 'nuscenes_dcn': [(1, 6, 928, 1600)],
               'scannet_fast': [(1, 50, 480, 640), (1, 20, 480, 640)], 'sunrgbd_fast': [(1, 1, 480, 640)], 'scannet_v1': [(1, 50, 480, 640)],
               'sunrgbd_total': [(1, 1, 480, 640)]}
IVX_F16_PAIR = 4


def load_lib(which):
    from imvoxelnet_amd import _lib
    if which == 'hip':
        L = _lib.lib()
    else:
        import importlib.util
        spec = importlib.util.spec_from_file_location('ivx_cpu_abi_build', os.path.join(ROOT, 'oracle', 'cpu_abi', 'build.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        L = C.CDLL(mod.build()[0])
    L.ivx_last_error.restype = C.c_char_p
    for f in ('ivx_model_workspace_bytes', 'ivx_neck3d_workspace_bytes', 'ivx_model_detect_workspace_bytes', 'ivx_backbone_fpn_workspace_bytes'):
        getattr(L, f).restype = C.c_int64
    _lib.declare_plan_view(L)
    return L


def family_model(family, n_voxels=None, seed=0, small_channels=False):
    """(module, test_cfg) of a family with seeded random weights; n_voxels overrides the volume (the weights do not depend on it)."""
    import torch
    import imvoxelnet_amd as ia
    from imvoxelnet_amd import workloads as kc
    if family == 'kitti':
        cfg, tcfg = (kc.kitti_model_cfg(in_ch=64, out_ch=64) if small_channels else kc.kitti_model_cfg()), dict(kc.KITTI_TEST_CFG, score_thr=0.05)
    elif family in ('nuscenes', 'nuscenes_dcn'):
        cfg, tcfg = kc.nuscenes_model_cfg(dcn=family == 'nuscenes_dcn'), dict(kc.NUSCENES_TEST_CFG)
    elif family == 'scannet_fast':
        cfg, tcfg = kc.scannet_fast_model_cfg(), dict(kc.SCANNET_FAST_TEST_CFG)
    elif family in ('sunrgbd_fast', 'sunrgbd_total'):
        cfg, tcfg = kc.sunrgbd_fast_model_cfg(), dict(kc.SUNRGBD_FAST_TEST_CFG)
        if family == 'sunrgbd_total':
            cfg['head_2d'] = dict(type='LayoutHead', n_channels=2048, linear_size=256, dropout=0.0)
    elif family == 'scannet_v1':
        cfg, tcfg = kc.scannet_v1_model_cfg(), dict(kc.SCANNET_V1_TEST_CFG)
    else:
        raise KeyError(family)
    if n_voxels is not None:
        cfg['n_voxels'] = tuple(n_voxels)
        if family == 'kitti':
            nv, ox = n_voxels, 0.5 + n_voxels[0] * .32 / 2
            cfg['bbox_head']['anchor_generator']['ranges'] = [[ox - nv[0] * .16, -nv[1] * .16, -1.78, ox + nv[0] * .16 - .32, nv[1] * .16 - .32, -1.78]]
        if family.startswith('nuscenes'):
            nv = n_voxels
            cfg['bbox_head']['anchor_generator']['ranges'] = [[-nv[0] * .16, -nv[1] * .16, -1.0, nv[0] * .16 - .64, nv[1] * .16 - .64, -1.0]]
    torch.manual_seed(1234 + seed)                      # (the LayoutHead's Linear layers initialise from the global generator)
    model = ia.build_detector(cfg, test_cfg=tcfg)
    ia.randomize_(model, seed)
    with torch.no_grad():
        g = torch.Generator().manual_seed(5 + seed)
        h = model.bbox_head
        if hasattr(h, 'conv_cls'):
            h.conv_cls.weight.normal_(0, 0.05, generator=g)
            h.conv_cls.bias.fill_(-1.5)
            h.conv_reg.weight.normal_(0, 0.002, generator=g)
        else:
            h.cls_conv.weight.normal_(0, 0.01, generator=g)
            h.cls_conv.bias.fill_(-1.0)
            h.centerness_conv.weight.normal_(0, 0.005, generator=g)
            h.reg_conv.weight.normal_(0, 0.002, generator=g)
    return model


class Handle:
    """ivx_model handle of a module on library L, in an explicit operand / storage mode (the configuration struct is built on the host)."""

    def __init__(self, L, model, storage=0, trunk_operands=IVX_F16_PAIR, wino_operands=IVX_F16_PAIR, stream=None):
        from imvoxelnet_amd import engine
        self.L, self.model, self.stream = L, model, stream
        cfg = engine.model_cfg(model, with_trunk=True)
        cfg.storage, cfg.trunk_operands, cfg.wino_operands = storage, trunk_operands, wino_operands
        self.cfg = cfg
        self.h = C.c_void_p()
        self.ok(L.ivx_create(C.byref(cfg), C.byref(self.h)), 'ivx_create')
        for key, t in model.state_dict().items():
            if t.dtype.is_floating_point:
                a = t.detach().to('cpu').float().contiguous()
                self.ok(L.ivx_weights_load(self.h, key.encode(), C.c_void_p(a.data_ptr()), (C.c_int64 * max(a.dim(), 1))(*a.shape), a.dim()), key)
        self.ok(L.ivx_weights_finalize(self.h, stream), 'ivx_weights_finalize')

    def ok(self, rc, what):
        if rc != 0:
            raise RuntimeError(f'{what}: {self.L.ivx_last_error().decode()}')

    def close(self):
        if self.h:
            self.L.ivx_destroy(self.h)
            self.h = C.c_void_p()

    def total(self, what, B, V, H, W):
        """Plan `what` through its workspace query; returns (bytes, plan key)."""
        L, h = self.L, self.h
        if what == 'forward':
            n, key = L.ivx_model_workspace_bytes(h, B, V, H, W), (B, V, H, W)
        elif what == 'detect':
            n, key = L.ivx_model_detect_workspace_bytes(h, B, V, H, W), (B, V, H, W)
        elif what == 'trunk':
            n, key = L.ivx_backbone_fpn_workspace_bytes(h, B * V, H, W), (B * V, 1, H, W)
        else:
            n, key = L.ivx_neck3d_workspace_bytes(h, B), (B, 1, 0, 0)
        if n < 0:
            raise RuntimeError(f'{what} {(B, V, H, W)}: {L.ivx_last_error().decode()}')
        return int(n), key

    def plan(self, what, B, V, H, W):
        from plan_check import read_plan
        n, key = self.total(what, B, V, H, W)
        return read_plan(self.L, self.h, what, *key), n


def plans_of(family):
    """The plans a family's entry points use (the LayoutHead predicts one camera: its handle runs through the detect entry point)."""
    return ('forward', 'detect', 'trunk', 'neck')


# ------------------------------------------------------------------------------------------------- job: plans
def job_plans(args):
    from plan_check import check_plan, PlanDefect
    L = load_lib(args.lib)
    out = {'plans': [], 'defects': []}
    for fam in FAMILIES:
        model = family_model(fam)
        hd = Handle(L, model)
        try:
            B, V, H, W = (1, 1, 128, 224) if fam == 'sunrgbd_total' else (2, 2, 128, 224)
            for what in plans_of(fam):
                p, n = hd.plan(what, B, V, H, W)
                try:
                    st = check_plan(p, n)
                except PlanDefect as e:
                    out['defects'].append(f'{fam} {what} {(B, V, H, W)}: {e}')
                    continue
                out['plans'].append(dict(family=fam, what=what, **st))
        finally:
            hd.close()
    print(json.dumps(out))


# ------------------------------------------------------------------------------------------------- job: run
def run_config(name):
    """(family, n_voxels, small channels, B, V, (H, W), storage, trunk_operands, fp8) of a run configuration."""
    return {
        'kitti_small': ('kitti', (24, 28, 12), True, 2, 1, (128, 224), 0, IVX_F16_PAIR, False),
        'kitti_small_f32': ('kitti', (24, 28, 12), True, 2, 1, (128, 224), 0, 0, False),
        'nuscenes_dcn': ('nuscenes_dcn', (24, 24, 12), False, 1, 6, (96, 160), 0, IVX_F16_PAIR, False),
        'scannet_v1_bf16': ('scannet_v1', (32, 32, 16), False, 1, 4, (96, 128), 1, IVX_F16_PAIR, False),
        'scannet_v1_fp8': ('scannet_v1', (32, 32, 16), False, 1, 6, (96, 128), 1, IVX_F16_PAIR, True),
        'scannet_fast': ('scannet_fast', (24, 24, 8), False, 1, 3, (96, 128), 0, IVX_F16_PAIR, False),
        'kitti_full': ('kitti', None, False, 4, 1, (384, 1280), 0, IVX_F16_PAIR, False),
    }[name]


def metas_for(family, B, V, hw):
    import numpy as np
    import imvoxelnet_amd as ia
    from imvoxelnet_amd import workloads as kc
    H, W = hw
    out = []
    for b in range(B):
        if family == 'kitti':
            if hw == (384, 1280):
                m = kc.kitti_meta(t=(0.02 * b, 0.01 * b, 0.0), box_type=ia.LiDARInstance3DBoxes)
            else:                                       # the small volume (24 x 28 x 12 voxels in front of the camera) seen by a short lens
                K = np.array([[36. * W / 160, 0, W / 2, 0], [0, 36. * W / 160, H / 2 - 10, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
                E = np.array([[0, -1, 0, 0.03 * b], [0, 0, -1, 0.2], [1, 0, 0, 0.1], [0, 0, 0, 1]], np.float32)
                m = dict(img_shape=(H, W, 3), ori_shape=(H // 2, W // 2, 3), box_type_3d=ia.LiDARInstance3DBoxes,
                         lidar2img=dict(intrinsic=K, extrinsic=[E], origin=np.array([0.5 + 24 * .16, 0, -1.0], np.float32)))
        elif family.startswith('nuscenes'):
            m = kc.nuscenes_meta(img_hw=hw, box_type=ia.LiDARInstance3DBoxes)
            m['lidar2img']['extrinsic'] = [np.ascontiguousarray(np.diag([H / 928.0, H / 928.0, 1, 1]).astype(np.float32) @ e) for e in m['lidar2img']['extrinsic']]
        else:
            m = kc.indoor_meta(V, img_hw=hw, origin=(0, 3, -1) if family.startswith('sunrgbd') else (0, 0, .5), box_type=ia.DepthInstance3DBoxes)
            m['lidar2img']['intrinsic'] = m['lidar2img']['intrinsic'].copy()
            m['lidar2img']['intrinsic'][:2] *= H / 480.0
        out.append(m)
    return out


def detect_once(hd, img, metas, dev, ws_cache):
    """One ivx_model_detect on device `dev` ('cpu' for the CPU restatement): {name: numpy array} of the plan's boundary tensors and detections."""
    import numpy as np
    import torch
    from imvoxelnet_amd._lib import SampleMeta
    from plan_check import read_plan
    L, h = hd.L, hd.h
    B, V, _, H, W = img.shape
    sm, keep = (SampleMeta * B)(), []
    for b, meta in enumerate(metas):
        K = np.zeros((4, 4), np.float32)
        Ki = np.asarray(meta['lidar2img']['intrinsic'], np.float32)
        K[:Ki.shape[0], :Ki.shape[1]] = Ki
        sm[b].intrinsic[:] = K.reshape(-1).tolist()
        if not hd.cfg.layout_head:
            E = np.zeros((V, 4, 4), np.float32)
            for v, e in enumerate(meta['lidar2img']['extrinsic']):
                e = np.asarray(e, np.float32)
                E[v, :e.shape[0], :e.shape[1]] = e
            keep.append(E)
            sm[b].extrinsics = E.ctypes.data
        sm[b].origin[:] = [float(v) for v in np.asarray(meta['lidar2img']['origin'], np.float32)]
        sm[b].img_h, sm[b].img_w, sm[b].ori_h = int(meta['img_shape'][0]), int(meta['img_shape'][1]), int(meta['ori_shape'][0])
    n, key = hd.total('detect', B, V, H, W)
    M = L.ivx_model_max_detections(h, B, V, H, W)
    assert M > 0, L.ivx_last_error()
    if ws_cache.get('n') != n:
        ws_cache['n'], ws_cache['raw'] = n, torch.zeros((n + 256,), dtype=torch.uint8, device=dev)
        ws_cache['plan'] = read_plan(L, h, 'detect', *key)
    raw = ws_cache['raw']
    shift = -raw.data_ptr() % 256
    ws = raw[shift:shift + n]
    boxes, scores = torch.zeros((B, M, 7), device=dev), torch.zeros((B, M), device=dev)
    labels, count = torch.zeros((B, M), dtype=torch.int64, device=dev), torch.zeros((B,), dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    hd.ok(L.ivx_model_detect(h, p(img), B, V, H, W, C.cast(sm, C.c_void_p), p(ws), C.c_int64(n), p(boxes), p(scores), p(labels), p(count),
                             None, None, None, hd.stream), 'ivx_model_detect')
    if dev != 'cpu':
        torch.cuda.synchronize()
    out = {}
    plan = ws_cache['plan']
    for t, ti in plan['tensors'].items():
        if ti['boundary'] and ti['off'] >= 0 and not ti['caller_owned'] and ti['first'] >= plan['info']['s0']:
            out[f'tensor{t}'] = ws[ti['off']:ti['off'] + ti['used']].cpu().numpy().copy()
    lift = [s for s in plan['steps'].values() if s['kind'] == 4][0]
    out['fpn0'] = out[f"tensor{lift['in']}"].view(np.uint16 if hd.cfg.storage == 1 else np.float32)
    cnt = count.cpu().numpy()
    out['count'] = cnt
    for b in range(B):
        k = int(cnt[b])
        out[f'boxes{b}'], out[f'scores{b}'], out[f'labels{b}'] = boxes[b, :k].cpu().numpy(), scores[b, :k].cpu().numpy(), labels[b, :k].cpu().numpy()
    return out


def job_run(args):
    import numpy as np
    import torch
    L = load_lib(args.lib)
    dev = 'cuda' if args.lib == 'hip' else 'cpu'
    fam, nv, small, B, V, hw, storage, trunk, fp8 = run_config(args.config)
    model = family_model(fam, n_voxels=nv, seed=3, small_channels=small)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if dev == 'cuda' else None
    hd = Handle(L, model, storage=storage, trunk_operands=trunk, stream=stream)
    imgs = [torch.randn(B, V, 3, *hw, generator=torch.Generator().manual_seed(11 + k)).to(dev).contiguous() for k in range(2)]
    metas = metas_for(fam, B, V, hw)
    if fp8:                                             # the 'conv3' variant: e4m3 conv3 of ResNet stages 3 and 4 (first_stage 2, conv2 stays bf16)
        x = imgs[0].reshape(B * V, 3, *hw)
        n = L.ivx_backbone_fpn_workspace_bytes(hd.h, B * V, *hw)
        raw = torch.zeros((n + 256,), dtype=torch.uint8, device=dev)
        ws = raw[-raw.data_ptr() % 256:]
        hd.ok(L.ivx_model_calibrate_fp8_ex(hd.h, C.c_void_p(x.data_ptr()), B * V, hw[0], hw[1], C.c_float(1.0), 2, 1, C.c_void_p(ws.data_ptr()),
                                           C.c_int64(n), stream), 'ivx_model_calibrate_fp8_ex')
    arrays, cache = {}, {}
    for level in [int(v) for v in args.phases.split(',')]:
        hd.ok(L.ivx_model_trace(hd.h, level), 'ivx_model_trace')
        for step in range(4):
            for k, a in detect_once(hd, imgs[step % 2], metas, dev, cache).items():
                arrays[f't{level}_s{step}_{k}'] = a
    info = cache['plan']['info']
    steps = cache['plan']['steps'].values()
    arrays['n_sides'] = np.int64(info['n_sides'])
    arrays['fuse'] = np.array(sorted({s['fuse'] for s in steps}), np.int64)
    hd.close()
    np.savez(args.out, **arrays)
    print(json.dumps(dict(config=args.config, n_sides=int(info['n_sides']), arrays=len(arrays), total=info['total'])))


def compare_runs(a, b, prefix_a, prefix_b=None):
    """Every saved array of run `a` equals run `b` bit for bit, step for step, and inside each run step 3 repeats step 1 and step 4 step 2.
    Returns the number of arrays per step."""
    prefix_b = prefix_b or prefix_a
    names = sorted(k[len(prefix_a) + 4:] for k in a.files if k.startswith(prefix_a + '_s0_'))
    assert names and 'fpn0' in names and 'count' in names
    for step in range(4):
        for nm in names:
            x, y = a[f'{prefix_a}_s{step}_{nm}'], b[f'{prefix_b}_s{step}_{nm}']
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), f'step {step + 1}: {nm} differs between the two runs'
    for run, pre in ((a, prefix_a), (b, prefix_b)):
        for step in (2, 3):
            for nm in names:
                assert run[f'{pre}_s{step}_{nm}'].tobytes() == run[f'{pre}_s{step - 2}_{nm}'].tobytes(), \
                    f'{nm}: step {step + 1} does not repeat step {step - 1} (something is carried over between calls)'
    assert any(a[f'{prefix_a}_s0_{nm}'].tobytes() != a[f'{prefix_a}_s1_{nm}'].tobytes() for nm in names), 'the two inputs give the same outputs'
    return len(names)


# ------------------------------------------------------------------------------------------------- job: routes
ROUTES_FILE = os.path.join(HERE, 'golden', 'conv_routes.json')
PLAN_MODES = [(0, 4, 4), (0, 0, 0), (1, 4, 4)]           # (storage, trunk_operands, wino_operands) of the handles the plan tests build
ROUTE_DEFAULTS = dict(winograd=True, winograd_tile=0, wino_operands=IVX_F16_PAIR, pair_mode=-1)      # the switches a route row may override
# FusedConv arguments (Cout, Cin, kernel, stride, padding, dims, layout) of the grid's layers
ROUTE_LAYERS = [(co, ci, (3, 3, 3), (1, 1, 1), 1, 3, lay) for co, ci, lay in ((64, 64, None), (128, 128, None), (256, 256, None), (32, 32, None),
                                                                             (48, 48, 0), (40, 40, None), (25, 64, None))] + \
               [(128, 64, (3, 3, 3), (1, 1, 2), 1, 3, None), (128, 64, (3, 3, 3), (2, 2, 2), 1, 3, None), (512, 256, (3, 3, 3), (2, 2, 2), 1, 3, None),
                (128, 64, (1, 1, 1), (1, 1, 1), 0, 3, None)] + \
               [(c, c, (3, 3), (1, 1), 1, 2, None) for c in (64, 128, 256)] + \
               [(128, 128, (3, 3), (2, 2), 1, 2, None), (64, 256, (1, 1), (1, 1), 0, 2, None), (64, 3, (7, 7), (2, 2), 3, 2, None)]
# input shapes (B, D, H, W) on both sides of every threshold: 1980 / 2000 positions, planes of 16256 / 16384 padded positions, 192 / 256 positions,
# the 31-bit refusals of the split form (64 x 216 x 248 x 12 at 64 channels) and of the Winograd form (one transformed plane past 2 GiB)
ROUTE_SHAPES_3D = [(1, 9, 11, 20), (1, 10, 10, 20), (1, 127, 128, 2), (1, 128, 128, 2), (1, 8, 8, 3), (1, 8, 8, 4), (1, 40, 40, 16), (64, 216, 248, 12),
                   (16, 1296, 1296, 12)]
# ... and for the 2-D layers: the same plane sizes, 197500 / 200000 positions (prefers_winograd), 1980 / 2000 positions, a plane past 2 GiB
ROUTE_SHAPES_2D = [(1, 1, 127, 128), (1, 1, 128, 128), (50, 1, 50, 79), (50, 1, 50, 80), (1, 1, 36, 55), (1, 1, 40, 50), (64, 1, 2592, 2592)]
ROUTE_SWITCHES = [{}, dict(winograd=False), dict(winograd_tile=2), dict(winograd_tile=4), dict(winograd_tile=6), dict(wino_operands=0),
                  dict(pair_mode=0), dict(res_mode=1), dict(res_mode=2), dict(naive=True), dict(winograd_tile=6, wino_operands=0),
                  dict(winograd_tile=2, wino_operands=0), dict(winograd=False, wino_operands=0), dict(winograd=False, pair_mode=0),
                  dict(winograd=False, res_mode=2), dict(winograd=False, naive=True), dict(res_mode=2, pair_mode=0), dict(res_mode=1, winograd_tile=4)]


def route_layer(spec):
    """The FusedConv of a ROUTE_LAYERS entry, built on the host under the default switches."""
    import torch
    from imvoxelnet_amd.conv import FusedConv
    co, ci, k, st, pad, dims, lay = spec
    return FusedConv(torch.zeros(co, ci, *k), stride=tuple(st), padding=pad, dims=dims, layout=lay).to('cpu')


class route_switches:
    """with route_switches(sw): the FusedConv class attributes of ROUTE_DEFAULTS, overridden by the entries of `sw` that name one."""

    def __init__(self, sw):
        self.sw = dict(ROUTE_DEFAULTS, **{k: v for k, v in sw.items() if k in ROUTE_DEFAULTS})

    def __enter__(self):
        from imvoxelnet_amd.conv import FusedConv
        self.old = {k: getattr(FusedConv, k) for k in self.sw}
        for k, v in self.sw.items():
            setattr(FusedConv, k, v)

    def __exit__(self, *exc):
        from imvoxelnet_amd.conv import FusedConv
        for k, v in self.old.items():
            setattr(FusedConv, k, v)
        return False


def route_answer(f, shape, sw):
    """What the FusedConv queries say about layer f on the input `shape` (B, D, H, W) under the switches `sw`:
    [m, operands of that tile, takes_pair_form, prefers_winograd] and the view [xs, wk, wst, wpad] of wino_tile."""
    x_shape = tuple(shape) + (f.cin_pad,)
    with route_switches(sw):
        m, xs, wk, wst, wpad = f.wino_tile(x_shape, res_mode=sw.get('res_mode', 0), naive=sw.get('naive', False))
        ans = [int(m), int(f._wino_operands(m)), bool(f.takes_pair_form(x_shape, naive=sw.get('naive', False))),
               bool(f.prefers_winograd(shape[0] * shape[1] * shape[2] * shape[3]))]
    return ans, [list(map(int, v)) for v in (xs, wk, wst, wpad)]


def conv_rows(plan):
    """(name, tile, pio, split, ws) of every conv step of a plan read through the plan view."""
    return [[s['name'], s['tile'], s['pio'], s['split'], s['ws']] for _, s in sorted(plan['steps'].items()) if s['kind'] == 2]


def plan_key(fam, mode, shape):
    return f'{fam} {"/".join(map(str, mode))} {"x".join(map(str, shape))}'


def job_routes(args):
    out = json.load(open(ROUTES_FILE)) if os.path.exists(ROUTES_FILE) else {}
    out['commit'] = args.commit
    if args.section in ('layers', 'all'):
        with route_switches({}):
            layers = [route_layer(spec) for spec in ROUTE_LAYERS]
        sec = dict(layers=[list(spec) + [bool(f._split_cand), f._w0_host is not None] for spec, f in zip(ROUTE_LAYERS, layers)],
                   switches=ROUTE_SWITCHES, views=[], rows=[])
        for li, f in enumerate(layers):
            for shape in (ROUTE_SHAPES_3D if f._dims == 3 else ROUTE_SHAPES_2D):
                for wi, sw in enumerate(ROUTE_SWITCHES):
                    ans, view = route_answer(f, shape, sw)
                    if wi == 0:
                        sec['views'].append([li, list(shape)] + view)
                    else:
                        assert view == sec['views'][-1][2:]            # the view is a matter of layer and shape alone
                    sec['rows'].append([li, list(shape), wi] + ans)
        out['layers'] = sec
    if args.section in ('plans', 'all'):
        L = load_lib('hip')
        sec = {}
        for fam in FAMILIES:
            model = family_model(fam)
            for mode in PLAN_MODES:
                hd = Handle(L, model, *mode)
                try:
                    for shape in FULL_SHAPES[fam]:
                        sec[plan_key(fam, mode, shape)] = conv_rows(hd.plan('detect', *shape)[0])
                finally:
                    hd.close()
        out['plans'] = sec
    with open(args.out or ROUTES_FILE, 'w') as fh:
        fh.write('{\n' + ',\n'.join(f' {json.dumps(k)}: ' + (json.dumps(v) if k == 'commit' else '{\n' + ',\n'.join(
            f'  {json.dumps(k2)}: {json.dumps(v2, separators=(",", ":"))}' for k2, v2 in v.items()) + '\n }') for k, v in out.items()) + '\n}\n')
    print(json.dumps({k: (v if k == 'commit' else {k2: len(v2) for k2, v2 in v.items()} if k == 'layers' else len(v)) for k, v in out.items()}))


# ------------------------------------------------------------------------------------------------- job: convplans
PLANS_FILE = os.path.join(HERE, 'golden', 'conv_plans.json')
# the grid of the direct path: the route grid's layers and shapes, plus a 9x9 kernel (no LDS-DMA form: the generic 64 x 64 tile), a wide 1x1 layer
# (the 8- / 16-wave tiles, the 256 x 256 tile of the trunk) and the shapes that put the pair-IO rule on both sides of its tile counts
PLAN_LAYERS = ROUTE_LAYERS + [(64, 16, (9, 9), (1, 1), 4, 2, None), (1024, 256, (1, 1), (1, 1), 0, 2, None), (256, 1024, (1, 1), (1, 1), 0, 2, None)]
PLAN_SHAPES_3D = ROUTE_SHAPES_3D
PLAN_SHAPES_2D = ROUTE_SHAPES_2D + [(4, 1, 48, 160), (4, 1, 24, 80), (6, 1, 116, 200), (4, 1, 96, 320)]
# operand modes: (in_dtype, out_dtype, ivx_pair_io?, 128-byte channel chunk of wgt_layout 1 in channels)
PLAN_MODES_CONV = [(0, 0, False, 32), (1, 1, False, 64), (2, 2, False, 128), (3, 0, False, 32), (4, 0, False, 32), (4, 4, True, 32)]
# per (layer, shape, mode): (allow_ws, plan mode, res_mode); a residual in the modes whose rules read it (fp32, pair IO), res_mode 2 on the 2-D shapes only
PLAN_CALLS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 0, 2), (0, 0, 1)]
# tile override: every row of csrc/conv_tiles.h (0 is the rest of the grid) on two layers at one shape each, every operand mode
PLAN_TILES = [1, 2, 3, 4, 5, 6, 7, 41, 43, 44, 46, 47, 48, 49, 51, 52, 53, 54, 55, 56, 57, 58, 59, 61, 63, 64, 66, 67, 71, 72, 73, 74, 75, 76, 77, 81, 82, 83, 85,
              91, 92, 93, 94, 166, 174, 177, 179, 183, 474, 475, 574] + [8, 45, 65, 90, 175]       # ... and numbers in no row
PLAN_TILE_CASES = [((256, 256, (3, 3), (1, 1), 1, 2, None), (50, 1, 50, 80)), ((128, 64, (1, 1, 1), (1, 1, 1), 0, 3, None), (1, 40, 40, 16))]
# grouped launches (one xi convolution of a Winograd-domain GEMM: 1x1xKW along z on `rows` tile columns): (Cout, Cin), (KW, stride, pad), slices, rows,
# groups, operands
PLAN_G_CH = [(64, 64), (128, 128), (256, 256), (32, 32), (128, 64), (512, 512), (48, 48)]
PLAN_G_K = [(3, 1, 1), (3, 2, 1), (3, 1, 0), (1, 1, 0)]
PLAN_G_Z = [3, 6, 12, 16]
PLAN_G_ROWS = [100, 1600, 13392]
PLAN_G_GROUPS = [16, 36]
PLAN_G_DTYPES = [0, 3, 4]
# halo mode: default, never, every row of IVX_CONV_HALO_CFGS and numbers in no row -- on the f16-pair layers of both z strides
PLAN_HALO_MODES = [-1, 0] + list(range(1, 15)) + [21, 22, 23, 24, 30, 31, 33, 34, 41, 42, 43, 44, 45, 46, 50, 51, 60, 71] + [25, 99, 15, 70]
PLAN_HALO_CASES = [(ch, k, z, 1600, 36) for ch in ((64, 64), (256, 256)) for k in PLAN_G_K[:3] for z in (3, 6)]
# environment switches, each at one value that is not its default (csrc/conv_plan.h IVX_CONV_ENV)
PLAN_ENV = dict(IVX_CONV_SKINNY=0, IVX_PIO_RULE=0, IVX_PIO_SPLITK=0, IVX_PIO_SPLIT_TILES=100, IVX_PIO_DEEP=0, IVX_PIO_DEEP_TILES=128, IVX_PIO_DEEP_SLABS=40,
                IVX_PIO_W16_TILES=0, IVX_PIO_W8_TILES=0, IVX_PIO_T183=0, IVX_PIO_TAIL=1, IVX_PIO_STAGGER_US=5, IVX_PIO_STAGGER_SHIFT=1, IVX_HALO_SMALL=0)


def plan_desc(spec, shape, mode, res_mode=0):
    """(ivx_conv_desc, ivx_pair_io or None) of a PLAN_LAYERS entry on the input `shape` (B, D, H, W) in an operand mode."""
    from imvoxelnet_amd._lib import ConvDesc, PairIO
    co, ci, k, st, pad, dims, _ = spec
    k, st = ((1,) + tuple(k), (1,) + tuple(st)) if dims == 2 else (tuple(k), tuple(st))
    pd = (0, pad, pad) if dims == 2 else (pad, pad, pad)
    ci = (ci + 3) // 4 * 4
    out = [(shape[1 + i] + 2 * pd[i] - k[i]) // st[i] + 1 for i in range(3)]
    in_dt, out_dt, pio, ck = mode
    d = ConvDesc(*shape, ci, co, *k, *st, *pd, 1, res_mode, (out[1] + 1) // 2 if res_mode == 2 else 0, (out[2] + 1) // 2 if res_mode == 2 else 0,
                 1 if ci % ck == 0 else 0, 0, 0, 1.0, in_dt, out_dt, 1.0, 0)
    some = C.c_void_p(64)           # (never read: the query makes no device call)
    return d, (PairIO(some, some, IVX_F16_PAIR, some, some, some, some, 1.0, 1.0) if pio else None)


def grouped_desc(ch, k, z, rows, dtype):
    from imvoxelnet_amd._lib import ConvDesc
    return ConvDesc(1, 1, rows, z, ch[1], ch[0], 1, 1, k[0], 1, 1, k[1], 0, 0, k[2], 0, 0, 0, 0, 1 if ch[1] % 32 == 0 else 0, 0, 0, 1.0, dtype, 0, 1.0, 0)


def plan_row(L, d, io, allow_ws, groups=0):
    """The answer of ivx_conv_plan_query as a list of integers: [rc] when it refuses; direct [samples per slice, then per distinct slice samples, cfg,
    ksplit, tail_ks, q_total, qa, bm, ws_bytes; ws_bytes of the call]; grouped [halo_cfg, tile, tile_matches, rows_dev_ok]."""
    from imvoxelnet_amd._lib import ConvPlanRec
    r = ConvPlanRec()
    rc = L.ivx_conv_plan_query(C.byref(d), C.byref(io) if io is not None else None, allow_ws, groups, C.byref(r))
    if rc != 0:
        return [rc]
    if groups:
        return [r.halo_cfg, r.grouped_tile, r.tile_matches, r.rows_dev_ok]
    row = [r.slice_samples]
    for i in range(r.n_slices):
        row += [r.samples[i], r.cfg[i], r.ksplit[i], r.tail_ks[i], r.q_total[i], r.qa[i], r.bm[i], r.slice_ws[i]]
    return row + [r.ws_bytes]


def plan_workspace(L, d, io):
    """What the two workspace entry points say (the query with allow_ws = 1 must agree)."""
    L.ivx_conv_workspace_bytes.restype = L.ivx_conv_pio_workspace_bytes.restype = C.c_int64
    return L.ivx_conv_pio_workspace_bytes(C.byref(d), C.byref(io)) if io is not None else L.ivx_conv_workspace_bytes(C.byref(d))


def plan_shapes(spec):
    return PLAN_SHAPES_3D if spec[5] == 3 else PLAN_SHAPES_2D


def plan_section(L, name, check=None):
    """The rows of a section of the fixture, in the order of its loops (the keys are not stored).  check(d, io, row): called on the direct rows asked
    with allow_ws = 1."""
    rows = []

    def direct(spec, shape, mode, allow_ws, pm, res):
        d, io = plan_desc(spec, shape, mode, res)
        L.ivx_conv_set_plan_mode(pm)
        rows.append(plan_row(L, d, io, allow_ws))
        if check and allow_ws:
            check(d, io, rows[-1])
        L.ivx_conv_set_plan_mode(0)

    if name == 'direct':
        for spec in PLAN_LAYERS:
            for shape in plan_shapes(spec):
                for mode in PLAN_MODES_CONV:
                    for aw, pm, res in PLAN_CALLS:
                        if res == 0 or (mode in (PLAN_MODES_CONV[0], PLAN_MODES_CONV[5]) and (res != 2 or spec[5] == 2)):
                            direct(spec, shape, mode, aw, pm, res)
    elif name == 'tiles':
        for spec, shape in PLAN_TILE_CASES:
            for mode in PLAN_MODES_CONV:
                for t in PLAN_TILES:
                    L.ivx_conv_set_tile_override(t)
                    direct(spec, shape, mode, 1, 0, 0)
        for t in PLAN_TILES:
            L.ivx_conv_set_tile_override(t)
            for dt in PLAN_G_DTYPES:
                rows.append(plan_row(L, grouped_desc((128, 128), PLAN_G_K[2], 3, 13392, dt), None, 0, 36))
        L.ivx_conv_set_tile_override(0)
    elif name == 'grouped':
        for ch in PLAN_G_CH:
            for k in PLAN_G_K:
                for z in PLAN_G_Z:
                    for n in PLAN_G_ROWS:
                        for g in PLAN_G_GROUPS:
                            for dt in PLAN_G_DTYPES:
                                rows.append(plan_row(L, grouped_desc(ch, k, z, n, dt), None, 0, g))
    elif name == 'halo':
        for hm in PLAN_HALO_MODES:
            L.ivx_conv_set_halo_mode(hm)
            for ch, k, z, n, g in PLAN_HALO_CASES:
                rows.append(plan_row(L, grouped_desc(ch, k, z, n, IVX_F16_PAIR), None, 0, g))
        L.ivx_conv_set_halo_mode(-1)
    elif name == 'env':                     # the reduced grid every environment child answers: what the switches bear on
        for spec in PLAN_LAYERS:
            for shape in plan_shapes(spec):
                for mode in (PLAN_MODES_CONV[5],) if spec[5] == 2 else (PLAN_MODES_CONV[0],) if spec[0] <= 32 else ():
                    for aw, pm, res in PLAN_CALLS[:2] + PLAN_CALLS[3:4]:
                        direct(spec, shape, mode, aw, pm, res)
        for ch in PLAN_G_CH[:3]:
            for z in PLAN_G_Z:
                for n in PLAN_G_ROWS:
                    rows.append(plan_row(L, grouped_desc(ch, PLAN_G_K[0], z, n, IVX_F16_PAIR), None, 0, 36))
    else:
        raise KeyError(name)
    return rows


def plan_tile_infos(L):
    """{number: [bm, bn, bk, wg_per_cu]} of every number the planner knows as an LDS-DMA tile (asked for 0 .. 999)."""
    out = {}
    v = (C.c_int32 * 4)()
    for t in range(1000):
        if L.ivx_conv_tile_info(t, v):
            out[str(t)] = list(v)
    return out


def plan_env_child(name, value):
    """The `env` section as a fresh process answers it with the switch `name` set (the switches are read once per process)."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if not k.startswith('IVX_') or k == 'IVX_LIB_PATH'}
    env[name] = str(value)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'convplans', '--section', 'env'], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f'{name}={value}: {r.stderr[-2000:]}'
    return json.loads(r.stdout.strip().splitlines()[-1])


def plan_env_diff(base, rows):
    """[[index, row]] of the rows that differ from the section under the default environment"""
    assert len(base) == len(rows)
    return [[i, r] for i, (b, r) in enumerate(zip(base, rows)) if b != r]


def job_convplans(args):
    from imvoxelnet_amd import _lib
    L = _lib.lib()
    if args.section == 'env':                # a child of plan_env_child
        print(json.dumps(plan_section(L, 'env'), separators=(',', ':')))
        return
    out = {'commit': args.commit, 'tile_info': plan_tile_infos(L)}
    for name in ('direct', 'tiles', 'grouped', 'halo', 'env'):
        out[name] = plan_section(L, name)
    out['env_switches'] = {k: plan_env_diff(out['env'], plan_env_child(k, v)) for k, v in PLAN_ENV.items()}
    with open(args.out or PLANS_FILE, 'w') as fh:
        fh.write('{\n' + ',\n'.join(f' {json.dumps(k)}: {json.dumps(v, separators=(",", ":"))}' for k, v in out.items()) + '\n}\n')
    print(json.dumps({k: (v if k == 'commit' else len(v)) for k, v in out.items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('job', choices=['plans', 'run', 'routes', 'convplans'])
    ap.add_argument('--lib', choices=['cpu', 'hip'], default='cpu')
    ap.add_argument('--config', default='kitti_small')
    ap.add_argument('--phases', default='0', help='comma-separated trace levels; the four steps run once per level')
    ap.add_argument('--out', default=None)
    ap.add_argument('--section', choices=['layers', 'plans', 'all', 'env'], default='all', help='routes: the section(s) to record; the other is kept')
    ap.add_argument('--commit', default='', help='routes: short hash of the commit whose rule is recorded')
    args = ap.parse_args()
    {'plans': job_plans, 'run': job_run, 'routes': job_routes, 'convplans': job_convplans}[args.job](args)


if __name__ == '__main__':
    main()
