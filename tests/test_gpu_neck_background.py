"""-m gpu: background tiles of the neck outside the camera frustum (include/imvoxel.h ivx_conv_winograd_bg_plan, csrc/winograd.hip): the
plan kernel's lists, maps and counts against a numpy restatement of the definitions, and the sparse form of a small KITTI-shaped chain
(64 -> 64 -> 64 -> 128 -> 128 -> 128 -> 256 -> 256 -> 256 channels, Z 12 -> 6 -> 3, X = 42 = 7 tiles, Y = 44 = 7 tiles and a 2-wide partial
one, batch 2) against the dense form, layer by layer and bit for bit.  Runs on the MI355X box."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, X, Y, Z, C0 = 2, 42, 44, 12, 64
TX, TY = (X + 5) // 6, (Y + 5) // 6
# (Cin, Cout, z stride, index of the residual tensor or None): tensor 0 is the volume, tensor i the output of layer i
LAYERS = [(64, 64, 1, None), (64, 64, 1, 0), (64, 128, 2, None), (128, 128, 1, None), (128, 128, 1, 3), (128, 256, 2, None),
          (256, 256, 1, None), (256, 256, 1, 6)]
OUT_SLICES = [12, 12, 6, 6, 6, 3, 3, 3]


@pytest.fixture(scope='module')
def ia():
    import imvoxelnet_amd
    from imvoxelnet_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    return imvoxelnet_amd


def _masks():
    """valid [B,X,Y,Z] bool per case of the issue."""
    xs, ys = np.arange(X)[:, None], np.arange(Y)[None, :]
    wedge = np.abs(ys - (Y - 1) / 2.0) <= 0.5 * (xs + 1)                      # a forward camera: opens with x, both far corners at small x stay empty
    a = np.zeros((B, X, Y, Z), bool)
    a[0] = wedge[:, :, None]
    d = np.zeros((B, X, Y, Z), bool)
    d[0, 1, 2, 5] = True
    return {'wedge_and_empty_sample': a, 'all_valid': np.ones((B, X, Y, Z), bool), 'all_invalid': np.zeros((B, X, Y, Z), bool),
            'one_voxel_in_a_corner_tile': d}


def plan_reference(valid, out_slices):
    """The definitions restated: Z1(b, T) = no valid voxel in T's 8 x 8 layer-1 window (columns inside the volume, all z); a tile of layer L is
    quiet when every tile of the grid within Chebyshev distance L - 1 has Z1; its key is the four distances to the grid's edges capped at
    L - 1.  Slots: the image-dependent tiles in their order, then one representative per key (the lowest tile index), keys ascending by
    ((left * L + right) * L + top) * L + bottom.  Returns per layer (list, src, image-dependent tiles, keys)."""
    col = valid.any(3)
    z1 = np.zeros((B, TX, TY), bool)
    for tx in range(TX):
        for ty in range(TY):
            z1[:, tx, ty] = ~col[:, max(6 * tx - 1, 0):min(6 * tx + 7, X), max(6 * ty - 1, 0):min(6 * ty + 7, Y)].any((1, 2))
    out = []
    for L in range(1, len(out_slices) + 1):
        r = L - 1
        active, reps, keys = [], {}, {}
        for b in range(B):
            for tx in range(TX):
                for ty in range(TY):
                    t = (b * TX + tx) * TY + ty
                    if z1[b, max(tx - r, 0):tx + r + 1, max(ty - r, 0):ty + r + 1].all():
                        k = ((min(tx, r) * L + min(TX - 1 - tx, r)) * L + min(ty, r)) * L + min(TY - 1 - ty, r)
                        keys[t] = k
                        reps.setdefault(k, t)
                    else:
                        active.append(t)
        order = sorted(reps)
        lst = active + [reps[k] for k in order]
        src = np.zeros(B * TX * TY, np.int64)
        src[active] = np.arange(len(active))
        for t, k in keys.items():
            src[t] = len(active) + order.index(k)
        out.append((np.array(lst, np.int64), src, len(active), len(order)))
    return out


@pytest.fixture(scope='module')
def chain(ia):
    """Volume, filters and epilogue vectors of the chain, made once."""
    from imvoxelnet_amd import ops
    g = torch.Generator().manual_seed(77)
    vol = torch.randn(B, X, Y, Z, C0, generator=g).cuda()
    layers = []
    for ci, co, sw, res in LAYERS:
        w = (torch.randn(co, 3, 3, 3, ci, generator=g) * (2.0 / (27 * ci)) ** 0.5).cuda()
        u = ops.conv_winograd_weights(w, 1, 6, ops.IVX_F16_PAIR)
        sc, sh = (torch.rand(co, generator=g) + 0.5).cuda(), (torch.randn(co, generator=g) * 0.1).cuda()
        layers.append((u, sc, sh, sw, res))
    return vol, layers


def _run_chain(ops, vol, layers, views):
    """The chain as the model handle runs it: every layer's operand scale from the producer's per-workgroup maxima.  views: the plan's
    per-layer blocks, or None for the dense form.  Returns every tensor and every array of maxima."""
    tensors, parts = [vol], [None]
    for l, (u, sc, sh, sw, res) in enumerate(layers):
        y, part = ops.conv_winograd_fwd(tensors[-1], u, sc, sh, 3, sw, (1, 1, 1), True, None if res is None else tensors[res], wgt_layout=1,
                                        operands=ops.IVX_F16_PAIR, amax_in=parts[-1], want_amax=True, bg=None if views is None else views[l])
        tensors.append(y)
        parts.append(part)
    return tensors, parts


@pytest.mark.parametrize('case', ['wedge_and_empty_sample', 'all_valid', 'all_invalid', 'one_voxel_in_a_corner_tile'])
def test_background_plan_matches_the_definitions(ia, case):
    """Lists, maps and counts of every layer against plan_reference; the plan is the same on a second run."""
    from imvoxelnet_amd import ops
    valid = _masks()[case]
    ref = plan_reference(valid, OUT_SLICES)
    vd = torch.from_numpy(valid).cuda()
    _, views = ops.winograd_bg_plan(vd, (B, X, Y, Z, C0), 64, OUT_SLICES)
    _, again = ops.winograd_bg_plan(vd, (B, X, Y, Z, C0), 64, OUT_SLICES)
    torch.cuda.synchronize()
    n = B * TX * TY
    for l, (lst, src, na, nk) in enumerate(ref):
        v = views[l].cpu().numpy().astype(np.int64)
        slots = na + nk
        print(f'{case}: layer {l + 1}: {na} image-dependent tiles + {nk} keys of {n} tiles')
        assert list(v[:4]) == [slots, slots * OUT_SLICES[l], na, nk], (l, v[:4])
        assert np.array_equal(v[4:4 + slots], lst), l
        assert np.array_equal(v[4 + n:4 + 2 * n], src), l
        w = again[l].cpu().numpy().astype(np.int64)
        assert np.array_equal(w[:4 + slots], v[:4 + slots]) and np.array_equal(w[4 + n:], v[4 + n:])
    if case == 'wedge_and_empty_sample':      # what the case is for: quiet tiles down to the last layer, every border key, mixed layers
        assert ref[-1][3] > 1 and ref[0][2] > 0 and ref[0][3] == 1
        assert ref[2][3] == 5 ** 2 and all(0 < r[2] < n for r in ref)      # layer 3: distances capped at 2 -> 5 classes per axis (TX, TY >= 5)
    if case == 'all_valid':
        assert all(r[2] == n and r[3] == 0 for r in ref)
    if case == 'all_invalid':
        assert all(r[2] == 0 for r in ref) and ref[0][3] == 1


@pytest.mark.parametrize('case', ['wedge_and_empty_sample', 'all_valid', 'all_invalid', 'one_voxel_in_a_corner_tile'])
def test_sparse_chain_equals_dense_chain_bit_for_bit(ia, chain, case):
    """Every layer's tensor, every array of per-workgroup maxima and the chain's output: torch.equal between the background form and the
    dense form on the same volume (exactly 0 where no camera sees it, as the unprojection leaves it)."""
    from imvoxelnet_amd import ops
    vol0, layers = chain
    valid = torch.from_numpy(_masks()[case]).cuda()
    vol = torch.where(valid[..., None], vol0, torch.zeros((), device=vol0.device)).contiguous()      # +0 where invalid, as the unprojection writes it
    _, views = ops.winograd_bg_plan(valid, (B, X, Y, Z, C0), 64, OUT_SLICES)
    dense_t, dense_p = _run_chain(ops, vol, layers, None)
    sparse_t, sparse_p = _run_chain(ops, vol, layers, views)
    for l in range(1, len(layers) + 1):
        assert torch.equal(sparse_t[l], dense_t[l]), f'layer {l}: {(sparse_t[l] != dense_t[l]).sum().item()} values differ'
        assert torch.equal(sparse_p[l], dense_p[l]), f'layer {l}: per-workgroup maxima differ'
    assert torch.isfinite(dense_t[-1]).all() and float(dense_t[-1].abs().max()) > 0


def test_native_handle_background_on_and_off(ia):
    """The model handle with the chain planned (default) against IVX_NECK_BACKGROUND=0: same detections bit for bit, and the GEMM records of
    the trace count the products actually issued -- fewer than the dense path's on the first layers of a single forward camera."""
    from imvoxelnet_amd import workloads as kc
    from imvoxelnet_amd.engine import NativeModel
    nv, hw, nb = (104, 120, 12), (192, 640), 2
    model = ia.build_detector(kc.kitti_model_cfg(n_voxels=nv), test_cfg=kc.KITTI_TEST_CFG)
    ia.randomize_(model, 21)
    with torch.no_grad():
        model.bbox_head.conv_cls.weight.normal_(0, 0.03, generator=torch.Generator().manual_seed(5))
        model.bbox_head.conv_cls.bias.fill_(-1.5)
    dev = torch.device('cuda')
    metas = [kc.kitti_meta(img_hw=hw, t=(0.02 * b, 0.01 * b, 0.0), box_type=ia.LiDARInstance3DBoxes) for b in range(nb)]
    p0 = (torch.randn(nb, 1, hw[0] // 4, hw[1] // 4, 64, generator=torch.Generator().manual_seed(3)) * 0.5).cuda()
    model.prepare(dev)
    proj, new_origin, crop = model._camera_setup(metas, 4, dev)
    outs, flops = {}, {}
    old = os.environ.get('IVX_NECK_BACKGROUND')
    try:
        for mode in ('0', '1'):
            os.environ['IVX_NECK_BACKGROUND'] = mode          # read when the handle plans the shape
            nat = NativeModel(model, dev, with_trunk=False, winograd_tile=6)      # (the rule's own tile at this plane size is 4)
            nat.trace(2)
            outs[mode] = nat.forward(p0, nb, 1, hw[0], hw[1], proj, new_origin, crop, want_valid=True)
            torch.cuda.synchronize()
            flops[mode] = [r['flops'] for r in nat.trace_records() if r['stage'] == 2 and r['is3d']]
            nat.trace(0)
            nat.close()
    finally:
        if old is None:
            os.environ.pop('IVX_NECK_BACKGROUND', None)
        else:
            os.environ['IVX_NECK_BACKGROUND'] = old
    for a, b in zip(outs['0'], outs['1']):
        assert torch.equal(a, b)
    assert int(outs['0'][3].sum()) > 0 and 0.0 < float(outs['0'][4].float().mean()) < 1.0
    print('GEMM flops, dense :', flops['0'])
    print('GEMM flops, sparse:', flops['1'])
    assert len(flops['0']) == len(flops['1']) == 9
    assert all(s <= d for s, d in zip(flops['1'], flops['0'])) and flops['1'][0] < 0.9 * flops['0'][0] and flops['1'][8] == flops['0'][8]
