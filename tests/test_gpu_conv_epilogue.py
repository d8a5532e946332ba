"""-m gpu: every copy of the conv epilogue (include/imvoxel.h: v = acc*scale + shift; [v += res]; [ReLU]; [v += res if res_after_act];
v *= post_scale) against the fp64 reference of tests/ref_conv.py, whose cases, drivers and the condition that they tell a wrong order
from the right one are proved on the CPU by tests/test_host_conv_epilogue.py.  Each case runs {res before act, res after act} x
{post_scale 1, 0.5, -1.25} x {ReLU on, off}; every output is pre-filled with NaN; every test states how it knows that the form it is
about ran (an explicit entry point, the library's own *_supported / workspace / route answer, or the per-thread variant knob taken with
the kernel's own precondition).  Every test prints its worst error / tolerance.  DESIGN.md lists the epilogue sites and the test that
reaches each."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref_conv as R
import ref_pair as P
from test_gpu_pair_range import GpuBackend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def L():
    from imvoxelnet_amd import _lib
    lib = _lib.lib()
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    return lib


@pytest.fixture(scope='module')
def be(L):
    return GpuBackend(L)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def nan_like(shape, dtype=torch.float32):
    return torch.full(tuple(shape), float('nan'), device='cuda', dtype=dtype)


class tile_override:
    """with tile_override(L, cfg, narrow): the per-thread A/B knobs of the direct kernel, put back on exit"""

    def __init__(self, L, cfg, narrow=0):
        self.L, self.cfg, self.narrow = L, cfg, narrow

    def __enter__(self):
        assert self.L.ivx_conv_set_tile_override(self.cfg) == 0 and self.L.ivx_conv_set_epilogue_mode(self.narrow) == 0

    def __exit__(self, *exc):
        self.L.ivx_conv_set_tile_override(0)
        self.L.ivx_conv_set_epilogue_mode(0)
        return False


# ---------------------------------------------------------------------------------------------------------------- direct fp32
@pytest.mark.parametrize('case', R.DIRECT + R.RES2_SMALL, ids=lambda c: c.name)
def test_direct_generic_kernel(be, L, case):
    """conv_epilogue of the generic kernel (filter layout 0, tile override 1: plan_conv takes the override as the configuration, and 1 .. 7
    are the generic kernel's).  No split: a forced tile never plans one."""
    with tile_override(L, 1):
        worst = R.run_direct_options(be, case, 0, want_split=False)
    print(f'gpu generic kernel {case.name}: worst error / tolerance = {worst:.3f}')


@pytest.mark.parametrize('narrow', [0, 1], ids=['wide', 'narrow'])
@pytest.mark.parametrize('case', R.DIRECT + R.RES2_SMALL, ids=lambda c: c.name)
def test_direct_lds_dma_kernel(be, L, case, narrow):
    """The LDS-DMA kernel: conv_epilogue_wide (Cout % 4 == 0, fp32 output, out_mode 0, the knob off) and, with
    ivx_conv_set_epilogue_mode(1) or a Cout that is no multiple of 4, conv_epilogue.  Tile 47 (64 x 64) where Cout > 32, else the rule's
    own choice for Cout <= 32 (44): both are LDS-DMA configurations, taken whenever the operands stay below 2 GiB."""
    cfg = 47 if case.cout > 32 else 0
    worst = 0.0
    for layout in (0, 1) if case.cin % 32 == 0 else (0,):
        with tile_override(L, cfg, narrow):
            worst = max(worst, R.run_direct_options(be, case, layout, want_split=False if cfg else None))
    print(f'gpu LDS-DMA kernel {case.name} narrow {narrow} (wide applies: {case.cout % 4 == 0 and not narrow}): worst error / tolerance = {worst:.3f}')


@pytest.mark.parametrize('case', R.SPLITK, ids=lambda c: c.name)
def test_direct_split_k(be, L, case):
    """conv_store_one in the split-K reduction: ivx_conv_workspace_bytes > 0 for every option (asserted by the driver); the FPN lateral
    2048 -> 64 reads the nearest-upsampled level (res_mode 2, exact x2 and 12 x 40 from 7 x 21)."""
    worst = max(R.run_direct_options(be, case, layout, want_split=True) for layout in (1, 0))
    print(f'gpu split-K {case.name}: worst error / tolerance = {worst:.3f}')


@pytest.mark.parametrize('cfg', [1, 0], ids=['generic', 'lds_dma'])
@pytest.mark.parametrize('case', R.UP2, ids=lambda c: c.name)
def test_transposed_conv_scatter(be, L, case, cfg):
    """out_mode 1 (ConvTranspose k2 s2) with BN, residual, ReLU and post_scale on the generic tile 1 and on the rule's LDS-DMA tile"""
    with tile_override(L, cfg):
        worst = R.run_direct_options(be, case, 0, want_split=False if cfg else None)
    print(f'gpu out_mode 1 {case.name} tile {cfg}: worst error / tolerance = {worst:.3f}')


# ---------------------------------------------------------------------------------------------------------------- bf16 storage
@pytest.mark.parametrize('case', R.BF16, ids=lambda c: c.name)
def test_bf16_storage(L, case):
    """conv_epilogue_wide_bf16 (bf16 output, Cout % 8 == 0; its own res2_row_base branch) and conv_epilogue_wide (fp32 output) on bf16
    operands, each against the one-channel-per-lane epilogue bit for bit and against fp64 on the bf16-rounded operands and residual"""
    from imvoxelnet_amd import ops
    case.make()
    bf = torch.bfloat16
    assert case.cin % 64 == 0 and case.cout % 8 == 0
    x, w = dev(case.x, bf), dev(R.pack_layout1(case.w, 64), bf)
    sc, sf = dev(case.scale), dev(case.shift)
    worst = {}
    for odt, tol in ((torch.float32, R.TOL_BF16_IN), (bf, R.TOL_BF16_OUT)):
        res = dev(case.res, odt)
        for o in case.options():
            outs = []
            for narrow in (0, 1):
                with tile_override(L, 0, narrow):
                    outs.append(ops.conv_fwd(x, w, sc, sf, case.kernel, case.stride, case.padding, o['relu'], res, case.res_mode, out=nan_like(case.oshape, odt),
                                             wgt_layout=1, res_after_act=o['after'], post_scale=o['post'], out_dtype=odt))
            assert outs[0].dtype == odt and torch.equal(outs[0], outs[1]), f'{case.name} {R.opt_id(o)}: wide and narrow epilogue differ'
            r = R.check(f'gpu {case.name} out {odt} {R.opt_id(o)}', outs[0].float().cpu().numpy(), case.ref(o), tol)
            worst[odt] = max(worst.get(odt, 0.0), r)
    print(f'gpu bf16 storage {case.name}: worst error / tolerance ' + ', '.join(f'{k}: {v:.3f}' for k, v in worst.items()))


def test_fp8_output_residual_after_act(L):
    """conv_epilogue_wide_fp8 with res_after_act and post_scale -1.25: the 'f8_1x1_64_256_res' case of test_conv_fp8_storage, with that
    test's reference construction (torch conv2d on the dequantised operands, quantised like the output) and its bounds"""
    from imvoxelnet_amd.conv import FusedConv, QTensor, FP8, FP8_MAX

    def to_dev(q):
        return q.view(torch.uint8).unsqueeze(2).permute(0, 2, 3, 4, 1).contiguous().cuda().view(FP8)

    def to_host(d):
        return d.view(torch.uint8).permute(0, 4, 1, 2, 3).contiguous().cpu().view(FP8).float()[:, :, 0]
    name, B, Cin, H, W, Cout = 'f8_1x1_64_256_res_after', 2, 64, 24, 40, 256
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(B, Cin, H, W, generator=g).abs() * 2.0
    w = torch.randn(Cout, Cin, 1, 1, generator=g) * (2.0 / Cin) ** 0.5
    bnp = (torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1, torch.randn(Cout, generator=g) * 0.1, torch.rand(Cout, generator=g) + 0.5)
    s_x = float(x.abs().max()) / FP8_MAX
    xq = (x / s_x).to(FP8)
    s_w = w.reshape(Cout, -1).abs().amax(1) / FP8_MAX
    wq = (w / s_w.view(-1, 1, 1, 1)).to(FP8)
    conv = F.batch_norm(F.conv2d(xq.float() * s_x, wq.float() * s_w.view(-1, 1, 1, 1)), bnp[2], bnp[3], bnp[0], bnp[1], False, 0.0, 1e-5)
    r = torch.randn(conv.shape, generator=g)                                   # both signs: the side of the ReLU shows
    s_r = float(r.abs().max()) / FP8_MAX
    rq = (r / s_r).to(FP8)
    ref = (F.relu(conv) + rq.float() * s_r) * -1.25
    other = F.relu(conv + rq.float() * s_r) * -1.25
    assert float(((ref - other).abs() > 0.25 * ref.abs() + 0.01 * float(ref.abs().max())).float().mean()) > 0.25      # (two e4m3 steps apart)
    FusedConv.calib = {'k': float(ref.abs().max())}
    try:
        fc = FusedConv(w, None, bnp, stride=1, padding=0, relu=True, dims=2, dtype=FP8, out_dtype=FP8, key='k').to('cuda')
    finally:
        FusedConv.calib = None
    xin, res = QTensor(to_dev(xq), s_x), QTensor(to_dev(rq), s_r)
    y = fc(xin, res=res, res_after_act=True, post_scale=-1.25)
    yn = fc(xin, res=res, res_after_act=True, post_scale=-1.25, naive=True)
    assert isinstance(y, QTensor) and y.data.dtype == FP8
    got, gotn = to_host(y.data) * y.scale, to_host(yn.data) * y.scale
    want = (ref / y.scale).clamp(-FP8_MAX, FP8_MAX).to(FP8).float() * y.scale
    for nm, a, b in (('mfma-vs-torch', got, want), ('mfma-vs-naive', got, gotn)):
        diff = (a - b).abs()
        ulp = torch.maximum(a.abs(), b.abs()) * 2 ** -3 + y.scale * 2 ** -9 + 1e-4 * float(ref.abs().max())
        print(f'gpu fp8 output {nm}: worst error / bound = {float((diff / ulp).max()):.3f}, {float((diff > 0).float().mean()):.4f} of the elements differ')
        assert bool((diff <= ulp).all()), f'{nm}: {int((diff > ulp).sum())} elements beyond one e4m3 step'
        assert float((diff > 0).float().mean()) < 0.03
    with tile_override(L, 0, 1):
        y_narrow = fc(xin, res=res, res_after_act=True, post_scale=-1.25)
    assert torch.equal(y.data.view(torch.uint8), y_narrow.data.view(torch.uint8))


# ---------------------------------------------------------------------------------------------------------------- split-operand form
@pytest.mark.parametrize('case', R.PAIR_SPLIT, ids=lambda c: c.name)
def test_split_operand_form(L, case):
    """ops.conv_fwd(pair=True) on bf16 (hi, lo) operands: ivx_conv_pair_supported says the layer takes the form"""
    from imvoxelnet_amd import ops
    from imvoxelnet_amd.conv import pack_pair_weights
    case.make()
    assert ops.conv_pair_supported((case.B,) + case.sp + (case.cin,), case.cout, case.kernel, case.stride, case.padding, 1)
    xp, wp = ops.bf16_pair_split(dev(case.x)), pack_pair_weights(dev(case.w), 1)
    sc, sf, res = dev(case.scale), dev(case.shift), dev(case.res)
    worst = 0.0
    for o in case.options():
        y = ops.conv_fwd(xp, wp, sc, sf, case.kernel, case.stride, case.padding, o['relu'], res, 1, out=nan_like(case.oshape), wgt_layout=1,
                         res_after_act=o['after'], post_scale=o['post'], pair=True)
        worst = max(worst, R.check(f'gpu split-operand {case.name} {R.opt_id(o)}', y.cpu().numpy(), case.ref(o), R.TOL_F32))
    print(f'gpu split-operand {case.name}: worst error / tolerance = {worst:.3f}')


# ---------------------------------------------------------------------------------------------------------------- ivx_conv_fwd_pio
@pytest.mark.parametrize('side', ['below', 'above'])
@pytest.mark.parametrize('case', P.AFTER_ACT_CONV, ids=lambda c: f'{c[0]}x{c[1][0]}x{c[1][1]}-{c[2]}-{c[3]}-k{c[4]}')
def test_pio_residual_after_act_tight(be, case, side):
    """conv_pio_finish4_rr with res_after_act on cases of ref_pair's table -- 1x1, 3x3 with fp32 and pair outputs, and the split-K shape
    2048 -> 512 at 12 x 40 (conv_splitk_reduce_pio_kernel) -- against ref_pair's derived bound"""
    worst, Lc = P.run_tight_conv(be, case, side, True)
    print(f'gpu tight conv res_after_act {case} {side}: worst error / bound = {worst:.3f}, L = {Lc:.5f}')


@pytest.mark.parametrize('k', [1, 3])
def test_pio_residual_after_act_signed(be, k):
    """the same on data of both signs with post_scale -1.25, where the side of the ReLU and of the multiplier shows"""
    worst = P.run_signed_after_act_conv(be, k)
    print(f'gpu conv {k}x{k} res_after_act on signed data: worst error / bound = {worst:.3f}')


# ---------------------------------------------------------------------------------------------------------------- Winograd
def _wino_setup(case, tile, operands):
    from imvoxelnet_amd import ops
    case.make()
    layout = 1 if case.cin % 32 == 0 else 0
    shape = (case.B,) + case.sp + (case.cin,)
    assert ops.conv_winograd_supported(shape, case.cout, case.kernel, case.stride, case.padding, tile, operands)
    u = ops.conv_winograd_weights(dev(case.w), layout, tile, operands)
    return layout, u, dev(case.x), dev(case.scale), dev(case.shift), dev(case.res)


def _check_partials(name, out, part):
    assert float(part.min()) >= 0.0, f'{name}: a negative partial maximum'
    assert float(part.max()) == float(out.abs().max()), f'{name}: max(partials) {float(part.max())!r} against max|stored| {float(out.abs().max())!r}'


@pytest.mark.parametrize('tile,operands', [(2, 0), (4, 0), (6, 0), (4, 4), (6, 4)], ids=['F2', 'F4', 'F6', 'F4-pair', 'F6-pair'])
@pytest.mark.parametrize('case', R.WINO, ids=lambda c: c.name)
def test_winograd_three_stage(L, case, tile, operands):
    """wino_finish through ops.conv_winograd_fwd (the Winograd entry points themselves): the one-shot call, the output stage that leaves
    per-workgroup maxima (max(partials) == max|stored| exactly, min >= 0) and, at tile 6, every output kernel 0 .. 5 of
    ivx_conv_winograd_set_variant"""
    from imvoxelnet_amd import ops
    layout, u, x, sc, sf, res = _wino_setup(case, tile, operands)
    kw = dict(kw=3, stride_w=case.stride[2], padding=case.padding, wgt_layout=layout, operands=operands)
    worst = 0.0
    for o in case.options():
        ek = dict(relu=o['relu'], res=res, res_after_act=o['after'], post_scale=o['post'])
        ref, name = case.ref(o), f'gpu winograd {case.name} F{tile} operands {operands} {R.opt_id(o)}'
        y = ops.conv_winograd_fwd(x, u, sc, sf, out=nan_like(case.oshape), **kw, **ek)
        worst = max(worst, R.check(name, y.cpu().numpy(), ref, R.TOL_F32))
        y2, part = ops.conv_winograd_fwd(x, u, sc, sf, out=nan_like(case.oshape), want_amax=True, **kw, **ek)
        worst = max(worst, R.check(name + ' with partial maxima', y2.cpu().numpy(), ref, R.TOL_F32))
        _check_partials(name, y2, part)
        if tile == 6:
            try:
                for v in range(6):
                    assert L.ivx_conv_winograd_set_variant(v, -1) == 0
                    yv = ops.conv_winograd_fwd(x, u, sc, sf, out=nan_like(case.oshape), **kw, **ek)
                    worst = max(worst, R.check(name + f' output kernel {v}', yv.cpu().numpy(), ref, R.TOL_F32))
            finally:
                L.ivx_conv_winograd_set_variant(-1, -1)
    print(f'gpu winograd three-stage {case.name} F{tile} operands {operands}: worst error / tolerance = {worst:.3f}')


@pytest.mark.parametrize('case', R.FUSED, ids=lambda c: c.name)
def test_winograd_fused_gemm_output(L, case):
    """the epilogue inside conv_wino_fold4_kernel (ops.conv_winograd_fwd(fused=True): it raises unless ivx_conv_winograd_fused_supported),
    default one-wave kernel, with the partial maxima"""
    from imvoxelnet_amd import ops
    PAIR = ops.IVX_F16_PAIR
    layout, u, x, sc, sf, res = _wino_setup(case, 4, PAIR)
    assert layout == 1
    worst = 0.0
    for o in case.options():
        name = f'gpu winograd fused {case.name} {R.opt_id(o)}'
        y, part = ops.conv_winograd_fwd(x, u, sc, sf, 3, 1, case.padding, o['relu'], res, out=nan_like(case.oshape), wgt_layout=1, res_after_act=o['after'],
                                        post_scale=o['post'], operands=PAIR, want_amax=True, fused=True)
        worst = max(worst, R.check(name, y.cpu().numpy(), case.ref(o), R.TOL_F32))
        _check_partials(name, y, part)
    print(f'gpu winograd fused {case.name}: worst error / tolerance = {worst:.3f}')


@pytest.mark.parametrize('fused', [False, True], ids=['three_stage', 'fused'])
def test_chained_scale_after_late_add_and_multiplier(L, fused):
    """A producer with res_after_act, post_scale -1.25 and want_amax feeds a pair-operand Winograd consumer: the consumer's operand scale
    from the producer's partial maxima and from a reduction of the tensor itself give identical bits (a maximum taken before the late add
    or the multiplier would give a smaller scale)."""
    from imvoxelnet_amd import ops
    PAIR = ops.IVX_F16_PAIR
    case = R.FUSED[2]
    layout, u, x, sc, sf, res = _wino_setup(case, 4, PAIR)
    o = dict(after=True, post=-1.25, relu=True)
    y, part = ops.conv_winograd_fwd(x, u, sc, sf, 3, 1, case.padding, True, res, out=nan_like(case.oshape), wgt_layout=1, res_after_act=True, post_scale=-1.25,
                                    operands=PAIR, want_amax=True, fused=fused)
    R.check(f'gpu chain producer fused={fused}', y.cpu().numpy(), case.ref(o), R.TOL_F32)
    _check_partials('chain producer', y, part)
    before = np.abs(np.maximum(case.pre, 0.0)).max()                           # what a maximum taken before the add and the multiplier would be
    assert float(part.max()) > 1.2 * before, 'the case cannot tell where the maximum is taken'
    g = torch.Generator().manual_seed(5)
    w2 = (torch.randn(64, 3, 3, 3, case.cout, generator=g) * (2.0 / (27 * case.cout)) ** 0.5).cuda()
    for tile in (4, 6):
        u2 = ops.conv_winograd_weights(w2, 1, tile, PAIR)
        a = ops.conv_winograd_fwd(y, u2, None, None, 3, 1, (1, 1, 1), True, wgt_layout=1, operands=PAIR, amax_in=part)
        b = ops.conv_winograd_fwd(y, u2, None, None, 3, 1, (1, 1, 1), True, wgt_layout=1, operands=PAIR)
        assert torch.isfinite(a).all() and torch.equal(a, b), f'tile {tile}: the consumer differs between the partial maxima and its own reduction'
        ref = np.maximum(R.accumulate(y.cpu().numpy(), w2.cpu().numpy(), (3, 3, 3), (1, 1, 1), (1, 1, 1)), 0.0)
        R.check(f'gpu chain consumer F{tile} fused={fused}', a.cpu().numpy(), ref, R.TOL_F32)


def test_background_form_with_the_options(L):
    """The wedge_and_empty_sample case of test_gpu_neck_background.py, two 64 -> 64 layers of its chain with the options on (layer 1:
    post_scale -1.25; layer 2: the volume as residual, res_after_act, post_scale -1.25): sparse == dense bit for bit -- tensors and partial
    maxima -- and the dense form against fp64, each layer on the input it was given.  ops.conv_winograd_fwd(bg=...) raises unless
    ivx_conv_winograd_bg_supported."""
    from imvoxelnet_amd import ops
    import test_gpu_neck_background as N
    PAIR = ops.IVX_F16_PAIR
    valid = torch.from_numpy(N._masks()['wedge_and_empty_sample']).cuda()
    g = torch.Generator().manual_seed(78)
    vol = torch.randn(N.B, N.X, N.Y, N.Z, 64, generator=g).cuda()
    vol = torch.where(valid[..., None], vol, torch.zeros((), device='cuda')).contiguous()
    lay = []
    for _ in range(2):
        w = (torch.randn(64, 3, 3, 3, 64, generator=g) * (2.0 / (27 * 64)) ** 0.5).cuda()
        lay.append((w, ops.conv_winograd_weights(w, 1, 6, PAIR), (torch.rand(64, generator=g) + 0.5).cuda(), (torch.randn(64, generator=g) * 0.1).cuda()))
    _, views = ops.winograd_bg_plan(valid, (N.B, N.X, N.Y, N.Z, 64), 64, [N.Z, N.Z])
    v0 = views[0].cpu().numpy()
    assert 0 < v0[2] < N.B * N.TX * N.TY and v0[3] >= 1, 'the plan has no background tiles: the sparse form would be the dense one'

    def chain(vs):
        t, p = [vol], [None]
        for l, (w, u, sc, sh) in enumerate(lay):
            y, part = ops.conv_winograd_fwd(t[-1], u, sc, sh, 3, 1, (1, 1, 1), True, vol if l == 1 else None, out=nan_like(vol.shape), wgt_layout=1,
                                            res_after_act=l == 1, post_scale=-1.25, operands=PAIR, amax_in=p[-1], want_amax=True, bg=None if vs is None else vs[l])
            t.append(y)
            p.append(part)
        return t, p
    dt, dp = chain(None)
    st, sp = chain(views)
    for l in (1, 2):
        assert torch.equal(st[l], dt[l]), f'layer {l}: {(st[l] != dt[l]).sum().item()} values differ between the background and the dense form'
        assert torch.equal(sp[l], dp[l]), f'layer {l}: partial maxima differ'
        _check_partials(f'background layer {l}', dt[l], dp[l])
        w, _, sc, sh = lay[l - 1]
        ref = R.conv3d(dt[l - 1].cpu().numpy(), w.cpu().numpy(), sc.cpu().numpy(), sh.cpu().numpy(), (3, 3, 3), (1, 1, 1), (1, 1, 1), True,
                       vol.cpu().numpy() if l == 2 else None, 1, l == 2, -1.25)
        R.check(f'gpu background chain layer {l} dense against fp64', dt[l].cpu().numpy(), ref, R.TOL_F32)


# ---------------------------------------------------------------------------------------------------------------- routing
@pytest.mark.parametrize('case', R.ROUTE, ids=lambda c: c.name)
def test_fused_conv_routes_with_the_options(L, case):
    """FusedConv under the default switches at the neck's production width on the smallest volume that still routes: 64 -> 64 3x3x3 at
    16 x 16 x 8 takes F(4x4,3x3) on pair operands (exec_flops < flops), the stride-2 64 -> 128 at 8 x 8 x 4 the split-operand form; each
    with res=skip, res_after_act=True (FastIndoorImVoxelNeck) and with post_scale=0.5 (the Atlas decoder)."""
    from imvoxelnet_amd import ops
    from imvoxelnet_amd.conv import FusedConv
    case.make()
    fc = FusedConv(torch.from_numpy(case.w).permute(0, 4, 1, 2, 3).contiguous(), bias=torch.from_numpy(case.shift), stride=case.stride, padding=case.padding,
                   relu=True).to('cuda')
    fc.scale = dev(case.scale)
    x, res = dev(case.x), dev(case.res)
    wino = case.stride == (1, 1, 1)
    rt = fc._route(tuple(x.shape))
    if wino:
        assert fc.wino_tile(tuple(x.shape))[0] == 4 and rt.run.wino_operands == ops.IVX_F16_PAIR, 'the layer is meant to route to F(4x4,3x3) on pair operands'
    else:
        assert fc.wino_tile(tuple(x.shape))[0] == 0 and fc.takes_pair_form(tuple(x.shape)), 'the layer is meant to route to the split-operand form'
    worst = 0.0
    for o in (dict(after=True, post=1.0, relu=True), dict(after=False, post=0.5, relu=True), dict(after=True, post=0.5, relu=True)):
        FusedConv.flops, FusedConv.exec_flops, FusedConv.count_flops = 0.0, 0.0, True
        try:
            y = fc(x, res=res, res_after_act=o['after'], post_scale=o['post'])
        finally:
            FusedConv.count_flops = False
        assert (FusedConv.exec_flops < FusedConv.flops) if wino else (FusedConv.exec_flops == 3.0 * FusedConv.flops), (FusedConv.exec_flops, FusedConv.flops)
        worst = max(worst, R.check(f'gpu FusedConv {case.name} {R.opt_id(o)}', y.cpu().numpy(), case.ref(o), R.TOL_F32))
    print(f'gpu FusedConv {case.name}: worst error / tolerance = {worst:.3f}')
