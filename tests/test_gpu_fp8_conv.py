"""-m gpu: the e4m3 forms of the direct convolution (csrc/conv_igemm.hip) through ops.conv_fwd with hand-folded vectors -- the kernel's
contract -- and through FusedConv (the Python host's fold), against the fp64 reference of tests/ref_fp8.py, whose codec, cases, comparison
rule and conditions tests/test_host_fp8_conv.py proves without a device.

Forms: a (bf16 in, e4m3 out), b (e4m3 in and out), c (e4m3 in, bf16 out + bf16 shortcut), d (e4m3 in and out + e4m3 shortcut), f (e4m3 in,
fp32 out); each with the ReLU on and off, post_scale 1 and -1.25 and, where the form has a residual, the residual on either side of the ReLU.
Every run starts from an output filled with byte 0x7F (e4m3) or NaN, every case also runs the validation kernel, every case with e4m3
operands runs under the rule's tile and under tiles 91, 92, 93 and 94, form a under the rule's tile and the bf16 tiles 74 and 61 (TN = 2:
conv_epilogue_wide_fp8 as NJ = 2) and 66 and 63 (TN = 1: NJ = 1); wherever the wide epilogue applies the narrow one runs as well.  Every
output is compared with the reference: an e4m3 output by the rule of ref_fp8 (the exact byte away from a rounding boundary, one of the
codes that meet within delta = 1e-4 max |reference| of one, nothing left out), a bf16 / fp32 output within ref_conv.TOL_BF16_OUT /
TOL_BF16_IN.  Wide and narrow epilogue must agree byte for byte under every tile, and so must the tiles among themselves (the rule's own
tile excepted where it splits K).  Every test prints, per distinct output, the runs that stored it, its worst error / bound and the share
of boundary elements; a failed comparison names the case, the runs, the element, the stored byte, the reference and the nearest boundary.

Measured on the MI355X: the reference lies at most 0.096 delta outside the stored code's cell with e4m3 operands (a boundary element took
the other code on at most 0.8 % of a run) and 0.000 with bf16 operands; bf16 outputs reach 0.47 of TOL_BF16_OUT, fp32 outputs 0.28 of
TOL_BF16_IN; the share of boundary elements is 0.8 % .. 5.6 %.  All tiles and both epilogues stored identical bytes in every case, the
split-K launches of the rule's tile too, except in one option of the bf16 form of k3_c128_n256.  The saturation case showed the NaN stored
as 0xFE (-448) by every path before f32x2_to_fp8 selected the unclamped operand for a NaN; it passes since.  Dropping res_scale from
conv_epilogue_wide_fp8, or swapping the tile pair in its NJ = 2 staging index, in a scratch build fails 8 and 23 of the 41 tests here."""
import ctypes as C

import numpy as np
import pytest
import torch

import ref_conv as R
import ref_fp8 as Q
from test_gpu_conv_epilogue import tile_override

pytestmark = pytest.mark.gpu

E4M3_TILES = (0, 91, 92, 93, 94)        # 91, 94: TN = 2 (NJ = 2);  92, 93: TN = 1
BF16_TILES = (0, 74, 61, 66, 63)        # 74, 61: TN = 2 (NJ = 2);  66, 63: TN = 1 (from the list of test_conv_bf16_tile_variants)
WIDE_MULTIPLE = {'e4m3': 16, 'bf16': 8, 'f32': 4}


@pytest.fixture(scope='module')
def L():
    from imvoxelnet_amd import _lib
    lib = _lib.lib()
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    return lib


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def workspace_bytes(L, case, o):
    """what plan_conv asks for under its own rule: > 0 exactly when it splits K"""
    from imvoxelnet_amd import ops
    p = case.k // 2
    d = ops.ConvDesc(case.B, 1, case.hw[0], case.hw[1], case.cin, case.cout, 1, case.k, case.k, 1, case.s, case.s, 0, p, p, int(o['relu']), 1 if o['res'] else 0,
                     0, 0, case.layout, 0, int(o['res'] == 'after'), o['post'], ops._DT[Q.TORCH_DT[case.in_t]], ops._DT[Q.TORCH_DT[case.out_t]], 1.0)
    return int(L.ivx_conv_workspace_bytes(C.byref(d)))


def compare(name, case, y, ex):
    """one output against the reference: (worst error / bound, boundary share or None)"""
    if case.out_t == 'e4m3':
        return Q.check_bytes(name, Q.to_host(case, y), ex)
    return R.check(name, Q.to_host(case, y), ex.u, Q.TOL[case.out_t]), None


def run_case(L, case, tiles, options=None):
    """Every option of the case under every tile, wide and narrow where the wide epilogue applies, and the validation kernel.  Outputs that
    are byte-identical are compared with the reference once, under the names of all the runs that stored them; then the identities are
    asserted.  Returns (worst ratio, largest boundary share, {option: groups of identical runs})."""
    from imvoxelnet_amd import ops
    case.make()
    operands = Q.to_device(case)
    wide = case.cout % WIDE_MULTIPLE[case.out_t] == 0
    worst, share, groups = 0.0, 0.0, {}
    for o in options or case.options():
        sc, sf, rs = Q.folded_f32(case, o)
        vec = (dev(sc), dev(sf), rs)
        ex = case.expect(o, sc, sf, rs)
        runs = []
        for cfg in tiles:
            for narrow in (0, 1) if wide else (0,):
                with tile_override(L, cfg, narrow):
                    runs.append((f'tile {cfg}{" narrow" if narrow else " wide" if wide else ""}', Q.run(ops, case, o, operands, vec)))
        runs.append(('validation kernel', Q.run(ops, case, o, operands, vec, naive=True)))
        distinct = []
        for label, y in runs:
            for y0, labels in distinct:
                if same_bytes(y0, y):
                    labels.append(label)
                    break
            else:
                distinct.append((y, [label]))
        for y, labels in distinct:
            ratio, b = compare(f'{case.name} {Q.opt_id(o)} [{", ".join(labels)}]{"" if wide else " (narrow epilogue by rule)"}', case, y, ex)
            worst, share = max(worst, ratio), max(share, b or 0.0)
        groups[Q.opt_id(o)] = [labels for _, labels in distinct]
        for cfg in tiles if wide else ():
            assert any(f'tile {cfg} wide' in g and f'tile {cfg} narrow' in g for g in groups[Q.opt_id(o)]), \
                f'{case.name} {Q.opt_id(o)} tile {cfg}: the wide and the narrow epilogue differ: {groups[Q.opt_id(o)]}'
    return worst, share, groups


def assert_tiles_identical(case, groups, tiles):
    """Tile against tile.  Under an override plan_conv plans no split of K, and every tile walks K in the same order of 16-element MFMA
    steps into the same fp32 accumulators, so all overridden tiles store identical bytes; the rule's own tile joins them unless it splits
    K (the partial sums are then added in another order and only the reference comparison holds for it; measured: identical there too
    with e4m3 operands, a few bytes apart in one option of the bf16 form of k3_c128_n256)."""
    split = (case.name.rsplit('_', 1)[0], case.form) in Q.SPLIT_K
    for oid, gs in groups.items():
        first = next(g for g in gs if any(l.split()[1] == str(tiles[1]) for l in g))
        missing = [t for t in tiles[1 if split else 0:] if not any(l.split()[1] == str(t) for l in first)]
        assert not missing, f'{case.name} {oid}: tiles {missing} differ from tile {tiles[1]}: {gs}'


E4M3_IN = [c for c in Q.ROUNDING if c.in_t == 'e4m3']
FORM_A = [c for c in Q.ROUNDING if c.in_t == 'bf16']


@pytest.mark.parametrize('case', E4M3_IN, ids=lambda c: c.name)
def test_e4m3_operands(L, case):
    """forms b, c, d and f: the rule's tile and tiles 91 .. 94, wide and narrow epilogue, the validation kernel; split K where the rule
    plans it (ivx_conv_workspace_bytes > 0 exactly there: 3x3 from 128 channels at 234 rows, 1x1 from 1024 channels at 35 rows -- 512
    channels are 8 slabs of 64 bytes, below the 16 the rule asks for)"""
    for o in case.options():
        nb = workspace_bytes(L, case, o)
        assert (nb > 0) == ((case.name.rsplit('_', 1)[0], case.form) in Q.SPLIT_K), f'{case.name} {Q.opt_id(o)}: ivx_conv_workspace_bytes = {nb}'
    worst, share, groups = run_case(L, case, E4M3_TILES)
    print(f'gpu e4m3 operands {case.name}: worst error / bound = {worst:.3f}, largest boundary share {share:.4f}, identical runs {groups}')
    assert_tiles_identical(case, groups, E4M3_TILES)


@pytest.mark.parametrize('case', FORM_A, ids=lambda c: c.name)
def test_bf16_operands_e4m3_output(L, case):
    """form a (one case with a signed input): conv_epilogue_wide_fp8 from bf16 accumulators as NJ = 2 (tiles 74, 61) and NJ = 1 (66, 63),
    the narrow epilogue, the validation kernel; split K where the rule plans it (3x3 from 128 channels at 234 rows, 1x1 from 512 and
    1024 channels at 35 rows)"""
    for o in case.options():
        nb = workspace_bytes(L, case, o)
        assert (nb > 0) == ((case.name.rsplit('_', 1)[0], case.form) in Q.SPLIT_K), f'{case.name} {Q.opt_id(o)}: ivx_conv_workspace_bytes = {nb}'
    worst, share, groups = run_case(L, case, BF16_TILES)
    print(f'gpu bf16 operands, e4m3 output {case.name}: worst error / bound = {worst:.3f}, largest boundary share {share:.4f}, identical runs {groups}')
    assert_tiles_identical(case, groups, BF16_TILES)


def test_saturation_and_non_finite(L):
    """s_out from a quarter of the maximum and a NaN, +inf and -inf in the shift of one channel each, without and with the ReLU, on the
    rule's tile, on tile 91, on the narrow epilogue and on the validation kernel: beyond +-448 and for +-inf the bytes 0x7E / 0xFE, for
    the NaN a NaN byte without the ReLU and 0 with it"""
    case = Q.SATURATION.make()
    worst, share, groups = run_case(L, case, (0, 91))
    for o in case.options():
        ex = case.expect(o, *Q.folded_f32(case, o))
        assert 0.01 <= ex.saturated_share <= 0.5 and bool(ex.nan.any()) == (not o['relu'])
    print(f'gpu saturation / non-finite {case.name}: worst error / bound = {worst:.3f}, largest boundary share {share:.4f}, identical runs {groups}')


@pytest.mark.parametrize('name', Q.FUSED, ids=lambda n: n)
def test_fused_conv_folds_the_scales(L, name):
    """FusedConv (dtype / out_dtype / QTensor) against the unfolded driver -- BN scale and shift, s_in, s_w[co], s_out, s_res folded by the
    header's rule in fp64 -- with the ReLU, post_scale -1.25 and, where the form has one, the residual after the ReLU; a second call with
    half the input scale (another key of the _qvec cache) and a third with the first again"""
    from imvoxelnet_amd.conv import FusedConv, QTensor, FP8
    case = Q.BY_NAME[name].make()
    o = dict(relu=True, res='after' if case.has_res else None, post=-1.25)
    x, w, res = Q.to_device(case)
    w_real = torch.from_numpy((case.w_op * case.s_w[:, None, None, None, None])[:, 0].transpose(0, 3, 1, 2).astype(np.float32))       # [Cout, Cin, k, k]
    bn = (torch.from_numpy(case.bn_scale.astype(np.float32)), torch.from_numpy(case.bn_shift.astype(np.float32)), torch.zeros(case.cout),
          torch.full((case.cout,), 1.0 - 1e-5))                                  # gamma / sqrt(var + eps) = gamma
    FusedConv.calib = {'k': case.s_out(o) * Q.FMAX}
    try:
        fc = FusedConv(w_real, None, bn, stride=case.s, padding=case.k // 2, relu=True, dims=2, dtype=Q.TORCH_DT[case.in_t], out_dtype=Q.TORCH_DT[case.out_t],
                       key='k').to('cuda')
    finally:
        FusedConv.calib = None
    assert fc.layout == case.layout and same_bytes(fc.w, w), 'FusedConv quantised or packed the filters differently'
    if case.in_t == 'e4m3':
        assert float(np.abs(fc.w_scale.numpy().astype(np.float64) / case.s_w - 1.0).max()) < 1e-6
    if case.out_t == 'e4m3':
        assert abs(fc.out_scale / case.s_out(o) - 1.0) < 1e-12
    rq = None if res is None else QTensor(res, case.s_res) if case.res_t == 'e4m3' else res
    worst = 0.0
    for s_in in (case.s_in, 0.5 * case.s_in, case.s_in):
        xin = QTensor(x, s_in) if case.in_t == 'e4m3' else x
        if case.in_t != 'e4m3' and s_in != case.s_in:
            continue                                                             # (a bf16 input carries no scale)
        y = fc(xin, res=rq, res_after_act=o['res'] == 'after', post_scale=o['post'])
        if case.out_t == 'e4m3':
            assert isinstance(y, QTensor) and y.data.dtype == FP8 and y.scale == fc.out_scale
            y = y.data
        ratio, _ = compare(f'FusedConv {name} s_in {s_in / case.s_in:g} x', case, y, case.expect_unfolded(o, s_in))
        worst = max(worst, ratio)
    assert case.in_t != 'e4m3' or len(fc._qvec) == 2
    print(f'gpu FusedConv {name}: worst error / bound = {worst:.3f}')
