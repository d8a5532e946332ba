"""The conv epilogue without a device: the fp64 reference of tests/ref_conv.py against torch in fp64, the nearest-neighbour indices of
res_mode 2, the condition that lets every case tell a wrong epilogue order from the right one, and the fp32 direct driver on the CPU
restatement of the C-ABI (oracle/cpu_abi, ivx_conv_fwd_ws; fp32 only, no Winograd there) -- so the reference, the cases and the drivers
are proved before tests/test_gpu_conv_epilogue.py runs them on the HIP library."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref_conv as R
import ref_pair as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    spec = importlib.util.spec_from_file_location('ivx_cpu_abi_host', os.path.join(ROOT, 'oracle', 'cpu_abi', 'host.py'))
    host = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(host)
    return host.load()


@pytest.fixture(scope='module')
def be(lib):
    return R.HostBackend(lib)


def _ncdhw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double().permute(0, 4, 1, 2, 3)


# ---------------------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize('kernel,stride,padding', [((3, 3, 3), (1, 1, 1), (1, 1, 1)), ((3, 3, 3), (1, 1, 2), (1, 1, 1)), ((3, 3, 3), (2, 2, 2), (1, 1, 1)),
                                                   ((1, 3, 3), (1, 2, 1), (0, 1, 0)), ((3, 1, 2), (2, 1, 1), (0, 0, 1)), ((1, 1, 1), (1, 1, 1), (0, 0, 0))])
def test_reference_matches_torch_fp64(kernel, stride, padding):
    """ref_conv.conv3d against F.conv3d in fp64 with the epilogue spelled in torch: every kernel / stride / padding per axis, both residual
    orders, a negative post_scale, with and without the ReLU"""
    r = np.random.RandomState(sum(kernel) + 7 * sum(stride))
    x, w = r.randn(2, 5, 7, 6, 5), r.randn(4, *kernel, 5)
    sc, sh = r.rand(4) + 0.5, r.randn(4)
    conv = F.conv3d(_ncdhw(x), _ncdhw(w), None, stride, padding).permute(0, 2, 3, 4, 1)
    v = conv * torch.from_numpy(sc) + torch.from_numpy(sh)
    res = r.randn(*v.shape)
    for after in (False, True):
        for relu in (False, True):
            want = v if after else v + torch.from_numpy(res)
            want = want.clamp_min(0) if relu else want
            want = (want + torch.from_numpy(res) if after else want) * -1.25
            got = R.conv3d(x, w, sc, sh, kernel, stride, padding, relu, res, 1, after, -1.25)
            assert got.shape == tuple(want.shape) and float(np.abs(got - want.numpy()).max()) < 1e-12
    assert float(np.abs(R.conv3d(x, w, None, None, kernel, stride, padding) - conv.numpy()).max()) < 1e-12


def test_reference_transposed_conv_matches_torch_fp64():
    """out_mode 1 against F.conv_transpose3d(kernel 2, stride 2) in fp64: the GEMM's column order and the scatter, then BN + residual +
    ReLU + post_scale on the scattered tensor"""
    r = np.random.RandomState(3)
    ci, co = 6, 5
    x, wt = r.randn(2, 3, 5, 4, ci), r.randn(ci, co, 2, 2, 2)                         # torch layout [Cin, Cout, 2, 2, 2]
    sc, sh = r.rand(co) + 0.5, r.randn(co)
    up = F.conv_transpose3d(_ncdhw(x), torch.from_numpy(wt), None, 2).permute(0, 2, 3, 4, 1).numpy()
    res = r.randn(*up.shape)
    w = wt.transpose(2, 3, 4, 1, 0).reshape(8 * co, 1, 1, 1, ci)                      # column n = ((a*2+e)*2+f)*Cout + co
    got = R.conv3d(x, w, sc, sh, (1, 1, 1), relu=True, res=res, res_mode=1, res_after_act=True, post_scale=0.5, out_mode=1)
    want = (np.maximum(up * sc + sh, 0) + res) * 0.5
    assert got.shape == (2, 6, 10, 8, co) and float(np.abs(got - want).max()) < 1e-12


def test_nearest_indices_known_answers():
    """res_mode 2: the indices of F.interpolate(mode='nearest') on an fp32 index tensor -- known answers, equality with exact rational floor
    at every size the cases use, and the reference's gather against F.interpolate on the residual itself"""
    assert R.nearest_index(12, 6).tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5]
    assert R.nearest_index(5, 5).tolist() == [0, 1, 2, 3, 4]
    assert R.nearest_index(13, 7).tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6]
    assert R.nearest_index(21, 11).tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10]
    assert R.nearest_index(12, 7).tolist() == [0, 0, 1, 1, 2, 2, 3, 4, 4, 5, 5, 6]
    for (ho, wo), (rh, rw) in R.RES2_SIZES:
        for n_out, n_in in ((ho, rh), (wo, rw)):
            assert np.array_equal(R.nearest_index(n_out, n_in), R.nearest_index_exact(n_out, n_in)), (n_out, n_in)
    assert {tuple(c.sp[1:]) + tuple(c.res_hw) for c in R.ALL_CASES if c.res_mode == 2} <= {a + b for a, b in R.RES2_SIZES}
    r = np.random.RandomState(5).randn(2, 1, 7, 11, 3)
    want = F.interpolate(torch.from_numpy(r[:, 0]).permute(0, 3, 1, 2), size=(13, 21), mode='nearest').permute(0, 2, 3, 1).numpy()
    assert np.array_equal(R.residual_at_output(r, 2, (2, 1, 13, 21, 3))[:, 0], want)


def test_reference_pair_conv2d_residual_after_act():
    """ref_pair.conv2d with res_after_act against ref_conv.conv3d"""
    r = np.random.RandomState(9)
    x, w = r.randn(1, 5, 6, 3), r.randn(4, 9, 3)
    sc, sh, res = r.rand(4) + 0.5, r.randn(4), r.randn(1, 5, 6, 4)
    for after in (False, True):
        got = P.conv2d(x, w, sc, sh, 3, 1, 1, True, res, 1, -1.25, after)
        want = R.conv3d(x[:, None], w.reshape(4, 1, 3, 3, 3), sc, sh, (1, 3, 3), (1, 1, 1), (0, 1, 1), True, res[:, None], 1, after, -1.25)[:, 0]
        assert float(np.abs(got - want).max()) < 1e-12
    assert float(np.abs(P.conv2d(x, w, sc, sh, 3, 1, 1, True, res, 1, 1.0, True) - P.conv2d(x, w, sc, sh, 3, 1, 1, True, res, 1, 1.0, False)).max()) > 0.1


# ---------------------------------------------------------------------------------------------------------------- the condition on the inputs
@pytest.mark.parametrize('case', R.ALL_CASES, ids=lambda c: c.name)
def test_cases_tell_the_orders_apart(case):
    """For every option with a residual and the ReLU the reference under the other residual order, and for every option whose post_scale
    does not commute, the reference that multiplies first, lies more than 100 x the case's tolerance away on >= 25 % of the elements."""
    fr = R.discrimination(case)
    res = [v[0] for v in fr.values() if v[0] is not None]
    post = [v[1] for v in fr.values() if v[1] is not None]
    print(f'{case.name}: smallest separated fraction: residual order {min(res) if res else float("nan"):.3f} over {len(res)} options, '
          f'multiplier order {min(post):.3f} over {len(post)} options')
    if case.rounding is not None:                       # the bf16-output bar is wider: the condition must hold under it as well
        R.discrimination(case, R.TOL_BF16_OUT)


# ---------------------------------------------------------------------------------------------------------------- the CPU restatement
@pytest.mark.parametrize('case', R.HOST_CASES, ids=lambda c: c.name)
def test_direct_driver_on_the_cpu_restatement(be, case):
    """ivx_conv_fwd_ws of oracle/cpu_abi through ref_conv.run_direct, every option, both filter layouts where the channels allow"""
    worst = R.run_direct_options(be, case, 0)
    if case.cin % 32 == 0:
        worst = max(worst, R.run_direct_options(be, case, 1))
    print(f'cpu {case.name}: worst error / tolerance over the option set = {worst:.3f}')


@pytest.mark.parametrize('order', ['swapped', 'scaled_early'])
def test_check_rejects_a_wrong_order(order):
    """ref_conv.check fails on a tensor computed in a wrong order (the checker itself is not vacuous)"""
    case = R.DIRECT[0]
    o = dict(after=True, post=-1.25, relu=True)
    with pytest.raises(AssertionError):
        R.check('wrong order', case.ref(o, order).astype(np.float32), case.ref(o), R.TOL_F32)
    nan = case.ref(o).astype(np.float32)
    nan[0, 0, 0, 0, 0] = np.nan
    with pytest.raises(AssertionError):
        R.check('unwritten element', nan, case.ref(o), R.TOL_F32)


# ---------------------------------------------------------------------------------------------------------------- ivx_conv_fwd_pio
@pytest.fixture(scope='module')
def pbe(lib):
    return P.HostBackend(lib)


@pytest.mark.parametrize('case', P.AFTER_ACT_CONV, ids=lambda c: f'{c[0]}x{c[1][0]}x{c[1][1]}-{c[2]}-{c[3]}-k{c[4]}')
def test_pio_residual_after_act_tight(pbe, case):
    """ivx_conv_fwd_pio with res_after_act on cases of ref_pair's table (1x1, 3x3, the split-K shape), against ref_pair's derived bound"""
    worst, L = P.run_tight_conv(pbe, case, 'below', True)
    print(f'cpu tight conv res_after_act {case}: worst error / bound = {worst:.3f}, L = {L:.5f}')


@pytest.mark.parametrize('k', [1, 3])
def test_pio_residual_after_act_signed(pbe, k):
    worst = P.run_signed_after_act_conv(pbe, k)
    print(f'cpu conv {k}x{k} res_after_act on signed data: worst error / bound = {worst:.3f}')
