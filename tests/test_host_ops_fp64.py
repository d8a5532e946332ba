"""The CPU restatement of the op-level C-ABI (oracle/cpu_abi) against the plain fp64 references of tests/ref_ops.py, on the small cases and
with the bounds of tests/test_gpu_ops_fp64.py: DCNv2 columns (fp32, pair), max-pool, trilinear x2, the layout changes, the global mean
and max |x|.  No device: this proves the references and the bounds before a GPU is involved, and it tests the restatement itself, which
is otherwise compared only through whole models."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import ref_ops as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = 64


@pytest.fixture(scope='module')
def L():
    spec = importlib.util.spec_from_file_location('ivx_cpu_abi_host', os.path.join(ROOT, 'oracle', 'cpu_abi', 'host.py'))
    host = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(host)
    return host.load()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _ok(L, rc, what):
    assert rc == 0, f'{what}: {L.ivx_last_error().decode()}'


def _slots_max(slots):
    return float(slots[:SLOTS].view(np.float32).max())


check_dcn, check_shares = R.check_dcn, R.check_shares


def _map(seed, B, H, W, Cn):
    return (np.random.RandomState(seed).randn(B, H, W, Cn) * 1.7).astype(np.float32)


def test_dcn_columns_fp32_cpu(L):
    worst = 0.0
    for seed, B, H, W, Cn, k, s, p, d, omc in R.dcn_small_cases('f32'):
        x = _map(seed, B, H, W, Cn)
        om = R.dcn_offsets_masks(seed + 1, B, H, W, k, s, p, d, omc)
        Ho, Wo = om.shape[1:3]
        col = np.full((B, Ho, Wo, k * k, Cn), np.nan, np.float32)
        _ok(L, L.ivx_dcn_im2col_fwd(_p(x), _p(om), B, H, W, Cn, k, k, s, p, d, omc, _p(col), None), 'ivx_dcn_im2col_fwd')
        ref, A = R.dcn_columns(x, om, k, s, p, d)
        name = f'cpu dcn fp32 B{B} {H}x{W} C{Cn} k{k} s{s} p{p} d{d} omc{omc}'
        check_shares(name, om, ref, H, W, k, s, p, d)
        worst = max(worst, check_dcn(name, col, ref, A))
    print(f'cpu dcn fp32: worst ratio {worst:.3f} of K = {R.K_DCN}')


def test_dcn_columns_fp32_cpu_nan_in_the_map(L):
    B, H, W, Cn, k, s, p, d = 2, 9, 11, 8, 3, 1, 1, 1
    x = _map(5, B, H, W, Cn)
    x[0, 0, 0, 1] = x[1, 4, 5, 2] = x[1, 8, 10, 7] = np.nan
    om = R.dcn_offsets_masks(6, B, H, W, k, s, p, d, 27)
    col = np.zeros((B, H, W, 9, Cn), np.float32)
    _ok(L, L.ivx_dcn_im2col_fwd(_p(x), _p(om), B, H, W, Cn, k, k, s, p, d, 27, _p(col), None), 'ivx_dcn_im2col_fwd')
    ref, A = R.dcn_columns(x, om, k, s, p, d)
    assert 0 < int(np.isnan(ref).sum()) < ref.size // 4
    check_dcn('cpu dcn fp32, NaN in the map', col, ref, A)


def test_dcn_columns_pair_cpu(L):
    for seed, B, H, W, Cn, k, s, p, d, omc in R.dcn_small_cases('pair'):
        x = _map(seed, B, H, W, Cn)
        scale = R.pow2_scale(np.abs(x).max())
        xp = R.pair_encode(x, scale)
        xd = R.pair_decode(xp, scale)
        om = R.dcn_offsets_masks(seed + 1, B, H, W, k, s, p, d, omc)
        Ho, Wo = om.shape[1:3]
        col = np.zeros((B, Ho, Wo, 2 * k * k * Cn), np.float16)
        sc_in, sc_out, slots = np.array([scale], np.float32), np.zeros(1, np.float32), np.zeros(SLOTS, np.uint32)
        _ok(L, L.ivx_dcn_im2col_fwd_pair(_p(xp), _p(sc_in), _p(om), B, H, W, Cn, k, k, s, p, d, omc, _p(col), _p(sc_out), _p(slots), None),
            'ivx_dcn_im2col_fwd_pair')
        assert float(sc_out[0]) == scale
        got = R.pair_decode(col, scale).reshape(B * Ho * Wo, k * k, Cn)
        ref, A = R.dcn_columns(xd, om, k, s, p, d)
        extra = 2.0 ** -21 * np.abs(ref) + 2.0 ** -24 / scale
        check_dcn(f'cpu dcn pair B{B} {H}x{W} C{Cn} k{k} s{s} p{p} d{d} omc{omc}', got, ref, A, extra)
        # the recorded maximum is the maximum before the split: after the split's rounding it is the maximum of the decoded columns
        assert R.pair_round(_slots_max(slots), scale) == float(np.abs(got).max())


def test_maxpool_fp32_cpu(L):
    for seed, B, H, W, Cn, k, s, p in R.pool_small_cases((4, 16, 64, 100)):
        x = R.pool_input(seed, (B, H, W, Cn))
        ref = R.maxpool2d(x, k, s, p)
        out = np.zeros(ref.shape, np.float32)
        _ok(L, L.ivx_maxpool2d_fwd(_p(x), B, H, W, Cn, k, s, p, _p(out), None), 'ivx_maxpool2d_fwd')
        assert np.array_equal(np.isnan(out), np.isnan(ref)) and np.array_equal(out.view(np.uint32)[~np.isnan(ref)], ref.view(np.uint32)[~np.isnan(ref)]), \
            (B, H, W, Cn, k, s, p)


def test_maxpool_pair_cpu(L):
    """negative inputs too: the scale is the one of the bound, the split rounds to 22 bits, the recorded maximum is max |pool|"""
    for seed, B, H, W, Cn, k, s, p in R.pool_small_cases((16, 64)):
        x = R.pool_input(seed, (B, H, W, Cn), special=0.0)
        ref = R.maxpool2d(x, k, s, p)
        amax_in = np.zeros(SLOTS, np.uint32)
        amax_in.view(np.float32)[3] = 2.0
        wb, sb = 7.5, 0.25
        out = np.zeros(ref.shape[:-1] + (2 * Cn,), np.float16)
        sc, slots = np.zeros(1, np.float32), np.zeros(SLOTS, np.uint32)
        _ok(L, L.ivx_maxpool2d_fwd_pair(_p(x), B, H, W, Cn, k, s, p, _p(out), _p(amax_in), C.c_float(wb), C.c_float(sb), _p(sc), _p(slots), None),
            'ivx_maxpool2d_fwd_pair')
        assert float(sc[0]) == R.pow2_scale(np.float32(np.float32(2.0) * np.float32(wb) + np.float32(sb)) * np.float32(1.001))
        got = R.pair_decode(out, float(sc[0]))
        assert float(np.abs(got.astype(np.float64) - ref).max()) <= float(np.abs(ref).max()) * 2.0 ** -21 + 2.0 ** -24 / float(sc[0])
        assert _slots_max(slots) == float(np.abs(ref).max())


def test_trilinear2x_cpu(L):
    worst = 0.0
    for B, D, H, W, Cn in R.TRI_CASES:
        x = (np.random.RandomState(D * 100 + H * 10 + W).randn(B, D, H, W, Cn) * 2).astype(np.float32)
        out = np.zeros((B, 2 * D, 2 * H, 2 * W, Cn), np.float32)
        _ok(L, L.ivx_upsample_trilinear2x_fwd(_p(x), B, D, H, W, Cn, _p(out), None), 'ivx_upsample_trilinear2x_fwd')
        ref, M = R.trilinear2x(x)
        d = np.abs(out - ref)
        worst = max(worst, float((d / (R.U * M)).max()))
        assert np.all(d <= R.trilinear_bound(M)), (B, D, H, W, Cn, float((d / R.trilinear_bound(M)).max()))
    print(f'cpu trilinear x2: worst |got - ref| / (2^-24 max|corner|) = {worst:.3f} of K = {R.K_TRI}')


def test_layout_cpu(L):
    for B, Cn, S, pad in [(B, Cn, S, 4) for B, Cn, S in R.LAYOUT_IMAGE_CASES] + R.LAYOUT_TILE_CASES:
        cp = Cn if pad is None else (Cn + pad - 1) // pad * pad
        x = np.random.RandomState(Cn * 1000 + S).randn(B, Cn, S).astype(np.float32)
        x[0, 0, 0] = -9.25
        ref = R.nchw_to_nhwc(x, cp)
        for with_amax in (False, True):
            out, slots = np.full((B, S, cp), np.nan, np.float32), np.zeros(SLOTS, np.uint32)
            if with_amax:
                _ok(L, L.ivx_nchw_to_nhwc_amax(_p(x), B, Cn, C.c_int64(S), cp, _p(out), _p(slots), None), 'ivx_nchw_to_nhwc_amax')
                assert _slots_max(slots) == R.amax(x) == 9.25
            else:
                _ok(L, L.ivx_nchw_to_nhwc(_p(x), B, Cn, C.c_int64(S), cp, _p(out), None), 'ivx_nchw_to_nhwc')
            assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)), (B, Cn, S, pad, with_amax)
        back = np.zeros((B, cp, S), np.float32)
        _ok(L, L.ivx_nhwc_to_nchw(_p(ref), B, C.c_int64(S), cp, _p(back), None), 'ivx_nhwc_to_nchw')
        assert np.array_equal(back, R.nhwc_to_nchw(ref)) and np.array_equal(back[:, :Cn], x) and not back[:, Cn:].any()


def test_layout_amax_ignores_nan_cpu(L):
    """include/imvoxel.h: ivx_nchw_to_nhwc_amax takes the maximum over the non-NaN elements; an Inf counts."""
    x = np.random.RandomState(2).randn(2, 3, 64).astype(np.float32)
    x[1, 2, 5] = np.nan
    out, slots = np.zeros((2, 64, 4), np.float32), np.zeros(SLOTS, np.uint32)
    _ok(L, L.ivx_nchw_to_nhwc_amax(_p(x), 2, 3, C.c_int64(64), 4, _p(out), _p(slots), None), 'ivx_nchw_to_nhwc_amax')
    assert _slots_max(slots) == R.amax(x) and np.isnan(out[1, 5, 2])
    x[0, 1, 7] = -np.inf
    slots[:] = 0
    _ok(L, L.ivx_nchw_to_nhwc_amax(_p(x), 2, 3, C.c_int64(64), 4, _p(out), _p(slots), None), 'ivx_nchw_to_nhwc_amax')
    assert _slots_max(slots) == np.inf


def test_amax_f32_cpu(L):
    for n in R.AMAX_SIZES:
        for name, a in R.amax_inputs(n, n + 1).items():
            buf = np.zeros(max(n, 4), np.float32)
            buf[:n] = a
            slots = np.zeros(SLOTS, np.uint32)
            _ok(L, L.ivx_amax_f32(_p(buf), C.c_int64(n), _p(slots), None), 'ivx_amax_f32')
            assert _slots_max(slots) == R.amax(a), (n, name)
            for pos in sorted({0, n - 1, n - (n % 4), n // 2}):              # a NaN anywhere counts as Inf
                if 0 <= pos < n:
                    b = buf.copy()
                    b[pos] = np.nan
                    slots[:] = 0
                    _ok(L, L.ivx_amax_f32(_p(b), C.c_int64(n), _p(slots), None), 'ivx_amax_f32')
                    assert _slots_max(slots) == np.inf, (n, name, pos)
    slots = np.full(SLOTS, 0x3f800000, np.uint32)                              # n = 0: the slots are not touched
    _ok(L, L.ivx_amax_f32(_p(np.ones(4, np.float32)), C.c_int64(0), _p(slots), None), 'ivx_amax_f32')
    assert np.all(slots == 0x3f800000)


def test_global_avgpool_cpu(L):
    for S in R.AVGPOOL_S:
        for Cn in R.AVGPOOL_C:
            B = 1 + (S + Cn) % 3
            x = (np.random.RandomState(S * 7 + Cn).randn(B, S, Cn) * 2 + 0.5).astype(np.float32)
            out = np.full((B, Cn), np.nan, np.float32)
            _ok(L, L.ivx_global_avgpool_fwd(_p(x), B, C.c_int64(S), Cn, _p(out), None), 'ivx_global_avgpool_fwd')
            ref, mabs = R.global_mean(x)
            assert np.all(np.abs(out - ref) <= R.avgpool_bound(S, mabs)), (S, Cn)
