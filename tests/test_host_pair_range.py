"""The scale rule of the pair tensors at both ends of its contract, on the CPU restatement of the C-ABI (oracle/cpu_abi: ivx_conv_fwd_pio,
both bottlenecks, ivx_stem_pool_fwd_pair, ivx_maxpool2d_fwd_pair, ivx_dcn_im2col_fwd_pair and the host-only packers, which are the
product's own code) against the fp64 references of tests/ref_pair.py.  No device: this proves the references, the construction of the
cases, the conditions on them (L <= 1.01 on the tight side, L within a factor 2 of the target on the loose side) and the derived bounds
before a GPU is involved; tests/test_gpu_pair_range.py runs the same drivers on the HIP library."""
import importlib.util
import os

import numpy as np
import pytest

import ref_pair as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDES = ['below', 'above']


@pytest.fixture(scope='module')
def be():
    spec = importlib.util.spec_from_file_location('ivx_cpu_abi_host', os.path.join(ROOT, 'oracle', 'cpu_abi', 'host.py'))
    host = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(host)
    return P.HostBackend(host.load())


# ---------------------------------------------------------------------------------------------------------------- the module itself
def test_formats_and_storage_term():
    """The encoder and decoder are inverse on 22-bit values, the filter layout is the one include/imvoxel.h states, and the storage term
    delta(T) = max(2^-22, 2^-39 L) max|T| holds for L = 1 .. 2^38 at three places of the binade of s * bound: the worst ratio is 1.000 of
    it, reached at s * bound = 2^14, and it still holds where the hi half goes subnormal (2^-40 L is exceeded there by a factor of two)."""
    r = np.random.RandomState(0)
    x = (r.randn(3, 5, 32) * np.logspace(-3, 2, 32)).astype(np.float32)
    s = P.pow2_scale(np.abs(x).max())
    assert 2.0 ** 14 <= s * np.abs(x).max() < 2.0 ** 15
    d = P.pair_encode(x, s)
    v = P.pair_decode(d, s)
    assert d.shape == (3, 5, 64) and np.array_equal(P.pair_decode(P.pair_encode(v.astype(np.float32), s), s), v)
    assert np.array_equal(d[..., 0:16].astype(np.float64) + d[..., 16:32].astype(np.float64), v[..., :16] * s)
    assert float((np.abs(v - x) - (np.abs(x) * 2.0 ** -22 + 2.0 ** -25 / s)).max()) <= 0
    w = r.randn(8, 9, 64).astype(np.float32)
    f = P.filters_encode(w, 2.0 ** 12)
    assert f.shape == (8, 2, 9, 64) and float(np.abs(P.filters_decode(f) / 2.0 ** 12 - w).max()) <= 2.0 ** -21 * np.abs(w).max()
    assert float(f[3, 1, 4, 32 + 5]) == float(np.float16(w[3, 4, 32 + 16 + 5] * 2.0 ** 12))          # chunk 1, tap 4, second group of 16, hi half
    worst = 0.0
    for e in range(0, 39):
        L = 2.0 ** e
        for place in (1.0, 1.37, 2.0 - 2.0 ** -20):                     # s * bound = 2^14 * place
            tmax = 2.0 ** 14 * place / L                                # s * max|T|, s = 1
            t = (r.uniform(-1, 1, 4096) * tmax).astype(np.float32)
            t[0] = tmax
            err = float(np.abs(P.pair_round(t, 1.0) - t.astype(np.float64)).max())
            worst = max(worst, err / (max(2.0 ** -22, 2.0 ** -39 * L) * float(np.abs(t).max())))
    print(f'storage term: worst error / (max(2^-22, 2^-39 L) max|T|) over L = 1 .. 2^38 = {worst:.3f}')
    assert 0.5 < worst <= 1.0


def test_references_known_answers():
    """conv2d against a direct loop, the residual forms, post_scale and the pool"""
    r = np.random.RandomState(1)
    x, w = r.randn(1, 5, 6, 3), r.randn(4, 9, 3)
    sc, sh = r.rand(4) + 0.5, r.randn(4)
    res = r.randn(1, 2, 3, 4)
    got = P.conv2d(x, w, sc, sh, 3, 2, 1, True, res, 2, 0.5)
    assert got.shape == (1, 3, 3, 4)
    for (oy, ox, co) in [(0, 0, 0), (2, 2, 3), (1, 2, 1)]:
        acc = sum(x[0, 2 * oy - 1 + ky, 2 * ox - 1 + kx] @ w[co, ky * 3 + kx] for ky in range(3) for kx in range(3)
                  if 0 <= 2 * oy - 1 + ky < 5 and 0 <= 2 * ox - 1 + kx < 6)
        want = max(acc * sc[co] + sh[co] + res[0, oy * 2 // 3, ox * 3 // 3, co], 0) * 0.5
        assert abs(got[0, oy, ox, co] - want) < 1e-12
    m = P.maxpool(-np.arange(12.0).reshape(1, 3, 4, 1))
    assert m.shape == (1, 2, 2, 1) and m.reshape(-1).tolist() == [0.0, -1.0, -4.0, -5.0]
    assert P.allowed_scales(2.0 ** 10 * (1 - 1e-4), np.float32(2.0 ** 10 * (1 - 1e-4))) == (2.0 ** 5, {2.0 ** 5})
    assert P.allowed_scales(2.0 ** 10 * (1 - 1e-9), np.float32(2.0 ** 10)) == (2.0 ** 5, {2.0 ** 5, 2.0 ** 4})


# ---------------------------------------------------------------------------------------------------------------- host-only packers
def test_pack_filters_bounds(be):
    worst = [0.0, 0.0]
    for name, w, sc, sh in P.pack_cases():
        ew, es = P.check_pack(be, name, w, sc, sh)
        worst = [max(worst[0], ew), max(worst[1], es)]
    print(f'ivx_pair_pack_filters: wbound / exact - 1 <= {worst[0]:.3e}, sbound / exact - 1 <= {worst[1]:.3e} (allowed 2^-20 = {2.0 ** -20:.3e})')


def test_pack_proj_and_stem_bounds(be):
    worst = 0.0
    for P_, cin, kind in [(32, 32, 'random'), (64, 64, 'random'), (64, 64, 'tight'), (128, 512, 'random'), (512, 2048, 'tight'), (64, 2048, 'mixed')]:
        r = np.random.RandomState(P_ + cin)
        mk = {'random': lambda co, ci: P.random_filters(r, co, 1, ci), 'tight': lambda co, ci: P.tight_filters(r, co, 1, ci, 0.75, 0.125),
              'mixed': lambda co, ci: P.mixed_filters(r, co, 1, ci, 0.75, 0.125)[:3]}[kind]
        (w3, s3, t3), (wd, sd, td) = mk(4 * P_, P_), mk(4 * P_, cin)
        worst = max(worst, *P.check_pack_proj(be, f'proj {kind} P {P_} Cin {cin}', w3[:, 0], s3, t3, wd[:, 0], sd, td))
    for seed in range(3):
        r = np.random.RandomState(seed)
        w = (r.randn(64, 3, 7, 7) * (2.0 / 147) ** 0.5).astype(np.float32)
        worst = max(worst, *P.check_pack_stem(be, f'stem random {seed}', w, (r.rand(64) + 0.5).astype(np.float32), (r.randn(64) * 0.1).astype(np.float32)))
    w = np.abs(w)
    w[9] = 0.0
    worst = max(worst, *P.check_pack_stem(be, 'stem non-negative, dead channel', w, np.ones(64, np.float32), np.full(64, -2.0 ** 20, np.float32)))
    print(f'ivx_bottleneck_proj_pack / stem: bound term / exact - 1 <= {worst:.3e} (allowed 2^-20)')


# ---------------------------------------------------------------------------------------------------------------- tight side
@pytest.mark.parametrize('side', SIDES)
@pytest.mark.parametrize('case', P.TIGHT_CONV, ids=lambda c: f'{c[0]}x{c[1][0]}x{c[1][1]}-{c[2]}-{c[3]}-k{c[4]}s{c[5]}{c[6]}')
def test_tight_conv_cpu(be, case, side):
    worst, L = P.run_tight_conv(be, case, side)
    print(f'cpu tight conv {case} {side}: worst error / bound = {worst:.3f}, L = {L:.5f}')


@pytest.mark.parametrize('side', SIDES)
@pytest.mark.parametrize('case', P.TIGHT_BOTTLENECK, ids=lambda c: f'{"proj" if c[0] else "identity"}-P{c[1]}-{c[2]}x{c[3]}x{c[4]}')
def test_tight_bottleneck_cpu(be, case, side):
    worst, Ls = P.run_tight_bottleneck(be, case, side)
    print(f'cpu tight bottleneck {case} {side}: worst error / bound = {worst:.3f}, L1 L2 L3 = {Ls[0]:.5f} {Ls[1]:.5f} {Ls[2]:.5f}')


@pytest.mark.parametrize('side', SIDES)
@pytest.mark.parametrize('case', P.TIGHT_STEM, ids=lambda c: f'{c[0]}x{c[1]}x{c[2]}')
def test_tight_stem_cpu(be, case, side):
    worst, L = P.run_tight_stem(be, case, side)
    print(f'cpu tight stem {case} {side}: worst error / bound = {worst:.3f}, L = {L:.5f}')


# ---------------------------------------------------------------------------------------------------------------- loose side
@pytest.mark.parametrize('how,target', P.LOOSE_TARGETS, ids=lambda v: v if isinstance(v, str) else f'L2^{int(np.log2(v))}')
@pytest.mark.parametrize('case', P.LOOSE_CONV, ids=lambda c: f'{c[0]}x{c[1][0]}x{c[1][1]}-k{c[4]}')
def test_loose_conv_cpu(be, case, how, target):
    worst, L = P.run_loose_conv(be, case, how, target)
    print(f'cpu loose conv {case} {how}: worst error / bound = {worst:.3f}, L = 2^{np.log2(L):.2f}')


@pytest.mark.parametrize('target', [2.0 ** 10, 2.0 ** 18, 2.0 ** 24], ids=lambda v: f'L2^{int(np.log2(v))}')
def test_loose_stem_cpu(be, target):
    worst, L = P.run_loose_stem(be, target)
    print(f'cpu loose stem: worst error / bound = {worst:.3f}, L = 2^{np.log2(L):.2f}')


@pytest.mark.parametrize('target', [2.0 ** 10, 2.0 ** 20], ids=lambda v: f'L2^{int(np.log2(v))}')
@pytest.mark.parametrize('case', P.LOOSE_BOTTLENECK, ids=lambda c: 'proj' if c[0] else 'identity')
def test_loose_bottleneck_cpu(be, case, target):
    worst, chain, Ls = P.run_loose_bottleneck(be, case, target)
    print(f'cpu loose bottleneck {case}: worst error / bound = {worst:.3f}, layer-wise chain error / (2e-5 range) = {chain:.3f}, '
          f'L1 L2 L3 = 2^{np.log2(Ls[0]):.2f} 2^{np.log2(Ls[1]):.2f} 2^{np.log2(Ls[2]):.2f}')


@pytest.mark.parametrize('below', [20, 26])
def test_loosely_scaled_input_cpu(be, below):
    out = [P.run_loose_input_conv(be, 1, below), P.run_loose_input_conv(be, 3, below), P.run_loose_input_bottleneck(be, False, below),
           P.run_loose_input_bottleneck(be, True, below)]
    dcn = P.run_loose_input_dcn(be, below)
    print(f'cpu input scaled 2^{below} below: error / (2e-5 range) conv 1x1 {out[0]:.3f}, 3x3 {out[1]:.3f}, identity block {out[2]:.3f}, '
          f'projection block {out[3]:.3f}; dcn columns error / bound = {dcn:.3f}')


# ---------------------------------------------------------------------------------------------------------------- one model-level case
@pytest.mark.parametrize('name', P.MODEL_CASES)
def test_model_dead_channels_operand_modes_cpu(name):
    """ref_pair.run_model_operand_modes on the CPU restatement: the handle with pair operands in the trunk against the same handle on fp32
    products (the project's own code on other arithmetic, not an fp64 reference), dead BatchNorm channels and a saturated image block."""
    import plan_worker as W
    ratios = P.run_model_operand_modes(W.load_lib('cpu'), 'cpu', name)
    print(f'cpu model {name}: error / (2e-4 range) ' + ', '.join(f'{k} {v:.3f}' for k, v in ratios.items()))
