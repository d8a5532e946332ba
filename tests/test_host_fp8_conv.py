"""The e4m3 convolution reference of tests/ref_fp8.py without a device: the codec against torch.float8_e4m3fn on the CPU, the operation
against torch in fp64 on the dequantised tensors, the comparison rule against known answers, and the conditions on the cases -- every
wrong fold and wrong order is told apart, at most 10 % of a run's elements hold a rounding boundary, the saturation case saturates on a
measurable share -- so the reference, the cases and the rule are proved before tests/test_gpu_fp8_conv.py runs them on the HIP library."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref_conv as R
import ref_fp8 as Q

F8 = torch.float8_e4m3fn


def _torch_encode(v32):
    """x.clamp(-448, 448).to(torch.float8_e4m3fn) as bytes.  Clamp first: torch's own conversion does not saturate (a value beyond the
    range becomes NaN) and the header's store does."""
    return torch.from_numpy(np.ascontiguousarray(v32, np.float32)).clamp(-448.0, 448.0).to(F8).view(torch.uint8).numpy()


# ---------------------------------------------------------------------------------------------------------------- the codec
def test_decode_all_bytes():
    """all 256 bytes decode as torch's; 0x7F and 0xFF are the NaNs; there is no infinity; the extremes"""
    b = np.arange(256, dtype=np.uint8)
    want = torch.from_numpy(b).view(F8).double().numpy()
    got = Q.decode(b)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.flatnonzero(np.isnan(got)).tolist() == [0x7F, 0xFF]
    assert np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)]) and np.array_equal(np.signbit(got[~np.isnan(got)]), np.signbit(want[~np.isnan(want)]))
    assert not np.isinf(got).any() and got[0x7E] == 448.0 and got[0xFE] == -448.0 and got[0x01] == 2.0 ** -9 and got[0x08] == 2.0 ** -6
    assert np.signbit(got[0x80]) and got[0x80] == 0.0


def test_encode_matches_torch_after_the_clamp():
    """encode == x.clamp(-448, 448).to(torch.float8_e4m3fn), byte for byte, on every finite value, every midpoint (the ties) and its fp32
    neighbours on both sides, both zeros, +-448 and beyond, +-inf, and the subnormal range in steps of 2^-13 with the 2^-10 tie to zero.
    Clamp first: torch's own conversion does not saturate, the header's does."""
    fin = Q.decode(np.arange(0x7F, dtype=np.uint8))
    mid = Q.boundaries()
    assert len(mid) == 253 and np.all(np.diff(mid) > 0) and mid[126] == 0.0 and mid[127] == 2.0 ** -10 and mid[-1] == 432.0
    m32 = mid.astype(np.float32)
    assert np.array_equal(m32.astype(np.float64), mid)                                  # the midpoints are fp32 values
    sub = np.arange(-2 ** 8, 2 ** 8 + 1) * 2.0 ** -13                                   # -2^-5 .. 2^-5
    v = np.concatenate([fin, -fin, mid, np.nextafter(m32, np.float32(np.inf)), np.nextafter(m32, np.float32(-np.inf)), sub,
                        [0.0, -0.0, 448.0, -448.0, 448.0001, 463.9, 464.0, 480.0, 1e6, -1e6, np.inf, -np.inf, 2.0 ** -10, -2.0 ** -10, 3 * 2.0 ** -10]])
    got, want = Q.encode(v), _torch_encode(v)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, [(float(v[i]), hex(got[i]), hex(want[i])) for i in bad[:8]]
    assert Q.encode(2.0 ** -10) == 0x00 and Q.encode(-2.0 ** -10) == 0x80 and Q.encode(3 * 2.0 ** -10) == 0x02      # ties to even
    assert Q.encode(np.inf) == 0x7E and Q.encode(-np.inf) == 0xFE and Q.encode(-0.0) == 0x80
    assert (Q.encode(np.nan) & 0x7F) == 0x7F and (_torch_encode([np.nan])[0] & 0x7F) == 0x7F
    assert np.array_equal(Q.encode(fin), np.arange(0x7F)) and np.array_equal(Q.encode(-fin), np.arange(0x7F) | 0x80)      # the round trip


def test_ordinals_and_cells():
    """the signed code line: ordinals rise with the value, -0 sits below +0, the NaN bytes fall outside"""
    b = np.concatenate([np.arange(0xFE, 0x7F, -1), np.arange(0x7F)]).astype(np.uint8)   # -448 .. -0, +0 .. 448
    assert np.array_equal(Q.ordinal(b), np.arange(-127, 127)) and np.all(np.diff(Q.decode(b)) >= 0)
    assert Q.ordinal(0x7F) == 127 and Q.ordinal(0xFF) == -128
    assert Q.steps(0x80) == 0 and Q.steps(0x85) == -5 and Q.steps(0x7E) == 126
    assert Q.nearest_boundary(20.4) == 21.0 and Q.nearest_boundary(-1e-4) == 0.0 and Q.nearest_boundary(1000.0) == 432.0


# ---------------------------------------------------------------------------------------------------------------- the operation
@pytest.mark.parametrize('name', ['k3s2_c48_n144_d', 'k3_c48_n48_c', 'k1_c16_n16_b', 'k3_c48_n48_signed_a'])
def test_unfolded_driver_matches_torch_fp64(name):
    """Case.value on the header's fold against torch in fp64 on the real (dequantised) tensors: conv2d, the BN affine, the residual on
    its side of the ReLU, the multiplier, divided by the output's scale"""
    c = Q.BY_NAME[name].make()
    x = torch.from_numpy(c.x_op * c.s_in)[:, 0].permute(0, 3, 1, 2)
    w = torch.from_numpy(c.w_op * c.s_w[:, None, None, None, None])[:, 0].permute(0, 3, 1, 2)
    conv = F.conv2d(x, w, None, c.s, c.k // 2).permute(0, 2, 3, 1)[:, None]
    v = conv * torch.from_numpy(c.bn_scale) + torch.from_numpy(c.bn_shift)
    for o in c.options():
        r = torch.from_numpy(c.r_op * c.s_res) if c.has_res else 0.0
        t = v + r if o['res'] == 'before' else v
        t = t.clamp_min(0) if o['relu'] else t
        t = t + r if o['res'] == 'after' else t
        want = (t * o['post'] / c.s_out(o)).numpy()
        got = c.value(o, *c.fold(o))
        assert got.shape == want.shape and float(np.abs(got - want).max()) < 1e-9 * max(1.0, float(np.abs(want).max())), (name, Q.opt_id(o))
        if c.out_t == 'e4m3':
            assert abs(float(np.abs(got).max()) - 448.0) < 1e-9                          # calibrated on its own maximum
            assert float((c.expect_unfolded(o).want != Q.encode(want)).mean()) < 1e-3    # (an fp64 rounding on a tie apart at most)


def test_relu_turns_a_nan_into_zero():
    """the reference states the kernels' ReLU, v > 0 ? v : 0: a NaN becomes 0 before a late residual and the multiplier; without the ReLU
    it stays"""
    v, r = np.array([np.nan, -1.0, 2.0, np.nan]), np.array([0.5, 0.5, 0.5, -0.5])
    assert np.array_equal(Q.finish(v, None, True, False, -1.25), [-0.0, -0.0, -2.5, -0.0])
    assert np.array_equal(Q.finish(v, r, True, True, 1.0), [0.5, 0.5, 2.5, -0.5])
    assert np.array_equal(Q.finish(v, r, True, False, 1.0), [0.0, 0.0, 2.5, 0.0])
    assert np.isnan(Q.finish(v, r, False, False, 1.0)[[0, 3]]).all()
    fin = np.array([-1.0, 2.0])
    for order in ('header', 'swapped', 'scaled_early'):
        assert np.array_equal(Q.finish(fin, r[:2], True, True, -1.25, order), R.finish(fin, r[:2], True, True, -1.25, order))


# ---------------------------------------------------------------------------------------------------------------- the rule
def test_rule_known_answers():
    """check_bytes on hand-made values: the exact code away from a boundary, either code at a boundary, no third code, the exact zero of
    the ReLU, the sign of zero, saturation, NaN, an unwritten byte"""
    #             0: 20 = 0x5A   1: 21, the boundary of 20 | 22   2: zeroed by the ReLU   3: saturates   4: NaN   5: 300.3 -> 288 = 0x79
    v = np.array([20.0, 21.0, -100.0, 1000.0, np.nan, 300.3])
    ex = Q.Expect(v, None, True, False, 1.0, 'e4m3')
    assert abs(ex.delta - 0.1) < 1e-12 and ex.boundary.tolist() == [False, True, False, False, False, False]
    good = np.array([0x5A, 0x5A, 0x00, 0x7E, 0x00, 0x79], np.uint8)                     # under the ReLU the NaN is a zero
    assert np.array_equal(Q.decode(good[[0, 5]]), [20.0, 288.0]) and np.array_equal(ex.want, good)
    Q.check_bytes('good', good, ex)
    Q.check_bytes('other side of the boundary', np.where(np.arange(6) == 1, 0x5B, good).astype(np.uint8), ex)
    for i, byte in ((0, 0x5B), (1, 0x5C), (1, 0x59), (2, 0x01), (2, 0x80), (3, 0x7D), (3, 0x7F), (4, 0x7F), (5, 0x7A), (5, 0x7F)):
        bad = good.copy()
        bad[i] = byte
        with pytest.raises(AssertionError, match='stored byte'):
            Q.check_bytes(f'element {i} as 0x{byte:02X}', bad, ex)
    # no ReLU, multiplier -1.25: -25 is the boundary of -24 | -26;  -26.25 -> -26;  125 -> 128;  -1250 -> -448;  NaN;  -375.4 -> -384
    lin = Q.Expect(v, None, False, False, -1.25, 'e4m3')
    assert abs(lin.delta - 0.125) < 1e-12 and lin.boundary.tolist() == [True, False, False, False, False, False]
    good = np.array([0xDC, 0xDD, 0x70, 0xFE, 0x7F, 0xFC], np.uint8)
    assert np.array_equal(lin.want[[0, 1, 2, 3, 5]], good[[0, 1, 2, 3, 5]]) and (lin.want[4] & 0x7F) == 0x7F
    Q.check_bytes('lin', good, lin)
    Q.check_bytes('lin, the other code and the other NaN byte', np.array([0xDD, 0xDD, 0x70, 0xFE, 0xFF, 0xFC], np.uint8), lin)
    for i, byte in ((4, 0xFE), (4, 0x7E), (4, 0x00), (3, 0x7E), (0, 0xDE), (1, 0xDC), (2, 0x6F)):
        bad = good.copy()
        bad[i] = byte
        with pytest.raises(AssertionError, match='stored byte'):
            Q.check_bytes(f'lin element {i} as 0x{byte:02X}', bad, lin)
    # a value just above zero: every subnormal code its interval touches, and -0 only when the interval reaches zero
    tiny = Q.Expect(np.array([0.004, 390.0]), None, False, False, 1.0, 'e4m3')           # delta 0.039: [-0.035, 0.043]
    assert tiny.boundary.tolist() == [True, False] and tiny.olo[0] == Q.ordinal(Q.encode(-0.035)) and tiny.ohi[0] == Q.ordinal(Q.encode(0.043))


def test_rule_rejects_every_wrong_fold():
    """the encoding of a wrong fold fails check_bytes on a real case (the checker is not vacuous), the reference's own encoding passes"""
    c = Q.BY_NAME['k1_c128_n144_d']
    o = dict(relu=True, res='after', post=-1.25)
    ex = c.expect_unfolded(o)
    ratio, share = Q.check_bytes('reference', ex.want, ex)
    assert ratio == 0.0 and 0.0 < share <= Q.BOUNDARY_CAP
    for wrong in Q.WRONG_FOLDS:
        bad = c.value(o, *c.fold(o), order=wrong) if wrong in ('swapped', 'scaled_early') else c.value(o, *c.fold(o, wrong=wrong))
        with pytest.raises(AssertionError, match='stored byte'):
            Q.check_bytes(wrong, Q.encode(bad), ex)


# ---------------------------------------------------------------------------------------------------------------- conditions on the cases
def test_case_table_reaches_the_branches():
    names = [c.name for c in Q.ROUNDING]
    assert len(set(names)) == len(names) and set(Q.FUSED) <= set(names) and {n + '_' + f for n, f in Q.SPLIT_K} <= set(names)
    assert {c.form for c in Q.ROUNDING} == set('abcdf') and {c.cout for c in Q.ROUNDING} == {16, 24, 48, 144, 256}
    assert {(c.k, c.cin, c.layout) for c in Q.ROUNDING} >= {(1, 16, 0), (1, 128, 1), (3, 48, 0), (3, 128, 1), (1, 512, 1)}
    assert {c.B * c.hw[0] * c.hw[1] for c in Q.ROUNDING if c.s == 1} == {234, 35} and any(c.s == 2 and c.k == 3 and c.hw == (11, 14) for c in Q.ROUNDING)
    for c in Q.ROUNDING:
        opts = c.options()
        assert {o['relu'] for o in opts} == {True, False} and {o['post'] for o in opts} == {1.0, -1.25}
        assert {o['res'] for o in opts} == ({'before', 'after'} if c.has_res else {None})
        assert c.layout == 0 or c.cin % (128 if c.in_t == 'e4m3' else 64) == 0
    c = Q.ROUNDING[1].make()
    chs = np.abs(c.w_op * c.s_w[:, None, None, None, None]).reshape(c.cout, -1).max(1)
    assert chs.max() / chs.min() >= 8.0 and np.all(np.maximum(c.s_w / c.s_w[np.arange(c.cout) ^ 1], c.s_w[np.arange(c.cout) ^ 1] / c.s_w) > 2.0)


def _folded_vr(case, o):
    sc, sf, rs = Q.folded_f32(case, o)
    return case.acc * sc.astype(np.float64) + sf.astype(np.float64), None if case.r_op is None else case.r_op * rs


@pytest.mark.parametrize('case', Q.ROUNDING, ids=lambda c: c.name)
def test_cases_tell_the_folds_apart_and_keep_the_cap(case):
    """For every option of the case that has the feature, the reference under each wrong fold -- res_scale taken as 1, the shift not
    divided by s_out, s_w from channel co ^ 1, the residual on the other side of the ReLU, post_scale before the ReLU -- lies more than two
    code steps (bf16 / fp32 output: more than 4 x the bar) away on >= 25 % of the elements; at most 10 % of the elements of any run hold
    a rounding boundary; an e4m3 run is calibrated on its own maximum; residuals and (where asked) inputs have both signs."""
    case.make()
    worst, seen, cap = {}, set(), 0.0
    for o in case.options():
        for wrong in Q.WRONG_FOLDS:
            if Q.has_feature(case, o, wrong):
                f = Q.separated(case, o, wrong)
                worst[wrong] = min(worst.get(wrong, 1.0), f)
                seen.add(wrong)
                assert f >= 0.25, f'{case.name} {Q.opt_id(o)}: {wrong} is told apart on {f:.3f} of the elements only'
        if case.out_t == 'e4m3':
            ex = case.expect_unfolded(o)
            cap = max(cap, ex.boundary_share)
            assert ex.boundary_share <= Q.BOUNDARY_CAP, f'{case.name} {Q.opt_id(o)}: {ex.boundary_share:.3f} of the elements hold a boundary'
            assert ex.saturated_share < 1e-4 and not ex.nan.any()            # (a rounding of the fold may push the maximum itself over 448)
            assert Q.Expect(*_folded_vr(case, o), o['relu'], o['res'] == 'after', o['post'], 'e4m3').saturated_share < 1e-4      # ... also in fp32
    want = {w for w in Q.WRONG_FOLDS if any(Q.has_feature(case, o, w) for o in case.options())}
    assert seen == want and 'scaled_early' in seen
    assert (case.x_op.min() < 0) == case.signed and (case.r_op is None or (case.r_op.min() < 0 < case.r_op.max()))
    pos = float((case.pre > 0).mean())
    assert 0.5 < pos < 0.85, f'{case.name}: {pos:.2f} of the pre-activations are positive'
    print(f'{case.name}: smallest separated share ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()) + f'; largest boundary share {cap:.4f}; '
          f'{pos:.2f} of the pre-activations positive')


def test_saturation_case():
    """s_out from a quarter of the maximum: between 1 % and 50 % of the elements lie beyond +-448 and are stored as 0x7E / 0xFE; the
    +-inf channels saturate with their sign, the NaN channel is a NaN byte without the ReLU and 0 with it; every other channel is as in the
    rounding case it was derived from"""
    c, base = Q.SATURATION.make(), Q.BY_NAME['k1_c128_n144_b'].make()
    assert np.array_equal(c.xb, base.xb) and np.array_equal(c.wb, base.wb) and np.array_equal(c.acc, base.acc)
    nan_c, pinf_c, ninf_c = (k for k, v in sorted(Q.SPECIAL.items()))
    assert np.isnan(c.bn_shift[nan_c]) and c.bn_shift[pinf_c] == np.inf and c.bn_shift[ninf_c] == -np.inf and len({nan_c // 64, pinf_c // 64, ninf_c // 64}) == 3
    lin, relu = c.options()
    assert not lin['relu'] and relu['relu']
    for o in (lin, relu):
        ex = c.expect_unfolded(o)
        fin = np.delete(ex.u, [nan_c, pinf_c, ninf_c], axis=-1)
        share = float((np.abs(fin) > 448.0).mean())
        print(f'saturation case {Q.opt_id(o)}: {share:.4f} of the finite-channel elements beyond +-448, largest {float(np.abs(fin).max()):.1f}')
        assert 0.01 <= share <= 0.50 and abs(float(np.abs(fin).max()) / 448.0 - 4.0) < 0.5
        assert set(np.unique(ex.want[np.abs(ex.u) > 448.0]).tolist()) <= {0x7E, 0xFE}
        assert (ex.want[..., pinf_c] == 0x7E).all()
        assert (ex.want[..., ninf_c] == (0x00 if o['relu'] else 0xFE)).all()
        if o['relu']:
            assert not ex.nan.any() and (ex.want[..., nan_c] == 0x00).all() and (ex.olo[..., nan_c] == 0).all() and (ex.ohi[..., nan_c] == 0).all()
        else:
            assert ex.nan[..., nan_c].all() and int(ex.nan.sum()) == ex.u[..., nan_c].size
            assert (ex.want[ex.u < -448.0] == 0xFE).all() and (ex.u < -448.0).any()
        Q.check_bytes(f'saturation reference {Q.opt_id(o)}', ex.want, ex)
        if not o['relu']:                                     # the byte the clamp-by-median would store for the NaN is rejected
            bad = ex.want.copy()
            bad[..., nan_c] = 0xFE
            with pytest.raises(AssertionError, match='stored byte'):
                Q.check_bytes('NaN stored as -448', bad, ex)
