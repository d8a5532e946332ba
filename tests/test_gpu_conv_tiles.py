"""-m gpu: every row of csrc/conv_tiles.h on the MI355X against plain fp64 at its own edges.  The rows are read from the header and the shapes
derived from each row's numbers by tests/ref_tiles.py (proved without a device by tests/test_host_conv_tiles.py), so a row added to the table is
tested with no edit here.  Every run is made under the forced number after ivx_conv_plan_query has named that number -- one launch, no K split --
which is how a test knows the row ran; outputs the wrappers take are pre-filled with NaN and followed by a guard of bm x Cout elements that must
come back untouched.  The bars are the project's own: ref_conv.TOL_F32, TOL_BF16_IN, 2e-5 of the range for both pair families (pair IO: as
ref_pair's checkers apply it, with the scale the bound rule must choose), ref_fp8.check_bytes for e4m3, 1e-4 + 1e-4 of the range for the
Winograd forms against fp64 and 2e-5 of the range against the generic kernel (halo mode 0) on the same operands.  Each test prints its worst
error / tolerance.  DESIGN.md ("tile rows and the test that reaches each") has the figures measured."""
import numpy as np
import pytest
import torch

import ref_conv as R
import ref_fp8 as Q
import ref_pair as P
import ref_tiles as T
from test_gpu_conv_epilogue import tile_override
from test_gpu_pair_chain import make_pair
from test_gpu_pair_range import GpuBackend

pytestmark = pytest.mark.gpu

ROWS = T.direct_rows()
HALO = T.halo_rows()
GROUPED = [r for r in ROWS if r.family in ('f32', 'pair_f16')]
GROUPS = (T.WINO_TILE + 2) ** 2
rid = lambda r: f'{r.family}-{r.number}'          # noqa: E731
# (number, family) -> the library's message, for a pair the library refuses by a documented precondition: none today.  Every other pair is run.
REFUSED = {}
ZBLK_REFUSAL = 'this z-blocked config is built for columns of'


@pytest.fixture(scope='module')
def L():
    from imvoxelnet_amd import _lib
    lib = _lib.lib()
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    return lib


@pytest.fixture(scope='module')
def be(L):
    return GpuBackend(L)


@pytest.fixture(scope='module')
def wino_refs(L):
    """per Winograd shape, once: the fp64 convolution (ref_conv.Case) and the generic LDS-DMA kernel's output (halo mode 0) on fp16-pair operands"""
    from imvoxelnet_amd import ops
    cache = {}

    def get(shape, stride):
        if (shape, stride) not in cache:
            with T.forced(L, halo=0):
                generic = T.run_wino(ops, 128, shape, stride, T.IVX_F16_PAIR)
            cache[(shape, stride)] = (T.wino_case(shape, stride).ref(T.WINO_OPTION), generic)
        return cache[(shape, stride)]
    return get


def _refusal():
    from imvoxelnet_amd import _lib
    return (ValueError, _lib.IvxError)


def _run_direct(L, be, row, s, layout):
    """one shape and filter layout of a row through its family's driver, checked; returns the worst error / tolerance"""
    from imvoxelnet_amd import ops
    fam = row.family
    name = f'{rid(row)} shape {s.tag} layout {layout}'
    if fam == 'pair_f16':
        worst = 0.0
        for out_pair in (False, True):
            T.assert_direct_plan(L, row, s, layout, True, out_pair)
            got, ref, allowed = T.run_pio(ops, make_pair, row, s, out_pair)
            if not out_pair:
                worst = max(worst, P.check_f32_output(name + ' fp32 out', got, ref))
                continue
            worst = max(worst, P.check_pair_output(name + ' pair out', got, ref, allowed))
            # the scalar block, as tests/test_gpu_bottleneck.py asserts it: the maximum of the stored values, a power-of-two scale under 2^15
            stored = float(np.abs(P.pair_decode(got['data'], got['scale'])).max())
            assert abs(got['rec'] - stored) <= 2.0 ** -20 * got['rec'], (name, got['rec'], stored)
            assert got['scale'] > 0 and got['scale'] * got['rec'] < 32768.0 and np.log2(got['scale']) == round(np.log2(got['scale'])), (name, got['scale'])
        return worst
    T.assert_direct_plan(L, row, s, layout)
    if fam in ('generic', 'f32'):
        return R.check(name, T.run_f32(be, row, s, layout), T.reference(fam, s), R.TOL_F32)
    if fam == 'e4m3':
        c, o = T.case_of(fam, s), T.fp8_option(s)
        ex = c.expect(o, *Q.folded_f32(c, o))
        assert ex.boundary_share <= Q.BOUNDARY_CAP, (name, ex.boundary_share)
        return Q.check_bytes(name, T.run_lowp(ops, row, s, layout), ex)[0]
    return R.check(name, T.run_lowp(ops, row, s, layout), T.reference(fam, s), T.FAMILIES[fam].tol)


@pytest.mark.parametrize('row', ROWS, ids=rid)
def test_direct_row_vs_fp64(L, be, row):
    """Every shape of ref_tiles.direct_shapes(row), in every filter layout its Cin allows (pair IO: with fp32 and with pair output), under the
    forced row against the fp64 reference of the family's operands."""
    worst = 0.0
    with tile_override(L, row.number):
        for s in T.direct_shapes(row):
            for layout in s.layouts:
                if (row.number, row.family) in REFUSED:
                    with pytest.raises(_refusal(), match=REFUSED[(row.number, row.family)]):
                        _run_direct(L, be, row, s, layout)
                    continue
                worst = max(worst, _run_direct(L, be, row, s, layout))
    print(f'gpu direct row {rid(row)} ({row.bm} x {row.bn}, bk {row.bk}, {row.nb} buffers): worst error / tolerance = {worst:.3f}')


@pytest.mark.parametrize('row', GROUPED, ids=rid)
def test_grouped_row_vs_fp64(L, row):
    """The fp32 and fp16-pair rows as the tile of the grouped launch of an F(4x4, 3x3) layer (540 rows x 192 channels per Winograd position,
    36 groups, K = 3 Cin): halo mode 0 keeps the z-halo kernels away, the query names the row as the grouped tile"""
    from imvoxelnet_amd import ops
    operands = T.IVX_F16_PAIR if row.family == 'pair_f16' else 0
    shape = T.GROUPED_SHAPE
    with T.forced(L, tile=row.number, halo=0):
        rc, rec = T.plan_query(L, T.wino_desc(shape, 1, operands), groups=GROUPS)
        assert rc == 0 and rec.halo_cfg == 0 and rec.grouped_tile == row.number and rec.tile_matches == 1, (rec.halo_cfg, rec.grouped_tile, rec.tile_matches)
        got = T.run_wino(ops, row.bm, shape, 1, operands)
    worst = R.check(f'grouped {rid(row)}', got, T.wino_case(shape, 1).ref(T.WINO_OPTION), T.WINO_TOL)
    print(f'gpu grouped row {rid(row)}: worst error / tolerance = {worst:.3f}')


@pytest.mark.parametrize('row', HALO, ids=lambda r: f'{r.kind}{r.number}')
def test_halo_row_vs_fp64(L, wino_refs, row):
    """Every z-halo / z-blocked row on every Winograd shape of its stride, against fp64 and against the generic kernel on the same operands; a
    z-blocked row refuses the column heights it is not built for and runs on those it is built for."""
    from imvoxelnet_amd import ops
    worst, ran = [0.0, 0.0], 0
    for shape in T.halo_shapes(row.stride):
        name = f'halo {row.kind}{row.number} {shape}'
        with T.forced(L, halo=row.number):
            rc, rec = T.plan_query(L, T.wino_desc(shape, row.stride, T.IVX_F16_PAIR), groups=GROUPS)
            assert rc == 0 and rec.halo_cfg == row.number, (name, rec.halo_cfg)
            if row.kind == 'Z' and not T.zblk_fits(row, shape):
                with pytest.raises(ValueError, match=ZBLK_REFUSAL):
                    T.run_wino(ops, row.bm, shape, row.stride, T.IVX_F16_PAIR)
                continue
            got = T.run_wino(ops, row.bm, shape, row.stride, T.IVX_F16_PAIR)
        ref, generic = wino_refs(shape, row.stride)
        worst[0] = max(worst[0], R.check(name + ' vs fp64', got, ref, T.WINO_TOL))
        worst[1] = max(worst[1], R.check(name + ' vs generic', got, generic, (0.0, T.HALO_VS_GENERIC, True)))
        ran += 1
    assert ran >= (1 if row.kind == 'Z' else 3)
    print(f'gpu halo row {row.kind}{row.number}: worst error / tolerance = {worst[0]:.3f} vs fp64, {worst[1]:.3f} vs the generic kernel')


def _first(family, number=None):
    return [r for r in ROWS if r.family == family and (number is None or r.number == number)][0]


def test_number_outside_the_family_is_refused(L, be):
    """A forced number that the operands' family has no instantiation of returns the launcher's error: no other tile runs in its place.
    (The planner remaps 41 .. 57 onto the bf16 tiles for bf16 storage on purpose: not here.)  e4m3 ignores a number outside 91 .. 94 by rule:
    the plan query says so, and the rule's tile gives the right bytes."""
    from imvoxelnet_amd import ops
    cases = [('pair_f16', 64, 1, 'tile 64 has no instantiation for these pair operands'),
             ('pair_bf16', 474, 1, 'tile 474 has no instantiation for these pair operands'),
             ('bf16', 166, 1, 'bf16 input is only implemented by the LDS-DMA kernel'),
             ('bf16', 58, 1, 'bf16 input is only implemented by the LDS-DMA kernel'),
             ('f32', 91, 0, 'tile 91 is not an fp32 LDS-DMA tile'),
             ('f32', 67, 0, 'tile 67 is not an fp32 LDS-DMA tile'),
             ('f32', 8, 0, 'unknown tile override 8'),
             ('f32', 1, 1, 'wgt_layout 1 is only implemented by the LDS-DMA kernel')]         # a generic row on chunk-major filters
    for fam, number, layout, msg in cases:
        row = _first(fam)
        s = [s for s in T.direct_shapes(row) if s.tag == 'c'][0]
        assert layout in s.layouts and (number, fam) not in {(r.number, r.family) for r in ROWS}
        with tile_override(L, number):
            with pytest.raises(_refusal(), match=msg):
                if fam == 'pair_f16':
                    T.run_pio(ops, make_pair, row, s, True)
                elif fam == 'f32':
                    T.run_f32(be, row, s, layout)
                else:
                    T.run_lowp(ops, row, s, layout)
    # the grouped launch: a tile of the other operand type; the halo launch: a number in no row of its stride
    for operands, number in ((0, 67), (T.IVX_F16_PAIR, 54)):
        with T.forced(L, tile=number, halo=0):
            rc, rec = T.plan_query(L, T.wino_desc(T.GROUPED_SHAPE, 1, operands), groups=GROUPS)
            assert rc == 0 and rec.grouped_tile == number and rec.tile_matches == 0
            with pytest.raises(_refusal(), match=f'tile {number} does not match the operand type'):
                T.run_wino(ops, 128, T.GROUPED_SHAPE, 1, operands)
    assert not any(r.number == 15 for r in HALO)
    with T.forced(L, halo=15):
        with pytest.raises(_refusal(), match='unknown config 15'):
            T.run_wino(ops, 128, T.GROUPED_SHAPE, 1, T.IVX_F16_PAIR)
    # e4m3: the override 74 is not the e4m3 family's; the rule's own tile runs, as the query says
    row = _first('e4m3')
    for s in T.direct_shapes(row)[:3]:
        with tile_override(L, 74):
            rc, rec = T.plan_query(L, *T.direct_desc(row, s, s.layouts[0]))
            assert rc == 0 and rec.cfg[0] in (91, 92, 93), rec.cfg[0]
            ruled = _first('e4m3', rec.cfg[0])
            c, o = T.case_of('e4m3', s), T.fp8_option(s)
            Q.check_bytes(f'e4m3 under override 74 (tile {rec.cfg[0]} by rule) shape {s.tag}', T.run_lowp(ops, ruled, s, s.layouts[0]), c.expect(o, *Q.folded_f32(c, o)))
