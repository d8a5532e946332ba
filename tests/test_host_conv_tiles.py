"""The tile tables of csrc/conv_tiles.h without a device: tests/ref_tiles.py finds every row (against what the library itself answers), the
shapes it derives from a row's numbers have the properties they are for (by arithmetic, and where a family's channel unit forbids one, by the
proof that no Cin has it), the planner names the forced row on every one of them and plans no split, the fp32 cases and their driver are right
on the CPU restatement oracle/cpu_abi, and the cases can tell a tile kernel's mistakes from the right result: the fp64 result without the last
K slab, and with the rows of the last partial M tile taken from the tile before, each lie more than 100 x the family's tolerance away on
every affected row.  tests/test_gpu_conv_tiles.py then runs the same rows, shapes and drivers on the HIP library."""
import importlib.util
import os
import re

import numpy as np
import pytest

import plan_worker as pw
import ref_conv as R
import ref_fp8 as Q
import ref_tiles as T

ROWS = T.direct_rows()
HALO = T.halo_rows()
rid = lambda r: f'{r.family}-{r.number}'          # noqa: E731
GROUPS = (T.WINO_TILE + 2) ** 2


@pytest.fixture(scope='module')
def L():
    from imvoxelnet_amd import _lib
    return _lib.lib()


@pytest.fixture(scope='module')
def cpu():
    spec = importlib.util.spec_from_file_location('ivx_cpu_abi_host', os.path.join(T.ROOT, 'oracle', 'cpu_abi', 'host.py'))
    host = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(host)
    return R.HostBackend(host.load())


# ---------------------------------------------------------------------------------------------------------------- the reader
def test_reader_finds_every_row(L):
    """The X numbers are the numbers ivx_conv_tile_info answers for plus the generic rows, with its bm / bn / bk; the H and Z numbers are
    the numbers the grouped rule accepts on the layers of their stride; and a line that opens a row but escapes the reader's pattern fails here.
    The table holds 51 X rows = 78 (row, family) pairs and 28 H + 4 Z rows today; those counts are floors."""
    text = open(T.TILES_H).read()
    rows = T.table_rows()
    numbers = [r[0] for r in rows]
    assert len(set(numbers)) == len(numbers) == len(re.findall(r'^\s*X\(\s*\d', text, re.M)) >= 51
    infos = pw.plan_tile_infos(L)
    generic = {r[0] for r in rows if r[1] == 'GENERIC'}
    assert set(numbers) - {int(k) for k in infos} == generic and {int(k) for k in infos} <= set(numbers) and len(generic) == 7
    assert all(r[1] in T.MASKS for r in rows)
    for r in ROWS:
        if r.family != 'generic':
            assert infos[str(r.number)][:3] == [r.bm, r.bn, r.bk], r
    assert len(ROWS) >= 78 and len({(r.number, r.family) for r in ROWS}) == len(ROWS)
    assert {f: sum(r.family == f for r in ROWS) for f in T.FAMILIES} == {'generic': 7, 'f32': 16, 'bf16': 12, 'e4m3': 4, 'pair_bf16': 18, 'pair_f16': 21} or len(ROWS) > 78
    h, z = T.halo_table()
    assert len(h) == len(re.findall(r'^\s*H\(\s*\d', text, re.M)) >= 28 and len(z) == len(re.findall(r'^\s*Z\(\s*\d', text, re.M)) >= 4
    assert len(HALO) == len(h) + len(z) >= 32 and len({r.number for r in HALO}) == len(HALO)
    assert all(T.halo_mode_stride(r[0]) == r[9] for r in h) and all(T.halo_mode_stride(r[0]) == r[5] for r in z)
    for row in HALO:                       # the library's halo_mode_stride: a forced number is answered on the layers of its stride, and only there
        for stride in (1, 2):
            with T.forced(L, halo=row.number):
                rc, rec = T.plan_query(L, T.wino_desc(T.halo_shapes(stride)[1], stride, T.IVX_F16_PAIR), groups=GROUPS)
            assert rc == 0 and rec.halo_cfg == (row.number if stride == row.stride else 0), (row, stride, rec.halo_cfg)


# ---------------------------------------------------------------------------------------------------------------- the generated shapes
def _reachable(row, k):
    """the slab counts the family's channel units can give a k x k layer"""
    u = min(T._units(row.family))
    return sorted({T.slabs(row, c, k) for c in range(u, 64 * u + 1, u) if T._layouts(row.family, c)})


@pytest.mark.parametrize('row', ROWS, ids=rid)
def test_generated_shapes_have_their_properties(row):
    f = T.FAMILIES[row.family]
    shapes = {s.tag: s for s in T.direct_shapes(row)}
    assert set(shapes) == set('abcdef' if row.family in ('generic', 'f32') else 'abcde')
    facts = {t: T.shape_facts(row, s) for t, s in shapes.items()}
    all_layouts = tuple(l for l, u in ((0, f.unit0), (1, f.unit1)) if u)
    s1, s3 = _reachable(row, 1), _reachable(row, 3)
    for t, s in shapes.items():
        assert s.layouts and s.layouts == T._layouts(row.family, s.cin) and s.cout % (f.off if f.off == 16 else 1) == 0
        assert s.res == s.relu == (bool(row.rpf) or t in 'bd'), (t, s)
        assert facts[t]['M'] <= 2049 and s.cout <= 2 * 256 + 32 and facts[t]['K'] <= 9 * 2 * 128, (t, s)
    a, fa = shapes['a'], facts['a']
    assert fa['M'] == row.bm - 1 and fa['Mt'] == 1 and a.cout == max(row.bn - f.off, f.off) and fa['Nt'] == 1 and a.k == 1
    assert fa['S'] == s1[0] and (fa['K'] < row.bk) == any(f.el * c < row.bk for c in range(min(T._units(row.family)), row.bk, min(T._units(row.family))))
    b, fb = shapes['b'], facts['b']
    assert fb['M'] == row.bm + 1 and fb['Mt'] == 2 and fb['rem_m'] == 1 and b.cout == row.bn + f.off and fb['Nt'] == 2 and fb['rem_n'] == f.off
    assert fb['S'] == min(v for v in s1 if v > row.nb), (fb, s1)          # nb + 1 wherever a Cin gives it: the first loop longer than the ring
    c, fc = shapes['c'], facts['c']
    assert fc['M'] == 8 * row.bm + 1 and fc['Mt'] == 9 and fc['q_total'] == 2 and c.cout == row.bn and fc['S'] == 2 and fc['rem_k'] == 0 and c.layouts == all_layouts
    d, fd = shapes['d'], facts['d']
    assert d.k == 3 and d.stride == 1 and d.H % 2 == 1 and d.W % 2 == 1 and fd['M'] >= row.bm + 1 and fd['Mt'] >= 2 and fd['rem_m'] and d.cout == row.bn
    odd = [v for v in s3 if v % 2 == 1 and v % row.nb]
    assert fd['S'] == (odd[0] if odd else [v for v in s3 if v % row.nb][0] if [v for v in s3 if v % row.nb] else s3[0]), (fd, s3)
    # (no odd count: fp16 pairs on bk = 32, 9 * 64 stored elements per 32 channels are 18 slabs; a multiple of nb only: the three-buffer ring,
    # whose 3x3 loops are multiples of 9 slabs)
    assert odd or (row.family == 'pair_f16' and row.bk == 32) or row.nb == 3, (row, s3[:6])
    e, fe = shapes['e'], facts['e']
    assert e.k == 3 and e.stride == 2 and e.B == 2 and e.H % 2 == 1 and e.W % 2 == 1 and e.cout == 2 * row.bn + 2 * f.off and fe['Nt'] == 3
    assert fe['rem_n'] == (2 * f.off) % row.bn and e.layouts == all_layouts and fe['S'] >= row.nb and s3[0] >= 2
    if 'f' in shapes:
        g, fg = shapes['f'], facts['f']
        assert fg['M'] == row.bm + 1 and g.cout == row.bn + 2 and g.cout % 4 and fg['S'] == 2
    # a K loop shorter than the ring, a K remainder and both filter layouts are each reached by some shape of the row
    assert min(v['S'] for v in facts.values()) < row.nb or row.nb == 2 and s1[0] == 2, facts
    u = min(T._units(row.family))
    can_rem = any((k * k * f.el * c) % row.bk for k in (1, 3) for c in range(u, 64 * u + 1, u) if T._layouts(row.family, c))
    assert any(v['rem_k'] for v in facts.values()) == can_rem, facts           # (a pair tensor's 32 or 64 stored elements per channel unit can be whole slabs only)
    assert {l for s in shapes.values() for l in s.layouts} == set(all_layouts)


def test_halo_shapes_have_their_properties():
    """The Winograd shapes, by arithmetic from the table: for every row fewer rows than a tile; at least three M tiles with a partial last
    one; for the 128-column tiles a whole and a partial column tile, for the 256-column tiles a whole one on two M tiles; a tile boundary
    inside a z column; every z-blocked row has a shape built for it and shapes it must refuse."""
    for row in HALO:
        bm = T.halo_bm_eff(row)
        shapes = T.halo_shapes(row.stride)
        ms = [T.halo_rows_m(s, row.stride) for s in shapes]
        if row.kind == 'Z':
            fits = [s for s in shapes if T.zblk_fits(row, s)]
            assert fits and len(fits) < len(shapes), row
            assert any(T.halo_rows_m(s, row.stride)[0] > bm and T.halo_rows_m(s, row.stride)[0] % bm for s in fits), row
            continue
        assert min(m for m, _ in ms) < bm, row
        assert any(-(-m // bm) >= 3 and m % bm for m, _ in ms), (row, ms)
        assert any(m > bm and bm % zo for m, zo in ms), (row, ms, 'no tile boundary inside a column')
        if row.bn == 128:
            assert any(s[2] > 128 and s[2] % 128 and T.halo_rows_m(s, row.stride)[0] > bm for s in shapes), row
        if row.bn == 256:
            assert any(s[2] == 256 and -(-T.halo_rows_m(s, row.stride)[0] // bm) == 2 and T.halo_rows_m(s, row.stride)[0] % bm for s in shapes), row
    assert [T.halo_rows_m(s, 1)[0] for s in T.halo_shapes(1)][:4] == [60, 540, 336, 210] and [T.halo_rows_m(s, 2)[0] for s in T.halo_shapes(2)] == [24, 540, 336]
    assert -(-540 // 254) == 3 and -(-540 // 126) == 5 and T.GROUPED_SHAPE == T.halo_shapes(1)[1]


# ---------------------------------------------------------------------------------------------------------------- the plan under the override
@pytest.mark.parametrize('row', ROWS, ids=rid)
def test_plan_names_the_forced_row(L, row):
    """ivx_conv_plan_query under the override, on every shape, layout and (pair IO) output form: the row, one launch, no workspace"""
    pio = row.family == 'pair_f16'
    n = 0
    with T.forced(L, tile=row.number):
        for s in T.direct_shapes(row):
            for layout in s.layouts:
                for out_pair in (False, True) if pio else (False,):
                    T.assert_direct_plan(L, row, s, layout, pio, out_pair)
                    n += 1
    assert n >= 5


def test_grouped_and_halo_plans_name_the_forced_row(L):
    """the grouped launch of the Winograd form: a forced tile of the operands' family is the grouped tile (halo mode 0); a forced halo or
    z-blocked number is the config on every shape of its stride"""
    for row in ROWS:
        if row.family in ('f32', 'pair_f16'):
            with T.forced(L, tile=row.number, halo=0):
                rc, rec = T.plan_query(L, T.wino_desc(T.GROUPED_SHAPE, 1, T.IVX_F16_PAIR if row.family == 'pair_f16' else 0), groups=GROUPS)
            assert rc == 0 and rec.halo_cfg == 0 and rec.grouped_tile == row.number and rec.tile_matches == 1, (row, rec.halo_cfg, rec.grouped_tile)
    for row in HALO:
        for s in T.halo_shapes(row.stride):
            with T.forced(L, halo=row.number):
                rc, rec = T.plan_query(L, T.wino_desc(s, row.stride, T.IVX_F16_PAIR), groups=GROUPS)
            assert rc == 0 and rec.halo_cfg == row.number and rec.rows_dev_ok == 1, (row, s, rec.halo_cfg)


# ---------------------------------------------------------------------------------------------------------------- the fp32 cases on the CPU
def test_fp32_cases_on_the_cpu_restatement(cpu):
    """every distinct fp32 case and filter layout through the fp32 driver (guard included) on oracle/cpu_abi, within TOL_F32"""
    seen, worst = set(), 0.0
    for row in ROWS:
        if row.family in ('generic', 'f32'):
            for s in T.direct_shapes(row):
                for layout in s.layouts:
                    key = (s[1:10], layout)
                    if key not in seen:
                        seen.add(key)
                        worst = max(worst, R.check(f'cpu {rid(row)} {s.tag} layout {layout}', T.run_f32(cpu, row, s, layout), T.reference(row.family, s), R.TOL_F32))
    assert len(seen) >= 30
    print(f'{len(seen)} fp32 cases on the CPU restatement: worst error / tolerance = {worst:.3f}')


# ---------------------------------------------------------------------------------------------------------------- discrimination
_WRONG = {}


@pytest.mark.parametrize('row', ROWS, ids=rid)
def test_cases_tell_a_wrong_tile_from_the_right_one(row):
    """From the reference alone: without the last K slab every output row, and with the last partial M tile stored from the tile before
    every row of that tile, lies more than 100 x the family's tolerance from the right result (the largest excess of the row's channels)."""
    for s in T.direct_shapes(row):
        key = (row.family, row.bk, row.bm, s)
        if key not in _WRONG:
            right, short, moved, bound, touched = T.wrong_results(row, s)
            M = right.size // s.cout
            assert touched.mean() >= (0.6 if s.k == 3 else 1.0), (rid(row), s.tag, touched.mean())      # (3x3: all but the last row and column of a map)
            ex_k = (np.abs(short - right) / bound).reshape(M, s.cout).max(1)[touched]
            ex_m = None
            if moved is not None:
                ex_m = (np.abs(moved - right) / bound).reshape(M, s.cout).max(1)[(M // row.bm) * row.bm:]
            _WRONG[key] = (float(ex_k.min()), None if ex_m is None else float(ex_m.min()), M)
        k_min, m_min, M = _WRONG[key]
        assert k_min > 100.0, f'{rid(row)} shape {s.tag}: a row lies only {k_min:.1f} x the tolerance from the result without the last K slab'
        assert (m_min is None) == (M < row.bm or M % row.bm == 0), (rid(row), s.tag, M)
        assert m_min is None or m_min > 100.0, f'{rid(row)} shape {s.tag}: a row of the last M tile lies only {m_min:.1f} x the tolerance from the tile before'
        if row.family == 'e4m3':                 # the comparison rule's condition on the inputs (ref_fp8): at most 10 % of the elements hold a boundary
            c, o = T.case_of('e4m3', s), T.fp8_option(s)
            share = c.expect(o, *Q.folded_f32(c, o)).boundary_share
            assert share <= Q.BOUNDARY_CAP, f'{rid(row)} shape {s.tag}: boundary share {share:.3f}'
