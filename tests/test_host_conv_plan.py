"""What the conv planner answers -- which tile, which K split, which grid-tail plan, which workspace, which batch slices; for the grouped launches
of the Winograd form which z-halo / z-blocked config or which tile -- is host code (csrc/conv_plan.cpp over the one tile table csrc/conv_tiles.h),
and ivx_conv_plan_query reports it from the functions the launchers call.  tests/golden/conv_plans.json holds the answers of the rules as they
stood before they moved into that file (tests/plan_worker.py convplans, run on a library of that commit with the query added): every row must come
out unchanged, under every lab knob and, one child process per switch, under every environment switch.  No GPU: the library loads and answers
without a device."""
import json
import re
import os

import plan_worker as pw

# The numbers a `return` or an assignment of the rules can produce under default knobs, read off plan_conv / grouped_tile_plan / grouped_halo_cfg
# (generic fallbacks 1, 3, 4, 6 included; 73 and 174 need plan mode 1 / IVX_PIO_W8_TILES and are asserted there).
REACH = {
    'f32': {54, 56, 49, 47, 46, 44, 1, 3, 4, 6},
    'bf16': {63, 74, 81, 82, 64, 66, 67},
    'e4m3': {91, 92, 93},
    'pair_io': {76, 74, 66, 166, 177, 179, 183},
    'grouped': {76, 81, 82, 183, 67, 58, 54, 49, 47, 46, 44},
    'halo': {30, 33, 50, 42},
}


def _lib():
    from imvoxelnet_amd import _lib
    return _lib.lib()


def _golden():
    return json.load(open(pw.PLANS_FILE))


def _slices(row):
    """per distinct slice (samples, cfg, ksplit, tail_ks, q_total, qa, bm, ws_bytes) of a direct row"""
    return [] if len(row) == 1 else [row[1 + 8 * i:9 + 8 * i] for i in range((len(row) - 2) // 8)]


def test_every_recorded_plan_comes_out_unchanged():
    L, fx = _lib(), _golden()

    def check_ws(d, io, row):               # allow_ws = 1: the query and the workspace entry point of the same path agree
        assert pw.plan_workspace(L, d, io) == (-1 if len(row) == 1 else row[-1]), (list(bytes(d)), row)
        assert len(row) == 1 or row[-1] == max(s[7] for s in _slices(row))

    for name in ('direct', 'tiles', 'grouped', 'halo', 'env'):
        got = pw.plan_section(L, name, check=check_ws)
        assert len(got) == len(fx[name]) and len(got) > 100, name
        bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, fx[name])) if g != w]
        assert not bad, f'section {name}: {len(bad)} rows differ, first (index, got, recorded): {bad[:3]}'


def test_the_grid_reaches_every_number_of_the_rules():
    fx = _golden()
    it = iter(fx['direct'])
    seen = {k: set() for k in ('f32', 'bf16', 'e4m3', 'bf16_pair', 'f16_pair', 'pair_io')}
    pm1, ksplit, tail, sliced, two = set(), 0, 0, 0, 0
    for spec in pw.PLAN_LAYERS:
        for shape in pw.plan_shapes(spec):
            for mode, key in zip(pw.PLAN_MODES_CONV, seen):
                for aw, pm, res in pw.PLAN_CALLS:
                    if res == 0 or (mode in (pw.PLAN_MODES_CONV[0], pw.PLAN_MODES_CONV[5]) and (res != 2 or spec[5] == 2)):
                        row = next(it)
                        for s in _slices(row):
                            (pm1 if pm else seen[key]).add(s[1])
                            ksplit += s[2] > 1
                            tail += s[3] > 1 and pm == 1
                        sliced += len(row) > 1 and row[0] != shape[0] and shape[0] * shape[1] * shape[2] * shape[3] * 64 * 4 >= 2 ** 31
                        two += len(_slices(row)) == 2
    assert next(it, None) is None
    for key in ('f32', 'bf16', 'e4m3', 'pair_io'):
        assert REACH[key] <= seen[key], (key, sorted(REACH[key] - seen[key]))
    assert 73 in pm1 and ksplit and tail and sliced and two, (sorted(pm1), ksplit, tail, sliced, two)
    grouped = {r[1] for r in fx['grouped'] if len(r) == 4 and not r[0]}
    halo = {r[0] for r in fx['grouped'] if len(r) == 4 and r[0]}
    assert REACH['grouped'] <= grouped and REACH['halo'] <= halo, (sorted(grouped), sorted(halo))
    # the forced numbers: every halo row answers itself on the layers of its stride; 25 and 99 (in no row) go to the stride-2 launch, which refuses
    # them, and fall through to another kernel on stride 1
    n = len(pw.PLAN_HALO_CASES)
    for i, hm in enumerate(pw.PLAN_HALO_MODES):
        for (ch, k, z, rows, g), r in zip(pw.PLAN_HALO_CASES, fx['halo'][i * n:(i + 1) * n]):
            if hm in (25, 99) and k[2] == 1 and (k[1] == 1 or z % 2 == 0):          # (a stride-2 layer of the z-halo kernel halves its slices)
                assert r[0] == (hm if k[1] == 2 else 0), (hm, k, r)
    # ... and the environment switches move what they are for (the two stagger values bear on the launch, not on the plan)
    sw = fx['env_switches']
    assert set(sw) == set(pw.PLAN_ENV) and all(sw[k] for k in sw if 'STAGGER' not in k) and not sw['IVX_PIO_STAGGER_US'] and not sw['IVX_PIO_STAGGER_SHIFT']
    assert any(s[1] == 174 for _, row in sw['IVX_PIO_W8_TILES'] for s in _slices(row))


def test_environment_switches_one_process_each():
    fx = _golden()
    for name, value in pw.PLAN_ENV.items():
        got = pw.plan_env_diff(fx['env'], pw.plan_env_child(name, value))
        assert got == fx['env_switches'][name], f'{name}={value}: {len(got)} rows move, {len(fx["env_switches"][name])} recorded'


def test_tile_table_gives_the_recorded_tile_figures():
    """bm / bn / bk / wg_per_cu derived from the rows of csrc/conv_tiles.h equal what the hand-written switch held, number for number, and the
    table is the only place that spells a tile's template arguments."""
    L, fx = _lib(), _golden()
    assert pw.plan_tile_infos(L) == fx['tile_info'] and len(fx['tile_info']) >= 44
    csrc = os.path.join(pw.ROOT, 'imvoxelnet_amd', 'csrc')
    rows = re.findall(r'^  X\((\d+), (\w+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\)', open(os.path.join(csrc, 'conv_tiles.h')).read(), re.M)
    assert sorted(int(r[0]) for r in rows) == sorted(t for t in pw.PLAN_TILES if t not in (8, 45, 65, 90, 175))
    for n, fam, tm, tn, wr, wc, bk, wpe, nb, rpf, wg in rows:
        if fam != 'GENERIC':
            assert fx['tile_info'][n] == [int(wr) * int(tm) * 32, int(wc) * int(tn) * 32, int(bk), int(wg)], n
    for f in (f for f in os.listdir(csrc) if f.endswith(('.h', '.hip', '.cpp'))):
        text = open(os.path.join(csrc, f), errors='replace').read()
        assert f == 'conv_tiles.h' or not re.search(r'launch_(v4|cfg|halo|zblk)<[^>]*\d+, \d+, \d+[^>]*>\(p, st\)', text), f'{f} spells a tile by hand'
        assert f == 'conv_plan.cpp' or not f.startswith('conv_') or 'getenv' not in text, f'{f} reads the environment itself'
