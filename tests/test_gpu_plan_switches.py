"""-m gpu: the model handle's per-process switches and its plans on libimvoxel_hip.so.

IVX_SIDE_STREAM, IVX_FUSE_BOTTLENECK and IVX_FUSE_STEM are read once per process, so each setting runs in a fresh child of
tests/plan_worker.py (one after another, each with its own time limit; after the first child that fails, times out or dies from a signal
no further child is started).  A child builds a seeded model, runs four steps alternating two inputs (A, B, A, B) through ivx_model_detect
and saves FPN level 0, the volume, the valid mask, the neck output or levels, the head output and the detections of every step.

  * IVX_SIDE_STREAM 1 against 0: every saved array bit-identical, step for step; steps 3 / 4 repeat steps 1 / 2 inside each process.
  * ivx_model_trace level 2 (every launch stays on the caller's stream) against tracing off, in ONE process: bit-identical.
  * IVX_FUSE_BOTTLENECK=0 / IVX_FUSE_STEM=0 against the default: another summation order, so FPN level 0 within 2e-5 of the map's range (the
    bar of tests/test_gpu_pair_chain.py::test_trunk_pair_chain_vs_fp32_mfma) and the same kept labels and counts.
  * tests/plan_check.py, unchanged, on this library's plans at the BASELINE shapes (other workspace sizes and tile rules than the CPU
    restatement: Winograd layers, split-K workspaces, chained per-workgroup maxima)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import plan_worker as pw
from plan_check import PlanDefect, check_plan
from plan_worker import compare_runs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, 'plan_worker.py')
_failed_child = []          # once a child failed, no test of this module starts another one


def _child(tmp_path, tag, config, phases='0', timeout=300, **switches):
    if _failed_child:
        pytest.fail(f'not started: an earlier child failed ({_failed_child[0]})')
    out = tmp_path / f'{tag}.npz'
    env = {k: v for k, v in os.environ.items() if not k.startswith('IVX_')}
    env.update(switches)
    cmd = [sys.executable, WORKER, 'run', '--lib', 'hip', '--config', config, '--phases', phases, '--out', str(out)]
    what = f'{config} {switches or ""} phases {phases}'
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _failed_child.append(f'{what}: no result within {timeout} s')
        pytest.fail(_failed_child[0])
    if r.returncode != 0:
        _failed_child.append(f'{what}: exit status {r.returncode}: {r.stderr[-1500:]}')
        pytest.fail(_failed_child[0])
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
    return np.load(out), rec


@pytest.mark.parametrize('config,timeout', [('kitti_small', 300), ('kitti_small_f32', 300), ('nuscenes_dcn', 300), ('scannet_v1_bf16', 300),
                                            ('scannet_v1_fp8', 300), ('kitti_full', 600)])
def test_side_stream_on_and_off_are_bit_identical(tmp_path, config, timeout):
    """The side launch issues the same kernel on the same operands on its own workspace, the split-K reduction is a kernel and the maxima
    are order-independent: IVX_SIDE_STREAM=1 and =0 must agree bit for bit, and nothing may be carried over between calls."""
    on, rec_on = _child(tmp_path, 'side1', config, timeout=timeout, IVX_SIDE_STREAM='1')
    off, rec_off = _child(tmp_path, 'side0', config, timeout=timeout, IVX_SIDE_STREAM='0')
    assert rec_on['n_sides'] > 0 and rec_off['n_sides'] == 0, (rec_on, rec_off)          # a site exists, and the switch took effect
    n = compare_runs(on, off, 't0')
    fpn = on['t0_s0_fpn0']
    assert fpn.size > 0 and (fpn.dtype != np.float32 or (np.isfinite(fpn).all() and np.abs(fpn).max() > 0))
    print(f'{config}: IVX_SIDE_STREAM 1 ({rec_on["n_sides"]} sites) vs 0: bit-identical over {n} arrays x 4 steps; '
          f'detections per step {[int(on[f"t0_s{s}_count"].sum()) for s in range(4)]}')


@pytest.mark.parametrize('config', ['kitti_small', 'scannet_fast'])
def test_tracing_keeps_the_same_bits(tmp_path, config):
    """ivx_model_trace level 2 keeps every launch on the caller's stream (run_steps checks trace_on): same bits as the untraced run."""
    res, rec = _child(tmp_path, 'trace', config, phases='0,2')
    assert rec['n_sides'] > 0
    n = compare_runs(res, res, 't0', 't2')
    print(f'{config}: tracing level 2 vs off ({rec["n_sides"]} sites): bit-identical over {n} arrays x 4 steps')


def test_fusion_switches_stay_within_the_pair_chain_bound(tmp_path):
    """One-launch bottlenecks / stem off: the layer-by-layer kernels sum in another order.  FPN level 0 within 2e-5 of the map's range, the
    bound of test_trunk_pair_chain_vs_fp32_mfma, and the same kept labels and counts on the small KITTI-like model."""
    BOUND = 2e-5
    base, _ = _child(tmp_path, 'default', 'kitti_small')
    assert {1, 3, 4, 5} <= set(base['fuse'].tolist())
    for name, gone in (('IVX_FUSE_BOTTLENECK', {1, 5}), ('IVX_FUSE_STEM', {3, 4})):
        got, _ = _child(tmp_path, name, 'kitti_small', **{name: '0'})
        fuse = set(got['fuse'].tolist())
        assert not (fuse & gone) and ({1, 3, 4, 5} - gone) <= fuse, (name, fuse)      # the switch took effect, and only it
        worst = 0.0
        for step in range(4):
            a, b = got[f't0_s{step}_fpn0'].astype(np.float64), base[f't0_s{step}_fpn0'].astype(np.float64)
            rng = float(np.abs(b).max())
            assert a.shape == b.shape and rng > 0
            worst = max(worst, float(np.abs(a - b).max()) / rng)
        print(f'{name}=0 vs default: FPN level 0 max |d| / range = {worst:.3e} (bound {BOUND:g})')
        assert worst <= BOUND, (name, worst)
        for step in range(4):
            assert np.array_equal(got[f't0_s{step}_count'], base[f't0_s{step}_count']), (name, step)
            for b in range(len(base['t0_s0_count'])):
                assert np.array_equal(got[f't0_s{step}_labels{b}'], base[f't0_s{step}_labels{b}']), (name, step, b)
        assert int(base['t0_s0_count'].sum()) > 0, 'the case has no detections'


def test_plan_invariants_on_the_hip_library():
    """The checker of tests/test_host_plan.py on libimvoxel_hip.so's plans at the BASELINE shapes, through the same read-only view.  The form
    of every conv step of the detect plans (tile, pair input, split-operand bytes, workspace) is the one recorded in tests/golden/conv_routes.json
    before the routing rule became one library function (plan_worker.py routes)."""
    import json
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    L = pw.load_lib('hip')
    routes = json.load(open(pw.ROUTES_FILE))['plans']
    n_routes = 0
    n_plans = n_site_plans = n_reused = n_chained = 0
    fuse_seen = set()
    for fam in pw.FAMILIES:
        model = pw.family_model(fam)
        for mode in [(0, 4, 4), (0, 0, 0), (1, 4, 4)]:
            hd = pw.Handle(L, model, *mode, stream=None)
            try:
                for shape in pw.FULL_SHAPES[fam]:
                    for what in pw.plans_of(fam):
                        plan, total = hd.plan(what, *shape)
                        try:
                            st = check_plan(plan, total)
                        except PlanDefect as e:
                            raise AssertionError(f'{fam} storage/trunk/wino {mode} plan "{what}" at (B, V, H, W) = {shape}: {e}') from None
                        assert st['steps'] == plan['info']['s1'] - plan['info']['s0'] > 0
                        n_plans += 1
                        n_site_plans += st['n_sides'] > 0
                        n_reused += st['reused']
                        n_chained += st['chained']
                        fuse_seen.update(st['fuse'])
                        if what == 'detect':
                            want, got = routes[pw.plan_key(fam, mode, shape)], pw.conv_rows(plan)
                            assert got == want, f'{fam} {mode} detect at {shape}: conv steps (name, tile, pio, split, ws) differ from the recorded routes: ' \
                                                f'{[(g, w) for g, w in zip(got, want) if g != w][:4]} ({len(got)} steps, {len(want)} recorded)'
                            n_routes += 1
                        if what == 'detect' and mode == (0, 4, 4):
                            print(f'  {fam} detect at {shape}: total {st["total"]} bytes, workspace {st["ws_bytes"]}, second workspace {st["ws2_bytes"]} '
                                  f'(sized as the whole workspace it would be {st["ws_bytes"]}: total {st["total"] - st["ws2_bytes"] + st["ws_bytes"]})')
            finally:
                hd.close()
                torch.cuda.synchronize()
    print(f'plans checked {n_plans}, plans with side sites {n_site_plans}, fuse values seen {sorted(fuse_seen)}, reused arena offsets seen {n_reused}, '
          f'chained maxima seen {n_chained}')
    assert n_plans == sum(len(v) for v in pw.FULL_SHAPES.values()) * 3 * 4
    assert n_routes == len(routes) == n_plans // 4
    assert n_site_plans > 0 and n_reused > 0 and {1, 3, 4, 5} <= fuse_seen
    assert n_chained > 0          # Winograd layers with pair operands hand per-workgroup maxima to each other on this library
