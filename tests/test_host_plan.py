"""CPU-only: the invariants of the model handle's plans (csrc/model.cpp make_plan / run_steps), checked on the CPU restatement of the ABI.

The planner decides where every tensor lives in one arena, which steps a fused launch covers and which shortcut conv runs on the side
stream.  A mistake there corrupts data only at the shapes where the first-fit allocator happens to reuse the offset, so these tests do not
run the model: tests/plan_check.py derives liveness from the step list on its own and compares it with the plan, for every family, storage
and operand mode, the full-size BASELINE shapes and a seeded sweep of small ones.  The checker is tested itself on hand-made broken plans,
and the per-process switches (IVX_SIDE_STREAM, IVX_FUSE_BOTTLENECK, IVX_FUSE_STEM) are exercised in child processes."""
import copy
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import plan_worker as pw
from plan_check import PlanDefect, check_plan
from plan_worker import compare_runs

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, 'plan_worker.py')
# (storage, trunk_operands, wino_operands): fp32 / bf16 storage, fp32 / fp16-pair operands in the trunk and in the Winograd-domain GEMMs
MODES = [(0, 4, 4), (0, 0, 0), (0, 4, 0), (0, 0, 4), (1, 4, 4)]


def _child_env(**switches):
    env = {k: v for k, v in os.environ.items() if not k.startswith('IVX_')}
    env.update(switches)
    return env


@pytest.fixture(scope='module')
def cpu_lib():
    return pw.load_lib('cpu')


def _sweep_shapes(family, rng, n):
    """Seeded small shapes: B in 1..4, V in {1, 2, 5, 12}, H and W multiples of 32 in [64, 512] (the LayoutHead predicts one camera)."""
    out = []
    for _ in range(n):
        V = 1 if family == 'sunrgbd_total' else rng.choice([1, 2, 5, 12])
        out.append((rng.randint(1, 4), V, 32 * rng.randint(2, 16), 32 * rng.randint(2, 16)))
    return out


def test_every_plan_keeps_its_invariants(cpu_lib):
    """Every family x storage x operand mode, the plans behind ivx_model_forward / _forward_levels ("forward"), ivx_model_detect ("detect"),
    ivx_backbone_fpn_fwd ("trunk") and the ivx_neck3d_* entry points ("neck"), at the BASELINE shapes and a seeded sweep: written before
    read, the planner's intervals cover the real ones, no aliasing, layout, side sites, chained maxima (tests/plan_check.py)."""
    rng = random.Random(20240607)
    n_plans = n_steps = n_site_plans = n_reused = 0
    fuse_seen, sites_by_family, kitti_pair_fuse = set(), {}, set()
    baseline = {}
    for fam in pw.FAMILIES:
        model = pw.family_model(fam)
        for mode in MODES:
            hd = pw.Handle(cpu_lib, model, *mode)
            try:
                shapes = pw.FULL_SHAPES[fam] + _sweep_shapes(fam, rng, 6)
                for shape in shapes:
                    for what in pw.plans_of(fam):
                        plan, total = hd.plan(what, *shape)
                        try:
                            st = check_plan(plan, total)
                        except PlanDefect as e:
                            raise AssertionError(f'{fam} storage/trunk/wino {mode} plan "{what}" at (B, V, H, W) = {shape}: {e}') from None
                        assert st['steps'] == plan['info']['s1'] - plan['info']['s0'] > 0            # every step of the range was visited
                        n_plans += 1
                        n_steps += st['steps']
                        n_reused += st['reused']
                        fuse_seen.update(st['fuse'])
                        if st['n_sides'] > 0:
                            n_site_plans += 1
                            sites_by_family[fam] = sites_by_family.get(fam, 0) + 1
                        if fam == 'kitti' and mode == (0, 4, 4):
                            kitti_pair_fuse.update(st['fuse'])
                        if shape == pw.FULL_SHAPES[fam][0] and mode == (0, 4, 4) and what == 'detect':
                            baseline[fam] = (st['total'], st['ws_bytes'], st['ws2_bytes'])
            finally:
                hd.close()
    print(f'plans checked {n_plans} ({n_steps} steps), plans with side sites {n_site_plans}, fuse values seen {sorted(fuse_seen)}, '
          f'reused arena offsets seen {n_reused}')
    for fam, (total, ws, ws2) in baseline.items():
        print(f'  {fam} detect at {pw.FULL_SHAPES[fam][0]}: total {total} bytes, workspace {ws}, second workspace {ws2}')
    assert n_plans == len(pw.FAMILIES) * len(MODES) * 4 * 6 + sum(len(v) for v in pw.FULL_SHAPES.values()) * len(MODES) * 4      # no plan skipped
    assert all(sites_by_family.get(fam, 0) > 0 for fam in pw.FAMILIES), sites_by_family         # every family has a trunk, so side sites
    assert {1, 3, 4, 5} <= kitti_pair_fuse, kitti_pair_fuse                                      # the one-launch forms of the pair chain
    assert n_reused > 0                                                                          # the aliasing rule had offsets to look at


# --------------------------------------------------------------------------------------------------------- the checker itself
def _tensor(off, nbytes, first, last, **kw):
    d = dict(off=off, bytes=nbytes, used=nbytes, slot=-1, first=first, last=last, fmt=0, esz=4, caller_owned=0, boundary=0)
    d.update(kw)
    return d


def _step(i, t_in, t_out, res=-1, **kw):
    d = dict(kind=2, res=res, out=t_out, out2=-1, fuse_out=-1, fuse=0, side=0, join=0, tile=0, pio=0, amax_n=0, amax_in_n=0, n_extra_in=0,
             n_extra_out=0, extra_in=[], extra_out=[], split=0, ws=0, amax_out=-1, amax_in=-1, name=f'conv{i}')
    d['in'] = t_in
    d.update(kw)
    return d


def _toy_plan():
    """A block with a shortcut conv on the side stream, by hand: step 0 conv (image 0 -> 1), 1 fork (1 -> 2, the shortcut), 2 conv (1 -> 3),
    3 conv (3 -> 4), 4 join (4 + shortcut 2 -> 5), 5 conv (5 -> 6, kept to the end).  Tensor 6 reuses the bytes of tensor 1."""
    K = 1024
    cam = 256
    tensors = {0: _tensor(-1, K, -2, 2, caller_owned=1),
               1: _tensor(cam, K, 0, 4), 2: _tensor(cam + K, K, 1, 4), 3: _tensor(cam + 2 * K, K, 2, 3), 4: _tensor(cam + 3 * K, K, 3, 4),
               5: _tensor(cam + 2 * K, K, 4, 5), 6: _tensor(cam, K, 5, 6, boundary=1)}
    steps = {0: _step(0, 0, 1, ws=512), 1: _step(1, 1, 2, side=1, ws=256), 2: _step(2, 1, 3), 3: _step(3, 3, 4), 4: _step(4, 4, 5, res=2, join=1),
             5: _step(5, 5, 6)}
    arena = cam + 4 * K
    info = dict(cam_bytes=cam, arena=arena, ws_off=arena, ws_bytes=512, ws2_off=arena + 512, ws2_bytes=256, total=arena + 768, scal_off=0,
                scal_bytes=0, slot_bytes=512, n_sides=1, s0=0, s1=6, n_steps=6, n_tensors=7)
    return dict(info=info, steps=steps, tensors=tensors)


def test_checker_accepts_the_hand_made_plan():
    st = check_plan(_toy_plan(), 256 + 4 * 1024 + 768)
    assert st['n_sides'] == 1 and st['reused'] >= 2 and st['steps'] == 6


def _freed_early(p):
    p['tensors'][3]['last'] = 2                     # step 3 still reads it


def _output_on_input(p):
    p['tensors'][4]['off'] = p['tensors'][3]['off']  # step 3 reads 3 and writes 4


def _reads_fuse2(p):
    p['steps'][2]['fuse'] = 2                       # nothing launches for step 2, step 3 still reads its output


def _never_joined(p):
    p['steps'][4]['join'] = 0


def _reads_shortcut(p):
    p['steps'][3]['res'] = 2                        # between fork (1) and join (4)


def _ws2_overlaps(p):
    p['info']['ws2_off'] = p['info']['ws_off'] + 256


def _side_input_reused(p):
    p['tensors'][1]['last'] = 2                     # the fork's input must stay until the join: the side launch may still read it
    p['tensors'][4]['off'] = p['tensors'][1]['off']


def _ws2_too_large(p):
    p['info']['ws2_bytes'] = p['info']['ws_bytes']  # sized as the whole workspace instead of the side launches' need
    p['info']['total'] = p['info']['ws2_off'] + p['info']['ws2_bytes']


@pytest.mark.parametrize('break_it,message', [
    (_freed_early, r'live interval: tensor 3 is in use through step 3, the plan frees it after 2'),
    (_output_on_input, r'aliasing: .*tensors? 3 .*4'),
    (_reads_fuse2, r'step 3 reads tensor 3 that only a fuse == 2 step'),
    (_never_joined, r'site 1 is never joined'),
    (_reads_shortcut, r'step 3 between fork 1 and join 4 reads the shortcut tensor 2'),
    (_ws2_overlaps, r'the second workspace .* overlaps the first'),
    (_side_input_reused, r'live interval: tensor 1 is in use through step 4'),
    (_ws2_too_large, r'the second workspace holds 512 bytes, the side launches need 256'),
], ids=['freed-one-step-early', 'output-on-input', 'reader-of-a-fuse2-output', 'site-never-joined', 'reads-shortcut-before-join',
        'second-workspace-on-first', 'side-input-freed-before-join', 'second-workspace-oversized'])
def test_checker_rejects_a_plan_with_one_defect(break_it, message):
    p = copy.deepcopy(_toy_plan())
    break_it(p)
    with pytest.raises(PlanDefect, match=message):
        check_plan(p)


# --------------------------------------------------------------------------------------------------------- per-process switches
def test_switches_in_child_processes_keep_the_invariants_and_take_effect():
    """IVX_SIDE_STREAM=0, IVX_FUSE_BOTTLENECK=0 and IVX_FUSE_STEM=0 are read once per process: one child of the CPU library per switch, one
    shape per family, every plan through the checker -- and the switch took effect (no sites / none of the fuse values it governs)."""
    switches = {'IVX_SIDE_STREAM': None, 'IVX_FUSE_BOTTLENECK': {1, 5}, 'IVX_FUSE_STEM': {3, 4}}
    procs = {name: subprocess.Popen([sys.executable, WORKER, 'plans', '--lib', 'cpu'], env=_child_env(**{name: '0'}), stdout=subprocess.PIPE,
                                    stderr=subprocess.PIPE, text=True) for name in switches}
    for name, banned in switches.items():
        out, err = procs[name].communicate(timeout=900)
        assert procs[name].returncode == 0, f'{name}=0: {err[-2000:]}'
        rec = json.loads([l for l in out.splitlines() if l.startswith('{')][-1])
        assert not rec['defects'], f'{name}=0: {rec["defects"]}'
        plans = rec['plans']
        assert len(plans) == len(pw.FAMILIES) * 4 and {p['family'] for p in plans} == set(pw.FAMILIES)
        fuse = set().union(*[set(p['fuse']) for p in plans])
        if banned is None:
            assert all(p['n_sides'] == 0 and p['ws2_bytes'] == 0 for p in plans), f'{name}=0 left side sites'
        else:
            assert not (fuse & banned), f'{name}=0 left fused steps {fuse & banned}'
            assert any(p['n_sides'] > 0 for p in plans)
        other = {1, 5} if name == 'IVX_FUSE_STEM' else {3, 4} if name == 'IVX_FUSE_BOTTLENECK' else {1, 3, 4, 5}
        assert other <= fuse, f'{name}=0 also switched off {other - fuse}'
        print(f'{name}=0: {len(plans)} plans keep the invariants; sites {sum(p["n_sides"] for p in plans)}, fuse values {sorted(fuse)}')


def test_side_stream_settings_compute_the_same_bits_on_the_cpu_library(tmp_path):
    """The CPU restatement's streams are synchronous, so this pins the side PATH (its own workspace, the fork / join bookkeeping): the small
    KITTI-like model gives bit-identical boundary tensors and detections with IVX_SIDE_STREAM=1 and =0, and steps 3 / 4 repeat steps 1 / 2."""
    res = {}
    for setting in ('1', '0'):
        out = tmp_path / f'side{setting}.npz'
        r = subprocess.run([sys.executable, WORKER, 'run', '--lib', 'cpu', '--config', 'kitti_small', '--out', str(out)],
                           env=_child_env(IVX_SIDE_STREAM=setting), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        res[setting] = np.load(out)
    assert int(res['1']['n_sides']) > 0 and int(res['0']['n_sides']) == 0
    n = compare_runs(res['1'], res['0'], 't0')
    assert int(sum(res['1']['t0_s0_count'])) > 0, 'the case has no detections'
    print(f'kitti_small on the CPU library, IVX_SIDE_STREAM 1 vs 0: bit-identical over {n} arrays x 4 steps')
