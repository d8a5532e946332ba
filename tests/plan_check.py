"""TEST INFRASTRUCTURE.  A checker of the model handle's plans (csrc/model.cpp make_plan / run_steps) that shares no code with the planner.

read_plan() copies a cached plan out of a library (libimvoxel_hip.so or the CPU restatement of the same ABI) through the read-only view of
include/imvoxel_lab.h into plain dicts.  check_plan() first derives, from the step list alone, what every launch reads and writes and how long
every tensor is really in use -- and only then compares with what the plan says: the planner's live intervals, the arena offsets, the
workspaces, the side stream's sites and the chained per-workgroup maxima.  The first violated invariant raises PlanDefect with a message that
names it.  The rules of the step list (what a `fuse` value means, which steps a side site spans) are those documented in the header."""
import ctypes as C

ALIGN = 256
INF = 1 << 30


class PlanDefect(AssertionError):
    pass


def _align(v):
    return (v + ALIGN - 1) // ALIGN * ALIGN


def read_plan(L, h, what, B, V, H, W):
    """The cached plan `what` of (B, V, H, W) as {'info': {...}, 'steps': {i: {...}}, 'tensors': {t: {...}}} (plain ints / strings)."""
    from imvoxelnet_amd._lib import PlanInfo, PlanStep, PlanTensor, declare_plan_view
    declare_plan_view(L)
    L.ivx_last_error.restype = C.c_char_p
    key = (h, what.encode(), B, V, H, W)

    def ok(rc):
        if rc != 0:
            raise RuntimeError(f'plan view {what} {(B, V, H, W)}: {L.ivx_last_error().decode()}')

    info = PlanInfo()
    ok(L.ivx_model_plan_info(*key, C.byref(info)))
    plan = {'info': {n: int(getattr(info, n)) for n, _ in PlanInfo._fields_}, 'steps': {}, 'tensors': {}, 'key': (what, B, V, H, W)}
    rec = PlanStep()
    for i in range(info.s0, info.s1):
        ok(L.ivx_model_plan_step(*key, i, C.byref(rec)))
        d = {n: int(getattr(rec, n)) for n, t in PlanStep._fields_ if t in (C.c_int32, C.c_int64)}
        d['in'] = d.pop('in_')
        d['extra_in'] = [int(v) for v in rec.extra_in[:rec.n_extra_in]]
        d['extra_out'] = [int(v) for v in rec.extra_out[:rec.n_extra_out]]
        d['name'] = rec.name.decode()
        plan['steps'][i] = d
    trec = PlanTensor()
    for t in range(info.n_tensors):
        ok(L.ivx_model_plan_tensor(*key, t, C.byref(trec)))
        plan['tensors'][t] = {n: int(getattr(trec, n)) for n, _ in PlanTensor._fields_}
    return plan


def _ids(*ts):
    out = []
    for t in ts:
        if t >= 0 and t not in out:
            out.append(t)
    return out


def _overlap(a0, a1, b0, b1):
    """Half-open byte ranges [a0, a1) and [b0, b1) share a byte."""
    return a0 < b1 and b0 < a1 and a1 > a0 and b1 > b0


def derive_io(plan):
    """What every step of the range launches, from the step list alone: {i: (reads, writes)} tensor ids, and the nominal writers of the covered
    (fuse == 2) steps.  fuse 0: the step itself; 1 / 5 / 4: one launch for a block of steps (see imvoxel_lab.h), which reads what the block's
    steps read from outside the block; 3: reads its input only; 2: nothing."""
    info, steps = plan['info'], plan['steps']
    s0, s1 = info['s0'], info['s1']
    if sorted(steps) != list(range(s0, s1)):
        raise PlanDefect(f'step records {sorted(steps)[:3]}.. do not cover the range [{s0}, {s1})')
    io, covered = {}, {}
    for i in range(s0, s1):
        st = steps[i]
        f = st['fuse']
        own_r, own_w = _ids(st['in'], st['res'], *st['extra_in']), _ids(st['out'], st['out2'], *st['extra_out'])
        if f == 0:
            io[i] = (own_r, own_w)
        elif f == 2:
            io[i] = ([], [])
        elif f == 3:
            io[i] = (_ids(st['in']), [])
        elif f in (1, 5, 4):
            block, want = {1: ([i, i + 1, i + 2], [1, 2, 2]), 5: ([i - 1, i, i + 1, i + 2], [2, 5, 2, 2]), 4: ([i - 2, i - 1, i], [3, 2, 4])}[f]
            if block[0] < s0 or block[-1] >= s1 or [steps[k]['fuse'] for k in block] != want:
                raise PlanDefect(f'step {i}: fused block (fuse {f}) needs the steps {block} with fuse {want} inside the range')
            inside = set()
            for k in block:
                inside.update(_ids(steps[k]['out'], steps[k]['out2'], *steps[k]['extra_out']))
                if steps[k]['fuse'] == 2:
                    if k in covered:
                        raise PlanDefect(f'step {k} (fuse 2) is covered by two fused launches ({covered[k]} and {i})')
                    covered[k] = i
            reads = []
            for k in block:
                reads += [t for t in _ids(steps[k]['in'], steps[k]['res'], *steps[k]['extra_in']) if t not in inside and t not in reads]
            if f == 4:
                writes = own_w
            else:
                if st['fuse_out'] != steps[block[-1]]['out'] or st['fuse_out'] < 0:
                    raise PlanDefect(f"step {i}: fuse_out {st['fuse_out']} is not the output of the block's last step {block[-1]}")
                writes = [st['fuse_out']]
            io[i] = (reads, writes)
        else:
            raise PlanDefect(f'step {i}: unknown fuse value {f}')
        if f not in (1, 5) and st['fuse_out'] >= 0:
            raise PlanDefect(f'step {i}: fuse_out set on a step with fuse {f}')
    return io, covered


def check_plan(plan, expect_total=None):
    """Raise PlanDefect at the first violated invariant; return counts of what was exercised."""
    info, steps, T = plan['info'], plan['steps'], plan['tensors']
    s0, s1 = info['s0'], info['s1']
    io, covered = derive_io(plan)
    arena = info['arena']

    # ---- written before read
    nominal = {}                                     # tensors a covered step would have written
    for i in range(s0, s1):
        if steps[i]['fuse'] == 2:
            for t in _ids(steps[i]['out'], steps[i]['out2']):
                nominal[t] = i
    writer, real_last = {}, {}
    for i in range(s0, s1):
        reads, writes = io[i]
        for t in reads:
            if T[t]['caller_owned']:
                continue
            if t not in writer:
                if t in nominal:
                    raise PlanDefect(f'written before read: step {i} reads tensor {t} that only a fuse == 2 step ({nominal[t]}) "wrote"')
                raise PlanDefect(f'written before read: step {i} reads tensor {t} that no earlier launch of the range wrote')
            real_last[t] = max(real_last[t], i)
        for t in writes:
            if T[t]['caller_owned']:
                raise PlanDefect(f'step {i} writes the caller-owned input tensor {t}')
            if t in writer:
                raise PlanDefect(f'tensor {t} is written twice (steps {writer[t]} and {i})')
            writer[t] = i
            real_last[t] = i
    for k in range(s0, s1):
        if steps[k]['fuse'] == 2 and k not in covered:
            raise PlanDefect(f'step {k} has fuse == 2 but no fused launch covers it')

    # ---- side sites (structure first: the real intervals depend on them)
    forks, joins = {}, {}
    for i in range(s0, s1):
        for name, d in (('side', forks), ('join', joins)):
            n = steps[i][name]
            if n:
                if not 1 <= n <= info['n_sides']:
                    raise PlanDefect(f"side sites: step {i} names site {n}, the plan has n_sides = {info['n_sides']}")
                d.setdefault(n, []).append(i)
    sites = []
    for n in range(1, info['n_sides'] + 1):
        if len(forks.get(n, [])) != 1:
            raise PlanDefect(f'side sites: site {n} has {len(forks.get(n, []))} fork steps')
        if len(joins.get(n, [])) != 1:
            raise PlanDefect(f'side sites: site {n} is never joined' if not joins.get(n) else f'side sites: site {n} has {len(joins[n])} join steps')
        i, j = forks[n][0], joins[n][0]
        if j <= i:
            raise PlanDefect(f'side sites: site {n} joins at step {j}, not after its fork {i}')
        sites.append((i, j, n))
    sites.sort()
    for (i1, j1, n1), (i2, j2, n2) in zip(sites, sites[1:]):
        if i2 <= j1:
            raise PlanDefect(f'side sites: sites {n1} [{i1}, {j1}] and {n2} [{i2}, {j2}] nest or overlap')
    for i, j, n in sites:
        fk, jn = steps[i], steps[j]
        if fk['kind'] != 2 or fk['tile'] != 0 or fk['fuse'] != 0:
            raise PlanDefect(f"side sites: fork step {i} of site {n} must be a direct conv (kind {fk['kind']}, tile {fk['tile']}, fuse {fk['fuse']})")
        if jn['fuse'] != 0 or jn['kind'] != 2:
            raise PlanDefect(f'side sites: join step {j} of site {n} does not launch a conv of its own (the wait would never be issued)')
        if jn['res'] != fk['out']:
            raise PlanDefect(f"side sites: join step {j} of site {n} takes residual {jn['res']}, the fork wrote {fk['out']}")
        for k in range(i + 1, j):
            reads, writes = io[k]
            if fk['out'] in reads:
                raise PlanDefect(f"side sites: step {k} between fork {i} and join {j} reads the shortcut tensor {fk['out']}")
            if fk['out'] in writes or fk['in'] in writes:
                raise PlanDefect(f'side sites: step {k} between fork {i} and join {j} writes a tensor of the side launch')
        for t in (fk['in'], fk['out']):              # the side launch may touch both until the join
            if t in real_last:
                real_last[t] = max(real_last[t], j)

    # ---- the planner's interval covers the real one
    for t in writer:
        if T[t]['boundary']:
            real_last[t] = s1                        # may be read back by the caller
    for t, w in writer.items():
        ti = T[t]
        if ti['off'] < 0 or ti['bytes'] <= 0:
            raise PlanDefect(f'tensor {t} is written by step {w} but has no place in the arena')
        if ti['first'] > w:
            raise PlanDefect(f"live interval: tensor {t} is written at step {w}, the plan allocates it at {ti['first']}")
        plast = ti['last'] if ti['last'] >= 0 else INF       # never read: the planner never releases it
        if plast < real_last[t]:
            raise PlanDefect(f"live interval: tensor {t} is in use through step {real_last[t]}, the plan frees it after {ti['last']}")

    # ---- no aliasing between tensors in use at the same time
    live = sorted(writer)
    reused = 0
    for a_i, a in enumerate(live):
        ta = T[a]
        for b in live[a_i + 1:]:
            tb = T[b]
            if not _overlap(ta['off'], ta['off'] + ta['bytes'], tb['off'], tb['off'] + tb['bytes']):
                continue
            if writer[a] <= real_last[b] and writer[b] <= real_last[a]:
                raise PlanDefect(f"aliasing: tensors {a} [{ta['off']}, +{ta['bytes']}) in use over steps [{writer[a]}, {real_last[a]}] and {b} "
                                 f"[{tb['off']}, +{tb['bytes']}) over [{writer[b]}, {real_last[b]}] overlap in bytes")
            reused += 1
    for i in range(s0, s1):                          # (also implied by the intervals; kept explicit: a launch's output never sits on what it reads)
        reads, writes = io[i]
        for w in writes:
            for r in reads:
                if T[r]['caller_owned'] or r == w:
                    continue
                if _overlap(T[w]['off'], T[w]['off'] + T[w]['bytes'], T[r]['off'], T[r]['off'] + T[r]['bytes']):
                    raise PlanDefect(f'aliasing: step {i} writes tensor {w} onto tensor {r}, which it reads')

    # ---- layout
    for name in ('cam_bytes', 'arena', 'ws_off', 'ws_bytes', 'ws2_off', 'ws2_bytes', 'total', 'scal_off'):
        if info[name] % ALIGN or info[name] < 0:
            raise PlanDefect(f'layout: {name} = {info[name]} is not a non-negative multiple of {ALIGN}')
    regions = [('camera block', 0, info['cam_bytes'])]
    for t, ti in T.items():
        if ti['off'] >= 0 and not ti['caller_owned'] and ti['bytes'] > 0:
            if ti['off'] % ALIGN:
                raise PlanDefect(f"layout: tensor {t} at offset {ti['off']} is not {ALIGN}-byte aligned")
            regions.append((f'tensor {t}', ti['off'], ti['off'] + ti['bytes']))
    amax = {}
    for i in range(s0, s1):
        st = steps[i]
        if st['amax_out'] >= 0:
            if st['amax_n'] <= 0 or st['amax_out'] % ALIGN:
                raise PlanDefect(f"layout: step {i} has maxima at {st['amax_out']} with {st['amax_n']} entries")
            if st['amax_out'] in amax:
                raise PlanDefect(f"layout: steps {amax[st['amax_out']]} and {i} write their maxima to the same offset")
            amax[st['amax_out']] = i
            regions.append((f'maxima of step {i}', st['amax_out'], st['amax_out'] + 4 * st['amax_n']))
    if info['scal_bytes'] > 0:
        regions.append(('scalar blocks', info['scal_off'], info['scal_off'] + info['scal_bytes']))
    for name, a0, a1 in regions:
        if a0 < 0 or a1 > arena:
            raise PlanDefect(f'layout: {name} [{a0}, {a1}) lies outside the arena [0, {arena})')
    order = sorted(regions, key=lambda r: r[1])
    tensors_only = lambda a, b: a.startswith('tensor') and b.startswith('tensor')      # noqa: E731  (tensor pairs: the aliasing rule above)
    for a_i, (na, a0, a1) in enumerate(order):
        for nb, b0, b1 in order[a_i + 1:]:
            if b0 >= a1:
                break
            if not tensors_only(na, nb) and _overlap(a0, a1, b0, b1):
                raise PlanDefect(f'layout: {na} [{a0}, {a1}) overlaps {nb} [{b0}, {b1})')
    w0, w1 = info['ws_off'], info['ws_off'] + info['ws_bytes']
    if w0 < arena:
        raise PlanDefect(f'layout: the workspace [{w0}, {w1}) overlaps the arena [0, {arena})')
    end = w1
    if info['n_sides'] > 0:
        v0, v1 = info['ws2_off'], info['ws2_off'] + info['ws2_bytes']
        if v0 <= 0:
            raise PlanDefect('layout: the plan has side sites but no second workspace')
        if v0 < arena:
            raise PlanDefect(f'layout: the second workspace [{v0}, {v1}) overlaps the arena [0, {arena})')
        if _overlap(w0, w1, v0, v1) or (v0 < w1 and v0 >= w0):
            raise PlanDefect(f'layout: the second workspace [{v0}, {v1}) overlaps the first [{w0}, {w1})')
        end = max(w1, v1)
        need = _align(max(steps[i]['ws'] for i, _, _ in sites))
        if info['ws2_bytes'] != need:
            raise PlanDefect(f"layout: the second workspace holds {info['ws2_bytes']} bytes, the side launches need {need} "
                             f"(the {ALIGN}-byte-aligned maximum of ws over the fork steps)")
    elif info['ws2_off'] != 0 or info['ws2_bytes'] != 0:
        raise PlanDefect('layout: a second workspace exists without side sites')
    if end != info['total']:
        raise PlanDefect(f"layout: the workspaces end at {end}, total is {info['total']}")
    if expect_total is not None and expect_total != info['total']:
        raise PlanDefect(f"layout: total is {info['total']}, the workspace query returned {expect_total}")
    for i in range(s0, s1):
        if not 0 <= steps[i]['ws'] <= info['ws_bytes']:
            raise PlanDefect(f"layout: step {i} needs {steps[i]['ws']} workspace bytes, the plan holds {info['ws_bytes']}")
    slots = {}
    for t, ti in T.items():
        if ti['slot'] < 0:
            continue
        rel = ti['slot'] - info['scal_off']
        if rel < 0 or rel + info['slot_bytes'] > info['scal_bytes'] or rel % info['slot_bytes']:
            raise PlanDefect(f"layout: the scalar block of tensor {t} at {ti['slot']} lies outside [scal_off, scal_off + scal_bytes)")
        if ti['slot'] in slots:
            raise PlanDefect(f"layout: tensors {slots[ti['slot']]} and {t} share a scalar block")
        slots[ti['slot']] = t

    # ---- chained maxima
    chained = 0
    for i in range(s0, s1):
        st = steps[i]
        if st['amax_in'] >= 0:
            p = writer.get(st['in'])
            if p is None or steps[p]['amax_out'] != st['amax_in'] or steps[p]['amax_n'] != st['amax_in_n']:
                raise PlanDefect(f"chained maxima: step {i} reads {st['amax_in_n']} maxima at {st['amax_in']}, the producer of its input "
                                 f"({p}) leaves {steps[p]['amax_n'] if p is not None else 0} at {steps[p]['amax_out'] if p is not None else -1}")
            chained += 1
        if st['amax_out'] >= 0:
            outs = io[i][1]
            if not any(steps[k]['in'] in outs and steps[k]['amax_in'] == st['amax_out'] for k in range(i + 1, s1)):
                raise PlanDefect(f'chained maxima: step {i} leaves per-workgroup maxima that no later step reads')

    return {'steps': s1 - s0, 'n_sides': info['n_sides'], 'fuse': sorted({steps[i]['fuse'] for i in range(s0, s1)}), 'reused': reused,
            'chained': chained, 'tensors': len(writer), 'total': info['total'], 'ws_bytes': info['ws_bytes'], 'ws2_bytes': info['ws2_bytes']}
