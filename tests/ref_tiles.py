"""Every row of the two tile tables of csrc/conv_tiles.h -- IVX_CONV_TILES (the direct kernels, one instantiation per operand family a row
names) and IVX_CONV_HALO_CFGS (the z-halo / z-blocked Winograd-domain GEMMs) -- against plain fp64 at the row's OWN edges: the reader of the
tables, the shapes derived from a row's numbers, the cases (cached: many rows share bm and bn), the plan query that proves the forced row is
what runs, and one driver per operand family.  Shared by tests/test_host_conv_tiles.py (no device) and tests/test_gpu_conv_tiles.py.

No kernel of the project is in here and no reference comes out of the library: the references are ref_conv.accumulate / ref_pair.conv2d /
ref_fp8.Case on the values the operands stand for.  A row added to the header appears in direct_rows() / halo_rows(), and so in every
parametrisation, with no edit here.

Where a tile kernel goes wrong, and the shape that goes there (direct_shapes; S = K slabs of bk stored elements, a pair value is two):
  a  M = bm - 1, Cout = bn - off, one tile, the shortest K loop the family's filter layout allows (K < bk where its smallest Cin is below bk)
  b  M = bm + 1, Cout = bn + off: a partial second M tile and N tile, S just above the ring (nb + 1 where the channel unit allows), residual + ReLU
  c  M = 8 bm + 1: the ninth M tile (tiles are dealt to 8 XCDs: q_total = 2, grid 8 * 2 * Nt), S = 2 exactly, both filter layouts
  d  3x3 pad 1 stride 1 on odd H and W (M >= bm + 1), S odd and no multiple of nb where the family's channel unit allows, residual + ReLU
  e  3x3 pad 1 stride 2 on odd H and W, two samples, Cout = 2 bn + 2 off (three N tiles, the last partial), the smallest Cin that both filter
     layouts take (a 3x3 loop is never shorter than the ring: 9 Cin stored elements are more than bk for every family)
  f  fp32 families: Cout = bn + 2, no multiple of 4, so the one-channel-per-lane epilogue runs by rule
off = 4 (16 where the output or the residual is e4m3 or an fp16 pair tensor: those need Cout % 16).  Rows with RPF = 1 take a residual on
every shape.  Where the arithmetic of a family forbids a property (an fp16-pair tensor has 64 stored elements per 32 channels, so S is even
on bk = 32) shape_facts() says so and tests/test_host_conv_tiles.py proves it impossible instead of assuming it."""
import collections
import copy
import ctypes as C
import math
import os
import re

import numpy as np

import ref_conv as R
import ref_fp8 as Q
import ref_pair as P

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TILES_H = os.path.join(ROOT, 'imvoxelnet_amd', 'csrc', 'conv_tiles.h')
IVX_BF16_PAIR, IVX_F16_PAIR = 3, 4

# the family masks of the header's enum, expanded
MASKS = {'GENERIC': ('generic',), 'F32': ('f32',), 'BF16': ('bf16',), 'E4M3': ('e4m3',), 'PAIR_BF16': ('pair_bf16',), 'PAIR_F16': ('pair_f16',),
         'PAIRS': ('pair_bf16', 'pair_f16'), 'BF16_PAIRS': ('bf16', 'pair_bf16', 'pair_f16')}
# per family: channel unit of filter layout 0 / 1 (None: the driver has no such layout), stored elements per channel, multiple of the Cout
# offsets, (in_dtype, out_dtype) of the descriptor, operand rounding of the reference, tolerance
Family = collections.namedtuple('Family', 'unit0 unit1 el off dtypes rounding tol')
PAIR_TOL = (0.0, 2e-5, True)                   # 2e-5 of the output range: the bar of test_conv_bf16_pair_operands and ref_pair.VALUE_TOL
WINO_TOL = (1e-4, 1e-4, True)                  # the bar of test_conv_winograd_f16_pair_operands / test_winograd_halo_kernel_* against fp64
HALO_VS_GENERIC = 2e-5                         # of the range: test_winograd_halo_kernel_matches_generic
FAMILIES = {'generic': Family(4, None, 1, 4, (0, 0), None, R.TOL_F32), 'f32': Family(4, 32, 1, 4, (0, 0), None, R.TOL_F32),
            'bf16': Family(8, 64, 1, 4, (1, 0), 'bf16', R.TOL_BF16_IN), 'e4m3': Family(16, 128, 1, 16, (2, 2), 'e4m3', None),
            'pair_bf16': Family(16, 32, 2, 4, (IVX_BF16_PAIR, 0), None, PAIR_TOL), 'pair_f16': Family(None, 32, 2, 16, (IVX_F16_PAIR, 0), 'f16_pair', PAIR_TOL)}
assert P.VALUE_TOL == PAIR_TOL[1]

DirectRow = collections.namedtuple('DirectRow', 'number family bm bn bk nb rpf')
HaloRow = collections.namedtuple('HaloRow', 'number kind bm bn nbuf tail stride zd')
Shape = collections.namedtuple('Shape', 'tag B H W cin cout k stride res relu layouts')


# ------------------------------------------------------------------------------------------------------------------ the tables
def _text():
    return open(TILES_H).read()


def table_rows():
    """[(number, mask, TM, TN, WR, WC, BK, WPE, NB, RPF, wg_per_cu)] of IVX_CONV_TILES, as written"""
    rows = re.findall(r'^  X\((\d+), (\w+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\)', _text(), re.M)
    return [(int(r[0]), r[1]) + tuple(int(v) for v in r[2:]) for r in rows]


def direct_rows():
    """(number, family, bm, bn, bk, nb, rpf) of every (row, family) pair"""
    return [DirectRow(n, fam, wr * tm * 32, wc * tn * 32, bk, nb, rpf) for n, mask, tm, tn, wr, wc, bk, wpe, nb, rpf, wg in table_rows() for fam in MASKS[mask]]


def halo_mode_stride(mode):
    """the numbering convention of the header (halo_mode_stride): the z stride a halo number is for"""
    return 0 if mode <= 0 else 2 if (21 <= mode < 30 or 40 <= mode < 50 or mode >= 70) else 1


def halo_table():
    """([H rows as written: number, TM, TN, WR, WC, WPE, PAIR, NBUF, TAIL, SW, ZR, DI], [Z rows: number, Z, WCOL, WN, WPE, SW])"""
    t = _text()
    h = [tuple(int(v) for v in r.split(',')) for r in re.findall(r'^  H\((\d+(?:, \d+){11})\)', t, re.M)]
    z = [tuple(int(v) for v in r.split(',')) for r in re.findall(r'^  Z\((\d+(?:, \d+){5})\)', t, re.M)]
    return h, z


def halo_rows():
    """(number, kind, bm, bn, nbuf, tail, stride, zd): bm the rows a tile stages (H) or stores (Z: whole columns, zd output slices each)"""
    h, z = halo_table()
    return [HaloRow(n, 'H', wr * tm * 32, wc * tn * 32, nbuf, tail, halo_mode_stride(n), 0) for n, tm, tn, wr, wc, wpe, pair, nbuf, tail, sw, zr, di in h] + \
           [HaloRow(n, 'Z', zd * wcol * 32, wn * 32, 0, 1, halo_mode_stride(n), zd) for n, zd, wcol, wn, wpe, sw in z]


def halo_bm_eff(row):
    """rows a tile STORES (launch_halo: overlapping tiles, TAIL 0, give up 2 rows at stride 1 -- 3 with the zero row -- and 1 at stride 2)"""
    if row.kind == 'Z' or row.tail:
        return row.bm
    zr = {r[0]: r[10] for r in halo_table()[0]}[row.number]
    return row.bm - (2 + zr if row.stride == 1 else 1)


# ------------------------------------------------------------------------------------------------------------------ direct shapes
def slabs(row, cin, k):
    """K slabs of a k x k layer on cin channels: ceil(k k el cin / bk)"""
    return -(-k * k * FAMILIES[row.family].el * cin // row.bk)


def _units(fam):
    f = FAMILIES[fam]
    return [u for u in (f.unit0, f.unit1) if u]


def _layouts(fam, cin):
    f = FAMILIES[fam]
    return tuple(l for l, u in ((0, f.unit0), (1, f.unit1)) if u and cin % u == 0)


def _cin_for(row, k, want, limit=64):
    """the smallest Cin the family's drivers take (a multiple of one of its channel units) whose K loop satisfies want(S); None if no Cin up
    to `limit` units does"""
    u = min(_units(row.family))
    for c in range(u, limit * u + 1, u):
        if _layouts(row.family, c) and want(slabs(row, c, k)):
            return c
    return None


def _cin_a(row):
    """shape a: the largest Cin with K < bk, else the smallest Cin"""
    f, u = FAMILIES[row.family], min(_units(row.family))
    below = [c for c in range(u, row.bk, u) if f.el * c < row.bk and _layouts(row.family, c)]
    return below[-1] if below else u


def _odd_hw(m_min):
    h = math.isqrt(m_min) | 1
    w = -(-m_min // h) | 1
    return h, w


def direct_shapes(row):
    f = FAMILIES[row.family]
    off = f.off
    rpf = bool(row.rpf)
    mk = lambda tag, B, H, W, cin, cout, k, s, res: Shape(tag, B, H, W, cin, cout, k, s, res or rpf, res or rpf, _layouts(row.family, cin))  # noqa: E731
    ge = lambda n: (lambda S: S >= n)                                                                                                       # noqa: E731
    out = [mk('a', 1, 1, row.bm - 1, _cin_a(row), max(row.bn - off, off), 1, 1, False),
           mk('b', 1, 1, row.bm + 1, _cin_for(row, 1, ge(row.nb + 1)), row.bn + off, 1, 1, True),
           mk('c', 1, 1, 8 * row.bm + 1, 2 * row.bk // f.el, row.bn, 1, 1, False)]
    H, W = _odd_hw(row.bm + 1)
    cd = _cin_for(row, 3, lambda S: S % 2 == 1 and S % row.nb != 0) or _cin_for(row, 3, lambda S: S % row.nb != 0) or min(_units(row.family))
    out.append(mk('d', 1, H, W, cd, row.bn, 3, 1, True))
    out.append(mk('e', 2, H, W, max(_units(row.family)), 2 * row.bn + 2 * off, 3, 2, False))
    if row.family in ('generic', 'f32'):
        out.append(mk('f', 1, 1, row.bm + 1, _cin_for(row, 1, ge(2)), row.bn + 2, 1, 1, False))
    return out


def out_hw(s):
    return P.out_hw(s.H, s.W, s.k, s.stride, s.k // 2)


def shape_facts(row, s):
    """what a generated shape is, by arithmetic: rows, tile counts, slabs, K"""
    ho, wo = out_hw(s)
    M = s.B * ho * wo
    K = s.k * s.k * FAMILIES[row.family].el * s.cin
    return dict(M=M, Mt=-(-M // row.bm), Nt=-(-s.cout // row.bn), q_total=-(-(-(-M // row.bm)) // 8), S=-(-K // row.bk), K=K, rem_m=M % row.bm, rem_n=s.cout % row.bn,
                rem_k=K % row.bk)


# ------------------------------------------------------------------------------------------------------------------ cases and references
_CASES = {}


def _rounding(fam):
    return R.bf16_round if FAMILIES[fam].rounding == 'bf16' else None


def case_of(fam, s):
    """the ref_conv.Case of a shape (fp32 tensors drawn once, fp64 pre-activation computed once), shared by every row and family with the
    same shape and operand rounding.  e4m3: the ref_fp8.Case (form b, or d with its e4m3 residual)."""
    e4 = fam == 'e4m3'
    key = (s.B, s.H, s.W, s.cin, s.cout, s.k, s.stride, s.res, 'e4m3' if e4 else FAMILIES[fam].rounding == 'bf16')
    if key not in _CASES:
        name = 'tile_' + '_'.join(str(v) for v in key)
        if e4:
            _CASES[key] = Q.Case(name, 'd' if s.res else 'b', s.B, (s.H, s.W), s.cin, s.cout, s.k, s.stride, 0, res_std=0.25 if s.res else 0.6,
                                 opts=[fp8_option(s)])
        else:
            _CASES[key] = R.Case(name, s.B, (1, s.H, s.W), s.cin, s.cout, kernel=(1, s.k, s.k), stride=(1, s.stride, s.stride), res_mode=1 if s.res else 0,
                                 rounding=_rounding(fam))
    return _CASES[key].make()


def option(s):
    return dict(after=False, post=1.0, relu=s.relu)


def fp8_option(s):
    return dict(relu=s.relu, res='before' if s.res else None, post=1.0)


def reference(fam, s):
    """fp64 result of a shape for the families whose reference needs no device (every one but the fp16 pairs, whose operands the device packs)"""
    c = case_of(fam, s)
    if fam == 'e4m3':
        o = fp8_option(s)
        return c.expect(o, *Q.folded_f32(c, o)).u
    return c.ref(option(s))


def wrong_results(row, s):
    """The two mistakes of a tile kernel, from the reference alone: (without the last K slab, with the rows of the last partial M tile taken
    from the tile before -- None on a single tile or a whole last tile), next to the right result and the tolerance as an absolute bound.
    The K order is the tap-major one of filter layout 0; bk stored elements are bk / el channels.  Last: the rows whose sum the last slab
    enters at all (on the last rows and columns of a 3x3 layer its tap lies in the padding)."""
    fam, f = row.family, FAMILIES[row.family]
    c = case_of(fam, s)
    per = row.bk // f.el
    Kc = s.k * s.k * s.cin                                   # K in channels, [tap][channel]
    first = (-(-Kc // per) - 1) * per
    if fam == 'e4m3':
        o = fp8_option(s)
        sc, sf, rs = Q.folded_f32(c, o)
        right = c.expect(o, sc, sf, rs).u
        w = c.w_op.reshape(s.cout, -1).copy()
        w[:, first:] = 0.0
        acc = R.accumulate(c.x_op, w.reshape(c.w_op.shape), c.kernel, c.stride, c.padding)
        v = acc * np.asarray(sc, np.float64) + np.asarray(sf, np.float64)
        touched = (acc != c.acc).any(-1).reshape(-1)
        short = Q.finish(v, None if c.r_op is None else c.r_op * float(rs), o['relu'], False, 1.0)
        bound = np.full(right.shape, Q.DELTA_REL * float(np.abs(right).max()))
    else:
        o = option(s)
        right = c.ref(o)
        w = np.asarray(c.w, np.float64).reshape(s.cout, -1).copy()
        w[:, first:] = 0.0
        acc = R.accumulate(c.x, w.reshape(c.w.shape), c.kernel, c.stride, c.padding)
        pre = acc * c.scale.astype(np.float64) + c.shift.astype(np.float64)
        touched = (pre != c.pre).any(-1).reshape(-1)
        short = R.finish(pre, c.res_up, o['relu'], False, 1.0)
        bound = R.bound_of(right, f.tol)
    M = right.size // s.cout
    r2, moved = right.reshape(M, s.cout), None
    full = (M // row.bm) * row.bm
    if M % row.bm and full:
        moved = r2.copy()
        moved[full:] = r2[full - row.bm:M - row.bm]
        moved = moved.reshape(right.shape)
    return right, short, moved, bound, touched


# ------------------------------------------------------------------------------------------------------------------ the plan query
def direct_desc(row, s, layout, pio=False, out_pair=False):
    """(ivx_conv_desc, ivx_pair_io or None) of a direct shape as the family's driver hands it to the library"""
    f = FAMILIES[row.family]
    pad = s.k // 2
    d = P.ConvDesc(s.B, 1, s.H, s.W, s.cin, s.cout, 1, s.k, s.k, 1, s.stride, s.stride, 0, pad, pad, int(s.relu), 1 if s.res else 0, 0, 0, layout, 0, 0, 1.0,
                   f.dtypes[0], IVX_F16_PAIR if out_pair else f.dtypes[1], 1.0, 0)
    some = C.c_void_p(64)                                    # (never read: the query makes no device call)
    return d, (P.PairIO(some, some, IVX_F16_PAIR, some, some, some, some, 1.0, 1.0) if pio else None)


def grouped_desc(B, X, Y, Z, cin, cout, stride, operands, tile=4):
    """descriptor of ONE xi convolution of an F(tile x tile, 3x3) layer (winograd.hip wino_group_desc): volume [B, TX, TY, Z, Cin], 1x1x3 along z"""
    return P.ConvDesc(B, -(-X // tile), -(-Y // tile), Z, cin, cout, 1, 1, 3, 1, 1, stride, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1.0, operands, 0, 1.0, operands)


def plan_query(L, d, io=None, groups=0):
    """ivx_conv_plan_query (no device call): (rc, record)"""
    from imvoxelnet_amd import _lib
    r = _lib.ConvPlanRec()
    d = _lib.ConvDesc.from_buffer_copy(bytes(d))             # (the binding's own structures: same fields as ref_pair's)
    io = None if io is None else _lib.PairIO.from_buffer_copy(bytes(io))
    rc = L.ivx_conv_plan_query(C.byref(d), C.byref(io) if io is not None else None, 1, groups, C.byref(r))
    return rc, r


def assert_direct_plan(L, row, s, layout, pio=False, out_pair=False):
    """under the override the plan names the row and plans no split: this is how a test knows the row ran"""
    rc, r = plan_query(L, *direct_desc(row, s, layout, pio, out_pair))
    assert rc == 0, L.ivx_last_error()
    assert r.n_slices == 1 and r.cfg[0] == row.number and r.ksplit[0] == 1 and r.tail_ks[0] == 1 and r.ws_bytes == 0, \
        f'{row.family} {row.number} shape {s.tag}: the plan says tile {r.cfg[0]}, ksplit {r.ksplit[0]}, tail {r.tail_ks[0]}, workspace {r.ws_bytes}'
    if row.family != 'generic':
        f = shape_facts(row, s)
        assert r.bm[0] == row.bm and r.q_total[0] == f['q_total'], (row, s.tag, r.bm[0], r.q_total[0])
    return r


class forced:
    """with forced(L, tile=N, halo=M): the per-thread lab knobs, put back to their defaults (0, -1) on exit"""

    def __init__(self, L, tile=0, halo=-1):
        self.L, self.tile, self.halo = L, tile, halo

    def __enter__(self):
        assert self.L.ivx_conv_set_tile_override(self.tile) == 0 and self.L.ivx_conv_set_halo_mode(self.halo) == 0

    def __exit__(self, *exc):
        self.L.ivx_conv_set_tile_override(0)
        self.L.ivx_conv_set_halo_mode(-1)
        return False


# ------------------------------------------------------------------------------------------------------------------ guards
GUARD_BYTE = 0xA5


def guard_elems(row, cout):
    return row.bm * cout


def check_guard(name, guard_bytes):
    """the bm * Cout elements behind the output still hold the pattern: no partial tile stored past M"""
    g = np.asarray(guard_bytes, np.uint8)
    bad = int((g != GUARD_BYTE).sum())
    assert bad == 0, f'{name}: {bad} bytes behind the output were overwritten (first at byte {int(np.argmax(g != GUARD_BYTE))})'


# ------------------------------------------------------------------------------------------------------------------ fp32 driver (either backend)
def run_f32(be, row, s, layout):
    """ivx_conv_fwd_ws on fp32 tensors (ref_conv.run_direct with a guard behind the NaN-filled output); returns the output as numpy.  `be` is
    ref_conv.HostBackend (the CPU restatement) or the device twin."""
    c, o = case_of(row.family, s), option(s)
    d, _ = direct_desc(row, s, layout)
    d = be.ConvDesc.from_buffer_copy(bytes(d))
    n, g = int(np.prod(c.oshape)), guard_elems(row, s.cout)
    x, w = be.up(c.x), be.up(R.pack_layout1(c.w) if layout == 1 else c.w)
    sc, sf = be.up(c.scale), be.up(c.shift)
    res = None if c.res is None else be.up(c.res)
    buf = be.up(np.concatenate([np.full(n, np.nan, np.float32), np.frombuffer(bytes([GUARD_BYTE]) * (4 * g), np.float32)]))
    nb = int(be.L.ivx_conv_workspace_bytes(C.byref(d)))
    assert nb >= 0, 'ivx_conv_workspace_bytes'
    ws = be.full((max(nb, 256),), np.uint8, 0)
    be.ok(be.L.ivx_conv_fwd_ws(C.byref(d), P._p(be, x), P._p(be, w), P._p(be, sc), P._p(be, sf), P._p(be, res), P._p(be, buf), P._p(be, ws), nb, be.stream),
          'ivx_conv_fwd_ws')
    got = np.asarray(be.get(buf))
    check_guard(f'{row.family} {row.number} shape {s.tag} layout {layout}', got[n:].view(np.uint8))
    return got[:n].reshape(c.oshape)


# ------------------------------------------------------------------------------------------------------------------ device drivers
def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def guarded_out(shape, dtype, n_guard):
    """(output view pre-filled with NaN -- e4m3: the NaN byte 0x7F --, the guard as a uint8 view) of one device allocation"""
    import torch
    n = int(np.prod(shape))
    if dtype == Q.FP8:
        buf = torch.full((n + n_guard,), 0x7F, device='cuda', dtype=torch.uint8)
        buf[n:] = GUARD_BYTE
        return buf[:n].view(Q.FP8).view(tuple(shape)), buf[n:]
    buf = torch.full((n + n_guard,), float('nan'), device='cuda', dtype=dtype)
    buf[n:].view(torch.uint8).fill_(GUARD_BYTE)
    return buf[:n].view(tuple(shape)), buf[n:].view(torch.uint8)


def run_lowp(ops, row, s, layout):
    """ops.conv_fwd for the bf16, bf16-pair and e4m3 families on a guarded output; returns the output as numpy (e4m3: the bytes)"""
    import torch
    fam = row.family
    c = case_of(fam, s)
    name = f'{fam} {row.number} shape {s.tag} layout {layout}'
    if fam == 'e4m3':
        o = fp8_option(s)
        c2 = copy.copy(c)
        c2.layout = layout
        x, w, res = Q.to_device(c2)
        sc, sf, rs = Q.folded_f32(c, o)
        out, guard = guarded_out(c.oshape, Q.FP8, guard_elems(row, s.cout))
        y = ops.conv_fwd(x, w, _dev(sc), _dev(sf), c.kernel, c.stride, c.padding, o['relu'], res if o['res'] else None, 1 if o['res'] else 0, out=out,
                         wgt_layout=layout, res_after_act=False, post_scale=1.0, out_dtype=Q.FP8, res_scale=rs)
        torch.cuda.synchronize()
        check_guard(name, guard.cpu().numpy())
        return Q.to_host(c, y)
    o = option(s)
    if fam == 'bf16':
        x, w = _dev(c.x, torch.bfloat16), _dev(R.pack_layout1(c.w, 64) if layout == 1 else c.w, torch.bfloat16)
    else:
        from imvoxelnet_amd.conv import pack_pair_weights
        x, w = ops.bf16_pair_split(_dev(c.x)), pack_pair_weights(torch.from_numpy(c.w), layout).cuda()
    out, guard = guarded_out(c.oshape, torch.float32, guard_elems(row, s.cout))
    y = ops.conv_fwd(x, w, _dev(c.scale), _dev(c.shift), c.kernel, c.stride, c.padding, o['relu'], None if c.res is None else _dev(c.res), c.res_mode, out=out,
                     wgt_layout=layout, out_dtype=torch.float32, pair=fam == 'pair_bf16')
    torch.cuda.synchronize()
    check_guard(name, guard.cpu().numpy())
    return y.cpu().numpy()


def pio_operands(ops, make_pair, s, c):
    """The pair-IO operands of a case, made once: the input and the residual as device pair tensors (make_pair of tests/test_gpu_pair_chain.py),
    the filters packed by ivx_pair_pack_filters -- and the fp64 reference on the values those bytes stand for, decoded here."""
    import torch
    if getattr(c, 'pio', None) is None:
        xp = make_pair(_dev(c.x))
        wt = torch.from_numpy(np.ascontiguousarray(c.w.reshape(s.cout, s.k * s.k, s.cin)))
        packed, sp, wb, sb = ops.pair_pack_filters(wt, torch.from_numpy(c.scale), torch.from_numpy(c.shift))
        rp = make_pair(_dev(c.res)) if c.res is not None else None
        xv = P.pair_decode(xp.data.cpu().numpy()[:, 0], xp.scale())
        rv = None if rp is None else P.pair_decode(rp.data.cpu().numpy()[:, 0], rp.scale())
        ref = P.conv2d(xv, P.filters_decode(packed.numpy()), sp.numpy(), c.shift, s.k, s.stride, s.k // 2, s.relu, rv, 1 if s.res else 0)
        a_in, a_res = xp.amax(), (rp.amax() if rp is not None else 0.0)
        allowed = P.allowed_scales(P.conv_bound(a_in, wb, sb, a_res), P.conv_bound(a_in, wb, sb, a_res, f=np.float32))
        c.pio = dict(x=xp, w=packed.cuda(), sp=sp.cuda(), shift=_dev(c.shift), wb=wb, sb=sb, res=rp, ref=ref, allowed=allowed)
    return c.pio


def run_pio(ops, make_pair, row, s, out_pair):
    """ops.conv_fwd_pio (the wrapper allocates the output: no guard here); returns (dict(data, scale, rec) as ref_pair's checkers take it, reference)"""
    import torch
    c = case_of(row.family, s)
    t = pio_operands(ops, make_pair, s, c)
    pad = s.k // 2
    y = ops.conv_fwd_pio(t['x'], t['w'], t['sp'], t['shift'], (1, s.k, s.k), (1, s.stride, s.stride), (0, pad, pad), s.relu, t['wb'], t['sb'], res=t['res'],
                         res_mode=1 if s.res else 0, out_pair=out_pair)
    torch.cuda.synchronize()
    if out_pair:
        assert isinstance(y, ops.PairTensor), 'a pair output was asked for'
        return dict(data=y.data.cpu().numpy()[:, 0], scale=y.scale(), rec=y.amax()), t['ref'], t['allowed']
    return dict(data=y.cpu().numpy()[:, 0], scale=1.0, rec=float(y.ivx_slots[:ops.AMAX_SLOTS].view(torch.float32).max())), t['ref'], t['allowed']


# ------------------------------------------------------------------------------------------------------------------ Winograd layers: halo, z-blocked, grouped
# F(4x4, 3x3) layers with chunk-major filters, z kernel 3, padding 1: (B, X, Y, Z), Cin, Cout per z stride.  Rows per Winograd position:
# M = B ceil(X/4) ceil(Y/4) Zout.  stride 1: 60 rows (less than any tile); 540 rows x 192 channels (three tiles of 254 and five of 126, each with a
# partial last one, a full and a partial 128-column tile, 3-slice columns for the z-blocked rows 50 / 51); 336 rows x 256 channels (a full
# 256-column tile on two M tiles, 6-slice columns for row 60); 210 rows of 7-slice columns (7 divides none of 125, 128, 253, 254, 256: a tile
# boundary inside a column -- but 126 = 7 * 18, and 3, 5, 6 divide 126 or leave one tile, so the overlapping 126-row tiles get 260 rows of 13-slice
# columns: 13 divides none of them).  stride 2: 24 rows; 540 rows x 192 from 6 -> 3 slices (row 71); 336 rows x 256.
HALO_SHAPES = {1: [((1, 13, 10, 5), 64, 64), ((2, 38, 33, 3), 64, 192), ((1, 30, 27, 6), 128, 256), ((1, 22, 18, 7), 64, 64), ((1, 18, 14, 13), 64, 64)],
               2: [((1, 13, 10, 4), 64, 64), ((2, 38, 33, 6), 64, 192), ((1, 30, 27, 12), 128, 256)]}
GROUPED_SHAPE = HALO_SHAPES[1][1]
WINO_TILE = 4
WINO_OPTION = dict(after=False, post=1.0, relu=True)


def halo_shapes(stride):
    return HALO_SHAPES[stride]


def halo_rows_m(shape, stride):
    (B, X, Y, Z), ci, co = shape
    zo = (Z + 2 - 3) // stride + 1
    return B * -(-X // WINO_TILE) * -(-Y // WINO_TILE) * zo, zo


def zblk_fits(row, shape):
    """a z-blocked row is built for columns of zd output slices (stride 2: from 2 zd input slices); the launcher refuses every other height"""
    (B, X, Y, Z), ci, co = shape
    return halo_rows_m(shape, row.stride)[1] == row.zd and (row.stride == 1 or Z == 2 * row.zd)


def wino_case(shape, stride):
    """the ref_conv.Case of a Winograd layer (BN scale / shift and ReLU, no residual), fp64 reference computed once"""
    (B, X, Y, Z), ci, co = shape
    key = ('wino', shape, stride)
    if key not in _CASES:
        _CASES[key] = R.Case(f'wino_{B}_{X}_{Y}_{Z}_{ci}_{co}_s{stride}', B, (X, Y, Z), ci, co, stride=(1, 1, stride), res_mode=0)
    return _CASES[key].make()


def wino_desc(shape, stride, operands):
    (B, X, Y, Z), ci, co = shape
    return grouped_desc(B, X, Y, Z, ci, co, stride, operands, WINO_TILE)


def run_wino(ops, row_bm, shape, stride, operands):
    """ops.conv_winograd_fwd under the knobs the caller set, on a guarded NaN-filled output; returns the output as numpy"""
    import torch
    c = wino_case(shape, stride)
    key = f'u{operands}'
    if getattr(c, key, None) is None:
        setattr(c, key, (ops.conv_winograd_weights(_dev(c.w), 1, WINO_TILE, operands=operands), _dev(c.x), _dev(c.scale), _dev(c.shift)))
    u, x, sc, sf = getattr(c, key)
    out, guard = guarded_out(c.oshape, torch.float32, row_bm * c.cout)
    y = ops.conv_winograd_fwd(x, u, sc, sf, 3, stride, (1, 1, 1), True, None, out=out, wgt_layout=1, operands=operands)
    torch.cuda.synchronize()
    check_guard(f'winograd {shape} stride {stride} operands {operands}', guard.cpu().numpy())
    return y.cpu().numpy()
