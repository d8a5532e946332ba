"""The route of a convolution -- direct, Winograd (which tile, which operands) or split-operand -- is ONE host function of the library,
ivx_conv_route, asked by the native handle and by FusedConv alike.  tests/golden/conv_routes.json holds what the layer-wise Python rule
answered on a grid of layers, shapes and switches before that function existed (tests/plan_worker.py routes, section `layers`): every row
must come out of ivx_conv_route on libimvoxel_hip.so and out of the FusedConv queries unchanged.  No GPU: the rule and its probes are host code.

Also here: the one packer of the split-operand filters, ivx_bf16_pair_pack_filters, against conv.pack_pair_weights and a numpy restatement."""
import ctypes as C
import json

import numpy as np
import torch

import plan_worker as pw

IVX_F16_PAIR, IVX_BF16_PAIR = 4, 3


def _ask(L, f, shape, sw, candidate=False):
    """ivx_conv_route for layer f on the input `shape` (B, D, H, W) under the switches of a fixture row; candidate: the query without a
    shape, with the split rule and the pair operands on (what a host asks when it loads the filters)."""
    from imvoxelnet_amd._lib import ConvDesc, ConvRoute, ConvRouteOpts
    s = dict(pw.ROUTE_DEFAULTS, **sw)
    o = ConvRouteOpts(int(s['winograd']), s['winograd_tile'], IVX_F16_PAIR if candidate else s['wino_operands'], 1 if candidate else int(s['pair_mode'] < 0), -1, 0)
    d = ConvDesc(*((0, 0, 0, 0) if candidate else shape), f.cin_pad, f.cout, *f.kernel, *f.stride, *f.padding, 0, s.get('res_mode', 0), 0, 0, f.layout, 0, 0, 1.0,
                 0, 0, 1.0, 0)
    r = ConvRoute()
    assert L.ivx_conv_route(C.byref(d), f.cin, C.byref(o), C.byref(r)) == 0, L.ivx_last_error()
    return d, r


def _view(d):
    return [[d.B, d.D, d.H, d.W, d.Cin], [d.KD, d.KH, d.KW], [d.sd, d.sh, d.sw], [d.pd, d.ph, d.pw]]


def test_conv_route_answers_the_recorded_rule():
    from imvoxelnet_amd import _lib
    L = _lib.lib()
    fx = json.load(open(pw.ROUTES_FILE))['layers']
    assert fx['switches'] == pw.ROUTE_SWITCHES and [rec[:7] for rec in fx['layers']] == json.loads(json.dumps(pw.ROUTE_LAYERS))
    with pw.route_switches({}):
        layers = [pw.route_layer(rec[:7]) for rec in fx['layers']]
    # what a host keeps when it loads the filters: the candidate flags (FusedConv adds only its own gate, which every layer here passes)
    for f, rec in zip(layers, fx['layers']):
        _, cand = _ask(L, f, None, {}, candidate=True)
        assert (bool(cand.split_candidate), bool(cand.wino_candidate)) == (rec[7], rec[8]) == (bool(f._split_cand), f._w0_host is not None), rec
    views = {(li, tuple(shape)): view for li, shape, *view in fx['views']}
    seen = {'wino': set(), 'split': 0, 'direct': 0, 'prefers': 0}
    n = 0
    for li, shape, wi, m, opnd, pair, prefers in fx['rows']:
        f, sw = layers[li], fx['switches'][wi]
        what = f'layer {fx["layers"][li][:7]} at {shape} under {sw}'
        naive = sw.get('naive', False)
        d, r = _ask(L, f, shape, sw)
        # the library's answer; `naive` (a validation run on the naive kernel) is the caller's own gate in front of both forms
        assert (0 if naive else r.tile if r.form == 1 else 0) == m, what
        assert (0 if naive or r.form != 1 else r.run.wino_operands) == opnd, what
        assert (bool(r.split_fits) and not naive) == pair and bool(r.prefers_winograd) == prefers, what
        assert r.form == (1 if r.tile else 2 if r.split_fits else 0), what                 # the split-operand form only where Winograd refused
        direct = _view(d)
        swapped = [[shape[0], shape[2], shape[3], 1, f.cin], [3, 3, 1], [1, 1, 1], [f.padding[1], f.padding[2], 0]]
        want_view = views[(li, tuple(shape))]
        if r.form == 1:                                                                    # the descriptor to launch: the recorded view
            assert _view(r.run) == want_view and want_view == (swapped if f._dims == 2 else direct), what
        else:           # not taken: the recorded view is one nobody launches (a 2-D 3x3 layer's is still the swapped one); the route hands out the direct form
            assert want_view == (swapped if f.kernel == (1, 3, 3) and f.stride == (1, 1, 1) else direct), what
            assert _view(r.run) == direct and r.run.wgt_layout == (1 if r.form == 2 else f.layout), what
            assert r.run.in_dtype == (IVX_BF16_PAIR if r.form == 2 else 0), what
        # the FusedConv queries: thin readings of the same call
        ans, view = pw.route_answer(f, shape, sw)
        assert ans == [m, opnd, pair, prefers], what
        assert view == (want_view if m else direct), what
        seen['wino'].add((m, opnd))
        seen['split'] += pair and not m
        seen['direct'] += not pair and not m
        seen['prefers'] += prefers
        n += 1
    assert n == len(fx['rows']) == sum(len(pw.ROUTE_SHAPES_3D if f._dims == 3 else pw.ROUTE_SHAPES_2D) for f in layers) * len(pw.ROUTE_SWITCHES)
    # the grid reaches every form: all three tiles with both operand types where they exist, the split-operand form, the direct form, the predicate
    assert {(2, 0), (4, 0), (4, 4), (6, 0), (6, 4), (0, 0)} <= seen['wino'] and seen['split'] and seen['direct'] and seen['prefers'], seen


def test_route_is_asked_once_per_shape():
    """FusedConv keeps the route of a shape: the queries of one __call__ (wino_tile, takes_pair_form, the operands) are one library call the
    first time and none afterwards (before: ivx_conv_winograd_supported and ivx_conv_pair_supported on every call)."""
    from imvoxelnet_amd import _lib
    L = _lib.lib()
    f = pw.route_layer((128, 64, (3, 3, 3), (2, 2, 2), 1, 3, None))
    calls = []
    real = L.ivx_conv_route

    def counted(*a):
        calls.append(1)
        return real(*a)
    L.ivx_conv_route = counted
    try:
        with pw.route_switches({}):
            for _ in range(3):
                assert f.wino_tile((1, 40, 40, 16, 64))[0] == 0 and f.takes_pair_form((1, 40, 40, 16, 64))
    finally:
        L.ivx_conv_route = real
    assert len(calls) == 1


def _bf16_bits(x):
    """fp32 array -> bf16 bit patterns, round to nearest even (finite values)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _pack_numpy(w, layout):
    co, taps, ci = w.shape
    hi = _bf16_bits(w)
    lo = _bf16_bits(w - (hi.astype(np.uint32) << 16).view(np.float32))
    p = np.concatenate([hi.reshape(co, taps, ci // 16, 16), lo.reshape(co, taps, ci // 16, 16)], -1).reshape(co, taps, 2 * ci)
    return p if layout == 0 else np.ascontiguousarray(p.reshape(co, taps, 2 * ci // 64, 64).transpose(0, 2, 1, 3))


def test_bf16_pair_pack_filters_is_the_one_packer():
    from imvoxelnet_amd import _lib
    from imvoxelnet_amd.conv import pack_pair_weights
    L = _lib.lib()
    g = torch.Generator().manual_seed(7)
    for layout, (co, k, ci) in ((0, (5, (3, 1, 2), 48)), (1, (5, (3, 1, 2), 64)), (0, (3, (1, 1, 1), 16)), (1, (4, (3, 3, 3), 96))):
        taps = k[0] * k[1] * k[2]
        w = torch.randn(co, *k, ci, generator=g) * torch.logspace(-20, 8, ci, base=2.0)      # magnitudes 2^-20 .. 2^8
        w[0, 0, 0, 0, ::5] = 0.0
        w[-1] = 0.0
        want = _pack_numpy(w.reshape(co, taps, ci).numpy(), layout)
        got = torch.empty(want.size, dtype=torch.bfloat16)
        assert L.ivx_bf16_pair_pack_filters(C.c_void_p(w.data_ptr()), co, taps, ci, layout, C.c_void_p(got.data_ptr())) == 0, L.ivx_last_error()
        py = pack_pair_weights(w, layout)
        assert tuple(py.shape) == ((co, 2 * ci // 64, *k, 64) if layout else (co, *k, 2 * ci)) and py.dtype == torch.bfloat16
        assert np.array_equal(got.view(torch.int16).numpy().view(np.uint16), want.reshape(-1)), (layout, co, k, ci)
        assert np.array_equal(py.reshape(-1).view(torch.int16).numpy().view(np.uint16), want.reshape(-1)), (layout, co, k, ci)
        # ... and the torch statement of the same thing that conv.py held before: hi = bf16(w), lo = bf16(w - hi)
        hi = w.to(torch.bfloat16)
        lo = (w - hi.float()).to(torch.bfloat16)
        t = torch.cat([hi.reshape(co, *k, ci // 16, 16), lo.reshape(co, *k, ci // 16, 16)], dim=-1).reshape(co, *k, 2 * ci)
        if layout == 1:
            t = t.reshape(co, *k, 2 * ci // 64, 64).permute(0, 4, 1, 2, 3, 5)
        assert torch.equal(t.contiguous().view(torch.int16), py.view(torch.int16))
    assert L.ivx_bf16_pair_pack_filters(C.c_void_p(w.data_ptr()), 4, 27, 48, 1, C.c_void_p(got.data_ptr())) != 0 and b'Cin' in L.ivx_last_error()
