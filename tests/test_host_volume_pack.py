"""Packing scene states without a device: ivx_volume_pack_fwd / ivx_volume_unpack_fwd / ivx_volume_pack_scratch_bytes are declared, bound and
exported and reject bad arguments before any launch; ops.volume_pack_count / volume_pack / volume_unpack_ raise their host errors and leave the
buffers; the numpy reference of tests/ref_volume_pack.py agrees with itself (pack then unpack is the identity on states that meet the precondition,
an all-unseen row has no records, the bf16 mean restores within the derived bound)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ref_volume_pack as RP
from helpers import ROOT

PACK, UNPACK, SCRATCH = 'ivx_volume_pack_fwd', 'ivx_volume_unpack_fwd', 'ivx_volume_pack_scratch_bytes'


@pytest.fixture(autouse=True)
def _library_of_this_version():
    """Everything here, the reference included, states what library version 0.5.6 does: the library under test must be one."""
    from imvoxelnet_amd import _lib
    assert _lib.lib().ivx_version() >= 560, 'the loaded libimvoxel_hip.so predates the 0.5.6 entries'


def test_entry_points_declared_bound_and_exported():
    from imvoxelnet_amd import _lib, _build
    header = open(os.path.join(ROOT, 'include', 'imvoxel.h')).read()
    declared = set(re.findall(r'\b(ivx_[a-z0-9_]+)\s*\(', header))
    L = _lib.lib()
    for name, n_args in ((PACK, 19), (UNPACK, 18), (SCRATCH, 4)):
        assert name in declared, f'{name} is not declared in include/imvoxel.h'
        assert name in _lib.EXPORTS and hasattr(L, name) and getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == n_args, name
        decl = re.search(r'\bint(?:64_t)? ' + name + r'\(([^;]*)\);', header).group(1)
        assert decl.count(',') + 1 == n_args, (name, decl)
        for src in ('model.cpp', 'api_common.cpp'):    # also compiled into the CPU restatement of the ABI, which does not define them
            assert name not in open(os.path.join(ROOT, 'imvoxelnet_amd', 'csrc', src)).read(), (name, src)
    assert L.ivx_version() >= 560 and getattr(L, SCRATCH).restype is ctypes.c_int64
    entry = [e for e in _build.SOURCES if e[0] == 'volume_pack.hip']
    assert len(entry) == 1 and '-ffp-contract=off' in entry[0][1]
    src = open(os.path.join(ROOT, 'imvoxelnet_amd', 'csrc', 'volume_pack.hip')).read()
    assert PACK in src and UNPACK in src and not re.search(r'\basm\b|__asm', src), 'no inline assembly in the file'


def test_scratch_bytes():
    from imvoxelnet_amd import _lib
    L = _lib.lib()
    for B, dims in ((1, (40, 40, 16)), (3, (37, 29, 3)), (40, (216, 248, 12))):
        nvox = dims[0] * dims[1] * dims[2]
        assert L.ivx_volume_pack_scratch_bytes(B, *dims) >= B * -(-nvox // 256) * 4
    for B, dims in ((0, (7, 5, 6)), (1, (0, 5, 6)), (1, (7, -1, 6)), (1, (2048, 1024, 1024))):
        assert L.ivx_volume_pack_scratch_bytes(B, *dims) == -1


def _pack(L, rows=(2, 0), B=None, R=3, dims=(7, 5, 6), C=8, dtype=0, cap=16, sum_=1 << 20, count=2 << 20, wsum=3 << 20, index=4 << 20, payload=5 << 20,
          wsum_out=6 << 20, count_out=7 << 20, n_out=8 << 20, scratch=9 << 20, null=()):
    """The pack entry with dummy device pointers (never dereferenced: every call here is rejected before any launch)."""
    n = len(rows)
    loc = dict(sum_=sum_, count=count, wsum=wsum, index=index, payload=payload, wsum_out=wsum_out, count_out=count_out, n_out=n_out, scratch=scratch)
    p = lambda name: None if name in null or loc[name] is None else ctypes.c_void_p(loc[name])     # noqa: E731
    return getattr(L, PACK)(n if B is None else B, None if 'row' in null else (ctypes.c_int32 * max(1, n))(*rows), R, *dims, C, p('sum_'), p('count'), p('wsum'),
                            dtype, cap, p('index'), p('payload'), p('wsum_out'), p('count_out'), p('n_out'), p('scratch'), None)


def _unpack(L, rows=(2, 0), ns=(3, 0), B=None, R=3, dims=(7, 5, 6), C=8, dtype=0, cap=16, index=4 << 20, payload=5 << 20, wsum_rec=6 << 20, count_rec=7 << 20,
            sum_=1 << 20, count=2 << 20, wsum=3 << 20, null=()):
    n = len(rows)
    loc = dict(index=index, payload=payload, wsum_rec=wsum_rec, count_rec=count_rec, sum_=sum_, count=count, wsum=wsum)
    p = lambda name: None if name in null or loc[name] is None else ctypes.c_void_p(loc[name])     # noqa: E731
    i32 = lambda v: (ctypes.c_int32 * max(1, len(v)))(*v)                                          # noqa: E731
    return getattr(L, UNPACK)(n if B is None else B, None if 'row' in null else i32(rows), None if 'n' in null else i32(ns), cap, p('index'), p('payload'),
                              p('wsum_rec'), p('count_rec'), dtype, R, *dims, C, p('sum_'), p('count'), p('wsum'), None)


def test_argument_validation_without_gpu():
    """Every pre-launch rejection of both entries: status -1 with its message, which names the export; nothing is launched."""
    from imvoxelnet_amd import _lib
    L = _lib.lib()

    def rejected(call, name, word, **kw):
        rc, err = call(L, **kw), L.ivx_last_error()
        assert rc == -1 and word in err and name.encode() in err, (name, kw, rc, err)

    for call, name in ((_pack, PACK), (_unpack, UNPACK)):
        for arg in ('row', 'sum_', 'count') + (('n_out',) if call is _pack else ('n',)):
            rejected(call, name, b'null argument', null=(arg,))
        for kw in (dict(B=0), dict(B=-1), dict(R=0), dict(R=-2), dict(dims=(0, 5, 6)), dict(dims=(7, -1, 6)), dict(dims=(7, 5, 0)), dict(C=0), dict(C=-4)):
            rejected(call, name, b'bad dims', **kw)
        for c in (1, 2, 6, 10):
            rejected(call, name, b'C % 4', C=c)
        for dims in ((2048, 1024, 1024), (65536, 32768, 1), (1290, 1290, 1291)):
            rejected(call, name, b'below 2^31', dims=dims)
        for at in (1, 4, 8):
            rejected(call, name, b'volume_sum must be 16-byte aligned', sum_=(1 << 20) + at)
            rejected(call, name, b'payload must be 16-byte aligned', payload=(5 << 20) + at)
        for at in (1, 2, 4):
            rejected(call, name, b'8-byte aligned for bf16', payload=(5 << 20) + at, dtype=1)
        assert call(L, payload=(5 << 20) + 8, dtype=1, rows=(1, 1)) == -1 and b'distinct' in L.ivx_last_error()      # 8-byte alignment is enough for bf16
        for dt in (2, 3, -1, 7):
            rejected(call, name, b'unknown payload_dtype', dtype=dt)
        for cap in (-1, -100):
            rejected(call, name, b'cap must not be negative', cap=cap)
        for rows in ((2, 3), (-1, 0)):
            rejected(call, name, b'outside [0, 3)', rows=rows)
        rejected(call, name, b'distinct', rows=(1, 1))
        assert b'row 1' in L.ivx_last_error()
    # the pack alone
    rejected(_pack, PACK, b'null scratch', null=('scratch',))
    for arg in ('index', 'payload', 'count_out'):
        rejected(_pack, PACK, b'cap > 0 with a null output', null=(arg,))
    rejected(_pack, PACK, b'both be given or both be NULL', null=('wsum_out',))
    rejected(_pack, PACK, b'both be given or both be NULL', null=('wsum',))
    # ... whose count-only form (cap == 0) needs no outputs: with null outputs the next rule that fails is reported instead
    rejected(_pack, PACK, b'distinct', cap=0, rows=(1, 1), null=('index', 'payload', 'wsum_out', 'count_out'))
    # the unpack alone
    for arg in ('index', 'payload', 'count_rec'):
        rejected(_unpack, UNPACK, b'cap > 0 with a null record list', null=(arg,))
    rejected(_unpack, UNPACK, b'both be given or both be NULL', null=('wsum_rec',))
    rejected(_unpack, UNPACK, b'both be given or both be NULL', null=('wsum',))
    for ns in ((17, 0), (0, -1), (3, 1 << 20)):
        rejected(_unpack, UNPACK, b'outside [0, cap = 16]', ns=ns)
    rejected(_unpack, UNPACK, b'outside [0, cap = 0]', ns=(0, 1), cap=0)
    with pytest.raises(ValueError, match=PACK):
        _lib.check(_pack(L, rows=(1, 1)), PACK)


def _state(R=3, dims=(7, 5, 6), C=8):
    return torch.full((R,) + dims + (C,), 3.0), torch.full((R,) + dims, 9, dtype=torch.int32), torch.full((R,) + dims, 5.0)


def test_ops_raise_their_host_errors_and_leave_the_buffers():
    """Host tensors throughout, so nothing can reach a launch: list, shape and record errors come first, and arguments that pass them stop at the
    first host tensor.  The buffers keep every value."""
    from imvoxelnet_amd import ops
    vol, cnt, ws = _state()
    n = 4
    rec = (np.array([0, 3, 9, 209], np.int32), np.ones((n, 8), np.float32), np.ones(n, np.float32), np.ones(n, np.int32))
    for fn in (ops.volume_pack_count, ops.volume_pack, lambda v, c, r, w=None: ops.volume_unpack_(v, c, r, [rec] * (len(r) if hasattr(r, '__len__') else 1), w)):
        for rows in ([], [0, 0], [3], [-1], [0, 1, 1]):
            with pytest.raises(ValueError, match='rows'):
                fn(vol, cnt, rows, ws)
        for rows in (torch.tensor([0]), 'ab', 0, [0.5], [True]):
            with pytest.raises(TypeError, match='rows'):
                fn(vol, cnt, rows, ws)
        with pytest.raises(ValueError, match=r'\[R,X,Y,Z,C\]'):
            fn(vol[0], cnt, [0], ws)
        with pytest.raises(ValueError, match='C % 4'):
            fn(torch.zeros(3, 7, 5, 6, 6), cnt, [0], ws)
        with pytest.raises(ValueError, match='count must be'):
            fn(vol, cnt[:2], [0], ws)
        with pytest.raises(ValueError, match='wsum must be'):
            fn(vol, cnt, [0], ws[:, :3])
        with pytest.raises(TypeError, match='torch.Tensor'):
            fn(vol.numpy(), cnt, [0], ws)
    with pytest.raises(TypeError, match='dtype'):
        ops.volume_pack(vol, cnt, [0], ws, dtype=torch.float16)
    # everything else is right: the call stops at the first host tensor (there is no CPU fallback)
    for call in (lambda: ops.volume_pack_count(vol, cnt, [0, 2], ws), lambda: ops.volume_pack(vol, cnt, [1], None), lambda: ops.volume_unpack_(vol, cnt, [2], [rec], ws)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
    # the records of an unpack
    bad = lambda **kw: tuple(kw.get(k, v) for k, v in zip(('index', 'payload', 'wsum', 'count'), rec))      # noqa: E731
    for r, words in ((bad(index=np.array([0, 3, 3, 9], np.int32)), 'strictly ascending'), (bad(index=np.array([3, 0, 9, 12], np.int32)), 'strictly ascending'),
                     (bad(index=np.array([0, 3, 9, 210], np.int32)), 'strictly ascending inside'), (bad(index=np.array([-1, 3, 9, 12], np.int32)), 'strictly ascending inside'),
                     (bad(payload=np.ones((n, 4), np.float32)), 'payload'), (bad(payload=np.ones((n + 1, 8), np.float32)), 'payload'),
                     (bad(count=np.ones(n + 1, np.int32)), 'count'), (bad(wsum=np.ones(2, np.float32)), 'wsum'), (bad(wsum=None), 'weight sum iff'),
                     (bad(index=np.zeros((2, 2), np.int32)), 'index')):
        with pytest.raises(ValueError, match=words):
            ops.volume_unpack_(vol, cnt, [1], [r], ws)
    with pytest.raises(ValueError, match='weight sum iff'):
        ops.volume_unpack_(vol, cnt, [1], [rec], None)
    for r in (bad(index=rec[0].astype(np.int64)), bad(payload=rec[1].astype(np.float64)), bad(payload=rec[1].astype(np.float16)), bad(count=rec[3].astype(np.int16)),
              bad(wsum=rec[2].astype(np.float64))):
        with pytest.raises(TypeError, match='records'):
            ops.volume_unpack_(vol, cnt, [1], [r], ws)
    with pytest.raises(TypeError, match='share a dtype'):
        ops.volume_unpack_(vol, cnt, [0, 1], [rec, bad(payload=np.ones((n, 8), np.uint16))], ws)
    for records in ([rec, rec], [], rec[0], [rec[:3]]):
        with pytest.raises(ValueError, match='records'):
            ops.volume_unpack_(vol, cnt, [1], records, ws)
    assert bool((vol == 3).all()) and bool((cnt == 9).all()) and bool((ws == 5).all())


@pytest.mark.parametrize('pattern', ['none', 'all', 'first', 'last', 'alternate', 'third', 'chunks', 'mixed'])
def test_reference_round_trip_is_the_identity(pattern):
    """On a state that meets the precondition (all-zero sums at unseen voxels), F32 pack then unpack gives back every bit -- NaN payloads, -0 and
    denormals included -- and the records are the kept voxels in ascending order."""
    dims, C = (9, 7, 13), 8
    S, cnt, ws = RP.random_state(np.random.default_rng(5), dims, C, pattern)
    idx, pay, wr, cr = RP.pack(S[0], cnt[0], ws[0])
    keep = ((cnt[0] != 0) | (RP.words(ws[0]) != 0)).reshape(-1)
    assert idx.dtype == np.int32 and np.array_equal(idx, np.flatnonzero(keep)) and (np.diff(idx) > 0).all()
    assert len(idx) == {'none': 0, 'all': keep.size, 'first': 1, 'last': 1, 'alternate': (keep.size + 1) // 2}.get(pattern, len(idx))
    if pattern == 'mixed':
        w = RP.words(wr)
        assert ((cr != 0) & (w == 0)).any() and ((cr == 0) & (w != 0)).any() and (w == np.int32(-2 ** 31)).any() and np.isnan(wr).any()
    if pattern == 'first':
        assert idx[0] == 0
    if pattern == 'last':
        assert idx[0] == keep.size - 1
    S2, c2, w2 = RP.unpack(dims, C, (idx, pay, wr, cr))
    assert np.array_equal(RP.words(S2), RP.words(S[0])) and np.array_equal(c2, cnt[0]) and np.array_equal(RP.words(w2), RP.words(ws[0]))
    # without a weight sum the count alone decides
    idx_p, pay_p, wr_p, cr_p = RP.pack(S[0], cnt[0])
    assert wr_p is None and np.array_equal(idx_p, np.flatnonzero(cnt[0].reshape(-1)))
    # ... and sums at unseen voxels, which the precondition excludes, are what a round trip drops
    if 0 < len(idx) < keep.size:
        dirty = S[0].copy().reshape(-1, C)
        dirty[np.flatnonzero(~keep)[0]] = 1.0
        S3, _, _ = RP.unpack(dims, C, RP.pack(dirty.reshape(S[0].shape), cnt[0], ws[0]))
        assert not np.array_equal(RP.words(S3), RP.words(dirty.reshape(S[0].shape))) and np.array_equal(RP.words(S3), RP.words(S[0]))


def test_reference_bf16_round_trip_within_the_derived_bound():
    dims, C = (9, 7, 13), 8
    rng = np.random.default_rng(6)
    for wsum in (True, False):
        S, cnt, ws = RP.random_state(rng, dims, C, 'third', wsum=wsum, raw=False)
        idx, pay, wr, cr = RP.pack(S[0], cnt[0], None if ws is None else ws[0], bf16=True)
        assert pay.dtype == np.uint16 and pay.shape == (len(idx), C)
        S2, c2, w2 = RP.unpack(dims, C, (idx, pay, wr, cr))
        err = np.abs(S2 - S[0].astype(np.float64))
        assert (err <= RP.BF16_BOUND * np.abs(S[0].astype(np.float64))).all() and err.max() > 0 and np.array_equal(c2, cnt[0])
        assert (w2 is None) == (not wsum) and (w2 is None or np.array_equal(RP.words(w2), RP.words(ws[0])))
    # the rounding itself: ties to even at 8 significant bits, the carry into the next binade, signs and zero
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 2.0 - 2.0 ** -9, -0.0, 0.0, -3.0, 2.0 ** -126, RP.BF16_MAX])
    assert RP.bf16_round(x).tolist() == [0x3f80, 0x3f80, 0x3f82, 0x4000, 0x8000, 0x0000, 0xc040, 0x0080, 0x7f7f]
    assert np.array_equal(RP.bf16_value(RP.bf16_round(x)), [1.0, 1.0, 1.0 + 2.0 ** -6, 2.0, -0.0, 0.0, -3.0, 2.0 ** -126, RP.BF16_MAX])
