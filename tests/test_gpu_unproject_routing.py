"""-m gpu: which kernel a lift call runs, where nothing else pins it (csrc/backproject.hip, the selection table of bp_launch; DESIGN.md
"Which lift kernel runs").  The nearest fp32 mean of ONE view must be the copy kernel -- bit for bit, and the only lift that writes per-workgroup maxima --
and a bf16 view sum must start from a zero state.  The dyadic scene of tests/ref_unproject.py, B = 2; every output buffer is pre-filled
with NaN / garbage, so an unwritten element fails."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ref_unproject as R

pytestmark = pytest.mark.gpu

GARBAGE = 0x7f7f7f7f
MEAN, SUM = 0, 1
NEAREST = 0
NV = R.N_VOXELS
# words a copy keeps and arithmetic does not: -0.0, the smallest denormal, +/-Inf, a quiet NaN with a payload, a signalling NaN
SPECIAL32 = np.array([0x80000000, 0x00000001, 0x7f800000, 0xff800000, 0x7fc12345, 0x7f812345], np.uint32).view(np.int32)
SPECIAL16 = np.array([0x8000, 0x0001, 0x7f80, 0xff80, 0x7fc1, 0x7f81], np.uint16).view(np.int16)
NEG0 = int(SPECIAL32[0])


@pytest.fixture(scope='module')
def L():
    from imvoxelnet_amd import _lib
    lib = _lib.lib()
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    return lib


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _older(L, name, feat, P, no, crop, *outs, nv=NV):
    """One raw call of an older export (feat, dims, proj, new_origin, crop_hw, voxel_size, grid, outputs..., stream); returns the status."""
    i32 = C.c_int32
    B, V = P.shape[0], P.shape[1]
    _, _, FH, FW, Cn = feat.shape
    return getattr(L, name)(_p(feat), i32(B), i32(V), i32(FH), i32(FW), i32(Cn), _p(P), _p(no), _p(crop), (C.c_float * 3)(*R.VOXEL_SIZE),
                            i32(nv[0]), i32(nv[1]), i32(nv[2]), *[_p(o) for o in outs], _stream())


def _ex(L, feat, P, no, crop, mode, volume, count=None, valid=None):
    """One raw ivx_backproject_fwd_ex call with the NEAREST rule; returns the status."""
    from imvoxelnet_amd import _lib
    B, V = P.shape[0], P.shape[1]
    _, _, FH, FW, Cn = feat.shape
    d = _lib.BackprojectDesc(B, V, FH, FW, Cn, NV[0], NV[1], NV[2], (C.c_float * 3)(*R.VOXEL_SIZE), 1 if feat.dtype == torch.bfloat16 else 0, mode, NEAREST, 0)
    return L.ivx_backproject_fwd_ex(C.byref(d), _p(feat), _p(P), _p(no), _p(crop), _p(volume), _p(count), None, _p(valid), _stream())


def _bufs(B, Cn, dtype=torch.float32, nv=NV):
    return (torch.full((B,) + tuple(nv) + (Cn,), float('nan'), device='cuda', dtype=dtype), torch.full((B,) + tuple(nv), 7, device='cuda', dtype=torch.uint8),
            torch.full((B,) + tuple(nv), GARBAGE, device='cuda', dtype=torch.int32))


@functools.lru_cache(maxsize=None)
def _scenes():
    return R.dyadic_scene(R.NEW_ORIGIN, R.CROP), R.dyadic_scene(R.NEW_ORIGIN_2, R.CROP_2)


@functools.lru_cache(maxsize=None)
def _geometry(views=(0, 1, 2)):
    s0, s1 = _scenes()
    v = list(views)
    P = torch.from_numpy(np.stack([s0['proj'][v], s1['proj'][v]])).cuda().contiguous()
    no = torch.from_numpy(np.stack([s0['new_origin'], s1['new_origin']])).cuda().contiguous()
    crop = torch.from_numpy(np.stack([s0['crop'], s1['crop']])).cuda().contiguous()
    return P, no, crop


def _special_words(Cn, special, seed):
    """[2, FH, FW, Cn] words: random normal numbers' bits with every 7th word one of the special ones, in turn."""
    rng = np.random.default_rng(seed)
    if special.dtype == np.int32:
        w = rng.standard_normal((2, R.FH, R.FW, Cn)).astype(np.float32).view(np.int32).copy()
    else:
        w = (rng.standard_normal((2, R.FH, R.FW, Cn)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16).view(np.int16).copy()
    flat = w.reshape(-1)
    flat[::7] = np.resize(special, len(flat[::7]))
    return w


def _copied_words(words, view):
    """What a one-view nearest lift is by definition: voxel n of sample b holds the words of pixel (rint(yf), rint(xf)) of that sample's map where
    the view sees it (the rule of ref_unproject.valid_views), +0 elsewhere.  words [2, FH, FW, Cw] -> ([2, N, Cw], seen [2, N])."""
    out, seen = [], []
    for b, sc in enumerate(_scenes()):
        xf, yf, d = sc['xf'][view], sc['yf'][view], sc['d'][view]
        ok = R.valid_views(xf, yf, d, sc['hc'], sc['wc'])
        e = np.zeros((xf.shape[0], words.shape[-1]), words.dtype)
        e[ok] = words[b, np.rint(yf[ok]).astype(np.int64), np.rint(xf[ok]).astype(np.int64)]
        out.append(e)
        seen.append(ok)
    return np.stack(out), np.stack(seen)


@pytest.mark.parametrize('Cn', [8, 6])
def test_one_fp32_view_is_copied_bit_for_bit_by_both_entry_points(L, Cn):
    """V = 1, fp32, nearest; C = 8: float4 chunks, C = 6: the scalar form.  Through ivx_backproject_mean_fwd and through ivx_backproject_fwd_ex
    (NEAREST) every seen voxel's words are the source pixel's words (int32 compare: -0.0, a denormal, +/-Inf, NaNs with payloads survive),
    an unseen voxel is +0, and the mask is the validity rule's."""
    words = _special_words(Cn, SPECIAL32, 11 + Cn)
    for view in (0, 1):
        want, seen = _copied_words(words, view)
        assert all((want[seen] == s).any() for s in SPECIAL32), 'a special word never reaches a seen voxel: the test would not tell a copy from a sum'
        feat = torch.from_numpy(words).view(torch.float32).reshape(2, 1, R.FH, R.FW, Cn).cuda()
        P, no, crop = _geometry((view,))
        for how in ('ivx_backproject_mean_fwd', 'ivx_backproject_fwd_ex'):
            vol, valid, _ = _bufs(2, Cn)
            rc = _older(L, how, feat, P, no, crop, vol, valid) if how != 'ivx_backproject_fwd_ex' else _ex(L, feat, P, no, crop, MEAN, vol, valid=valid)
            assert rc == 0, (how, L.ivx_last_error())
            got = vol.view(torch.int32).cpu().numpy().reshape(want.shape)
            assert np.array_equal(got, want), (how, view, int((got != want).sum()))
            assert np.array_equal(valid.cpu().numpy().reshape(seen.shape), seen.astype(np.uint8)), (how, view)


def test_one_bf16_view_goes_as_words_through_the_copy(L):
    """ops.backproject_mean with a bf16 map, one view, C = 8: passed as C/2 32-bit words to ivx_backproject_mean_fwd, so every bf16 word survives
    (the bf16 mean kernel would turn -0.0 into +0)."""
    from imvoxelnet_amd import ops
    words = _special_words(8, SPECIAL16, 23)
    want, seen = _copied_words(words, 0)
    assert all((want[seen] == s).any() for s in SPECIAL16)
    feat = torch.from_numpy(words).view(torch.bfloat16).reshape(2, 1, R.FH, R.FW, 8).cuda()
    P, no, crop = _geometry((0,))
    vol, valid = ops.backproject_mean(feat, P, no, crop, R.VOXEL_SIZE, NV)
    assert vol.dtype == torch.bfloat16 and tuple(vol.shape) == (2,) + NV + (8,)
    assert np.array_equal(vol.view(torch.int16).cpu().numpy().reshape(want.shape), want)
    assert np.array_equal(valid.cpu().numpy().reshape(seen.shape), seen)


def test_two_equal_views_run_the_mean_kernel_which_adds(L):
    """The same view twice (V = 2) takes backproject_mean_kernel: its sum starts from +0, so a -0.0 feature comes out as +0.0 -- today's
    behaviour, and the proof that the bit tests above tell the copy kernel from the mean kernel."""
    words = _special_words(8, SPECIAL32, 19)
    want, seen = _copied_words(words, 0)
    neg0 = seen[:, :, None] & (want == NEG0)
    assert neg0.sum() > 0
    feat = torch.from_numpy(words).view(torch.float32).reshape(2, 1, R.FH, R.FW, 8).cuda()
    feat2 = torch.stack([feat, feat], 1).reshape(4, 1, R.FH, R.FW, 8).contiguous()
    P, no, crop = _geometry((0, 0))
    vol, valid, _ = _bufs(2, 8)
    assert _older(L, 'ivx_backproject_mean_fwd', feat2, P, no, crop, vol, valid) == 0, L.ivx_last_error()
    got = vol.view(torch.int32).cpu().numpy().reshape(want.shape)
    assert np.all(got[neg0] == 0), 'a -0.0 survived two views: this is not the mean kernel'
    normal = seen[:, :, None] & np.isfinite(want.view(np.float32)) & (np.abs(want.view(np.float32)) > 1e-30)
    assert normal.sum() > 0 and np.array_equal(got[normal], want[normal]) and np.array_equal(valid.cpu().numpy().reshape(seen.shape), seen.astype(np.uint8))


def _amax(L, feat, P, no, crop, vol, valid, partials, nv):
    i32 = C.c_int32
    B, V = P.shape[0], P.shape[1]
    _, _, FH, FW, Cn = feat.shape
    return L.ivx_backproject_mean_fwd_amax(_p(feat), i32(B), i32(V), i32(FH), i32(FW), i32(Cn), _p(P), _p(no), _p(crop), (C.c_float * 3)(*R.VOXEL_SIZE),
                                           i32(nv[0]), i32(nv[1]), i32(nv[2]), _p(vol), _p(valid), _p(partials), _stream())


@pytest.mark.parametrize('Cn,nv', [(8, NV), (6, NV), (8, (9, 8, 7)), (6, (9, 8, 7))], ids=['C8', 'C6', 'C8-2blocks', 'C6-2blocks'])
def test_single_view_maxima(L, Cn, nv):
    """ivx_backproject_mean_fwd_amax, V = 1: every one of the ivx_backproject_amax_blocks floats is written, entry b * gridX + i is the
    max |volume| over voxels [256 i, 256 i + 256) of sample b (exact: a max rounds nothing), and volume / mask are ivx_backproject_mean_fwd's.
    The scene's own grid is one workgroup per sample; 9 x 8 x 7 = 504 voxels are two, the second one partly filled."""
    g = torch.Generator().manual_seed(40 + Cn)
    feat = torch.randn(2, 1, R.FH, R.FW, Cn, generator=g).cuda()
    P, no, crop = _geometry((0,))
    n = nv[0] * nv[1] * nv[2]
    gx = (n + 255) // 256
    nblk = L.ivx_backproject_amax_blocks(C.c_int32(2), C.c_int32(1), C.c_int32(nv[0]), C.c_int32(nv[1]), C.c_int32(nv[2]))
    assert nblk == 2 * gx and L.ivx_backproject_amax_blocks(C.c_int32(2), C.c_int32(3), C.c_int32(nv[0]), C.c_int32(nv[1]), C.c_int32(nv[2])) == 0
    part = torch.full((nblk,), float('nan'), device='cuda')
    vol, valid, _ = _bufs(2, Cn, nv=nv)
    assert _amax(L, feat, P, no, crop, vol, valid, part, nv) == 0, L.ivx_last_error()
    ref_vol, ref_valid, _ = _bufs(2, Cn, nv=nv)
    assert _older(L, 'ivx_backproject_mean_fwd', feat, P, no, crop, ref_vol, ref_valid, nv=nv) == 0, L.ivx_last_error()
    assert torch.equal(vol.view(torch.int32), ref_vol.view(torch.int32)) and torch.equal(valid, ref_valid) and int(valid.sum()) > 0
    a = torch.zeros(2, gx * 256, device='cuda')
    a[:, :n] = vol.abs().reshape(2, n, Cn).amax(-1)
    want = a.reshape(2, gx, 256).amax(-1).reshape(-1)
    assert not bool(torch.isnan(part).any()), 'a workgroup did not write its maximum'
    assert torch.equal(part, want) and float(want.min()) > 0


@pytest.mark.parametrize('Cn', [8, 6])
def test_amax_entry_without_partials_is_the_plain_mean(L, Cn):
    """partials = NULL and V = 3: ivx_backproject_mean_fwd_amax is ivx_backproject_mean_fwd (the multi-view kernel, no maxima)."""
    g = torch.Generator().manual_seed(50 + Cn)
    feat = torch.randn(6, 1, R.FH, R.FW, Cn, generator=g).cuda()
    P, no, crop = _geometry()
    vol, valid, _ = _bufs(2, Cn)
    ref_vol, ref_valid, _ = _bufs(2, Cn)
    assert _amax(L, feat, P, no, crop, vol, valid, None, NV) == 0, L.ivx_last_error()
    assert _older(L, 'ivx_backproject_mean_fwd', feat, P, no, crop, ref_vol, ref_valid) == 0, L.ivx_last_error()
    assert not bool(torch.isnan(vol).any()) and torch.equal(vol, ref_vol) and torch.equal(valid, ref_valid) and 0 < int(valid.sum()) < valid.numel()


def test_bf16_sum_starts_from_a_zero_state(L):
    """ivx_backproject_fwd_ex, SUM, bf16 features, NEAREST runs the accumulate kernel, which must not read its state: over NaN / garbage the
    result is ops.backproject_accum_(first=True)'s on the same inputs (torch.equal), and the count is the fp32 ops.backproject_sum's."""
    from imvoxelnet_amd import ops
    g = torch.Generator().manual_seed(61)
    feat = torch.randn(6, 1, R.FH, R.FW, 8, generator=g).bfloat16().cuda()
    P, no, crop = _geometry()
    vol, _, count = _bufs(2, 8)
    assert _ex(L, feat, P, no, crop, SUM, vol, count=count) == 0, L.ivx_last_error()
    ref_vol, _, ref_count = _bufs(2, 8)
    ops.backproject_accum_(feat, P, no, crop, R.VOXEL_SIZE, ref_vol, ref_count, True)
    assert not bool(torch.isnan(vol).any()) and torch.equal(vol, ref_vol) and torch.equal(count, ref_count)
    _, cnt32 = ops.backproject_sum(feat.float(), P, no, crop, R.VOXEL_SIZE, NV)
    assert torch.equal(count, cnt32) and int(count.max()) == 3 and int(count.min()) == 0
