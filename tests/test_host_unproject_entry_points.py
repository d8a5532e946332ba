"""The older lift exports without a device: ivx_backproject_mean_fwd, _mean_fwd_amax, _mean_fwd_bf16 and _sum_fwd reject every bad
argument with IVX_ERR_INVALID_ARG and a message that names the export the caller called, before any launch (csrc/backproject.hip
bp_validate, the one validator of every lift).  The dummy pointers are never dereferenced: every call here is one that must be refused.
(ivx_backproject_accum_fwd*, _fwd_ex and _gather_fwd have the same tests in test_host_scene_stream.py, test_host_unproject_bilinear.py and
test_host_scene_window.py.)"""
import ctypes as C

import pytest

NAMES = ('ivx_backproject_mean_fwd', 'ivx_backproject_mean_fwd_amax', 'ivx_backproject_mean_fwd_bf16', 'ivx_backproject_sum_fwd')
P = C.c_void_p(64)
DIMS = dict(B=1, V=2, FH=6, FW=8, C=8, X=4, Y=4, Z=2)


def _caller(name):
    from imvoxelnet_amd import _lib
    L = _lib.lib()
    fn = getattr(L, name)
    i32 = C.c_int32

    def call(feat=P, proj=P, origin=P, crop=P, vs=True, vol=P, out=P, partials=None, **dims):
        """out: valid of the mean forms, count of the sum form; partials: ivx_backproject_mean_fwd_amax only."""
        d = dict(DIMS, **dims)
        tail = (vol, out, partials, None) if name.endswith('_amax') else (vol, out, None)
        return fn(feat, i32(d['B']), i32(d['V']), i32(d['FH']), i32(d['FW']), i32(d['C']), proj, origin, crop, (C.c_float * 3)(.5, .5, .5) if vs else None,
                  i32(d['X']), i32(d['Y']), i32(d['Z']), *tail)

    def refused(fragment, **kw):
        rc, err = call(**kw), L.ivx_last_error()
        assert rc == -1 and fragment in err and name.encode() + b':' in err, (name, kw, rc, err)

    return refused


@pytest.mark.parametrize('name', NAMES)
def test_older_exports_validate_without_gpu(name):
    refused = _caller(name)
    for ptr in ('feat', 'proj', 'origin', 'crop', 'vs', 'vol', 'out'):
        refused(b'null', **{ptr: None})
    for dim in DIMS:
        for bad in (0, -1):
            refused(b'non-positive', **{dim: bad})
    refused(b'voxel grid too large', X=2048, Y=2048, Z=512)                      # X*Y*Z = 2^31
    refused(b'feature maps too large', B=4, V=32, FH=4096, FW=4096)              # B*V*FH*FW = 2^31
    refused(b'batch too large', B=65536, V=1, FH=1, FW=1, X=1, Y=1, Z=1)
    refused(b'too large (max 1024)', C=1028)                                     # 257 float4 chunks


@pytest.mark.parametrize('name', ('ivx_backproject_sum_fwd', 'ivx_backproject_mean_fwd_bf16'))
def test_sum_and_bf16_mean_need_float4_channels(name):
    refused = _caller(name)
    for Cn in (6, 1, 1026):
        refused(b'C % 4', C=Cn)


@pytest.mark.parametrize('name', ('ivx_backproject_mean_fwd', 'ivx_backproject_mean_fwd_amax'))
def test_fp32_mean_takes_scalar_channels_up_to_256(name):
    """C % 4 != 0 is the fp32 mean's VEC 1 form: what is refused is only more than 256 of them, as too large and not as C % 4 (that C = 6 runs is
    the GPU suite's test_one_fp32_view_is_copied_bit_for_bit_by_both_entry_points)."""
    refused = _caller(name)
    for Cn in (257, 1026):
        refused(b'too large (max 256)', C=Cn)


def test_partial_maxima_need_a_single_view():
    refused = _caller('ivx_backproject_mean_fwd_amax')
    for V in (2, 3):
        refused(b'single-view', V=V, partials=P)
