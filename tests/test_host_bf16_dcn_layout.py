"""bf16 storage with DCNv2 stages / a LayoutHead, the parts that need no device: the model handle accepts the configuration on the
CPU restatement of the C-ABI (csrc/model.cpp compiled against oracle/cpu_abi), which has no bf16 kernels and reports the forward as
unsupported; the Python host builds its bf16 layers."""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import kitti_cfg as kc  # noqa: E402

IVX_ERR_UNSUPPORTED = -3


def _load_cpu_host():
    import importlib.util
    spec = importlib.util.spec_from_file_location('ivx_cpu_abi_host', os.path.join(ROOT, 'oracle', 'cpu_abi', 'host.py'))
    host = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(host)
    return host


def _dcn_model(ia):
    model = ia.build_detector(kc.nuscenes_model_cfg(n_voxels=(16, 16, 12), dcn=True), test_cfg=dict(kc.NUSCENES_TEST_CFG))
    ia.randomize_(model, 31)
    return model


def _total_model(ia):
    cfg = kc.sunrgbd_fast_model_cfg()
    cfg['n_voxels'] = (16, 16, 8)
    cfg['head_2d'] = dict(type='LayoutHead', n_channels=2048, linear_size=32, dropout=0.0)
    torch.manual_seed(1234)
    model = ia.build_detector(cfg, test_cfg=dict(kc.SUNRGBD_FAST_TEST_CFG, nms_pre=60))
    ia.randomize_(model, 5)
    return model


def test_cpu_handle_accepts_bf16_with_dcn_and_reports_forward_unsupported():
    import imvoxelnet_amd as ia
    host = _load_cpu_host()
    model = _dcn_model(ia)
    model.storage_dtype = torch.bfloat16              # what prepare(dtype=torch.bfloat16) records; engine.model_cfg reads it
    cm = host.CpuModel(model)                         # ivx_create + ivx_weights_load + ivx_weights_finalize
    try:
        assert cm.cfg.storage == 1 and list(cm.cfg.dcn_stages) == [0, 0, 1, 1]
        vp = C.c_void_p
        x = np.ascontiguousarray(np.random.default_rng(3).standard_normal((2, 3, 64, 96)).astype(np.float32))
        n = cm.L.ivx_backbone_fpn_workspace_bytes(cm.h, 2, 64, 96)
        raw = np.empty(max(n, 0) + 256, np.uint8)
        ws = raw.ctypes.data + (-raw.ctypes.data % 256)
        fpn0 = np.zeros((2, 1, 16, 24, 64), np.uint16)
        rc = cm.L.ivx_backbone_fpn_fwd(cm.h, x.ctypes.data_as(vp), 2, 64, 96, fpn0.ctypes.data_as(vp), vp(ws), C.c_int64(max(n, 0)), None) if n > 0 else n
        err = cm.L.ivx_last_error().decode()
        print('bf16 DCN forward on the CPU restatement:', rc, err)
        assert rc == IVX_ERR_UNSUPPORTED and 'bf16' in err, (rc, err)
    finally:
        cm.close()


def test_cpu_handle_accepts_bf16_with_layout_head_and_reports_detect_unsupported():
    import imvoxelnet_amd as ia
    host = _load_cpu_host()
    model = _total_model(ia)
    model.storage_dtype = torch.bfloat16
    cm = host.CpuModel(model)
    try:
        assert cm.cfg.storage == 1 and cm.cfg.layout_head == 1 and cm.family == 'indoor'
        hw = (64, 96)
        meta = kc.indoor_meta(1, img_hw=hw, origin=(0, 3, -1))
        img = torch.randn(1, 1, 3, *hw, generator=torch.Generator().manual_seed(8))
        try:
            cm.detect(img, [meta])
        except RuntimeError as e:
            print('bf16 LayoutHead detect on the CPU restatement:', e)
            assert 'bf16' in str(e)
        else:
            raise AssertionError('the CPU restatement has no bf16 kernels: detect must report the mode as unsupported')
    finally:
        cm.close()


def test_prepare_bf16_builds_the_dcn_layers():
    """prepare(dtype=torch.bfloat16) on a DCNv2 backbone (packing only, no kernel launch): conv_offset reads bf16 and writes fp32 offsets /
    masks, the contraction over the columns is a bf16 1x1; the handle's configuration asks for bf16 storage with the DCN stages."""
    import imvoxelnet_amd as ia
    from imvoxelnet_amd import engine
    model = _dcn_model(ia)
    model.prepare(torch.device('cpu'), dtype=torch.bfloat16, native=False)
    for i in (3, 4):
        for blk in getattr(model.backbone, f'layer{i}'):
            assert blk.dcn
            assert (blk.f_off.dtype, blk.f_off.out_dtype) == (torch.bfloat16, torch.float32)
            assert (blk.f2.dtype, blk.f2.out_dtype) == (torch.bfloat16, torch.bfloat16) and blk.f2.cin == 9 * blk.f1.cout
    cfg = engine.model_cfg(model)
    assert cfg.storage == 1 and list(cfg.dcn_stages) == [0, 0, 1, 1]


def test_cpu_handle_refuses_fp8_on_bf16_dcn_and_layout_handles():
    """ivx_model_calibrate_fp8_ex refuses both forms with IVX_ERR_UNSUPPORTED before any device work."""
    import imvoxelnet_amd as ia
    host = _load_cpu_host()
    for model in (_dcn_model(ia), _total_model(ia)):
        model.storage_dtype = torch.bfloat16
        cm = host.CpuModel(model)
        try:
            img = np.zeros((1, 3, 64, 96), np.float32)
            ws = np.zeros(256, np.uint8)
            rc = cm.L.ivx_model_calibrate_fp8_ex(cm.h, img.ctypes.data_as(C.c_void_p), 1, 64, 96, C.c_float(1.0), 2, 1,
                                                 ws.ctypes.data_as(C.c_void_p), C.c_int64(256), None)
            err = cm.L.ivx_last_error().decode()
            assert rc == IVX_ERR_UNSUPPORTED and 'DCNv2' in err, (rc, err)
        finally:
            cm.close()
