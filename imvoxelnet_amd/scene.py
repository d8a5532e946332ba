"""Streaming scenes: add the views of ONE scene to a running volume as they arrive and detect at any time.

simple_test knows "all views at once": a caller who wants detections while scanning re-runs the 2-D trunk on every frame seen so
far, and the trunk is the part of a multi-view step that grows with the number of views.  A SceneSession runs the trunk on the NEW
views only and folds them into a persistent (sum, count) volume (ops.backproject_accum_, csrc/backproject.hip), so an update costs the
trunk of the new frames plus the volume stages.

The view sum continues the stored fp32 sum in view order, so the volume after the last add is bit for bit the one-shot lift of the
same features in the same order (include/imvoxel.h, ivx_backproject_accum_fwd).  The FEATURES of a view may differ in the last bits
from the one-shot run when the trunk's per-tensor operand scales depend on which views share a call (the default fp16-pair trunk).

The session samples the features by its model's rule (prepare(sampling=...)) in every add; the bit identity with the one-shot lift
holds for the bilinear rule as well (one sample function, the same view order).

Out of scope: removing or re-weighting views (sliding windows) -- subtracting in fp32 is not the inverse of adding, the state would
drift away from any one-shot result; batches of scenes in one session (B = 1; open one session per scene, they share the prepared
model); a model-level C handle for sessions (the state lives here, over the op-level ABI and the handle's sub-range calls).
"""
import numpy as np
import torch

from . import ops
from .boxes import bbox3d2result
from .heads import Anchor3DHead


class SceneSession:
    """model.open_scene(meta): meta as one entry of simple_test's img_metas without lidar2img['extrinsic'] -- the extrinsics come with
    the views.  img_shape / ori_shape (/ pad_shape) may be left out when the views come through add_views_u8, which fills them."""

    def __init__(self, model, meta):
        if getattr(model, 'head_2d', None) is not None:
            raise NotImplementedError('a model with a head_2d (SUN RGB-D Total) predicts its extrinsics from the image: there is no running '
                                      'volume to add views to')
        meta = dict(meta)
        try:
            l2i = dict(meta['lidar2img'])
            K, origin = np.asarray(l2i['intrinsic']), l2i['origin']
        except (KeyError, TypeError):
            raise ValueError("the scene meta needs lidar2img = dict(intrinsic=K, origin=o)") from None
        if K.dtype != np.float32:
            raise TypeError('lidar2img intrinsic must be float32 (as the reference datasets produce)')
        if K.ndim != 2 or K.shape[0] < 3 or K.shape[1] < 3:
            raise ValueError(f'lidar2img intrinsic must be at least 3x3, got {K.shape}')
        l2i['extrinsic'] = []                     # grows with the views: `meta` stays a complete simple_test meta of everything added
        meta['lidar2img'] = l2i
        self._model, self.meta = model, meta
        self._sum = self._count = self._mean = self._valid = self._origin = self._crop = None
        self._hw, self._stale, self._closed, self.n_views = None, False, False, 0

    # ------------------------------------------------------------------ state
    def _check_open(self):
        if self._closed:
            raise RuntimeError('this SceneSession is closed')

    def reset(self):
        """Forget every view; the buffers are kept and the next add starts them from zero."""
        self._check_open()
        self.meta['lidar2img']['extrinsic'] = []
        self._hw, self._origin, self._crop, self._stale, self.n_views = None, None, None, False, 0

    def close(self):
        self._sum = self._count = self._mean = self._valid = self._origin = self._crop = None
        self._closed = True

    # ------------------------------------------------------------------ adding views
    def _features(self, img):
        """[V,3,H,W] -> FPN level 0 of these views.  The native handle's trunk sub-range is the same kernels with the same plans as
        features_2d_cl in one C call (equal bit for bit: tests/test_gpu_engine.py)."""
        m = self._model
        nat = m._native
        if nat is not None and nat.cfg.with_trunk and img.shape[-2] % 32 == 0 and img.shape[-1] % 32 == 0:
            return nat.backbone_fpn(img)
        return m.features_2d_cl(img[None])

    @staticmethod
    def _check_extrinsics(extrinsics, V):
        E = [np.asarray(e) for e in extrinsics]
        if len(E) != V:
            raise ValueError(f'{len(E)} extrinsics for {V} views')
        for e in E:
            if e.dtype != np.float32:
                raise TypeError(f'extrinsics must be float32 (as the reference datasets produce), got {e.dtype}')
            if e.shape != (4, 4):
                raise ValueError(f'every extrinsic must be 4x4, got {e.shape}')
        return E

    def add_views(self, img, extrinsics, emit=True):
        """img [V,3,H,W] float32 on the device (normalised and padded as for simple_test), extrinsics: V float32 4x4 matrices.
        emit=False skips the store of the mean volume (detect() / volume() then compute it once from the sums): for callers that add
        many chunks between two detections.  Views count in the order they are added."""
        return self._add_views(img, extrinsics, emit, {})

    def _add_views(self, img, extrinsics, emit, shapes):
        """add_views with the img_shape / ori_shape / pad_shape of these views (add_views_u8); the session changes only when the
        views are in: a call that raises leaves meta, state and n_views as they were."""
        self._check_open()
        if not isinstance(img, torch.Tensor):
            raise TypeError('img must be a torch.Tensor [V,3,H,W]')
        if img.dim() != 4 or img.shape[0] < 1 or img.shape[1] != 3:
            raise ValueError(f'img must be [V,3,H,W] with V >= 1, got {tuple(img.shape)}')
        if img.dtype != torch.float32:
            raise TypeError(f'img must be float32, got {img.dtype}')
        V, H, W = int(img.shape[0]), int(img.shape[2]), int(img.shape[3])
        E = self._check_extrinsics(extrinsics, V)
        if self._hw is not None and (H, W) != self._hw:
            raise ValueError(f'image size {(H, W)} differs from the {self._hw} of the views already in the scene')
        meta = dict(self.meta, **shapes)
        if 'img_shape' not in meta or 'ori_shape' not in meta:
            raise ValueError('the scene meta needs img_shape and ori_shape (add_views_u8 fills them from its frames)')
        if not img.is_cuda:
            raise RuntimeError('img must be a device (HIP) tensor; the MI355X path has no CPU fallback')
        m = self._model
        if m._prepared_device is None:
            m.prepare(img.device)
        p0 = self._features(img.contiguous())
        view_meta = dict(meta, lidar2img=dict(meta['lidar2img'], extrinsic=E))
        if self._origin is None:                  # new_origin and the crop do not depend on the views: uploaded once per scene
            proj, origin, crop = m._camera_setup([view_meta], 4, p0.device)
        else:
            proj, origin, crop = m._compute_projection(view_meta, 4)[None].contiguous().to(p0.device), self._origin, self._crop
        if self._sum is None:                     # the state, allocated once: sum fp32, count, mean in the storage type, valid
            X, Y, Z = m.n_voxels
            Cn, dev = p0.shape[-1], p0.device
            self._sum = torch.empty((1, X, Y, Z, Cn), device=dev, dtype=torch.float32)
            self._count = torch.empty((1, X, Y, Z), device=dev, dtype=torch.int32)
            self._mean = torch.empty((1, X, Y, Z, Cn), device=dev, dtype=p0.dtype)
            self._valid = torch.empty((1, X, Y, Z), device=dev, dtype=torch.uint8)
        ops.backproject_accum_(p0, proj, origin, crop, m.voxel_size, self._sum, self._count, self.n_views == 0,
                               self._mean if emit else None, self._valid if emit else None, sampling=getattr(m, 'sampling', 'nearest'))
        self._origin, self._crop = origin, crop
        self._stale = not emit
        self._hw = (H, W)
        self.meta.update(shapes)
        self.meta['lidar2img']['extrinsic'] = self.meta['lidar2img']['extrinsic'] + E
        self.n_views += V
        return self

    def add_views_u8(self, frames, extrinsics, img_scale, emit=True, **pipeline_kw):
        """add_views from uint8 camera frames ((H,W,3) BGR arrays / tensors, or one [V,H,W,3]): the test pipeline runs on the device
        (data.prepare_images_device; pipeline_kw: img_norm_cfg, size_divisor, keep_ratio, device) and fills img_shape / ori_shape /
        pad_shape of the scene meta.  Later frames must come out at the same shapes."""
        from .data import prepare_images_device
        self._check_open()
        frames = list(frames)
        E = self._check_extrinsics(extrinsics, len(frames))
        img, shapes = prepare_images_device([frames], img_scale, **pipeline_kw)       # one multi-view sample
        for k, v in shapes[0].items():
            if self.n_views and k in self.meta and tuple(self.meta[k]) != tuple(v):
                raise ValueError(f'{k} {tuple(v)} of these frames differs from the {tuple(self.meta[k])} of the views already in the scene')
        return self._add_views(img[0], E, emit, shapes[0])

    # ------------------------------------------------------------------ reading the scene
    def volume(self):
        """(mean volume [1,X,Y,Z,C] channels-last, valid bool [1,X,Y,Z]) of the views so far: the session's own buffers, rewritten by
        the next add (clone what must outlive it)."""
        self._check_open()
        if self.n_views == 0:
            raise RuntimeError('the scene has no views yet')
        if self._stale:
            ops.volume_mean(self._sum, self._count, self._mean.dtype, out=self._mean, valid_out=self._valid)
            self._stale = False
        return self._mean, self._valid.view(torch.bool)

    def detect(self):
        """Detections from the views so far: [dict(boxes_3d, scores_3d, labels_3d)] as simple_test returns for one sample."""
        vol, valid = self.volume()
        m, metas = self._model, [self.meta]
        if isinstance(m.bbox_head, Anchor3DHead):
            boxes, scores, labels, count = m.detect_cl(vol, metas)
            return m._results_one_copy(boxes, scores, labels, count, metas)
        return [bbox3d2result(b, s, l) for b, s, l in m.detect_indoor_cl(vol, valid, metas)]
