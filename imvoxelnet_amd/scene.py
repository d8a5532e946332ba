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

Sliding windows and view removal (open_scene(meta, window=W)).  Subtracting in fp32 is not the inverse of adding, so a view is never
taken out of a running sum: a windowed session keeps no sum at all.  It keeps the FPN level-0 maps of the views that are in the scene
in a ring of W slots and, when the set has changed, lifts that set again in ONE launch straight from the ring, in arrival order
(ops.backproject_gather_mean's kernel, ivx_backproject_gather_fwd: the lift kernel reading its views through a slot list).  The trunk
still runs once per view; the lift is the cheap stage.  The volume is bit for bit the one-shot lift of the kept views' features in
arrival order -- what an unbounded session given only those views holds.  A full window drops its oldest view when a new one arrives
(FIFO); remove_views drops any view by id.  Ring memory is W * FH * FW * C * sizeof(element): at 480 x 640 input (FH x FW = 120 x 160)
ScanNet-fast (C = 256) takes 19.7 MB per slot in fp32, 393 MB at W = 20 (bf16 storage: 9.8 MB, 197 MB); ScanNet-v1 (C = 64) 4.9 MB per
slot, 98 MB at W = 20 (bf16: 2.5 MB, 49 MB).

Out of scope: re-weighting views; batches of scenes in one session (B = 1; open one session per scene, they share the prepared
model); a model-level C handle for sessions (the state lives here, over the op-level ABI and the handle's sub-range calls).
"""
import numpy as np
import torch

from . import ops
from .boxes import bbox3d2result
from .heads import Anchor3DHead


class SceneSession:
    """model.open_scene(meta): meta as one entry of simple_test's img_metas without lidar2img['extrinsic'] -- the extrinsics come with
    the views.  img_shape / ori_shape (/ pad_shape) may be left out when the views come through add_views_u8, which fills them.
    window=None: the scene only grows (a running (sum, count) volume).  window=W >= 1: the scene holds the last W views at most and
    remove_views works; state: a feature ring [W,FH,FW,C] in the storage type and a projection ring [W,3,4] (allocated at the first
    add; W * FH * FW * C * sizeof(element) bytes: the module docstring has the ScanNet figures), the mean / mask buffers and the
    ordered host list of (view id, slot) -- no (sum, count) volume."""

    def __init__(self, model, meta, window=None):
        if window is not None:
            if isinstance(window, bool) or not isinstance(window, (int, np.integer)):
                raise TypeError(f'window must be None or an integer >= 1, got {window!r}')
            if window < 1:
                raise ValueError(f'window must be None or an integer >= 1, got {window}')
            window = int(window)
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
        # window=W: the rings, the views in the scene, oldest first, as (id, slot, extrinsic), and the id of the next arrival
        self._window, self._ring, self._pring, self._views, self._next_id = window, None, None, [], 0

    # ------------------------------------------------------------------ state
    def _check_open(self):
        if self._closed:
            raise RuntimeError('this SceneSession is closed')

    def reset(self):
        """Forget every view; the buffers are kept and the next add starts them from zero."""
        self._check_open()
        self.meta['lidar2img']['extrinsic'] = []
        self._hw, self._origin, self._crop, self._stale, self.n_views = None, None, None, False, 0
        self._views, self._next_id = [], 0

    def close(self):
        self._sum = self._count = self._mean = self._valid = self._origin = self._crop = None
        self._ring = self._pring = None
        self._closed = True

    @property
    def view_ids(self):
        """The ids of the views in the scene, oldest first.  An id is the view's arrival ordinal since reset()."""
        if self._window is None:
            return list(range(self.n_views))
        return [v[0] for v in self._views]

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
        many chunks between two detections.  Views count in the order they are added.  On a windowed session (window=W) the views go
        into free slots of the ring, the oldest views leaving first when the window is full; more than W views in one call raise
        ValueError; emit has no effect (the lift runs when volume() / detect() is asked and the set has changed)."""
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
        if self._window is not None and V > self._window:
            raise ValueError(f'{V} views in one call do not fit a window of {self._window}')
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
        if self._window is not None:
            return self._add_windowed(p0, proj, origin, crop, E, (H, W), shapes)
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

    def _add_windowed(self, p0, proj, origin, crop, E, hw, shapes):
        """The new views' maps p0 [V,1,FH,FW,C] and projection rows proj [1,V,3,4] into free slots of the rings; the oldest views
        leave first when the window is full.  Everything that can fail comes before the first change of the session."""
        m, W, V = self._model, self._window, len(E)
        X, Y, Z = m.n_voxels
        Cn, dev = p0.shape[-1], p0.device
        ring, pring, mean, valid = self._ring, self._pring, self._mean, self._valid
        if ring is None or tuple(ring.shape[1:]) != tuple(p0.shape[1:]) or ring.dtype != p0.dtype:     # first add (or another size after reset())
            ring = torch.empty((W,) + tuple(p0.shape[1:]), device=dev, dtype=p0.dtype)
            pring = torch.empty((W, 3, 4), device=dev, dtype=torch.float32)
            mean = torch.empty((1, X, Y, Z, Cn), device=dev, dtype=p0.dtype)
            valid = torch.empty((1, X, Y, Z), device=dev, dtype=torch.uint8)
        kept = self._views[max(0, len(self._views) + V - W):]
        used = {v[1] for v in kept}
        slots = [s for s in range(W) if s not in used][:V]     # the slots of the views that leave are free for this call's views
        for i, s in enumerate(slots):
            ring[s].copy_(p0[i])
            pring[s].copy_(proj[0, i])
        self._ring, self._pring, self._mean, self._valid = ring, pring, mean, valid
        self._views = kept + [(self._next_id + i, slots[i], E[i]) for i in range(V)]
        self._next_id += V
        self._origin, self._crop, self._hw, self._stale = origin, crop, hw, True
        self.meta.update(shapes)
        self.meta['lidar2img']['extrinsic'] = [v[2] for v in self._views]
        self.n_views = len(self._views)
        return self

    def remove_views(self, ids):
        """Drop the views with these ids (view_ids) from a windowed scene and free their slots; an unknown id raises KeyError and
        leaves the scene as it was."""
        self._check_open()
        if self._window is None:
            raise RuntimeError('remove_views needs a windowed session: open_scene(meta, window=W)')
        ids = [ids] if isinstance(ids, (int, np.integer)) else list(ids)
        have = {v[0] for v in self._views}
        unknown = [i for i in ids if i not in have]
        if unknown:
            raise KeyError(f'no view with id {unknown} in the scene (view_ids: {sorted(have)})')
        drop = set(ids)
        if drop:
            self._views = [v for v in self._views if v[0] not in drop]
            self.meta['lidar2img']['extrinsic'] = [v[2] for v in self._views]
            self.n_views, self._stale = len(self._views), True
        return self

    def add_views_u8(self, frames, extrinsics, img_scale, emit=True, **pipeline_kw):
        """add_views from uint8 camera frames ((H,W,3) BGR arrays / tensors, or one [V,H,W,3]): the test pipeline runs on the device
        (data.prepare_images_device; pipeline_kw: img_norm_cfg, size_divisor, keep_ratio, device) and fills img_shape / ori_shape /
        pad_shape of the scene meta.  Later frames must come out at the same shapes."""
        from .data import prepare_images_device
        self._check_open()
        frames = list(frames)
        E = self._check_extrinsics(extrinsics, len(frames))
        if self._window is not None and len(frames) > self._window:
            raise ValueError(f'{len(frames)} views in one call do not fit a window of {self._window}')
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
        if self._stale and self._window is not None:      # the set changed since the last lift: ONE gathered lift of the views in it, in order
            view_slot = torch.tensor([[v[1] for v in self._views]], dtype=torch.int32).to(self._ring.device)
            ops.backproject_gather_mean_(self._ring, self._pring, view_slot, self._origin, self._crop, self._model.voxel_size, self._mean, self._valid,
                                         getattr(self._model, 'sampling', 'nearest'))
            self._stale = False
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
