"""Streaming scenes: add the views of a scene (SceneSession) or of N scenes at once (SceneBatch) to running volumes as they arrive and
detect at any time.

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

Batches of scenes (model.open_scenes(metas, window=None) -> SceneBatch).  A server that follows several scans at once would otherwise run
a 1-view trunk call, a B = 1 lift, a B = 1 neck and a B = 1 tail per scene and tick.  A SceneBatch keeps the state of N scenes in pools
of N rows and shares the launches: one trunk call over all the new views of a tick, ONE listed lift that adds them to the touched
scenes (ops.backproject_lists_accum_, ivx_backproject_lists_fwd: ragged slot lists, a row and a `first` flag per scene), one batched
neck + head + NMS in detect().  State per scene: X*Y*Z * (C * (4 + sizeof(element)) + 5) bytes -- ScanNet-fast (40 x 40 x 16, C = 256)
52.6 MB in fp32 (39.5 MB with bf16 storage), ScanNet-v1 (80 x 80 x 32, C = 64) 105.9 MB (79.7 MB); a windowed batch keeps the mean / mask
pools and N rings instead of the sums.  The volume of every scene is exact (the one-shot lift of the features it was given, bit for
bit); the features and the batched neck depend on what shares a call, so boxes are not claimed equal to a single session's: the
SceneBatch docstring states each claim.  SceneSession is not built on the batch: its path and bits are what they were.

Fading scenes (open_scene(meta, decay=lam, forget_below=t) / open_scenes(metas, decay=...)).  The two ways above never forget, or forget exactly
at the price of a ring of W maps, and both weigh a blurred or badly posed frame like a good one.  A session opened with `decay` keeps the usual
weighted running mean of a fusing volume instead: every view carries a weight (add_views(..., weights=...), 1 by default), every add_views call is
one tick -- the state (sum, weight sum) fades by `decay` once, then the call's views are added with their weights -- and a voxel whose faded weight
sum falls below `forget_below` becomes unseen again.  State: the (sum, count) volume plus one fp32 weight sum per voxel; no ring.  The lift is
ops.backproject_weighted_accum_ (ivx_backproject_weighted_fwd; include/imvoxel.h has the definition); with decay=1.0 and unit weights the session
holds, tick by tick, the bits of a plain session.  A windowed scene takes weights too (a weight per kept view, reweight(ids, weights) changes
them): its re-lift is then the weighted mean of the kept views (ops.backproject_weighted_mean_).  `decay` and `window` are alternative ways to
forget and exclude each other.

Scrolling scenes (SceneSession.scroll(voxels) / scroll_to(center), SceneBatch.scroll(scenes, voxels)).  Forgetting what lies behind a moving
platform is half of following it; the other half is carrying the grid along, or every new view of a robot that has left the 6.4 m ScanNet grid
sees no voxel.  scroll moves the grid by whole voxels: the state (sum, count, weight sum) of a plain or fading scene is shifted in place by
ops.volume_scroll_ (ivx_volume_scroll_fwd, csrc/volume_scroll.hip: a pure move of bits, voxels that enter are unseen), a windowed scene has
nothing to move and lifts its kept views again, and the meta's origin follows ONE rule, scrolled_origin = float32(origin) + float32(voxels) *
float32(voxel_size), from which the device new_origin is recomputed by the model's own rule.  Everything after a scroll is the existing lift at
the new origin, so a scrolled scene is, bit for bit, a scene opened at the new origin whose state is the moved state.  A scroll is not a tick:
nothing fades.  Like bilinear sampling and fading it is an extra outside the reference-parity claims; a session that never scrolls runs the code
it ran before.  Models with an Anchor3DHead refuse: their anchors are fixed in the LiDAR frame.

Warping scenes (SceneSession.warp(T) / SceneBatch.warp(scenes, Ts); warped_extrinsic, frame).  scroll carries the grid along by whole voxels and
moves the origin, which excludes the platforms that move most: a vehicle whose grid and anchors live in the vehicle frame needs the previous state
in the CURRENT vehicle frame on every tick -- a rotation plus a fractional translation -- and a robot with a robot-aligned grid cannot turn.  warp is
the one operation both need: T is a host 4x4 with x_old = T x_new (inv(world_from_old_ego) @ world_from_new_ego), the grid stays where the head
expects it (origin, anchors and head code are untouched, so Anchor3DHead models warp like any other), and the state is resampled under T.  A fading
scene already keeps the right state: a float weight sum resamples linearly beside the sums, both with the same trilinear weights, so the mean stays
a convex combination of neighbouring means and evidence thins at the grid's border and at the edge of what was seen (ops.volume_warp,
ivx_volume_warp_fwd, csrc/volume_warp.hip; include/imvoxel.h has the definition; out of place, into a twin state that a session keeps from its
first warp on -- twice the state memory -- and a batch allocates per call for the rows it moves).  A windowed scene needs no kernel: it re-poses its
kept views and lifts them again, which is exact.  Every extrinsic a scene holds follows ONE rule, warped_extrinsic(E, T) = float32(float64(E) @
float64(T)), so `meta` stays a complete simple_test meta in the new frame; after a warp the caller's extrinsics and the returned boxes are in the
grid's current frame, and `frame` (float64 4x4, the product of every T since open or reset()) takes a point of the current frame back to the
opening one: x_opening = frame @ x_grid.  A warp is not a tick: nothing fades, but the session's forget_below applies to the thinned weight sums.
A plain scene raises NotImplementedError -- integer view counts cannot be resampled; decay=1.0 fades nothing and can.  The identity launches
nothing; a session that never warps runs the code it ran before.  scroll keeps its behaviour, its refusal for anchor heads included.

Merging scenes (SceneSession.merge(other, T=None, weight=1.0) / SceneBatch.merge(scenes, sources, Ts=None, weights=None)).  Every operation above acts
on one scene; two scenes could not become one except by pushing every frame through the trunk again.  But a fading scene's (sum, weight sum, count)
state is linear: two such states named in one frame add.  merge adds the other scene's state to this one's under a rigid T with x_other = T x_self
(None: the two were opened in one common frame, T = inv(other.frame) @ self.frame) -- two robots or two passes that fused the same rooms, a
relocalisation against a map built earlier, two rows of a batch that turn out to be one flat.  One launch (ops.volume_merge_, ivx_volume_merge_fwd,
the MERGE instantiation of the resample kernel of csrc/volume_warp.hip; include/imvoxel.h has the definition) reads the other state by the warp's
trilinear rule, in the OTHER grid -- the two grids keep their own origins, so a scrolled scene merges -- and adds it in place, scaled by `weight`, at
the voxels where the other scene holds evidence; no other voxel is written, no scratch row exists, and this scene's forget_below applies to what was
merged.  The host record follows the warp's rule: the other's extrinsics arrive as warped_extrinsic(E, T) behind this scene's own, n_views adds, the
mean is recomputed when next asked for, and frame, origin and scrolled stay.  A merge is not a tick: nothing fades.  The other scene is unchanged.
Evidence both scenes hold of the same views counts twice.  A batch merges rows of its own pools, all pairs of a call in one launch.  Plain and
windowed scenes refuse.  A scene that never merges runs the code it ran before.

Matching scenes (SceneSession.match(other, Ts=None, step=1, min_overlap=0.3) / register(other, T0=None, yaw, shift, levels, step, min_overlap);
SceneBatch.match(scenes, sources, Ts) / register(scene, source, ...); pose_candidates; MatchResult).  scroll, warp, merge and restore all take the
transform between two frames as given, and a pose that is off by a voxel smears a merge without a warning.  But the state holds what judges a pose:
two fading states are per-voxel mean feature vectors with weights, and for a candidate T (x_other = T x_self, the merge's convention) the
correlation of the two means over the voxels both scenes have seen says how well they agree.  match scores K candidates in one call
(ops.volume_match, ivx_volume_match_fwd, csrc/volume_match.hip; include/imvoxel.h has the definition): the other state is read by the merge's
trilinear rule, each grid with its own origin, nothing is written, and per candidate come back pairs (voxels both hold evidence for), own, and the
fp64 sums (dot, na, nb) of the means' products -- deterministic, with no atomics, so a batch's answer equals a session's bit for bit.  The host
forms ncc = dot / sqrt(na * nb) and overlap = pairs / own; a candidate below min_overlap is not eligible.  register is a thin LOCAL search on top:
per level the 81 candidates of pose_candidates around the current pose (yaw and three shifts, each offset in {-h, 0, +h}, about the grid's
centre), move to the best eligible one, halve the offsets.  Plain and windowed scenes refuse, as for merge.  A scene that never matches runs the
code it ran before.

Aligning scenes (SceneSession.refine(other, T0=None, iters=12, dof, step, min_overlap, damping, tol_shift, tol_rot) / SceneBatch.refine(scenes,
sources, T0s); register(..., refine=True); rigid_increment; solve_align; AlignResult).  register scores 486 candidates for six levels, resolves the
pose to its last lattice step and searches yaw and translation only; a hand-held camera, a robot on a ramp and a vehicle that pitches under braking
need pitch and roll too.  The state already holds what a direct method needs: the mean field b(x) = S(x) / W(x) is read trilinearly, so its spatial
gradient comes from the same eight corners the match loads.  One evaluation (ops.volume_align, ivx_volume_align_fwd, the ALIGN instantiation of the
match kernel in csrc/volume_match.hip; include/imvoxel.h has the definition) returns, beside the match's own numbers bit for bit, the cost
e = sum |b - a|^2 over the USED voxels (paired, all eight corners of the read inside the other grid and seen), g = sum J r and H = sum J J^T for the
six degrees of freedom (three translations, three rotation-vector components about the grid's centre) as 31 fp64 sums -- deterministic, no atomics,
so a batch's answer equals a session's bit for bit.  The host solves (H + damping diag H) delta = -g (solve_align), tries
T @ rigid_increment(delta, about) and keeps it iff it is eligible (used > 0, used / own >= min_overlap) and its cost e / (used * C) is strictly
lower: Levenberg-Marquardt with one stated rule (_refine), 31 doubles read back per evaluation.  refine is LOCAL: the gradient is that of a
trilinear read, so its basin is about a voxel and a few degrees on real features -- run register with coarse levels first, then refine, or
register(..., refine=True), which refines the degrees the lattice searched unless told otherwise.  A scene that never refines runs the code it ran
before.

Scene snapshots (SceneSession.snapshot(dtype) / model.restore_scene(snapshot) / SceneBatch.snapshot(scene) / SceneBatch.restore(scene, snapshot);
SceneSnapshot.save / load).  Everything above happens inside one process, on one device, in one kind of container.  A snapshot is the fused state of a
plain or fading scene as HOST data: a state row is large (26 / 54 / 170 MB of fp32 at the ScanNet-fast / ScanNet-v1 / KITTI grids) and partly unseen --
a single frustum, a scrolled grid and a faded scene leave all-zero voxels -- so ONE ordered stream compaction (ops.volume_pack, ivx_volume_pack_fwd,
csrc/volume_pack.hip; include/imvoxel.h has the definition) keeps the voxels whose count or weight-sum word is non-zero, in ascending voxel order, and
only those records cross the link, beside the scene's host record (kind, decay, threshold, gate, grid, meta, views, scrolled, frame).  restore unpacks
them into a whole row in one launch (ops.volume_unpack_).  The float32 payload is the sums as words: the restored (sum, weight sum, count) are the
original's bit for bit -- the state's invariant that unseen voxels hold all-zero sums is what makes dropping them exact -- so a restored scene goes on
exactly as the original would.  The bfloat16 payload is the mean, half the bytes, sums within (2^-8 + 2^-22) |S|.  A snapshot does not remember its
container: a session's opens as a batch row and a batch row's as a session, on any device, after a restart (.npz, loaded with allow_pickle=False and
validated before it is believed).  A scene that never snapshots runs the code it ran before.

Pixel maps (add_views(..., pixel_weights=..., depths=...); open_scene(meta, ..., depth_gate=(behind, front))).  A weight per view scales a whole
frame, but a person walking through the scan, the robot's own arm, lens dirt and the black border after undistortion are properties of pixels, and
an RGB-D camera knows which voxels on a pixel's ray lie behind the surface it shows.  Sessions that take weights (decay= or window=) take two
optional maps per view at feature resolution: a confidence map that multiplies the view's weight per pixel, and a depth map that, with the gate
fixed at open, lets the view count at a voxel only where the voxel's depth d lies within D - front .. D + behind of the measured D (occlusion carving,
or a truncation band; a pixel with no measurement -- 0, negative, NaN, inf -- gates nothing).  Both are read at the nearest pixel the voxel projects
to, in the same single launch (ops.backproject_mapped_accum_ / _mean_, ivx_backproject_mapped_fwd; include/imvoxel.h has the definition).  Each map
is one float32 tensor [V,FH,FW], host or device, or [V,H,W] at the padded input size, which is reduced by the strided pick map[:, ::s, ::s] with
s = H // FH (pick_map: feature pixel (x, y) is input pixel (s*x, s*y), as in the projection rule; exact); add_views_u8 takes feature resolution only,
and depth frames at the source size through depth_frames= (below).
Fading scenes consume the maps in the tick's launch and keep nothing.  Windowed scenes keep two device rings beside the feature ring ([W,FH,FW] fp32
each, 77 KB per slot at 480 x 640; [N*W,FH,FW] in a batch, scene s owning slots s*W .. s*W+W-1), each allocated when its first map is given -- weights
filled with 1, depths with 0 (no measurement) -- and a slot reused by a view without a map goes back to 1 / 0; eviction, remove_views and scroll need
nothing further, because maps travel with slots and are per view, not per voxel.  depth_gate=None (the default) refuses depth maps; a plain session
refuses both.  A session that never passes a map calls the ops it called before.

View coverage and the keyframe gate (SceneSession.coverage(extrinsics) / SceneBatch.coverage(extrinsics, scene); add_views(..., min_novelty=m)).  Every
frame that reaches add_views pays for the 2-D trunk, and most frames of a 30 Hz camera look at voxels the scene has fused already.  Whether a pose adds
anything depends on the geometry and on the scene's state only, so it is counted before the trunk runs: coverage returns, per candidate pose, how many
voxels the lift would count the view at (seen) and how many of those hold less than fresh_below of evidence (fresh) -- the view count of a plain
session, the weight sum of a fading one, the valid mask of a windowed one -- in one small integer launch (ops.view_coverage, ivx_view_coverage_fwd;
include/imvoxel.h has the definition) whose validity decision is the lift's own, bit for bit, with the confidence map and the gated depth when they
are given.  add_views(..., min_novelty=m) with m in (0, 1] admits a view iff seen > 0 and fresh / seen >= m, tested against the state BEFORE the call
(the views of one call do not see each other; a fading scene's coming fade is not anticipated), and drops the rejected views with their images,
extrinsics, weights and maps before the trunk; a call whose views are all rejected launches nothing more and changes nothing -- no tick on a fading
session, an untouched scene in a batch -- and last_admitted holds the verdicts (None after an ungated call).  min_novelty=None runs the code it ran
before.

Lenses and depth frames (add_views_u8(..., lens=, depth_frames=, depth_scale=)).  The cameras scenes are built for have radial distortion, and the
black border after undistortion is the first use of a confidence map.  One geometric map from a pixel of the network input back to the raw frame
(include/imvoxel.h, the map G of ivx_image_prep_lens_u8) gives all three things such a camera needs, on the device: the undistorted, resized,
normalised image in the pipeline's own launch and in ONE interpolation (data.prepare_images_device(lens=)); the cover map at feature resolution
(ops.map_prep_lens: 1 where the input pixel shows the frame), which multiplies the view's confidence on sessions that take maps and which the
keyframe gate sees as well; and the depth frame of an RGB-D camera, picked at the nearest source pixel of each feature pixel by the same rule.
The cover depends on (lens, source shape, pipeline shapes) only and is cached on the scene or batch.  The meta's intrinsic must be the lens's
new_K.  A scene that never passes lens or depth_frames calls what it called before.

How the module is laid out.  Every host rule is written once.  _SceneRecord is the host state of ONE scene (meta, view list, ids, stale flag, image
size, window, decay, threshold) with the rules that need no device: the checks of meta / window / fading, reset, view_ids, remove_views, which slots
of a range [base, base + W) a windowed add frees and fills, the id-to-slot lookup, the body of reweight.  The argument checks of an add (images,
extrinsics, weights, pixel maps, image size), the strided pick of a map, the weight-ring and map-ring updates, the trunk call and the detection tail are module functions.  A SceneSession IS such a
record plus its own buffers and launches; a SceneBatch HOLDS N records (_scenes) plus its pools and launches.  Only the launches differ between
the two, for a measured reason (profiles/scene_batch.md: the listed lift at one row is about 20 us slower than the plain one), so they stay in
the classes, and nothing shared asks which class called it: wording that differs in a noun is passed in.

Out of scope: a gate in which the views of one call see each other (sequential gating), anticipating a fading scene's next decay in coverage(),
choosing which kept view of a window to evict; decay on windowed scenes; confidence maps at the source size through the add_views_u8 pipeline, a soft (ramp) or signed-distance gate, maps for plain
sessions and for simple_test; warping a plain session (integer view counts cannot be resampled: open it with decay=1.0); non-rigid transforms
(a scale or a shear would not keep the voxel size; ops.check_rigid refuses them); scrolling by a fraction of a voxel (warp resamples instead);
scrolling a model with an Anchor3DHead (its boxes would have to be translated; warp keeps the origin and needs no translation); scene batches across ranks; a model-level C handle for sessions
(the state lives here, over the op-level ABI and the handle's sub-range calls); merging windowed scenes (adopting the other's kept views into the
ring); merging plain scenes (their integer counts cannot be resampled: open them with decay=1.0); merges between a session and a batch row, or
across batches (ops.volume_merge_ takes any pools); several sources into one destination in one launch; de-duplicating views both scenes saw;
estimating T without a start (a global search, no T0), pitch and roll in register's candidate lattice (refine moves them),
weighting pairs by evidence in match or refine, zero-mean (Pearson) correlation, gradient-based refinement with a robust loss (refine's loss is the plain sum of
squares), refining against a snapshot directly (restore it, then refine), solving the normal equations on the device (six unknowns: the host
solves them after a read-back of 31 doubles), matching plain or windowed scenes; saving a scene to disk other than through a snapshot; merging scenes on different devices or ranks directly (snapshot
one and restore it beside the other); snapshots of windowed scenes (the state is the feature ring, a plain copy); merge taking a snapshot directly
(restore it, then merge); turning a plain snapshot into a fading scene; compression of a snapshot beyond the bf16 mean; any check that the weights of
the restoring model are those that fused the state.
"""
import math

import numpy as np
import torch

from . import ops
from .boxes import bbox3d2result
from .heads import Anchor3DHead


# ------------------------------------------------------------------ the argument checks of an add: they need no device and no scene
def _check_images(img, n):
    """img [n,3,H,W] float32 (n: the caller's letter for the views of a call, 'V' or 'T') -> (n, H, W)."""
    if not isinstance(img, torch.Tensor):
        raise TypeError(f'img must be a torch.Tensor [{n},3,H,W]')
    if img.dim() != 4 or img.shape[0] < 1 or img.shape[1] != 3:
        raise ValueError(f'img must be [{n},3,H,W] with {n} >= 1, got {tuple(img.shape)}')
    if img.dtype != torch.float32:
        raise TypeError(f'img must be float32, got {img.dtype}')
    return int(img.shape[0]), int(img.shape[2]), int(img.shape[3])


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


def _check_weights(weights, V):
    """weights: None or V finite floats >= 0 -> list of float."""
    if weights is None:
        return None
    if isinstance(weights, torch.Tensor):
        weights = weights.tolist()
    w = [float(x) for x in (np.asarray(weights, np.float64).reshape(-1).tolist())]
    if len(w) != V:
        raise ValueError(f'{len(w)} weights for {V} views')
    if any(not (math.isfinite(x) and x >= 0) for x in w):
        raise ValueError(f'weights must be finite and >= 0, got {w}')
    return w


def _check_size(hw, have, where):
    """The image size of a call against the one of the views already in `where` ('scene' / 'batch'; have None: there are none)."""
    if have is not None and hw != have:
        raise ValueError(f'image size {hw} differs from the {have} of the views already in the {where}')


def _ring_weights(wring, size, slots, weights):
    """The host weight ring after a windowed add that put its views into `slots`: the ring (None until then, and the re-lift unweighted) starts
    with the first weight given; from then on a reused slot takes its new view's weight (1 when the call gives none)."""
    if weights is not None and wring is None:
        wring = [1.0] * size
    if wring is not None:
        for i, s in enumerate(slots):
            wring[s] = weights[i] if weights is not None else 1.0
    return wring


# ------------------------------------------------------------------ pixel maps: the host rules
MAP_FILL = {'pixel_weights': 1.0, 'depths': 0.0}      # what a view without a map has: confidence 1 everywhere, no measurement anywhere


def _check_map(t, name, V):
    """A pixel map argument of an add before the trunk has run: None, or one float32 tensor [V,h,w] (host or device) -> the tensor."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise TypeError(f'{name} must be None or one float32 torch.Tensor [V,FH,FW] (or [V,H,W]), got {type(t).__name__}')
    if t.dtype != torch.float32:
        raise TypeError(f'{name} must be float32, got {t.dtype}')
    if t.dim() != 3 or t.shape[0] != V:
        raise ValueError(f'{name} must be [V,FH,FW] at feature resolution or [V,H,W] at the input size for the {V} views of this call, got {tuple(t.shape)}')
    return t


def pick_map(t, name, hw, fhw, strided=True):
    """A checked map [V,h,w] at the feature resolution fhw = (FH, FW) of images of the padded size hw = (H, W): a map that has it is taken as it
    is; one at the input size is reduced by the strided pick  map[:, ::s, ::s]  with s = H // FH -- feature pixel (x, y) is input pixel
    (s*x, s*y), as in the model's projection rule -- which moves numbers and rounds nothing.  strided=False (frames resized on the device:
    add_views_u8) takes feature resolution only.  Any other shape raises ValueError."""
    (H, W), (FH, FW) = hw, fhw
    if tuple(t.shape[1:]) == (FH, FW):
        return t
    s = H // FH
    if strided and tuple(t.shape[1:]) == (H, W) and s >= 1 and W // FW == s and tuple(t[:, ::s, ::s].shape[1:]) == (FH, FW):
        return t[:, ::s, ::s]
    raise ValueError(f'{name} must be [V,{FH},{FW}] at feature resolution' + (f' or [V,{H},{W}] at the input size' if strided else
                     ' (frames that are resized on the device take no maps at the input size)') + f', got {tuple(t.shape)}')


def _ring_map(ring, size, fhw, dev, slots, maps, fill):
    """The device ring [size,FH,FW] fp32 of one kind of map after a windowed add that put its views into `slots`: the ring (None until then, and
    the re-lift without that map) starts with the first map given, filled with `fill`; from then on a reused slot takes its new view's map
    (`fill` when the call gives none).  A ring of another feature size (after reset()) is dropped first.  maps: [len(slots),FH,FW] or None."""
    if ring is not None and tuple(ring.shape[1:]) != tuple(fhw):
        ring = None
    if maps is not None and ring is None:
        ring = torch.full((size,) + tuple(fhw), fill, dtype=torch.float32, device=dev)
    if ring is not None:
        idx = torch.tensor(list(slots), dtype=torch.int64).to(dev)
        if maps is not None:
            ring.index_copy_(0, idx, maps.to(dev))
        else:
            ring.index_fill_(0, idx, fill)
    return ring


def _lift_maps(pixel_weight, depth, gate):
    """('mapped', the map arguments of the mapped ops) when a map is there, ('weighted', {}) otherwise: a scene that never sees a map calls the
    weighted ops it called before maps existed."""
    if pixel_weight is None and depth is None:
        return 'weighted', {}
    return 'mapped', dict(pixel_weight=pixel_weight, depth=depth, gate=gate if gate is not None else (math.inf, math.inf))


def _maps_at(maps, hw, p0, strided=True):
    """The checked maps of an add (pixel_weights, depths) at the resolution of the trunk's output p0 [V,1,FH,FW,C], on its device, contiguous."""
    fhw = tuple(int(v) for v in p0.shape[-3:-1])
    return tuple(None if t is None else pick_map(t, name, hw, fhw, strided).to(p0.device).contiguous() for t, name in zip(maps, MAP_FILL))


# ------------------------------------------------------------------ lenses and depth frames of add_views_u8: the host rules and the two small launches
def _check_depth_frames(t, V):
    """depth_frames of an add_views_u8 call: None, or one [V,H,W] uint16 / float32 array or tensor at the source size (host or device) -> tensor."""
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    if not isinstance(t, torch.Tensor):
        raise TypeError(f'depth_frames must be None or one [V,H,W] uint16 / float32 array or tensor, got {type(t).__name__}')
    if t.dtype not in (torch.uint16, torch.float32):
        raise TypeError(f'depth_frames must be uint16 or float32, got {t.dtype}')
    if t.dim() != 3 or t.shape[0] != V:
        raise ValueError(f'depth_frames must be [V,H,W] at the source size for the {V} frames of this call, got {tuple(t.shape)}')
    return t


def _check_intrinsic(meta, lens):
    """The lift projects with the meta's intrinsic, the undistorted image shows lens.new_K: the two must be one camera (an identity intrinsic --
    a meta whose extrinsics carry the whole projection -- is not judged).  More than 1e-6 relative apart raises ValueError."""
    K = np.asarray(meta['lidar2img']['intrinsic'], np.float64)[:3, :3]
    if np.array_equal(K, np.eye(3)) or np.allclose(K, lens.new_K, rtol=1e-6, atol=0.0):
        return
    raise ValueError(f"the scene meta's intrinsic {K.tolist()} is not the lens's new_K {lens.new_K.tolist()}: the lift would project with another "
                     'camera than the undistorted image shows (build the intrinsic from lens.new_K)')


def _lens_maps(records, cache, frames, maps, lens, depth_frames, depth_scale, img_scale, pipeline_kw, what, format=None):
    """What lens= / depth_frames= of an add_views_u8 call add to its checked pixel maps, before the gate and the pipeline run: -> (one lens
    entry per frame or None, (pixel_weights, depths) at feature resolution).  records: the _SceneRecords the call touches (their metas must
    agree with the lenses); cache: the owner's cover cache {(lens, source shape, resized shape, padded shape, device): cover [FH,FW]}.
    On a scene that takes maps a lens makes the cover map (ops.map_prep_lens: 1 where the input pixel shows the frame, 0 on the border)
    part of the view's confidence -- pixel_weights * cover, or the cover alone; a frame whose entry is None keeps its weights -- and
    depth_frames go through the same geometry to feature resolution (one launch per run of frames of one lens).  A plain scene gets the
    undistorted image and no mask."""
    from .data import _check_lenses, _check_formats, _pipeline_shapes
    V, rec = len(frames), records[0]
    lenses = _check_lenses(lens, V)
    dframes = _check_depth_frames(depth_frames, V)
    takes_maps = rec._window is not None or rec._decay is not None
    if dframes is not None:
        if not takes_maps:
            raise ValueError(f'this {what} was opened plain and takes no depth frames: open it with decay=1.0 (weights, nothing fades) or with window=W')
        if rec._gate is None:
            raise ValueError(f'this {what} was opened without depth_gate and takes no depth frames: open it with depth_gate=(behind, front)')
        if maps[1] is not None:
            raise ValueError('depth_frames (at the source size) and depths (at feature resolution) exclude each other')
        if isinstance(depth_scale, bool) or not isinstance(depth_scale, (int, float, np.integer, np.floating)) or not math.isfinite(depth_scale):
            raise ValueError(f'depth_scale must be a finite number, got {depth_scale!r}')
    formats = _check_formats(format, V)                  # (the source size is that of the converted frame)
    src = {(int(f.shape[0]), int(f.shape[1])) if formats is None else formats[i].frame_hw(f.shape) for i, f in enumerate(frames)}
    if len(src) != 1:
        raise ValueError(f'frames that come with a lens or with depth frames must share one source size in a call, got {sorted(src)}')
    src_hw = src.pop()
    if dframes is not None and tuple(dframes.shape[1:]) != src_hw:
        raise ValueError(f'depth_frames must be at the source size {src_hw} of the frames, got {tuple(dframes.shape[1:])}')
    distinct = [] if lenses is None else [l for l in dict.fromkeys(lenses) if l is not None]
    for l in distinct:
        for r in records:
            _check_intrinsic(r.meta, l)
    if not takes_maps:
        return lenses, maps
    size_hw, pad_hw = _pipeline_shapes(src_hw, img_scale, pipeline_kw.get('size_divisor', 32), pipeline_kw.get('keep_ratio', True))
    dev = torch.device(pipeline_kw.get('device', 'cuda'))
    pw, dp = maps
    if distinct:
        for l in distinct:
            key = (l, src_hw, size_hw, pad_hw, str(dev))
            if key not in cache:
                cache[key] = ops.map_prep_lens(size_hw, pad_hw, src_hw, lens=l, stride=4, device=dev)[0]
        covers = {l: cache[(l, src_hw, size_hw, pad_hw, str(dev))] for l in distinct}
        cover = torch.stack([covers[l] if l is not None else torch.ones_like(covers[distinct[0]]) for l in lenses])
        pw = cover if pw is None else pick_map(pw, 'pixel_weights', pad_hw, tuple(cover.shape[1:]), strided=False).to(dev) * cover
    if dframes is not None:
        dframes, ls = dframes.to(dev), lenses if lenses is not None else [None] * V
        dp = torch.empty((V, (pad_hw[0] - 1) // 4 + 1, (pad_hw[1] - 1) // 4 + 1), device=dev, dtype=torch.float32)
        a = 0
        while a < V:                              # runs of frames of one lens: one launch each
            b = a + 1
            while b < V and ls[b] == ls[a]:
                b += 1
            ops.map_prep_lens(size_hw, pad_hw, src_hw, lens=ls[a], src=dframes[a:b], scale=float(depth_scale), stride=4, out=dp[a:b])
            a = b
    return lenses, (pw, dp)


# ------------------------------------------------------------------ view coverage and the keyframe gate: the host rules
def _check_novelty(min_novelty, fresh_below, alone=False):
    """The gate arguments of an add or of coverage() -> (min_novelty as a float or None, fresh_below as a float; None means 1.0: less than one
    full-weight view's worth of evidence).  min_novelty must lie in (0, 1]; fresh_below must be finite and > 0 and, in an add (alone=False),
    needs min_novelty."""
    if fresh_below is not None and min_novelty is None and not alone:
        raise ValueError('fresh_below belongs to the gate: give min_novelty with it')
    if fresh_below is not None and (isinstance(fresh_below, bool) or not isinstance(fresh_below, (int, float, np.integer, np.floating))
                                    or not (math.isfinite(fresh_below) and fresh_below > 0)):
        raise ValueError(f'fresh_below must be None or a finite number > 0, got {fresh_below!r}')
    if min_novelty is not None and (isinstance(min_novelty, bool) or not isinstance(min_novelty, (int, float, np.integer, np.floating))
                                    or not 0 < min_novelty <= 1):
        raise ValueError(f'min_novelty must be None or a number in (0, 1], got {min_novelty!r}')
    return (None if min_novelty is None else float(min_novelty)), (1.0 if fresh_below is None else float(fresh_below))


def admitted(counts, min_novelty):
    """The gate's rule on coverage counts [K,2] (seen, fresh): view k is admitted iff seen > 0 and fresh / seen >= min_novelty, in Python
    floats -> list of K bools."""
    return [bool(int(s) > 0 and int(f) / int(s) >= min_novelty) for s, f in np.asarray(counts).reshape(-1, 2).tolist()]


def _kept(keep, seq):
    """The entries of a per-view argument of an add that the gate admitted: a list stays a list, a tensor is indexed along its first axis on
    its own device, None stays None."""
    idx = [i for i, k in enumerate(keep) if k]
    if seq is None:
        return None
    if isinstance(seq, torch.Tensor):
        return seq[torch.tensor(idx, dtype=torch.int64).to(seq.device)].contiguous()
    return [seq[i] for i in idx]


def _coverage_fhw(hw, meta):
    """The feature-map size (FH, FW) coverage clamps the crop to and reads maps at, before any feature exists: the scene's known padded image
    size // 4 (the stride of FPN level 0), else the meta's pad_shape // 4."""
    if hw is None:
        if 'pad_shape' not in meta:
            raise ValueError('coverage before the first view needs the padded image size: give the scene meta a pad_shape (add_views_u8 fills it)')
        hw = tuple(int(v) for v in meta['pad_shape'][:2])
    return hw, (hw[0] // 4, hw[1] // 4)


def _scene_device(model, *tensors):
    """Where a scene's launches go before it has features: the device of a buffer it holds, else the model's, else the current HIP device."""
    for t in tensors:
        if t is not None:
            return t.device
    return model._prepared_device if model._prepared_device is not None else torch.device('cuda', torch.cuda.current_device())


# ------------------------------------------------------------------ scrolling: the host rules
def scrolled_origin(origin, voxels, voxel_size):
    """The origin rule of a scroll, per component in fp32:  float32(origin) + float32(voxels) * float32(voxel_size)  -- the product is rounded,
    then the sum.  -> float32 array [3]."""
    return np.asarray(origin, np.float32) + np.asarray(voxels).astype(np.float32) * np.asarray(voxel_size, np.float32)


def _check_scroll(model, voxels):
    """voxels of a scroll -> [sx, sy, sz] as ints; a model whose head has anchors refuses."""
    if isinstance(getattr(model, 'bbox_head', None), Anchor3DHead):
        raise NotImplementedError('scroll: the anchors of an Anchor3DHead are fixed in the LiDAR frame (anchor_generator ranges), so its boxes would not '
                                  'follow the grid; translating them is out of scope')
    s = ops._host_ints(voxels, 'voxels')
    if len(s) != 3 or any(not -2 ** 31 <= v < 2 ** 31 for v in s):
        raise ValueError(f'voxels must be three int32 integers (sx, sy, sz), got {voxels!r}')
    return s


# ------------------------------------------------------------------ warping: the host rules
def warped_extrinsic(E, T):
    """The extrinsic of a view after a warp by T (x_old = T x_new):  float32(float64(E) @ float64(T))  -- the camera sees the same points, now
    named in the new frame.  -> float32 array [4,4]."""
    return (np.asarray(E, np.float64) @ np.asarray(T, np.float64)).astype(np.float32)


def _check_warp(T):
    """T of a warp -> float64 array [4,4]: a host 4x4 of numbers, finite, last row (0, 0, 0, 1), rigid by ops.check_rigid's rule."""
    if isinstance(T, torch.Tensor) and not T.is_cuda:
        T = T.detach().numpy()
    if isinstance(T, torch.Tensor) or np.shape(T) != (4, 4):
        raise ValueError(f'T must be a host 4x4 matrix with x_old = T x_new, got {type(T).__name__} of shape {tuple(np.shape(T)) if not isinstance(T, torch.Tensor) else tuple(T.shape)}')
    ops.check_rigid(T, 'T')
    return np.asarray(T, np.float64)


_PLAIN_WARP = ('warp: a plain {what} keeps integer view counts, which cannot be resampled; open it with decay=1.0 (a weight sum beside the sums, '
               'nothing fades) or with window=W')


# ------------------------------------------------------------------ merging: the host rules
_PLAIN_MERGE = ('merge: a plain {what} keeps integer view counts, which cannot be resampled; open it with decay=1.0 (a weight sum beside the sums, '
                'nothing fades)')
_WINDOW_MERGE = ('merge: a windowed {what} (window=W) keeps views, not a running state; adopting the kept views of another scene into the ring is '
                 'out of scope: open it with decay=')


def _check_merge_kind(window, fading, what):
    """Only fading scenes merge: a windowed or a plain one (what: 'session' / 'batch', as it was opened) refuses."""
    if window is not None:
        raise NotImplementedError(_WINDOW_MERGE.format(what=what))
    if not fading:
        raise NotImplementedError(_PLAIN_MERGE.format(what=what))


def _check_merge_weight(weight):
    """weight of a merge -> float: one finite number > 0 (as float32 too: it reaches the kernel as alpha)."""
    if isinstance(weight, bool) or not isinstance(weight, (int, float, np.integer, np.floating)):
        raise TypeError(f'weight must be a number > 0, got {weight!r}')
    weight = float(weight)
    if not (math.isfinite(weight) and np.float32(weight) > 0 and np.isfinite(np.float32(weight))):
        raise ValueError(f'weight must be finite and > 0, got {weight}')
    return weight


def _merge_transform(dst, src, T):
    """T of a merge of the record src into the record dst (x_src = T x_dst) -> float64 [4,4]: the caller's, by the _check_warp rule, or for None
    inv(src.frame) @ dst.frame in float64 -- the two scenes were opened in one common frame."""
    if T is not None:
        return _check_warp(T)
    T = np.linalg.inv(src._frame) @ dst._frame
    T[3] = (0, 0, 0, 1)
    return T


# ------------------------------------------------------------------ matching: the host rules
_PLAIN_MATCH = ('{op}: a plain {what} keeps integer view counts and no weight sum, so it has no mean field to sample; open it with decay=1.0 (a weight '
                'sum beside the sums, nothing fades)')
_WINDOW_MATCH = ('{op}: a windowed {what} (window=W) keeps views, not a running state; matching it is out of scope: open it with decay=')


def _check_match_kind(window, fading, what, op='match'):
    """Only fading scenes match: a windowed or a plain one (what: 'session' / 'batch', as it was opened) refuses."""
    if window is not None:
        raise NotImplementedError(_WINDOW_MATCH.format(what=what, op=op))
    if not fading:
        raise NotImplementedError(_PLAIN_MATCH.format(what=what, op=op))


def _check_min_overlap(min_overlap):
    if isinstance(min_overlap, bool) or not isinstance(min_overlap, (int, float, np.integer, np.floating)) or not 0 <= float(min_overlap) <= 1:
        raise ValueError(f'min_overlap must be a number in [0, 1], got {min_overlap!r}')
    return float(min_overlap)


def _rigid_yaw(yaw, t, about):
    """float64 [4,4]: the turn by `yaw` about the vertical through the point `about`, then the translation t."""
    c, s = math.cos(yaw), math.sin(yaw)
    T = np.eye(4)
    T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    about = np.asarray(about, np.float64)
    T[:3, 3] = about - T[:3, :3] @ about + np.asarray(t, np.float64)
    return T


def pose_candidates(T_c, yaw, shift, about=(0, 0, 0)):
    """The 81 candidates of one level of register around T_c (a 4x4 with x_other = T x_self):  T_c @ rigid(yaw=a, t=(x, y, z), about=about)  with
    a in (-yaw, 0, +yaw) and x, y, z in (-h, 0, +h) of shift = (h_x, h_y, h_z), in the order a, x, y, z with z fastest -- so candidate 40 is T_c
    itself, bit for bit, and candidates i and 80 - i carry opposite offsets.  yaw in radians, shift in metres, both >= 0; `about` is the point the
    turn goes through (register: the grid's centre).  Needs no device.  -> list of 81 float64 [4,4]."""
    T_c = _check_warp(T_c)
    sh = np.asarray(shift, np.float64).reshape(-1)
    ab = np.asarray(about, np.float64).reshape(-1)
    if isinstance(yaw, bool) or not isinstance(yaw, (int, float, np.integer, np.floating)) or not (math.isfinite(yaw) and yaw >= 0):
        raise ValueError(f'yaw must be a finite number >= 0 (radians), got {yaw!r}')
    if sh.shape != (3,) or not (np.isfinite(sh).all() and (sh >= 0).all()):
        raise ValueError(f'shift must be three finite numbers >= 0 (h_x, h_y, h_z), got {shift!r}')
    if ab.shape != (3,) or not np.isfinite(ab).all():
        raise ValueError(f'about must be three finite coordinates, got {about!r}')
    out = []
    for a in (-1, 0, 1):
        for x in (-1, 0, 1):
            for y in (-1, 0, 1):
                for z in (-1, 0, 1):
                    out.append(T_c.copy() if (a, x, y, z) == (0, 0, 0, 0) else T_c @ _rigid_yaw(a * float(yaw), (x * sh[0], y * sh[1], z * sh[2]), ab))
    return out


class MatchResult:
    """What a match says about K candidate transforms, as host numpy arrays:
      pairs   [K] int64    the voxels of this scene that hold evidence and whose sample of the other scene does too
      own     int          the voxels of this scene that hold evidence (of those visited)
      overlap [K] float64  pairs / own (0 where own is 0)
      score   [K] float64  ncc = dot / sqrt(na * nb), the cosine of the two mean fields over the paired voxels; -inf where a candidate is not
                           eligible: pairs == 0, overlap < min_overlap, or a norm that is not positive
      stats   [K,3] float64  (dot, na, nb) as the device summed them
      best    int or None  the eligible candidate of the highest score (the first of equals); None when none is eligible
      T       float64 [4,4] or None  that candidate
      Ts      the candidates."""

    def __init__(self, pairs, own, stats, Ts, min_overlap=0.3):
        self.pairs, self.own, self.stats = np.asarray(pairs, np.int64).reshape(-1), int(own), np.asarray(stats, np.float64).reshape(-1, 3)
        self.Ts, self.min_overlap = [np.asarray(T, np.float64) for T in Ts], _check_min_overlap(min_overlap)
        if not (len(self.pairs) == len(self.stats) == len(self.Ts)):
            raise ValueError(f'{len(self.pairs)} pair counts, {len(self.stats)} statistics and {len(self.Ts)} candidates')
        self.overlap = self.pairs / self.own if self.own > 0 else np.zeros(len(self.pairs))
        dot, den = self.stats[:, 0], self.stats[:, 1] * self.stats[:, 2]
        ok = (self.pairs > 0) & (self.overlap >= self.min_overlap) & (den > 0)
        with np.errstate(invalid='ignore', divide='ignore'):
            self.score = np.where(ok, dot / np.sqrt(np.where(ok, den, 1.0)), -np.inf)
        self.best = int(np.argmax(self.score)) if ok.any() else None
        self.T = None if self.best is None else self.Ts[self.best].copy()

    def __repr__(self):
        return f'MatchResult(K={len(self.pairs)}, best={self.best}, score={None if self.best is None else float(self.score[self.best]):}, own={self.own})'


def _match_candidates(dst, src, Ts):
    """Ts of a match of the record dst against the record src -> list of float64 [4,4] with x_src = T x_dst: the caller's host list, each by the
    _check_warp rule, or for None the one candidate a merge would default to."""
    if Ts is None:
        return [_merge_transform(dst, src, None)]
    if isinstance(Ts, (str, bytes, torch.Tensor, np.ndarray)) or not hasattr(Ts, '__len__') or not len(Ts):
        raise ValueError('Ts must be None or a non-empty host list of 4x4 matrices with x_other = T x_self')
    return [_check_warp(T) for T in Ts]


def _match_results(pairs, own, stats, cands, min_overlap):
    """The device outputs of one ops.volume_match over P pairs -> P MatchResults (the one host sync of a match)."""
    pairs, own, stats = pairs.cpu().numpy(), own.cpu().numpy(), stats.cpu().numpy()
    return [MatchResult(pairs[p], own[p], stats[p], cands[p], min_overlap) for p in range(len(cands))]


def _register(match, T0, yaw, shift, levels, step, min_overlap, about, voxel_size):
    """The coarse-to-fine search of register, shared by sessions and batches: match(Ts, step) -> MatchResult scores one level's candidates.
    -> (T float64 [4,4], the MatchResult of the last level)."""
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or levels < 1:
        raise ValueError(f'levels must be an integer >= 1, got {levels!r}')
    steps = list(step) if hasattr(step, '__len__') and not isinstance(step, (str, bytes, torch.Tensor)) else [step] * levels
    if len(steps) != levels:
        raise ValueError(f'step must be one integer for every level or a list of one lattice step per level: {levels} levels, got {step!r}')
    steps = [ops._match_step(s) for s in steps]
    vs = np.asarray(voxel_size, np.float64)
    shift = np.array([2 * vs[0], 2 * vs[1], vs[2]]) if shift is None else np.asarray(shift, np.float64).reshape(-1)
    min_overlap = _check_min_overlap(min_overlap)
    T = T0
    pose_candidates(T, yaw, shift, about)                                    # (every argument is checked before the first launch)
    res = None
    for lv in range(levels):
        res = match(pose_candidates(T, yaw, shift, about), steps[lv])
        if res.best is not None:
            T = res.T
        yaw, shift = yaw / 2, shift / 2
    return T, res


# ------------------------------------------------------------------ aligning: the host rules
ALIGN_DOF = ('x', 'y', 'z', 'rx', 'ry', 'rz')     # the order of g and of the rows of H: three translations, three rotation-vector components
REGISTER_DOF = ('x', 'y', 'z', 'rz')              # what register(refine=True) refines unless told otherwise: the degrees its lattice searches
DAMPING_FLOOR, DAMPING_CAP = 1e-9, 1e6            # Levenberg-Marquardt: accepted steps divide the damping by 10 down to the floor; beyond the cap it stops
_TRIU = tuple((i, j) for i in range(6) for j in range(i, 6))


def _check_dof(dof):
    """dof: a non-empty host sequence of names out of ALIGN_DOF, each once -> the sorted list of their indices."""
    if isinstance(dof, (str, bytes)) or not hasattr(dof, '__len__') or not len(dof) or any(d not in ALIGN_DOF for d in dof) or len(set(dof)) != len(dof):
        raise ValueError(f'dof must be a non-empty sequence of distinct names out of {ALIGN_DOF}, got {dof!r}')
    return sorted(ALIGN_DOF.index(d) for d in dof)


def rigid_increment(xi, about=(0, 0, 0)):
    """float64 [4,4]: the rotation by the rotation vector xi[3:] (radians, Rodrigues' formula) about the point `about`, then the translation
    xi[:3] -- the small motion of a destination point that ivx_volume_align_fwd differentiates by:  p -> about + R (p - about) + xi[:3].
    Needs no device."""
    xi, about = np.asarray(xi, np.float64).reshape(-1), np.asarray(about, np.float64).reshape(-1)
    if xi.shape != (6,) or not np.isfinite(xi).all():
        raise ValueError(f'xi must be six finite numbers (x, y, z, rx, ry, rz), got {xi!r}')
    if about.shape != (3,) or not np.isfinite(about).all():
        raise ValueError(f'about must be three finite coordinates, got {about!r}')
    w = xi[3:]
    th = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    s, c = (1.0 - th * th / 6, 0.5 - th * th / 24) if th < 1e-8 else (math.sin(th) / th, (1 - math.cos(th)) / (th * th))
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + s * K + c * (K @ K)
    T[:3, 3] = about - T[:3, :3] @ about + xi[:3]
    return T


def solve_align(H, g, damping=0.0, dof=ALIGN_DOF):
    """The Levenberg-Marquardt step of the normal equations H [6,6], g [6] of ivx_volume_align_fwd:  (H + damping * diag(H)) delta = -g  on the
    degrees of freedom `dof` (names out of ALIGN_DOF), zeros elsewhere.  -> delta float64 [6]; NaN on the selected degrees where the system is
    singular or not finite.  Needs no device."""
    H, g = np.asarray(H, np.float64), np.asarray(g, np.float64).reshape(-1)
    if H.shape != (6, 6) or g.shape != (6,):
        raise ValueError(f'H must be [6,6] and g [6], got {H.shape} and {g.shape}')
    if isinstance(damping, bool) or not isinstance(damping, (int, float, np.integer, np.floating)) or not (math.isfinite(damping) and damping >= 0):
        raise ValueError(f'damping must be a finite number >= 0, got {damping!r}')
    sel = _check_dof(dof)
    A, delta = H[np.ix_(sel, sel)], np.zeros(6)
    A = A + float(damping) * np.diag(np.diag(A))
    try:
        if not (np.isfinite(A).all() and np.isfinite(g).all()):
            raise np.linalg.LinAlgError
        delta[sel] = np.linalg.solve(A, -g[sel])
    except np.linalg.LinAlgError:
        delta[sel] = np.nan
    return delta


class AlignResult:
    """What a refinement says, as host data: the pose it ends at and the normal equations there.
      T        float64 [4,4]  the pose (x_other = T x_self)
      cost     float          e / (used * C), the mean squared difference of the two mean fields over the used voxels (inf where used == 0)
      used, pairs, own  int   the voxels that carry the gradient / that both scenes hold evidence for / that this scene holds evidence for
      overlap  float          used / own (0 where own is 0)
      ncc      float          dot / sqrt(na * nb) over the paired voxels, match's score (-inf where a norm is not positive)
      g, H     float64 [6], [6,6]   sum J r and sum J J^T in the order ALIGN_DOF
      stats    float64 [31]   as the device summed them
      evaluations, accepted  int   launches of the refinement; steps that lowered the cost
      converged  bool         the last step was below both tolerances
      history  list of float  the cost at the start and after every accepted step, strictly decreasing
      ok       bool           the start was eligible: used > 0 and overlap >= min_overlap."""

    def __init__(self, T, pairs, used, own, stats, channels, min_overlap=0.3):
        self.T, self.stats = np.array(T, np.float64), np.asarray(stats, np.float64).reshape(-1)
        if self.T.shape != (4, 4) or self.stats.shape != (31,):
            raise ValueError(f'T must be [4,4] and stats [31], got {self.T.shape} and {self.stats.shape}')
        self.pairs, self.used, self.own, self.channels = int(pairs), int(used), int(own), int(channels)
        self.min_overlap = _check_min_overlap(min_overlap)
        self.overlap = self.used / self.own if self.own > 0 else 0.0
        dot, na, nb, e = (float(v) for v in self.stats[:4])
        self.e, self.cost = e, (e / (self.used * self.channels) if self.used > 0 else math.inf)
        self.ncc = dot / math.sqrt(na * nb) if na * nb > 0 else -math.inf
        self.g = self.stats[4:10].copy()
        self.H = np.zeros((6, 6))
        for n, (i, j) in enumerate(_TRIU):
            self.H[i, j] = self.H[j, i] = self.stats[10 + n]
        self.ok = self.eligible
        self.evaluations, self.accepted, self.converged, self.history = 1, 0, False, [self.cost]

    @property
    def eligible(self):
        return self.used > 0 and self.overlap >= self.min_overlap and math.isfinite(self.cost)

    def __repr__(self):
        return (f'AlignResult(ok={self.ok}, cost={self.cost:.6g}, used={self.used}, overlap={self.overlap:.3f}, evaluations={self.evaluations}, '
                f'accepted={self.accepted}, converged={self.converged})')


def _check_refine(iters, dof, min_overlap, damping, tol_shift, tol_rot, voxel_size):
    """The host arguments of a refinement -> (iters, dof indices as names, min_overlap, damping, tol_shift, tol_rot)."""
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or iters < 1:
        raise ValueError(f'iters must be an integer >= 1 (the evaluations a refinement may spend), got {iters!r}')
    sel = _check_dof(dof)
    min_overlap = _check_min_overlap(min_overlap)
    num = lambda v: not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(v)      # noqa: E731
    if not num(damping) or not 0 < damping <= DAMPING_CAP:
        raise ValueError(f'damping must be a finite number in (0, {DAMPING_CAP:g}], got {damping!r}')
    if tol_shift is None:
        tol_shift = 1e-3 * float(np.min(np.asarray(voxel_size, np.float64)))
    if not num(tol_shift) or tol_shift < 0 or not num(tol_rot) or tol_rot < 0:
        raise ValueError(f'tol_shift (metres) and tol_rot (radians) must be finite numbers >= 0, got {tol_shift!r} and {tol_rot!r}')
    return int(iters), tuple(ALIGN_DOF[i] for i in sel), min_overlap, float(damping), float(tol_shift), float(tol_rot)


def _refine(align, T0s, abouts, channels, iters, dof, min_overlap, damping, tol_shift, tol_rot):
    """The Levenberg-Marquardt loop of refine, shared by sessions and batches, over P pairs in lockstep: align(idx, Ts) evaluates the poses Ts of
    the pairs idx (two lists of one length) in ONE call and returns one (pairs, used, own, stats [31]) of host numbers per pose.  The arguments
    have passed _check_refine.  One rule, per pair:
      evaluate at T (the first evaluation is T0; a T0 that is not eligible -- used > 0 and used / own >= min_overlap -- ends the pair, ok False);
      delta = solve_align(H, g, damping, dof); a non-finite delta ends the pair; a delta below tol_shift (|delta[:3]|) AND tol_rot (|delta[3:]|)
      ends it converged; `iters` evaluations end it;
      the trial T @ rigid_increment(delta, about) is evaluated and ACCEPTED iff it is eligible and its cost is strictly lower: then T is the trial
      and damping = max(damping / 10, DAMPING_FLOOR); otherwise damping *= 10, and a damping above DAMPING_CAP ends the pair.
    A pair's numbers do not depend on which other pairs run beside it.  -> list of P (T float64 [4,4], AlignResult at T)."""
    P = len(T0s)
    first = align(list(range(P)), [np.array(T, np.float64) for T in T0s])
    cur = [AlignResult(T0s[p], *first[p], channels, min_overlap) for p in range(P)]
    lam, running = [damping] * P, [p for p in range(P) if cur[p].ok]
    while running:
        idx, trials = [], []
        for p in running:
            c = cur[p]
            delta = solve_align(c.H, c.g, lam[p], dof)
            if not np.isfinite(delta).all():
                continue                                                     # a non-finite solve
            if np.linalg.norm(delta[:3]) < tol_shift and np.linalg.norm(delta[3:]) < tol_rot:
                c.converged = True
                continue
            if c.evaluations >= iters:
                continue
            idx.append(p)
            trials.append(c.T @ rigid_increment(delta, abouts[p]))
        if not idx:
            break
        res, running = align(idx, trials), []
        for p, T, out in zip(idx, trials, res):
            c, t = cur[p], AlignResult(T, *out, channels, min_overlap)
            if t.eligible and t.cost < c.cost:
                t.evaluations, t.accepted, t.history = c.evaluations + 1, c.accepted + 1, c.history + [t.cost]
                cur[p], lam[p] = t, max(lam[p] / 10, DAMPING_FLOOR)
            else:
                c.evaluations += 1
                lam[p] *= 10
            if lam[p] <= DAMPING_CAP:
                running.append(p)
    return [(c.T.copy(), c) for c in cur]


def _refine_T0s(pairs, T0s):
    """T0s of a refinement over the record pairs [(dst, src)] -> list of float64 [4,4]: None (every pair starts where a merge would default to),
    or one 4x4 or None per pair."""
    if T0s is None:
        T0s = [None] * len(pairs)
    if isinstance(T0s, (str, bytes, torch.Tensor, np.ndarray)) or not hasattr(T0s, '__len__') or len(T0s) != len(pairs):
        raise ValueError(f'T0s must be None or a host list of one 4x4 (or None) per pair: {len(pairs)} pairs, got {T0s!r}')
    return [_merge_transform(d, s, T) for (d, s), T in zip(pairs, T0s)]


def _align_host(outs, n):
    """The device outputs of one ops.volume_align over n pairs with K = 1 -> n (pairs, used, own, stats [31]) of host numbers: the one host sync of
    an iteration, 31 doubles and three counts per pair."""
    pairs, used, own, stats = (t.cpu().numpy() for t in outs)
    return [(int(pairs[p, 0]), int(used[p, 0]), int(own[p]), stats[p, 0]) for p in range(n)]


def _check_register_refine(refine, dof):
    """refine / dof of a register -> the dof names its refinement moves (None without refine): checked before the first launch."""
    if not isinstance(refine, (bool, np.bool_)):
        raise ValueError(f'refine must be True or False, got {refine!r}')
    if not refine:
        if dof is not None:
            raise ValueError('dof names what refine=True moves; without refine= it has no meaning')
        return None
    return tuple(ALIGN_DOF[i] for i in _check_dof(REGISTER_DOF if dof is None else dof))


def _last_step(step):
    """The lattice step of the last level of a register: `step` itself, or the last of a list of one step per level."""
    return step[-1] if hasattr(step, '__len__') and not isinstance(step, (str, bytes, torch.Tensor)) and len(step) else step


# ------------------------------------------------------------------ snapshots: a scene's fused state as host data
SNAPSHOT_FORMAT = 1
LIBRARY_VERSION = 560                             # the library version that wrote a snapshot (ivx_version() of the 0.5.6 entries)
_WINDOW_SNAPSHOT = ('snapshot: a windowed {what} (window=W) keeps views, not a running state; its state is the feature ring, a plain copy with no kernel, '
                    'which is out of scope: open it with decay= or plain')
_SNAP_SCALARS = ('format', 'version', 'kind', 'decay', 'forget_below', 'channels', 'sampling', 'n_views', 'box_type', 'payload_dtype')
_SNAP_ARRAYS = ('index', 'payload', 'count', 'wsum', 'depth_gate', 'grid', 'voxel_size', 'intrinsic', 'origin', 'extrinsics', 'img_shape', 'ori_shape', 'pad_shape',
                'hw', 'scrolled', 'frame')


class SceneSnapshot:
    """The fused state of one plain or fading scene as HOST data: the packed records of the voxels that hold evidence (ops.volume_pack) and the
    scene's host record.  No device buffer, no model reference: a snapshot outlives the process, the device and the container (a SceneSession or a
    row of a SceneBatch) it was taken from.  scene.snapshot() / batch.snapshot(scene) make one, model.restore_scene(snapshot) / batch.restore(scene,
    snapshot) open a scene from one, save(path) / SceneSnapshot.load(path) move it through an .npz file.

    Records (numpy, n_seen of them, in ascending flat voxel index n = (i*Y + j)*Z + k): index int32 [n]; payload [n,C] -- float32, the sums, every
    bit as it was, or uint16, the bf16 words of the mean S / den (dtype=torch.bfloat16: half the bytes; restored sums lie within (2^-8 + 2^-22) |S|);
    count int32 [n]; wsum float32 [n] (a fading scene; None for a plain one).
    The scene: kind ('plain' / 'fading'), decay, forget_below, depth_gate (None or (behind, front)); grid (X, Y, Z), channels C, voxel_size and the
    sampling rule of the model that fused it; the meta's lidar2img intrinsic, origin and extrinsics [V,4,4]; img_shape / ori_shape / pad_shape when
    the meta had them; hw, the padded image size of the views; n_views, scrolled, frame; box_type, the name of the meta's box_type_3d class (None:
    the head's default); payload_dtype, version (the library's) and format.  Other keys of the meta are not kept.
    nbytes: the bytes of the records; n_seen; seen_fraction = n_seen / (X*Y*Z).

    A snapshot built from arrays -- by hand, or by load -- is validated before it is believed: ValueError names what is wrong.  load reads with
    allow_pickle=False, so nothing in a file is executed.
    Out of scope: windowed scenes; merge taking a snapshot directly (restore it, then merge); turning a plain snapshot into a fading scene;
    compression beyond the bf16 mean; any check that the weights of the restoring model are those that fused the state."""

    def __init__(self, index, payload, count, wsum=None, *, kind, grid, channels, voxel_size, sampling, intrinsic, origin, extrinsics=None, decay=None,
                 forget_below=0.0, depth_gate=None, img_shape=None, ori_shape=None, pad_shape=None, hw=None, n_views=0, scrolled=(0, 0, 0), frame=None,
                 box_type=None, version=LIBRARY_VERSION, format=SNAPSHOT_FORMAT):
        opt = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt)      # noqa: E731
        self.index, self.payload, self.count, self.wsum = np.ascontiguousarray(index), np.ascontiguousarray(payload), np.ascontiguousarray(count), opt(wsum, None)
        self.kind, self.decay, self.forget_below = kind, (None if decay is None else float(decay)), float(forget_below)
        self.depth_gate = None if depth_gate is None else tuple(float(v) for v in depth_gate)
        self.grid, self.channels = tuple(int(v) for v in grid), int(channels)
        self.voxel_size, self.sampling = tuple(float(v) for v in voxel_size), sampling
        self.intrinsic, self.origin = np.ascontiguousarray(intrinsic), np.ascontiguousarray(origin)
        self.extrinsics = np.zeros((0, 4, 4), np.float32) if extrinsics is None or len(extrinsics) == 0 else np.ascontiguousarray(extrinsics)
        self.img_shape, self.ori_shape, self.pad_shape, self.hw = (None if v is None else tuple(int(x) for x in v) for v in (img_shape, ori_shape, pad_shape, hw))
        self.n_views, self.scrolled = int(n_views), tuple(int(v) for v in scrolled)
        self.frame = np.eye(4) if frame is None else np.ascontiguousarray(frame, np.float64)
        self.box_type, self.version, self.format = box_type, int(version), int(format)
        self._validate()

    def _validate(self):
        """ValueError that names what is wrong with this snapshot; nothing of it is used before this has passed."""
        if self.format != SNAPSHOT_FORMAT:
            raise ValueError(f'snapshot: format {self.format} is not the format {SNAPSHOT_FORMAT} this version reads')
        if self.kind not in ('plain', 'fading'):
            raise ValueError(f"snapshot: kind must be 'plain' or 'fading', got {self.kind!r}")
        if self.sampling not in ('nearest', 'bilinear'):
            raise ValueError(f"snapshot: sampling must be 'nearest' or 'bilinear', got {self.sampling!r}")
        if len(self.grid) != 3 or any(v < 1 for v in self.grid) or self.grid[0] * self.grid[1] * self.grid[2] >= 2 ** 31:
            raise ValueError(f'snapshot: grid must be three positive sizes with X*Y*Z below 2^31, got {self.grid}')
        if self.channels < 4 or self.channels % 4:
            raise ValueError(f'snapshot: channels must be a positive multiple of 4, got {self.channels}')
        if len(self.voxel_size) != 3 or not all(math.isfinite(v) and v > 0 for v in self.voxel_size):
            raise ValueError(f'snapshot: voxel_size must be three finite numbers > 0, got {self.voxel_size}')
        if (self.kind == 'fading') != (self.decay is not None) or (self.decay is not None and not 0 < self.decay <= 1):
            raise ValueError(f'snapshot: a fading scene has a decay in (0, 1] and a plain one has none, got kind {self.kind!r} with decay {self.decay!r}')
        if not (math.isfinite(self.forget_below) and self.forget_below >= 0) or (self.kind == 'plain' and self.forget_below != 0):
            raise ValueError(f'snapshot: forget_below must be finite and >= 0 (0 on a plain scene), got {self.forget_below}')
        if self.depth_gate is not None and (len(self.depth_gate) != 2 or self.kind == 'plain' or not all(v >= 0 for v in self.depth_gate)):
            raise ValueError(f'snapshot: depth_gate must be None or (behind, front), both >= 0, on a fading scene, got {self.depth_gate}')
        n, nvox = (int(self.index.shape[0]) if self.index.ndim == 1 else -1), self.grid[0] * self.grid[1] * self.grid[2]
        if n < 0 or self.index.dtype != np.int32:
            raise ValueError(f'snapshot: index must be int32 [n], got {self.index.dtype} {self.index.shape}')
        if self.payload.dtype not in (np.float32, np.uint16):
            raise ValueError(f'snapshot: payload must be float32 (the sums) or uint16 (bf16 words of the mean), got {self.payload.dtype}')
        if self.payload.shape != (n, self.channels):
            raise ValueError(f'snapshot: payload must be [{n},{self.channels}] (one row of C = {self.channels} channels per index), got {self.payload.shape}')
        if self.count.dtype != np.int32 or self.count.shape != (n,):
            raise ValueError(f'snapshot: count must be int32 [{n}], got {self.count.dtype} {self.count.shape}')
        if (self.wsum is not None) != (self.kind == 'fading'):
            raise ValueError(f'snapshot: a fading scene has a weight sum per record and a plain one has none (kind {self.kind!r})')
        if self.wsum is not None and (self.wsum.dtype != np.float32 or self.wsum.shape != (n,)):
            raise ValueError(f'snapshot: wsum must be float32 [{n}], got {self.wsum.dtype} {self.wsum.shape}')
        if n and (self.index[0] < 0 or self.index[-1] >= nvox or (np.diff(self.index.astype(np.int64)) <= 0).any()):
            raise ValueError(f'snapshot: index must be strictly ascending inside [0, {nvox})')
        if self.intrinsic.dtype != np.float32 or self.intrinsic.ndim != 2 or min(self.intrinsic.shape) < 3 or not np.isfinite(self.intrinsic).all():
            raise ValueError(f'snapshot: intrinsic must be a finite float32 matrix of at least 3x3, got {self.intrinsic.dtype} {self.intrinsic.shape}')
        if self.origin.shape != (3,) or not np.isfinite(np.asarray(self.origin, np.float64)).all():
            raise ValueError(f'snapshot: origin must be three finite numbers, got shape {self.origin.shape}')
        if self.extrinsics.dtype != np.float32 or self.extrinsics.ndim != 3 or self.extrinsics.shape[1:] != (4, 4) or not np.isfinite(self.extrinsics).all():
            raise ValueError(f'snapshot: extrinsics must be finite float32 [V,4,4], got {self.extrinsics.dtype} {self.extrinsics.shape}')
        if self.n_views < 0 or self.extrinsics.shape[0] != self.n_views:
            raise ValueError(f'snapshot: {self.extrinsics.shape[0]} extrinsics for n_views = {self.n_views}')
        if (n != 0 or self.hw is not None) if self.n_views == 0 else self.hw is None:
            raise ValueError(f'snapshot: a scene without views has no records and no image size, one with views has an image size (n_views {self.n_views}, '
                             f'{n} records, hw {self.hw})')
        if self.n_views and (self.img_shape is None or self.ori_shape is None):
            raise ValueError('snapshot: a scene with views knows its img_shape and ori_shape')
        if self.frame.shape != (4, 4) or not np.isfinite(self.frame).all():
            raise ValueError(f'snapshot: frame must be a finite 4x4 matrix, got shape {self.frame.shape}')
        if len(self.scrolled) != 3:
            raise ValueError(f'snapshot: scrolled must be three integers, got {self.scrolled}')
        for name in ('img_shape', 'ori_shape', 'pad_shape', 'hw'):
            v = getattr(self, name)
            if v is not None and (len(v) not in ((2,) if name == 'hw' else (2, 3)) or any(x < 1 for x in v)):
                raise ValueError(f'snapshot: {name} must be None or positive sizes, got {v}')
        if self.box_type is not None and not isinstance(self.box_type, str):
            raise ValueError(f'snapshot: box_type must be None or the name of a box class, got {self.box_type!r}')

    @property
    def payload_dtype(self):
        """'float32' (the sums, as words) or 'bfloat16' (the mean)."""
        return 'float32' if self.payload.dtype == np.float32 else 'bfloat16'

    @property
    def n_seen(self):
        return int(self.index.shape[0])

    @property
    def seen_fraction(self):
        return self.n_seen / float(self.grid[0] * self.grid[1] * self.grid[2])

    @property
    def nbytes(self):
        """The bytes of the packed records."""
        return int(sum(a.nbytes for a in (self.index, self.payload, self.count, self.wsum) if a is not None))

    def records(self):
        """(index, payload, wsum or None, count): the record tuple of ops.volume_unpack_."""
        return self.index, self.payload, self.wsum, self.count

    def save(self, path):
        """Write the snapshot to `path` as an uncompressed .npz of plain arrays (no pickled object).  A field that is None is left out.  Returns path."""
        out = {k: np.asarray(getattr(self, k)) for k in _SNAP_SCALARS + _SNAP_ARRAYS if getattr(self, k) is not None}
        with open(path, 'wb') as f:
            np.savez(f, **out)
        return path

    @classmethod
    def load(cls, path):
        """Read a snapshot written by save.  allow_pickle=False: a file that holds a pickled object raises ValueError and nothing in it is executed;
        the result is validated like any snapshot built from arrays."""
        try:
            z = np.load(path, allow_pickle=False)
        except ValueError as e:                   # (a bare pickle instead of an archive)
            raise ValueError(f'snapshot {path}: not an .npz archive of plain arrays ({e})') from None
        if not hasattr(z, 'files'):
            raise ValueError(f'snapshot {path}: not an .npz archive')
        with z:
            unknown = sorted(set(z.files) - set(_SNAP_SCALARS + _SNAP_ARRAYS))
            missing = sorted({'format', 'kind', 'index', 'payload', 'count', 'grid', 'channels', 'voxel_size', 'sampling', 'intrinsic', 'origin'} - set(z.files))
            if unknown or missing:
                raise ValueError(f'snapshot {path}: not a scene snapshot (missing fields {missing}, unknown fields {unknown})')
            try:
                d = {k: z[k] for k in z.files}
            except ValueError as e:               # numpy's refusal of an object array
                raise ValueError(f'snapshot {path}: a field holds a pickled object, which is never loaded ({e})') from None
        if int(d['format']) != SNAPSHOT_FORMAT:
            raise ValueError(f'snapshot {path}: format {int(d["format"])} is not the format {SNAPSHOT_FORMAT} this version reads')
        for k in _SNAP_SCALARS:
            if k in d:
                if d[k].ndim != 0:
                    raise ValueError(f'snapshot {path}: {k} must be a scalar, got shape {d[k].shape}')
                d[k] = d[k].item()
        d.pop('payload_dtype', None)              # (told by the payload's own dtype)
        return cls(d.pop('index'), d.pop('payload'), d.pop('count'), d.pop('wsum', None), **d)


_BOX_TYPES = ('LiDARInstance3DBoxes', 'DepthInstance3DBoxes')


def _snapshot_of(rec, model, records, channels):
    """The SceneSnapshot of the record `rec` of a plain or fading scene of `model` with the host records (index, payload, wsum, count) as numpy."""
    l2i, bt = rec.meta['lidar2img'], rec.meta.get('box_type_3d')
    index, payload, wsum, count = records
    return SceneSnapshot(index, payload, count, wsum, kind='plain' if rec._decay is None else 'fading', decay=rec._decay, forget_below=rec._forget,
                         depth_gate=rec._gate, grid=model.n_voxels, channels=channels, voxel_size=model.voxel_size, sampling=getattr(model, 'sampling', 'nearest'),
                         intrinsic=np.array(l2i['intrinsic']), origin=np.array(l2i['origin']), extrinsics=[np.asarray(e) for e in l2i['extrinsic']],
                         img_shape=rec.meta.get('img_shape'), ori_shape=rec.meta.get('ori_shape'), pad_shape=rec.meta.get('pad_shape'), hw=rec._hw,
                         n_views=rec.n_views, scrolled=rec._scrolled, frame=rec._frame.copy(), box_type=None if bt is None else getattr(bt, '__name__', str(bt)),
                         version=ops._lib.lib().ivx_version())


def _host_records(recs, channels, dtype, fading):
    """The device records of ops.volume_pack (None: an empty scene) -> numpy (index, payload, wsum, count): the copy to the host of n records only."""
    if recs is None:
        pay = np.zeros((0, channels), np.float32 if dtype == torch.float32 else np.uint16)
        return np.zeros((0,), np.int32), pay, (np.zeros((0,), np.float32) if fading else None), np.zeros((0,), np.int32)
    index, payload, wsum, count = recs
    payload = payload.cpu().numpy() if payload.dtype == torch.float32 else payload.view(torch.int16).cpu().numpy().view(np.uint16)
    return index.cpu().numpy(), payload, (None if wsum is None else wsum.cpu().numpy()), count.cpu().numpy()


def _check_snapshot_dtype(dtype):
    if dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f'dtype must be torch.float32 (the sums, every bit) or torch.bfloat16 (the mean), got {dtype!r}')


def _check_restore(model, snap, fading=None, what='model'):
    """A snapshot against the model that is to restore it (and, fading not None, against the kind of the batch): ValueError names the difference."""
    if not isinstance(snap, SceneSnapshot):
        raise TypeError(f'restore takes a SceneSnapshot, got {type(snap).__name__}')
    snap._validate()
    if tuple(model.n_voxels) != snap.grid or tuple(np.float32(model.voxel_size)) != tuple(np.float32(snap.voxel_size)):
        raise ValueError(f'restore: the {what} has grid {tuple(model.n_voxels)} with voxel size {tuple(model.voxel_size)}, the snapshot {snap.grid} with {snap.voxel_size}')
    if int(model.neck.out_channels) != snap.channels:
        raise ValueError(f'restore: the {what} lifts {int(model.neck.out_channels)} channels per voxel, the snapshot holds {snap.channels}')
    if getattr(model, 'sampling', 'nearest') != snap.sampling:
        raise ValueError(f"restore: the model samples by the {getattr(model, 'sampling', 'nearest')!r} rule, the snapshot was fused by the {snap.sampling!r} rule")
    if fading is not None and fading != (snap.kind == 'fading'):
        raise ValueError(f"restore: a {snap.kind} snapshot into a {'fading' if fading else 'plain'} batch (the kind must match; turning one into the other is out of scope)")


def _restored_meta(snap):
    """The scene meta a snapshot describes (without extrinsics: open_scene's form)."""
    from . import boxes
    meta = dict(lidar2img=dict(intrinsic=snap.intrinsic.copy(), origin=snap.origin.copy()))
    for k in ('img_shape', 'ori_shape', 'pad_shape'):
        if getattr(snap, k) is not None:
            meta[k] = getattr(snap, k)
    if snap.box_type is not None:
        if snap.box_type not in _BOX_TYPES:
            raise ValueError(f'restore: unknown box type {snap.box_type!r} (known: {_BOX_TYPES})')
        meta['box_type_3d'] = getattr(boxes, snap.box_type)
    return meta


def _adopt(rec, snap):
    """The record takes the host fields of a snapshot: extrinsics, view count, image size, scrolled, frame, origin and shapes; the mean is behind."""
    meta = _restored_meta(snap)
    rec.meta['lidar2img'] = dict(meta['lidar2img'], extrinsic=[e.copy() for e in snap.extrinsics])
    for k in ('img_shape', 'ori_shape', 'pad_shape', 'box_type_3d'):
        if k in meta:
            rec.meta[k] = meta[k]
    rec.n_views, rec._hw, rec._stale = snap.n_views, snap.hw, snap.n_views > 0
    rec._views, rec._next_id = [], snap.n_views
    rec._scrolled, rec._frame = snap.scrolled, snap.frame.copy()


# ------------------------------------------------------------------ the two model calls around the lift
def _trunk(m, img):
    """[V,3,H,W] -> FPN level 0 of these views.  The native handle's trunk sub-range is the same kernels with the same plans as
    features_2d_cl in one C call (equal bit for bit: tests/test_gpu_engine.py)."""
    nat = m._native
    if nat is not None and nat.cfg.with_trunk and img.shape[-2] % 32 == 0 and img.shape[-1] % 32 == 0:
        return nat.backbone_fpn(img)
    return m.features_2d_cl(img[None])


def _detect(m, vol, valid, metas):
    """The model's detection stage on mean rows vol [B,X,Y,Z,C] / valid bool [B,X,Y,Z]: one result dict per meta."""
    if isinstance(m.bbox_head, Anchor3DHead):
        boxes, scores, labels, count = m.detect_cl(vol, metas)
        return m._results_one_copy(boxes, scores, labels, count, metas)
    return [bbox3d2result(b, s, l) for b, s, l in m.detect_indoor_cl(vol, valid, metas)]


# ------------------------------------------------------------------ one scene on the host
class _SceneRecord:
    """The host state of one scene and every rule that needs no device.  meta: a complete simple_test meta of everything added; n_views;
    _views: the views of a windowed scene, oldest first, as (id, slot, extrinsic); _next_id: the id of the next arrival; _stale: the mean is
    behind the state; _hw: the image size of the views in the scene; _window, _decay, _forget, _gate (the depth gate, None: depths are refused) as opened.  No device buffers: a SceneSession
    adds its own, a SceneBatch keeps pools beside N of these."""

    def __init__(self, model, meta, window=None, decay=None, forget_below=0.0, depth_gate=None):
        decay, forget_below = self._check_fading(window, decay, forget_below)
        gate = None if depth_gate is None else ops.check_gate(depth_gate)
        if gate is not None and window is None and decay is None:
            raise ValueError('depth_gate needs a session that takes weights: open with decay=... (decay=1.0 fades nothing) or with window=W')
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
        self.meta, self.n_views, self._hw, self._stale = meta, 0, None, False
        self._window, self._views, self._next_id = window, [], 0
        self._decay, self._forget, self._gate = decay, forget_below, gate
        self._scrolled = (0, 0, 0)
        self._frame = np.eye(4)

    @staticmethod
    def _check_fading(window, decay, forget_below):
        """(decay, forget_below) as floats (decay None: a plain session); the rules that need no model."""
        if isinstance(forget_below, bool) or not isinstance(forget_below, (int, float, np.integer, np.floating)):
            raise TypeError(f'forget_below must be a number >= 0, got {forget_below!r}')
        forget_below = float(forget_below)
        if not (math.isfinite(forget_below) and forget_below >= 0):
            raise ValueError(f'forget_below must be finite and >= 0, got {forget_below}')
        if decay is None:
            if forget_below != 0:
                raise ValueError('forget_below needs a fading session: open with decay=... (decay=1.0 fades nothing)')
            return None, 0.0
        if window is not None:
            raise ValueError('decay together with window: the two are alternative ways to forget (a windowed scene takes weights, not a decay)')
        if isinstance(decay, bool) or not isinstance(decay, (int, float, np.integer, np.floating)):
            raise TypeError(f'decay must be None or a number in (0, 1], got {decay!r}')
        decay = float(decay)
        if not 0 < decay <= 1:
            raise ValueError(f'decay must be in (0, 1], got {decay}')
        return decay, forget_below

    def reset(self):
        """Forget every view."""
        self.meta['lidar2img']['extrinsic'] = []
        self.n_views, self._hw, self._stale = 0, None, False
        self._views, self._next_id = [], 0
        self._scrolled = (0, 0, 0)
        self._frame = np.eye(4)

    @property
    def frame(self):
        """float64 [4,4]: the product of every T warped by since the scene was opened or reset(), so that x_opening = frame @ x_grid -- a point named
        in the grid's current frame, in the frame the scene was opened in.  A copy."""
        return self._frame.copy()

    def _warped(self, T):
        """What a warp by T (float64 [4,4], x_old = T x_new) makes of the extrinsics this record holds -> (the meta's list, the windowed views):
        warped_extrinsic of each.  Changes nothing."""
        views = [(i, s, warped_extrinsic(e, T)) for i, s, e in self._views]
        return ([v[2] for v in views] if self._window is not None else [warped_extrinsic(e, T) for e in self.meta['lidar2img']['extrinsic']]), views

    def _warp(self, T, extrinsics, views):
        """A warp by T is in: the extrinsics (_warped) replace the record's, frame takes T on the right, the mean of a scene with views is behind."""
        self.meta['lidar2img']['extrinsic'], self._views = extrinsics, views
        self._frame = self._frame @ T
        self._stale = self._stale or self.n_views > 0

    def _merged(self, other, T):
        """A merge of the record `other` under T (x_other = T x_self) is in: the other's extrinsics, each by warped_extrinsic, count behind this
        scene's own, in the other's order; the view counts add; an empty scene takes the other's image size and the shapes its meta lacks; the
        mean is behind.  frame, origin and scrolled stay."""
        self.meta['lidar2img']['extrinsic'] = self.meta['lidar2img']['extrinsic'] + [warped_extrinsic(e, T) for e in other.meta['lidar2img']['extrinsic']]
        self.n_views += other.n_views
        if self._hw is None:
            self._hw = other._hw
        for k in ('img_shape', 'ori_shape', 'pad_shape'):
            if k not in self.meta and k in other.meta:
                self.meta[k] = other.meta[k]
        self._stale = True

    @property
    def scrolled(self):
        """The cumulative shift (sx, sy, sz) in voxels since the scene was opened or reset() (the origin stays where the scrolls took it)."""
        return self._scrolled

    def _scroll(self, s, origin):
        """A scroll by s is in: `origin` (scrolled_origin of this meta's) replaces the meta's, and the mean of a scene with views is behind."""
        self.meta['lidar2img']['origin'] = origin
        self._scrolled = tuple(a + b for a, b in zip(self._scrolled, s))
        self._stale = self._stale or self.n_views > 0

    def _scroll_to(self, center, voxel_size):
        """The shift that brings the grid's origin nearest to `center`: rint((center - origin) / voxel_size) per axis in float64, as ints."""
        c = np.asarray(center, np.float64).reshape(-1)
        if c.shape != (3,) or not np.isfinite(c).all():
            raise ValueError(f'center must be three finite coordinates, got {center!r}')
        return [int(v) for v in np.rint((c - np.asarray(self.meta['lidar2img']['origin'], np.float64)) / np.asarray(voxel_size, np.float64))]

    @property
    def view_ids(self):
        """The ids of the views in the scene, oldest first.  An id is the view's arrival ordinal since reset()."""
        if self._window is None:
            return list(range(self.n_views))
        return [v[0] for v in self._views]

    # ---- what a call may ask of this scene (each raises before anything changes)
    def _check_fits(self, V, of=''):
        """V views `of` this scene (' of scene 2'; '': the caller has one scene) in one call fit its window."""
        if self._window is not None and V > self._window:
            raise ValueError(f'{V} views{of} in one call do not fit a window of {self._window}')

    def _take_weights(self, weights, V, what):
        """_check_weights, and the refusal of a scene opened plain (what: 'session' / 'batch', as the caller was opened)."""
        weights = _check_weights(weights, V)
        if weights is not None and self._window is None and self._decay is None:
            raise ValueError(f'this {what} was opened plain and takes no weights: open it with decay=1.0 (weights, nothing fades) or with window=W')
        return weights

    def _take_maps(self, pixel_weights, depths, V, what):
        """_check_map of both pixel maps of an add, the refusal of a scene opened plain (in the wording of the weights' refusal) and of depths on
        a scene opened without depth_gate -> (pixel_weights, depths)."""
        maps = tuple(_check_map(t, name, V) for t, name in zip((pixel_weights, depths), MAP_FILL))
        if any(t is not None for t in maps) and self._window is None and self._decay is None:
            raise ValueError(f'this {what} was opened plain and takes no pixel maps: open it with decay=1.0 (weights, nothing fades) or with window=W')
        if maps[1] is not None and self._gate is None:
            raise ValueError(f'this {what} was opened without depth_gate and takes no depths: open it with depth_gate=(behind, front)')
        return maps

    def _check_shapes(self, shapes, have_views, where):
        """The img_shape / ori_shape / pad_shape of new frames (add_views_u8) against this meta's, once `where` ('scene' / 'batch') has views."""
        for k, v in shapes.items():
            if have_views and k in self.meta and tuple(self.meta[k]) != tuple(v):
                raise ValueError(f'{k} {tuple(v)} of these frames differs from the {tuple(self.meta[k])} of the views already in the {where}')

    def _slot_of(self, ids, where='the scene'):
        """{id: slot} of the views in a windowed scene; an id of `ids` that is not among them raises KeyError."""
        slot_of = {v[0]: v[1] for v in self._views}
        unknown = [i for i in ids if i not in slot_of]
        if unknown:
            raise KeyError(f'no view with id {unknown} in {where} (view_ids: {sorted(slot_of)})')
        return slot_of

    # ---- adding and removing views
    def _free_slots(self, V, base=0):
        """The slot rule of a windowed add of V views into the slots [base, base + W): (kept, slots) -- the newest W - V views stay, the
        leavers' slots are free for this call's views, and the free slots are handed out in order.  Changes nothing."""
        W = self._window
        kept = self._views[max(0, len(self._views) + V - W):]
        used = {v[1] for v in kept}
        return kept, [s for s in range(base, base + W) if s not in used][:V]

    def _admit(self, kept, slots, E, hw):
        """A windowed add is in: the views with extrinsics E sit in `slots` behind `kept` (_free_slots)."""
        self._views = kept + [(self._next_id + i, s, e) for i, (s, e) in enumerate(zip(slots, E))]
        self._next_id += len(E)
        self._hw, self._stale = hw, True
        self.meta['lidar2img']['extrinsic'] = [v[2] for v in self._views]
        self.n_views = len(self._views)

    def _grow(self, E, hw, stale):
        """An unbounded add is in: the views with extrinsics E count behind those in the scene; stale: the call stored no mean."""
        self._hw, self._stale = hw, stale
        self.meta['lidar2img']['extrinsic'] = self.meta['lidar2img']['extrinsic'] + E
        self.n_views += len(E)

    def remove_views(self, ids):
        """Drop the views with these ids (view_ids) from a windowed scene and free their slots; an unknown id raises KeyError and
        leaves the scene as it was."""
        if self._window is None:
            raise RuntimeError('remove_views needs a windowed session: open_scene(meta, window=W)')
        ids = [ids] if isinstance(ids, (int, np.integer)) else list(ids)
        self._slot_of(ids)
        drop = set(ids)
        if drop:
            self._views = [v for v in self._views if v[0] not in drop]
            self.meta['lidar2img']['extrinsic'] = [v[2] for v in self._views]
            self.n_views, self._stale = len(self._views), True
        return self

    def _reweight(self, ids, weights, wring, n_scenes, windowed, where):
        """The body of reweight on the caller's host weight ring (None: not started; n_scenes * W slots): the ring with the weights of these
        views changed, and the scene stale.  windowed / where: the caller's words for what it needs and where the ids were looked for."""
        if self._window is None:
            raise RuntimeError(f'reweight needs a windowed {windowed}')
        scalar = isinstance(ids, (int, np.integer))
        ids = [ids] if scalar else list(ids)
        weights = _check_weights([weights] if scalar and not hasattr(weights, '__len__') else weights, len(ids))
        slot_of = self._slot_of(ids, where)
        if ids:
            if wring is None:
                wring = [1.0] * (n_scenes * self._window)
            for i, w in zip(ids, weights):
                wring[slot_of[i]] = w
            self._stale = True
        return wring


class SceneSession(_SceneRecord):
    """model.open_scene(meta): meta as one entry of simple_test's img_metas without lidar2img['extrinsic'] -- the extrinsics come with
    the views.  img_shape / ori_shape (/ pad_shape) may be left out when the views come through add_views_u8, which fills them.
    window=None: the scene only grows (a running (sum, count) volume).  window=W >= 1: the scene holds the last W views at most and
    remove_views works; state: a feature ring [W,FH,FW,C] in the storage type and a projection ring [W,3,4] (allocated at the first
    add; W * FH * FW * C * sizeof(element) bytes: the module docstring has the ScanNet figures), the mean / mask buffers and the
    ordered host list of (view id, slot) -- no (sum, count) volume.
    decay=lam in (0, 1] (unbounded sessions only): a fading scene -- a weight sum [1,X,Y,Z] fp32 beside (sum, count); every add_views call is one
    tick: the state is multiplied by lam once, voxels whose weight sum falls below forget_below (>= 0) are forgotten, then the call's views are
    added with their weights.  Decided here, not lazily: a session opened without decay runs the plain path and refuses weights.
    depth_gate=(behind, front) (with decay= or window= only; two numbers >= 0, inf: no limit on that side): the gate of the depth maps that
    add_views(..., depths=) may bring, fixed here like decay; None: depth maps are refused.  Pixel maps (the module docstring) need no state on a
    fading session; a windowed one keeps a device ring [W,FH,FW] fp32 per kind of map from the first map it is given.
    The session is a _SceneRecord (the host state and its rules) with its own device buffers, camera uploads and launches."""

    def __init__(self, model, meta, window=None, decay=None, forget_below=0.0, depth_gate=None):
        super().__init__(model, meta, window, decay, forget_below, depth_gate)
        self._model, self._closed = model, False
        self._sum = self._count = self._mean = self._valid = self._origin = self._crop = None
        # window=W: the rings, and the host ring of the slots' weights, None until a weight is given.  decay=lam: a weight sum beside sum / count
        self._ring = self._pring = self._wring = self._wsum = None
        self._mring = self._dring = None          # window=W: the device rings of the slots' pixel-weight / depth maps [W,FH,FW], each None until a map is given
        self._covers = {}                         # add_views_u8(lens=): the cover maps [FH,FW] by (lens, source shape, pipeline shapes, device)
        self.last_admitted = None                 # the gate's verdict per view of the last add_views(..., min_novelty=) call; None after an ungated one
        self._twin = None                         # decay=lam: the (sum, wsum, count) buffers a warp writes into, None until the first warp

    # ------------------------------------------------------------------ state
    def _check_open(self):
        if self._closed:
            raise RuntimeError('this SceneSession is closed')

    def reset(self):
        """Forget every view; the buffers are kept and the next add starts them from zero."""
        self._check_open()
        super().reset()
        self._origin = self._crop = self._wring = self._mring = self._dring = None

    def close(self):
        self._sum = self._count = self._mean = self._valid = self._origin = self._crop = None
        self._ring = self._pring = self._wsum = self._wring = self._mring = self._dring = self._twin = None
        self._covers = {}
        self._closed = True

    # ------------------------------------------------------------------ adding views
    def _features(self, img):
        return _trunk(self._model, img)

    def add_views(self, img, extrinsics, emit=True, weights=None, pixel_weights=None, depths=None, min_novelty=None, fresh_below=None):
        """img [V,3,H,W] float32 on the device (normalised and padded as for simple_test), extrinsics: V float32 4x4 matrices.
        min_novelty in (0, 1] (None: no gate, the code as it was): a keyframe gate.  Each view of the call is tested by coverage() against the
        state BEFORE the call -- the views of one call do not see each other -- and is admitted iff seen > 0 and fresh / seen >= min_novelty
        (Python floats; fresh_below as for coverage(), only together with min_novelty).  Rejected views are dropped before the trunk runs, with
        their images, extrinsics, weights and maps; if none is admitted nothing is launched after the count and nothing changes (no tick on a
        fading session).  last_admitted holds the verdicts, one bool per view of the call (None after an ungated call).
        emit=False skips the store of the mean volume (detect() / volume() then compute it once from the sums): for callers that add
        many chunks between two detections.  Views count in the order they are added.  On a windowed session (window=W) the views go
        into free slots of the ring, the oldest views leaving first when the window is full; more than W views in one call raise
        ValueError; emit has no effect (the lift runs when volume() / detect() is asked and the set has changed).
        weights: one finite float >= 0 per view (None: 1; 0: the view does not count), on a session opened with decay= or window=.  On a fading
        session every call is one tick: the state fades once by `decay`, then these views are added with their weights.
        pixel_weights, depths (sessions that take weights; depths need depth_gate= at open): one float32 tensor each, host or device, [V,FH,FW] at
        the resolution of the features or [V,H,W] at the size of img, which is reduced by the exact strided pick map[:, ::s, ::s], s = H // FH
        (pick_map); other shapes raise ValueError.  A view's weight at a voxel is its weight times the confidence of the pixel the voxel
        projects to; a pixel with a measured depth D lets the view count only at voxels of depth D - front .. D + behind (the module docstring,
        "Pixel maps")."""
        return self._add_views(img, extrinsics, emit, {}, weights, (pixel_weights, depths), gate=_check_novelty(min_novelty, fresh_below))

    def _add_views(self, img, extrinsics, emit, shapes, weights=None, maps=(None, None), strided=True, gate=(None, 1.0), verdict=None):
        """add_views with the img_shape / ori_shape / pad_shape of these views (add_views_u8); the session changes only when the
        views are in: a call that raises leaves meta, state and n_views as they were.  gate = (min_novelty, fresh_below) as _check_novelty
        returns them; verdict: the gate has run already (add_views_u8, before its pipeline), these views are the ones it admitted and this is
        what last_admitted becomes."""
        self._check_open()
        V, H, W = _check_images(img, 'V')
        E = _check_extrinsics(extrinsics, V)
        self._check_fits(V)
        weights = self._take_weights(weights, V, 'session')
        maps = self._take_maps(*maps, V, 'session')
        _check_size((H, W), self._hw, 'scene')
        meta = dict(self.meta, **shapes)
        if 'img_shape' not in meta or 'ori_shape' not in meta:
            raise ValueError('the scene meta needs img_shape and ori_shape (add_views_u8 fills them from its frames)')
        if not img.is_cuda:
            raise RuntimeError('img must be a device (HIP) tensor; the MI355X path has no CPU fallback')
        m = self._model
        if gate[0] is not None:                   # the keyframe gate: against the state before the call, before the trunk
            verdict = admitted(self._coverage(E, maps, (H, W), meta, gate[1], strided, img.device), gate[0])
            if not any(verdict):
                self.last_admitted = verdict
                return self
            if not all(verdict):
                img, E, weights, maps = _kept(verdict, img), _kept(verdict, E), _kept(verdict, weights), tuple(_kept(verdict, t) for t in maps)
        if m._prepared_device is None:
            m.prepare(img.device)
        p0 = self._features(img.contiguous())
        maps = _maps_at(maps, (H, W), p0, strided)     # (a map of the wrong size raises here: the session has not changed yet)
        view_meta = dict(meta, lidar2img=dict(meta['lidar2img'], extrinsic=E))
        if self._origin is None:                  # new_origin and the crop do not depend on the views: uploaded once per scene
            proj, origin, crop = m._camera_setup([view_meta], 4, p0.device)
        else:
            proj, origin, crop = m._compute_projection(view_meta, 4)[None].contiguous().to(p0.device), self._origin, self._crop
        if self._window is not None:
            self._add_windowed(p0, proj, E, (H, W), weights, maps)
        else:
            self._add_unbounded(p0, proj, origin, crop, E, (H, W), weights, emit, maps)
        self._origin, self._crop = origin, crop
        self.meta.update(shapes)
        self.last_admitted = verdict
        return self

    # ------------------------------------------------------------------ view coverage
    def coverage(self, extrinsics, pixel_weights=None, depths=None, fresh_below=None):
        """What would these K candidate views add?  extrinsics: K float32 4x4 matrices -> np.ndarray [K,2] int64, columns (seen, fresh): the
        number of voxels of the scene's grid the lift would count the view at, and how many of those hold less than fresh_below of evidence
        (None: 1.0, less than one full-weight view's worth).  One small launch and one device-to-host read, no trunk, no image
        (ops.view_coverage, ivx_view_coverage_fwd): the decision is the lift's own, bit for bit, at the scene's origin and crop, by the model's
        projection rule.  The evidence is the view count of a plain session, the weight sum of a fading one and the valid mask of a windowed
        one (a kept view of weight 0 leaves its voxels fresh); an empty scene has none, so fresh == seen.  A fading session's state is read as
        it is stored: the fade of its next tick is not anticipated.  A stale windowed scene refreshes first, with its one gathered lift -- the
        only thing the call may change; views, state and meta stay as they are.
        pixel_weights, depths: as for add_views ([K,FH,FW], or [K,H,W] at the input size through pick_map), accepted on every kind of
        session because nothing is fused; depths need depth_gate= at open.  The feature-map size is the scene's image size // 4, before the
        first view the meta's pad_shape // 4 (ValueError without one); the meta needs img_shape and ori_shape as in add_views."""
        self._check_open()
        extrinsics = list(extrinsics)
        E = _check_extrinsics(extrinsics, len(extrinsics))
        if not E:
            raise ValueError('coverage needs at least one candidate view')
        maps = tuple(_check_map(t, name, len(E)) for t, name in zip((pixel_weights, depths), MAP_FILL))
        if maps[1] is not None and self._gate is None:
            raise ValueError('this session was opened without depth_gate and takes no depths: open it with depth_gate=(behind, front)')
        if 'img_shape' not in self.meta or 'ori_shape' not in self.meta:
            raise ValueError('the scene meta needs img_shape and ori_shape (add_views_u8 fills them from its frames)')
        return self._coverage(E, maps, self._hw, self.meta, _check_novelty(None, fresh_below, alone=True)[1])

    def _coverage(self, E, maps, hw, meta, fresh_below, strided=True, dev=None):
        """coverage() of checked arguments on the meta of the call (add_views_u8 brings shapes the scene's meta does not have yet); hw: the
        padded image size, None: from the meta."""
        m = self._model
        hw, fhw = _coverage_fhw(hw, meta)
        dev = _scene_device(m, self._origin, self._count, self._valid) if dev is None else dev
        view_meta = dict(meta, lidar2img=dict(meta['lidar2img'], extrinsic=E))
        if self._origin is None:
            proj, origin, crop = m._camera_setup([view_meta], 4, dev)
            proj = proj[0]
        else:
            proj, origin, crop = m._compute_projection(view_meta, 4).contiguous().to(dev), self._origin, self._crop
        pw, dp = (None if t is None else pick_map(t, name, hw, fhw, strided).to(dev).contiguous() for t, name in zip(maps, MAP_FILL))
        state = None
        if self.n_views and self._window is not None:     # the evidence: the mask of the kept views (refreshed when stale) ...
            self.volume()
            state = self._valid
        elif self.n_views:                                # ... or the weight sum / the view count of the running state
            state = self._wsum if self._decay is not None else self._count
        n = ops.MAX_COVERAGE_VIEWS
        out = [ops.view_coverage(proj[k:k + n].contiguous(), [list(range(min(n, len(E) - k)))], [0], origin, crop, m.voxel_size, m.n_voxels, fhw, state, fresh_below,
                                 None if pw is None else pw[k:k + n], None if dp is None else dp[k:k + n], self._gate)[0] for k in range(0, len(E), n)]
        return (out[0] if len(out) == 1 else torch.cat(out)).cpu().numpy().astype(np.int64)

    def _add_unbounded(self, p0, proj, origin, crop, E, hw, weights, emit, maps=(None, None)):
        """The new views' maps p0 [V,1,FH,FW,C] added to the running (sum, count) state in one launch: the plain lift, or one tick of the
        weighted one on a fading session -- with the call's pixel maps [V,FH,FW], which are consumed here and not kept (no map: the weighted
        launch as it was)."""
        m = self._model
        if self._sum is None:                     # the state, allocated once: sum fp32, count, mean in the storage type, valid
            X, Y, Z = m.n_voxels
            Cn, dev = p0.shape[-1], p0.device
            self._sum = torch.empty((1, X, Y, Z, Cn), device=dev, dtype=torch.float32)
            self._count = torch.empty((1, X, Y, Z), device=dev, dtype=torch.int32)
            self._mean = torch.empty((1, X, Y, Z, Cn), device=dev, dtype=p0.dtype)
            self._valid = torch.empty((1, X, Y, Z), device=dev, dtype=torch.uint8)
            self._wsum = torch.empty((1, X, Y, Z), device=dev, dtype=torch.float32) if self._decay is not None else None
        if self._decay is not None:                # one tick: fade once, then this call's views with their weights (the call's maps are the pool)
            form, kw = _lift_maps(*maps, self._gate)
            getattr(ops, f'backproject_{form}_accum_')(p0, proj[0], [list(range(len(E)))], weights, [0], [self.n_views == 0], [self._decay], origin, crop,
                                                       m.voxel_size, self._sum, self._wsum, self._count, self._mean if emit else None,
                                                       self._valid if emit else None, forget_below=self._forget,
                                                       sampling=getattr(m, 'sampling', 'nearest'), **kw)
        else:
            ops.backproject_accum_(p0, proj, origin, crop, m.voxel_size, self._sum, self._count, self.n_views == 0,
                                   self._mean if emit else None, self._valid if emit else None, sampling=getattr(m, 'sampling', 'nearest'))
        self._grow(E, hw, stale=not emit)

    def _add_windowed(self, p0, proj, E, hw, weights, maps=(None, None)):
        """The new views' maps p0 [V,1,FH,FW,C] and projection rows proj [1,V,3,4] into free slots of the rings, their pixel maps into the same
        slots of the map rings; the oldest views leave first when the window is full.  Everything that can fail comes before the first
        change of the session."""
        m, W = self._model, self._window
        X, Y, Z = m.n_voxels
        Cn, dev = p0.shape[-1], p0.device
        ring, pring, mean, valid = self._ring, self._pring, self._mean, self._valid
        if ring is None or tuple(ring.shape[1:]) != tuple(p0.shape[1:]) or ring.dtype != p0.dtype:     # first add (or another size after reset())
            ring = torch.empty((W,) + tuple(p0.shape[1:]), device=dev, dtype=p0.dtype)
            pring = torch.empty((W, 3, 4), device=dev, dtype=torch.float32)
            mean = torch.empty((1, X, Y, Z, Cn), device=dev, dtype=p0.dtype)
            valid = torch.empty((1, X, Y, Z), device=dev, dtype=torch.uint8)
        kept, slots = self._free_slots(len(E))
        for i, s in enumerate(slots):
            ring[s].copy_(p0[i])
            pring[s].copy_(proj[0, i])
        self._wring = _ring_weights(self._wring, W, slots, weights)
        self._mring = _ring_map(self._mring, W, p0.shape[-3:-1], dev, slots, maps[0], MAP_FILL['pixel_weights'])
        self._dring = _ring_map(self._dring, W, p0.shape[-3:-1], dev, slots, maps[1], MAP_FILL['depths'])
        self._ring, self._pring, self._mean, self._valid = ring, pring, mean, valid
        self._admit(kept, slots, E, hw)

    def remove_views(self, ids):
        """Drop the views with these ids (view_ids) from a windowed scene and free their slots; an unknown id raises KeyError and
        leaves the scene as it was."""
        self._check_open()
        return super().remove_views(ids)

    def reweight(self, ids, weights):
        """Change the weights of views that are in a windowed scene (ids: view_ids; one finite float >= 0 per id; 0 takes the view out of the
        mean without freeing its slot) and mark the scene stale: the next volume() / detect() lifts the kept views again with the new weights.
        An unknown id raises KeyError and leaves the scene as it was."""
        self._check_open()
        self._wring = self._reweight(ids, weights, self._wring, 1, 'session: open_scene(meta, window=W)', 'the scene')
        return self

    # ------------------------------------------------------------------ scrolling
    def scroll(self, voxels):
        """Move the grid by voxels = (sx, sy, sz) whole voxels: what was at index i + s is afterwards at index i, voxels that enter the grid are
        unseen, and meta['lidar2img']['origin'] becomes scrolled_origin(origin, voxels, voxel_size), a float32 array, from which the device
        new_origin follows by the model's own rule -- so detect() returns boxes in world coordinates through the unchanged head code.
        After scroll the session behaves exactly like a session opened at the new origin whose state is the moved state: every later add is the
        existing lift at that origin.  Plain and fading sessions move (sum, count[, weight sum]) in place in one ops.volume_scroll_ (a pure move
        of bits; a scroll is not a tick, nothing fades) and recompute the mean when it is next asked for.  A windowed session has no state to
        move: its next volume() / detect() is the gathered re-lift of the kept views at the new origin, bit for bit their one-shot lift there.
        An empty scene only changes its origin.  A zero shift changes nothing.  A model with an Anchor3DHead raises NotImplementedError.  A call
        that raises leaves the session as it was.  Returns self."""
        self._check_open()
        s = _check_scroll(self._model, voxels)
        if not any(s):
            return self
        m = self._model
        origin = scrolled_origin(self.meta['lidar2img']['origin'], s, m.voxel_size)
        new_origin = m._new_origin(origin)[None].contiguous().to(self._origin.device) if self._origin is not None else None
        if self._window is None and self.n_views:
            ops.volume_scroll_(self._sum, self._count, [0], [s], self._wsum)
        self._origin = new_origin
        self._scroll(s, origin)
        return self

    def scroll_to(self, center):
        """Host-only convenience: scroll by rint((center - origin) / voxel_size) per axis (computed in float64), so that the grid's origin comes as
        near to `center` as whole voxels allow.  Applies the shift when it is non-zero and returns it as (sx, sy, sz)."""
        self._check_open()
        s = self._scroll_to(center, self._model.voxel_size)
        if any(s):
            self.scroll(s)
        return tuple(s)

    # ------------------------------------------------------------------ warping
    def warp(self, T):
        """Bring the scene into a frame that has turned and moved: T is a host float 4x4 with x_old = T x_new -- for a vehicle
        inv(world_from_old_ego) @ world_from_new_ego.  The grid stays where the head expects it: origin, anchors and head code are untouched, so
        models with an Anchor3DHead warp like any other.  After a warp the caller's extrinsics and the returned boxes are in the grid's current
        frame; every extrinsic the session holds follows warped_extrinsic, so `meta` stays a complete simple_test meta in the new frame, and
        `frame` accumulates T.
        A fading session (decay=) resamples its state (sum, weight sum, count) in one ops.volume_warp (ivx_volume_warp_fwd) into a twin state and
        swaps the two; the session's forget_below is passed through, nothing fades (a warp is not a tick) and the mean is recomputed when next
        asked for.  The twin is allocated at the first warp and kept: a session that warps holds its state twice (ScanNet-fast 2 x 26.4 MB,
        ScanNet-v1 2 x 54.1 MB).  A windowed session has no state to resample: its kept views are re-posed and the next volume() / detect() is the
        gathered re-lift, bit for bit a fresh windowed scene given the same views with the warped extrinsics; maps and weights stay in their
        slots.  A plain session raises NotImplementedError and goes on as before.  An empty scene only changes `frame`.  The identity changes
        nothing and launches nothing.  A call that raises leaves the session as it was.  Returns self."""
        self._check_open()
        T = _check_warp(T)
        if self._window is None and self._decay is None:
            raise NotImplementedError(_PLAIN_WARP.format(what='session'))
        if np.array_equal(T, np.eye(4)):
            return self
        m = self._model
        extrinsics, views = self._warped(T)
        if self.n_views and self._window is not None:     # the kept views' projection rows, by the rule their add used; the rings keep their slots
            idx = torch.tensor([v[1] for v in views], dtype=torch.int64).to(self._pring.device)
            rows = m._compute_projection(dict(self.meta, lidar2img=dict(self.meta['lidar2img'], extrinsic=extrinsics)), 4).contiguous().to(self._pring.device)
            self._pring.index_copy_(0, idx, rows)
        elif self.n_views:
            state = (self._sum, self._wsum, self._count)
            twin = self._twin if self._twin is not None else tuple(torch.empty_like(t) for t in state)
            ops.volume_warp(*state, [0], [T], m._new_origin(self.meta['lidar2img']['origin']).numpy()[None], m.voxel_size, out=twin, forget_below=self._forget)
            (self._sum, self._wsum, self._count), self._twin = twin, state
        self._warp(T, extrinsics, views)
        return self

    # ------------------------------------------------------------------ merging
    def merge(self, other, T=None, weight=1.0):
        """Add the fused state of another session to this one's: T is a host float 4x4 with x_other = T x_self -- it takes a point of this scene's
        grid frame to the other's (two robots that fused the same rooms, a relocalisation against an earlier map).  T=None: the two scenes were
        opened in one common frame, and T = inv(other.frame) @ self.frame in float64.  weight > 0 scales the other's evidence (alpha).
        Both sessions must be fading (decay=; decay=1.0 fades nothing), open, on one device and of the same prepared model.  ONE
        ops.volume_merge_ (ivx_volume_merge_fwd) reads the other's (sum, weight sum, count) trilinearly at T x and adds it in place where the other
        holds evidence; each scene's grid keeps its own origin (a scrolled scene's differs), this session's forget_below applies to the merged
        voxels, and nothing fades: a merge is not a tick.  The host record follows: meta['lidar2img']['extrinsic'] grows by
        warped_extrinsic(E, T) of the other's extrinsics, in the other's order after this scene's own, n_views adds, and the mean is recomputed
        when next asked for; frame, origin and scrolled stay.  `other` is unchanged and stays usable.  An empty `other` changes nothing and
        launches nothing; an empty `self` starts its state from zero as its first add would, on the other's device, and takes the other's image
        size; when both hold views their image sizes must agree.
        Evidence that both scenes hold of the same views counts twice: the merge adds states and cannot know which views they share.
        A plain session on either side raises NotImplementedError (open it with decay=1.0), so does a windowed one; `other is self` raises
        ValueError.  A call that raises leaves both scenes as they were.  Returns self."""
        self._check_open()
        if not isinstance(other, SceneSession):
            raise TypeError(f'merge takes another SceneSession, got {type(other).__name__}')
        other._check_open()
        if other is self:
            raise ValueError('merge: other is self (a scene cannot be added to itself: the kernel reads its source while it writes)')
        _check_merge_kind(self._window if self._window is not None else other._window, self._decay is not None and other._decay is not None, 'session')
        if other._model is not self._model:
            raise ValueError('merge: the two sessions must be of the same prepared model')
        T = _merge_transform(self, other, T)
        weight = _check_merge_weight(weight)
        if self.n_views and other.n_views:
            _check_size(other._hw, self._hw, 'scene')
            if other._sum.device != self._sum.device:
                raise ValueError(f'merge: the two scenes must be on one device, got {self._sum.device} and {other._sum.device}')
        if other.n_views == 0:
            return self
        m = self._model
        mine, fresh = (self._sum, self._wsum, self._count, self._mean, self._valid), False
        if self.n_views == 0:                     # the state as the first add would start it: from zero, on the other's device
            theirs = (other._sum, other._wsum, other._count, other._mean, other._valid)
            fits = self._sum is not None and all(a.shape == b.shape and a.dtype == b.dtype and a.device == b.device for a, b in zip(mine, theirs))
            mine = tuple(t.zero_() for t in mine) if fits else tuple(torch.zeros_like(t) for t in theirs)
            fresh = not fits
        ops.volume_merge_(*mine[:3], [0], (other._sum, other._wsum, other._count), [0], [T], m._new_origin(self.meta['lidar2img']['origin']).numpy()[None],
                          m._new_origin(other.meta['lidar2img']['origin']).numpy()[None], m.voxel_size, alpha=weight, forget_below=self._forget)
        self._sum, self._wsum, self._count, self._mean, self._valid = mine
        if fresh:                                 # new buffers, perhaps on another device: what belonged to the old ones goes (each is made again when next needed)
            self._twin = self._origin = self._crop = None
        self._merged(other, T)
        return self

    # ------------------------------------------------------------------ matching
    def _check_match(self, other, op):
        """The refusals of match / register against another session: both open, fading, of one prepared model, holding views, on one device and of
        one grid and channel count."""
        self._check_open()
        if not isinstance(other, SceneSession):
            raise TypeError(f'{op} takes another SceneSession, got {type(other).__name__}')
        other._check_open()
        _check_match_kind(self._window if self._window is not None else other._window, self._decay is not None and other._decay is not None, 'session', op)
        if other._model is not self._model:
            raise ValueError(f'{op}: the two sessions must be of the same prepared model')
        if self.n_views == 0 or other.n_views == 0:
            raise ValueError(f'{op}: {"this" if self.n_views == 0 else "the other"} scene is empty (it holds no views, so there is no state to compare)')
        if other._sum.device != self._sum.device:
            raise ValueError(f'{op}: the two scenes must be on one device, got {self._sum.device} and {other._sum.device}')
        if other._sum.shape != self._sum.shape:
            raise ValueError(f'{op}: the two scenes must have one grid and channel count, got {tuple(self._sum.shape[1:])} and {tuple(other._sum.shape[1:])}')

    def _match(self, other, Ts, step, min_overlap):
        m = self._model
        pairs, own, stats = ops.volume_match(self._sum, self._wsum, [0], (other._sum, other._wsum), [0], [Ts],
                                             m._new_origin(self.meta['lidar2img']['origin']).numpy()[None],
                                             m._new_origin(other.meta['lidar2img']['origin']).numpy()[None], m.voxel_size, step)
        return _match_results(pairs, own, stats, [Ts], min_overlap)[0]

    def match(self, other, Ts=None, step=1, min_overlap=0.3):
        """How well does this scene agree with another under candidate transforms?  Ts: a host list of K float 4x4 with x_other = T x_self, the
        merge's convention (None: the one candidate a merge would default to, inv(other.frame) @ self.frame).  ONE ops.volume_match
        (ivx_volume_match_fwd) visits this scene's voxels, reads the other's state trilinearly at T x -- each scene's grid keeps its own origin, so
        scrolled scenes match -- and sums, over the voxels both hold evidence for, the correlation of the two mean feature fields; the score of a
        candidate is ncc = dot / sqrt(na * nb) and its overlap pairs / own.  step: the lattice step, one integer or (px, py, pz): only every
        step-th voxel per axis is visited (a coarse look).  A candidate is eligible iff pairs > 0 and overlap >= min_overlap.
        Both sessions must be fading (decay=; decay=1.0 fades nothing), open, hold views, be on one device and of the same prepared model; both are
        left bit-unchanged, records included.  A plain session on either side raises NotImplementedError, so does a windowed one; an empty scene
        raises ValueError.  -> MatchResult (host arrays: score, overlap, pairs, own, stats, best, T)."""
        self._check_match(other, 'match')
        Ts = _match_candidates(self, other, Ts)
        return self._match(other, Ts, ops._match_step(step), _check_min_overlap(min_overlap))

    def _align(self, other, Ts, step):
        m = self._model
        about = np.asarray(self.meta['lidar2img']['origin'], np.float64)
        outs = ops.volume_align(self._sum, self._wsum, [0] * len(Ts), (other._sum, other._wsum), [0] * len(Ts), [[T] for T in Ts], about,
                                m._new_origin(self.meta['lidar2img']['origin']).numpy(), m._new_origin(other.meta['lidar2img']['origin']).numpy(),
                                m.voxel_size, step)
        return _align_host(outs, len(Ts))

    def refine(self, other, T0=None, iters=12, dof=ALIGN_DOF, step=1, min_overlap=0.3, damping=1e-3, tol_shift=None, tol_rot=1e-5):
        """Refine a transform between this scene and another (x_other = T x_self) in all six degrees of freedom by a direct method: each
        evaluation is ONE ops.volume_align (ivx_volume_align_fwd), which returns the cost e = sum |b - a|^2 of the two mean feature fields over
        the used voxels with its Gauss-Newton normal equations, and the host takes a Levenberg-Marquardt step
        T <- T @ rigid_increment(delta, about), (H + damping diag H) delta = -g, with `about` the grid's centre (the point register turns about).
        This is a LOCAL method: its basin is about a voxel and a few degrees on real features, because the gradient is that of a trilinear read.
        For anything wider run register with coarse levels first, then refine (or register(..., refine=True)).
        T0: the start (None: inv(other.frame) @ self.frame).  iters: the evaluations it may spend.  dof: the degrees of freedom that move, names
        out of ('x', 'y', 'z', 'rx', 'ry', 'rz').  step: the lattice step.  A pose is eligible iff used > 0 and used / own >= min_overlap; a
        trial is accepted iff it is eligible and its cost e / (used * C) is strictly lower; accepted steps divide the damping by 10, rejected
        ones multiply it by 10.  It stops after `iters` evaluations, on a step below tol_shift (metres; None: 1e-3 of the smallest voxel edge)
        and tol_rot (radians), on a damping above 1e6 or on a solve that is not finite.  A T0 that is not eligible comes back as it is with
        ok False: no exception.  Each evaluation reads 31 doubles and three counts back.  Refusals are match's.  Both scenes are unchanged.
        -> (T float64 [4,4], AlignResult at T)."""
        self._check_match(other, 'refine')
        T0 = _merge_transform(self, other, T0)
        args = _check_refine(iters, dof, min_overlap, damping, tol_shift, tol_rot, self._model.voxel_size)
        step = ops._match_step(step)
        about = np.asarray(self.meta['lidar2img']['origin'], np.float64)
        return _refine(lambda idx, Ts: self._align(other, Ts, step), [T0], [about], int(self._sum.shape[-1]), *args)[0]

    def register(self, other, T0=None, yaw=math.radians(8), shift=None, levels=6, step=1, min_overlap=0.3, refine=False, dof=None):
        """Refine a transform between this scene and another (x_other = T x_self) by a coarse-to-fine search over yaw and translation, built on
        match.  This is a LOCAL search around T0 (None: inv(other.frame) @ self.frame): it finds the best pose within about twice the first
        level's offsets of T0 and does not look further.  Each of `levels` levels scores the 81 candidates pose_candidates(T_c, yaw, shift,
        about=the grid's centre) -- T_c @ rigid(yaw=a, t=(x, y, z)) with each offset in {-h, 0, +h} -- in one match, moves T_c to the best eligible
        candidate (keeps it when none is eligible), then halves yaw and shift.  shift (h_x, h_y, h_z) in metres defaults to (2 vs_x, 2 vs_y,
        vs_z); yaw is in radians.  step: one integer for every level or a list of one lattice step per level (a coarse level may pass 2).
        Pitch and roll are not searched.  Refusals are match's.  Both scenes are unchanged.
        refine=True then runs refine (its defaults, the same min_overlap, the last level's lattice step) from the last level's pose over
        dof = ('x', 'y', 'z', 'rz') -- the degrees the lattice searches -- unless a `dof` is given, and returns refine's answer with the last
        level's MatchResult as its .match; the default changes nothing, launch for launch.
        -> (T float64 [4,4], the MatchResult of the last level);  refine=True: (T float64 [4,4], AlignResult)."""
        self._check_match(other, 'register')
        T0 = _merge_transform(self, other, T0)
        min_overlap = _check_min_overlap(min_overlap)
        dof = _check_register_refine(refine, dof)
        T, res = _register(lambda Ts, p: self._match(other, Ts, p, min_overlap), T0, yaw, shift, levels, step, min_overlap,
                           np.asarray(self.meta['lidar2img']['origin'], np.float64), self._model.voxel_size)
        if not refine:
            return T, res
        T, out = self.refine(other, T, dof=dof, step=_last_step(step), min_overlap=min_overlap)
        out.match = res
        return T, out

    # ------------------------------------------------------------------ snapshots
    def snapshot(self, dtype=torch.float32):
        """The scene as host data (SceneSnapshot): ONE ops.volume_pack (ivx_volume_pack_fwd) compacts the voxels that hold evidence, in ascending
        voxel order, and only those n records are copied to the host, beside the scene's host record.  dtype=torch.float32 keeps every bit of the
        state: model.restore_scene(snapshot) holds the (sum, weight sum, count) this session holds, bit for bit.  dtype=torch.bfloat16 keeps the
        mean in bf16 instead of the sums (half the payload; count and weight sum stay exact, restored sums lie within (2^-8 + 2^-22) |S|).  Plain
        and fading sessions; the session is unchanged.  An empty scene gives a snapshot with no records and launches nothing.  A windowed session
        raises NotImplementedError (its state is the feature ring: out of scope), a closed one RuntimeError."""
        self._check_open()
        _check_snapshot_dtype(dtype)
        if self._window is not None:
            raise NotImplementedError(_WINDOW_SNAPSHOT.format(what='session'))
        m = self._model
        if self.n_views == 0:
            Cn = int(m.neck.out_channels)         # (the channels of FPN level 0: what the state of this model's scenes holds per voxel)
            return _snapshot_of(self, m, _host_records(None, Cn, dtype, self._decay is not None), Cn)
        recs = ops.volume_pack(self._sum, self._count, [0], self._wsum, dtype)[0]
        return _snapshot_of(self, m, _host_records(recs, int(self._sum.shape[-1]), dtype, self._decay is not None), int(self._sum.shape[-1]))

    def _restore(self, snap, device):
        """This freshly opened session takes the state and the host fields of a checked snapshot (model.restore_scene)."""
        m = self._model
        if snap.n_views:
            X, Y, Z = m.n_voxels
            Cn, dev = snap.channels, torch.device(device) if device is not None else _scene_device(m)
            store = m.storage_dtype if m.storage_dtype in (torch.float32, torch.bfloat16) else torch.float32
            state = (torch.empty((1, X, Y, Z, Cn), device=dev, dtype=torch.float32), torch.empty((1, X, Y, Z), device=dev, dtype=torch.int32),
                     torch.empty((1, X, Y, Z), device=dev, dtype=torch.float32) if self._decay is not None else None)
            with torch.cuda.device(dev):
                ops.volume_unpack_(state[0], state[1], [0], [snap.records()], state[2])
            self._sum, self._count, self._wsum = state
            self._mean = torch.empty((1, X, Y, Z, Cn), device=dev, dtype=store)
            self._valid = torch.empty((1, X, Y, Z), device=dev, dtype=torch.uint8)
        _adopt(self, snap)
        return self

    def add_views_u8(self, frames, extrinsics, img_scale, emit=True, weights=None, pixel_weights=None, depths=None, min_novelty=None, fresh_below=None,
                     lens=None, depth_frames=None, depth_scale=0.001, format=None, **pipeline_kw):
        """add_views from uint8 camera frames ((H,W,3) BGR arrays / tensors, or one [V,H,W,3]): the test pipeline runs on the device
        (data.prepare_images_device; pipeline_kw: img_norm_cfg, size_divisor, keep_ratio, device) and fills img_shape / ori_shape /
        pad_shape of the scene meta.  Later frames must come out at the same shapes.  weights as for add_views; pixel_weights and depths at
        feature resolution [V,FH,FW] only (the frames are resized on the device; confidence maps at the source size are out of scope).  min_novelty /
        fresh_below as for add_views: once the scene knows its shapes (it has had views) the gate runs before the pipeline, so a rejected
        frame is not even resized; on the first call it runs after the pipeline, which is what tells the shapes.
        lens: a data.Lens for every frame of the call, or one entry (a Lens or None) per frame (a rig): the frames of a real camera are
        undistorted in the pipeline's own launch (ops.image_prep_lens_u8, one interpolation), and the scene meta's intrinsic must describe the
        lens's new_K (ValueError when it is not the identity and differs by more than 1e-6 relative).  On a session that takes maps (decay= or
        window=) the cover map of the lens -- 1 where an input pixel shows the frame, 0 on the black border after undistortion -- becomes
        part of each view's confidence: pixel_weights * cover, or the cover alone.  It depends on (lens, source shape, pipeline shapes)
        only, is computed once by ops.map_prep_lens and cached on the scene; the gate sees it too, so coverage still equals the lift's
        mask.  A plain session takes the undistorted image and, refusing maps as before, no mask: border pixels then enter as the mean
        colour (zeros after normalisation).
        depth_frames: [V,H,W] uint16 or float32 at the SOURCE size, host or device (a depth camera registered to the colour frame), in
        units of depth_scale metres (0.001: millimetres); needs depth_gate= at open and excludes depths=.  They are taken to feature
        resolution through the same geometry (ops.map_prep_lens with the frame's lens, or with none: the nearest source pixel of each
        feature pixel, 0 -- no measurement -- on the border).  Frames that come with a lens or with depth frames must share one source size
        in a call.  A scene that never passes lens or depth_frames calls what it called before.
        format: the pixel format of the frames (a data.FrameFormat or layout name for all, or one per frame; data.prepare_images_device):
        decoder frames -- NV12, YUYV, BGRA ... -- are converted inside the pipeline's launch, with or without a lens, and the scene is the
        one the converted BGR frames give, bit for bit.  depth_frames, the cover map and the gate depend on geometry only."""
        from .data import prepare_images_device, FrameFormat
        self._check_open()
        frames = list(frames)
        E = _check_extrinsics(extrinsics, len(frames))
        self._check_fits(len(frames))
        weights = self._take_weights(weights, len(frames), 'session')
        maps = self._take_maps(pixel_weights, depths, len(frames), 'session')
        if lens is not None or depth_frames is not None:
            lens, maps = _lens_maps([self], self._covers, frames, maps, lens, depth_frames, depth_scale, img_scale, pipeline_kw, 'session', format)
        gate, verdict = _check_novelty(min_novelty, fresh_below), None
        if gate[0] is not None and self._hw is not None and 'img_shape' in self.meta and 'ori_shape' in self.meta:
            verdict = admitted(self._coverage(E, maps, self._hw, self.meta, gate[1], strided=False), gate[0])
            if not any(verdict):
                self.last_admitted = verdict
                return self
            frames, E, weights, maps = _kept(verdict, frames), _kept(verdict, E), _kept(verdict, weights), tuple(_kept(verdict, t) for t in maps)
            gate, lens = (None, gate[1]), _kept(verdict, lens)
            format = format if format is None or isinstance(format, (str, FrameFormat)) else _kept(verdict, list(format))
        if lens is not None:
            pipeline_kw = dict(pipeline_kw, lens=lens)
        if format is not None:
            pipeline_kw = dict(pipeline_kw, format=format)
        img, shapes = prepare_images_device([frames], img_scale, **pipeline_kw)       # one multi-view sample
        self._check_shapes(shapes[0], self.n_views, 'scene')
        return self._add_views(img[0], E, emit, shapes[0], weights, maps, strided=False, gate=gate, verdict=verdict)

    # ------------------------------------------------------------------ reading the scene
    def volume(self):
        """(mean volume [1,X,Y,Z,C] channels-last, valid bool [1,X,Y,Z]) of the views so far: the session's own buffers, rewritten by
        the next add (clone what must outlive it)."""
        self._check_open()
        if self.n_views == 0:
            raise RuntimeError('the scene has no views yet')
        if self._stale:
            self._refresh()
            self._stale = False
        return self._mean, self._valid.view(torch.bool)

    def _refresh(self):
        """Bring the mean / valid buffers up to date with the state, in one launch."""
        m = self._model
        if self._window is not None and (self._wring is not None or self._mring is not None or self._dring is not None):
            # the same lift with the weight ring and the map rings that exist: the weighted mean of the kept views (no map ring: the weighted launch)
            form, kw = _lift_maps(self._mring, self._dring, self._gate)
            getattr(ops, f'backproject_{form}_mean_')(self._ring, self._pring, [[v[1] for v in self._views]], self._wring, [0], self._origin, self._crop,
                                                      m.voxel_size, self._mean, self._valid, sampling=getattr(m, 'sampling', 'nearest'), **kw)
        elif self._window is not None:                                # the set changed since the last lift: ONE gathered lift of the views in it, in order
            view_slot = torch.tensor([[v[1] for v in self._views]], dtype=torch.int32).to(self._ring.device)
            ops.backproject_gather_mean_(self._ring, self._pring, view_slot, self._origin, self._crop, m.voxel_size, self._mean, self._valid,
                                         getattr(m, 'sampling', 'nearest'))
        elif self._decay is not None:                                 # (emit=False adds on a fading session: the mean of (sum, weight sum))
            ops.volume_wmean(self._sum, self._wsum, self._mean.dtype, out=self._mean, valid_out=self._valid)
        else:
            ops.volume_mean(self._sum, self._count, self._mean.dtype, out=self._mean, valid_out=self._valid)

    def detect(self):
        """Detections from the views so far: [dict(boxes_3d, scores_3d, labels_3d)] as simple_test returns for one sample."""
        vol, valid = self.volume()
        return _detect(self._model, vol, valid, [self.meta])


class SceneBatch:
    """model.open_scenes(metas, window=None): N streaming scenes on one prepared model that share their launches.  metas: one scene meta
    per scene, as for open_scene (intrinsic, origin and box type may differ; the image size and the model are common).  Per tick,
    add_views takes the new views of ANY subset of the scenes (0, 1 or several per scene), runs the trunk ONCE over all of them and adds
    them to the touched scenes in ONE launch (ops.backproject_lists_accum_, ivx_backproject_lists_fwd: ragged slot lists, one row of
    the state pools per scene, a `first` flag per scene); detect() runs ONE batched neck + head + NMS over the stacked mean rows.

    State, allocated at the first add: sum fp32 [N,X,Y,Z,C], count int32 [N,X,Y,Z], mean [N,X,Y,Z,C] in the storage type, valid uint8
    [N,X,Y,Z] -- per scene X*Y*Z * (C * (4 + sizeof(element)) + 5) bytes (the module docstring has the ScanNet figures).  window=W keeps
    no sums: a feature ring [N*W,1,FH,FW,C] (scene s owns slots s*W .. s*W+W-1) and a projection ring [N*W,3,4], per-scene ordered
    (id, slot, extrinsic) lists with FIFO eviction per scene, and the mean / valid pools; the scenes whose set changed are lifted again, all
    in one launch (ops.backproject_lists_mean_), when volume() / detect() asks.  The host state of scene s is the _SceneRecord _scenes[s]:
    the rules of a scene are the record's, the pools, the packed camera upload and the launches are the batch's.

    What is exact and what is not.
      Volume.   Row s of the batch's volume is bit for bit ONE ops.backproject_mean over the features the trunk produced for scene s's
                views, tick by tick, in arrival order -- what a SceneSession fed the same features holds.  Mask and count do not depend on
                the features at all: they are the one-shot lift's.
      Features. With the default fp16-pair trunk the per-tensor operand scales depend on which views share a trunk call, so a view's
                features may differ in the last bits from those a single session computes for it.
      Neck and boxes.  The batched neck's operand scales depend on the batch too: there is NO claim that scene s's boxes equal those of
                a B = 1 SceneSession.detect().
      Detection stage.  detect() is exactly the model's batched detection stage (detect_cl / detect_indoor_cl) on the stacked rows.
    A call that raises before its launch leaves every scene as it was.

    Fading batches (open_scenes(metas, decay=lam or [lam_0 .. lam_N-1], forget_below=t); SceneSession has the rules): a weight-sum pool [N,X,Y,Z]
    fp32 beside the sums, and ONE weighted listed lift per tick (ops.backproject_weighted_accum_).  Every add_views call is one tick FOR THE SCENES
    IT TOUCHES: only the touched scenes fade (each by its own decay); a scene that gets no view in a call is neither read nor written, so its
    state does not age.  A caller who wants wall-clock fading gives every scene a view (or a zero-weight view) per tick.  A windowed batch takes
    weights and reweight(scene, ids, weights); its re-lift is then the weighted mean of the kept views (a host weight ring [N*W]).

    Pixel maps (open_scenes(metas, ..., depth_gate=(behind, front)), add_views(..., pixel_weights=, depths=); SceneSession has the rules): one gate for
    every scene; row t of a map tensor belongs to view t of the call.  A fading batch passes the call's maps to the tick's one launch; a windowed
    batch keeps device rings [N*W,FH,FW] beside the feature ring, scene s owning slots s*W .. s*W+W-1 as for the features."""

    def __init__(self, model, metas, window=None, decay=None, forget_below=0.0, depth_gate=None):
        metas = list(metas)
        if not metas:
            raise ValueError('open_scenes needs at least one scene meta')
        decays = list(decay) if hasattr(decay, '__len__') else [decay] * len(metas)
        if len(decays) != len(metas):
            raise ValueError(f'{len(decays)} decays for {len(metas)} scenes (one value for all, or one per scene)')
        if any(d is None for d in decays) and any(d is not None for d in decays):
            raise ValueError('decay must be given for every scene of a batch or for none')
        self._scenes = [_SceneRecord(model, meta, window, d, forget_below, depth_gate) for meta, d in zip(metas, decays)]      # checks every meta, window, decay, gate and head_2d
        self._fading, self._forget, self._wsum, self._wring = decays[0] is not None, self._scenes[0]._forget, None, None
        self._mring = self._dring = None          # windowed: the device rings of the slots' pixel maps [N*W,FH,FW], each None until a map is given
        self._covers = {}                         # add_views_u8(lens=): the cover maps [FH,FW] by (lens, source shape, pipeline shapes, device)
        self._model, self._window, self._N = model, self._scenes[0]._window, len(metas)
        self._sum = self._count = self._mean = self._valid = self._ring = self._pring = None
        self._hw, self._closed = None, False
        self._cam = [None] * self._N              # per scene: host (new_origin [3], crop [2]) of its last add
        self.last_admitted = None                 # the gate's verdict per view of the last add_views(..., min_novelty=) call; None after an ungated one

    # ------------------------------------------------------------------ state
    def _check_open(self):
        if self._closed:
            raise RuntimeError('this SceneBatch is closed')

    def _scene_index(self, s):
        if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 0 <= s < self._N:
            raise ValueError(f'unknown scene index {s!r} (this batch has scenes 0 .. {self._N - 1})')
        return int(s)

    def __len__(self):
        return self._N

    @property
    def metas(self):
        """The scenes' metas: complete simple_test metas of everything added."""
        return [r.meta for r in self._scenes]

    @property
    def n_views(self):
        return [r.n_views for r in self._scenes]

    def view_ids(self, scene):
        self._check_open()
        return self._scenes[self._scene_index(scene)].view_ids

    def reset(self, scenes=None):
        """Forget every view of these scenes (None: all); the pools are kept."""
        self._check_open()
        for s in (range(self._N) if scenes is None else [self._scene_index(s) for s in scenes]):
            self._scenes[s].reset()
            self._cam[s] = None
            if self._wring is not None:
                self._wring[s * self._window:(s + 1) * self._window] = [1.0] * self._window
        if not any(self.n_views):
            self._hw = None
        return self

    def close(self):
        self._sum = self._count = self._mean = self._valid = self._ring = self._pring = self._wsum = self._wring = self._mring = self._dring = None
        self._closed = True

    def remove_views(self, scene, ids):
        """Drop the views with these ids from one scene of a windowed batch; an unknown id raises KeyError and changes nothing."""
        self._check_open()
        self._scenes[self._scene_index(scene)].remove_views(ids)
        return self

    def reweight(self, scene, ids, weights):
        """Change the weights of kept views of one scene of a windowed batch (SceneSession.reweight); an unknown id raises KeyError and
        changes nothing."""
        self._check_open()
        s = self._scene_index(scene)              # (the record's slots are the batch's: scene s owns s*W .. s*W+W-1)
        self._wring = self._scenes[s]._reweight(ids, weights, self._wring, self._N, 'batch: open_scenes(metas, window=W)', f'scene {s}')
        return self

    def scrolled(self, scene):
        """The cumulative shift of one scene since it was opened or reset."""
        self._check_open()
        return self._scenes[self._scene_index(scene)].scrolled

    def scroll(self, scenes, voxels):
        """SceneSession.scroll for scenes of the batch: one scene index with one (sx, sy, sz), or a list of distinct indices with one triple each.
        All named scenes move in ONE ops.volume_scroll_ on their rows of the pools; their metas and host camera records follow the same origin
        rule.  Scenes not named are neither read nor written.  A call that raises leaves every scene as it was."""
        self._check_open()
        if isinstance(scenes, (int, np.integer)) and not isinstance(scenes, bool):
            scenes, voxels = [scenes], [voxels]
        if isinstance(scenes, torch.Tensor) or not hasattr(scenes, '__len__') or isinstance(voxels, torch.Tensor) or not hasattr(voxels, '__len__') \
                or len(scenes) != len(voxels):
            raise ValueError(f'scroll takes one scene index with one (sx, sy, sz), or lists of both of one length, got {scenes!r} and {voxels!r}')
        scenes = [self._scene_index(s) for s in scenes]
        if len(set(scenes)) != len(scenes):
            raise ValueError(f'a scene can be scrolled once per call, got {scenes}')
        m = self._model
        moves = [(s, v) for s, v in zip(scenes, [_check_scroll(m, v) for v in voxels]) if any(v)]
        origins = [scrolled_origin(self._scenes[s].meta['lidar2img']['origin'], v, m.voxel_size) for s, v in moves]
        rows = [(s, v) for s, v in moves if self._window is None and self._scenes[s].n_views]
        if rows:
            ops.volume_scroll_(self._sum, self._count, [s for s, _ in rows], [v for _, v in rows], self._wsum)
        for (s, v), origin in zip(moves, origins):
            self._scenes[s]._scroll(v, origin)
            if self._cam[s] is not None:
                self._cam[s] = (m._new_origin(origin), self._cam[s][1])
        return self

    def frame(self, scene):
        """The product of every T one scene was warped by since it was opened or reset (SceneSession.frame)."""
        self._check_open()
        return self._scenes[self._scene_index(scene)].frame

    def warp(self, scenes, Ts):
        """SceneSession.warp for scenes of the batch: one scene index with one T, or a list of distinct indices with one T each.  A fading batch
        warps the rows of all named scenes in ONE ops.volume_warp into a scratch pool of as many rows as scenes it has to move -- allocated for
        the call, so the batch does not hold its state twice -- and copies those rows back; a windowed batch re-poses the kept views of the named
        scenes (one index_copy_ of their projection rows).  Scenes not named are neither read nor written.  A plain batch raises
        NotImplementedError.  A call that raises leaves every scene as it was."""
        self._check_open()
        if isinstance(scenes, (int, np.integer)) and not isinstance(scenes, bool):
            scenes, Ts = [scenes], [Ts]
        if isinstance(scenes, torch.Tensor) or not hasattr(scenes, '__len__') or (isinstance(Ts, torch.Tensor) and Ts.is_cuda) or not hasattr(Ts, '__len__') \
                or len(scenes) != len(Ts):
            raise ValueError(f'warp takes one scene index with one T, or lists of both of one length, got {scenes!r} and {len(Ts) if hasattr(Ts, "__len__") else Ts!r} transforms')
        scenes = [self._scene_index(s) for s in scenes]
        if len(set(scenes)) != len(scenes):
            raise ValueError(f'a scene can be warped once per call, got {scenes}')
        Ts = [_check_warp(T) for T in Ts]
        if self._window is None and not self._fading:
            raise NotImplementedError(_PLAIN_WARP.format(what='batch'))
        m = self._model
        moves = [(s, T) + self._scenes[s]._warped(T) for s, T in zip(scenes, Ts) if not np.array_equal(T, np.eye(4))]
        rows = [mv for mv in moves if self._scenes[mv[0]].n_views]
        if rows and self._window is not None:
            dev = self._pring.device
            idx = torch.tensor([v[1] for _, _, _, views in rows for v in views], dtype=torch.int64).to(dev)
            proj = torch.cat([m._compute_projection(dict(self._scenes[s].meta, lidar2img=dict(self._scenes[s].meta['lidar2img'], extrinsic=ext)), 4)
                              for s, _, ext, _ in rows])
            self._pring.index_copy_(0, idx, proj.contiguous().to(dev))
        elif rows:
            named = [s for s, _, _, _ in rows]
            scratch = tuple(torch.empty((len(named),) + tuple(t.shape[1:]), device=t.device, dtype=t.dtype) for t in (self._sum, self._wsum, self._count))
            ops.volume_warp(self._sum, self._wsum, self._count, named, [T for _, T, _, _ in rows], torch.stack([self._cam[s][0] for s in named]).float().numpy(),
                            m.voxel_size, out=scratch, out_rows=list(range(len(named))), forget_below=self._forget)
            idx = torch.tensor(named, dtype=torch.int64).to(self._sum.device)
            for pool, part in zip((self._sum, self._wsum, self._count), scratch):
                pool.index_copy_(0, idx, part)
        for s, T, ext, views in moves:
            self._scenes[s]._warp(T, ext, views)
        return self

    def merge(self, scenes, sources, Ts=None, weights=None):
        """SceneSession.merge between scenes of the batch: one destination index with one source index, or two lists of one length; scene
        scenes[i] takes the state of scene sources[i] under Ts[i] (x_source = T x_destination; None: inv(frame(source)) @ frame(destination))
        with weights[i] (None: 1).  Destinations are distinct, no index is both a destination and a source, a source may repeat.  All pairs go in
        ONE ops.volume_merge_ in place on the pools, with no scratch: the pools are their own source, on disjoint rows.  The records follow the
        session rule.  A source without views is skipped; a destination without views has its rows zeroed first.  Scenes not named are neither
        read nor written.  Evidence two scenes hold of the same views counts twice.  A plain batch and a windowed batch raise
        NotImplementedError.  A call that raises leaves every scene as it was."""
        self._check_open()
        one = isinstance(scenes, (int, np.integer)) and not isinstance(scenes, bool)
        if one:
            scenes, sources, Ts, weights = [scenes], [sources], (None if Ts is None else [Ts]), (None if weights is None else [weights])
        if isinstance(scenes, torch.Tensor) or not hasattr(scenes, '__len__') or isinstance(sources, torch.Tensor) or not hasattr(sources, '__len__') \
                or len(scenes) != len(sources) or not len(scenes):
            raise ValueError(f'merge takes one destination index with one source index, or lists of both of one length, got {scenes!r} and {sources!r}')
        P = len(scenes)
        scenes, sources = [self._scene_index(s) for s in scenes], [self._scene_index(s) for s in sources]
        if len(set(scenes)) != P:
            raise ValueError(f'a scene can be the destination of one merge per call, got {scenes}')
        both = sorted(set(scenes) & set(sources))
        if both:
            raise ValueError(f'scenes {both} are named both as a destination and as a source of one call')
        for arg, name in ((Ts, 'Ts'), (weights, 'weights')):
            if arg is not None and (isinstance(arg, (str, bytes)) or (isinstance(arg, torch.Tensor) and arg.is_cuda) or not hasattr(arg, '__len__') or len(arg) != P):
                raise ValueError(f'{name} must be None or hold one entry per pair: {P} pairs, got {len(arg) if hasattr(arg, "__len__") else arg!r}')
        _check_merge_kind(self._window, self._fading, 'batch')
        Ts = [_merge_transform(self._scenes[d], self._scenes[s], None if Ts is None else Ts[i]) for i, (d, s) in enumerate(zip(scenes, sources))]
        weights = [1.0] * P if weights is None else [_check_merge_weight(w) for w in weights]
        pairs = [(d, s, T, w) for d, s, T, w in zip(scenes, sources, Ts, weights) if self._scenes[s].n_views]
        if not pairs:
            return self
        m = self._model
        origin = lambda s: (self._cam[s][0] if self._cam[s] is not None else m._new_origin(self._scenes[s].meta['lidar2img']['origin'])).float().numpy()      # noqa: E731
        fresh = [d for d, _, _, _ in pairs if not self._scenes[d].n_views]
        if fresh:                                 # what a `first` add would do to these rows (they hold nothing: no scene changes)
            idx = torch.tensor(fresh, dtype=torch.int64).to(self._sum.device)
            for pool in (self._sum, self._wsum, self._count):
                pool.index_fill_(0, idx, 0)
        state = (self._sum, self._wsum, self._count)
        ops.volume_merge_(*state, [d for d, _, _, _ in pairs], state, [s for _, s, _, _ in pairs], [T for _, _, T, _ in pairs],
                          np.stack([origin(d) for d, _, _, _ in pairs]), np.stack([origin(s) for _, s, _, _ in pairs]), m.voxel_size,
                          alpha=[w for _, _, _, w in pairs], forget_below=self._forget)
        for d, s, T, _ in pairs:
            self._scenes[d]._merged(self._scenes[s], T)
            if self._cam[d] is None:              # a scene with views has its host camera record (warp, scroll and the refresh read it): what its first add
                meta = self._scenes[d].meta       # would have stored, by _camera_setup's rules at the lifts' stride of 4
                self._cam[d] = (m._new_origin(meta['lidar2img']['origin']), torch.tensor([meta['img_shape'][0] // 4, meta['img_shape'][1] // 4], dtype=torch.int32))
        return self

    # ------------------------------------------------------------------ matching
    def _check_match(self, scenes, sources, op):
        """Scene indices of a match -> (scenes, sources) as int lists; the batch is open and fading and every named scene holds views."""
        self._check_open()
        scenes, sources = [self._scene_index(s) for s in scenes], [self._scene_index(s) for s in sources]
        _check_match_kind(self._window, self._fading, 'batch', op)
        empty = sorted({s for s in scenes + sources if not self._scenes[s].n_views})
        if empty:
            raise ValueError(f'{op}: scenes {empty} are empty (they hold no views, so there is no state to compare)')
        return scenes, sources

    def _origin_of(self, s):
        m = self._model
        return (self._cam[s][0] if self._cam[s] is not None else m._new_origin(self._scenes[s].meta['lidar2img']['origin'])).float().numpy()

    def _match(self, scenes, sources, cands, step, min_overlap):
        state = (self._sum, self._wsum)
        pairs, own, stats = ops.volume_match(*state, scenes, state, sources, cands, np.stack([self._origin_of(d) for d in scenes]),
                                             np.stack([self._origin_of(s) for s in sources]), self._model.voxel_size, step)
        return _match_results(pairs, own, stats, cands, min_overlap)

    def match(self, scenes, sources, Ts=None, step=1, min_overlap=0.3):
        """SceneSession.match between scenes of the batch: one scene index with one source index and one candidate list (-> one MatchResult), or
        two lists of one length with one candidate list per pair (-> a list).  Pair i scores Ts[i], K host 4x4 with x_source = T x_scene -- the
        same K for every pair -- or, with Ts None, the one candidate inv(frame(source)) @ frame(scene).  All pairs go in ONE ops.volume_match on
        the pools, which are read only: a scene may appear in any number of pairs, on either side.  A plain batch and a windowed batch raise
        NotImplementedError, a scene without views ValueError.  Every scene is unchanged."""
        one = isinstance(scenes, (int, np.integer)) and not isinstance(scenes, bool)
        if one:
            scenes, sources, Ts = [scenes], [sources], (None if Ts is None else [Ts])
        if isinstance(scenes, torch.Tensor) or not hasattr(scenes, '__len__') or isinstance(sources, torch.Tensor) or not hasattr(sources, '__len__') \
                or len(scenes) != len(sources) or not len(scenes):
            raise ValueError(f'match takes one scene index with one source index, or lists of both of one length, got {scenes!r} and {sources!r}')
        P = len(scenes)
        if Ts is not None and (isinstance(Ts, (str, bytes, torch.Tensor)) or not hasattr(Ts, '__len__') or len(Ts) != P):
            raise ValueError(f'Ts must be None or hold one candidate list per pair: {P} pairs, got {len(Ts) if hasattr(Ts, "__len__") else Ts!r}')
        scenes, sources = self._check_match(scenes, sources, 'match')
        cands = [_match_candidates(self._scenes[d], self._scenes[s], None if Ts is None else Ts[i]) for i, (d, s) in enumerate(zip(scenes, sources))]
        if len({len(c) for c in cands}) != 1:
            raise ValueError(f'every pair of a call takes the same number of candidates, got {[len(c) for c in cands]}')
        res = self._match(scenes, sources, cands, ops._match_step(step), _check_min_overlap(min_overlap))
        return res[0] if one else res

    def register(self, scene, source, T0=None, yaw=math.radians(8), shift=None, levels=6, step=1, min_overlap=0.3, refine=False, dof=None):
        """SceneSession.register between two scenes of the batch (x_source = T x_scene): the same local coarse-to-fine search around T0 over yaw
        and translation, one ops.volume_match per level; refine=True then refines the last level's pose as SceneSession.register does.
        -> (T float64 [4,4], the MatchResult of the last level);  refine=True: (T float64 [4,4], AlignResult)."""
        (d,), (s,) = self._check_match([scene], [source], 'register')
        T0 = _merge_transform(self._scenes[d], self._scenes[s], T0)
        min_overlap = _check_min_overlap(min_overlap)
        dof = _check_register_refine(refine, dof)
        T, res = _register(lambda Ts, p: self._match([d], [s], [Ts], p, min_overlap)[0], T0, yaw, shift, levels, step, min_overlap,
                           np.asarray(self._scenes[d].meta['lidar2img']['origin'], np.float64), self._model.voxel_size)
        if not refine:
            return T, res
        T, out = self.refine(d, s, T, dof=dof, step=_last_step(step), min_overlap=min_overlap)
        out.match = res
        return T, out

    def _align(self, scenes, sources, Ts, abouts, step):
        state = (self._sum, self._wsum)
        outs = ops.volume_align(*state, scenes, state, sources, [[T] for T in Ts], np.stack(abouts), np.stack([self._origin_of(d) for d in scenes]),
                                np.stack([self._origin_of(s) for s in sources]), self._model.voxel_size, step)
        return _align_host(outs, len(Ts))

    def refine(self, scenes, sources, T0s=None, iters=12, dof=ALIGN_DOF, step=1, min_overlap=0.3, damping=1e-3, tol_shift=None, tol_rot=1e-5):
        """SceneSession.refine between scenes of the batch: one scene index with one source index and one T0 (-> (T, AlignResult)), or two
        lists of one length with one T0 (or None) per pair (-> a list of (T, AlignResult)); x_source = T x_scene, T0s None: every pair starts
        at inv(frame(source)) @ frame(scene).  Every iteration makes ONE ops.volume_align over all the pairs that are still running (B = those
        pairs, K = 1) and reads 31 doubles and three counts per pair back; a pair's answer does not depend on the pairs beside it and equals a
        session's on the same two states bit for bit.  LOCAL like the session's: run register first for anything wider than about a voxel and
        a few degrees.  The pools are read only: a scene may appear in any number of pairs, on either side.  Refusals are match's."""
        one = isinstance(scenes, (int, np.integer)) and not isinstance(scenes, bool)
        if one:
            scenes, sources, T0s = [scenes], [sources], [T0s]
        if isinstance(scenes, torch.Tensor) or not hasattr(scenes, '__len__') or isinstance(sources, torch.Tensor) or not hasattr(sources, '__len__') \
                or len(scenes) != len(sources) or not len(scenes):
            raise ValueError(f'refine takes one scene index with one source index, or lists of both of one length, got {scenes!r} and {sources!r}')
        scenes, sources = self._check_match(scenes, sources, 'refine')
        T0s = _refine_T0s([(self._scenes[d], self._scenes[s]) for d, s in zip(scenes, sources)], T0s)
        args = _check_refine(iters, dof, min_overlap, damping, tol_shift, tol_rot, self._model.voxel_size)
        step = ops._match_step(step)
        abouts = [np.asarray(self._scenes[d].meta['lidar2img']['origin'], np.float64) for d in scenes]
        res = _refine(lambda idx, Ts: self._align([scenes[p] for p in idx], [sources[p] for p in idx], Ts, [abouts[p] for p in idx], step),
                      T0s, abouts, int(self._sum.shape[-1]), *args)
        return res[0] if one else res

    # ------------------------------------------------------------------ snapshots
    def _scene_list(self, scenes, others=None, what='snapshot'):
        """One scene index (with one entry of `others`) or a list of distinct indices (with a list of as many) -> (one, indices, others)."""
        one = isinstance(scenes, (int, np.integer)) and not isinstance(scenes, bool)
        if one:
            scenes, others = [scenes], [others]
        if isinstance(scenes, torch.Tensor) or not hasattr(scenes, '__len__') or not len(scenes) or \
                (others is not None and (not isinstance(others, (list, tuple)) or len(others) != len(scenes))):
            raise ValueError(f'{what} takes one scene index, or a list of distinct indices (with one snapshot each), got {scenes!r}')
        scenes = [self._scene_index(s) for s in scenes]
        if len(set(scenes)) != len(scenes):
            raise ValueError(f'a scene can be named once per {what} call, got {scenes}')
        return one, scenes, others

    def snapshot(self, scene, dtype=torch.float32):
        """SceneSession.snapshot for scenes of a plain or fading batch: one scene index -> a SceneSnapshot, a list of distinct indices -> a list.
        The rows of all named scenes that have views go in ONE ops.volume_pack; a scene without views gives a snapshot with no records.  The
        batch is unchanged.  A snapshot does not remember its container: model.restore_scene opens it as a SceneSession, restore puts it into a
        row of any batch of the same kind.  A windowed batch raises NotImplementedError."""
        self._check_open()
        _check_snapshot_dtype(dtype)
        one, scenes, _ = self._scene_list(scene)
        if self._window is not None:
            raise NotImplementedError(_WINDOW_SNAPSHOT.format(what='batch'))
        m = self._model
        rows = [s for s in scenes if self._scenes[s].n_views]
        Cn = int(self._sum.shape[-1]) if self._sum is not None else int(m.neck.out_channels)
        recs = dict(zip(rows, ops.volume_pack(self._sum, self._count, rows, self._wsum, dtype))) if rows else {}
        out = [_snapshot_of(self._scenes[s], m, _host_records(recs.get(s), Cn, dtype, self._fading), Cn) for s in scenes]
        return out[0] if one else out

    def restore(self, scene, snapshot, device=None):
        """Put snapshots into rows of a plain or fading batch: one scene index with one SceneSnapshot, or a list of distinct indices with one
        snapshot each.  Each named row takes its snapshot's state -- ONE ops.volume_unpack_ for all rows of the call: every voxel of the row is
        written, so what the scene held before is gone -- and its record takes the snapshot's host fields: extrinsics, n_views, origin, shapes,
        scrolled, frame; the decay of a fading scene becomes the snapshot's.  The mean is recomputed when next asked for.  The snapshot's kind
        must be the batch's, forget_below and depth_gate the batch's own, grid / voxel size / channels / sampling rule the model's, and the image
        size of a snapshot with views what the batch already holds (an empty batch takes it).  A batch that has not allocated its pools
        allocates them as its first add would (on `device`, else the model's).  A snapshot without views resets the scene to it.  A windowed
        batch raises NotImplementedError.  A call that raises leaves every scene as it was."""
        self._check_open()
        one, scenes, snaps = self._scene_list(scene, snapshot, 'restore')
        if self._window is not None:
            raise NotImplementedError(_WINDOW_SNAPSHOT.format(what='batch').replace('snapshot:', 'restore:'))
        m = self._model
        hw = self._hw
        for s, snap in zip(scenes, snaps):
            _check_restore(m, snap, self._fading, 'batch')
            _restored_meta(snap)
            if snap.forget_below != self._forget or snap.depth_gate != self._scenes[s]._gate:
                raise ValueError(f'restore: the snapshot was fused with forget_below {snap.forget_below} and depth_gate {snap.depth_gate}, the batch with '
                                 f'{self._forget} and {self._scenes[s]._gate}')
            if snap.n_views:
                _check_size(snap.hw, hw, 'batch')
                hw = snap.hw
        full = [(s, snap) for s, snap in zip(scenes, snaps) if snap.n_views]
        if full:
            X, Y, Z = m.n_voxels
            Cn = full[0][1].channels
            if self._sum is None:                 # the state pools, as the first add allocates them
                dev, N = torch.device(device) if device is not None else _scene_device(m), self._N
                store = m.storage_dtype if m.storage_dtype in (torch.float32, torch.bfloat16) else torch.float32
                pools = (torch.empty((N, X, Y, Z, Cn), device=dev, dtype=torch.float32), torch.empty((N, X, Y, Z), device=dev, dtype=torch.int32),
                         torch.empty((N, X, Y, Z), device=dev, dtype=torch.float32) if self._fading else None,
                         torch.empty((N, X, Y, Z, Cn), device=dev, dtype=store), torch.empty((N, X, Y, Z), device=dev, dtype=torch.uint8))
            else:
                pools = (self._sum, self._count, self._wsum, self._mean, self._valid)
            with torch.cuda.device(pools[0].device):
                ops.volume_unpack_(pools[0], pools[1], [s for s, _ in full], [snap.records() for _, snap in full], pools[2])
            self._sum, self._count, self._wsum, self._mean, self._valid = pools
            self._hw = hw
        for s, snap in zip(scenes, snaps):
            r = self._scenes[s]
            _adopt(r, snap)
            r._decay = snap.decay
            self._cam[s] = None
            if snap.n_views:                      # the host camera record its first add would have stored (warp, scroll and the refresh read it)
                self._cam[s] = (m._new_origin(r.meta['lidar2img']['origin']), torch.tensor([r.meta['img_shape'][0] // 4, r.meta['img_shape'][1] // 4], dtype=torch.int32))
        if not any(self.n_views):
            self._hw = None
        return self

    # ------------------------------------------------------------------ adding views
    def _features(self, img):
        return _trunk(self._model, img)

    def add_views(self, img, extrinsics, scene, emit=True, weights=None, pixel_weights=None, depths=None, min_novelty=None, fresh_below=None):
        """img [T,3,H,W] float32 on the device, extrinsics: T float32 4x4 matrices, scene: T scene indices -- view t belongs to scene
        scene[t]; the views of one scene count in the order given.  emit=False skips the store of the means (computed when asked).
        Windowed batch: more than W views for one scene in a call raise ValueError; emit has no effect.
        weights: one finite float >= 0 per view, on a batch opened with decay= or window=.  Fading batch: one tick for the touched scenes only.
        pixel_weights, depths: one float32 tensor [T,FH,FW] or [T,H,W] each, as for SceneSession.add_views (row t is view t's map).
        min_novelty in (0, 1] / fresh_below: the keyframe gate of SceneSession.add_views, ONE coverage launch for all the T views against their
        scenes' states before the call; rejected views are dropped before the trunk, a scene whose views are all rejected is untouched (and
        does not fade), and last_admitted holds the T verdicts (None after an ungated call)."""
        return self._add_views(img, extrinsics, scene, emit, {}, weights=weights, maps=(pixel_weights, depths), gate=_check_novelty(min_novelty, fresh_below))

    def add_views_u8(self, frames, extrinsics, scene, img_scale, emit=True, weights=None, pixel_weights=None, depths=None, min_novelty=None,
                     fresh_below=None, lens=None, depth_frames=None, depth_scale=0.001, format=None, **pipeline_kw):
        """add_views from uint8 camera frames through data.prepare_images_device (as SceneSession.add_views_u8); fills img_shape /
        ori_shape / pad_shape of every scene's meta, which later frames must reproduce.  Pixel maps at feature resolution only.  The gate
        runs before the pipeline once the batch knows its shapes, after it on the first call.  lens / depth_frames / depth_scale as for
        SceneSession.add_views_u8 (entry t belongs to frame t; the metas of the touched scenes must agree with the lenses; the cover
        cache is the batch's); format as for SceneSession.add_views_u8."""
        from .data import prepare_images_device, FrameFormat
        self._check_open()
        frames = list(frames)
        E = _check_extrinsics(extrinsics, len(frames))
        groups = self._groups(scene, len(frames))
        weights = self._scenes[0]._take_weights(weights, len(frames), 'batch')
        maps = self._scenes[0]._take_maps(pixel_weights, depths, len(frames), 'batch')
        if lens is not None or depth_frames is not None:
            lens, maps = _lens_maps([self._scenes[s] for s in groups], self._covers, frames, maps, lens, depth_frames, depth_scale, img_scale, pipeline_kw, 'batch', format)
        gate, verdict = _check_novelty(min_novelty, fresh_below), None
        if gate[0] is not None and self._hw is not None and all('img_shape' in self._scenes[s].meta and 'ori_shape' in self._scenes[s].meta for s in groups):
            verdict = admitted(self._coverage(E, groups, maps, self._hw, {}, gate[1], strided=False), gate[0])
            if not any(verdict):
                self.last_admitted = verdict
                return self
            frames, E, scene, weights = _kept(verdict, frames), _kept(verdict, E), _kept(verdict, list(scene)), _kept(verdict, weights)
            maps, groups, gate, lens = tuple(_kept(verdict, t) for t in maps), self._groups(scene, len(frames)), (None, gate[1]), _kept(verdict, lens)
            format = format if format is None or isinstance(format, (str, FrameFormat)) else _kept(verdict, list(format))
        if lens is not None:
            pipeline_kw = dict(pipeline_kw, lens=lens)
        if format is not None:
            pipeline_kw = dict(pipeline_kw, format=format)
        img, shapes = prepare_images_device([frames], img_scale, **pipeline_kw)
        for r in self._scenes:
            r._check_shapes(shapes[0], any(self.n_views), 'batch')
        return self._add_views(img[0], E, scene, emit, shapes[0], groups, weights, maps, strided=False, gate=gate, verdict=verdict)

    def _groups(self, scene, T, fit=True):
        """scene (T indices) -> {scene: [t, ...]} in first-touch order; the checks that need no device (fit: the views are to be added, so
        those of one scene must fit its window)."""
        if isinstance(scene, torch.Tensor) or not hasattr(scene, '__len__') or len(scene) != T:
            raise ValueError(f'scene must list one scene index per view: {T} views, got {scene!r}')
        groups = {}
        for t, s in enumerate(scene):
            groups.setdefault(self._scene_index(s), []).append(t)
        for s, ts in groups.items():
            if fit:
                self._scenes[s]._check_fits(len(ts), f' of scene {s}')
        return groups

    def coverage(self, extrinsics, scene, pixel_weights=None, depths=None, fresh_below=None):
        """SceneSession.coverage for T candidate views of any subset of the scenes: extrinsics: T float32 4x4 matrices, scene: T scene indices
        -> np.ndarray [T,2] int64 (seen, fresh) in the order of the call's views.  ONE launch (ops.view_coverage: ragged lists per scene,
        rows equal to the scene indices) and one device-to-host read.  The evidence is the scenes' rows of the count pool (plain batch), of the
        weight-sum pool (fading) or of the valid pool (windowed; the stale ones among the named scenes are lifted again first, in one launch);
        a scene without views has none.  pixel_weights / depths: [T,FH,FW] or [T,H,W], row t is view t's map."""
        self._check_open()
        extrinsics = list(extrinsics)
        E = _check_extrinsics(extrinsics, len(extrinsics))
        if not E:
            raise ValueError('coverage needs at least one candidate view')
        groups = self._groups(scene, len(E), fit=False)
        maps = tuple(_check_map(t, name, len(E)) for t, name in zip((pixel_weights, depths), MAP_FILL))
        if maps[1] is not None and self._scenes[0]._gate is None:
            raise ValueError('this batch was opened without depth_gate and takes no depths: open it with depth_gate=(behind, front)')
        return self._coverage(E, groups, maps, self._hw, {}, _check_novelty(None, fresh_below, alone=True)[1])

    def _coverage(self, E, groups, maps, hw, shapes, fresh_below, strided=True, dev=None):
        """coverage() of checked arguments: groups {scene: [t, ...]} of the T views, shapes: the img_shape / ori_shape / pad_shape of frames that
        are not in the metas yet (add_views_u8), hw: the padded image size, None: from the first named scene's meta."""
        m, touched, T = self._model, sorted(groups), len(E)
        metas = {s: dict(self._scenes[s].meta, **shapes) for s in touched}
        for s in touched:
            if 'img_shape' not in metas[s] or 'ori_shape' not in metas[s]:
                raise ValueError('every scene meta needs img_shape and ori_shape (add_views_u8 fills them from its frames)')
        hw, fhw = _coverage_fhw(hw, metas[touched[0]])
        if max(len(groups[s]) for s in touched) > ops.MAX_COVERAGE_VIEWS:
            raise ValueError(f'more than {ops.MAX_COVERAGE_VIEWS} candidate views of one scene in one call')
        dev = _scene_device(m, self._count, self._valid) if dev is None else dev
        cpu = torch.device('cpu')
        proj_h, cams = torch.empty((T, 3, 4), dtype=torch.float32), []
        for s in touched:                         # the host camera set-up of _add_views: rows of proj in the order of the T views
            view_meta = dict(metas[s], lidar2img=dict(metas[s]['lidar2img'], extrinsic=[E[t] for t in groups[s]]))
            p, origin, crop = m._camera_setup([view_meta], 4, cpu)
            proj_h[torch.tensor(groups[s])] = p[0]
            cams.append(self._cam[s] if self._cam[s] is not None else (origin[0], crop[0]))
        proj, origin, crop = self._upload(dev, proj_h, cams)
        pw, dp = (None if t is None else pick_map(t, name, hw, fhw, strided).to(dev).contiguous() for t, name in zip(maps, MAP_FILL))
        with_views = [s for s in touched if self._scenes[s].n_views]
        state = None
        if with_views:                            # the evidence pool; the rows of named scenes without views hold nothing yet: zero is what they mean
            if self._window is not None:
                self._refresh(with_views)
            state = self._valid if self._window is not None else self._wsum if self._fading else self._count
            for s in touched:
                if not self._scenes[s].n_views:
                    state[s].zero_()
        out =ops.view_coverage(proj, [groups[s] for s in touched], touched, origin, crop, m.voxel_size, m.n_voxels, fhw, state, fresh_below, pw, dp,
                                self._scenes[0]._gate).cpu().numpy().astype(np.int64)
        counts = np.zeros((T, 2), np.int64)
        for i, s in enumerate(touched):
            counts[groups[s]] = out[i, :len(groups[s])]
        return counts

    def _add_views(self, img, extrinsics, scene, emit, shapes, groups=None, weights=None, maps=(None, None), strided=True, gate=(None, 1.0), verdict=None):
        self._check_open()
        T, H, W = _check_images(img, 'T')
        E = _check_extrinsics(extrinsics, T)
        if groups is None:
            groups = self._groups(scene, T)
        weights = self._scenes[0]._take_weights(weights, T, 'batch')      # (the scenes of a batch are opened alike)
        maps = self._scenes[0]._take_maps(*maps, T, 'batch')
        _check_size((H, W), self._hw, 'batch')
        touched = sorted(groups)
        for s in touched:
            meta = dict(self._scenes[s].meta, **shapes)
            if 'img_shape' not in meta or 'ori_shape' not in meta:
                raise ValueError('every scene meta needs img_shape and ori_shape (add_views_u8 fills them from its frames)')
        if not img.is_cuda:
            raise RuntimeError('img must be a device (HIP) tensor; the MI355X path has no CPU fallback')
        m = self._model
        if gate[0] is not None:                   # the keyframe gate: ONE coverage launch against the states before the call, before the trunk
            verdict = admitted(self._coverage(E, groups, maps, (H, W), shapes, gate[1], strided, img.device), gate[0])
            if not any(verdict):
                self.last_admitted = verdict
                return self
            if not all(verdict):
                img, E, weights, maps = _kept(verdict, img), _kept(verdict, E), _kept(verdict, weights), tuple(_kept(verdict, t) for t in maps)
                groups = self._groups(_kept(verdict, list(scene)), len(E))
                T, touched = len(E), sorted(groups)
        if m._prepared_device is None:
            m.prepare(img.device)
        p0 = self._features(img.contiguous())                      # ONE trunk call over the T views of this tick
        maps = _maps_at(maps, (H, W), p0, strided)                 # (a map of the wrong size raises here: the batch has not changed yet)
        # host camera set-up: one _compute_projection per touched scene; rows of proj in the order of the T views
        cpu = torch.device('cpu')
        proj_h, cam = torch.empty((T, 3, 4), dtype=torch.float32), {}
        for s in touched:
            ts = groups[s]
            r = self._scenes[s]
            view_meta = dict(r.meta, **shapes)
            view_meta['lidar2img'] = dict(r.meta['lidar2img'], extrinsic=[E[t] for t in ts])
            p, origin, crop = m._camera_setup([view_meta], 4, cpu)
            proj_h[torch.tensor(ts)] = p[0]
            cam[s] = (origin[0], crop[0])
        if self._window is not None:
            self._add_windowed(p0, proj_h, groups, touched, E, (H, W), weights, maps)
        else:
            self._add_unbounded(p0, proj_h, groups, touched, cam, E, (H, W), weights, emit, maps)
        self._hw = (H, W)
        for r in self._scenes:
            r.meta.update(shapes)
        for s in touched:
            self._cam[s] = cam[s]
        self.last_admitted = verdict
        return self

    @staticmethod
    def _upload(dev, proj_h, cams):
        """Projection rows [T,3,4], new_origin [B,3] and crop [B,2] int32 in ONE host-to-device copy (the crop travels as bits)."""
        T, B = (proj_h.shape[0] if proj_h is not None else 0), len(cams)
        parts = ([proj_h.reshape(-1)] if T else []) + [torch.stack([c[0] for c in cams]).reshape(-1).float(),
                                                       torch.stack([c[1] for c in cams]).to(torch.int32).reshape(-1).view(torch.float32)]
        buf = torch.cat(parts).to(dev)
        proj = buf[:T * 12].view(T, 3, 4) if T else None
        origin = buf[T * 12:T * 12 + B * 3].view(B, 3)
        crop = buf[T * 12 + B * 3:].view(torch.int32).view(B, 2)
        return proj, origin, crop

    def _add_unbounded(self, p0, proj_h, groups, touched, cam, E, hw, weights, emit, maps=(None, None)):
        """The new maps p0 [T,1,FH,FW,C] added to the rows of the touched scenes in ONE listed launch (the call's maps are the pool): the plain
        listed lift, or one tick of the weighted one on a fading batch, with the call's pixel maps [T,FH,FW] (consumed here, not kept)."""
        m, dev = self._model, p0.device
        proj, origin, crop = self._upload(dev, proj_h, [cam[s] for s in touched])
        X, Y, Z = m.n_voxels
        Cn = p0.shape[-1]
        if self._sum is None or self._sum.shape[-1] != Cn or self._mean.dtype != p0.dtype:     # the state pools, allocated once
            N = self._N
            self._sum = torch.empty((N, X, Y, Z, Cn), device=dev, dtype=torch.float32)
            self._count = torch.empty((N, X, Y, Z), device=dev, dtype=torch.int32)
            self._mean = torch.empty((N, X, Y, Z, Cn), device=dev, dtype=p0.dtype)
            self._valid = torch.empty((N, X, Y, Z), device=dev, dtype=torch.uint8)
            self._wsum = torch.empty((N, X, Y, Z), device=dev, dtype=torch.float32) if self._fading else None
        lists, first = [groups[s] for s in touched], [self._scenes[s].n_views == 0 for s in touched]
        if self._fading:                          # one tick of the touched scenes: each fades by its own decay, the others are not read
            form, kw = _lift_maps(*maps, self._scenes[0]._gate)
            getattr(ops, f'backproject_{form}_accum_')(p0, proj, lists, weights, touched, first, [self._scenes[s]._decay for s in touched], origin, crop,
                                                       m.voxel_size, self._sum, self._wsum, self._count, self._mean if emit else None,
                                                       self._valid if emit else None, forget_below=self._forget,
                                                       sampling=getattr(m, 'sampling', 'nearest'), **kw)
        else:
            ops.backproject_lists_accum_(p0, proj, lists, touched, first, origin, crop, m.voxel_size, self._sum, self._count,
                                         self._mean if emit else None, self._valid if emit else None, sampling=getattr(m, 'sampling', 'nearest'))
        for s in touched:
            self._scenes[s]._grow([E[t] for t in groups[s]], hw, stale=not emit)

    def _add_windowed(self, p0, proj_h, groups, touched, E, hw, weights, maps=(None, None)):
        """The new maps and projection rows into free slots of their scenes' parts of the rings (one index_copy_ each), the pixel maps into the
        same slots of the map rings; the oldest views of a full scene leave first.  Everything that can fail comes before the first change
        of the batch."""
        m, W, N = self._model, self._window, self._N
        X, Y, Z = m.n_voxels
        Cn, dev = p0.shape[-1], p0.device
        ring, pring, mean, valid = self._ring, self._pring, self._mean, self._valid
        if ring is None or tuple(ring.shape[1:]) != tuple(p0.shape[1:]) or ring.dtype != p0.dtype:
            ring = torch.empty((N * W,) + tuple(p0.shape[1:]), device=dev, dtype=p0.dtype)
            pring = torch.empty((N * W, 3, 4), device=dev, dtype=torch.float32)
            mean = torch.empty((N, X, Y, Z, Cn), device=dev, dtype=p0.dtype)
            valid = torch.empty((N, X, Y, Z), device=dev, dtype=torch.uint8)
        slot_of, placed = [0] * p0.shape[0], {}
        for s in touched:                         # scene s owns the slots s*W .. s*W+W-1
            placed[s] = self._scenes[s]._free_slots(len(groups[s]), s * W)
            for t, q in zip(groups[s], placed[s][1]):
                slot_of[t] = q
        idx = torch.tensor(slot_of, dtype=torch.int64).to(dev)
        ring.index_copy_(0, idx, p0)
        pring.index_copy_(0, idx, proj_h.to(dev))
        self._wring = _ring_weights(self._wring, N * W, slot_of, weights)
        self._mring = _ring_map(self._mring, N * W, p0.shape[-3:-1], dev, slot_of, maps[0], MAP_FILL['pixel_weights'])
        self._dring = _ring_map(self._dring, N * W, p0.shape[-3:-1], dev, slot_of, maps[1], MAP_FILL['depths'])
        self._ring, self._pring, self._mean, self._valid = ring, pring, mean, valid
        for s in touched:
            self._scenes[s]._admit(*placed[s], [E[t] for t in groups[s]], hw)

    # ------------------------------------------------------------------ reading the scenes
    def _refresh(self, scenes):
        """Bring the mean / valid rows of these scenes up to date: a windowed batch re-lifts the stale ones only, in ONE launch."""
        stale = [s for s in scenes if self._scenes[s]._stale]
        if not stale:
            return
        m = self._model
        if self._window is not None:
            _, origin, crop = self._upload(self._ring.device, None, [self._cam[s] for s in stale])
            lists = [[v[1] for v in self._scenes[s]._views] for s in stale]
            if self._wring is not None or self._mring is not None or self._dring is not None:
                form, kw = _lift_maps(self._mring, self._dring, self._scenes[0]._gate)
                getattr(ops, f'backproject_{form}_mean_')(self._ring, self._pring, lists, self._wring, stale, origin, crop, m.voxel_size, self._mean,
                                                          self._valid, sampling=getattr(m, 'sampling', 'nearest'), **kw)
            else:
                ops.backproject_lists_mean_(self._ring, self._pring, lists, stale, origin, crop, m.voxel_size, self._mean, self._valid,
                                            sampling=getattr(m, 'sampling', 'nearest'))
        elif self._fading:
            for s in stale:                       # (emit=False adds: the mean of the stored (sum, weight sum), row by row)
                ops.volume_wmean(self._sum[s:s + 1], self._wsum[s:s + 1], self._mean.dtype, out=self._mean[s:s + 1], valid_out=self._valid[s:s + 1])
        else:
            for s in stale:                       # (emit=False adds: the mean of the stored sums, row by row)
                ops.volume_mean(self._sum[s:s + 1], self._count[s:s + 1], self._mean.dtype, out=self._mean[s:s + 1], valid_out=self._valid[s:s + 1])
        for s in stale:
            self._scenes[s]._stale = False

    def _with_views(self, scenes):
        scenes = [self._scene_index(s) for s in scenes]
        empty = [s for s in scenes if self._scenes[s].n_views == 0]
        if empty:
            raise RuntimeError(f'scenes {empty} have no views yet')
        return scenes

    def volume(self, scene):
        """(mean volume [1,X,Y,Z,C], valid bool [1,X,Y,Z]) of one scene: views of the batch's pools, rewritten by later adds."""
        self._check_open()
        s, = self._with_views([scene])
        self._refresh([s])
        return self._mean[s:s + 1], self._valid[s:s + 1].view(torch.bool)

    def detect(self, scenes=None):
        """One result dict (boxes_3d, scores_3d, labels_3d) per scene, in the order asked; None: every scene that has views.  ONE batched
        neck + head + NMS over the stacked mean rows: the pools as they are when all N scenes are asked in order, one index_select
        otherwise."""
        self._check_open()
        scenes = [s for s in range(self._N) if self._scenes[s].n_views] if scenes is None else self._with_views(scenes)
        if not scenes:
            raise RuntimeError('no scene of the batch has views yet')
        self._refresh(scenes)
        vol, valid = self._mean, self._valid
        if scenes != list(range(self._N)):
            idx = torch.tensor(scenes, dtype=torch.int64).to(vol.device)
            vol, valid = vol.index_select(0, idx), valid.index_select(0, idx)
        return _detect(self._model, vol, valid.view(torch.bool), [self._scenes[s].meta for s in scenes])

