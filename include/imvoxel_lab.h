/* imvoxel_lab.h -- measurement and A/B entry points of libimvoxel_hip.so.  NOT part of the operator ABI a reference maintainer binds
 * (include/imvoxel.h): per-thread knobs that force a kernel variant for the A/B tools under tools/, and the two micro-benchmarks bench.py
 * prices its roofline fractions against.  Defaults (never calling anything here) are the product's behaviour. */
#ifndef IMVOXEL_LAB_H_
#define IMVOXEL_LAB_H_
#include "imvoxel.h"
#ifdef __cplusplus
extern "C" {
#endif

/* A/B knob (per calling thread) of the Winograd-domain GEMMs on fp16 pairs: -1 (default) = the z-halo kernel where it applies (1x1x3 along z,
 * stride 1, pad 1, Cin % 32 == 0: one staged tile serves the three z-taps), 0 = the generic LDS-DMA kernel always, 1 .. 4 = force a config. */
int ivx_conv_set_halo_mode(int mode);

/* Tuning knob for A/B experiments only (per calling thread): 0 = automatic tile choice (default); 1..7 force a tile
 * of the generic kernel, 41..53 of the LDS-DMA fp32 kernel, 61..73 of its bf16 instantiation. */
int ivx_conv_set_tile_override(int cfg);
/* Per calling thread, A/B only (tools/wino_ab.py): kernel of the F(6x6,3x3) output transform.  -1 = the library's rule (2 with a
 * residual, 1 without); 0 whole 8x8 tile per thread, 2 channels per lane (the round-2 kernel); 1 the same with 1 channel per lane;
 * 2 buffer addressing + column accumulation, 2 channels per lane; 3 the same with 1 channel per lane.  input_variant: -1 / 0 two
 * channels per lane, 1 one channel per lane. */
int ivx_conv_winograd_set_variant(int32_t output_variant, int32_t input_variant);
/* Per calling thread, A/B only: 1 = one-channel-per-lane epilogue stores in the LDS-DMA conv kernel; 0 (default) = the
 * LDS-transposed epilogue (a lane stores 4 consecutive channels as one 16-byte word) wherever it applies. */
int ivx_conv_set_epilogue_mode(int narrow);
/* Per calling thread, A/B only: 1 = the round-1 tile rule of the direct convolution planner, 0 (default) = scored choice. */
int ivx_conv_set_plan_mode(int mode);
/* What the conv planner answers for `d` under the calling thread's knobs, from the functions the launchers call.  Host code only: no launch, no
 * device call.  groups == 0: the direct path (ivx_conv_fwd / _ws with allow_ws, ivx_conv_fwd_pio with `io`) -- per distinct batch slice (the
 * full slices, then the shorter last one if there is one) the plan's fields; ws_bytes is what ivx_conv_workspace_bytes /
 * ivx_conv_pio_workspace_bytes return.  groups > 0: one Winograd-domain convolution of a grouped launch -- the z-halo / z-blocked config, or 0 and
 * the tile of the LDS-DMA kernel (tile_matches 0: the launch refuses it for these operands). */
typedef struct ivx_conv_plan_rec {
  int32_t slice_samples, n_slices;    /* samples per batch slice (B: not sliced); distinct slices below (1 or 2) */
  int32_t samples[2], cfg[2], ksplit[2], tail_ks[2], q_total[2], qa[2], bm[2];
  int64_t slice_ws[2];
  int64_t ws_bytes;                   /* maximum over the slices */
  int32_t halo_cfg, grouped_tile, tile_matches, rows_dev_ok;
} ivx_conv_plan_rec;
/* The planner's figures of an LDS-DMA tile: v = {rows, columns, K slab, workgroups per CU}; returns 1, or 0 for a number that is no such tile. */
int ivx_conv_tile_info(int cfg, int32_t *v);
int ivx_conv_plan_query(const ivx_conv_desc *d, const ivx_pair_io *io_or_null, int allow_ws, int groups, ivx_conv_plan_rec *out);
/* Per calling thread, A/B and tests only: 1 = the candidate top-k of the detection tails (ivx_anchor_head_get_bboxes,
 * ivx_fcos_head_level_candidates) always runs as the one-workgroup radix select; 0 (default) = lists of >= 16 384 scores take
 * the chip-wide histogram / compaction form.  Both return the same indices in the same order. */
int ivx_topk_set_mode(int32_t single_workgroup);

/* ---------------------------------------------------------------------------------------
 * Device ceilings measured on the box (measurement only; bench.py prices its roofline fractions against the data-sheet
 * peaks AND these): the dense issue rate of the MFMA form the conv kernel uses for `dtype` (IVX_F32:
 * v_mfma_f32_32x32x2_f32, IVX_BF16: v_mfma_f32_32x32x16_bf16; scratch >= 512 KiB of device memory), and the streaming
 * copy rate of HBM (read + written bytes per second over `bytes` from src to dst; use buffers well past the 256 MiB
 * Infinity Cache).  Both synchronise the stream and return the best of a few repetitions. */
int ivx_ubench_mfma(int32_t dtype, void *scratch, int64_t scratch_bytes, double *tflops, ivx_stream_t stream);
int ivx_ubench_copy(const void *src, void *dst, int64_t bytes, double *gbps, ivx_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Read-only view of a cached plan of the model handle (tests/test_host_plan.py checks its invariants: liveness, aliasing, the side
 * stream's sites, the workspaces).  `what` names the plan: "forward" (the forward and forward_levels entry points, key B, V, H, W),
 * "detect" (the detect entry point, same key), "trunk" (the backbone + FPN entry point, key BV, 1, H, W) or "neck" (the 3-D neck entry
 * points, key B, 1, 0, 0).  Nothing here creates a plan: the matching workspace-size query (or a forward) must have run before, else
 * IVX_ERR_INVALID_ARG.  Host code only; the same functions exist in the CPU restatement of the ABI.
 *
 * Steps and tensors are numbered as in the handle's graph (the whole model); a plan covers the steps [s0, s1).  What a step does:
 *   fuse 0  runs by itself: reads in, res and extra_in, writes out, out2 and extra_out;
 *   fuse 1  one-launch identity bottleneck: runs the steps i .. i + 2 (the two behind it carry fuse 2) and writes fuse_out;
 *   fuse 5  one-launch projection bottleneck: runs the steps i - 1 .. i + 2 (the shortcut conv in front and the two behind carry fuse 2),
 *           writes fuse_out;
 *   fuse 3  image layout change of the one-launch stem: only reads `in` (the maximum of the image goes to out's scalar block);
 *   fuse 4  max-pool step of the one-launch stem: runs the steps i - 2 .. i (fuse 3, fuse 2, itself) from the caller's image, writes out;
 *   fuse 2  covered by a neighbour, launches nothing.
 * side / join: site number (1 .. n_sides) on the shortcut conv that goes to the side stream and on the step that waits for it. */
typedef struct ivx_plan_info {
  int64_t cam_bytes, arena, ws_off, ws_bytes, ws2_off, ws2_bytes, total, scal_off, scal_bytes;
  int32_t slot_bytes;                 /* bytes of one tensor's scalar block inside [scal_off, scal_off + scal_bytes) */
  int32_t n_sides, s0, s1, n_steps, n_tensors;
} ivx_plan_info;

typedef struct ivx_plan_step {
  int32_t kind;                       /* 0 image layout, 1 image space-to-depth, 2 conv, 3 max-pool, 4 unprojection, 5 anchor tail, 6 upsample,
                                         7 DCN columns, 8 average pool, 9 LayoutHead, 10 anchor-free candidates, 11 anchor-free tail */
  int32_t in, res, out, out2, fuse_out;   /* tensor ids, -1: none */
  int32_t fuse, side, join, tile, pio;
  int32_t amax_n, amax_in_n;
  int32_t n_extra_in, n_extra_out;    /* tensors read / written besides the five above (the anchor-free tail reads every level's candidates) */
  int32_t extra_in[12], extra_out[4];
  int64_t split, ws;                  /* ws: workspace bytes of this step's launches */
  int64_t amax_out, amax_in;          /* arena offsets of per-workgroup maxima (4 * amax_n bytes), -1: none */
  char name[48];                      /* layer name of a conv step, else "" */
} ivx_plan_step;

typedef struct ivx_plan_tensor {
  int64_t off, bytes;                 /* arena placement; off -1: not placed (caller-owned input, or outside the plan) */
  int64_t used;                       /* bytes the tensor's elements take (bytes is this, rounded up to 256) */
  int64_t slot;                       /* arena offset of the scalar block, -1: none */
  int32_t first, last;                /* the planner's live interval in steps (last == s1: kept to the end) */
  int32_t fmt, esz;
  int32_t caller_owned;               /* 1: an input of the plan, never placed in the arena */
  int32_t boundary;                   /* 1: FPN level 0, volume, valid mask, neck output, head output, levels, angle, layout */
} ivx_plan_tensor;

int ivx_model_plan_info(ivx_model *m, const char *what, int32_t B, int32_t V, int32_t H, int32_t W, ivx_plan_info *info);
int ivx_model_plan_step(ivx_model *m, const char *what, int32_t B, int32_t V, int32_t H, int32_t W, int32_t step, ivx_plan_step *rec);
int ivx_model_plan_tensor(ivx_model *m, const char *what, int32_t B, int32_t V, int32_t H, int32_t W, int32_t tensor, ivx_plan_tensor *rec);

#ifdef __cplusplus
}
#endif
#endif /* IMVOXEL_LAB_H_ */
