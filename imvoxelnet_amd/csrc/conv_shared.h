// Private to the convolution files: the launch parameters and the plan every translation unit of conv_igemm.hip, the host-only planner
// (conv_plan.cpp) and winograd.hip agree on, and the prototypes of the functions they call across translation units.
#ifndef IVX_CONV_SHARED_H_
#define IVX_CONV_SHARED_H_
#include "ivx_common.h"

struct ConvParams {
  const float *in, *wgt, *scale, *shift, *res;
  float *out;
  int B, D, H, W, Cin;
  int Cout, KD, KH, KW;
  int sd, sh, sw, pd, ph, pw;
  int Do, Ho, Wo;
  int M, K;
  int relu, res_mode, rH, rW;
  int kmode;  // 0: k = tap*Cin + ci   1: k = (ci/32)*taps*32 + tap*32 + ci%32
  int out_mode;       // 1: ConvTranspose(k2,s2) scatter: column n = tap*Cr + co goes to output voxel 2*(d,h,w) + tap
  int Cr;             // real output channels (Cout / 8 when out_mode == 1, else Cout)
  int res_after_act;  // add the residual after the activation (skip connections of the U-shaped necks)
  float post_scale;   // final multiplier (Atlas neck (x + y) / 2); 1 = none
  int ksplit;         // > 1: split-K, grid.y = slice; raw partial sums go to `partial` [ksplit][8*q_count*BM][Cout]
  float *partial;
  // M-tile range of this launch (LDS-DMA kernel): XCD x owns tiles [x*q_total, (x+1)*q_total); this launch covers the
  // q_count tiles starting at q_begin inside every XCD's range.  Whole problem: q_begin 0, q_count q_total.
  int q_total, q_begin, q_count, bm;
  int in_bf16;        // in / wgt are bf16 (LDS-DMA kernel only); accumulation is always fp32
  int out_bf16;       // out / res are bf16 (converted round-to-nearest-even in the epilogue)
  // grouped launch (LDS-DMA kernel, grid.z = group; the Winograd-domain GEMMs): group g reads in + g*g_in, wgt + g*g_w
  // and writes out + g*g_out (element strides; all 0 for an ordinary convolution)
  long long g_in, g_w, g_out;
  int groups;
  int narrow_epilogue;  // A/B knob: 1 = the one-channel-per-lane epilogue everywhere (ivx_conv_set_epilogue_mode)
  int in_fp8;         // in / wgt are OCP e4m3 bytes (v_mfma_f32_32x32x16_fp8_fp8); dequantisation is folded into scale[]
  int out_fp8;        // out / res are e4m3 bytes (saturating round-to-nearest-even at the store)
  float res_scale;    // multiplier of the residual (fp8 storage: res_scale_of_tensor / out_scale); 1 otherwise
  int in_pair;        // 1 / 2: in / wgt hold every fp32 value as a (hi, lo) bf16 / fp16 pair, 16-channel groups [hi16 | lo16] (IVX_*_PAIR); Cin and K
                      // count bf16 elements (2 per real channel); the K loop issues hi*hi + hi*lo + lo*hi per group
  // fp16-pair ACTIVATIONS with device-side power-of-two scales (ivx_pair_io, include/imvoxel.h): the 2-D trunk chained on the 16-bit
  // matrix cores without split passes -- the producing epilogue writes the operand its consumer reads.
  int pio;                       // any of the fields below is in use (in_pair == 2 kernels, the split-K reduction, the validation kernel)
  const float *in_scale_p;       // device: the scale the pair input was written with (NULL: 1); the accumulator is divided by it
  int out_pair, res_pair;        // out / res are IVX_F16_PAIR tensors [.., 2*Cout] (independently of each other)
  const float *res_scale_p;      // device: scale of the pair residual
  float *out_scale_p;            // device: receives the scale chosen for the output
  const unsigned *amax_in, *amax_res;   // device, IVX_AMAX_SLOTS words: bits of max |in| / max |res| (true values); out_pair only
  unsigned *amax_out;            // device, IVX_AMAX_SLOTS words the epilogue accumulates max |out| into (atomic max), or NULL
  float wbound, sbound;          // |out| <= amax_in * wbound + sbound (+ amax_res): max_co |scale[co]| * sum_k |w[co][k]| and max_co |shift[co]|
  // one device word copied by workgroup 0 of the launch (grouped Winograd-domain GEMMs: the filter scale travels to the workspace header
  // the output transform reads -- was a 4-byte hipMemcpyAsync, i.e. one more launch per neck layer); NULL = none
  const unsigned *cp_src;
  unsigned *cp_dst;
  // Row count of the launch on the DEVICE (conv_wino_halo_kernel / conv_wino_zblk_kernel: the compacted Winograd-domain GEMMs of a neck
  // whose background tiles are computed once, winograd.hip): *m_dev <= M rows are computed; the grid keeps the size of M rows and the
  // surplus workgroups return before their first barrier.  NULL = M.
  const int *m_dev;
  // Phase stagger of the first round of workgroups (pair-IO launches with a residual epilogue, run_conv): workgroups whose XCD-local index q has bit
  // stagger_shift set and q < stagger_first wait stagger_ticks (100 MHz) before their first request, so that the K loops of one half of the resident
  // workgroups overlap the epilogues of the other half for the rest of the launch.  0 ticks = off.
  int stagger_ticks, stagger_shift, stagger_first;
#ifdef IVX_CONV_TIMELINE
  unsigned long long *tl;        // debug build only (tools/conv_timeline.py): 8 words per workgroup of conv_igemm_v4_kernel's pair-IO path --
                                 // s_memrealtime (100 MHz) at entry, after the prologue barrier, after the K loop, at the end; HW_ID; XCC_ID
#endif
};

struct ConvPlan {
  int cfg;       // tile / kernel selector (see launch_one)
  int ksplit;    // > 1: split K over the whole problem (small outputs)
  int tail_ks;   // > 1: the last partial round of M-tiles runs as a second launch with K split tail_ks ways
  int q_total;   // M-tiles per XCD (LDS-DMA kernels)
  int qa;        // M-tiles per XCD covered by the first launch when tail_ks > 1
  int bm;        // tile rows of the chosen config
  int64_t ws_bytes;
};

// conv_igemm.hip, one launcher per IVX_CONV_TU (the tile numbers: conv_tiles.h)
int ivx_conv_launch_f32(ConvParams &p, const ConvPlan &pl, hipStream_t st);
int ivx_conv_launch_lowp(ConvParams &p, const ConvPlan &pl, hipStream_t st);
int ivx_conv_launch_pair_bf16(ConvParams &p, const ConvPlan &pl, hipStream_t st);
int ivx_conv_launch_pair_f16(ConvParams &p, const ConvPlan &pl, hipStream_t st);
int ivx_conv_launch_halo(ConvParams &p, int cfg, hipStream_t st);    // TU 5: the z-halo kernel of the Winograd-domain GEMMs (pair operands)
int ivx_conv_launch_fold4(ConvParams &p, const IvxWinoFold &f, int n2, hipStream_t st);    // TU 5: GEMM + output transform of F(4x4,3x3) fused
int ivx_conv_fold4_blocks(long long M, int Cout);

// conv_igemm.hip TU 0, called by winograd.hip: the Winograd-domain GEMMs as one grouped launch (see the definitions)
int ivx_conv_grouped_launch(const ivx_conv_desc *d, int groups, const float *in, long long g_in, const float *wgt, long long g_w,
                            float *out, long long g_out, hipStream_t st, const unsigned *cp_src, unsigned *cp_dst, const int *m_dev);
int ivx_conv_grouped_rows_dev_ok(const ivx_conv_desc *d, int groups);
int ivx_conv_grouped_fold4(const ivx_conv_desc *d, int groups, const float *in, long long g_in, const float *wgt, long long g_w, const IvxWinoFold *f,
                           hipStream_t st);
// fold4w.hip
int ivx_conv_launch_fold4w(const _Float16 *V, long long vs, const _Float16 *U, long long us, int M, int Cin_stored, int Cout, int Z, const IvxWinoFold &f,
                           hipStream_t st);

#endif   // IVX_CONV_SHARED_H_
