// Channels-last implicit-GEMM convolution on the CDNA4 matrix cores: exact fp32 (default) or bf16 storage.
//
//   GEMM view:  M = B*Do*Ho*Wo output positions, N = Cout, K = KD*KH*KW*Cin; im2col is done on the fly.
//   MFMA:       v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate == an fmaf chain, 64 cyc/SIMD), or
//               v_mfma_f32_32x32x16_bf16 for the optional bf16 storage mode (fp32 accumulate).
//   Workgroup:  256 threads = 4 wave64, block tile BM x BN = (WR*TM*32) x (WC*TN*32),
//               each wave owns TM x TN MFMA tiles of 32x32 (16 accumulator VGPRs each).
//   Kernels:    conv_igemm_v4_kernel (production: buffer loads with hardware zero-fill, LDS-DMA staging, XOR
//               swizzled LDS rows, chunk-major K order, split-K / grid-tail plan) -- see its header below;
//               conv_igemm_f32_kernel (generic: global loads into registers one slab ahead, ds_write_b128 into
//               padded 144-byte LDS rows, 64-bit addressing) for tensors >= 2 GiB or kernel extents > 8;
//               conv_naive_f32_kernel (validation only).
//   Fragments:  lane l reads 16 bytes of row (l & 31); half-wave h = l>>5 takes the k-chunk 2*kk + h, so one
//               ds_read_b128 per operand feeds 4 fp32 MFMAs (or 1 bf16 MFMA).  The k permutation is the same for A
//               and B, so the sum over k is unchanged.
//   Epilogue:   y = acc*scale[n] + shift[n] (+ residual, same-shape or nearest-upsampled) (ReLU) ..., stored with
//               32 consecutive lanes on 32 consecutive channels (128-byte rows).
//   Grid:       M tiles with an XCD-aware remap (block b runs on XCD b % 8; every XCD gets a contiguous range of
//               M tiles so halo re-reads hit its own L2).
//
// Reference call sites replaced: see include/imvoxel.h (ivx_conv_fwd).
#include "conv_plan.h"      // ConvParams / ConvPlan and the cross-unit prototypes (conv_shared.h), the tile table (conv_tiles.h), the planner
#include "../../include/imvoxel_lab.h"
#include <string.h>

// This file is compiled six times (imvoxelnet_amd/_build.py), each translation unit instantiating one family of the LDS-DMA kernel, so that
// the families build in parallel:  IVX_CONV_TU 0 = the host side, the generic / naive / reduce kernels;  1 = fp32;  2 = bf16 and e4m3;
// 3 = bf16 (hi, lo) pair operands;  4 = fp16 pair operands;  5 = the z-halo kernel (conv_wino_halo_kernel).
// Which tile number is which instantiation: conv_tiles.h (every launch switch below expands its rows).  Which number a launch takes:
// conv_plan.cpp (host only); TU 0 keeps fill_params, run_conv, conv_dispatch and the entry points.
#ifndef IVX_CONV_TU
#define IVX_CONV_TU 0
#endif

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// What a wave needs of the pair-IO state: multipliers of the accumulator / the residual (exact: powers of two) and the output scale.
struct PairIO { float inv_in, inv_res, s_out; bool sat; float post; };      // post = ConvParams::post_scale (carried here: see conv_igemm_v4_kernel)
// Every wave computes the same values from the same device words (no communication): the output scale comes from a BOUND of the
// output -- |out| <= max|in| * wbound + sbound + max|res| with the MEASURED maxima of the operands, which their producers left in the
// amax slots -- so nothing has to pass over the output before it is written as (hi, lo) halves.  A bound that is loose by a factor L
// costs nothing up to L = 2^17: a value's error is max(2^-22 |x|, 2^-25 / s), i.e. relative to the tensor's maximum max(2^-22, 2^-39 L).
__device__ __forceinline__ PairIO conv_pair_io(const ConvParams &p) {
  PairIO io = {1.0f, 1.0f, 1.0f, false, p.post_scale};
  if (p.in_scale_p) io.inv_in = 1.0f / *p.in_scale_p;
  if (p.res_pair && p.res_scale_p) io.inv_res = 1.0f / *p.res_scale_p;
  if (p.out_pair) {
    const int lane = threadIdx.x & 63;
    float a = p.amax_in ? __uint_as_float(p.amax_in[lane]) : 0.f;
    float r = (p.amax_res && p.res_mode) ? __uint_as_float(p.amax_res[lane]) : 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      a = fmaxf(a, __shfl_xor(a, o));
      r = fmaxf(r, __shfl_xor(r, o));
    }
    const float bound = (a * p.wbound + p.sbound + r) * fabsf(p.post_scale) * 1.001f;
    io.s_out = ivx_pow2_scale(bound);
    // a non-finite bound (an Inf / NaN among the operands) says nothing about the finite outputs: fixed scale 2^-8 and a saturating
    // split, so that the damage stays where fp32 arithmetic keeps it instead of the whole tensor overflowing to Inf
    io.sat = !(bound < 3.0e38f);
    if (io.sat) io.s_out = 0.00390625f;
  }
  return io;
}
// element offset (in halves) of channel n of row `row` (C channels) inside an IVX_F16_PAIR tensor: hi; lo is 16 further
__device__ __forceinline__ size_t pair_off(size_t row, int n, int C) { return row * (size_t)(2 * C) + (size_t)((n >> 4) * 32 + (n & 15)); }

struct fp8_t { unsigned char v; };       // storage element of the fp8 instantiation (size 1)
typedef long i64_t;

__device__ __forceinline__ float fp8_to_f32(unsigned char b) { return __builtin_amdgcn_cvt_f32_fp8((int)b, 0); }
// saturating e4m3 conversion of two floats -> low / high byte pair; +-inf saturates, NaN stays NaN.  The clamp alone does not keep a
// NaN: fminf(fmaxf(x, -448), 448) compiles to a median of three, which returns the smaller of the other two for a NaN operand, and the
// byte stored was 0xFE (-448) -- so a value that is not equal to itself goes to the conversion unclamped.
__device__ __forceinline__ float fp8_clamp(float x) {
  const float c = __builtin_fminf(__builtin_fmaxf(x, -448.f), 448.f);
  return x != x ? x : c;
}
__device__ __forceinline__ unsigned int f32x2_to_fp8(float a, float b) {
  a = fp8_clamp(a);
  b = fp8_clamp(b);
  return (unsigned int)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false) & 0xffffu;
}

__device__ __forceinline__ float conv_ld_res(const ConvParams &p, size_t i) {
  if (p.res_pair) {      // (generic one-element paths only: split-K reduction, validation kernel); the caller multiplies by 1 / scale
    const _Float16 *r = reinterpret_cast<const _Float16 *>(p.res) + pair_off(i / p.Cout, (int)(i % p.Cout), p.Cout);
    return (float)r[0] + (float)r[16];
  }
  if (p.out_fp8) return fp8_to_f32(reinterpret_cast<const unsigned char *>(p.res)[i]);
  return p.out_bf16 ? (float)reinterpret_cast<const __bf16 *>(p.res)[i] : p.res[i];
}
__device__ __forceinline__ void conv_st_out(const ConvParams &p, size_t i, float v) {
  if (p.out_pair) {      // v is already multiplied by the output scale
    _Float16 *o = reinterpret_cast<_Float16 *>(p.out) + pair_off(i / p.Cout, (int)(i % p.Cout), p.Cout);
    const _Float16 h = (_Float16)v;
    o[0] = h;
    o[16] = (_Float16)(v - (float)h);
    return;
  }
  if (p.out_fp8)
    reinterpret_cast<unsigned char *>(p.out)[i] = (unsigned char)(f32x2_to_fp8(v, 0.f) & 0xffu);
  else if (p.out_bf16)
    reinterpret_cast<__bf16 *>(p.out)[i] = (__bf16)v;
  else
    p.out[i] = v;
}

#define IVX_BK 32
#define IVX_LDK 36

// Row base (in floats) of the nearest-upsampled residual for output row m (res_mode 2; FPN top-down,
// F.interpolate(mode='nearest', size=...): src = min(floor(dst * in/out), in-1), identity / >>1 when exact).
__device__ __noinline__ size_t res2_row_base(int m, int Ho, int Wo, int rH, int rW, int Cout) {
  const int ow = m % Wo;
  const int t = m / Wo;
  const int oh = t % Ho;
  const int b = t / Ho;  // Do == 1 for this mode
  int sh_ = (Ho == rH) ? oh : (Ho == 2 * rH ? (oh >> 1) : (int)floorf(oh * ((float)rH / Ho)));
  int sw_ = (Wo == rW) ? ow : (Wo == 2 * rW ? (ow >> 1) : (int)floorf(ow * ((float)rW / Wo)));
  sh_ = sh_ < rH - 1 ? sh_ : rH - 1;
  sw_ = sw_ < rW - 1 ? sw_ : rW - 1;
  return (((size_t)b * rH + sh_) * rW + sw_) * Cout;
}

// y = act(acc*scale + shift [+ res]) [+ res] [* post_scale] for one output element; `oidx` is its flat offset.
__device__ __forceinline__ float conv_finish(const ConvParams &p, float acc, float sc, float sf, size_t ridx, float rscale) {
  float v = acc * sc + sf;
  // one fused multiply-add, spelled out so that every epilogue variant rounds the same way; res_scale is 1 outside the fp8 mode,
  // where fma(r, 1, v) == v + r exactly
  if (p.res_mode && !p.res_after_act) v = __builtin_fmaf(conv_ld_res(p, ridx), rscale, v);
  if (p.relu) v = v > 0.f ? v : 0.f;
  if (p.res_mode && p.res_after_act) v = __builtin_fmaf(conv_ld_res(p, ridx), rscale, v);
  return v * p.post_scale;
}
__device__ __forceinline__ float conv_finish(const ConvParams &p, float acc, float sc, float sf, size_t ridx) {
  return conv_finish(p, acc, sc, sf, ridx, p.res_scale);
}

// Flat output offset of (row m, column n) for out_mode 1 (ConvTranspose3d kernel 2, stride 2): row m is the INPUT
// voxel (b,d,h,w) (the GEMM is a 1x1x1 conv), column n = ((a*2+e)*2+f)*Cr + co.
__device__ __noinline__ size_t up2_row_base(int m, int D, int H, int W, int Cr) {
  const int w = m % W;
  int t = m / W;
  const int h = t % H;
  t /= H;
  const int d = t % D;
  const int b = t / D;
  return ((((size_t)b * 2 * D + 2 * d) * 2 * H + 2 * h) * 2 * W + 2 * w) * Cr;
}

template <int TM, int TN>
__device__ __forceinline__ void conv_epilogue(const ConvParams &p, f32x16 (&acc)[TM][TN], int m0, int n0, int wr, int wc,
                                              int lane, size_t obase = 0) {
  const int col_l = lane & 31, hh = lane >> 5;
  float sc[TN], sf[TN];
  int nn[TN];
  size_t coff[TN];  // out_mode 1: per-column offset inside the 2x2x2 output cell
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    nn[j] = n0 + (wc * TN + j) * 32 + col_l;
    const bool nok = nn[j] < p.Cout;
    int ch = nn[j];
    coff[j] = 0;
    if (p.out_mode == 1 && nok) {
      const int tap = nn[j] / p.Cr;
      ch = nn[j] - tap * p.Cr;
      const int a = tap >> 2, e = (tap >> 1) & 1, f = tap & 1;
      coff[j] = (((size_t)a * 2 * p.H + e) * 2 * p.W + f) * p.Cr + ch;
    }
    sc[j] = (nok && p.scale) ? p.scale[ch] : 1.0f;
    sf[j] = (nok && p.shift) ? p.shift[ch] : 0.0f;
  }
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + (wr * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
      if (m >= p.M) continue;
      if (p.out_mode == 1) {
        const size_t ob = up2_row_base(m, p.D, p.H, p.W, p.Cr);
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          if (nn[j] >= p.Cout) continue;
          conv_st_out(p, ob + coff[j], conv_finish(p, acc[i][j][r], sc[j], sf[j], ob + coff[j]));
        }
        continue;
      }
      size_t rbase = (size_t)m * p.Cout;
      if (p.res_mode == 2) rbase = res2_row_base(m, p.Ho, p.Wo, p.rH, p.rW, p.Cout);
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        if (nn[j] >= p.Cout) continue;
        conv_st_out(p, obase + (size_t)m * p.Cout + nn[j], conv_finish(p, acc[i][j][r], sc[j], sf[j], rbase + nn[j]));
      }
    }
  }
}

// Wide-store epilogue of the LDS-DMA kernel (fp32 output, plain layout, Cout % 4 == 0; residual: none, same shape, or the
// nearest-upsampled coarser FPN level).
// The MFMA accumulator layout gives a lane ONE channel of 16 rows, so the direct epilogue above issues 16 dword stores per
// 32x32 tile and lane (64 per wave for a 64x64 quadrant): the store issue, not the bytes, sets its duration, and while a
// wave sits in it its SIMD runs with one MFMA wave fewer.  With short K (the Winograd-domain GEMMs: K = 192 .. 768, the
// 1x1 layers of the 2-D trunk) that is the largest loss of the kernel.  Here each 32x32 tile is transposed through the
// wave's own slice of the (now idle) staging LDS -- 16 ds_write_b32, 4 ds_read_b128 -- so that a lane owns 4 consecutive
// channels: the tile leaves as 4 dwordx4 stores per lane (8 rows x 128 bytes per wave instruction, whole cache lines), the
// residual arrives as 4 dwordx4 loads, scale / shift as one float4 each.  No barrier is needed: after the K loop's last
// barrier every wave holds its remaining fragments in registers, and a wave touches only its own 4 KB slice.
template <int TM, int TN>
__device__ __forceinline__ void conv_epilogue_wide(const ConvParams &p, f32x16 (&acc)[TM][TN], int m0, int n0, int wr, int wc,
                                                   int lane, float *stage, size_t obase) {
  const int col_l = lane & 31, hh = lane >> 5;
  const int rrow = lane >> 3, c4 = (lane & 7) * 4;     // read side: row rrow + 8q, channels c4 .. c4+3 of the tile
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int nb = n0 + (wc * TN + j) * 32 + c4;
    const bool nok = nb < p.Cout;                        // Cout % 4 == 0: a 4-channel chunk is inside or outside as a whole
    f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sf = {0.f, 0.f, 0.f, 0.f};
    if (nok && p.scale) sc = *reinterpret_cast<const f32x4 *>(p.scale + nb);
    if (nok && p.shift) sf = *reinterpret_cast<const f32x4 *>(p.shift + nb);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) stage[((r & 3) + 8 * (r >> 2) + 4 * hh) * 32 + col_l] = acc[i][j][r];
      const int mb = m0 + (wr * TM + i) * 32 + rrow;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 v = *reinterpret_cast<const f32x4 *>(stage + (rrow + 8 * q) * 32 + c4);
        const int m = mb + 8 * q;
        if (m < p.M && nok) {
          const size_t o = (size_t)m * p.Cout + nb;
          v = v * sc + sf;
          f32x4 rr = {0.f, 0.f, 0.f, 0.f};
          if (p.res_mode == 2) rr = *reinterpret_cast<const f32x4 *>(p.res + res2_row_base(m, p.Ho, p.Wo, p.rH, p.rW, p.Cout) + nb);
          else if (p.res_mode) rr = *reinterpret_cast<const f32x4 *>(p.res + o);
          if (p.res_mode && !p.res_after_act) v += rr;
          if (p.relu) {
            v[0] = v[0] > 0.f ? v[0] : 0.f; v[1] = v[1] > 0.f ? v[1] : 0.f;
            v[2] = v[2] > 0.f ? v[2] : 0.f; v[3] = v[3] > 0.f ? v[3] : 0.f;
          }
          if (p.res_mode && p.res_after_act) v += rr;
          v *= p.post_scale;
          *reinterpret_cast<f32x4 *>(p.out + obase + o) = v;
        }
      }
    }
  }
}

// Pair-IO variant of the wide epilogue (in_pair == 2 kernels; ConvParams::pio): the accumulator is divided by the input's scale, the
// residual is fp32 or an fp16 (hi, lo) pair tensor with its own scale, the output is fp32 or a pair tensor written with the scale of
// conv_pair_io -- a lane's 4 channels are 8 bytes of hi halves and, 32 bytes further, 8 bytes of lo halves -- and the maximum of the
// stored values (true values, before the output scale) goes to the amax slots for the next layer's bound.
// epilogue of 4 consecutive channels nb .. nb + 3 of output row m (pair IO): v = the accumulators; returns max |stored value|
typedef unsigned u32x4r __attribute__((ext_vector_type(4)));
typedef unsigned u32x2r __attribute__((ext_vector_type(2)));
// the residual of 4 consecutive channels nb .. nb + 3 of row `row` as it lies in memory: 4 floats, or (pair tensor) 8 bytes of hi halves
// and, 32 bytes further, 8 bytes of lo halves
__device__ __forceinline__ u32x4r conv_pio_res_load(const ConvParams &p, const size_t row, const int nb) {
  if (p.res_pair) {
    const _Float16 *rp = reinterpret_cast<const _Float16 *>(p.res) + pair_off(row, nb, p.Cout);
    const u32x2r h = *reinterpret_cast<const u32x2r *>(rp), l = *reinterpret_cast<const u32x2r *>(rp + 16);
    return u32x4r{h.x, h.y, l.x, l.y};
  }
  return *reinterpret_cast<const u32x4r *>(p.res + row * (size_t)p.Cout + nb);
}
__device__ __forceinline__ f32x4 conv_pio_res_decode(const ConvParams &p, const PairIO io, const u32x4r raw) {
  typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
  f32x4 rr;
  if (p.res_pair) {
    const f16x4 rh = __builtin_bit_cast(f16x4, u32x2r{raw.x, raw.y}), rl = __builtin_bit_cast(f16x4, u32x2r{raw.z, raw.w});
#pragma unroll
    for (int e = 0; e < 4; ++e) rr[e] = ((float)rh[e] + (float)rl[e]) * io.inv_res;
  } else {
    rr = __builtin_bit_cast(f32x4, raw);
  }
  return rr;
}
// v = the accumulators, rr = the decoded residual (zeros without one); stores the 4 channels, returns max |stored value|
__device__ __forceinline__ float conv_pio_finish4_rr(const ConvParams &p, const PairIO io, f32x4 v, const int m, const int nb, const f32x4 sc, const f32x4 sf,
                                                     const f32x4 rr) {
  typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
  v = v * sc + sf;
  if (p.res_mode && !p.res_after_act) v += rr;
  if (p.relu) {
    v[0] = v[0] > 0.f ? v[0] : 0.f; v[1] = v[1] > 0.f ? v[1] : 0.f;
    v[2] = v[2] > 0.f ? v[2] : 0.f; v[3] = v[3] > 0.f ? v[3] : 0.f;
  }
  if (p.res_mode && p.res_after_act) v += rr;
  v *= io.post;
  if (p.out_pair) {
    f16x4 h, l;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float y = v[e] * io.s_out;
      if (io.sat) y = (y > 65504.f && y < __builtin_inff()) ? 65504.f : ((y < -65504.f && y > -__builtin_inff()) ? -65504.f : y);
      h[e] = (_Float16)y;
      l[e] = (_Float16)(y - (float)h[e]);
    }
    _Float16 *op = reinterpret_cast<_Float16 *>(p.out) + pair_off((size_t)m, nb, p.Cout);
    *reinterpret_cast<f16x4 *>(op) = h;
    *reinterpret_cast<f16x4 *>(op + 16) = l;
  } else {
    *reinterpret_cast<f32x4 *>(p.out + (size_t)m * p.Cout + nb) = v;
  }
  return fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3])));
}
__device__ __forceinline__ float conv_pio_finish4(const ConvParams &p, const PairIO io, f32x4 v, const int m, const int nb, const f32x4 sc, const f32x4 sf) {
  f32x4 rr = {0.f, 0.f, 0.f, 0.f};
  if (p.res_mode) {
    const size_t row = p.res_mode == 2 ? res2_row_base(m, p.Ho, p.Wo, p.rH, p.rW, 1) : (size_t)m;
    rr = conv_pio_res_decode(p, io, conv_pio_res_load(p, row, nb));
  }
  return conv_pio_finish4_rr(p, io, v, m, nb, sc, sf, rr);
}

// Measured and removed (round 4, profiles/r04_pio_epilogue_prefetch_ab.md): requesting the residual of block b + 2 before block b is
// transposed and stored (two blocks = 32 registers in flight) so that a wave waits for one memory round trip instead of TM * TN --
// the 128 x 128 tile went from 5 to 26 spilled registers and every residual layer got SLOWER (64 -> 256 at 50 views 0.67 -> 0.77 ms,
// 128 -> 512 0.41 -> 0.45, 256 -> 1024 0.27 -> 0.29): the serial load -> store chain of a wave is hidden by the other fifteen waves of
// the CU; what bounds these layers is not the residual's latency.  (A one-block-ahead form with the request issued before the block is
// consumed: 55 spilled registers, 0.68 -> 1.11 ms.)
// RPF (round 5): the residual of the whole tile was requested BEFORE the K loop (conv_pio_res_prefetch: raw bits, 4 dwords per lane, block
// and pass -- 64 registers for the 128 x 128 tile) and is decoded here; taken when p.res_mode == 1, everything else goes the path above.
template <int TM, int TN>
__device__ __forceinline__ void conv_pio_res_prefetch(const ConvParams &p, u32x4r (&rraw)[TM][TN][4], int m0, int n0, int wr, int wc, int lane) {
  const int rrow = lane >> 3, c4 = (lane & 7) * 4;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int nb = n0 + (wc * TN + j) * 32 + c4;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int m = m0 + (wr * TM + i) * 32 + rrow + 8 * q;
        rraw[i][j][q] = u32x4r{0u, 0u, 0u, 0u};
        if (m < p.M && nb < p.Cout) rraw[i][j][q] = conv_pio_res_load(p, (size_t)m, nb);
      }
  }
}
// The maximum is committed ONCE PER WORKGROUP (round 5): every wave leaves its maximum in the first word of its own staging slice, one
// barrier, wave 0 reduces and issues the atomic.  The 64 slots of a tensor lie in two cache lines, so atomics on different slots still
// serialise at one memory channel; with one atomic per WAVE the 960 .. 3840 waves of a trunk launch whose slots had just been zeroed
// queued there and the last workgroups of the launch waited 10 - 20 us in their epilogue (workgroup timelines inside the model,
// profiles/r05_trunk_wg_timeline.md; isolated launches do not show it: their slots already hold the maximum and the read skips the atomic).
template <int TM, int TN, int RPF = 0>
__device__ __forceinline__ void conv_epilogue_wide_pio(const ConvParams &p, const PairIO io, f32x16 (&acc)[TM][TN], int m0, int n0, int wr, int wc,
                                                       int lane, float *stage, int wid, int nw, const u32x4r (*rraw)[TN][4] = nullptr) {
  const int col_l = lane & 31, hh = lane >> 5;
  const int rrow = lane >> 3, c4 = (lane & 7) * 4;
  float omax = 0.f;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int nb = n0 + (wc * TN + j) * 32 + c4;
    const bool nok = nb < p.Cout;
    f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sf = {0.f, 0.f, 0.f, 0.f};
    if (nok && p.scale) sc = *reinterpret_cast<const f32x4 *>(p.scale + nb);
    if (nok && p.shift) sf = *reinterpret_cast<const f32x4 *>(p.shift + nb);
    sc *= io.inv_in;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) stage[((r & 3) + 8 * (r >> 2) + 4 * hh) * 32 + col_l] = acc[i][j][r];
      const int mb = m0 + (wr * TM + i) * 32 + rrow;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(stage + (rrow + 8 * q) * 32 + c4);
        const int m = mb + 8 * q;
        if (m < p.M && nok) {
          if (RPF && p.res_mode == 1) omax = fmaxf(omax, conv_pio_finish4_rr(p, io, v, m, nb, sc, sf, conv_pio_res_decode(p, io, rraw[i][j][q])));
          else omax = fmaxf(omax, conv_pio_finish4(p, io, v, m, nb, sc, sf));
        }
      }
    }
  }
  if (p.amax_out) {        // (uniform over the workgroup)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) omax = fmaxf(omax, __shfl_xor(omax, o));
    if (lane == 0) stage[0] = omax;
    __syncthreads();
    if (wid == 0) ivx_amax_commit(p.amax_out, lane < nw ? stage[lane * 1024] : 0.f, (int)blockIdx.x);
  }
}

// bf16-output variant of the wide epilogue (Cout % 8 == 0).  The one-channel-per-lane epilogue stores 2 bytes per lane --
// sub-dword writes, which the memory side handles as read-modify-write: the Cout-expanding 1x1 layers of the bf16 trunk ran
// at ~1.1 TB/s of algorithmic traffic.  Here NJ (2 when TN is even, else 1) 32x32 tiles are transposed through the wave's LDS
// slice so that a lane owns 8 consecutive channels of a row: the tile pair leaves as 16-byte stores (8 bf16), 8 lanes to a
// 128-byte row segment; the residual arrives as 16-byte loads.  Rounding is the same round-to-nearest-even conversion.
template <int TM, int TN, int NJ>
__device__ __forceinline__ void conv_epilogue_wide_bf16(const ConvParams &p, f32x16 (&acc)[TM][TN], int m0, int n0, int wr, int wc,
                                                        int lane, float *stage, size_t obase) {
  static_assert(TN % NJ == 0, "tile pairs");
  constexpr int LPR = 4 * NJ;        // lanes per row: 8 channels each over NJ*32 channels
  constexpr int RPP = 64 / LPR;      // rows per pass
  const int col_l = lane & 31, hh = lane >> 5;
  const int rrow = lane / LPR, c8 = (lane % LPR) * 8;
  const float *rd = stage + (c8 >> 5) * 1024 + (c8 & 31);
  __bf16 *outp = reinterpret_cast<__bf16 *>(p.out);
  const __bf16 *resp = reinterpret_cast<const __bf16 *>(p.res);
#pragma unroll
  for (int j = 0; j < TN; j += NJ) {
    const int nb = n0 + (wc * TN + j) * 32 + c8;
    const bool nok = nb < p.Cout;                        // Cout % 8 == 0: an 8-channel chunk is inside or outside as a whole
    f32x4 sc0 = {1.f, 1.f, 1.f, 1.f}, sc1 = sc0, sf0 = {0.f, 0.f, 0.f, 0.f}, sf1 = sf0;
    if (nok && p.scale) { sc0 = *reinterpret_cast<const f32x4 *>(p.scale + nb); sc1 = *reinterpret_cast<const f32x4 *>(p.scale + nb + 4); }
    if (nok && p.shift) { sf0 = *reinterpret_cast<const f32x4 *>(p.shift + nb); sf1 = *reinterpret_cast<const f32x4 *>(p.shift + nb + 4); }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
        for (int r = 0; r < 16; ++r) stage[jj * 1024 + ((r & 3) + 8 * (r >> 2) + 4 * hh) * 32 + col_l] = acc[i][j + jj][r];
      const int mb = m0 + (wr * TM + i) * 32 + rrow;
#pragma unroll
      for (int q = 0; q < 32 / RPP; ++q) {
        f32x4 v0 = *reinterpret_cast<const f32x4 *>(rd + (rrow + RPP * q) * 32);
        f32x4 v1 = *reinterpret_cast<const f32x4 *>(rd + (rrow + RPP * q) * 32 + 4);
        const int m = mb + RPP * q;
        if (m < p.M && nok) {
          const size_t o = (size_t)m * p.Cout + nb;
          v0 = v0 * sc0 + sf0;
          v1 = v1 * sc1 + sf1;
          f32x4 r0 = {0.f, 0.f, 0.f, 0.f}, r1 = r0;
          if (p.res_mode) {
            const size_t ro = p.res_mode == 2 ? res2_row_base(m, p.Ho, p.Wo, p.rH, p.rW, p.Cout) + nb : o;
            const bf16x8 rb = *reinterpret_cast<const bf16x8 *>(resp + ro);
#pragma unroll
            for (int e = 0; e < 4; ++e) { r0[e] = (float)rb[e] * p.res_scale; r1[e] = (float)rb[e + 4] * p.res_scale; }
          }
          if (p.res_mode && !p.res_after_act) { v0 += r0; v1 += r1; }
          if (p.relu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { v0[e] = v0[e] > 0.f ? v0[e] : 0.f; v1[e] = v1[e] > 0.f ? v1[e] : 0.f; }
          }
          if (p.res_mode && p.res_after_act) { v0 += r0; v1 += r1; }
          v0 *= p.post_scale;
          v1 *= p.post_scale;
          bf16x8 ob;
#pragma unroll
          for (int e = 0; e < 4; ++e) { ob[e] = (__bf16)v0[e]; ob[e + 4] = (__bf16)v1[e]; }
          *reinterpret_cast<bf16x8 *>(outp + obase + o) = ob;
        }
      }
    }
  }
}

// e4m3-output variant (Cout % 16 == 0): a lane owns 16 consecutive channels of a row -- one 16-byte store of 16 fp8 values,
// 4 lanes to a 64-byte row segment of a tile pair; the residual (e4m3, its own scale) arrives as one 16-byte load.
template <int TM, int TN, int NJ>
__device__ __forceinline__ void conv_epilogue_wide_fp8(const ConvParams &p, f32x16 (&acc)[TM][TN], int m0, int n0, int wr, int wc,
                                                       int lane, float *stage, size_t obase) {
  static_assert(TN % NJ == 0, "tile pairs");
  constexpr int LPR = 2 * NJ;        // lanes per row: 16 channels each over NJ*32 channels
  constexpr int RPP = 64 / LPR;      // rows per pass
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  const int col_l = lane & 31, hh = lane >> 5;
  const int rrow = lane / LPR, c16 = (lane % LPR) * 16;
  const float *rd = stage + (c16 >> 5) * 1024 + (c16 & 31);
  unsigned char *outp = reinterpret_cast<unsigned char *>(p.out);
  const unsigned char *resp = reinterpret_cast<const unsigned char *>(p.res);
#pragma unroll
  for (int j = 0; j < TN; j += NJ) {
    const int nb = n0 + (wc * TN + j) * 32 + c16;
    const bool nok = nb < p.Cout;                        // Cout % 16 == 0
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
        for (int r = 0; r < 16; ++r) stage[jj * 1024 + ((r & 3) + 8 * (r >> 2) + 4 * hh) * 32 + col_l] = acc[i][j + jj][r];
      const int mb = m0 + (wr * TM + i) * 32 + rrow;
#pragma unroll
      for (int q = 0; q < 32 / RPP; ++q) {
        const int m = mb + RPP * q;
        if (!(m < p.M && nok)) continue;
        const size_t o = (size_t)m * p.Cout + nb;
        u32x4 rb = {0u, 0u, 0u, 0u};
        if (p.res_mode) rb = *reinterpret_cast<const u32x4 *>(resp + (p.res_mode == 2 ? res2_row_base(m, p.Ho, p.Wo, p.rH, p.rW, p.Cout) + nb : o));
        u32x4 ob;
        // four channels at a time (scale / shift come from the cache again for every row: keeps the live registers low -- the
        // first version held 16 scales + 16 shifts + 16 values + 16 residuals beside the 64 accumulators and spilled 75 VGPRs)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          f32x4 v = *reinterpret_cast<const f32x4 *>(rd + (rrow + RPP * q) * 32 + 4 * w);
          f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sf = {0.f, 0.f, 0.f, 0.f};
          if (p.scale) sc = *reinterpret_cast<const f32x4 *>(p.scale + nb + 4 * w);
          if (p.shift) sf = *reinterpret_cast<const f32x4 *>(p.shift + nb + 4 * w);
          v = v * sc + sf;
          f32x4 r = {0.f, 0.f, 0.f, 0.f};
          if (p.res_mode) {
            const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)rb[w], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)rb[w], true);
            r[0] = lo[0]; r[1] = lo[1]; r[2] = hi[0]; r[3] = hi[1];
          }
          if (p.res_mode && !p.res_after_act) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaf(r[e], p.res_scale, v[e]);     // as conv_finish
          }
          if (p.relu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
          }
          if (p.res_mode && p.res_after_act) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaf(r[e], p.res_scale, v[e]);
          }
          v *= p.post_scale;
          ob[w] = f32x2_to_fp8(v[0], v[1]) | (f32x2_to_fp8(v[2], v[3]) << 16);
        }
        *reinterpret_cast<u32x4 *>(outp + obase + o) = ob;
      }
    }
  }
}

template <int TM, int TN, int WR, int WC>
__global__ __launch_bounds__(256) void conv_igemm_f32_kernel(const ConvParams p) {
  constexpr int BM = WR * TM * 32, BN = WC * TN * 32;
  constexpr int AR = BM / 32, BR = BN / 32;
  static_assert(WR * WC == 4, "4 waves per workgroup");
  __shared__ __attribute__((aligned(16))) float smem[2 * (BM + BN) * IVX_LDK];
  float *As = smem;
  float *Bs = smem + 2 * BM * IVX_LDK;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid / WC, wc = wid % WC;

  // XCD-aware bijective remap of the M-tile index.
  int bid = blockIdx.x;
  {
    const int nb = gridDim.x;
    const int q = nb >> 3, r = nb & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const int m0 = bid * BM;
  const int n0 = blockIdx.y * BN;

  // ---- loader state -------------------------------------------------------------------------
  const int cc = tid & 7;   // 16-byte chunk column inside the slab
  const int lr = tid >> 3;  // 0..31
  int a_bd[AR], a_id[AR], a_ih[AR], a_iw[AR];
#pragma unroll
  for (int j = 0; j < AR; ++j) {
    const int m = m0 + lr + 32 * j;
    if (m < p.M) {
      const int ow = m % p.Wo;
      int t = m / p.Wo;
      const int oh = t % p.Ho;
      t /= p.Ho;
      const int od = t % p.Do;
      const int b = t / p.Do;
      a_bd[j] = b * p.D;
      a_id[j] = od * p.sd - p.pd;
      a_ih[j] = oh * p.sh - p.ph;
      a_iw[j] = ow * p.sw - p.pw;
    } else {
      a_bd[j] = 0;
      a_id[j] = -(1 << 28);  // fails the bounds test for every tap
      a_ih[j] = 0;
      a_iw[j] = 0;
    }
  }
  // per-thread k cursor: k4 = slab*32 + cc*4 = tap*Cin + kc
  int k4 = cc * 4;
  int kc, ka, ke, kf;
  if (p.kmode == 1) {  // chunk-major: slab s = (channel chunk s / taps, tap s % taps)
    kc = cc * 4;
    ka = ke = kf = 0;
  } else {
    const int tap = k4 / p.Cin;
    kc = k4 - tap * p.Cin;
    kf = tap % p.KW;
    const int t2 = tap / p.KW;
    ke = t2 % p.KH;
    ka = t2 / p.KH;
  }
  const int S = (p.K + IVX_BK - 1) / IVX_BK;

  f32x4 ra[AR], rb[BR];
  auto load_slab = [&]() {
    const bool kok = k4 < p.K;
#pragma unroll
    for (int j = 0; j < AR; ++j) {
      const int id = a_id[j] + ka, ih = a_ih[j] + ke, iw = a_iw[j] + kf;
      const bool ok = kok && (unsigned)id < (unsigned)p.D && (unsigned)ih < (unsigned)p.H &&
                      (unsigned)iw < (unsigned)p.W;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (ok) {
        const size_t off = (((size_t)(a_bd[j] + id) * p.H + ih) * p.W + iw) * (size_t)p.Cin + kc;
        v = *reinterpret_cast<const f32x4 *>(p.in + off);
      }
      ra[j] = v;
    }
#pragma unroll
    for (int j = 0; j < BR; ++j) {
      const int n = n0 + lr + 32 * j;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (kok && n < p.Cout) v = *reinterpret_cast<const f32x4 *>(p.wgt + (size_t)n * p.K + k4);
      rb[j] = v;
    }
  };
  auto advance_k = [&]() {
    k4 += IVX_BK;
    if (p.kmode == 1) {  // next tap of the same 32-channel chunk; after the last tap move to the next chunk
      if (++kf == p.KW) {
        kf = 0;
        if (++ke == p.KH) {
          ke = 0;
          if (++ka == p.KD) {
            ka = 0;
            kc += IVX_BK;
          }
        }
      }
      return;
    }
    kc += IVX_BK;
    while (kc >= p.Cin) {
      kc -= p.Cin;
      if (++kf == p.KW) {
        kf = 0;
        if (++ke == p.KH) {
          ke = 0;
          ++ka;
        }
      }
    }
  };
  auto store_slab = [&](int buf) {
    float *Ab = As + buf * BM * IVX_LDK + lr * IVX_LDK + cc * 4;
    float *Bb = Bs + buf * BN * IVX_LDK + lr * IVX_LDK + cc * 4;
#pragma unroll
    for (int j = 0; j < AR; ++j) *reinterpret_cast<f32x4 *>(Ab + 32 * j * IVX_LDK) = ra[j];
#pragma unroll
    for (int j = 0; j < BR; ++j) *reinterpret_cast<f32x4 *>(Bb + 32 * j * IVX_LDK) = rb[j];
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  load_slab();
  store_slab(0);
  __syncthreads();

  const int frag_off = (lane & 31) * IVX_LDK + 4 * (lane >> 5);
  for (int s = 0; s < S; ++s) {
    const int cur = s & 1;
    const bool more = (s + 1) < S;
    if (more) {
      advance_k();
      load_slab();
    }
    const float *Ac = As + cur * BM * IVX_LDK + wr * TM * 32 * IVX_LDK + frag_off;
    const float *Bc = Bs + cur * BN * IVX_LDK + wc * TN * 32 * IVX_LDK + frag_off;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      f32x4 a[TM], b[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const f32x4 *>(Ac + i * 32 * IVX_LDK + kk * 8);
#pragma unroll
      for (int j = 0; j < TN; ++j) b[j] = *reinterpret_cast<const f32x4 *>(Bc + j * 32 * IVX_LDK + kk * 8);
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][q], b[j][q], acc[i][j], 0, 0, 0);
    }
    if (more) store_slab(cur ^ 1);
    __syncthreads();
  }

  conv_epilogue<TM, TN>(p, acc, m0, n0, wr, wc, lane);
}

// ------------------------------------------------------------------------------------------------
// v4, the production kernel: same tiling as the generic kernel above, cheaper slab loop.
//   * operands are fetched with raw buffer loads: an out-of-image tap, a row past M or a k past K gets the
//     out-of-range offset 0x80000000 and the hardware returns zeros -- no exec-mask branches, no 64-bit address
//     arithmetic in the loop (needs the tensor < 2 GiB); per-row tap validity is a precomputed bit mask (kernel
//     extents <= 8), so the per-slab work per load is one AND/compare, one add, one select;
//   * LDS-DMA staging (buffer_load_dwordx4 ... offen lds): the operands go global -> LDS without passing through
//     VGPRs, so the slab loop has no ds_write pass and no vmcnt -> ds_write dependency;
//   * MFMA fragments are double-buffered in registers: the ds_read_b128 of k-group kk+1 is issued before the MFMAs
//     of group kk.  The DMA writes
// wave-uniform base + lane*16 B, so LDS rows are unpadded 128-byte rows and bank conflicts are avoided by an XOR
// swizzle applied on the SOURCE side (lane with slot c of row r fetches k-chunk c ^ ((r >> SW_SH) & SW_MSK)) and
// again on the fragment read.  BK (K-slab depth) is 32 or 16; 16 halves the LDS so three workgroups fit on a CU.
// s_waitcnt vmcnt(0) (expcnt / lgkmcnt untouched): the LDS-DMA loads are VMEM operations; the compiler does not order
// them against the ds_reads of a LATER loop iteration, so the wait before the publishing barrier is explicit.
__device__ __forceinline__ void lds_dma_wait_all() { __builtin_amdgcn_s_waitcnt(0x0f70); }

// One matrix instruction on a (hi | lo) operand pair: PAIR 1 = bf16 halves, 2 = fp16 halves (same shape and rate)
template <int PAIR>
__device__ __forceinline__ f32x16 pair_mfma(const f32x4 a, const f32x4 b, const f32x16 c) {
  if constexpr (PAIR == 2) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// s_waitcnt vmcnt(n) with n = PER * newer, newer a runtime value in 0 .. 7 (the tail of a deep ring: fewer slabs are outstanding than in the
// steady state).  gfx9 encoding: vmcnt[3:0] in bits 3:0, vmcnt[5:4] in bits 15:14; expcnt / lgkmcnt fields all ones = untouched.  A count
// above 63 is clamped (waiting for fewer outstanding requests than needed is always correct).
template <int N>
__device__ __forceinline__ void lds_dma_wait_imm() {
  constexpr int n = N > 63 ? 63 : N;
  __builtin_amdgcn_s_waitcnt(0x0f70 | (n & 15) | ((n >> 4) << 14));
}
template <int PER>
__device__ __forceinline__ void lds_dma_wait_slabs(const int newer) {
  switch (newer) {
    case 1: lds_dma_wait_imm<PER>(); break;
    case 2: lds_dma_wait_imm<2 * PER>(); break;
    case 3: lds_dma_wait_imm<3 * PER>(); break;
    case 4: lds_dma_wait_imm<4 * PER>(); break;
    case 5: lds_dma_wait_imm<5 * PER>(); break;
    case 6: lds_dma_wait_imm<6 * PER>(); break;
    case 7: lds_dma_wait_imm<7 * PER>(); break;
    default: lds_dma_wait_imm<0>(); break;      // 0 (and anything else: waiting for everything is always correct)
  }
}

// NB (round 5): depth of the LDS ring.  2 = the form described above (prefetch distance two slabs).  With NB buffers the DMA of slab s + NB is
// issued when slab s retires, so NB slabs are in flight per workgroup: the layers of the 2-D trunk whose launch has fewer tiles than the chip
// has workgroup slots (every /8 .. /32 layer at KITTI's batch of 4: 240 - 480 tiles of 0.7 - 1.5 us per slab with 6 - 12 MFMAs of work in it)
// are bound by that latency, and resident workgroups cannot hide it when there are not enough tiles to be resident.  The products are
// accumulated in the same order: results are bit-identical to NB = 2.
template <typename T, int TM, int TN, int WR, int WC, int BK, int WPE, int UNI, int PAIR = 0, int NB = 2, int RPF = 0>
__global__ __launch_bounds__(64 * WR * WC, WPE) void conv_igemm_v4_kernel(const ConvParams p, const unsigned in_bytes,
                                                                  const unsigned w_bytes) {
  constexpr int BM = WR * TM * 32, BN = WC * TN * 32;
  constexpr int EL = sizeof(T);        // 4 (fp32) or 2 (bf16)
  constexpr int EPC = 16 / EL;         // elements per 16-byte chunk
  constexpr int CK = 128 / EL;         // channels per chunk of the chunk-major K order (128 bytes)
  constexpr int NCH = BK / EPC;        // 16-byte chunks per LDS row (8 or 4)
  constexpr int NT = 64 * WR * WC;     // 4 waves (256 threads) or 8 waves (512: the B slab is shared by twice the MFMAs)
  constexpr int RP = NT / NCH;         // rows covered by one pass of the workgroup's threads
  constexpr int AR = BM / RP, BR = BN / RP;
  constexpr int SW_SH = NCH == 8 ? 1 : 2, SW_MSK = NCH - 1;   // slot c of row r holds k-chunk c ^ ((r >> SW_SH) & SW_MSK)
  static_assert(NCH == 8 || NCH == 4, "BK: LDS rows are 128 or 64 bytes");
  static_assert(BM % RP == 0 && BN % RP == 0, "tile rows");
  static_assert(WR * WC == 4 || WR * WC == 8 || WR * WC == 16, "4, 8 or 16 waves per workgroup");
  // LDS-DMA staging: rows are BK elements (128 or 64 B), unpadded
  static_assert(NB >= 2 && NB <= 8, "ring depth");
  static_assert(NB == 2 || (NB - 1) * (AR + BR) <= 63, "deep ring: vmcnt immediates of the tail waits (6 bits)");
  __shared__ __attribute__((aligned(16))) T smem[NB * (BM + BN) * BK];
  T *As = smem;
  T *Bs = smem + NB * BM * BK;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid / WC, wc = wid % WC;

  // 1-D grid of 8 * ceil(Mt/8) * Nt workgroups.  Workgroup b runs on XCD b % 8 (observed dispatch rule; used for
  // speed only): XCD x owns the contiguous M-tiles [x*q, (x+1)*q) so halo re-reads of neighbouring x-slabs hit its own
  // L2, and inside an XCD the Nt workgroups that share one A-tile are consecutive, so they run together and the
  // A-tile is fetched into that L2 once instead of once per N-tile.  Ids past the last M-tile exit (< 8*Nt of them).
  int mt, nt, ct;   // ct: compact tile id inside this launch (split-K partial rows)
  {
    const int Nt = (p.Cout + BN - 1) / BN;
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const int lt = idx / Nt;
    nt = idx - lt * Nt;
    mt = xcd * p.q_total + p.q_begin + lt;
    ct = xcd * p.q_count + lt;
  }
  if (mt * BM >= p.M) return;
  const int m0 = mt * BM;
  const int n0 = nt * BN;
  if (p.cp_dst && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) *p.cp_dst = *p.cp_src;
#ifdef IVX_CONV_TIMELINE
  unsigned long long tl0 = __builtin_amdgcn_s_memrealtime(), tl1 = 0, tl2 = 0;
#endif
  if constexpr (PAIR == 2) {
    if (p.stagger_ticks > 0) {      // (uniform per workgroup)
      const unsigned q = blockIdx.x >> 3;
      if (q < (unsigned)p.stagger_first && ((q >> p.stagger_shift) & 1u)) {
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        while (__builtin_amdgcn_s_memrealtime() - t0 < (unsigned long long)p.stagger_ticks) __builtin_amdgcn_s_sleep(32);
      }
    }
  }

  const size_t gz = blockIdx.z;   // group of a grouped launch (strides are 0 otherwise)
  const __amdgpu_buffer_rsrc_t rs_in =
      __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)p.in + gz * (size_t)p.g_in * EL), 0, in_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_w =
      __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)p.wgt + gz * (size_t)p.g_w * EL), 0, w_bytes, 0x00020000);

  const int lr = tid / NCH;
  const int cc = (tid & (NCH - 1)) ^ ((lr >> SW_SH) & SW_MSK);   // the k-chunk this lane fetches (its LDS slot is tid % NCH)
  const int wid_u = __builtin_amdgcn_readfirstlane(wid);
  int a_off[AR];
  unsigned a_msk[AR];
#pragma unroll
  for (int j = 0; j < AR; ++j) {
    const int m = m0 + lr + RP * j;
    a_off[j] = 0;
    a_msk[j] = 0;
    if (m < p.M) {
      const int ow = m % p.Wo;
      int t = m / p.Wo;
      const int oh = t % p.Ho;
      t /= p.Ho;
      const int od = t % p.Do;
      const int b = t / p.Do;
      const int id0 = od * p.sd - p.pd, ih0 = oh * p.sh - p.ph, iw0 = ow * p.sw - p.pw;
      a_off[j] = (((b * p.D + id0) * p.H + ih0) * p.W + iw0) * p.Cin;
      unsigned md = 0, mh = 0, mw = 0;
      for (int a = 0; a < p.KD; ++a) md |= ((unsigned)(id0 + a) < (unsigned)p.D) ? (1u << a) : 0u;
      for (int e = 0; e < p.KH; ++e) mh |= ((unsigned)(ih0 + e) < (unsigned)p.H) ? (1u << e) : 0u;
      for (int f = 0; f < p.KW; ++f) mw |= ((unsigned)(iw0 + f) < (unsigned)p.W) ? (1u << f) : 0u;
      a_msk[j] = md | (mh << 8) | (mw << 16);
    }
  }
  int b_off[BR];
#pragma unroll
  for (int j = 0; j < BR; ++j) {
    const int n = n0 + lr + RP * j;
    b_off[j] = n < p.Cout ? n * p.K : -1;
  }
  // slab range of this workgroup (split-K: grid.y slices the K loop)
  const int S_all = (p.K + BK - 1) / BK;
  int s_begin = 0, s_end = S_all;
  if (p.ksplit > 1) {
    const int per = (S_all + p.ksplit - 1) / p.ksplit;
    s_begin = blockIdx.y * per;
    s_end = s_begin + per < S_all ? s_begin + per : S_all;
  }
  // K-loop state.  UNI (the production case: chunk-major weights, or tap-major with Cin % BK == 0): every lane of a
  // slab works on the same filter tap, so tap indices, the tap's input offset and its validity mask are wave-uniform
  // (scalar registers / SALU) and the per-slab vector work is one and/compare/add/select per A row and one add per B
  // row.  Otherwise (tiny Cin: the 3-channel stem, odd test shapes) the tap differs per 16-byte chunk and the state is
  // per lane.
  const int S = s_end - s_begin;
  const unsigned OOB = 0x80000000u;
  typedef __attribute__((address_space(3))) void *lds_ptr_t;
  int k4 = s_begin * BK + cc * EPC;      // per lane (generic path)
  int kc, ka, ke, kf;                    // generic: per lane; UNI: uniform (kc without the lane's chunk offset)
  int khalf = 0;   // 64-byte rows, chunk-major: which half of the 128-byte channel chunk this slab covers
  if (p.kmode == 1) {  // chunk-major: slab s = (CK-channel chunk, tap, half)
    constexpr int HPS = CK / BK;                       // slabs per (chunk, tap)
    const int ntap = p.KD * p.KH * p.KW;
    const int chunk = s_begin / (ntap * HPS);
    const int rem = s_begin - chunk * ntap * HPS;
    const int tap = rem / HPS;
    khalf = rem - tap * HPS;
    kc = chunk * CK + khalf * (CK / 2) + (UNI ? 0 : cc * EPC);
    kf = tap % p.KW;
    const int t2 = tap / p.KW;
    ke = t2 % p.KH;
    ka = t2 / p.KH;
  } else {
    const int kfirst = UNI ? s_begin * BK : k4;
    const int tap = kfirst / p.Cin;
    kc = kfirst - tap * p.Cin;
    kf = tap % p.KW;
    const int t2 = tap / p.KW;
    ke = t2 % p.KH;
    ka = t2 / p.KH;
  }
  int a_base[AR];          // UNI: a_off + the lane's chunk offset (elements)
  unsigned b_base[BR];     // UNI: byte offset of (row n, the lane's chunk) or the out-of-range marker
  unsigned kb = (unsigned)(s_begin * BK) * EL;   // UNI: byte offset of the slab inside a weight row
  if constexpr (UNI) {
#pragma unroll
    for (int j = 0; j < AR; ++j) a_base[j] = a_off[j] + cc * EPC;
#pragma unroll
    for (int j = 0; j < BR; ++j) b_base[j] = b_off[j] >= 0 ? (unsigned)(b_off[j] + cc * EPC) * EL : OOB;
  }

  auto load_slab = [&](int buf) {
    T *Ab = As + buf * BM * BK + wid_u * (64 / NCH) * BK;   // wave-uniform base; the DMA adds lane*16 B
    T *Bb = Bs + buf * BN * BK + wid_u * (64 / NCH) * BK;
    if constexpr (UNI) {
      const int delta = ((ka * p.H + ke) * p.W + kf) * p.Cin + kc;                       // scalar
      const unsigned tap = (1u << ka) | (1u << (8 + ke)) | (1u << (16 + kf));           // scalar
#pragma unroll
      for (int j = 0; j < AR; ++j) {
        const unsigned vo = ((a_msk[j] & tap) == tap) ? (unsigned)(a_base[j] + delta) * EL : OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_in, (lds_ptr_t)(Ab + RP * j * BK), 16, vo, 0, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < BR; ++j) {
        const unsigned vo = b_base[j] + kb;   // an out-of-range marker stays out of range: kb < 2^31
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_ptr_t)(Bb + RP * j * BK), 16, vo, 0, 0, 0);
      }
    } else {
      // branch-free: a k past K turns the tap mask into all-ones, which no row mask can satisfy
      const unsigned kbad = (k4 < p.K) ? 0u : 0xffffffffu;
      const int delta = ((ka * p.H + ke) * p.W + kf) * p.Cin + kc;
      const unsigned tap = ((1u << ka) | (1u << (8 + ke)) | (1u << (16 + kf))) | kbad;
#pragma unroll
      for (int j = 0; j < AR; ++j) {
        const unsigned good = ((a_msk[j] & tap) == tap) ? 0xffffffffu : 0u;
        const unsigned vo = (((unsigned)(a_off[j] + delta) * EL) & good) | (OOB & ~good);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_in, (lds_ptr_t)(Ab + RP * j * BK), 16, vo, 0, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < BR; ++j) {
        const unsigned good = (b_off[j] >= 0 ? 0xffffffffu : 0u) & ~kbad;
        const unsigned vo = (((unsigned)(b_off[j] + k4) * EL) & good) | (OOB & ~good);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_ptr_t)(Bb + RP * j * BK), 16, vo, 0, 0, 0);
      }
    }
  };
  auto advance_k = [&]() {
    k4 += BK;
    kb += BK * EL;
    if (p.kmode == 1) {  // next tap of the same channel chunk; after the last tap move to the next chunk
      if (BK < CK) {
        khalf ^= 1;
        kc += khalf ? CK / 2 : -(CK / 2);
        if (khalf) return;
      }
      if (++kf == p.KW) {
        kf = 0;
        if (++ke == p.KH) {
          ke = 0;
          if (++ka == p.KD) {
            ka = 0;
            kc += CK;
          }
        }
      }
      return;
    }
    kc += BK;
    while (kc >= p.Cin) {
      kc -= p.Cin;
      if (++kf == p.KW) {
        kf = 0;
        if (++ke == p.KH) {
          ke = 0;
          ++ka;
        }
      }
    }
  };
  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // RPF: the tile's residual is requested here, in front of the K loop, and consumed by the epilogue (pair IO, res_mode 1): the Cout-expanding
  // 1x1 layers of the bottlenecks have 4 .. 32 slabs of K and twice the output's bytes to move; with the residual requested block by block
  // in the epilogue the launch ran as K loop + (load -> store) chains, 90 us for 283 MB at 64 -> 256 / 96 x 320 x 4 against 46 without one.
  u32x4r rraw[RPF ? TM : 1][RPF ? TN : 1][4];
  if constexpr (RPF) {
    static_assert(PAIR == 2, "residual prefetch: the pair-IO epilogue");
    if (p.pio && p.res_mode == 1 && p.ksplit <= 1) conv_pio_res_prefetch<TM, TN>(p, rraw, m0, n0, wr, wc, lane);
  }
  // Software pipeline over two LDS buffers with a prefetch distance of two slabs.  The fragments of a slab's LAST k-step
  // are read into registers before the barrier, so after the barrier the buffer of the CURRENT slab is already free:
  // the DMA of slab s+2 is issued into it right there and has the last MFMA group of slab s plus all but the last
  // group of slab s+1 to land (a full slab of MFMA time), instead of being issued only at the top of the next slab.
  load_slab(0);
#pragma unroll
  for (int j = 1; j < NB; ++j)
    if (S > j) {
      advance_k();
      load_slab(j);
    }
  if constexpr (NB == 2) {
    lds_dma_wait_all();
  } else {
    const int newer = (S - 1 < NB - 1) ? S - 1 : NB - 1;      // slabs issued after slab 0
    lds_dma_wait_slabs<AR + BR>(newer);
  }
  // (NB > 2: a RAW barrier -- the workgroup fence of __syncthreads() waits for vmcnt(0), i.e. for every request of the ring, which makes
  // any ring deeper than two a two-deep one: seen in the ISA, round 5.  The clobbers keep LDS accesses on their side of it.)
  if constexpr (NB == 2) {
    __syncthreads();   // slabs 0 and 1 landed in every wave's view
  } else {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }

  const int frow = (lane & 31) * BK, fsw = ((lane & 31) >> SW_SH) & SW_MSK, fh = lane >> 5;
#ifdef IVX_CONV_TIMELINE
  tl1 = __builtin_amdgcn_s_memrealtime();
#endif
  int cur = 0;
  for (int s = 0; s < S; ++s) {
    const T *Ac = As + cur * BM * BK + wr * TM * 32 * BK + frow;
    const T *Bc = Bs + cur * BN * BK + wc * TN * 32 * BK + frow;
    // one 16-byte read per operand tile and k-step: half-wave h takes chunk 2*kk + h (4 fp32 k -> 4 MFMAs 32x32x2,
    // or 8 bf16 k -> 1 MFMA 32x32x16); A and B use the same k permutation, so the sum over k is unchanged
    f32x4 fa[2][TM], fb[2][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) fa[0][i] = *reinterpret_cast<const f32x4 *>(Ac + i * 32 * BK + ((fh ^ fsw) * EPC));
#pragma unroll
    for (int j = 0; j < TN; ++j) fb[0][j] = *reinterpret_cast<const f32x4 *>(Bc + j * 32 * BK + ((fh ^ fsw) * EPC));
#pragma unroll
    for (int kk = 0; kk < NCH / 2; ++kk) {
      const int cb = kk & 1, nb = cb ^ 1;
      // PAIR: k-group 2t holds the hi halves of 16 channels, 2t+1 their lo halves; the odd step needs both register buffers
      // (hi in nb, lo in cb), so the read of the next group is issued after its MFMAs instead of before
      const bool defer = PAIR && (kk & 1);
      if (kk < NCH / 2 - 1) {
        if (!defer) {
#pragma unroll
          for (int i = 0; i < TM; ++i) fa[nb][i] = *reinterpret_cast<const f32x4 *>(Ac + i * 32 * BK + (((2 * (kk + 1) + fh) ^ fsw) * EPC));
#pragma unroll
          for (int j = 0; j < TN; ++j) fb[nb][j] = *reinterpret_cast<const f32x4 *>(Bc + j * 32 * BK + (((2 * (kk + 1) + fh) ^ fsw) * EPC));
        }
      } else {
        // every wave holds its last fragments of buffer `cur`; slab s+1 (other buffer) must have landed: each wave
        // waits for its own DMA (issued one barrier ago), the barrier then publishes all of them
        if constexpr (NB == 2) {
          lds_dma_wait_all();
        } else {           // slab s + 1 has landed when only the slabs issued after it are outstanding: min(NB - 2, S - s - 2) of them
          int newer = S - s - 2;
          newer = newer < 0 ? 0 : (newer > NB - 2 ? NB - 2 : newer);
          lds_dma_wait_slabs<AR + BR>(newer);
        }
        if constexpr (NB == 2) {
          __syncthreads();
        } else {           // this wave's fragment reads of slab s are complete (they sit in registers: the compiler waited for them)
          __builtin_amdgcn_s_waitcnt(0xc07f);      // lgkmcnt(0)
          asm volatile("" ::: "memory");
          __builtin_amdgcn_s_barrier();
          asm volatile("" ::: "memory");
        }
        if (s + NB < S) {
          advance_k();
          load_slab(cur);
        }
      }
      if constexpr (EL == 4) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[cb][i][q], fb[cb][j][q], acc[i][j], 0, 0, 0);
      } else if constexpr (EL == 2 && PAIR) {
        static_assert(NCH % 4 == 0, "pair operands: a slab holds whole [hi16 | lo16] groups");
        if ((kk & 1) == 0) {   // hi * hi
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
              acc[i][j] = pair_mfma<PAIR>(fa[cb][i], fb[cb][j], acc[i][j]);
        } else {               // hi * lo + lo * hi (hi: buffer nb, lo: buffer cb)
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
              acc[i][j] = pair_mfma<PAIR>(fa[nb][i], fb[cb][j], acc[i][j]);
              acc[i][j] = pair_mfma<PAIR>(fa[cb][i], fb[nb][j], acc[i][j]);
            }
          if (kk < NCH / 2 - 1) {
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[nb][i] = *reinterpret_cast<const f32x4 *>(Ac + i * 32 * BK + (((2 * (kk + 1) + fh) ^ fsw) * EPC));
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[nb][j] = *reinterpret_cast<const f32x4 *>(Bc + j * 32 * BK + (((2 * (kk + 1) + fh) ^ fsw) * EPC));
          }
        }
      } else if constexpr (EL == 2) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[cb][i]), __builtin_bit_cast(bf16x8, fb[cb][j]),
                                                               acc[i][j], 0, 0, 0);
      } else {   // e4m3: the lane's 16-byte chunk holds 16 k -> two MFMAs 32x32x16 (8 bytes per operand each)
        typedef i64_t i64x2 __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(__builtin_bit_cast(i64x2, fa[cb][i])[q], __builtin_bit_cast(i64x2, fb[cb][j])[q],
                                                                    acc[i][j], 0, 0, 0);
      }
    }
    cur = cur + 1 == NB ? 0 : cur + 1;
  }
#ifdef IVX_CONV_TIMELINE
  tl2 = __builtin_amdgcn_s_memrealtime();
#endif
  if (p.ksplit > 1) {
    // raw partial sums; ivx split-K reduce kernel applies the epilogue
    float *part = p.partial + ((size_t)blockIdx.y * 8 * p.q_count + ct) * BM * p.Cout;   // rows of this tile, slice y
    const int col_l = lane & 31, hh = lane >> 5;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + (wr * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
        if (m >= p.M) continue;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int n = n0 + (wc * TN + j) * 32 + col_l;
          if (n < p.Cout) part[(size_t)(m - m0) * p.Cout + n] = acc[i][j][r];
        }
      }
    return;
  }
  if constexpr (PAIR == 2) {
    if (p.pio) {        // fill_params guarantees out_mode 0, Cout % 16 == 0, no grouped launch
      static_assert(sizeof(smem) >= (size_t)NT / 64 * 4096, "4 KB of staging LDS per wave for the transposed epilogue");
      PairIO io = conv_pair_io(p);
      // the three multipliers are the same in every lane: say so (SGPRs).  As VGPR values they were spilled at four workgroups per CU and
      // RELOADED FROM SCRATCH in every pass of the epilogue -- two more memory round trips per pass, each behind an `s_waitcnt vmcnt(0)` that
      // also waits for the pass's own stores (ISA, round 5)
      io.inv_in = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, io.inv_in)));
      io.inv_res = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, io.inv_res)));
      io.s_out = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, io.s_out)));
      io.post = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, p.post_scale)));      // (the compiler kept
      // {post_scale, ksplit, partial} of the by-value ConvParams in a 16-byte private array and re-read post_scale from scratch in every pass)
      if (p.out_scale_p && blockIdx.x == 0 && tid == 0) *p.out_scale_p = io.s_out;     // (workgroup 0 owns M-tile q_begin of XCD 0: never out of range)
      if constexpr (RPF) conv_epilogue_wide_pio<TM, TN, 1>(p, io, acc, m0, n0, wr, wc, lane, reinterpret_cast<float *>(smem) + wid_u * 1024, wid_u, NT / 64, rraw);
      else conv_epilogue_wide_pio<TM, TN>(p, io, acc, m0, n0, wr, wc, lane, reinterpret_cast<float *>(smem) + wid_u * 1024, wid_u, NT / 64);
#ifdef IVX_CONV_TIMELINE
      if (p.tl && tid == 0) {
        unsigned long long *t = p.tl + (size_t)blockIdx.x * 8;
        t[0] = tl0; t[1] = tl1; t[2] = tl2; t[3] = __builtin_amdgcn_s_memrealtime();
        t[4] = __builtin_amdgcn_s_getreg(63492); t[5] = __builtin_amdgcn_s_getreg(63508);
      }
#endif
      return;
    }
  }
  if (p.out_mode == 0 && !p.out_bf16 && !p.out_fp8 && (p.Cout & 3) == 0 && !p.narrow_epilogue) {
    static_assert(sizeof(smem) >= (size_t)NT / 64 * 4096, "4 KB of staging LDS per wave for the transposed epilogue");
    conv_epilogue_wide<TM, TN>(p, acc, m0, n0, wr, wc, lane, reinterpret_cast<float *>(smem) + wid_u * 1024, gz * (size_t)p.g_out);
    return;
  }
  if constexpr (EL < 4)    // e4m3 outputs come from bf16 (the stem) or e4m3 inputs only: keeps the fp32 instantiations as they were
  if (p.out_mode == 0 && p.out_fp8 && (p.Cout & 15) == 0 && !p.narrow_epilogue) {
    constexpr int NJ = (TN % 2 == 0 && sizeof(smem) >= (size_t)NT / 64 * 8192) ? 2 : 1;
    static_assert(sizeof(smem) >= (size_t)NT / 64 * 4096 * NJ, "staging LDS for the transposed fp8 epilogue");
    conv_epilogue_wide_fp8<TM, TN, NJ>(p, acc, m0, n0, wr, wc, lane, reinterpret_cast<float *>(smem) + wid_u * 1024 * NJ, gz * (size_t)p.g_out);
    return;
  }
  if (p.out_mode == 0 && p.out_bf16 && (p.Cout & 7) == 0 && !p.narrow_epilogue) {
    constexpr int NJ = (TN % 2 == 0 && sizeof(smem) >= (size_t)NT / 64 * 8192) ? 2 : 1;
    static_assert(sizeof(smem) >= (size_t)NT / 64 * 4096 * NJ, "staging LDS for the transposed bf16 epilogue");
    conv_epilogue_wide_bf16<TM, TN, NJ>(p, acc, m0, n0, wr, wc, lane, reinterpret_cast<float *>(smem) + wid_u * 1024 * NJ, gz * (size_t)p.g_out);
    return;
  }
  conv_epilogue<TM, TN>(p, acc, m0, n0, wr, wc, lane, gz * (size_t)p.g_out);
}

// Epilogue + store of one output element (row m, column n) from its finished accumulator: shared by the validation
// kernel and the split-K reduction.
#if IVX_CONV_TU == 0
// (pair IO: the scales of conv_pair_io; returns |stored value| before the output scale, for the amax slots)
__device__ __forceinline__ float conv_store_one(const ConvParams &p, int m, int n, float acc, const PairIO io = {1.0f, 1.0f, 1.0f, false, 1.0f}) {
  if (p.pio) {
    const size_t idx = (size_t)m * p.Cout + n;
    size_t ridx = idx;
    if (p.res_mode == 2) ridx = res2_row_base(m, p.Ho, p.Wo, p.rH, p.rW, p.Cout) + n;
    const float v = conv_finish(p, acc, (p.scale ? p.scale[n] : 1.0f) * io.inv_in, p.shift ? p.shift[n] : 0.0f, ridx, p.res_pair ? io.inv_res : 1.0f);
    float y = p.out_pair ? v * io.s_out : v;
    if (p.out_pair && io.sat) y = (y > 65504.f && y < __builtin_inff()) ? 65504.f : ((y < -65504.f && y > -__builtin_inff()) ? -65504.f : y);
    conv_st_out(p, idx, y);
    return fabsf(v);
  }
  if (p.out_mode == 1) {
    const int tap = n / p.Cr, ch = n - tap * p.Cr;
    const int a2 = tap >> 2, e2 = (tap >> 1) & 1, f2 = tap & 1;
    const size_t o = up2_row_base(m, p.D, p.H, p.W, p.Cr) + (((size_t)a2 * 2 * p.H + e2) * 2 * p.W + f2) * p.Cr + ch;
    conv_st_out(p, o, conv_finish(p, acc, p.scale ? p.scale[ch] : 1.0f, p.shift ? p.shift[ch] : 0.0f, o));
    return 0.f;
  }
  const size_t idx = (size_t)m * p.Cout + n;
  size_t ridx = idx;
  if (p.res_mode == 2) ridx = res2_row_base(m, p.Ho, p.Wo, p.rH, p.rW, p.Cout) + n;
  conv_st_out(p, idx, conv_finish(p, acc, p.scale ? p.scale[n] : 1.0f, p.shift ? p.shift[n] : 0.0f, ridx));
  return 0.f;
}

// Split-K reduction: out = epilogue(sum over slices in slice order) -- deterministic.  Partial rows are compact:
// row cr = (xcd*q_count + local_tile)*bm + row_in_tile  <->  m = (xcd*q_total + q_begin + local_tile)*bm + row_in_tile.
__global__ __launch_bounds__(256) void conv_splitk_reduce_kernel(const ConvParams p) {
  const size_t rows = (size_t)8 * p.q_count * p.bm;
  const size_t total = rows * p.Cout;
  PairIO io = {1.0f, 1.0f, 1.0f, false, p.post_scale};
  if (p.pio) {
    io = conv_pair_io(p);
    if (p.out_scale_p && blockIdx.x == 0 && threadIdx.x == 0) *p.out_scale_p = io.s_out;
  }
  float omax = 0.f;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int n = (int)(idx % p.Cout);
    const size_t cr = idx / p.Cout;
    const int ctile = (int)(cr / p.bm), rit = (int)(cr - (size_t)ctile * p.bm);
    const int xcd = ctile / p.q_count, lt = ctile - xcd * p.q_count;
    const long long m = (long long)(xcd * p.q_total + p.q_begin + lt) * p.bm + rit;
    if (m >= p.M) continue;
    float acc = 0.f;
    for (int z = 0; z < p.ksplit; ++z) acc += p.partial[(size_t)z * total + idx];
    omax = fmaxf(omax, conv_store_one(p, (int)m, n, acc, io));
  }
  if (p.pio && p.amax_out) {        // (uniform)
    __shared__ float red[4];
    ivx_amax_commit_wg(p.amax_out, omax, red, (int)blockIdx.x);
  }
}

// The same reduction for pair IO (the chained fp16-pair trunk), four channels per thread: 16-byte partial loads, the epilogue of
// conv_pio_finish4 (8-byte hi / lo stores).  32-bit indexing: split K is only planned for small outputs (the launcher checks).
__global__ __launch_bounds__(256) void conv_splitk_reduce_pio_kernel(const ConvParams p) {
  const PairIO io = conv_pair_io(p);
  if (p.out_scale_p && blockIdx.x == 0 && threadIdx.x == 0) *p.out_scale_p = io.s_out;
  const unsigned C4 = (unsigned)p.Cout >> 2, rows = 8u * (unsigned)p.q_count * (unsigned)p.bm, total4 = rows * C4;
  const size_t total = (size_t)rows * p.Cout;
  float omax = 0.f;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += gridDim.x * blockDim.x) {
    const unsigned cr = i / C4, nb = (i - cr * C4) * 4;
    const unsigned ctile = cr / (unsigned)p.bm, rit = cr - ctile * (unsigned)p.bm;
    const unsigned xcd = ctile / (unsigned)p.q_count, lt = ctile - xcd * (unsigned)p.q_count;
    const long long m = (long long)(xcd * p.q_total + p.q_begin + lt) * p.bm + rit;
    if (m >= p.M) continue;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int z = 0; z < p.ksplit; ++z) acc += *reinterpret_cast<const f32x4 *>(p.partial + (size_t)z * total + (size_t)cr * p.Cout + nb);
    f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sf = {0.f, 0.f, 0.f, 0.f};
    if (p.scale) sc = *reinterpret_cast<const f32x4 *>(p.scale + nb);
    if (p.shift) sf = *reinterpret_cast<const f32x4 *>(p.shift + nb);
    sc *= io.inv_in;
    omax = fmaxf(omax, conv_pio_finish4(p, io, acc, (int)m, (int)nb, sc, sf));
  }
  if (p.amax_out) {        // (uniform)
    __shared__ float red[4];
    ivx_amax_commit_wg(p.amax_out, omax, red, (int)blockIdx.x);
  }
}

// Validation kernel: one thread per output element, sequential fmaf over (kd,kh,kw,ci).
__global__ __launch_bounds__(256) void conv_naive_f32_kernel(const ConvParams p) {
  const size_t total = (size_t)p.M * p.Cout;
  PairIO io = {1.0f, 1.0f, 1.0f, false, p.post_scale};
  if (p.pio) {
    io = conv_pair_io(p);
    if (p.out_scale_p && blockIdx.x == 0 && threadIdx.x == 0) *p.out_scale_p = io.s_out;
  }
  float omax = 0.f;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int n = (int)(idx % p.Cout);
    const int m = (int)(idx / p.Cout);
    const int ow = m % p.Wo;
    int t = m / p.Wo;
    const int oh = t % p.Ho;
    t /= p.Ho;
    const int od = t % p.Do;
    const int b = t / p.Do;
    float acc = 0.f;
    for (int a = 0; a < p.KD; ++a) {
      const int id = od * p.sd - p.pd + a;
      if ((unsigned)id >= (unsigned)p.D) continue;
      for (int e = 0; e < p.KH; ++e) {
        const int ih = oh * p.sh - p.ph + e;
        if ((unsigned)ih >= (unsigned)p.H) continue;
        for (int f = 0; f < p.KW; ++f) {
          const int iw = ow * p.sw - p.pw + f;
          if ((unsigned)iw >= (unsigned)p.W) continue;
          const size_t xo = ((((size_t)b * p.D + id) * p.H + ih) * p.W + iw) * p.Cin;
          const int tap = (a * p.KH + e) * p.KW + f;
          const int ntap = p.KD * p.KH * p.KW;
          const size_t wo = (size_t)n * p.K;
          const int ck = p.in_fp8 ? 128 : (p.in_bf16 ? 64 : 32);   // channels per 128-byte chunk of the chunk-major order
          if (p.in_pair) {   // the value a (hi, lo) pair stands for is hi + lo (exact in fp32): plain fp32 products of those
            for (int c = 0; c < p.Cin / 2; ++c) {
              const int eh = (c >> 4) * 32 + (c & 15), el = eh + 16;
              const size_t wh = p.kmode == 1 ? (size_t)((eh / ck) * ntap + tap) * ck + (eh % ck) : (size_t)tap * p.Cin + eh;
              if (p.in_pair == 2) {
                const _Float16 *xp = reinterpret_cast<const _Float16 *>(p.in) + xo, *wp = reinterpret_cast<const _Float16 *>(p.wgt) + wo;
                acc = fmaf((float)xp[eh] + (float)xp[el], (float)wp[wh] + (float)wp[wh + 16], acc);
              } else {
                const __bf16 *xp = reinterpret_cast<const __bf16 *>(p.in) + xo, *wp = reinterpret_cast<const __bf16 *>(p.wgt) + wo;
                acc = fmaf((float)xp[eh] + (float)xp[el], (float)wp[wh] + (float)wp[wh + 16], acc);
              }
            }
            continue;
          }
          for (int c = 0; c < p.Cin; ++c) {
            const size_t wi = wo + (p.kmode == 1 ? (size_t)((c / ck) * ntap + tap) * ck + (c % ck) : (size_t)tap * p.Cin + c);
            const float xv = p.in_fp8 ? fp8_to_f32(reinterpret_cast<const unsigned char *>(p.in)[xo + c])
                                      : (p.in_bf16 ? (float)reinterpret_cast<const __bf16 *>(p.in)[xo + c] : p.in[xo + c]);
            const float wv = p.in_fp8 ? fp8_to_f32(reinterpret_cast<const unsigned char *>(p.wgt)[wi])
                                      : (p.in_bf16 ? (float)reinterpret_cast<const __bf16 *>(p.wgt)[wi] : p.wgt[wi]);
            acc = fmaf(xv, wv, acc);
          }
        }
      }
    }
    omax = fmaxf(omax, conv_store_one(p, m, n, acc, io));
  }
  if (p.pio && p.amax_out) {        // (uniform)
    __shared__ float red[4];
    ivx_amax_commit_wg(p.amax_out, omax, red, (int)blockIdx.x);
  }
}

#ifdef IVX_CONV_TIMELINE
static unsigned long long *g_timeline = nullptr;
extern "C" int ivx_conv_set_timeline(void *buf) { g_timeline = (unsigned long long *)buf; return 0; }
#endif

static int fill_params(const ivx_conv_desc *d, const void *in, const void *wgt, const float *scale,
                       const float *shift, const void *res, void *out, ConvParams *p, const ivx_pair_io *io = nullptr) {
  IVX_REQUIRE(d && in && wgt && out, "ivx_conv_fwd: null argument");
  IVX_REQUIRE(d->B > 0 && d->D > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0, "ivx_conv_fwd: non-positive dims");
  IVX_REQUIRE(d->Cin % 4 == 0, "ivx_conv_fwd: Cin (%d) must be a multiple of 4 (pad the input channels)", d->Cin);
  IVX_REQUIRE(d->KD > 0 && d->KH > 0 && d->KW > 0 && d->sd > 0 && d->sh > 0 && d->sw > 0, "ivx_conv_fwd: bad kernel/stride");
  IVX_REQUIRE(d->pd >= 0 && d->ph >= 0 && d->pw >= 0, "ivx_conv_fwd: negative padding");
  int32_t Do, Ho, Wo;
  if (ivx_conv_out_dims(d, &Do, &Ho, &Wo) != IVX_OK) return IVX_ERR_INVALID_ARG;
  const int64_t M = (int64_t)d->B * Do * Ho * Wo;
  const bool pair = d->in_dtype == IVX_BF16_PAIR || d->in_dtype == IVX_F16_PAIR;
  const int cin_el = pair ? 2 * d->Cin : d->Cin;     // stored elements per voxel (a pair tensor holds two bf16 per channel)
  const int64_t K = (int64_t)d->KD * d->KH * d->KW * cin_el;
  IVX_REQUIRE(M < (1LL << 31) - 512 && K < (1LL << 30), "ivx_conv_fwd: problem too large for 32-bit row index");
  IVX_REQUIRE((int64_t)d->B * d->D * d->H * d->W < (1LL << 31), "ivx_conv_fwd: input voxel count exceeds 2^31");
  IVX_REQUIRE(d->res_mode >= 0 && d->res_mode <= 2, "ivx_conv_fwd: bad res_mode");
  IVX_REQUIRE(d->out_mode == 0 || (d->out_mode == 1 && d->KD == 1 && d->KH == 1 && d->KW == 1 && d->sd == 1 && d->sh == 1 && d->sw == 1 &&
                                     d->pd == 0 && d->ph == 0 && d->pw == 0 && d->Cout % 8 == 0 && d->res_mode != 2),
              "ivx_conv_fwd: out_mode 1 (ConvTranspose k2 s2) needs a 1x1x1 stride-1 GEMM with Cout = 8 * real channels");
  IVX_REQUIRE(d->in_dtype >= IVX_F32 && d->in_dtype <= IVX_F16_PAIR && d->out_dtype >= IVX_F32 && (d->out_dtype <= IVX_FP8 || (io && d->out_dtype == IVX_F16_PAIR)),
              "ivx_conv_fwd: dtypes are IVX_F32 (0), IVX_BF16 (1), IVX_FP8 (2) or, for the input, IVX_BF16_PAIR (3) / IVX_F16_PAIR (4); an IVX_F16_PAIR "
              "output needs ivx_conv_fwd_pio");
  if (io) {
    IVX_REQUIRE(d->in_dtype == IVX_F16_PAIR && d->out_mode == 0 && d->Cout % 4 == 0 && (d->out_dtype == IVX_F32 || d->out_dtype == IVX_F16_PAIR),
                "ivx_conv_fwd_pio: needs an IVX_F16_PAIR input, out_mode 0, Cout %% 4 == 0 and an IVX_F32 or IVX_F16_PAIR output");
    IVX_REQUIRE(io->res_dtype == IVX_F32 || io->res_dtype == IVX_F16_PAIR, "ivx_conv_fwd_pio: res_dtype is IVX_F32 or IVX_F16_PAIR");
    IVX_REQUIRE(d->out_dtype != IVX_F16_PAIR || (d->Cout % 16 == 0 && io->out_scale && io->amax_in && (d->res_mode == 0 || io->amax_res)),
                "ivx_conv_fwd_pio: a pair output needs Cout %% 16 == 0, out_scale, amax_in (and amax_res with a residual)");
    IVX_REQUIRE(!(d->res_mode && io->res_dtype == IVX_F16_PAIR) || (d->Cout % 16 == 0 && io->res_scale), "ivx_conv_fwd_pio: a pair residual needs Cout %% 16 == 0 and res_scale");
  }
  IVX_REQUIRE(!pair || (d->Cin % 16 == 0 && d->out_mode == 0), "ivx_conv_fwd: bf16-pair input needs Cin %% 16 == 0 and out_mode 0");
  IVX_REQUIRE(d->in_dtype != IVX_FP8 || d->Cin % 16 == 0, "ivx_conv_fwd: fp8 input needs Cin %% 16 == 0");
  IVX_REQUIRE((d->in_dtype != IVX_FP8 && d->out_dtype != IVX_FP8) || d->out_mode == 0, "ivx_conv_fwd: fp8 is built for out_mode 0 only");
  const int ck = d->in_dtype == IVX_FP8 ? 128 : (d->in_dtype == IVX_BF16 ? 64 : 32);   // pair: 32 real channels = 64 stored elements
  IVX_REQUIRE(d->wgt_layout == 0 || (d->wgt_layout == 1 && d->Cin % ck == 0),
              "ivx_conv_fwd: wgt_layout 1 needs Cin %% %d == 0 (128-byte channel chunks)", ck);
  IVX_REQUIRE(d->in_dtype == IVX_F32 || d->Cin % 8 == 0, "ivx_conv_fwd: bf16 input needs Cin %% 8 == 0");
  IVX_REQUIRE(d->res_mode == 0 || res, "ivx_conv_fwd: res_mode set but res is NULL");
  if (d->res_mode == 2) {
    IVX_REQUIRE(Do == 1 && d->res_h > 0 && d->res_w > 0, "ivx_conv_fwd: res_mode 2 needs a 2-D output and res dims");
  }
  p->in = (const float *)in; p->wgt = (const float *)wgt; p->scale = scale; p->shift = shift;
  p->res = d->res_mode ? (const float *)res : nullptr; p->out = (float *)out;
  p->in_bf16 = d->in_dtype == IVX_BF16 || pair; p->out_bf16 = d->out_dtype == IVX_BF16;
  p->in_pair = d->in_dtype == IVX_BF16_PAIR ? 1 : (d->in_dtype == IVX_F16_PAIR ? 2 : 0);
  p->in_fp8 = d->in_dtype == IVX_FP8; p->out_fp8 = d->out_dtype == IVX_FP8;
  p->res_scale = d->res_scale == 0.f ? 1.0f : d->res_scale;
  p->B = d->B; p->D = d->D; p->H = d->H; p->W = d->W; p->Cin = cin_el;
  p->Cout = d->Cout; p->KD = d->KD; p->KH = d->KH; p->KW = d->KW;
  p->sd = d->sd; p->sh = d->sh; p->sw = d->sw; p->pd = d->pd; p->ph = d->ph; p->pw = d->pw;
  p->Do = Do; p->Ho = Ho; p->Wo = Wo; p->M = (int)M; p->K = (int)K;
  p->relu = d->relu; p->res_mode = d->res_mode; p->rH = d->res_h; p->rW = d->res_w; p->kmode = d->wgt_layout;
  p->out_mode = d->out_mode; p->Cr = d->out_mode == 1 ? d->Cout / 8 : d->Cout; p->res_after_act = d->res_after_act;
  p->post_scale = d->post_scale == 0.f ? 1.0f : d->post_scale;
  p->ksplit = 1; p->partial = nullptr; p->q_total = 0; p->q_begin = 0; p->q_count = 0; p->bm = 0;
  p->stagger_ticks = 0; p->stagger_shift = 0; p->stagger_first = 0;
  p->groups = 1; p->g_in = p->g_w = p->g_out = 0;
  p->narrow_epilogue = conv_lab().narrow_epilogue;
#ifdef IVX_CONV_TIMELINE
  p->tl = g_timeline;
#endif
  p->cp_src = nullptr; p->cp_dst = nullptr; p->m_dev = nullptr;
  p->pio = 0; p->in_scale_p = nullptr; p->out_pair = 0; p->res_pair = 0; p->res_scale_p = nullptr; p->out_scale_p = nullptr;
  p->amax_in = p->amax_res = nullptr; p->amax_out = nullptr; p->wbound = 0.f; p->sbound = 0.f;
  if (io) {
    p->pio = 1;
    p->in_scale_p = io->in_scale;
    p->out_pair = d->out_dtype == IVX_F16_PAIR; p->out_bf16 = 0;
    p->res_pair = d->res_mode && io->res_dtype == IVX_F16_PAIR;
    p->res_scale_p = io->res_scale; p->out_scale_p = p->out_pair ? io->out_scale : nullptr;
    p->amax_in = io->amax_in; p->amax_res = d->res_mode ? io->amax_res : nullptr; p->amax_out = io->amax_out;
    p->wbound = io->wbound; p->sbound = io->sbound;
  }
  return IVX_OK;
}

extern "C" int ivx_conv_out_dims(const ivx_conv_desc *d, int32_t *Do, int32_t *Ho, int32_t *Wo) {
  IVX_REQUIRE(d && Do && Ho && Wo, "ivx_conv_out_dims: null argument");
  const int od = (d->D + 2 * d->pd - d->KD) / d->sd + 1;
  const int oh = (d->H + 2 * d->ph - d->KH) / d->sh + 1;
  const int ow = (d->W + 2 * d->pw - d->KW) / d->sw + 1;
  IVX_REQUIRE(d->D + 2 * d->pd >= d->KD && d->H + 2 * d->ph >= d->KH && d->W + 2 * d->pw >= d->KW && od > 0 && oh > 0 && ow > 0,
              "ivx_conv_out_dims: kernel larger than padded input");
  *Do = od; *Ho = oh; *Wo = ow;
  return IVX_OK;
}

// Generic kernel (64-bit addressing, any kernel extent; weight layout 0 only): the fallback for tensors >= 2 GiB.
template <int TM, int TN, int WR, int WC>
static void launch_cfg(const ConvParams &p, hipStream_t st) {
  constexpr int BM = WR * TM * 32, BN = WC * TN * 32;
  dim3 grid((p.M + BM - 1) / BM, (p.Cout + BN - 1) / BN);
  hipLaunchKernelGGL((conv_igemm_f32_kernel<TM, TN, WR, WC>), grid, dim3(256), 0, st, p);
}

#endif   // IVX_CONV_TU == 0

template <typename T, int TM, int TN, int WR, int WC, int BK, int WPE = 1, int PAIR = 0, int NB = 2, int RPF = 0>
static void launch_v4(ConvParams &p, hipStream_t st) {
  constexpr int BM = WR * TM * 32, BN = WC * TN * 32;
  const int64_t in_bytes = (int64_t)p.B * p.D * p.H * p.W * p.Cin * sizeof(T);
  const int64_t w_bytes = (int64_t)p.Cout * p.K * sizeof(T);
  const long long Mt = (p.M + BM - 1) / BM, Nt = (p.Cout + BN - 1) / BN;
  p.bm = BM;
  if (p.q_total == 0) {  // whole problem in one launch
    p.q_total = (int)((Mt + 7) / 8);
    p.q_begin = 0;
    p.q_count = p.q_total;
  }
  const long long g1 = 8LL * p.q_count * Nt;
  const dim3 grid((unsigned)g1, p.ksplit > 1 ? p.ksplit : 1, p.groups > 1 ? p.groups : 1);
  // every slab lies inside one filter tap -> uniform K-loop state
  const bool uni = p.kmode == 1 || p.Cin % BK == 0;
  if constexpr (NB > 2) {      // deep ring: the uniform K-loop state only (every pair layer of the trunk: chunk-major filters)
    if (!uni) {
      launch_v4<T, TM, TN, WR, WC, BK, WPE, PAIR, 2>(p, st);
      return;
    }
    auto kern = conv_igemm_v4_kernel<T, TM, TN, WR, WC, BK, WPE, 1, PAIR, NB, RPF>;
    hipLaunchKernelGGL(kern, grid, dim3(64 * WR * WC), 0, st, p, (unsigned)in_bytes, (unsigned)w_bytes);
  } else {
    auto kern = uni ? conv_igemm_v4_kernel<T, TM, TN, WR, WC, BK, WPE, 1, PAIR, 2, RPF> : conv_igemm_v4_kernel<T, TM, TN, WR, WC, BK, WPE, 0, PAIR>;
    hipLaunchKernelGGL(kern, grid, dim3(64 * WR * WC), 0, st, p, (unsigned)in_bytes, (unsigned)w_bytes);
  }
}


// The launch switch of an LDS-DMA translation unit: the rows of conv_tiles.h that name the operand family FAM, on the element type T.
// false: FAM has no instantiation of `cfg`.
template <typename T, int FAM, int PAIR = 0>
static bool launch_tile(ConvParams &p, int cfg, hipStream_t st) {
  switch (cfg) {
#define IVX_ROW(n, fam, TM, TN, WR, WC, BK, WPE, NB, RPF, WG) \
    case n: if constexpr ((IVX_FAM_##fam & FAM) != 0) { launch_v4<T, TM, TN, WR, WC, BK, WPE, PAIR, NB, RPF>(p, st); return true; } else return false;
    IVX_CONV_TILES(IVX_ROW)
#undef IVX_ROW
    default: return false;
  }
}

#if IVX_CONV_TU == 3 || IVX_CONV_TU == 4
static int no_pair_tile(int cfg) {
  ivx_set_error("ivx_conv_fwd: tile %d has no instantiation for these pair operands (conv_tiles.h)", cfg);
  return IVX_ERR_INVALID_ARG;
}
#if IVX_CONV_TU == 3
int ivx_conv_launch_pair_bf16(ConvParams &p, const ConvPlan &pl, hipStream_t st) {
  return launch_tile<__bf16, IVX_FAM_PAIR_BF16, 1>(p, pl.cfg, st) ? IVX_OK : no_pair_tile(pl.cfg);
}
#else
int ivx_conv_launch_pair_f16(ConvParams &p, const ConvPlan &pl, hipStream_t st) {
  return launch_tile<__bf16, IVX_FAM_PAIR_F16, 2>(p, pl.cfg, st) ? IVX_OK : no_pair_tile(pl.cfg);
}
#endif
#endif

#if IVX_CONV_TU == 5
// Winograd-domain GEMM of a stride-1, pad-1, 1x1x3 convolution along z on pair operands, with the THREE z-taps served from ONE staged
// tile.  The rows of a transformed plane are (tile column, z), z fastest, so the A rows of tap kz are the output rows shifted by
// kz - 1: the generic kernel stages them three times (one K slab per tap: 3 x the L2 -> LDS traffic, 3 x the barriers), and at the 16-bit
// MFMA rate that staging is what the pair GEMMs wait for (5.8 TB/s of LDS-DMA for 3.8 TB/s of HBM traffic, the per-slab
// MFMA work of 0.18 us cannot hide one load).  Here an iteration covers one 16-channel pair group: BM + 2 rows of A (a one-row halo on
// either side) and the three taps' B rows are staged once, and 9 * TM * TN MFMAs (3 taps x hi*hi + hi*lo + lo*hi) run on them; fragments
// of tap kz are read kz rows further down, rows whose z + kz - 1 falls outside the column are zeroed in registers.
// Same LDS row format as conv_igemm_v4_kernel (64-byte rows of 32 stored elements, XOR swizzle by (row >> 2) & 3), same epilogue.
// (T = __bf16: the 2-byte storage element, as in conv_igemm_v4_kernel.)  NBUF staging buffers form a ring with a prefetch distance of
// NBUF - 1 groups: at 16-bit MFMA rates one group of a 128 x 128 tile is 0.5 us of matrix work against 2-3 us of load latency under
// load, so the tiles are large (bytes staged per MFMA fall with the tile edge) and the ring is as deep as the 160 KB of LDS allow.
// TAIL 1: a tile stores BM rows and stages BM + 16 (the last 16 by wave 0).  TAIL 0: a tile stages exactly BM rows and stores the BM - 2
// in the middle, consecutive tiles overlapping by two rows (1.6 % more tiles at BM = 128): 40 KB of LDS for the 128 x 64 tile, i.e. a
// fourth workgroup per CU -- and resident workgroups are what hides the load latency here.
// SW 2 (TAIL 0 only): the z-stride-2 layers.  With an even Z the input row of output row r' and tap kz is 2 r' - 1 + kz whatever the
// column, so a tile stages 2 BM consecutive input rows, stores BM - 1 output rows and reads the fragments of tap kz at rows 2 o + kz;
// only tap 0 can fall outside the column (z' = 0).  One staged row serves 1.5 taps instead of 3.
// ZR 1: a lane whose z - 1 / z + 1 neighbour lies outside the column reads the fragments of that tap from an LDS row that is ALWAYS zero
// instead of zeroing the eight dwords it read (32 v_cndmask per group in the 126 x 64 tile, where the loop has 18 MFMAs): the address is
// chosen once per tile.  The zero row costs no LDS: it is a staged row that no stored output reads -- row BM + 2 of the tail pass, the
// last of the 2 BM rows of the stride-2 form, and for the overlapping stride-1 tiles the last staged row, given up as a source row (a
// tile then stores BM - 3 rows instead of BM - 2) -- whose DMA lanes get an out-of-range offset, i.e. zeros, in every group.
// DI 1 (SW 2 only): the staged rows are de-interleaved -- LDS rows 0 .. BM - 1 hold the even staged rows, BM .. 2 BM - 1 the odd ones -- so
// that the fragment rows of a tap are CONSECUTIVE LDS rows as in the stride-1 form (rows two apart start on two of the four 16-bank groups
// only: 27 % of the LDS cycles of the interleaved form were bank conflicts, profiles/r04_bench_pmc.md).  Only the global row a DMA lane
// fetches changes; tap kz of output row o reads LDS row o (kz 0), BM + o (kz 1), o + 1 (kz 2).
template <typename T, int TM, int TN, int WR, int WC, int WPE, int PAIR, int NBUF, int TAIL = 1, int SW = 1, int ZR = 0, int DI = 0>
__global__ __launch_bounds__(64 * WR * WC, WPE) void conv_wino_halo_kernel(const ConvParams p, const unsigned in_bytes, const unsigned w_bytes) {
  constexpr int BM = WR * TM * 32, BN = WC * TN * 32, NT = 64 * WR * WC;
  constexpr int BK = 32, EPC = 8, NCH = 4, RP = NT / NCH;
  static_assert((SW * BM) % RP == 0 && (3 * BN) % RP == 0, "A rows and the three taps of B rows in whole passes (+ one 16-row tail pass of A)");
  static_assert(SW == 1 || TAIL == 0, "the stride-2 form uses overlapping tiles");
  static_assert(!DI || SW == 2, "de-interleaved staging is the stride-2 form's");
  constexpr int APASS = SW * BM / RP, AROWS = SW * BM + 16 * TAIL;        // staged input rows: plane rows SW * m0 - 1 ...
  constexpr int BMO = TAIL ? BM : (SW == 1 ? BM - 2 - ZR : BM - 1);        // rows a tile stores
  constexpr int ZROW = TAIL ? BM + 2 : SW * BM - 1;                        // ZR: the LDS row of A that stays zero
  constexpr int BPASS = 3 * BN / RP;
  constexpr int BUF = (AROWS + 3 * BN) * BK;                               // elements per buffer
  constexpr int D = NBUF - 1;                                              // prefetch distance in groups
  constexpr int LPG = APASS + BPASS;                                       // DMA instructions per group and wave (wave 0: TAIL more)
  static_assert((D - 1) * (LPG + TAIL) <= 15, "vmcnt immediate");
  __shared__ __attribute__((aligned(16))) T smem[NBUF * BUF];
  static_assert(sizeof(smem) >= (size_t)NT / 64 * 4096, "4 KB of staging LDS per wave for the transposed epilogue");
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid / WC, wc = wid % WC;
  // device-side row count: the XCD quota follows it (the host's q_total would leave whole XCDs with empty tiles)
  const int M = p.m_dev ? *p.m_dev : p.M;
  const int q_total = p.m_dev ? ((M + BMO - 1) / BMO + 7) >> 3 : p.q_total;
  int mt, nt;
  {
    const int Nt = (p.Cout + BN - 1) / BN;
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const int lt = idx / Nt;
    nt = idx - lt * Nt;
    mt = xcd * q_total + lt;
    if (p.cp_dst && blockIdx.x == 0 && blockIdx.z == 0 && tid == 0) *p.cp_dst = *p.cp_src;      // (before the returns: *m_dev may be 0)
    if (lt >= q_total) return;                    // (only with m_dev: the grid was sized for p.M rows)
  }
  if (mt * BMO >= M) return;
  const int m0 = mt * BMO, n0 = nt * BN;
  const size_t gz = blockIdx.z;
#ifdef IVX_CONV_TIMELINE
  const unsigned long long tl0 = __builtin_amdgcn_s_memrealtime();
  unsigned long long tl1 = 0, tl2 = 0;
#endif
  const __amdgpu_buffer_rsrc_t rs_in =
      __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)p.in + gz * (size_t)p.g_in * sizeof(T)), 0, in_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_w =
      __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)p.wgt + gz * (size_t)p.g_w * sizeof(T)), 0, w_bytes, 0x00020000);
  const int lr = tid / NCH;
  const int cc = (tid & (NCH - 1)) ^ ((lr >> 2) & 3);            // the k-chunk this lane fetches (its LDS slot is tid % NCH)
  const int wid_u = __builtin_amdgcn_readfirstlane(wid);
  const unsigned OOB = 0x80000000u;
  typedef __attribute__((address_space(3))) void *lds_ptr_t;
  // A: LDS row i holds plane row m0 - 1 + i; the last 16 rows are staged by wave 0 alone (only two of them are used)
  unsigned a_base[APASS + 1];
  a_base[APASS] = OOB;
#pragma unroll
  for (int j = 0; j < APASS + TAIL; ++j) {
    const int li = j < APASS ? lr + RP * j : BM + (lane >> 2);
    const int row = SW * m0 - 1 + (DI ? (li < BM ? 2 * li : 2 * (li - BM) + 1) : li);
    const bool zr = ZR && !TAIL && li == ZROW;
    a_base[j] = (row >= 0 && row < SW * M && (j < APASS || (lane >> 2) < 2) && !zr) ? ((unsigned)row * (unsigned)p.Cin + cc * EPC) * (unsigned)sizeof(T) : OOB;
  }
  // B: LDS row t * BN + n holds filter row n0 + n of tap t; chunk-major K: (32 real channels = 64 stored) x tap
  unsigned b_base[BPASS];
#pragma unroll
  for (int j = 0; j < BPASS; ++j) {
    const int r = lr + RP * j, tap = r / BN, n = n0 + (r - tap * BN);
    b_base[j] = n < p.Cout ? ((unsigned)n * (unsigned)p.K + tap * 64 + cc * EPC) * (unsigned)sizeof(T) : OOB;
  }
  const int G = p.Cin / BK;                                    // 16-channel pair groups
  auto load_group = [&](int g, int buf) {
    T *Ab = smem + buf * BUF + wid_u * (64 / NCH) * BK;     // wave-uniform base; the DMA adds lane * 16 B
    T *Bb = Ab + AROWS * BK;
    const unsigned ka = (unsigned)g * BK * (unsigned)sizeof(T);                                             // byte offset of the group inside an A row
    const unsigned kb = ((unsigned)(g >> 1) * 3u * 64u + (unsigned)(g & 1) * 32u) * (unsigned)sizeof(T);    // ... inside a filter row (tap 0)
    // (the offset goes through a named variable: with the conditional written inside the builtin's argument list the host pass of
    // this clang drops the whole kernel without a diagnostic)
#pragma unroll
    for (int j = 0; j < APASS; ++j) {
      const unsigned vo = a_base[j] == OOB ? OOB : a_base[j] + ka;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_in, (lds_ptr_t)(Ab + RP * j * BK), 16, vo, 0, 0, 0);
    }
    if (TAIL && wid_u == 0) {
      const unsigned vo = a_base[APASS] == OOB ? OOB : a_base[APASS] + ka;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_in, (lds_ptr_t)(smem + buf * BUF + BM * BK), 16, vo, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < BPASS; ++j) {
      const unsigned vo = b_base[j] == OOB ? OOB : b_base[j] + kb;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_ptr_t)(Bb + RP * j * BK), 16, vo, 0, 0, 0);
    }
  };
  // validity of the z - 1 / z + 1 neighbours of this lane's rows (Wo = W = Z rows per tile column)
  const int rl = lane & 31, fh = lane >> 5;
  bool ok0[TM], ok2[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int z = (m0 + (wr * TM + i) * 32 + rl) % p.Wo;      // output z (Wo = W for stride 1)
    ok0[i] = z >= 1;
    ok2[i] = SW == 2 || z + 1 < p.Wo;                        // stride 2: input z = 2 z' + 1 <= Z - 1 always
  }
  // ZR: element offset of this lane's hi fragment of taps 0 and 2 inside the A area of a buffer (lo: the same ^ 2 chunks)
  int aoff[2][TM];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int ar = DI ? rl + t : SW * rl + 2 * t;
      const bool ok = t == 0 ? ok0[i] : ok2[i];
      aoff[t][i] = ok ? ((DI ? 1 : SW) * (wr * TM + i) * 32 + ar) * BK + ((fh ^ ((ar >> 2) & 3)) * EPC) : ZROW * BK + fh * EPC;
    }
  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

#pragma unroll
  for (int g = 0; g < D; ++g)
    if (g < G) load_group(g, g);
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  int cur = 0, nxt = D % NBUF;          // buffer of group g / of group g + D
  for (int g = 0; g < G; ++g) {
    // group g has landed when at most the D - 1 younger groups are outstanding (this wave's own loads; the barrier publishes all waves')
    if (D > 1 && g + D - 1 < G) {
      if (TAIL && wid_u == 0) __builtin_amdgcn_s_waitcnt(0x0f70 | ((D - 1) * (LPG + 1)));
      else __builtin_amdgcn_s_waitcnt(0x0f70 | ((D - 1) * LPG));
    } else {
      lds_dma_wait_all();
    }
#ifdef IVX_CONV_TIMELINE
    if (g == 0) tl1 = __builtin_amdgcn_s_memrealtime();      // the first group has landed
#endif
    if constexpr (NBUF == 2) {
      __syncthreads();                  // ... and every wave is done reading the buffer of group g - 1, which group g + D now overwrites
    } else {
      // a ring deeper than two needs a RAW barrier: the fence of __syncthreads() waits for vmcnt(0), i.e. for the whole ring (round 5; the
      // three-buffer rings of rounds 3 - 4 were two-deep rings with a third buffer).  This wave's fragment reads of group g - 1 are complete
      // (its MFMAs consumed them); the clobbers keep LDS accesses on their side of the barrier.
      __builtin_amdgcn_s_waitcnt(0xc07f);
      asm volatile("" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    }
    if (g + D < G) load_group(g + D, nxt);
    const T *Ac = smem + cur * BUF + (DI ? 1 : SW) * wr * TM * 32 * BK;
    const T *Bc = smem + cur * BUF + AROWS * BK + wc * TN * 32 * BK;
#pragma unroll
    for (int kz = 0; kz < 3; ++kz) {
      f32x4 ah[TM], al[TM], bh[TN], bl[TN];
      // A rows of this tap: LDS row SW * o + kz (LDS row 0 is plane row SW * m0 - 1); DI: o + (kz >> 1) in the even (kz 0, 2) / odd (kz 1) half
      const int ar = DI ? rl + (kz >> 1) + (kz & 1) * BM : SW * rl + kz, asw = (ar >> 2) & 3;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        if (ZR && kz != 1) {
          const T *A0 = smem + cur * BUF;
          ah[i] = *reinterpret_cast<const f32x4 *>(A0 + aoff[kz >> 1][i]);
          al[i] = *reinterpret_cast<const f32x4 *>(A0 + (aoff[kz >> 1][i] ^ (2 * EPC)));
        } else {
          const T *rowp = Ac + ((DI ? 1 : SW) * i * 32 + ar) * BK;
          ah[i] = *reinterpret_cast<const f32x4 *>(rowp + ((fh ^ asw) * EPC));
          al[i] = *reinterpret_cast<const f32x4 *>(rowp + (((2 + fh) ^ asw) * EPC));
        }
      }
      const int bsw = (rl >> 2) & 3;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const T *rowp = Bc + (kz * BN + j * 32 + rl) * BK;
        bh[j] = *reinterpret_cast<const f32x4 *>(rowp + ((fh ^ bsw) * EPC));
        bl[j] = *reinterpret_cast<const f32x4 *>(rowp + (((2 + fh) ^ bsw) * EPC));
      }
      if (!ZR && kz != 1) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const bool ok = kz == 0 ? ok0[i] : ok2[i];
          ah[i] = ok ? ah[i] : zero4;
          al[i] = ok ? al[i] : zero4;
        }
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          acc[i][j] = pair_mfma<PAIR>(ah[i], bh[j], acc[i][j]);
          acc[i][j] = pair_mfma<PAIR>(ah[i], bl[j], acc[i][j]);
          acc[i][j] = pair_mfma<PAIR>(al[i], bh[j], acc[i][j]);
        }
    }
    cur = cur + 1 == NBUF ? 0 : cur + 1;
    nxt = nxt + 1 == NBUF ? 0 : nxt + 1;
  }
#ifdef IVX_CONV_TIMELINE
  tl2 = __builtin_amdgcn_s_memrealtime();
#endif
  __syncthreads();                      // the staging area of the epilogue overlaps the ring
  if constexpr (TAIL) {
    conv_epilogue_wide<TM, TN>(p, acc, m0, n0, wr, wc, lane, reinterpret_cast<float *>(smem) + wid_u * 1024, gz * (size_t)p.g_out);
  } else {
    // the same LDS-transposed 16-byte stores (conv_epilogue_wide), plain values, rows limited to the BM - 2 this tile owns
    float *stage = reinterpret_cast<float *>(smem) + wid_u * 1024;
    float *outp = p.out + gz * (size_t)p.g_out;
    const int mlim = (m0 + BMO < M) ? m0 + BMO : M;
    const int col_l = lane & 31, hh = lane >> 5, rrow = lane >> 3, c4 = (lane & 7) * 4;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int nb = n0 + (wc * TN + j) * 32 + c4;
      const bool nok = nb < p.Cout;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) stage[((r & 3) + 8 * (r >> 2) + 4 * hh) * 32 + col_l] = acc[i][j][r];
        const int mb = m0 + (wr * TM + i) * 32 + rrow;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 v = *reinterpret_cast<const f32x4 *>(stage + (rrow + 8 * q) * 32 + c4);
          const int m = mb + 8 * q;
          if (m < mlim && nok) *reinterpret_cast<f32x4 *>(outp + (size_t)m * p.Cout + nb) = v;
        }
      }
    }
  }
#ifdef IVX_CONV_TIMELINE
  if (p.tl && tid == 0) {
    unsigned long long *t = p.tl + ((size_t)blockIdx.z * gridDim.x + blockIdx.x) * 8;
    t[0] = tl0; t[1] = tl1; t[2] = tl2; t[3] = __builtin_amdgcn_s_memrealtime();
    t[4] = __builtin_amdgcn_s_getreg(63492); t[5] = __builtin_amdgcn_s_getreg(63508);
  }
#endif
}

template <int TM, int TN, int WR, int WC, int WPE, int PAIR, int NBUF, int TAIL = 1, int SW = 1, int ZR = 0, int DI = 0>
static void launch_halo(ConvParams &p, hipStream_t st) {
  constexpr int BM = (WR * TM * 32) - (TAIL ? 0 : (SW == 1 ? 2 + ZR : 1)), BN = WC * TN * 32;     // rows a tile stores
  const int64_t in_bytes = (int64_t)p.B * p.D * p.H * p.W * p.Cin * 2, w_bytes = (int64_t)p.Cout * p.K * 2;
  const long long Mt = (p.M + BM - 1) / BM, Nt = (p.Cout + BN - 1) / BN;
  p.bm = BM;
  p.q_total = (int)((Mt + 7) / 8); p.q_begin = 0; p.q_count = p.q_total;
  const dim3 grid((unsigned)(8LL * p.q_total * Nt), 1, p.groups > 1 ? p.groups : 1);
  auto kern = conv_wino_halo_kernel<__bf16, TM, TN, WR, WC, WPE, PAIR, NBUF, TAIL, SW, ZR, DI>;
  hipLaunchKernelGGL(kern, grid, dim3(64 * WR * WC), 0, st, p, (unsigned)in_bytes, (unsigned)w_bytes);
}

// z-BLOCKED form of the same GEMM for shallow columns (Z = 3 or 6: the 256- and 128-channel stride-1 layers of the KITTI neck), where the
// halo kernel multiplies zeros: with z the fastest row index a 32-row MFMA block mixes all z, so the taps that fall outside the column
// (kz = 0 at z = 0, kz = 2 at z = Z - 1: 2 of the 3 Z tap-slices) are issued and masked -- 22 % of the matrix work at Z = 3, 11 % at
// Z = 6, on launches whose clock the matrix pipe already pulls down to 1.7 GHz (PMC).  Here a tile is CT = 32 WCOL whole
// columns and the DMA lanes place plane row m0 + c Z + z at LDS row z CT + c (the lane -> global row map of an LDS-DMA is free): every
// 32-row block of the staged tile then holds ONE z, a wave owns three consecutive output z-blocks of 32 columns and 32 channels, and a
// tap whose source block lies outside the column is a wave-uniform skip -- no masks, no zero products, no halo rows (a tile stores every
// row it stages).  V and M keep their layout: only this kernel's addressing differs.  Per output element the products are accumulated
// in the halo kernel's order (group by group, tap 0, 1, 2), so the results are bit-identical.
// Z = output slices per column (3 or 6); SW = z stride (1, or 2 with Z_in = 2 Z: the source block of output block zo and tap kz is
// SW zo + kz - 1, and only zo = 0, kz = 0 falls outside).
template <typename T, int Z, int WCOL, int WN, int WPE, int PAIR, int SW = 1>
__global__ __launch_bounds__(64 * WCOL * (Z / 3) * WN, WPE) void conv_wino_zblk_kernel(const ConvParams p, const unsigned in_bytes, const unsigned w_bytes) {
  static_assert(Z == 3 || Z == 6, "three output z-blocks per wave");
  constexpr int ZI = SW * Z;                     // input slices per column
  constexpr int ZH = Z / 3, NW = WCOL * ZH * WN, NT = 64 * NW;
  constexpr int CT = WCOL * 32, AR = ZI * CT, BN = WN * 32;
  constexpr int NS = 2 * SW + 3;                 // source blocks of a wave's three output blocks
  constexpr int BK = 32, EPC = 8, NCH = 4, RP = NT / NCH;
  constexpr int APASS = (AR + RP - 1) / RP, BPASS = (3 * BN + RP - 1) / RP;
  static_assert(AR % 16 == 0 && (3 * BN) % 16 == 0, "a wave's 16 rows of a pass are inside or outside as a whole");
  constexpr int BUF = (AR + 3 * BN) * BK;
  __shared__ __attribute__((aligned(16))) T smem[2 * BUF];
  static_assert(sizeof(smem) >= (size_t)NW * 4096, "4 KB of staging LDS per wave for the transposed epilogue");
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wid_u = __builtin_amdgcn_readfirstlane(wid);
  const int cg = wid_u / (ZH * WN), zh = (wid_u / WN) % ZH, nb = wid_u % WN;
  const int M = p.m_dev ? *p.m_dev : p.M;         // device-side row count (see conv_wino_halo_kernel)
  const int q_total = p.m_dev ? ((M + CT * Z - 1) / (CT * Z) + 7) >> 3 : p.q_total;
  int mt, nt;
  {
    const int Nt = (p.Cout + BN - 1) / BN;
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const int lt = idx / Nt;
    nt = idx - lt * Nt;
    mt = xcd * q_total + lt;
    if (p.cp_dst && blockIdx.x == 0 && blockIdx.z == 0 && tid == 0) *p.cp_dst = *p.cp_src;
    if (lt >= q_total) return;
  }
  const int c0 = mt * CT, n0 = nt * BN;          // first column of the tile
  const int m0 = c0 * Z;                         // its first OUTPUT row (columns x Z)
  if (m0 >= M) return;
#ifdef IVX_CONV_TIMELINE
  const unsigned long long tl0 = __builtin_amdgcn_s_memrealtime();
  unsigned long long tl1 = 0, tl2 = 0;
#endif
  const size_t gz = blockIdx.z;
  const __amdgpu_buffer_rsrc_t rs_in =
      __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)p.in + gz * (size_t)p.g_in * sizeof(T)), 0, in_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_w =
      __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)p.wgt + gz * (size_t)p.g_w * sizeof(T)), 0, w_bytes, 0x00020000);
  const int lr = tid / NCH;
  const int cc = (tid & (NCH - 1)) ^ ((lr >> 2) & 3);            // the k-chunk this lane fetches (its LDS slot is tid % NCH); RP % 16 == 0
  const unsigned OOB = 0x80000000u;
  typedef __attribute__((address_space(3))) void *lds_ptr_t;
  unsigned a_base[APASS], b_base[BPASS];
#pragma unroll
  for (int j = 0; j < APASS; ++j) {
    const int li = lr + RP * j;                                  // LDS row: z * CT + c
    const int z = li / CT, c = li - z * CT;
    const int row = (c0 + c) * ZI + z;                           // input plane row of (column, z)
    a_base[j] = (li < AR && row < SW * M) ? ((unsigned)row * (unsigned)p.Cin + cc * EPC) * (unsigned)sizeof(T) : OOB;
  }
#pragma unroll
  for (int j = 0; j < BPASS; ++j) {
    const int r = lr + RP * j, tap = r / BN, n = n0 + (r - tap * BN);
    b_base[j] = (r < 3 * BN && n < p.Cout) ? ((unsigned)n * (unsigned)p.K + tap * 64 + cc * EPC) * (unsigned)sizeof(T) : OOB;
  }
  const int G = p.Cin / BK;
  auto load_group = [&](int g, int buf) {
    T *Ab = smem + buf * BUF + wid_u * (64 / NCH) * BK;     // wave-uniform base; the DMA adds lane * 16 B
    T *Bb = Ab + AR * BK;
    const unsigned ka = (unsigned)g * BK * (unsigned)sizeof(T);
    const unsigned kb = ((unsigned)(g >> 1) * 3u * 64u + (unsigned)(g & 1) * 32u) * (unsigned)sizeof(T);
#pragma unroll
    for (int j = 0; j < APASS; ++j) {
      if (RP * j + wid_u * 16 < AR) {                       // (wave-uniform: the last pass may be a partial one)
        const unsigned vo = a_base[j] == OOB ? OOB : a_base[j] + ka;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_in, (lds_ptr_t)(Ab + RP * j * BK), 16, vo, 0, 0, 0);
      }
    }
#pragma unroll
    for (int j = 0; j < BPASS; ++j) {
      if (RP * j + wid_u * 16 < 3 * BN) {
        const unsigned vo = b_base[j] == OOB ? OOB : b_base[j] + kb;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_ptr_t)(Bb + RP * j * BK), 16, vo, 0, 0, 0);
      }
    }
  };
  const int rl = lane & 31, fh = lane >> 5, sw = (rl >> 2) & 3;
  const int z0 = zh * 3;
  f32x16 acc[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  load_group(0, 0);
  int cur = 0;
  for (int g = 0; g < G; ++g) {
    lds_dma_wait_all();                 // this wave's loads of group g have landed; the barrier publishes all waves'
#ifdef IVX_CONV_TIMELINE
    if (g == 0) tl1 = __builtin_amdgcn_s_memrealtime();
#endif
    __syncthreads();                    // ... and every wave is done reading the other buffer (group g - 1)
    if (g + 1 < G) load_group(g + 1, cur ^ 1);
    const T *A0 = smem + cur * BUF + (cg * 32 + rl) * BK;
    const T *B0 = smem + cur * BUF + AR * BK + (nb * 32 + rl) * BK;
    f32x4 ah[NS], al[NS];               // source blocks SW z0 - 1 .. SW (z0 + 2) + 1 of this wave's columns
#pragma unroll
    for (int s5 = 0; s5 < NS; ++s5) {
      const int zs = SW * z0 + s5 - 1;
      if (zs >= 0 && zs < ZI) {
        const T *rowp = A0 + zs * CT * BK;
        ah[s5] = *reinterpret_cast<const f32x4 *>(rowp + ((fh ^ sw) * EPC));
        al[s5] = *reinterpret_cast<const f32x4 *>(rowp + (((2 + fh) ^ sw) * EPC));
      }
    }
#pragma unroll
    for (int kz = 0; kz < 3; ++kz) {
      const T *rowp = B0 + kz * BN * BK;
      const f32x4 bh = *reinterpret_cast<const f32x4 *>(rowp + ((fh ^ sw) * EPC));
      const f32x4 bl = *reinterpret_cast<const f32x4 *>(rowp + (((2 + fh) ^ sw) * EPC));
#pragma unroll
      for (int zo = 0; zo < 3; ++zo) {
        const int zs = SW * (z0 + zo) + kz - 1;
        if (zs >= 0 && zs < ZI) {       // (wave-uniform) a tap outside the column is skipped, not multiplied by zeros
          acc[zo] = pair_mfma<PAIR>(ah[SW * zo + kz], bh, acc[zo]);
          acc[zo] = pair_mfma<PAIR>(ah[SW * zo + kz], bl, acc[zo]);
          acc[zo] = pair_mfma<PAIR>(al[SW * zo + kz], bh, acc[zo]);
        }
      }
    }
    cur ^= 1;
  }
#ifdef IVX_CONV_TIMELINE
  tl2 = __builtin_amdgcn_s_memrealtime();
#endif
  __syncthreads();                      // the staging area of the epilogue overlaps the ring
  float *stage = reinterpret_cast<float *>(smem) + wid_u * 1024;
  float *outp = p.out + gz * (size_t)p.g_out;
  const int col_l = lane & 31, hh = lane >> 5, rrow = lane >> 3, c4 = (lane & 7) * 4;
  const int nbc = n0 + nb * 32 + c4;
  const bool nok = nbc < p.Cout;
#pragma unroll
  for (int zo = 0; zo < 3; ++zo) {
#pragma unroll
    for (int r = 0; r < 16; ++r) stage[((r & 3) + 8 * (r >> 2) + 4 * hh) * 32 + col_l] = acc[zo][r];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 v = *reinterpret_cast<const f32x4 *>(stage + (rrow + 8 * q) * 32 + c4);
      const int m = m0 + (cg * 32 + rrow + 8 * q) * Z + z0 + zo;      // plane row of (column, z)
      if (m < M && nok) *reinterpret_cast<f32x4 *>(outp + (size_t)m * p.Cout + nbc) = v;
    }
  }
#ifdef IVX_CONV_TIMELINE
  if (p.tl && tid == 0) {
    unsigned long long *t = p.tl + ((size_t)blockIdx.z * gridDim.x + blockIdx.x) * 8;
    t[0] = tl0; t[1] = tl1; t[2] = tl2; t[3] = __builtin_amdgcn_s_memrealtime();
    t[4] = __builtin_amdgcn_s_getreg(63492); t[5] = __builtin_amdgcn_s_getreg(63508);
  }
#endif
}

template <int Z, int WCOL, int WN, int WPE, int SW = 1>
static void launch_zblk(ConvParams &p, hipStream_t st) {
  constexpr int AR = Z * WCOL * 32, BN = WN * 32;          // output rows of a tile
  const int64_t in_bytes = (int64_t)p.B * p.D * p.H * p.W * p.Cin * 2, w_bytes = (int64_t)p.Cout * p.K * 2;
  const long long Mt = (p.M + AR - 1) / AR, Nt = (p.Cout + BN - 1) / BN;
  p.bm = AR;
  p.q_total = (int)((Mt + 7) / 8); p.q_begin = 0; p.q_count = p.q_total;
  const dim3 grid((unsigned)(8LL * p.q_total * Nt), 1, p.groups > 1 ? p.groups : 1);
  auto kern = conv_wino_zblk_kernel<__bf16, Z, WCOL, WN, WPE, 2, SW>;
  hipLaunchKernelGGL(kern, grid, dim3(64 * WCOL * (Z / 3) * WN), 0, st, p, (unsigned)in_bytes, (unsigned)w_bytes);
}

static int zblk_wrong_z(int want, int got) {
  ivx_set_error("ivx_conv_launch_halo: this z-blocked config is built for columns of %d slices, the layer has %d", want, got);
  return IVX_ERR_INVALID_ARG;
}

int ivx_conv_launch_halo(ConvParams &p, int cfg, hipStream_t st) {
  if (p.in_pair != 2) {
    ivx_set_error("ivx_conv_launch_halo: fp16 pair operands only");
    return IVX_ERR_INVALID_ARG;
  }
  switch (cfg) {       // the rows of IVX_CONV_HALO_CFGS (conv_tiles.h)
#define IVX_H(n, TM, TN, WR, WC, WPE, PAIR, NBUF, TAIL, SW, ZR, DI) case n: launch_halo<TM, TN, WR, WC, WPE, PAIR, NBUF, TAIL, SW, ZR, DI>(p, st); return IVX_OK;
#define IVX_Z(n, ZD, WCOL, WN, WPE, SW) \
    case n: if (p.Wo != ZD || (SW > 1 && p.W != SW * ZD)) return zblk_wrong_z(ZD, p.Wo); launch_zblk<ZD, WCOL, WN, WPE, SW>(p, st); return IVX_OK;
    IVX_CONV_HALO_CFGS(IVX_H, IVX_Z)
#undef IVX_H
#undef IVX_Z
    default:
      ivx_set_error("ivx_conv_launch_halo: unknown config %d", cfg);
      return IVX_ERR_INVALID_ARG;
  }
}

// ------------------------------------------------------------------------------------------------
// Round 5: the Winograd-domain GEMM of an F(4x4, 3x3) layer with its OUTPUT TRANSFORM AND EPILOGUE FUSED -- M never reaches HBM.
// (Round-4 verdict item 1; reference layers: mmdet3d/models/necks/imvoxelnet.py:94-123, the ResModule convolutions of the stack necks.)
// A workgroup owns BM - 2 = 62 rows (tile column, z) x 64 output channels for ALL 36 frequency points xi.  It walks xi = (i, j), j fastest;
// for each xi the z-halo K loop of conv_wino_halo_kernel (one staged tile serves the three z-taps; hi*hi + hi*lo + lo*hi per 16-channel pair
// group) leaves M[xi] of its tile in 16 accumulator registers per lane, which are folded into the output domain right away:
//     P[e]      += At[e][j] * M[i][j]          (e = 0 .. 3; after the six j of a row i:)
//     out[a][e] += At[a][i] * P[e]             (a = 0 .. 3)        ->  out = At M A  in 16 + 4 + 1 accumulator tiles instead of 36
// -- an all-xi workgroup that kept M itself would hold 36 tiles (576 registers per lane at this tile size).  The groups of all xi form ONE
// stream of 36 * Cin / 16 iterations through an NBUF-deep LDS ring (16 KB per group: 64 rows of V[xi] and the three taps' 64 filter rows of
// U[xi]), so the pipeline fills once per tile, not once per xi.  The epilogue transposes each of the 16 output tiles through LDS and applies
// the scales of the pair operands, BN scale / shift, residual and ReLU exactly as wino_output_kernel does, writing 16-byte pieces of the
// channels-last output, and leaves the workgroup's max |out| for the next layer's operand scale.
// Cost: the filters of all 36 xi are re-read (from L2) by every row tile: 36 x 12 KB x Cin / 16 per 62 rows; V is read once per 64 output
// channels.  One workgroup per CU (64 KB of LDS, > 256 registers per lane: the accumulators spill into the AGPR half of the file).
__constant__ float kWinoAt4[4][6] = {{1.f, 1.f, 1.f, 1.f, 1.f, 0.f}, {0.f, 1.f, -1.f, 2.f, -2.f, 0.f}, {0.f, 1.f, 1.f, 4.f, 4.f, 0.f}, {0.f, 1.f, -1.f, 8.f, -8.f, 1.f}};

__device__ __forceinline__ float fold4_vscale(const float amax) {      // == winograd.hip wino_pair_vscale: 2^k with 256 amax 2^k in [2^14, 2^15)
  if (!(amax < 3.0e38f)) return 0.00390625f;
  if (!(amax > 0.f)) return 1.0f;
  int e;
  (void)frexpf(amax, &e);
  int k = 15 - 8 - e;
  k = k < -120 ? -120 : (k > 120 ? 120 : k);
  return ldexpf(1.0f, k);
}

template <int PAIR, int NA, int NB>
__global__ __launch_bounds__(256, 1) void conv_wino_fold4_kernel(const ConvParams p, const IvxWinoFold f, const unsigned in_bytes, const unsigned w_bytes) {
  typedef __bf16 T;
  constexpr int BM = 64, BN = 64, NT = 256, BK = 32, EPC = 8, NCH = 4, RP = NT / NCH;
  constexpr int BMO = BM - 2;                       // rows a tile stores (consecutive tiles overlap by two staged rows)
  // Two rings with their own depths: the rows of V[xi] come from HBM (every byte is read once: 2 - 4 us under load), the filter rows of
  // U[xi] from L2 (all 36 banks are re-read by every row tile), and with one wave per SIMD nothing but the ring hides either.  An A slot
  // holds the 64 staged rows and one row that is ALWAYS ZERO (row 64: the DMA never writes it): a lane whose z - 1 / z + 1 neighbour lies
  // outside the column reads that tap's fragments from it -- an address chosen once -- instead of masking 8 registers per group.
  constexpr int ASL = (BM + 1) * BK, BSL = 3 * BN * BK;   // elements per slot of the A ring (4160 B) / of the B ring (12 KB)
  constexpr int NXI = 36;
  static_assert(RP == BM && RP == BN, "one pass of the workgroup's lanes covers the A rows / one tap of the B rows");
  static_assert(NA >= NB && NB >= 3 && (NB - 2) * 4 <= 15, "vmcnt immediates; the A ring runs at least as far ahead as the B ring");
  __shared__ __attribute__((aligned(16))) T smem[NA * ASL + NB * BSL];
  __shared__ float wmax[4];
  static_assert(sizeof(smem) >= 4 * 4096, "4 KB of staging LDS per wave for the transposed epilogue");
  T *const As = smem, *const Bs = smem + NA * ASL;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  int mt, nt;
  {
    const int Nt = (p.Cout + BN - 1) / BN;
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const int lt = idx / Nt;
    nt = idx - lt * Nt;
    mt = xcd * p.q_total + lt;
  }
  if (mt * BMO >= p.M) {                            // padding of the last XCD's range
    if (f.pmax && tid == 0) f.pmax[blockIdx.x] = 0.f;
    return;
  }
  const int m0 = mt * BMO, n0 = nt * BN;
  const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc((void *)p.in, 0, in_bytes, 0x00020000);     // all 36 planes of V
  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc((void *)p.wgt, 0, w_bytes, 0x00020000);      // all 36 filter banks
  const int lr = tid / NCH;
  const int cc = (tid & (NCH - 1)) ^ ((lr >> 2) & 3);
  const int wid_u = __builtin_amdgcn_readfirstlane(wid);
  const unsigned OOB = 0x80000000u;
  typedef __attribute__((address_space(3))) void *lds_ptr_t;
  typedef __attribute__((address_space(3))) T *lds_t;
  // A: LDS row lr of a slot holds plane row m0 - 1 + lr;  B: LDS row t * BN + lr of a slot holds filter row n0 + lr of tap t (chunk-major K).
  // The per-lane part of a request's address never changes (voffset); the group / xi part is a wave-uniform running byte offset (soffset).
  const int arow = m0 - 1 + lr;
  const unsigned a_vo = (arow >= 0 && arow < p.M) ? ((unsigned)arow * (unsigned)p.Cin + cc * EPC) * 2u : OOB;
  unsigned b_vo[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) b_vo[t] = (n0 + lr < p.Cout) ? ((unsigned)(n0 + lr) * (unsigned)p.K + t * 64 + cc * EPC) * 2u : OOB;
  const int G = p.Cin / BK;                                   // 16-channel pair groups per xi
  const unsigned xi_in = (unsigned)p.g_in * 2u, xi_w = (unsigned)p.g_w * 2u;      // byte strides between the xi planes / filter banks
  const int NIT = NXI * G;
  // zero rows of the A slots
  for (int t = tid; t < NA * 16; t += NT) reinterpret_cast<float *>(smem)[(t >> 4) * (ASL / 2) + BM * (BK / 2) + (t & 15)] = 0.f;
  // request cursors (all wave-uniform): byte offset of the next group inside V / U, its group index inside the xi, its ring slot
  unsigned sa = 0, sb = 0;
  int ga = 0, gb = 0, slot_a = 0, slot_b = 0;
  const unsigned a_lds0 = (unsigned)(uintptr_t)(lds_t)As + (unsigned)(wid_u * (64 / NCH) * BK * 2);
  const unsigned b_lds0 = (unsigned)(uintptr_t)(lds_t)Bs + (unsigned)(wid_u * (64 / NCH) * BK * 2);
  auto issue_a = [&]() {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_in, (lds_ptr_t)(uintptr_t)(a_lds0 + (unsigned)slot_a * (ASL * 2)), 16, a_vo, sa, 0, 0);
    sa += BK * 2;
    if (++ga == G) { ga = 0; sa += xi_in - (unsigned)G * (BK * 2); }
    slot_a = slot_a + 1 == NA ? 0 : slot_a + 1;
  };
  auto issue_b = [&]() {
    const unsigned l = b_lds0 + (unsigned)slot_b * (BSL * 2);
#pragma unroll
    for (int t = 0; t < 3; ++t) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_ptr_t)(uintptr_t)(l + t * RP * BK * 2), 16, b_vo[t], sb, 0, 0);
    // next group of the chunk-major K order: the second half of a 32-channel chunk lies 64 bytes on, the next chunk 3 * 128 bytes after the chunk's start
    sb += (gb & 1) ? (3 * 128 - 64) : 64;
    if (++gb == G) { gb = 0; sb += xi_w - (unsigned)(G >> 1) * (3 * 128); }
    slot_b = slot_b + 1 == NB ? 0 : slot_b + 1;
  };
  auto skip_a = [&]() {                                       // advance the A cursor by one group without a request
    sa += BK * 2;
    if (++ga == G) { ga = 0; sa += xi_in - (unsigned)G * (BK * 2); }
    slot_a = slot_a + 1 == NA ? 0 : slot_a + 1;
  };
  const int rl = lane & 31, fh = lane >> 5;
  const int Z = p.Wo;
  const int zl = (m0 + wr * 32 + rl) % Z;                     // z of this lane's output row
  const bool ok0 = zl >= 1, ok2 = zl + 1 < Z;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  // The 16 output-domain tiles live in the AGPR half of the register file (every access below goes through v_accvgpr_read / _write with
  // an "a" operand), the four row accumulators P, the product tile and everything the group loop touches in VGPRs: left to itself the
  // compiler put `out` into VGPRs and P / the product tile into AGPRs, i.e. the moves on the per-xi path instead of the per-row path.
  float outa[4][4][16];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int r = 0; r < 16; ++r) asm volatile("v_accvgpr_write_b32 %0, 0" : "=a"(outa[a][e][r]));
  f32x16 acc, P[4];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) P[e] = acc;
  // Prologue: requests in the order the steady state leaves behind (one A and three B requests per group, group after group; the A ring
  // runs NA - NB groups further ahead, so its extra requests are the OLDEST): A of groups NB - 1 .. NA - 2 first, then (A, B) of 0 .. NB - 2.
  {
    for (int k = 0; k < NB - 1; ++k) skip_a();
    for (int k = NB - 1; k < NA - 1; ++k) issue_a();           // (NIT >= 36 > NA)
    const unsigned e_sa = sa; const int e_ga = ga, e_slot = slot_a;
    sa = 0; ga = 0; slot_a = 0;
    for (int k = 0; k < NB - 1; ++k) { issue_a(); issue_b(); }
    sa = e_sa; ga = e_ga; slot_a = e_slot;                     // next A request: group NA - 1
  }
  // group 0 (and the zero rows) has landed when only the (A, B) pairs of groups 1 .. NB - 2 are younger.  No __syncthreads() from here to
  // the epilogue: its fence waits for vmcnt(0), i.e. for every request of the rings (the first form of this kernel ran at the full memory
  // latency per group whatever the ring depth -- as every deeper ring tried in this library did).  RAW barriers, bracketed by compiler-level
  // memory clobbers; a wave's fragment reads of a group are complete when it arrives (its MFMAs consumed them).
  __builtin_amdgcn_s_waitcnt(0x0070 | ((NB - 2) * 4));        // vmcnt(..) lgkmcnt(0): the zero-row stores too
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  // Fragment reads as inline asm: the compiler's wait-count pass puts s_waitcnt vmcnt(0) in front of any LDS read it can see while an
  // LDS-DMA request is in flight (it cannot tell the ring slots apart).  Byte offsets of this lane's fragments inside a slot (hi chunk fh,
  // lo chunk 2 + fh, XOR-swizzled by the row as the DMA lanes wrote them); a masked tap points at the slot's zero row.
  const unsigned as_lds = (unsigned)(uintptr_t)(lds_t)As, bs_lds = (unsigned)(uintptr_t)(lds_t)Bs;
  unsigned aoh[3], aol[3];
#pragma unroll
  for (int kz = 0; kz < 3; ++kz) {
    const int ar = rl + kz, asw = (ar >> 2) & 3;              // A rows of tap kz: slot row o + kz (row 0 is plane row m0 - 1)
    const bool ok = kz == 0 ? ok0 : (kz == 2 ? ok2 : true);
    aoh[kz] = ok ? (unsigned)(((wr * 32 + ar) * BK + ((fh ^ asw) * EPC)) * 2) : (unsigned)(BM * BK * 2);
    aol[kz] = ok ? (unsigned)(((wr * 32 + ar) * BK + (((2 + fh) ^ asw) * EPC)) * 2) : (unsigned)(BM * BK * 2);
  }
  const int bsw = (rl >> 2) & 3;
  const unsigned boh = (unsigned)(((wc * 32 + rl) * BK + ((fh ^ bsw) * EPC)) * 2), bol = (unsigned)(((wc * 32 + rl) * BK + (((2 + fh) ^ bsw) * EPC)) * 2);
#define FOLD_DS_READ(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))
  unsigned abase = as_lds, bbase = bs_lds;                    // slot bases of the current group
  int it = 0;
  // Three nested loops (i, j, group) over ONE request stream: the innermost touches only the product tile and the fragments.
  for (int i = 0; i < 6; ++i) {
    for (int j = 0; j < 6; ++j) {
      for (int gq = 0; gq < G; ++gq, ++it) {
        f32x4 ah[3], al[3], bh[3], bl[3];
        {
          const unsigned b0 = bbase + boh, b1 = bbase + bol;
          FOLD_DS_READ(ah[0], abase + aoh[0], 0); FOLD_DS_READ(al[0], abase + aol[0], 0);
          FOLD_DS_READ(bh[0], b0, 0);             FOLD_DS_READ(bl[0], b1, 0);
          FOLD_DS_READ(ah[1], abase + aoh[1], 0); FOLD_DS_READ(al[1], abase + aol[1], 0);
          FOLD_DS_READ(bh[1], b0, BN * BK * 2);   FOLD_DS_READ(bl[1], b1, BN * BK * 2);
          FOLD_DS_READ(ah[2], abase + aoh[2], 0); FOLD_DS_READ(al[2], abase + aol[2], 0);
          FOLD_DS_READ(bh[2], b0, 2 * BN * BK * 2); FOLD_DS_READ(bl[2], b1, 2 * BN * BK * 2);
        }
        // LDS returns in order: tap 0's four fragments are there when eight reads are outstanding, and so on (the operands tie the MFMAs
        // to the wait).  The four requests that refill the slots group it - 1 left (A: group it + NA - 1, B: group it + NB - 1) are issued
        // BETWEEN the MFMAs: an LDS-DMA instruction holds the issuing wave for 60 - 180 cycles, which only its own matrix work can cover.
        asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(ah[0]), "+v"(al[0]), "+v"(bh[0]), "+v"(bl[0]));
        acc = pair_mfma<PAIR>(ah[0], bh[0], acc);
        acc = pair_mfma<PAIR>(ah[0], bl[0], acc);
        __builtin_amdgcn_sched_barrier(0);
        if (it + NA - 1 < NIT) issue_a();
        __builtin_amdgcn_sched_barrier(0);
        acc = pair_mfma<PAIR>(al[0], bh[0], acc);
        asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(ah[1]), "+v"(al[1]), "+v"(bh[1]), "+v"(bl[1]));
        acc = pair_mfma<PAIR>(ah[1], bh[1], acc);
        acc = pair_mfma<PAIR>(ah[1], bl[1], acc);
        acc = pair_mfma<PAIR>(al[1], bh[1], acc);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ah[2]), "+v"(al[2]), "+v"(bh[2]), "+v"(bl[2]));
        acc = pair_mfma<PAIR>(ah[2], bh[2], acc);
        __builtin_amdgcn_sched_barrier(0);
        if (it + NB - 1 < NIT) issue_b();
        __builtin_amdgcn_sched_barrier(0);
        acc = pair_mfma<PAIR>(ah[2], bl[2], acc);
        acc = pair_mfma<PAIR>(al[2], bh[2], acc);
        // group it + 1 must have landed: younger are the requests of groups it + 2 .. it + NB - 1 (B ring) with their A partners while
        // the A ring still issues
        if (it + 1 < NIT) {
          if (it + NA - 1 < NIT) __builtin_amdgcn_s_waitcnt(0x0f70 | ((NB - 2) * 4));         // steady state
          else if (it + NB - 1 < NIT) __builtin_amdgcn_s_waitcnt(0x0f70 | ((NB - 2) * 3));    // the A ring has run dry: only B requests are younger
          else lds_dma_wait_all();
          asm volatile("" ::: "memory");
          __builtin_amdgcn_s_barrier();   // group it + 1 is visible to every wave; every wave is done with the slots of group `it`
          asm volatile("" ::: "memory");
        }
        abase = abase + ASL * 2 == as_lds + NA * ASL * 2 ? as_lds : abase + ASL * 2;
        bbase = bbase + BSL * 2 == bs_lds + NB * BSL * 2 ? bs_lds : bbase + BSL * 2;
      }
      // M[xi] of this tile is complete (xi = 6 i + j): fold it into the row accumulators
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float c = kWinoAt4[e][j];
        if (c != 0.f) P[e] = c * acc + P[e];
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    }
    // the six j of row i are in: out[a][e] += At[a][i] * P[e]
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const float c = kWinoAt4[a][i];
      if (c != 0.f) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float t;
            asm("v_accvgpr_read_b32 %0, %1" : "=v"(t) : "a"(outa[a][e][r]));
            t = __builtin_fmaf(c, P[e][r], t);
            asm("v_accvgpr_write_b32 %0, %1" : "=a"(outa[a][e][r]) : "v"(t));
          }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int r = 0; r < 16; ++r) P[e][r] = 0.f;
  }
  __syncthreads();                      // the staging area of the epilogue overlaps the rings
  // ---- epilogue: out[a][e] is the (4 tx + a, 4 ty + e) output of the tile rows; as wino_output_kernel: v = act(M * sc + sf [+ res])
  float *stage = reinterpret_cast<float *>(smem) + wid_u * 1024;
  const float mscale = 1.0f / (fold4_vscale(__uint_as_float(f.hdr_v[0])) * f.uscale[0]);
  const int col_l = lane & 31, hh = lane >> 5, rrow = lane >> 3, c4 = (lane & 7) * 4;
  const int nb = n0 + wc * 32 + c4;
  const bool nok = nb < p.Cout;
  f32x4 sc = {mscale, mscale, mscale, mscale}, sf = {0.f, 0.f, 0.f, 0.f};
  if (nok && f.scale) sc = mscale * *reinterpret_cast<const f32x4 *>(f.scale + nb);
  if (nok && f.shift) sf = *reinterpret_cast<const f32x4 *>(f.shift + nb);
  size_t base[4];
  int xlim[4], ylim[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int o = wr * 32 + rrow + 8 * q, m = m0 + o;
    xlim[q] = 0; ylim[q] = 0; base[q] = 0;
    if (o < BMO && m < p.M && nok) {
      const int z = m % Z, col = m / Z;
      const int ty = col % f.TY, t2 = col / f.TY;
      const int tx = t2 % f.TX, b = t2 / f.TX;
      base[q] = ((((size_t)b * f.Xo + 4 * tx) * f.Yo + 4 * ty) * Z + z) * (size_t)f.Co + nb;
      xlim[q] = f.Xo - 4 * tx;
      ylim[q] = f.Yo - 4 * ty;
    }
  }
  const size_t ystep = (size_t)Z * f.Co, xstep = (size_t)f.Yo * ystep;
  float omax = 0.f;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float t;
        asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(t) : "a"(outa[a][e][r]));
        stage[((r & 3) + 8 * (r >> 2) + 4 * hh) * 32 + col_l] = t;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 v = *reinterpret_cast<const f32x4 *>(stage + (rrow + 8 * q) * 32 + c4);
        if (a < xlim[q] && e < ylim[q]) {
          const size_t o = base[q] + a * xstep + e * ystep;
          v = v * sc + sf;
          f32x4 rr = zero4;
          if (f.res_mode) rr = *reinterpret_cast<const f32x4 *>(f.res + o);
          if (f.res_mode && !f.res_after_act) v += rr;
          if (f.relu) {
            v[0] = v[0] > 0.f ? v[0] : 0.f; v[1] = v[1] > 0.f ? v[1] : 0.f;
            v[2] = v[2] > 0.f ? v[2] : 0.f; v[3] = v[3] > 0.f ? v[3] : 0.f;
          }
          if (f.res_mode && f.res_after_act) v += rr;
          v *= f.post_scale;
          *reinterpret_cast<f32x4 *>(f.out + o) = v;
          omax = fmaxf(omax, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
        }
      }
    }
  if (f.pmax) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) omax = fmaxf(omax, __shfl_xor(omax, o));
    if (lane == 0) wmax[wid_u] = omax;
    __syncthreads();
    if (tid == 0) f.pmax[blockIdx.x] = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
  }
}

// workgroups of the fused launch for M rows and Cout channels (= entries of its partial-maximum array)
int ivx_conv_fold4_blocks(long long M, int Cout) {
  const long long Mt = (M + 61) / 62, Nt = (Cout + 63) / 64;
  return (int)(8 * ((Mt + 7) / 8) * Nt);
}

int ivx_conv_launch_fold4(ConvParams &p, const IvxWinoFold &f, int n2, hipStream_t st) {
  if (p.in_pair != 2 || n2 != 36 || p.kmode != 1 || p.Cin % 64 != 0 || p.K != 3 * p.Cin) {
    ivx_set_error("ivx_conv_launch_fold4: fp16 pair operands, F(4x4,3x3), chunk-major filters, Cin %% 32 == 0 and a 3-tap z kernel only");
    return IVX_ERR_INVALID_ARG;
  }
  const long long in_bytes = (long long)n2 * p.g_in * 2, w_bytes = (long long)n2 * p.g_w * 2;
  if (in_bytes >= (1LL << 31) || w_bytes >= (1LL << 31)) {
    ivx_set_error("ivx_conv_launch_fold4: the %d transformed planes must stay below 2 GiB together", n2);
    return IVX_ERR_UNSUPPORTED;
  }
  const long long Mt = (p.M + 61) / 62, Nt = (p.Cout + 63) / 64;
  p.bm = 62;
  p.q_total = (int)((Mt + 7) / 8); p.q_begin = 0; p.q_count = p.q_total;
  const dim3 grid((unsigned)(8LL * p.q_total * Nt));
  hipLaunchKernelGGL((conv_wino_fold4_kernel<2, 16, 5>), grid, dim3(256), 0, st, p, f, (unsigned)in_bytes, (unsigned)w_bytes);      // A ring 16 slots, B ring 5: 124 KB (8 + 4 and 20 + 5 slots measured the same)
  return IVX_OK;
}
#endif

#if IVX_CONV_TU == 1
int ivx_conv_launch_f32(ConvParams &p, const ConvPlan &pl, hipStream_t st) {
  if (launch_tile<float, IVX_FAM_F32>(p, pl.cfg, st)) return IVX_OK;
  ivx_set_error("ivx_conv_fwd: tile %d is not an fp32 LDS-DMA tile", pl.cfg);
  return IVX_ERR_INVALID_ARG;
}
#endif

#if IVX_CONV_TU == 2
int ivx_conv_launch_lowp(ConvParams &p, const ConvPlan &pl, hipStream_t st) {
  if (p.in_fp8 ? launch_tile<fp8_t, IVX_FAM_E4M3>(p, pl.cfg, st) : launch_tile<__bf16, IVX_FAM_BF16>(p, pl.cfg, st)) return IVX_OK;
  ivx_set_error("ivx_conv_fwd: tile %d is not a bf16 / e4m3 LDS-DMA tile", pl.cfg);
  return IVX_ERR_INVALID_ARG;
}
#endif

#if IVX_CONV_TU == 0
// (a template, as launch_tile is, so that the rows of the other families are discarded before they instantiate a kernel)
template <int FAM>
static bool launch_generic_tile(const ConvParams &p, int cfg, hipStream_t st) {
  switch (cfg) {
#define IVX_ROW(n, fam, TM, TN, WR, WC, BK, WPE, NB, RPF, WG) \
    case n: if constexpr ((IVX_FAM_##fam & FAM) != 0) { launch_cfg<TM, TN, WR, WC>(p, st); return true; } else return false;
    IVX_CONV_TILES(IVX_ROW)
#undef IVX_ROW
    default: return false;
  }
}

static int launch_one(ConvParams &p, const ConvPlan &pl, hipStream_t st) {
  if (p.in_pair) return p.in_pair == 2 ? ivx_conv_launch_pair_f16(p, pl, st) : ivx_conv_launch_pair_bf16(p, pl, st);
  if (pl.cfg >= 40) return (p.in_bf16 || p.in_fp8) ? ivx_conv_launch_lowp(p, pl, st) : ivx_conv_launch_f32(p, pl, st);
  if (launch_generic_tile<IVX_FAM_GENERIC>(p, pl.cfg, st)) return IVX_OK;
  ivx_set_error("ivx_conv_fwd: unknown tile override %d", pl.cfg);
  return IVX_ERR_INVALID_ARG;
}

static void launch_reduce(const ConvParams &p, hipStream_t st) {
  const size_t total = (size_t)8 * p.q_count * p.bm * p.Cout;
  if (p.pio && (p.Cout & 3) == 0 && total < (1ull << 31)) {
    size_t b4 = (total / 4 + 255) / 256;
    if (b4 > 4096) b4 = 4096;
    hipLaunchKernelGGL(conv_splitk_reduce_pio_kernel, dim3((unsigned)b4), dim3(256), 0, st, p);
    return;
  }
  size_t blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(conv_splitk_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, st, p);
}

static int run_conv(ConvParams &p, const ConvPlan &pl, void *workspace, hipStream_t st) {
  TileInfo ti;
  if (p.in_fp8 && (!dma_applicable(p) || pl.cfg < 91 || pl.cfg > 94)) {
    ivx_set_error("ivx_conv_fwd: fp8 input is only implemented by the LDS-DMA kernel (tensor < 2 GiB, kernel extents <= 8)");
    return IVX_ERR_UNSUPPORTED;
  }
  const bool deep_cfg = tile_deep_form(pl.cfg);      // deep-ring / residual-prefetch pair tiles
  if (p.in_bf16 && (!dma_applicable(p) || !(tile_info(pl.cfg, &ti) && ((pl.cfg >= 61 && pl.cfg < 91) || (deep_cfg && p.in_pair))))) {
    ivx_set_error("ivx_conv_fwd: bf16 input is only implemented by the LDS-DMA kernel (tensor < 2 GiB, kernel extents <= 8)");
    return IVX_ERR_UNSUPPORTED;
  }
  if (p.kmode == 1 && (!dma_applicable(p) || pl.cfg < 40)) {
    ivx_set_error("ivx_conv_fwd: wgt_layout 1 is only implemented by the LDS-DMA kernel (tensor < 2 GiB, kernel extents <= 8)");
    return IVX_ERR_UNSUPPORTED;
  }
  p.stagger_ticks = 0;
  if (p.pio && p.res_mode == 1 && pl.ksplit <= 1 && pl.tail_ks <= 1 && tile_info(pl.cfg, &ti)) {
    // (experiment, default off: IVX_PIO_STAGGER_US = delay in us, IVX_PIO_STAGGER_SHIFT = which bit of the XCD-local workgroup index picks the late half)
    const int st_us = (int)conv_env().pio_stagger_us, st_sh = (int)conv_env().pio_stagger_shift;
    const long long tiles = (long long)((p.M + ti.bm - 1) / ti.bm) * ((p.Cout + ti.bn - 1) / ti.bn);
    if (st_us > 0 && tiles >= 2LL * 256 * ti.wg_per_cu) {
      p.stagger_ticks = st_us * 100;
      p.stagger_shift = st_sh;
      p.stagger_first = 32 * ti.wg_per_cu;
    }
  }
  int rc;
  if (pl.tail_ks > 1) {
    // full rounds ...
    p.q_total = pl.q_total; p.q_begin = 0; p.q_count = pl.qa; p.ksplit = 1; p.partial = nullptr;
    if ((rc = launch_one(p, pl, st)) != IVX_OK) return rc;
    // ... then the remainder, K split so that it fills every workgroup slot once
    p.q_begin = pl.qa; p.q_count = pl.q_total - pl.qa; p.ksplit = pl.tail_ks; p.partial = (float *)workspace;
    if ((rc = launch_one(p, pl, st)) != IVX_OK) return rc;
    launch_reduce(p, st);
    return IVX_OK;
  }
  if (pl.ksplit > 1) {
    p.ksplit = pl.ksplit;
    p.partial = (float *)workspace;
  }
  if ((rc = launch_one(p, pl, st)) != IVX_OK) return rc;
  if (pl.ksplit > 1) launch_reduce(p, st);
  return IVX_OK;
}

// Plan (and with `launch`, run) the whole problem: one call, or one call per batch slice.  *need = workspace bytes.  rec: the plans of the
// distinct slices are written there (ivx_conv_plan_query).
static int conv_dispatch(const ConvParams &p, bool allow_ws, bool launch, void *workspace, int64_t workspace_bytes, hipStream_t st,
                         int64_t *need, const char *who, ivx_conv_plan_rec *rec = nullptr) {
  const int nb = conv_batch_slice(p);
  if (rec) rec->slice_samples = nb;
  *need = 0;
  for (int b0 = 0; b0 < p.B; b0 += nb) {
    ConvParams q = nb == p.B ? p : conv_slice_params(p, b0, (p.B - b0) < nb ? (p.B - b0) : nb);
    const ConvPlan pl = plan_conv(q, allow_ws);
    if (pl.ws_bytes > *need) *need = pl.ws_bytes;
    if (rec && rec->n_slices < 2 && (rec->n_slices == 0 || rec->samples[rec->n_slices - 1] != q.B)) {
      const int i = rec->n_slices++;
      rec->samples[i] = q.B; rec->cfg[i] = pl.cfg; rec->ksplit[i] = pl.ksplit; rec->tail_ks[i] = pl.tail_ks; rec->q_total[i] = pl.q_total;
      rec->qa[i] = pl.qa; rec->bm[i] = pl.bm; rec->slice_ws[i] = pl.ws_bytes;
    }
    if (!launch) continue;
    if (pl.ws_bytes > 0 && (!workspace || workspace_bytes < pl.ws_bytes)) {
      ivx_set_error("%s: workspace too small (%lld < %lld); size it with ivx_conv_workspace_bytes", who, (long long)workspace_bytes,
                    (long long)pl.ws_bytes);
      return IVX_ERR_WORKSPACE;
    }
    const int rc = run_conv(q, pl, workspace, st);
    if (rc != IVX_OK) return rc;
  }
  return IVX_OK;
}

extern "C" int ivx_conv_fwd(const ivx_conv_desc *d, const void *in, const void *wgt, const float *scale,
                            const float *shift, const void *res, void *out, ivx_stream_t stream) {
  ConvParams p;
  int rc = fill_params(d, in, wgt, scale, shift, res, out, &p);
  if (rc != IVX_OK) return rc;
  int64_t need;
  rc = conv_dispatch(p, false, true, nullptr, 0, (hipStream_t)stream, &need, "ivx_conv_fwd");
  if (rc != IVX_OK) return rc;
  IVX_CHECK_LAUNCH("ivx_conv_fwd");
  return IVX_OK;
}

// Internal (winograd.hip): can the grouped launch of `d` take its row count from the device (ConvParams::m_dev)?  Only the z-halo and
// z-blocked kernels read it.
int ivx_conv_grouped_rows_dev_ok(const ivx_conv_desc *d, int groups) {
  ConvParams p;
  float dummy;
  if (!d || fill_params(d, &dummy, &dummy, nullptr, nullptr, nullptr, &dummy, &p) != IVX_OK || !dma_applicable(p)) return 0;
  return grouped_halo_cfg(p, d, groups) != 0;
}

// Internal (winograd.hip): `groups` independent convolutions of the same shape in ONE launch of the LDS-DMA kernel
// (grid.z = group), identity epilogue.  `d` describes one group; operands of group g start g*stride elements further.
int ivx_conv_grouped_launch(const ivx_conv_desc *d, int groups, const float *in, long long g_in, const float *wgt, long long g_w,
                            float *out, long long g_out, hipStream_t st, const unsigned *cp_src, unsigned *cp_dst, const int *m_dev) {
  ConvParams p;
  int rc = fill_params(d, in, wgt, nullptr, nullptr, nullptr, out, &p);
  if (rc != IVX_OK) return rc;
  IVX_REQUIRE(groups >= 1 && groups <= 65535, "ivx_conv_grouped_launch: bad group count");
  IVX_REQUIRE((d->in_dtype == IVX_F32 || d->in_dtype == IVX_BF16_PAIR || d->in_dtype == IVX_F16_PAIR) && d->out_dtype == IVX_F32 &&
                  d->out_mode == 0 && d->res_mode == 0,
              "ivx_conv_grouped_launch: fp32 or pair operands, plain fp32 output only");
  if (!dma_applicable(p)) {
    ivx_set_error("ivx_conv_grouped_launch: one group must stay below 2 GiB");
    return IVX_ERR_UNSUPPORTED;
  }
  // (after the argument checks: a rejected call has no side effect -- round-5 advisor)
  if (cp_dst && !p.in_pair) {                    // (only the pair-operand kernels carry the word; not reached by the library's own callers)
    if (hipMemcpyAsync(cp_dst, cp_src, 4, hipMemcpyDeviceToDevice, st) != hipSuccess) {
      ivx_set_error("ivx_conv_grouped_launch: hipMemcpyAsync failed");
      return IVX_ERR_HIP;
    }
  } else {
    p.cp_src = cp_src; p.cp_dst = cp_dst;
  }
  p.groups = groups; p.g_in = g_in; p.g_w = g_w; p.g_out = g_out;
  p.m_dev = m_dev;
  if (const int halo_cfg = grouped_halo_cfg(p, d, groups)) return ivx_conv_launch_halo(p, halo_cfg, st);
  if (m_dev) {
    ivx_set_error("ivx_conv_grouped_launch: only the z-halo and z-blocked kernels take a device-side row count");
    return IVX_ERR_UNSUPPORTED;
  }
  const ConvPlan pl = grouped_tile_plan(p, groups);
  TileInfo t;
  if (!tile_info(pl.cfg, &t) || (pl.cfg >= 61) != (p.in_pair != 0)) {
    ivx_set_error("ivx_conv_grouped_launch: tile %d does not match the operand type", pl.cfg);
    return IVX_ERR_INVALID_ARG;
  }
  return launch_one(p, pl, st);
}

// Internal (winograd.hip): the n2 = 36 Winograd-domain convolutions of an F(4x4,3x3) layer with the output transform and the layer's epilogue
// fused into the launch (conv_wino_fold4_kernel).  `d` describes one xi convolution (as for ivx_conv_grouped_launch).
int ivx_conv_grouped_fold4(const ivx_conv_desc *d, int groups, const float *in, long long g_in, const float *wgt, long long g_w, const IvxWinoFold *f,
                           hipStream_t st) {
  ConvParams p;
  float dummy;
  int rc = fill_params(d, in, wgt, nullptr, nullptr, nullptr, &dummy, &p);
  if (rc != IVX_OK) return rc;
  IVX_REQUIRE(d->in_dtype == IVX_F16_PAIR && d->KD == 1 && d->KH == 1 && d->KW == 3 && d->sw == 1 && d->pw == 1 && d->wgt_layout == 1 && f && f->out,
              "ivx_conv_grouped_fold4: fp16 pair operands, 1x1x3 along z with stride 1 and padding 1, chunk-major filters");
  p.groups = groups; p.g_in = g_in; p.g_w = g_w; p.g_out = 0;
  return ivx_conv_launch_fold4(p, *f, groups, st);
}

extern "C" int64_t ivx_conv_workspace_bytes(const ivx_conv_desc *d) {
  ConvParams p;
  float dummy;
  if (fill_params(d, &dummy, &dummy, nullptr, nullptr, d && d->res_mode ? &dummy : nullptr, &dummy, &p) != IVX_OK) return -1;
  int64_t need;
  if (conv_dispatch(p, true, false, nullptr, 0, nullptr, &need, "ivx_conv_workspace_bytes") != IVX_OK) return -1;
  return need;
}

extern "C" int ivx_conv_fwd_ws(const ivx_conv_desc *d, const void *in, const void *wgt, const float *scale,
                               const float *shift, const void *res, void *out, void *workspace, int64_t workspace_bytes,
                               ivx_stream_t stream) {
  ConvParams p;
  int rc = fill_params(d, in, wgt, scale, shift, res, out, &p);
  if (rc != IVX_OK) return rc;
  int64_t need;
  rc = conv_dispatch(p, true, true, workspace, workspace_bytes, (hipStream_t)stream, &need, "ivx_conv_fwd_ws");
  if (rc != IVX_OK) return rc;
  IVX_CHECK_LAUNCH("ivx_conv_fwd_ws");
  return IVX_OK;
}

extern "C" int64_t ivx_conv_pio_workspace_bytes(const ivx_conv_desc *d, const ivx_pair_io *io) {
  ConvParams p;
  float dummy;
  if (!io) { ivx_set_error("ivx_conv_pio_workspace_bytes: null pair io"); return -1; }
  if (fill_params(d, &dummy, &dummy, nullptr, nullptr, d && d->res_mode ? &dummy : nullptr, &dummy, &p, io) != IVX_OK) return -1;
  int64_t need;
  if (conv_dispatch(p, true, false, nullptr, 0, nullptr, &need, "ivx_conv_pio_workspace_bytes") != IVX_OK) return -1;
  return need;
}

extern "C" int ivx_conv_fwd_pio(const ivx_conv_desc *d, const ivx_pair_io *io, const void *in, const void *wgt, const float *scale, const float *shift,
                                const void *res, void *out, void *workspace, int64_t workspace_bytes, ivx_stream_t stream) {
  ConvParams p;
  IVX_REQUIRE(io, "ivx_conv_fwd_pio: null pair io");
  int rc = fill_params(d, in, wgt, scale, shift, res, out, &p, io);
  if (rc != IVX_OK) return rc;
  int64_t need;
  rc = conv_dispatch(p, true, true, workspace, workspace_bytes, (hipStream_t)stream, &need, "ivx_conv_fwd_pio");
  if (rc != IVX_OK) return rc;
  IVX_CHECK_LAUNCH("ivx_conv_fwd_pio");
  return IVX_OK;
}

extern "C" int ivx_conv_fwd_pio_naive(const ivx_conv_desc *d, const ivx_pair_io *io, const void *in, const void *wgt, const float *scale, const float *shift,
                                      const void *res, void *out, ivx_stream_t stream) {
  ConvParams p;
  IVX_REQUIRE(io, "ivx_conv_fwd_pio_naive: null pair io");
  int rc = fill_params(d, in, wgt, scale, shift, res, out, &p, io);
  if (rc != IVX_OK) return rc;
  const size_t total = (size_t)p.M * p.Cout;
  size_t blocks = (total + 255) / 256;
  if (blocks > 65536 * 8) blocks = 65536 * 8;
  hipLaunchKernelGGL(conv_naive_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
  IVX_CHECK_LAUNCH("ivx_conv_fwd_pio_naive");
  return IVX_OK;
}

extern "C" int ivx_conv_pair_supported(const ivx_conv_desc *d) {
  if (!d || d->in_dtype != IVX_F32 || d->out_dtype != IVX_F32 || d->out_mode != 0 || d->Cin % 16 != 0 || d->Cin <= 0) return 0;
  if (d->wgt_layout == 1 && d->Cin % 32 != 0) return 0;
  if (d->KD > 8 || d->KH > 8 || d->KW > 8 || d->KD < 1 || d->KH < 1 || d->KW < 1) return 0;
  const int64_t in_b = (int64_t)d->B * d->D * d->H * d->W * d->Cin * 4, w_b = (int64_t)d->Cout * d->KD * d->KH * d->KW * d->Cin * 4;
  return in_b < (1LL << 31) && w_b < (1LL << 31) ? 1 : 0;   // no batch slicing in this form: the caller falls back to fp32 MFMA
}

extern "C" int ivx_conv_fwd_naive(const ivx_conv_desc *d, const void *in, const void *wgt, const float *scale,
                                  const float *shift, const void *res, void *out, ivx_stream_t stream) {
  ConvParams p;
  int rc = fill_params(d, in, wgt, scale, shift, res, out, &p);
  if (rc != IVX_OK) return rc;
  const size_t total = (size_t)p.M * p.Cout;
  size_t blocks = (total + 255) / 256;
  if (blocks > 65536 * 8) blocks = 65536 * 8;
  hipLaunchKernelGGL(conv_naive_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
  IVX_CHECK_LAUNCH("ivx_conv_fwd_naive");
  return IVX_OK;
}
// Lab (include/imvoxel_lab.h): what the planner answers, from the functions the launchers above call.  No launch, no device call.
extern "C" int ivx_conv_tile_info(int cfg, int32_t *v) {
  TileInfo t;
  if (!v || !tile_info(cfg, &t)) return 0;
  v[0] = t.bm; v[1] = t.bn; v[2] = t.bk; v[3] = t.wg_per_cu;
  return 1;
}

extern "C" int ivx_conv_plan_query(const ivx_conv_desc *d, const ivx_pair_io *io, int allow_ws, int groups, ivx_conv_plan_rec *out) {
  IVX_REQUIRE(out && groups >= 0, "ivx_conv_plan_query: null record or negative group count");
  memset(out, 0, sizeof(*out));
  ConvParams p;
  float dummy;
  if (groups == 0) {
    int rc = fill_params(d, &dummy, &dummy, nullptr, nullptr, d && d->res_mode ? &dummy : nullptr, &dummy, &p, io);
    if (rc != IVX_OK) return rc;
    return conv_dispatch(p, allow_ws != 0, false, nullptr, 0, nullptr, &out->ws_bytes, "ivx_conv_plan_query", out);
  }
  int rc = fill_params(d, &dummy, &dummy, nullptr, nullptr, nullptr, &dummy, &p);
  if (rc != IVX_OK) return rc;
  if (!dma_applicable(p)) {
    ivx_set_error("ivx_conv_plan_query: one group must stay below 2 GiB");
    return IVX_ERR_UNSUPPORTED;
  }
  out->rows_dev_ok = ivx_conv_grouped_rows_dev_ok(d, groups);
  out->halo_cfg = grouped_halo_cfg(p, d, groups);
  if (out->halo_cfg) return IVX_OK;
  TileInfo t;
  out->grouped_tile = grouped_tile_plan(p, groups).cfg;
  out->tile_matches = tile_info(out->grouped_tile, &t) && (out->grouped_tile >= 61) == (p.in_pair != 0);
  return IVX_OK;
}
#endif   // IVX_CONV_TU == 0
