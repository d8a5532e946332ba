// The convolution planner: see conv_plan.h.  Host code only.
#include "conv_plan.h"
#include <stdlib.h>

ConvLab &conv_lab() {
  static thread_local ConvLab lab;
  return lab;
}
extern "C" int ivx_conv_set_tile_override(int cfg) {
  conv_lab().tile_override = cfg;
  return IVX_OK;
}
extern "C" int ivx_conv_set_halo_mode(int mode) {
  conv_lab().halo_mode = mode;
  return IVX_OK;
}
extern "C" int ivx_conv_set_plan_mode(int mode) {
  conv_lab().plan_mode = mode;
  return IVX_OK;
}
extern "C" int ivx_conv_set_epilogue_mode(int narrow) {
  conv_lab().narrow_epilogue = narrow ? 1 : 0;
  return IVX_OK;
}

const ConvEnv &conv_env() {
  static const ConvEnv env = [] {
    ConvEnv e;
    const char *v;
#define IVX_READ(field, name, def) e.field = (v = getenv(name)) ? atoll(v) : def;
    IVX_CONV_ENV(IVX_READ)
#undef IVX_READ
    return e;
  }();
  return env;
}

bool dma_applicable(const ConvParams &p) {
  const int el = p.in_fp8 ? 1 : (p.in_bf16 ? 2 : 4);
  const int64_t in_b = (int64_t)p.B * p.D * p.H * p.W * p.Cin * el, w_b = (int64_t)p.Cout * p.K * el;
  return in_b < (1LL << 31) && w_b < (1LL << 31) && p.KD <= 8 && p.KH <= 8 && p.KW <= 8;
}

// Kernel / tile / split-K choice (measured per layer on MI355X with tools/conv_bench.py).
//  * Big problems want the 128-row tiles with the best MFMA : staging ratio; BK 16 keeps LDS at 32 KB and the
//    128 x 128 kernel is compiled for <= 128 registers (launch bound 4 waves/SIMD), so four workgroups share a CU
//    (+2.5 % per layer over three; measured).  When 128 x 128 tiles would not fill the workgroup slots several
//    times over -- every ResNet/FPN layer at KITTI resolution, the indoor necks -- 64 x 64 tiles win by occupancy.
//  * When even 64 x 64 tiles leave most of the 256 CUs idle and K is long (ResNet stage 4, FPN laterals on C5, the
//    coarse levels of the indoor necks), K is split across grid.y and a second pass sums the slices.
//  * Grid tail: with uniform tiles the last partial round costs a whole workgroup time on a few CUs while the rest
//    idle (measured: 10 044 tiles on 768 slots = 13.08 rounds runs 4 % slower per tile than exactly 13 rounds).
//    When the remainder is at most half a round, the full rounds run as one launch and the remainder as a second
//    launch with K split so that it fills every slot once (needs the caller's workspace: ivx_conv_fwd_ws).
//  * The LDS-DMA kernel (cfg 4x/5x fp32, 6x/7x bf16) is used whenever its preconditions hold, else the same tile on
//    the generic kernel (cfg 1..7).
ConvPlan plan_conv(const ConvParams &p, bool allow_ws) {
  const ConvLab &lab = conv_lab();
  const ConvEnv &env = conv_env();
  ConvPlan pl = {lab.tile_override, 1, 1, 0, 0, 0, 0};
  const bool dma_ok = dma_applicable(p);
  bool small = false;
  if (pl.cfg == 0 && dma_ok && !p.in_bf16 && p.Cout > 32 && lab.plan_mode == 0) {
    // fp32 LDS-DMA kernel: score the three tile shapes by (tile efficiency) x (useful fraction of the padded tile grid) x (fill
    // of the last round of workgroup slots) and take the best.  The round-1 rule (128 x 128 from 2500 tiles on, else 64 x 64)
    // left the mid-sized layers of the 2-D trunk -- 900 .. 2500 big tiles, i.e. 0.9 .. 2.4 rounds of 1024 slots -- on 64 x 64
    // tiles at ~0.8 of the big tile's rate, or on a half-empty second round; 128 x 64 at five per CU sits in between.
    // Efficiencies are the measured per-tile rates on long layers relative to 128 x 128 (141 / 131 / 113 TFLOP/s).
    // Short K (the 1x1 layers up to 512 input channels): one or two K slabs per tile, the tile's time is its epilogue and the
    // latency of its loads, and six 128 x 64 workgroups per CU (56) overlap those better than four 128 x 128: interleaved A/B
    // at 50 views (tools/conv_ab.py, profiles/r02_conv_ab_f32.log) 64->256 0.547 vs 0.640 ms, 128->512 0.378 vs 0.417,
    // 256->1024 0.293 vs 0.310, 512->2048 0.269 vs 0.290; from K = 1024 on the 128 x 128 tile is ahead again.
    const bool short_k = p.K <= 512;
    const int c64 = p.K <= 640 ? 47 : 46;
    const int cand[3] = {54, short_k ? 56 : 49, c64};
    const double eff[3] = {short_k ? 0.93 : 1.00, short_k ? 1.00 : 0.93, short_k ? 0.85 : 0.80};
    double best = -1.0;
    for (int i = 0; i < 3; ++i) {
      TileInfo ti;
      tile_info(cand[i], &ti);
      const double tiles = (double)((p.M + ti.bm - 1) / ti.bm) * ((p.Cout + ti.bn - 1) / ti.bn);
      const double util = (double)p.M * p.Cout / (tiles * ti.bm * ti.bn);
      const double rounds = tiles / (256.0 * ti.wg_per_cu);
      const double fill = rounds >= 1.0 ? rounds / (double)(long long)(rounds + 0.999999) : rounds;
      const double score = eff[i] * util * fill;
      if (score > best) { best = score; pl.cfg = cand[i]; }
    }
    small = pl.cfg == c64;
    // (Round 6, measured and not adopted -- profiles/r06_skinny_convs.md: 128 x 128 / 256 x 128 tiles + split K for the layers of a few hundred rows
    // under a K loop of 13824 .. 27648 (512 -> 512 at 10 x 10 x 4): 0.084 -> 0.140 / 0.243 ms per launch.  These launches are bound by the number of
    // slabs a workgroup runs one after the other, not by L2 -> LDS bytes: 64 x 64 tiles with K split 27 ways stay.)
  }
  if (pl.cfg == 0) {
    const long long nblk = (long long)((p.M + 127) / 128) * ((p.Cout + 127) / 128);
    if (p.Cout <= 32) {
      pl.cfg = dma_ok ? 44 : 4;
      // the head convs of the indoor configs (Cout = 25) on the coarse levels: 4 .. 25 row tiles under a K loop of 54 .. 108 slabs ran as that
      // many workgroups, one slab after the other (89 us for 69 MFLOP at 10 x 10 x 4); K is split as for every other small layer
      // (IVX_CONV_SKINNY=0: the round-5 rule, for A/B)
      small = dma_ok && !p.in_bf16 && !p.in_fp8 && env.skinny != 0;
    } else if (nblk >= 2500) {
      pl.cfg = p.Cout > 64 ? (dma_ok ? 54 : 1) : (dma_ok ? (p.K <= 640 ? 49 : 56) : 3);   // 49: the stem
    } else {
      // short-K layers (1x1 convolutions, 3x3 on 64 channels, the stem) are staging/latency-bound: the 64-byte-row
      // variant at six workgroups per CU keeps more loads in flight; long-K layers prefer the 128-byte rows
      pl.cfg = dma_ok ? (p.K <= 640 ? 47 : 46) : 6;
      small = true;
    }
  }
  if (p.in_fp8) {
    // e4m3 storage (2-D trunk of the bf16 + fp8 mode): HBM / latency-bound like the bf16 trunk, same rule: 128 x 128 at four per
    // CU, 128 x 64 for Cout <= 64, 64 x 64 (+ split K) when the tiles would not fill the workgroup slots
    if (lab.tile_override >= 91 && lab.tile_override <= 94) {
      pl.cfg = lab.tile_override;
    } else {
      const long long t128 = (long long)((p.M + 127) / 128) * ((p.Cout + 127) / 128);
      if (p.Cout <= 64) pl.cfg = ((long long)((p.M + 127) / 128) * 2 > 256 * 5) ? 92 : 93;
      else pl.cfg = t128 * 2 > 1024 ? 91 : 93;
      small = pl.cfg == 93;
    }
  }
  if (p.in_bf16 && lab.tile_override == 0 && dma_ok && p.Cout > 32 && lab.plan_mode == 0) {
    // bf16: interleaved A/B over the layers of the 2-D trunk at 50 views (tools/conv_ab.py, profiles/r02_conv_ab_bf16.log).
    // At 8x the MFMA rate every 1x1 layer and most 3x3 layers are bound by HBM / staging latency, and what matters is how
    // many workgroups a CU holds to overlap one tile's epilogue with another's loads: 128 x 128 with 64-byte LDS rows at four
    // per CU (74) is the best or within 5 % of it on all of them (the 1 / 2 per CU of 82 / 81 / 61 lose 20-40 % on short K);
    // Cout <= 64 takes 128 x 64 (63).  The 8- / 16-wave tiles keep the long-K layers with many tiles (the 3-D necks), and
    // layers that would leave most workgroup slots empty keep the 64 x 64 + split-K path below.
    const long long t128 = (long long)((p.M + 127) / 128) * ((p.Cout + 127) / 128);
    if (p.Cout <= 64) {
      if ((long long)((p.M + 127) / 128) * 2 > 256 * 3) pl.cfg = 63;
    } else if (t128 * 2 > 1024 && !(t128 >= 2500 && p.K >= 1024)) {
      pl.cfg = 74;
    }
    if (pl.cfg == 63 || pl.cfg == 74) small = false;
  }
  if (p.in_bf16 && pl.cfg >= 41 && pl.cfg <= 57) {
    // same tile, bf16 instantiation -- except for the big layers: at 8x the MFMA rate the kernel is bound by the
    // L2 -> LDS staging traffic (ablation: +33 % without the loads), so the 256 x 128 / 256 x 256 workgroups of 8 / 16
    // waves, which move 25 % / 50 % fewer bytes per flop, win there (measured, tools/conv_bench.py --dtype bf16)
    if (lab.tile_override == 0 && pl.cfg == 54) pl.cfg = p.Cout > 128 ? 82 : 81;   // 16 / 8 waves: less L2->LDS traffic per flop
    else if (pl.cfg == 54 || pl.cfg == 55) pl.cfg = 74;
    else if (pl.cfg == 48) pl.cfg = 66;
    else if (pl.cfg == 49 || pl.cfg == 56) pl.cfg = 73;
    else if (pl.cfg == 57) pl.cfg = 72;
    else if (pl.cfg <= 53) pl.cfg += 20;   // 41..47, 51..53 -> 61..67, 71..73
  }
  if (p.in_pair && lab.tile_override == 0) {   // pair operands are instantiated for a subset of the bf16 tiles
    if (pl.cfg == 64) pl.cfg = 67;
    else if (pl.cfg == 71) pl.cfg = 74;
    else if (pl.cfg == 72) pl.cfg = 73;
  }
  if (p.in_pair == 2 && p.pio && lab.tile_override == 0 && dma_ok && env.pio_rule) {        // (IVX_PIO_RULE, IVX_PIO_SPLITK: A/B knobs of the round-4 measurements)
    // Chained fp16-pair activations (the 2-D trunk): interleaved A/B of every pair tile on the trunk's layer shapes at KITTI batch 4 and at
    // 50 views (tools/pio_ab.py, profiles/r04_pio_ab_*.md).  128 x 128 with 64-byte LDS rows at four per CU (74) is the best or within
    // 5-10 % of it wherever it fills the chip, also for Cout = 64 at KITTI size (half of its B tile is zero fill, and it still beats
    // 128 x 64 / 256 x 64: 43 vs 50 / 47 us); the 50-view maps of 64 output channels take 256 x 64 (76); layers with few tiles take
    // 64 x 64 with 128-byte rows (66: 63 vs 90 us on 256 -> 256 3x3 at 24 x 80 x 4, 49 vs 58 on 1024 -> 256) + split K.
    const long long t128 = (long long)((p.M + 127) / 128) * ((p.Cout + 127) / 128);
    if (p.Cout <= 64) pl.cfg = p.M >= 400000 ? 76 : (p.M >= 60000 ? 74 : 66);
    else pl.cfg = t128 >= 200 ? 74 : 66;
    small = pl.cfg == 66 && env.pio_splitk;
    // Round 5: a launch with fewer tiles than the chip has workgroup slots (every /8 .. /32 layer of the trunk at KITTI's batch of 4: 240 - 480
    // tiles) cannot hide its slab latency behind other resident workgroups; it takes the deep-ring form of its tile (166 / 174: FOUR slabs
    // in flight per workgroup, raw barriers; bit-identical results) unless the split-K rule below takes it.  Measured (profiles/
    // r05_trunk_deep_ring.md): trunk span 3.85 -> 3.39 ms at KITTI; tiles <= 512 is the best threshold (1024 / 2048 / all: 3.61 -- above one
    // tile per slot the 64 KB workgroups lose more occupancy than the depth returns).  The first form of the deep ring kept __syncthreads(),
    // whose fence waits for vmcnt(0): no effect in the model and +25 us per launch in isolation.  IVX_PIO_DEEP=0 turns the rule off (A/B).
    if (env.pio_deep == 4) {
      TileInfo td;
      tile_info(pl.cfg, &td);
      const long long tl = (long long)((p.M + td.bm - 1) / td.bm) * ((p.Cout + td.bn - 1) / td.bn);
      const int Sd = (p.K + td.bk - 1) / td.bk;
      const bool will_split = small && allow_ws && Sd >= 16 && tl <= env.pio_split_tiles && (tl <= 100 || Sd >= 48);      // (the rule of the split-K block below)
      if (!will_split && p.kmode == 1 && Sd >= env.pio_deep_slabs && tl <= env.pio_deep_tiles && (pl.cfg == 66 || pl.cfg == 74)) {      // (only these two have a deep-ring form)
        pl.cfg += 100;       // 66 -> 166, 74 -> 174
        // ... and the 128 x 128 tile runs on MORE WAVES where the launch leaves SIMDs idle: 16 waves (179: wave tile 32 x 32, 128-byte rows, 128 KB, one
        // workgroup per CU) up to one tile per CU, 8 waves (177: wave tile 64 x 32) up to two.  A slab's LDS-DMA requests, fragment reads, barriers
        // and the epilogue are issued by 4x / 2x the waves (workgroup timelines, profiles/r05_trunk_wg_timeline.md: 512 -> 128 at 48 x 160 x 4
        // 27.1 -> 23.1 -> 20.2 us, 128 -> 128 3x3 46.8 -> 41.1 -> 34.9, 512 -> 2048 + residual at 12 x 40 33.5 -> 26.9 -> 21.9).  Same products in
        // the same order per output: bit-identical.
        if (pl.cfg == 174) pl.cfg = tl <= env.pio_w16_tiles ? 179 : (tl <= env.pio_w8_tiles ? 177 : 174);
        small = false;
      }
    }
    // Round 6: the 256 x 256 tile on 16 waves (183: three-buffer ring, one workgroup per CU; built for the neck's last layer) for the wide layers of the
    // multi-view maps -- half the L2 -> LDS bytes per product of the 128 x 128 tile.  It wins where its tiles fill the 256 CUs in whole rounds: interleaved
    // A/B over the trunk's layers at 50 / 20 ScanNet views, nuScenes and KITTI (tools/pio_ab.py --cfgs 0,74,81,82,183; profiles/r06_tile183_trunk.md):
    // 235 - 1876 tiles at 50 views -5 .. -19 % per launch (1024 -> 256 0.141 -> 0.114 ms, 256 -> 256 3x3 0.239 -> 0.202, 256 -> 1024 + residual 0.225 -> 0.215),
    // 272 tiles (1.06 rounds) +4 .. +10 %, 94 - 136 tiles +30 %; the nearest-upsampled FPN laterals lose 4 %.  Rule: last-round fill of the 256 x 256 grid
    // >= 0.7.  Same products in the same order per output: bit-identical.  IVX_PIO_T183=0 turns it off (A/B).
    if (env.pio_t183 && pl.cfg == 74 && p.in_pair == 2 && p.kmode == 1 && p.res_mode != 2 && p.Cout >= 256 && p.Cout % 256 == 0) {
      const long long t256 = (long long)((p.M + 255) / 256) * (p.Cout / 256);
      const long long rounds = (t256 + 255) / 256;
      if (t256 * 10 >= rounds * 256 * 7) {
        pl.cfg = 183;
        small = false;
      }
    }
  }
  TileInfo t;
  if (!tile_info(pl.cfg, &t) || !dma_ok) return pl;
  const long long Mt = (p.M + t.bm - 1) / t.bm, Nt = (p.Cout + t.bn - 1) / t.bn;
  pl.q_total = (int)((Mt + 7) / 8);
  pl.bm = t.bm;
  if (!allow_ws || lab.tile_override != 0) return pl;
  const int S = (p.K + t.bk - 1) / t.bk;
  if (small) {
    const long long tiles = Mt * Nt;
    const long long slots = 256LL * t.wg_per_cu;           // resident workgroups on the chip
    // Pair IO: at 16-bit MFMA rates a tile is short and a split costs a second launch plus the partial sums' round trip, so it pays only
    // below about one tile per CU, and for the mid-sized layers only when the K loop is long.  Measured through bench.py's trunk span
    // (profiles/r04_pio_split_rule.md): KITTI 4.24 ms with the fp32 rule (2 * tiles <= slots), 4.01 without any split, 3.88 with
    // tiles <= 320; single-view SUN RGB-D 2.42 without, 2.06 with tiles <= 320, 1.86 with tiles <= 100 (its 150 / 160-tile layers have
    // K loops of 16 .. 36 slabs and lose from the split; KITTI's 240-tile layers have 64 .. 144 and gain).
    const bool pio_split = tiles <= env.pio_split_tiles && (tiles <= 100 || S >= 48);
    if ((p.pio ? pio_split : 2 * tiles <= slots) && S >= 16) {     // under half a round: split K until the slots are filled once
      long long ks = (slots + tiles - 1) / tiles;
      if (ks > S / 8) ks = S / 8;
      if (ks > 32) ks = 32;
      if (ks >= 2) {
        pl.ksplit = (int)ks;
        pl.ws_bytes = ivx_align_up((int64_t)ks * 8 * pl.q_total * t.bm * p.Cout * 4, 256);
      }
    }
    return pl;
  }
  // tail plan
  // (Round 6: not for pair IO.  At 16-bit MFMA rates a tile is short: the second launch + the partial sums' round trip + the reduction cost more than
  // the idle slots of the last round -- the same layers run 5 - 12 % faster as ONE launch (tools/pio_ab.py, cfg 0 vs the same tile forced:
  // nuScenes 512 -> 1024 s2 0.177 -> 0.156 ms, 256 -> 512 s2 0.215 -> 0.195, 256 -> 128 0.257 -> 0.235; profiles/r06_tile183_trunk.md (c)).  IVX_PIO_TAIL=1 restores it.)
  if (p.pio && !env.pio_tail) return pl;
  const long long spx = 32LL * t.wg_per_cu;              // workgroup slots per XCD
  const long long bpx = (long long)pl.q_total * Nt;      // workgroups per XCD
  const long long fr = bpx / spx, rem = bpx - fr * spx;
  if (fr >= 2 && rem > 0 && 2 * rem <= spx && (fr * spx) % Nt == 0) {
    long long ks = spx / rem;
    if (ks > S / 8) ks = S / 8;
    if (ks > 16) ks = 16;
    if (ks >= 2) {
      pl.tail_ks = (int)ks;
      pl.qa = (int)(fr * spx / Nt);
      pl.ws_bytes = ivx_align_up((int64_t)ks * 8 * (pl.q_total - pl.qa) * t.bm * p.Cout * 4, 256);
    }
  }
  return pl;
}

// Batch slicing: the LDS-DMA kernel addresses its operands with 31-bit buffer offsets.  When the input of a launch
// reaches 2 GiB (e.g. the first KITTI neck layers from batch 13 up) the batch is cut into the largest slices that fit
// and the slices run back to back on the stream, sharing the workspace; B is the outermost dimension, so a slice is a
// pointer offset.  Returns the number of samples per slice (B = no slicing needed or not possible).
int conv_batch_slice(const ConvParams &p) {
  if (dma_applicable(p) || p.B == 1 || p.KD > 8 || p.KH > 8 || p.KW > 8) return p.B;
  const int el = p.in_fp8 ? 1 : (p.in_bf16 ? 2 : 4);
  const int64_t in_s = (int64_t)p.D * p.H * p.W * p.Cin * el;
  if ((int64_t)p.Cout * p.K * el >= (1LL << 31) || in_s >= (1LL << 31)) return p.B;
  const int64_t nb = ((1LL << 31) - 1) / in_s;
  return (int)(nb < p.B ? nb : p.B);
}

ConvParams conv_slice_params(const ConvParams &p, int b0, int nb) {
  ConvParams q = p;
  const size_t in_el = p.in_fp8 ? 1 : (p.in_bf16 ? 2 : 4), out_el = p.out_fp8 ? 1 : (p.out_bf16 ? 2 : 4);
  const size_t in_s = (size_t)p.D * p.H * p.W * p.Cin;
  const size_t out_s = p.out_mode == 1 ? (size_t)8 * p.D * p.H * p.W * p.Cr : (size_t)p.Do * p.Ho * p.Wo * p.Cout;
  q.B = nb;
  q.M = nb * p.Do * p.Ho * p.Wo;
  q.in = (const float *)((const char *)p.in + (size_t)b0 * in_s * in_el);
  q.out = (float *)((char *)p.out + (size_t)b0 * out_s * out_el);
  if (p.res) {
    const size_t res_s = p.res_mode == 2 ? (size_t)p.rH * p.rW * p.Cout : out_s;
    q.res = (const float *)((const char *)p.res + (size_t)b0 * res_s * out_el);
  }
  return q;
}

// The grouped launches of winograd.hip (ivx_conv_grouped_launch, conv_igemm.hip).
// the default rule takes the z-blocked tile (conv_wino_zblk_kernel, config 50) for 3-slice columns with more than 64 output channels
static bool zblk_rule(const ConvParams &p) { return p.Wo == 3 && p.W == 3 && p.Cout > 64; }

// Fraction of the 3 Z tap-slices a stride-1, pad-1 Winograd-domain GEMM issues under the default rule (for FLOP accounting: the z-blocked
// tile skips the taps outside the column, the halo tile multiplies zeros there).  d: the LAYER descriptor (W = slices, KW = 3).
extern "C" float ivx_conv_winograd_issued_fraction(const ivx_conv_desc *d) {
  const ConvLab &lab = conv_lab();
  if (!d || d->wino_operands != IVX_F16_PAIR || d->KW != 3 || d->sw != 1 || d->pw != 1 || d->W != 3 || d->Cin % 64 || d->Cout <= 64 || d->wgt_layout != 1 ||
      lab.halo_mode >= 0 || lab.tile_override != 0)
    return 1.0f;
  return 7.0f / 9.0f;
}

// The z-halo / z-blocked config (ivx_conv_launch_halo) the library's rule gives one xi convolution of a grouped launch, 0 = another kernel.
int grouped_halo_cfg(const ConvParams &p, const ivx_conv_desc *d, int groups) {
  const ConvLab &lab = conv_lab();
  const ConvEnv &env = conv_env();
  // z-halo kernel (TU 5): 1x1x3 along z, stride 1, pad 1, chunk-major fp16 pairs -- the ResModule layers of the stack necks
  if (p.in_pair == 2 && p.kmode == 1 && d->KD == 1 && d->KH == 1 && d->KW == 3 && d->sw == 2 && d->pw == 1 && p.W == 2 * p.Wo && p.Cin % 64 == 0 &&
      (halo_mode_stride(lab.halo_mode) == 2 || (lab.halo_mode < 0 && lab.tile_override == 0))) {
    // (round 4, tools/halo_ab.py, profiles/r04_halo_ab.md: the zero-row form 42 vs 22: 0.494 / 0.790 vs 0.492 / 0.811 ms; de-interleaved staging
    // 43 / 45: equal -- neither the masks nor the bank conflicts are what this kernel waits for)
    return lab.halo_mode >= 21 ? lab.halo_mode : 42;
  }
  if (p.in_pair == 2 && p.kmode == 1 && d->KD == 1 && d->KH == 1 && d->KW == 3 && d->sw == 1 && d->pw == 1 && p.Cin % 64 == 0 &&
      (halo_mode_stride(lab.halo_mode) == 1 || (lab.halo_mode < 0 && lab.tile_override == 0))) {
    // measured (tools/pair_ab.py --halo N, profiles/r03b_pair_ab_halo.log; generic kernel 0.73 / 0.90 / 1.41 ms for Cout 64 / 128 / 256):
    // with the 16-row tail pass: 128 x 64 at three per CU 0.57 / 0.84 / 1.44, 256 x 64 0.60-0.64 / 0.83 / 1.33, 256 x 128 0.99 / 0.84 / 1.37,
    // 256 x 256 (16 waves) 1.40-1.44 / 1.19 / 1.24-1.27; every three-buffer ring is slower than its two-buffer form (resident workgroups
    // hide the load latency better than depth does).  Overlapping tiles without the tail pass: 126 x 64 at FOUR per CU 0.49 / 0.74 / 1.35,
    // 254 x 64 0.51 / 0.72 / 1.23, 254 x 128 (8 waves, two per CU) 0.65 / 0.64 / 1.15, 254 x 256 1.19 / 1.10 / 1.20
    // round 4: the zero-row forms (30 / 33: the fragment ADDRESS of a masked tap selected once per tile instead of 32 v_cndmask per group):
    // 125 x 64 0.487 / 0.756 / 1.410 (= 10), 253 x 128 0.597 / 0.644 / 1.144 (13: 0.607 / 0.653 / 1.167); bit-identical results
    // round 4, z-blocked tiles for 3-slice columns (50: a tap outside the column is skipped instead of multiplied by zeros: 7 of 9
    // tap-slices): 256 -> 256 at 216 x 248 x 3 0.99 vs 1.135-1.15 ms, bit-identical; at 6 slices (60) 0.626-0.651 vs 0.637-0.650: a wash
    // round 6: small volumes (the indoor necks: 200 .. 1600 rows per Winograd position).  The 253 x 128 tile on 8 waves leaves most CUs idle there --
    // 72 workgroups for 256 -> 256 at 20 x 20 x 8 -- and the 125 x 64 tile at four per CU wins for every Cout: 0.073 -> 0.050 ms (12 launches per ScanNet v1
    // step), 512 -> 512 0.208 -> 0.163, 128 -> 128 at 40 x 40 x 16 0.037 -> 0.033 (tools/neck_halo_ab.py, profiles/r06_halo_small_volumes.md); bit-identical
    // results.  Rule: fewer workgroups of the 253 x 128 tile than the chip has slots for them (512).  IVX_HALO_SMALL=0 turns it off (A/B).
    const bool few = env.halo_small && p.Cout > 64 && !zblk_rule(p) && (long long)((p.M + 252) / 253) * ((p.Cout + 127) / 128) * groups < 512;
    return lab.halo_mode > 0 ? lab.halo_mode : ((p.Cout <= 64 || few) ? 30 : (zblk_rule(p) ? 50 : 33));
  }
  return 0;
}

// The tile of the LDS-DMA kernel a grouped launch takes when no z-halo / z-blocked config applies.
ConvPlan grouped_tile_plan(const ConvParams &p, int groups) {
  const ConvLab &lab = conv_lab();
  ConvPlan pl = {lab.tile_override, 1, 1, 0, 0, 0, 0};
  if (pl.cfg == 0 && p.in_pair) {
    // pair operands: three bf16-rate products per staged operand pair; 8- / 16-wave workgroups stage the fewest bytes per product
    // (tools/gemm_ab.py --pair, profiles/r03_gemm_ab_pair.log)
    // measured on the KITTI neck (tools/pair_ab.py, profiles/r03_pair_ab.log): Cout 64: 256 x 64 at four per CU 0.69 ms (128 x 64: 0.74-0.84);
    // Cout 128: 256 x 128 8 waves 0.60 / 0.88 (128 x 128: 0.63 / 0.89); Cout 256: 256 x 256 16 waves 0.87 / 1.39 (8 waves: 0.91 / 1.41)
    // round 5: the 256 x 256 tile with a THREE-buffer ring behind raw barriers (183; one workgroup of 16 waves per CU either way): the last KITTI
    // neck layer (256 -> 256, z 3 -> 1: a dense GEMM with K = 3 Cin, 48 slabs of 1.9 us for 0.64 us of matrix work) 0.633 -> 0.579 ms (four
    // buffers 0.582; tools/l9_ab.py); same products in the same order
    pl.cfg = p.Cout <= 64 ? 76 : (p.Cout <= 128 ? 81 : (p.in_pair == 2 && p.kmode == 1 ? 183 : 82));
    // few tiles (the 2-D 3x3 layers of the trunk at KITTI size, the indoor necks): the 8- / 16-wave tiles would leave most CUs idle
    const long long nblk = (long long)groups * ((p.M + 127) / 128) * ((p.Cout + 127) / 128);
    if (nblk < 2500) pl.cfg = 67;
  }
  if (pl.cfg == 0) {
    const long long nblk = (long long)groups * ((p.M + 127) / 128) * ((p.Cout + 127) / 128);
    if (p.Cout <= 32) pl.cfg = 44;
    // measured on the Winograd-domain GEMMs of the KITTI neck (tools/conv_bench.py --winograd --wcfgs ...): K is only
    // KW*Cin here (192 .. 768), so a workgroup's prologue and epilogue weigh more than in the direct form and one more
    // resident workgroup per CU pays: 128 x 64 at six per CU for Cout <= 64 (1.51 vs 1.85 ms at five), 128 x 128 at five
    // per CU up to K = 512 (2.50 vs 2.90 ms at four); at K = 768 four and five tie
    // re-measured with the LDS-transposed epilogue, configs interleaved inside one process (tools/gemm_ab.py,
    // profiles/r02_gemm_ab.log; run-to-run spread exceeds most tile effects otherwise): the shorter epilogue removes the
    // advantage of a fifth / sixth resident workgroup -- 128 x 128 at four per CU wins for every Cout >= 128 layer
    // (K = 192: 1.05 vs 1.12 ms at five; K = 384: 1.79 vs 1.86; K = 768: 3.37 vs 3.40), 128 x 64 at five for Cout <= 64
    // (1.08 vs 1.09 at six, 1.14 for 256 x 64)
    // round 3, same tool with the 8-wave 256 x 128 tile added: it wins only the 128 -> 128 layers (K = 384: 1.838 vs
    // 1.903 ms, spreads disjoint) and ties at K = 192 / 768 (profiles/r03_gemm_ab.log)
    else if (nblk >= 2500) pl.cfg = p.Cout > 64 ? (p.Cout == 128 && p.K == 384 ? 58 : 54) : 49;
    else pl.cfg = p.K <= 640 ? 47 : 46;
  }
  return pl;
}
