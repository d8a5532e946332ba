// The tile numbers of the convolution kernels (conv_igemm.hip): ONE table for the LDS-DMA and generic tiles, one for the z-halo / z-blocked
// configs.  Everything that knows a number reads it from here -- the planner's tile figures, the launch switches of the translation units
// (each expands the rows of its own operand family, so it instantiates those kernels and no others), the accepted-number tests.  Adding,
// dropping or re-shaping a tile is an edit of one row.  Plain C++: no HIP types, so the host-only planner (conv_plan.cpp) includes it too.
#ifndef IVX_CONV_TILES_H_
#define IVX_CONV_TILES_H_

// Operand families: which instantiations of a row exist.
enum {
  IVX_FAM_GENERIC = 1,      // conv_igemm_f32_kernel (64-bit addressing), TU 0
  IVX_FAM_F32 = 2,          // conv_igemm_v4_kernel<float>, TU 1
  IVX_FAM_BF16 = 4,         // <__bf16>, TU 2
  IVX_FAM_E4M3 = 8,         // <fp8_t>, TU 2
  IVX_FAM_PAIR_BF16 = 16,   // <__bf16, PAIR = 1>, TU 3
  IVX_FAM_PAIR_F16 = 32,    // <__bf16, PAIR = 2>, TU 4
  IVX_FAM_PAIRS = IVX_FAM_PAIR_BF16 | IVX_FAM_PAIR_F16,
  IVX_FAM_BF16_PAIRS = IVX_FAM_BF16 | IVX_FAM_PAIRS,
};

// X(number, families, TM, TN, WR, WC, BK, WPE, NB, RPF, wg_per_cu)
//   TM x TN   MFMA tiles of 32 x 32 per wave;  WR x WC waves: the block tile is (WR TM 32) x (WC TN 32)
//   BK        K slab in stored elements;  WPE the launch bound (waves per SIMD the kernel is compiled for);  NB buffers of the LDS ring;
//   RPF       residual prefetch;  wg_per_cu the PLANNER's occupancy figure (not always WPE: LDS or registers may bind first)
// Generic rows use the first four template arguments only and take no M-tile plan (wg_per_cu 0).
#define IVX_CONV_TILES(X)                                                                                                                           \
  X(1, GENERIC, 2, 2, 2, 2, 32, 0, 2, 0, 0)        /* 128 x 128, 2 workgroups/CU */                                                                 \
  X(2, GENERIC, 2, 2, 4, 1, 32, 0, 2, 0, 0)        /* 256 x 64, 1 workgroup/CU */                                                                   \
  X(3, GENERIC, 2, 1, 2, 2, 32, 0, 2, 0, 0)        /* 128 x 64 */                                                                                   \
  X(4, GENERIC, 1, 1, 4, 1, 32, 0, 2, 0, 0)        /* 128 x 32 */                                                                                   \
  X(5, GENERIC, 1, 2, 4, 1, 32, 0, 2, 0, 0)        /* 128 x 64 (wave 32 x 64) */                                                                    \
  X(6, GENERIC, 1, 1, 2, 2, 32, 0, 2, 0, 0)        /* 64 x 64 */                                                                                    \
  X(7, GENERIC, 1, 2, 2, 2, 32, 0, 2, 0, 0)        /* 64 x 128 */                                                                                   \
  X(41, F32, 2, 2, 2, 2, 32, 1, 2, 0, 2)           /* LDS-DMA: 128 x 128, 128-byte LDS rows */                                                      \
  X(43, F32, 2, 1, 2, 2, 32, 1, 2, 0, 3)           /*          128 x 64 */                                                                          \
  X(44, F32, 1, 1, 4, 1, 32, 1, 2, 0, 4)           /*          128 x 32 */                                                                          \
  X(46, F32, 1, 1, 2, 2, 32, 1, 2, 0, 5)           /*          64 x 64 */                                                                           \
  X(51, F32, 2, 2, 2, 2, 16, 1, 2, 0, 3)           /*          128 x 128, 64-byte rows: 32 KB LDS, 3 workgroups/CU */                               \
  X(53, F32, 2, 1, 2, 2, 16, 1, 2, 0, 5)                                                                                                            \
  X(52, F32, 2, 2, 4, 1, 16, 1, 2, 0, 3)           /*          256 x 64, 64-byte rows: 40 KB LDS */                                                 \
  X(54, F32, 2, 2, 2, 2, 16, 4, 2, 0, 4)           /* 51 squeezed to 128 registers: 4 workgroups/CU */                                              \
  X(55, F32, 2, 2, 2, 2, 16, 5, 2, 0, 5)           /*    ... to 102 registers: 5 workgroups/CU (all 160 KB of LDS) */                               \
  X(56, F32, 2, 1, 2, 2, 16, 6, 2, 0, 6)           /* 53 at 6 workgroups/CU */                                                                      \
  X(57, F32, 2, 2, 4, 1, 16, 4, 2, 0, 4)           /* 52 at 4 workgroups/CU */                                                                      \
  X(58, F32, 2, 2, 4, 2, 16, 4, 2, 0, 2)           /* 8 waves, 256 x 128: two workgroups per CU, half the tiles per FLOP */                         \
  X(59, F32, 2, 2, 2, 4, 16, 4, 2, 0, 2)           /* 8 waves, 128 x 256 */                                                                         \
  X(47, F32, 1, 1, 2, 2, 16, 6, 2, 0, 6)           /* 64 x 64, 64-byte rows: 16 KB LDS, 6 workgroups/CU */                                          \
  X(48, F32, 1, 2, 2, 2, 16, 5, 2, 0, 5)           /* 64 x 128 */                                                                                   \
  X(49, F32, 2, 1, 2, 2, 16, 5, 2, 0, 5)           /* 128 x 64 at 5 workgroups/CU */                                                                \
  /* bf16 operands, v_mfma_f32_32x32x16_bf16 (cfg + 20: same tile, same LDS bytes, BK counts bf16 elements); pair operands (IVX_BF16_PAIR /         \
     IVX_F16_PAIR) are instantiated for a subset of them, with the three-product K loop */                                                          \
  X(63, BF16_PAIRS, 2, 1, 2, 2, 64, 1, 2, 0, 3)                                                                                                     \
  X(66, BF16_PAIRS, 1, 1, 2, 2, 64, 1, 2, 0, 5)                                                                                                     \
  X(67, BF16_PAIRS, 1, 1, 2, 2, 32, 6, 2, 0, 6)                                                                                                     \
  X(73, BF16_PAIRS, 2, 1, 2, 2, 32, 1, 2, 0, 5)                                                                                                     \
  X(75, PAIRS, 2, 1, 2, 2, 32, 5, 2, 0, 5)         /* 73 at five workgroups per CU */                                                               \
  X(74, BF16_PAIRS, 2, 2, 2, 2, 32, 4, 2, 0, 4)    /* 71 at 4 workgroups/CU */                                                                      \
  X(61, BF16_PAIRS, 2, 2, 2, 2, 64, 1, 2, 0, 2)                                                                                                     \
  X(81, BF16_PAIRS, 2, 2, 4, 2, 32, 4, 2, 0, 2)    /* 8 waves, 256 x 128: 25 % less L2->LDS traffic per flop */                                     \
  X(82, BF16_PAIRS, 2, 2, 4, 4, 32, 4, 2, 0, 1)    /* 16 waves, 256 x 256: half the traffic per flop */                                             \
  X(83, BF16_PAIRS, 2, 2, 4, 2, 64, 2, 2, 0, 1)    /* 8 waves, 256 x 128, 128-byte rows */                                                          \
  /* larger wave tiles: fewer LDS fragment reads per product (the pair loop reads 4 fragments for 3 products; at 16x the fp32 MFMA rate             \
     the LDS port, shared by the DMA writes and the fragment reads, is as busy as the matrix pipe) */                                               \
  X(76, PAIRS, 2, 2, 4, 1, 32, 4, 2, 0, 4)         /* 256 x 64, wave tile 64 x 64 */                                                                \
  /* deep LDS rings (NB = 4: four slabs in flight per workgroup, raw barriers): 64 KB, two per CU -- the rule's choice for launches of at           \
     most 512 tiles (plan_conv; profiles/r05_trunk_deep_ring.md); NB = 3 -> 48 KB, three per CU */                                                  \
  X(166, PAIRS, 1, 1, 2, 2, 64, 2, 4, 0, 2)        /* 66 (64 x 64, 128-byte rows) */                                                                \
  X(174, PAIRS, 2, 2, 2, 2, 32, 2, 4, 0, 2)        /* 74 (128 x 128, 64-byte rows) */                                                               \
  /* residual prefetch (RPF; fp16 pairs only): 74 at three / two workgroups per CU, 174 */                                                          \
  X(474, PAIR_F16, 2, 2, 2, 2, 32, 3, 2, 1, 3)                                                                                                      \
  X(475, PAIR_F16, 2, 2, 2, 2, 32, 2, 2, 1, 2)                                                                                                      \
  X(574, PAIR_F16, 2, 2, 2, 2, 32, 2, 4, 1, 2)                                                                                                      \
  /* the 128 x 128 tile of 174 on 8 / 16 waves (wave tile 64 x 32 / 32 x 32): more waves issue the slab's LDS-DMA requests and barriers in          \
     parallel */                                                                                                                                    \
  X(177, PAIRS, 2, 1, 2, 4, 32, 2, 4, 0, 2)                                                                                                         \
  X(179, PAIRS, 1, 1, 4, 4, 64, 1, 4, 0, 1)                                                                                                         \
  X(77, PAIRS, 2, 1, 2, 4, 32, 2, 2, 0, 2)         /* 177 with a two-buffer ring */                                                                 \
  X(183, PAIRS, 2, 2, 4, 4, 32, 1, 3, 0, 1)        /* 82 (256 x 256, 16 waves) with a three-buffer ring: 96 KB */                                   \
  /* (round 5, measured and removed -- profiles/r05_trunk_deep_ring.md (e): rings of six / eight buffers (96 / 128 KB): trunk 3.40 -> 3.9 /         \
     4.05 ms, and 3.43 / 3.47 when only launches of at most one tile per CU take them; a slab-level software pipeline of the four-buffer loop       \
     (next slab's fragments read and the next DMA issued in front of the slab's last eight MFMAs): -0.09 us per slab in a long K loop, but          \
     3.42 -> 3.45 ms)                                                                                                                               \
     (measured and removed, profiles/r05_trunk_deep_ring.md: 74 with three buffers for launches of 513 .. 4096 tiles: trunk 3.44 -> 3.57 ms; on     \
     the last neck layer's grouped GEMM 81 / 76 / 74 with three or four buffers: 0.66 / 0.67 / 0.74 / 0.62 ms against 0.57 of tile 82) */           \
  /* 128 x 256, 4 waves, wave tile 64 x 128: no gain over 81 / 82, so the fragment reads are not what limits the loop (TM = 4 variants: the         \
     compiler keeps the accumulators in scratch, 10x slower; removed) */                                                                            \
  X(85, PAIRS, 2, 4, 2, 2, 32, 2, 2, 0, 2)                                                                                                          \
  /* bf16 only */                                                                                                                                   \
  X(64, BF16, 1, 1, 4, 1, 64, 1, 2, 0, 4)                                                                                                           \
  X(71, BF16, 2, 2, 2, 2, 32, 1, 2, 0, 3)                                                                                                           \
  X(72, BF16, 2, 2, 4, 1, 32, 1, 2, 0, 3)                                                                                                           \
  X(91, E4M3, 2, 2, 2, 2, 64, 4, 2, 0, 4)          /* e4m3 operands, v_mfma_f32_32x32x16_fp8_fp8: 128 x 128, 64-byte rows */                        \
  X(92, E4M3, 2, 1, 2, 2, 64, 5, 2, 0, 5)          /*   128 x 64 */                                                                                 \
  X(93, E4M3, 1, 1, 2, 2, 64, 6, 2, 0, 6)          /*   64 x 64 */                                                                                  \
  X(94, E4M3, 2, 2, 2, 2, 128, 2, 2, 0, 2)         /*   128 x 128, 128-byte rows */

struct TileInfo { int bm, bn, bk, wg_per_cu; };

// The planner's figures of an LDS-DMA tile; false for a generic tile or a number in no row.
inline bool tile_info(int cfg, TileInfo *t) {
  switch (cfg) {
#define IVX_ROW(n, fam, TM, TN, WR, WC, BK, WPE, NB, RPF, WG) \
    case n: if (IVX_FAM_##fam == IVX_FAM_GENERIC) return false; *t = {WR * TM * 32, WC * TN * 32, BK, WG}; return true;
    IVX_CONV_TILES(IVX_ROW)
#undef IVX_ROW
    default: return false;
  }
}

// The operand families a number is instantiated for (0: in no row).
inline int tile_families(int cfg) {
  switch (cfg) {
#define IVX_ROW(n, fam, TM, TN, WR, WC, BK, WPE, NB, RPF, WG) case n: return IVX_FAM_##fam;
    IVX_CONV_TILES(IVX_ROW)
#undef IVX_ROW
    default: return 0;
  }
}

// The pair-only forms numbered past the bf16 range 61 .. 90: a ring deeper than two buffers, or the residual prefetch.
inline bool tile_deep_form(int cfg) {
  switch (cfg) {
#define IVX_ROW(n, fam, TM, TN, WR, WC, BK, WPE, NB, RPF, WG) case n: return NB > 2 || RPF != 0;
    IVX_CONV_TILES(IVX_ROW)
#undef IVX_ROW
    default: return false;
  }
}

// ------------------------------------------------------------------------------------------------
// Configs of the Winograd-domain GEMMs along z on fp16 pairs (ivx_conv_launch_halo, TU 5; the number is what ivx_conv_set_halo_mode forces).
// H(number, TM, TN, WR, WC, WPE, PAIR, NBUF, TAIL, SW, ZR, DI)   conv_wino_halo_kernel: TAIL 0 = overlapping tiles without the tail pass, SW = z
//                                                                stride, ZR = masked taps read a zero row, DI = de-interleaved staging
// Z(number, Z, WCOL, WN, WPE, SW)                                conv_wino_zblk_kernel, built for columns of Z output slices (SW Z input slices)
#define IVX_CONV_HALO_CFGS(H, Z)                                                                                                                    \
  H(1, 2, 2, 4, 1, 2, 2, 2, 1, 1, 0, 0)            /* 256 x 64, 4 waves, 2 buffers: 58 KB, two workgroups per CU */                                 \
  H(2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 0, 0)            /* 128 x 128, 4 waves, 2 buffers: 66 KB */                                                       \
  H(3, 2, 2, 4, 2, 1, 2, 2, 1, 1, 0, 0)            /* 256 x 128, 8 waves, 2 buffers: 82 KB */                                                       \
  H(4, 2, 1, 2, 2, 3, 2, 2, 1, 1, 0, 0)            /* 128 x 64, 4 waves, 2 buffers: 42 KB, three per CU */                                          \
  H(5, 2, 2, 4, 4, 1, 2, 2, 1, 1, 0, 0)            /* 256 x 256, 16 waves, 2 buffers: 130 KB */                                                     \
  H(6, 2, 2, 4, 2, 1, 2, 3, 1, 1, 0, 0)            /* 256 x 128, 8 waves, 3 buffers: 123 KB */                                                      \
  H(7, 2, 1, 2, 2, 2, 2, 3, 1, 1, 0, 0)            /* 128 x 64, 4 waves, 3 buffers: 63 KB, two per CU */                                            \
  H(8, 2, 2, 4, 1, 1, 2, 3, 1, 1, 0, 0)            /* 256 x 64, 4 waves, 3 buffers: 87 KB */                                                        \
  H(9, 2, 2, 2, 2, 1, 2, 3, 1, 1, 0, 0)            /* 128 x 128, 4 waves, 3 buffers: 99 KB */                                                       \
  H(10, 2, 1, 2, 2, 4, 2, 2, 0, 1, 0, 0)           /* 126 (of 128) x 64, overlapping tiles, 40 KB: four per CU */                                   \
  H(11, 2, 2, 4, 1, 2, 2, 2, 0, 1, 0, 0)           /* 254 x 64, overlapping tiles, 56 KB: two per CU */                                             \
  H(12, 2, 2, 4, 4, 1, 2, 2, 0, 1, 0, 0)           /* 254 x 256, 16 waves, overlapping tiles, 128 KB */                                             \
  H(13, 2, 2, 4, 2, 1, 2, 2, 0, 1, 0, 0)           /* 254 x 128, 8 waves, overlapping tiles, 80 KB: two per CU */                                   \
  H(14, 2, 2, 2, 2, 2, 2, 2, 0, 1, 0, 0)           /* 126 x 128, 4 waves, overlapping tiles, 64 KB: two per CU */                                   \
  /* z stride 2 (p.W == 2 * p.Wo): 2 BM staged rows */                                                                                              \
  H(21, 2, 1, 2, 2, 2, 2, 2, 0, 2, 0, 0)           /* 127 x 64, 4 waves: 56 KB, two per CU */                                                       \
  H(22, 2, 2, 2, 2, 2, 2, 2, 0, 2, 0, 0)           /* 127 x 128, 4 waves: 80 KB, two per CU */                                                      \
  H(23, 2, 2, 4, 2, 1, 2, 2, 0, 2, 0, 0)           /* 255 x 128, 8 waves: 112 KB, one per CU */                                                     \
  H(24, 1, 2, 4, 1, 2, 2, 2, 0, 2, 0, 0)           /* 127 x 64, 4 waves in M (wave tile 32 x 64): 56 KB */                                          \
  /* ZR: masked taps read a zero row (10 / 13 / 14 / 11 / 22 / 21 with the fragment address selected instead of the fragment zeroed) */            \
  H(30, 2, 1, 2, 2, 4, 2, 2, 0, 1, 1, 0)           /* 125 x 64 */                                                                                   \
  /* (round 5, with the raw barrier that makes a third buffer a real prefetch distance of two groups -- measured and removed, profiles/            \
     r05_fused_gemm_output.md: 125 x 64 with three / four buffers 0.535 / 0.600 ms against 0.493 (64 channels); 253 x 128 with three 0.806         \
     against 0.659 (128) and 1.314 against 1.171 (256): on these launches resident workgroups DO hide the latency better than depth) */            \
  H(31, 2, 2, 4, 1, 2, 2, 2, 0, 1, 1, 0)           /* 253 x 64 */                                                                                   \
  H(33, 2, 2, 4, 2, 1, 2, 2, 0, 1, 1, 0)           /* 253 x 128, 8 waves */                                                                         \
  H(34, 2, 2, 2, 2, 2, 2, 2, 0, 1, 1, 0)           /* 125 x 128 */                                                                                  \
  H(41, 2, 1, 2, 2, 2, 2, 2, 0, 2, 1, 0)           /* stride 2: 127 x 64 */                                                                         \
  H(42, 2, 2, 2, 2, 2, 2, 2, 0, 2, 1, 0)           /* stride 2: 127 x 128 */                                                                        \
  H(43, 2, 2, 2, 2, 2, 2, 2, 0, 2, 1, 1)           /* 42 with de-interleaved staging */                                                             \
  H(44, 2, 1, 2, 2, 2, 2, 2, 0, 2, 1, 1)           /* 41 with de-interleaved staging */                                                             \
  H(45, 2, 2, 2, 2, 2, 2, 2, 0, 2, 0, 1)           /* 22 with de-interleaved staging */                                                             \
  /* round 5 (A/B): the tile of 42 on twice the waves (wave tile 64 x 32 instead of 64 x 64) -- 0.520 / 0.807 ms against 0.519 / 0.802: unlike     \
     the trunk's one-wave-per-SIMD launches these kernels are not bound by what a single wave issues */                                             \
  H(46, 2, 1, 2, 4, 2, 2, 2, 0, 2, 1, 0)           /* stride 2: 127 x 128, 8 waves, 80 KB, two per CU */                                            \
  /* z-blocked tiles (Wo = 3 or 6 only): 50 / 51 = 8 / 16 waves at Z = 3, 60 at Z = 6.  Measured and not kept as instantiations                    \
     (profiles/r04_zblk_ab.md): 384 x 64 (8 waves) 1.04, 192 x 64 (4 waves) 1.07, 192 x 256 (16 waves) 1.05, 96 x 128 1.22 ms at Z = 3 (50:        \
     0.99); at Z = 6: 192 x 64 0.675, 192 x 256 1.08, 384 x 128 0.67 (60: 0.63-0.65); z stride 2: 6 -> 3 slices 64 columns 0.874, 12 -> 6 0.578    \
     (the halo form 42: 0.785 / 0.507) */                                                                                                           \
  Z(50, 3, 2, 4, 4, 1)                             /* 192 rows (64 columns) x 128: 72 KB, two per CU */                                             \
  Z(51, 3, 4, 4, 4, 1)                             /* 384 rows x 128, 16 waves: 96 KB, one per CU */                                                \
  Z(60, 6, 1, 4, 4, 1)                             /* 192 rows (32 columns) x 128 */                                                                \
  /* z stride 2 (p.W == 2 p.Wo), 6 -> 3 slices: 0.818 ms against 0.785 of the halo form 42 -- an A/B point, not the rule */                        \
  Z(71, 3, 1, 4, 2, 2)                             /* 32 columns x 128 (two waves per SIMD) */

// The z stride of the layers a halo number is for, by the numbering convention: 1 .. 20, 30 .. 39 and 50 .. 69 stride 1; 21 .. 29, 40 .. 49 and
// 70 on stride 2 (0 for no number).  It holds for numbers in no row as well: the grouped rule hands such a number to the launch of its own
// stride, which refuses it, and ignores it on the other.  Every row is checked against it below.
constexpr int halo_mode_stride(int mode) {
  return mode <= 0 ? 0 : ((mode >= 21 && mode < 30) || (mode >= 40 && mode < 50) || mode >= 70) ? 2 : 1;
}
#define IVX_H(n, TM, TN, WR, WC, WPE, PAIR, NBUF, TAIL, SW, ZR, DI) static_assert(halo_mode_stride(n) == SW, "halo row outside its stride's numbers");
#define IVX_Z(n, ZD, WCOL, WN, WPE, SW) static_assert(halo_mode_stride(n) == SW, "zblk row outside its stride's numbers");
IVX_CONV_HALO_CFGS(IVX_H, IVX_Z)
#undef IVX_H
#undef IVX_Z

#endif   // IVX_CONV_TILES_H_
