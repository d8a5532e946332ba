// The host side that chooses what the convolution launchers run (conv_plan.cpp; plain C++, no device code): the lab knobs and environment
// switches in one record each, and the rules -- which tile, which K split, which workspace, which batch slices for the direct path; which
// z-halo / z-blocked config or which tile for the grouped launches of winograd.hip.  conv_igemm.hip launches what these answer, and
// ivx_conv_plan_query (include/imvoxel_lab.h) reports it; tests/golden/conv_plans.json holds the answers.
#ifndef IVX_CONV_PLAN_H_
#define IVX_CONV_PLAN_H_
#include "conv_shared.h"
#include "conv_tiles.h"

// The four lab settings (include/imvoxel_lab.h: ivx_conv_set_tile_override / _halo_mode / _plan_mode / _epilogue_mode), per calling thread.
struct ConvLab {
  int tile_override = 0;     // 0 = automatic choice, else force a tile of conv_tiles.h
  int halo_mode = -1;        // -1 default rule | 0 never | a number of IVX_CONV_HALO_CFGS: force that config on the layers of its z stride
  int plan_mode = 0;         // 1 = the round-1 tile rule of plan_conv, 0 = the scored choice
  int narrow_epilogue = 0;   // 1 = one-channel-per-lane epilogue stores in the LDS-DMA kernel
};
ConvLab &conv_lab();

// The environment switches of the conv files (A/B only; the defaults are the measured rules; DESIGN.md 5 lists them): X(field, name, default).
// Read once per process, all by conv_env().
#define IVX_CONV_ENV(X)                                                                                                                     \
  X(skinny, "IVX_CONV_SKINNY", 1)                  /* 0: no K split for the Cout <= 32 head convs (the round-5 rule) */                     \
  X(pio_rule, "IVX_PIO_RULE", 1)                   /* 0: chained fp16 pairs take the bf16 tile rule */                                      \
  X(pio_splitk, "IVX_PIO_SPLITK", 1)               /* 0: no split K for pair IO */                                                          \
  X(pio_split_tiles, "IVX_PIO_SPLIT_TILES", 320)   /* pair IO splits K up to this many tiles */                                             \
  X(pio_deep, "IVX_PIO_DEEP", 4)                   /* other than 4: no deep LDS ring for the trunk's small launches */                      \
  X(pio_deep_tiles, "IVX_PIO_DEEP_TILES", 512)     /* ... which are launches of at most this many tiles */                                  \
  X(pio_deep_slabs, "IVX_PIO_DEEP_SLABS", 6)       /* ... and at least this many K slabs */                                                 \
  X(pio_w16_tiles, "IVX_PIO_W16_TILES", 256)       /* the deep 128 x 128 tile runs on 16 waves up to this many tiles */                     \
  X(pio_w8_tiles, "IVX_PIO_W8_TILES", 512)         /* ... on 8 waves up to this many */                                                     \
  X(pio_t183, "IVX_PIO_T183", 1)                   /* 0: no 256 x 256 tile in the trunk */                                                  \
  X(pio_tail, "IVX_PIO_TAIL", 0)                   /* 1: grid-tail plan for pair IO back on */                                              \
  X(pio_stagger_us, "IVX_PIO_STAGGER_US", 0)       /* phase stagger experiment of run_conv: delay in us, 0 = off */                         \
  X(pio_stagger_shift, "IVX_PIO_STAGGER_SHIFT", 0) /* ... which bit of the XCD-local workgroup index picks the late half */                 \
  X(halo_small, "IVX_HALO_SMALL", 1)               /* 0: the 253 x 128 z-halo tile also on small volumes */
struct ConvEnv {
#define IVX_FIELD(field, name, def) long long field;
  IVX_CONV_ENV(IVX_FIELD)
#undef IVX_FIELD
};
const ConvEnv &conv_env();

bool dma_applicable(const ConvParams &p);
ConvPlan plan_conv(const ConvParams &p, bool allow_ws);
int conv_batch_slice(const ConvParams &p);
ConvParams conv_slice_params(const ConvParams &p, int b0, int nb);
int grouped_halo_cfg(const ConvParams &p, const ivx_conv_desc *d, int groups);
ConvPlan grouped_tile_plan(const ConvParams &p, int groups);

#endif   // IVX_CONV_PLAN_H_
