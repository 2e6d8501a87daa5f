// The one launch of vsd_plan_set_options (csrc/plan_options.hip), called from csrc/plan.hip.
#pragma once
#include "common.h"

constexpr int PLAN_OPT_ROWS = 50;    // timesteps an LCM schedule can hold (19, 39, ... 999): rows of every table of a plan file
constexpr int PLAN_OPT_TABLES = 3;   // time tables of a program at most: UNet, ControlNet, the reference-only WRITE pass
constexpr int PLAN_OPT_COEF = 6;     // per timestep: sqrt(a_t), sqrt(1 - a_t), c_skip, c_out, the two add-noise values

struct PlanOptTable {
  const uint32_t* src;  // the 50-row table of the file, rows of row_words
  uint32_t* dst;        // the table the captured graph reads: n rows, dst_stride_words apart
  uint32_t row_words, dst_stride_words;
};

struct PlanOptArgs {
  int n, nres, ntab;
  float scale;                       // (float)controlnet_scale
  unsigned char row[PLAN_OPT_ROWS];  // step -> table row
  const float* coef;                 // [50][6], then logspace(-1, 0, nres)
  float* consts;                     // the live block: [0:2] add-noise, [2 + 6 i : 8 + 6 i] step i, then nres residual scales
  PlanOptTable tab[PLAN_OPT_TABLES];
};

int plan_options_launch(vsd_ctx* ctx, hipStream_t stream, const PlanOptArgs& a);
