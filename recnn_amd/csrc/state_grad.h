// state_grad.h -- argument block of the input-gradient launch of the DDPG / TD3 step (state_grad.hip):
//   out[rows, S] (fp32) = sum over segments of scale_seg[rows] . (dz_seg[rows, K] * W_seg[K, S]),  segment 0 first, k ascending.
#pragma once
#include "common.h"

struct StateGradSeg {
  const void* dz; int64_t ld_dz;   // layer-1 pre-activation gradient, compute type, [rows, ld_dz] (k contiguous)
  const void* W; int64_t ld_w;     // the state columns of a layer-1 weight in the compute type: row k = hidden unit, [K, ld_w], already
                                   // offset to the first state column; 16-byte aligned rows whose padding reaches roundup(S, one chunk)
  const float* scale;              // optional fp32 [rows] seed: this segment's part of out row m is multiplied by scale[m] (unit backward
                                   // tensors), in fp32 on the accumulator.  With two segments any seed makes the launch fold per segment.
};

struct StateGradArgs {
  int rows, S, K, nseg;            // K % 8 == 0 (a multiple of one 16-byte chunk in either compute type); S, rows arbitrary
  StateGradSeg seg[2];
  float* out; int64_t ld_out;      // fp32, caller owned; columns [S, ld_out) are not touched
};

// dtype: RECNN_F32 (v_mfma_f32_16x16x4_f32) | RECNN_BF16 (v_mfma_f32_16x16x32_bf16, fp32 accumulation)
int state_grad_launch(const StateGradArgs& a, int dtype, hipStream_t s);
