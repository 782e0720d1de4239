// dwadam.h -- the critics' weight-gradient GEMMs with the optimizer in their epilogue (dwadam.hip).
#pragma once
#include "optim.h"

// One weight tensor of a network: dW[M, N] = dZ[rows, M]^T X[rows, N], M = N.L.t[tensor].rows (a multiple of 32), N = .cols
struct DwAdamProb {
  const void* dz;        // bf16 [rows, ldz]: backward tensor, ALREADY times the per-row loss seed (mlpt.hip)
  const void* x;         // bf16 [rows, ldx]: the layer's input, columns in SHADOW order (critic W1: [action | state]), zero padded to 64
  int64_t ldz, ldx;
  int tensor;            // index into NetLayout.t
  int tiles_m, tiles_n;  // 32 x 64 output tiles
  int nslab;             // 8 | 16: batch slices summed exactly like the slabs of the two-launch path (NetLayout.t[tensor].nslab)
};
struct DwAdamNet {
  NetLayout L;
  ApplyArgs a;           // finished by dwadam_launch (apply_args_finish)
  DwAdamProb w[2];       // launch order: the small contraction (W2) first
  int rows;
  int x3;                // split-bf16 operands and shadows (filled by dwadam_launch from a.tc_bf16)
  int nsmall;            // optimizer workgroups of the tensors that are NOT weight tiles (biases, the last layer)
  int ntile[2];
};
constexpr int DWADAM_MAX_NETS = 2;
struct DwAdamBatch {
  DwAdamNet n[DWADAM_MAX_NETS];
};

int dwadam_init();
// whether tensor `ti` of layout L can be a tile problem of this kernel at `rows` batch rows
bool dwadam_tensor_ok(const NetLayout& L, int ti, int rows, int x3 = 0);
int dwadam_launch(DwAdamBatch& b, int nnet, hipStream_t s);

// ---- the gradient-only form (dw_grad_kernel): ONE network's three weight matrices, the same tiles and slab order, the summed tile
// straight into the flat gradient arena; the biases' panel sums reduced as grad_reduce_kernel does.  For a network whose optimizer
// cannot ride in the epilogue: the actor's clip quirk needs the whole gradient's L1 norm first.
constexpr int DWGRAD_MAX_W = 3;
struct DwGradNet {
  NetLayout L;
  ApplyArgs a;           // filled by dwgrad_launch: only g_out is read
  DwAdamProb w[DWGRAD_MAX_W];   // launch order (tensors W1 / W2 / W3 of the layout, each once)
  int rows;
  int nsmall;
  int ntile[DWGRAD_MAX_W];
};
// whether the layout's three matrices fit the tile plan at `rows` rows and its three biases are panel-summed small tensors
bool dwgrad_ok(const NetLayout& L, int rows);
int dwgrad_launch(DwGradNet& n, float* gflat, hipStream_t s);
