// fc_adjoint_loop_batch.hip.h -- the controllers of k lock-step closed loops inside the batched backward march
// (fc_run_adjoint_closed_loop_batch; host side in fc_adjoint_loop_batch_run.hpp; DESIGN §5.4 "Batched closed loops").  Column s of the
// batch carries ITS controller: the arithmetic of fc_adjoint_loop.hip.h (fc_ctrl_adj_step_body, fc_ctrl_adj_grad_entry) on block s of the
// bank, row s of the tape, the signals and the limits.  The columns never mix and every sum is formed by one lane in index order: equal
// columns come out bit-equal, two marches are bit-identical.
//
// Layouts (simulation index in the middle, like the rest of the batch API):
//     loop tape   [capacity][k][nx + n_sens + n_act]     written by fc_ctrl_step (FcCtrlIO::tape_stride = the row length)
//     bank copy   [k][FcCtrlBank::stride]                every block untransposed (row-major), offsets as FcCtrlBank's
//     adjoint rows [n + 1][k][FcLoopRow::stride]
//     g, r, w_u   [n][k][n_act]      w, dy0 [.][k][n_sens]      w_y [rows][k][nyc]      limits [k][n_act]
#pragma once

#include "fc_adjoint_loop.hip.h"

// Backward step m of all k controllers: grid k, ONE wave per column.  io holds the pointers of COLUMN 0 (null where the single kernel
// takes null); column s finds its own one row of its kind further on.  g_out [k][n_act] holds B~_a^T mu_s, left there by fc_adj_reduce_b
// (partial == null, the default).  With `partial` non-null (FC_ADJ_LOOP_FUSE=1) the wave forms it first from the tail's workgroup
// partials exactly as fc_adj_reduce_b does -- lane l takes partials l, l + 64, .. in order, then the fixed shuffle tree -- for
// a = 0 .. n_act - 1, stores it to the g row and hands it to the body through LDS: the same bits without the launch, but measured
// slower.  All stores are ordinary vector stores.
__global__ __launch_bounds__(64) void fc_ctrl_adj_step_b(FcCtrlBank bk, FcCtrlAdjIO io, double* __restrict__ g_out, const double* __restrict__ partial, int gx,
                                                         int KB) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const int nx = bk.nx, nyc = bk.nyc, ns = bk.n_sens, na = bk.n_act;
  const long long LR = fc_loop_row(nx, nyc, bk.nuc, na).stride, TR = (long long)nx + ns + na;
  __shared__ double gs[FC_CTRL_NUC_MAX];
  FcCtrlAdjIO c = io;
  c.matn = io.matn + (long long)s * bk.stride;
  c.tape = io.tape + (long long)s * TR;
  c.g = g_out + (long long)s * na;
  if (io.r) c.r = io.r + (long long)s * na;
  if (io.w_y) c.w_y = io.w_y + (long long)s * nyc;
  if (io.u_lo) c.u_lo = io.u_lo + (long long)s * na, c.u_hi = io.u_hi + (long long)s * na;
  c.row = io.row + (long long)s * LR;
  c.row_prev = io.row_prev + (long long)s * LR;
  if (io.w_prev) c.w_prev = io.w_prev + (long long)s * ns;
  if (io.dy0) c.dy0 = io.dy0 + (long long)s * ns;
  if (partial) {
    for (int a = 0; a < na; ++a) {
      const double* __restrict__ p = partial + ((size_t)a * KB + s) * gx;
      double sum = 0.0;
      for (int q = lane; q < gx; q += 64) sum += p[q];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
      if (lane == 0) {
        gs[a] = sum;
        g_out[(long long)s * na + a] = sum;
      }
    }
    __syncthreads();
    c.g = gs;
  }
  fc_ctrl_adj_step_body(bk, bk.mat + (long long)s * bk.stride, c);
}

// The seven parameter gradients of every column behind the march: out [k][FcCtrlBank::stride], one thread per (column, entry), summed
// in ascending m (fc_ctrl_adj_grad_entry): the result does not depend on the launch geometry.
__global__ __launch_bounds__(256) void fc_ctrl_adj_grads_b(FcCtrlBank bk, int k, int n, const double* __restrict__ tape, const double* __restrict__ rows,
                                                           double* __restrict__ out) {
  const FcLoopRow L = fc_loop_row(bk.nx, bk.nyc, bk.nuc, bk.n_act);
  const long long LR = L.stride, TR = (long long)bk.nx + bk.n_sens + bk.n_act, total = (long long)k * bk.stride;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long s = i / bk.stride, e = i % bk.stride;
    out[i] = fc_ctrl_adj_grad_entry(bk, L, e, n, tape + s * TR, rows + ((long long)k + s) * LR, (long long)k * TR, (long long)k * LR);
  }
}
