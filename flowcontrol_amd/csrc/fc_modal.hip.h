// fc_modal.hip.h -- the snapshot bank of the time-stepping handle (fc_state_snap_*): state history on the device, POD / DMD from it.
//   fc_ssnap_capture: the state of a step (permuted numbering) into a column of the bank (W layout, original numbering)
//   fc_ssnap_mean, fc_ssnap_combine: column mean (optionally subtracted in place), linear combinations of columns; one thread per row,
//                     columns in a fixed order, no atomics
//   fc_ssnap_gram:    tall-skinny product L^T W of real columns on the fp64 matrix cores: the real-operand counterpart of fc_snap_gram
//                     (fc_shifted.hip.h), whose LDS layout, chunking and two-sum it keeps; slice partials are added by fc_snap_gram_reduce
// A set is [col][n] doubles.  Everything here writes with vector stores.
#pragma once

// dst[j] = src[iperm[j]]: reads gathered from the 450 KB state that the step just wrote (cache-resident), writes coalesced.  NT: the
// column is not read again before the run ends -- nontemporal stores keep it from displacing the factors in the Infinity Cache.
template <bool NT>
__global__ __launch_bounds__(256) void fc_ssnap_capture(int n, const int* __restrict__ iperm, const double* __restrict__ src,
                                                        double* __restrict__ dst) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const double v = src[iperm[j]];
  if (NT)
    __builtin_nontemporal_store(v, &dst[j]);
  else
    dst[j] = v;
}

// mean[row] = (sum of columns [0, m) of X in column order) / m; subtract: X[c][row] -= mean[row]
__global__ __launch_bounds__(256) void fc_ssnap_mean(int n, int m, double* __restrict__ X, double* __restrict__ mean, int subtract) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  double s = 0.0;
  for (int c = 0; c < m; ++c) s += X[(size_t)c * n + row];
  s /= (double)m;
  mean[row] = s;
  if (subtract)
    for (int c = 0; c < m; ++c) X[(size_t)c * n + row] -= s;
}

// out[c][row] = sum_j Q[j][c] X[j][row], j = 0 .. m - 1 in order (Q: m x k, row-major); grid (rows / 256, k).  out may be columns of
// the set X lives in, behind the m it reads.
__global__ __launch_bounds__(256) void fc_ssnap_combine(int n, int m, int k, const double* X, const double* __restrict__ Q, double* out) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  const int c = blockIdx.y;
  if (row >= n || c >= k) return;
  double s = 0.0;
  for (int j = 0; j < m; ++j) s += Q[(size_t)j * k + c] * X[(size_t)j * n + row];
  out[(size_t)c * n + row] = s;
}

// part[blockIdx.z][i][j0 + j] = sum over the slice's rows r of L[r][i] W[r][j] for real columns L (ncl of them), W (ncr of them), both
// [col][n].  One workgroup = a 64 x 64 tile of the output (blockIdx.x: 64 columns of L, blockIdx.y: 64 of W) over the rows
// [blockIdx.z * slice, + slice) of n; wave w owns the 32 x 32 quarter (w & 1, w >> 1) as 2 x 2 accumulators of
// v_mfma_f64_16x16x4_f64, exactly as in fc_snap_gram.  Operand tiles go through LDS in chunks of 32 rows: 8-byte global reads along the
// columns (32 consecutive doubles per column and half-wave), LDS [column][row] with the row stride of 36 doubles.  Columns past ncl / ncr
// and rows past the slice or n read as zero.  ld: leading dimension of the output, j0: first output column of this launch.
__global__ __launch_bounds__(256) void fc_ssnap_gram(int n, int slice, int ncl, int ncr, const double* __restrict__ L,
                                                     const double* __restrict__ W, int ld, int j0, double* __restrict__ part) {
  __shared__ double Ls[64][kSnapLD], Ws[64][kSnapLD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int wi = 32 * (wave & 1), wj = 32 * (wave >> 1);
  const int a0 = 64 * blockIdx.x, b0 = 64 * blockIdx.y;
  const int r0 = blockIdx.z * slice, r1 = min(n, r0 + slice);
  const int tr = threadIdx.x & 31, tc = threadIdx.x >> 5;  // staging: row of the chunk, column (+ 8 per pass)
  fc_d4 acc[2][2], hi[2][2], lo[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) hi[x][y] = lo[x][y] = fc_d4{0.0, 0.0, 0.0, 0.0};
  for (int rc = r0; rc < r1; rc += kSnapKC) {
    const int row = rc + tr;
    double lv[8], wv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int c = tc + 8 * u;
      lv[u] = (row < r1 && a0 + c < ncl) ? L[(size_t)(a0 + c) * n + row] : 0.0;
      wv[u] = (row < r1 && b0 + c < ncr) ? W[(size_t)(b0 + c) * n + row] : 0.0;
    }
    __syncthreads();  // (the previous chunk's reads are done)
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int c = tc + 8 * u;
      Ls[c][tr] = lv[u];
      Ws[c][tr] = wv[u];
    }
    __syncthreads();
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y) acc[x][y] = fc_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < kSnapKC / 4; ++s) {
      const double av0 = Ls[wi + lr][4 * s + lk], av1 = Ls[wi + 16 + lr][4 * s + lk];
      const double bv0 = Ws[wj + lr][4 * s + lk], bv1 = Ws[wj + 16 + lr][4 * s + lk];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av0, bv0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av0, bv1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av1, bv0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av1, bv1, acc[1][1], 0, 0, 0);
    }
    // only the 32-term sums inside the matrix instructions round: the chunks join the running sum by two-sum
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y) fc_two_sum(hi[x][y], lo[x][y], acc[x][y]);
  }
  double* __restrict__ P = part + (size_t)blockIdx.z * (size_t)ncl * ld;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = a0 + wi + 16 * x + lk + 4 * r, j = b0 + wj + 16 * y + lr;
        if (i < ncl && j < ncr) P[(size_t)i * ld + j0 + j] = hi[x][y][r] + lo[x][y][r];
      }
}
