// What the in-situ analysis units (lattice, grain, texture, curvature, fatigue) share on the device and around their launches.  Every analysis
// promises the same bits on every call; that promise is the ORDER of each operation below, so it is stated here once:
//   wave tree       __shfl_down by 32, 16, 8, 4, 2, 1, x = op(x, value of lane + d), result in lane 0
//   row staging     64 rows through LDS per 64-lane block, flat index i = 64 j + lane over (row, column), all loads before the first LDS write,
//                   rows past nv of a last, partial block repeat row nv - 1
//   tile write-out  64 x K doubles leave an LDS tile as one contiguous run, flat index 64 j + lane
//   summary         launch 1 (256 threads, grid = summary_grid): every lane folds its own elements in ascending order -> wave tree -> lane 0 of
//                   every wave to LDS -> thread 0 merges the block's waves in wave order -> one value vector per block in ctx->scratch_dev;
//                   launch 2 (one wave): lane l merges blocks l, l + 64, ... in ascending order -> wave tree -> lane 0 writes the result.
//                   No atomics; the grid depends on E and the cap alone, so the cap is part of the summation order.
// The helpers are force-inlined and hold no barrier of a staging scheme: the __syncthreads between staging, use and write-out stay in the kernels.
#pragma once
#include "exa_internal.hpp"

namespace exa_analysis {

constexpr double RAD2DEG = 57.295779513082320876798154814105;

// ---- wave tree ---------------------------------------------------------------------------------------------------------------------------

template <class Op>
__device__ __forceinline__ double wave_reduce(double x, Op op) {
#pragma unroll
   for (int d = 32; d > 0; d >>= 1) x = op(x, __shfl_down(x, d));
   return x;   // lane 0
}
__device__ __forceinline__ double wave_sum(double x) { return wave_reduce(x, [](double a, double b) { return a + b; }); }

// ---- one 64-lane block over 64 rows -----------------------------------------------------------------------------------------------------------

// block b of a launch of 64-lane blocks over n rows: first row, valid rows (< 64 in a last, partial block), lane
struct BlockView {
   int64_t base; int nv, lane;
   __device__ __forceinline__ explicit BlockView(const int64_t n) : base((int64_t)blockIdx.x * 64), lane(threadIdx.x) { nv = (int)(n - base < 64 ? n - base : 64); }
};

// NC columns of the block's rows -> LDS tile of row stride LD (NC: dense; NC + 1: odd stride, lane = row reads hit distinct banks).  Tile row
// r < nv, column c is src[row_off(r) + col(c)]: row_off gives the offset of the source row (through a gathered order or not), col the source
// column.  (An offset, not a pointer per row: a pointer per row moved the listings of kernels that the offset leaves identical.)  The caller
// places the barrier.
template <int NC, int LD, class RowOff, class Col>
__device__ __forceinline__ void stage_rows(double* sm, const int nv, const int lane, const double* src, RowOff row_off, Col col) {
   double st[NC];
#pragma unroll
   for (int j = 0; j < NC; j++) {
      const int i = j * 64 + lane, r = i / NC, c = i - r * NC;
      const int rr = r < nv ? r : nv - 1;
      st[j] = src[row_off(rr) + col(c)];
   }
   if constexpr (LD == NC) {
#pragma unroll
      for (int j = 0; j < NC; j++) sm[j * 64 + lane] = st[j];
   } else {
#pragma unroll
      for (int j = 0; j < NC; j++) {
         const int i = j * 64 + lane, r = i / NC, c = i - r * NC;
         sm[r * LD + c] = st[j];
      }
   }
}
struct IdentityCol { __device__ __forceinline__ constexpr int operator()(int c) const { return c; } };

// rows 0 .. nv-1 of an LDS tile [64][K] of row stride LD -> rows base .. base + nv - 1 of out[][K], one contiguous run
template <int K, int LD>
__device__ __forceinline__ void store_tile(double* out, const int64_t base, const double* sm, const int nv, const int lane) {
#pragma unroll
   for (int j = 0; j < K; j++) {
      const int i = j * 64 + lane;
      if constexpr (LD == K) { if (i < nv * K) out[base * K + i] = sm[i]; }
      else { const int r = i / K, k = i - r * K; if (r < nv) out[base * K + i] = sm[r * LD + k]; }
   }
}

// ---- the two-launch summary -----------------------------------------------------------------------------------------------------------------
// Policy: N values, init(v) their neutral elements, merge(v, y) folds the value vector y into v (whole vectors: a pair such as "largest value,
// smallest id on a tie" is not componentwise).  merge must be associative for the result to be a function of the data alone.

template <class Policy>
__device__ __forceinline__ void wave_merge(double (&v)[Policy::N]) {
#pragma unroll
   for (int d = 32; d > 0; d >>= 1) {
      double y[Policy::N];
#pragma unroll
      for (int k = 0; k < Policy::N; k++) y[k] = __shfl_down(v[k], d);
      Policy::merge(v, y);
   }
}

// v: this lane's values; sm: one vector per wave of the block; holds the block's barrier
template <class Policy, int WAVES>
__device__ __forceinline__ void summary_block_partial(double (&v)[Policy::N], double (&sm)[WAVES][Policy::N], double* partial) {
   constexpr int N = Policy::N;
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   wave_merge<Policy>(v);
   if (lane == 0) {
#pragma unroll
      for (int k = 0; k < N; k++) sm[wave][k] = v[k];
   }
   __syncthreads();
   if (threadIdx.x == 0) {
      double t[N];
#pragma unroll
      for (int k = 0; k < N; k++) t[k] = sm[0][k];
#pragma unroll
      for (int w = 1; w < WAVES; w++) Policy::merge(t, sm[w]);
#pragma unroll
      for (int k = 0; k < N; k++) partial[(int64_t)blockIdx.x * N + k] = t[k];
   }
}

// one wave over the nb partials of launch 1
template <class Policy>
__device__ __forceinline__ void summary_reduce(const int nb, const double* partial, double* out) {
   constexpr int N = Policy::N;
   const int lane = threadIdx.x;
   double v[N];
   Policy::init(v);
   for (int b = lane; b < nb; b += 64) Policy::merge(v, partial + (int64_t)b * N);
   wave_merge<Policy>(v);
   if (lane == 0) {
#pragma unroll
      for (int k = 0; k < N; k++) out[k] = v[k];
   }
}

// grid of launch 1: one block per `threads` elements up to max_blocks (the cap decides the summation order: it is the entry point's own and
// does not change), checked against the nvals doubles per block of ctx->scratch_dev
inline int summary_grid(exa_ctx* ctx, const char* who, const int threads, const int max_blocks, const int nvals, int* nb) {
   const int64_t need = ((int64_t)ctx->E + threads - 1) / threads;
   *nb = (int)(need < max_blocks ? need : max_blocks);
   if (sizeof(double) * (size_t)*nb * nvals > ctx->scratch_bytes) { ctx->err = std::string(who) + ": reduction scratch too small"; return EXA_ERR_UNSUPPORTED; }
   return EXA_OK;
}

// ---- signed permutations of a cubic orbit ---------------------------------------------------------------------------------------------------
// The axes of a family are signed permutations of its first axis, so they travel by value as 16-bit codes: component i of the image of b under
// code c = ((c >> (6 + i)) & 1 ? -1 : 1) * b[(c >> 2 i) & 3].  A sign flip and a permutation are exact: the decoded axes are the host's doubles.

__host__ __device__ __forceinline__ void perm_apply(const double* b, const int c, double& p0, double& p1, double& p2) {
   p0 = ((c >> 6) & 1) ? -b[c & 3] : b[c & 3];
   p1 = ((c >> 7) & 1) ? -b[(c >> 2) & 3] : b[(c >> 2) & 3];
   p2 = ((c >> 8) & 1) ? -b[(c >> 4) & 3] : b[(c >> 4) & 3];
}

// the code taking v to c, or -1
inline int perm_code(const double* v, const double* c) {
   static const int P[6][3] = { { 0, 1, 2 }, { 0, 2, 1 }, { 1, 0, 2 }, { 1, 2, 0 }, { 2, 0, 1 }, { 2, 1, 0 } };
   for (int p = 0; p < 6; p++) {
      int cd = P[p][0] | (P[p][1] << 2) | (P[p][2] << 4);
      bool ok = true;
      for (int i = 0; i < 3 && ok; i++) {
         const double x = v[P[p][i]];
         if (c[i] == x) continue;
         if (c[i] == -x) { cd |= 1 << (6 + i); continue; }
         ok = false;
      }
      if (ok) return cd;
   }
   return -1;
}

// the 24 proper rotations of the cubic group as codes: the signed permutations of determinant +1 (= parity x product of the signs), even
// permutations first, the signs counting up within a permutation.  Row i of the rotation has its entry s_i in column P[p][i].
inline void cubic_proper_rotations(uint16_t out[24]) {
   static const int P[6][3] = { { 0, 1, 2 }, { 1, 2, 0 }, { 2, 0, 1 }, { 0, 2, 1 }, { 2, 1, 0 }, { 1, 0, 2 } };
   int n = 0;
   for (int p = 0; p < 6; p++)
      for (int sg = 0; sg < 8; sg++) {
         const int par = p < 3 ? 1 : -1, sgn = ((sg & 1) ? -1 : 1) * ((sg & 2) ? -1 : 1) * ((sg & 4) ? -1 : 1);
         if (par * sgn == 1) out[n++] = (uint16_t)(P[p][0] | (P[p][1] << 2) | (P[p][2] << 4) | (sg << 6));
      }
}

}  // namespace exa_analysis
