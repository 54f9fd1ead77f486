// Kernels of the restarted GMRES solver (gfx950, FP64; host/krylov.hip): the two bandwidth kernels of classical Gram-Schmidt - a
// multi-dot h = V^T W w and a multi-axpy w -= V h - two gated pointwise passes, and the one-block scalar kernel that turns partial sums into a column
// of H, the rotations, the residual and the decisions.  Every scalar lives in the device record of gmres_slots.hpp; every kernel leaves at once
// when its FLAG is set.  No atomics: a block stores its sums into a table and the scalar kernel adds them in a fixed order, so a solve gives the
// same bits in every run.  Vectors are read in pairs (16-byte loads): their base addresses and the stride of the basis are multiples of 16 bytes.
#include "host/device_utils.hpp"
#include "gmres_slots.hpp"
#include "gmres_small.hpp"

namespace {

constexpr int GBLK = 256, GWAVES = GBLK / 64;
// basis vectors a thread accumulates against per pass over w (w is read once per chunk).  16: 32 accumulator + 64 load registers, no scratch
#ifndef EXA_GMRES_CHUNK
#define EXA_GMRES_CHUNK 16
#endif
constexpr int CH = EXA_GMRES_CHUNK;
static_assert(CH >= 8 && CH <= 16, "chunk of the multi-dot");

__device__ __forceinline__ int64_t node_of(const int64_t i, const int64_t nn) { return i - (i >= 2 * nn ? 2 * nn : (i >= nn ? nn : 0)); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
   for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s);
   return v;   // lane 0 holds the sum
}

// FLAG (and REORTH where asked) through one thread and LDS: the scalar kernel writes both, and a block must not split at a barrier
__device__ __forceinline__ bool gate_closed(const double* S, int gate, int* sm_gate) {
   if (gate == 2) return false;
   if (threadIdx.x == 0) *sm_gate = (S[gmres::FLAG] != 0.0 || (gate == 1 && S[gmres::REORTH] == 0.0)) ? 1 : 0;
   __syncthreads();
   return *sm_gate != 0;
}

template <bool FULL>
__device__ __forceinline__ void dot_chunk(const int64_t np, const int64_t n, const int64_t nn, const double* __restrict__ wgt, const double* __restrict__ Vc, const int64_t stride,
                                          const int nc, const double* __restrict__ w, const bool norm, double (&acc)[CH], double& accn) {
   const int64_t tid = (int64_t)blockIdx.x * GBLK + threadIdx.x, nth = (int64_t)gridDim.x * GBLK;
   for (int64_t q = tid; q < np; q += nth) {
      const double2 wv = reinterpret_cast<const double2*>(w)[q];
      const double a0 = wgt[node_of(2 * q, nn)] * wv.x, a1 = wgt[node_of(2 * q + 1, nn)] * wv.y;
      if (norm) accn += a0 * wv.x + a1 * wv.y;
#pragma unroll
      for (int c = 0; c < CH; c++)
         if (FULL || c < nc) {
            const double2 v = reinterpret_cast<const double2*>(Vc + (int64_t)c * stride)[q];
            acc[c] += a0 * v.x + a1 * v.y;
         }
   }
   if ((n & 1) && tid == 0) {   // the odd last entry
      const double wl = w[n - 1], a0 = wgt[node_of(n - 1, nn)] * wl;
      if (norm) accn += a0 * wl;
#pragma unroll
      for (int c = 0; c < CH; c++) if (FULL || c < nc) acc[c] += a0 * Vc[(int64_t)c * stride + n - 1];
   }
}

// table[(c) nb + block] = this block's part of (v_j0+c, w)_W for c < k; with_norm: table[k nb + block] = its part of (w, w)_W
__global__ void __launch_bounds__(GBLK) k_gm_multidot(int64_t n, int64_t nn, const double* __restrict__ wgt, const double* __restrict__ V, int64_t stride, int j0, int k,
                                                      const double* __restrict__ w, int with_norm, const double* __restrict__ S, int gate, double* __restrict__ table) {
   __shared__ double sm[GWAVES * (CH + 1)];
   __shared__ int sm_gate;
   if (gate_closed(S, gate, &sm_gate)) return;
   const int64_t np = n >> 1;
   const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nb = gridDim.x;
   for (int c0 = 0; c0 < k || (c0 == 0 && with_norm); c0 += CH) {
      const int nc = k - c0 < CH ? k - c0 : CH;
      const bool norm = with_norm && c0 == 0;
      double acc[CH], accn = 0.0;
#pragma unroll
      for (int c = 0; c < CH; c++) acc[c] = 0.0;
      const double* Vc = V + (int64_t)(j0 + c0) * stride;
      if (nc == CH) dot_chunk<true>(np, n, nn, wgt, Vc, stride, nc, w, norm, acc, accn);
      else dot_chunk<false>(np, n, nn, wgt, Vc, stride, nc, w, norm, acc, accn);
#pragma unroll
      for (int c = 0; c < CH; c++) { const double v = wave_sum(acc[c]); if (lane == 0) sm[wave * (CH + 1) + c] = v; }
      { const double v = wave_sum(accn); if (lane == 0) sm[wave * (CH + 1) + CH] = v; }
      __syncthreads();
      if ((int)threadIdx.x <= CH) {
         const int c = threadIdx.x;
         double v = sm[c];
#pragma unroll
         for (int wv = 1; wv < GWAVES; wv++) v += sm[wv * (CH + 1) + c];
         if (c < nc) table[(int64_t)(c0 + c) * nb + blockIdx.x] = v;
         else if (c == CH && norm) table[(int64_t)k * nb + blockIdx.x] = v;
      }
      __syncthreads();
   }
}

// w += sign sum_j S[coef + j] v_j0+j; table (may be null): this block's part of (w, w)_W of what it wrote
__global__ void __launch_bounds__(GBLK) k_gm_multiaxpy(int64_t n, int64_t nn, const double* __restrict__ wgt, const double* __restrict__ V, int64_t stride, int j0, int k,
                                                       const double* __restrict__ S, int coef, double sign, double* __restrict__ w, int gate, double* __restrict__ table) {
   __shared__ double cf[gmres::PAD];
   __shared__ double sm[GWAVES];
   __shared__ int sm_gate;
   if (gate_closed(S, gate, &sm_gate)) return;
   for (int j = threadIdx.x; j < k; j += GBLK) cf[j] = sign * S[coef + j];
   __syncthreads();
   const int64_t np = n >> 1, tid = (int64_t)blockIdx.x * GBLK + threadIdx.x, nth = (int64_t)gridDim.x * GBLK;
   const double* V0 = V + (int64_t)j0 * stride;
   double acc = 0.0;
   for (int64_t q = tid; q < np; q += nth) {
      double2 x = reinterpret_cast<double2*>(w)[q];
#pragma unroll 8
      for (int j = 0; j < k; j++) {
         const double2 v = reinterpret_cast<const double2*>(V0 + (int64_t)j * stride)[q];
         x.x += cf[j] * v.x; x.y += cf[j] * v.y;
      }
      reinterpret_cast<double2*>(w)[q] = x;
      if (table) acc += wgt[node_of(2 * q, nn)] * x.x * x.x + wgt[node_of(2 * q + 1, nn)] * x.y * x.y;
   }
   if ((n & 1) && tid == 0) {
      double x = w[n - 1];
      for (int j = 0; j < k; j++) x += cf[j] * V0[(int64_t)j * stride + n - 1];
      w[n - 1] = x;
      if (table) acc += wgt[node_of(n - 1, nn)] * x * x;
   }
   if (!table) return;
   const double v = wave_sum(acc);
   if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
   __syncthreads();
   if (threadIdx.x == 0) { double t = sm[0]; for (int wv = 1; wv < GWAVES; wv++) t += sm[wv]; table[blockIdx.x] = t; }
}

// dst = src (* dinv) (* S[slot]); dst may be src
__global__ void __launch_bounds__(GBLK) k_gm_scale(int64_t n, double* dst, const double* src, const double* __restrict__ dinv, const double* __restrict__ S, int slot) {
   if (S[gmres::FLAG] != 0.0) return;
   const double f = slot >= 0 ? S[slot] : 1.0;
   for (int64_t i = (int64_t)blockIdx.x * GBLK + threadIdx.x; i < n; i += (int64_t)gridDim.x * GBLK) dst[i] = (dinv ? dinv[i] * src[i] : src[i]) * f;
}

// dst = (b - t) (* dinv)
__global__ void __launch_bounds__(GBLK) k_gm_resid(int64_t n, double* __restrict__ dst, const double* __restrict__ b, const double* __restrict__ t, const double* __restrict__ dinv,
                                                   const double* __restrict__ S) {
   if (S[gmres::FLAG] != 0.0) return;
   for (int64_t i = (int64_t)blockIdx.x * GBLK + threadIdx.x; i < n; i += (int64_t)gridDim.x * GBLK) { const double r = b[i] - t[i]; dst[i] = dinv ? dinv[i] * r : r; }
}

// The scalar kernel, one block.  First the sums of reduce_cols columns of the table into S[RED ...] (a wave per column, lanes over the blocks in
// a fixed order); then thread 0 runs the stage.  On several ranks the all-reduce of S[RED ...] sits between a launch that only reduces and one that
// only runs the stage.
__global__ void __launch_bounds__(GBLK) k_gm_scalar(double* __restrict__ S, const double* __restrict__ table, int nb, exa_host::GmStage a) {
   __shared__ int sm_gate;
   if (gate_closed(S, a.force ? 2 : (a.gate_reorth ? 1 : 0), &sm_gate)) return;
   if (a.reduce_cols > 0) {
      const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
      for (int c = wave; c < a.reduce_cols; c += GWAVES) {
         double v = 0.0;
         for (int b = lane; b < nb; b += 64) v += table[(int64_t)c * nb + b];
         v = wave_sum(v);
         if (lane == 0) S[gmres::RED + c] = v;
      }
      __syncthreads();
   }
   if (threadIdx.x != 0) return;
   using namespace gmres;
   double* s = S + SVEC;
   switch (a.stage) {
   case exa_host::GmStage::REDUCE: break;
   case exa_host::GmStage::START:
   case exa_host::GmStage::RESTART: {
      const double beta = std::sqrt(S[RED]);
      if (a.stage == exa_host::GmStage::START) {
         S[BETA0] = beta; S[FINAL] = std::fmax(a.rel_tol * beta, a.abs_tol); S[ITERS] = 0.0; S[RESTARTS] = 0.0; S[REORTH_PASSES] = 0.0;
      } else S[RESTARTS] += 1.0;
      S[BETA] = beta; S[RESID] = beta; S[NCOL] = 0.0; S[REORTH] = 0.0;
      for (int k = 0; k <= MAXK; k++) s[k] = 0.0;
      s[0] = beta;
      if (!std::isfinite(beta)) S[FLAG] = F_BREAKDOWN;
      else if (beta <= S[FINAL]) S[FLAG] = F_CONVERGED;
      else { S[SCALE] = 1.0 / beta; S[FLAG] = F_RUNNING; }
      break;
   }
   case exa_host::GmStage::COEF: {
      double* h = S + H + a.col * LDH + a.j0;
      for (int c = 0; c < a.k; c++) { const double v = S[RED + c]; S[COEF + c] = v; h[c] = a.accumulate ? h[c] + v : v; }
      if (a.with_norm) S[WN2_BEFORE] = S[RED + a.k];
      break;
   }
   case exa_host::GmStage::NORM: {
      const double wn2 = S[RED];
      // Daniel, Gragg, Kaufman, Stewart: a second pass when the first one took more than 1 / sqrt(2) of the norm away
      if (a.decide == 2 || (a.decide == 1 && wn2 < 0.5 * S[WN2_BEFORE])) { S[REORTH] = 1.0; break; }
      if (a.gate_reorth) { S[REORTH_PASSES] += 1.0; S[REORTH] = 0.0; }
      const double hn = std::sqrt(wn2);
      S[HNEXT] = hn;
      if (!a.column_update) break;
      double* h = S + H + a.col * LDH;
      h[a.col + 1] = hn;
      const double resid = column_update(a.col, h, S + CS, S + SN, s);
      S[ITERS] += 1.0; S[NCOL] = a.col + 1; S[RESID] = resid;
      S[FLAG] = step_flag(resid, S[FINAL], hn, S[ITERS], (double)a.max_iter);
      if (S[FLAG] == F_RUNNING) S[SCALE] = 1.0 / hn;
      break;
   }
   case exa_host::GmStage::SOLVE:
      (void)back_substitute((int)S[NCOL], S + H, LDH, s, S + Y);
      break;
   }
}

}  // namespace

namespace exa_host {

int gm_chunk() { return CH; }
unsigned gm_blocks(int64_t n) { const int64_t b = ((n >> 1) + GBLK - 1) / GBLK; return (unsigned)(b < 1 ? 1 : (b > GM_BLOCKS ? GM_BLOCKS : b)); }

void gm_multidot(int64_t n, int64_t nn, const double* wgt, const double* V, int64_t stride, int j0, int k, const double* w, bool with_norm, const double* S, int gate,
                 double* table, hipStream_t s) {
   hipLaunchKernelGGL(k_gm_multidot, dim3(gm_blocks(n)), dim3(GBLK), 0, s, n, nn, wgt, V, stride, j0, k, w, with_norm ? 1 : 0, S, gate, table);
}
void gm_multiaxpy(int64_t n, int64_t nn, const double* wgt, const double* V, int64_t stride, int j0, int k, const double* S, int coef, double sign, double* w, int gate,
                  double* table, hipStream_t s) {
   hipLaunchKernelGGL(k_gm_multiaxpy, dim3(gm_blocks(n)), dim3(GBLK), 0, s, n, nn, wgt, V, stride, j0, k, S, coef, sign, w, gate, table);
}
void gm_scale(int64_t n, double* dst, const double* src, const double* dinv, const double* S, int slot, hipStream_t s) {
   hipLaunchKernelGGL(k_gm_scale, dim3(gm_blocks(n) * 2), dim3(GBLK), 0, s, n, dst, src, dinv, S, slot);
}
void gm_resid(int64_t n, double* dst, const double* b, const double* t, const double* dinv, const double* S, hipStream_t s) {
   hipLaunchKernelGGL(k_gm_resid, dim3(gm_blocks(n) * 2), dim3(GBLK), 0, s, n, dst, b, t, dinv, S);
}
void gm_scalar(double* S, const double* table, int nb, const GmStage& a, hipStream_t s) { hipLaunchKernelGGL(k_gm_scalar, dim3(1), dim3(GBLK), 0, s, S, table, nb, a); }

}  // namespace exa_host
