// Checkpoint support: quadrature functions between the context's layout and the canonical (vdim, Q, E) rows of a checkpoint
// file, with the 64-bit checksum of the section computed in the same pass.
//   EXA_QLAYOUT_EB64  one wave per block of 64 elements.  Per pass the wave moves the 512-byte (q, component) rows of QG quadrature points of
//                     the block and, per element, the run of QG vdim contiguous canonical doubles of those points through a [QG vdim][65]
//                     tile of its own LDS (odd row stride: both the row-wise and the column-wise pass are free of bank conflicts); the
//                     canonical side is touched with 16-byte accesses whenever vdim is even and the buffer is 16-byte aligned.  QG = as
//                     many points as fit 48 tile rows: all 8 for the stress (the block's 64 Q vdim canonical doubles are then ONE
//                     contiguous run written front to back), one for the 28 state variables (runs of 224 bytes).
//   EXA_QLAYOUT_AOS   the context's layout is the canonical one: a grid-stride copy (16-byte accesses) that also sums.
// Checksum = sum of the values' bit patterns as unsigned 64-bit integers modulo 2^64.  Integer addition is associative, so the value does
// not depend on the order of the blocks, on the layout or on how the elements are spread over ranks; the padding lanes of the last
// element block are not part of it.  One integer atomic per wave (plain C++ atomicAdd on device memory).
#include <algorithm>
#include "exa_internal.hpp"

namespace {

constexpr int TILE_STRIDE = 65;
constexpr int QF_PACK_MAX_VDIM = 96;
// rows of a pass: as many quadrature points as fit 48 rows (25 KB of LDS, 6 waves per CU).  Measured at 128^3 with 96 rows: the stress (all 8 points
// in one pass) packs in 0.45 ms instead of 0.77, but the state (3 points, 44 KB, 3 waves per CU) unpacks in 3.5 ms instead of 1.6 - the canonical
// reads of the unpack need the waves more than the longer runs.  A vdim above 48 takes one point per pass.
constexpr int TILE_MAX_ROWS = 48;

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
   for (int off = 32; off > 0; off >>= 1) {
      const unsigned lo = __shfl_down((unsigned)(v & 0xffffffffull), off), hi = __shfl_down((unsigned)(v >> 32), off);
      v += ((unsigned long long)hi << 32) | lo;
   }
   return v;
}

// PACK: eb (element-blocked) -> can (canonical); otherwise can -> eb.  V2: 16-byte accesses on the canonical side (W even, can 16-byte aligned).
// QG quadrature points per pass: an element's canonical doubles of those points are one run of QG W doubles, so a pass moves nel runs of that
// length (the block's whole contiguous region when QG = Q)
template <bool PACK, bool V2>
__global__ __launch_bounds__(64) void k_qf_eb64(const int W, const int Q, const int QG, const int64_t E, const double* __restrict__ src, double* __restrict__ dst,
                                                unsigned long long* __restrict__ cks) {
   extern __shared__ double tile[];   // [QG W][TILE_STRIDE]
   const int lane = threadIdx.x;
   const int64_t b = blockIdx.x;
   const int nel = (int)(E - 64 * b < 64 ? E - 64 * b : 64);
   const double* eb_r = PACK ? src : nullptr; double* eb_w = PACK ? nullptr : dst;
   const double* can_r = PACK ? nullptr : src; double* can_w = PACK ? dst : nullptr;
   const int64_t can0 = 64 * b * Q * (int64_t)W;   // first canonical double of this block
   unsigned long long sum = 0;
   for (int q0 = 0; q0 < Q; q0 += QG) {
      const int R = (Q - q0 < QG ? Q - q0 : QG) * W;   // rows of the tile = doubles of an element's run in this pass
      const int64_t eb0 = ((b * Q + q0) * (int64_t)W) << 6;      // (q, component) rows of the pass are consecutive: row r at eb0 + 64 r
      const int n = nel * R;
      if (PACK) {
         if (lane < nel)
            for (int r = 0; r < R; r++) { const double v = eb_r[eb0 + ((int64_t)r << 6) + lane]; tile[r * TILE_STRIDE + lane] = v; sum += (unsigned long long)__double_as_longlong(v); }
         __syncthreads();
         if (V2) {
            for (int i2 = lane; 2 * i2 < n; i2 += 64) {
               const int i = 2 * i2, e = i / R, r = i - e * R;
               *reinterpret_cast<double2*>(can_w + can0 + ((int64_t)e * Q + q0) * W + r) = make_double2(tile[r * TILE_STRIDE + e], tile[(r + 1) * TILE_STRIDE + e]);
            }
         } else {
            for (int i = lane; i < n; i += 64) { const int e = i / R, r = i - e * R; can_w[can0 + ((int64_t)e * Q + q0) * W + r] = tile[r * TILE_STRIDE + e]; }
         }
         __syncthreads();
      } else {
         if (V2) {
            for (int i2 = lane; 2 * i2 < n; i2 += 64) {
               const int i = 2 * i2, e = i / R, r = i - e * R;
               const double2 v = *reinterpret_cast<const double2*>(can_r + can0 + ((int64_t)e * Q + q0) * W + r);
               tile[r * TILE_STRIDE + e] = v.x; tile[(r + 1) * TILE_STRIDE + e] = v.y;
            }
         } else {
            for (int i = lane; i < n; i += 64) { const int e = i / R, r = i - e * R; tile[r * TILE_STRIDE + e] = can_r[can0 + ((int64_t)e * Q + q0) * W + r]; }
         }
         __syncthreads();
         if (lane < nel)
            for (int r = 0; r < R; r++) { const double v = tile[r * TILE_STRIDE + lane]; eb_w[eb0 + ((int64_t)r << 6) + lane] = v; sum += (unsigned long long)__double_as_longlong(v); }
         __syncthreads();
      }
   }
   if (cks) { sum = wave_sum_u64(sum); if (lane == 0) atomicAdd(cks, sum); }
}

template <bool V2>
__global__ __launch_bounds__(256) void k_qf_copy(const int64_t n, const double* __restrict__ src, double* __restrict__ dst, unsigned long long* __restrict__ cks) {
   unsigned long long sum = 0;
   const int64_t stride = (int64_t)gridDim.x * blockDim.x, t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
   if (V2) {
      for (int64_t i = t; 2 * i + 1 < n; i += stride) {
         const double2 v = reinterpret_cast<const double2*>(src)[i]; reinterpret_cast<double2*>(dst)[i] = v;
         sum += (unsigned long long)__double_as_longlong(v.x) + (unsigned long long)__double_as_longlong(v.y);
      }
      if (t == 0 && (n & 1)) { const double v = src[n - 1]; dst[n - 1] = v; sum += (unsigned long long)__double_as_longlong(v); }
   } else {
      for (int64_t i = t; i < n; i += stride) { const double v = src[i]; dst[i] = v; sum += (unsigned long long)__double_as_longlong(v); }
   }
   if (cks) { sum = wave_sum_u64(sum); if ((threadIdx.x & 63) == 0) atomicAdd(cks, sum); }
}

int launch(exa_ctx* ctx, bool pack, int vdim, const double* src, double* dst, unsigned long long* cks, hipStream_t s) {
   if (vdim < 1 || vdim > QF_PACK_MAX_VDIM) { ctx->err = "exa_qf_pack / exa_qf_unpack: vdim must lie in 1 ... 96"; return EXA_ERR_ARG; }
   if (cks) EXA_HIP_CHECK(ctx, hipMemsetAsync(cks, 0, sizeof(unsigned long long), s));
   if (ctx->E <= 0) return EXA_OK;
   const double* can = pack ? dst : src;
   const bool al16 = ((reinterpret_cast<uintptr_t>(can) & 15u) == 0);
   if (ctx->qblk) {
      const bool v2 = al16 && (vdim % 2 == 0);
      const unsigned nb = (unsigned)((ctx->E + 63) / 64);
      const int QG = std::max(1, std::min(ctx->Q, TILE_MAX_ROWS / vdim));
      const size_t lds = sizeof(double) * (size_t)vdim * QG * TILE_STRIDE;
      const int64_t E = ctx->E;
      if (pack) { if (v2) hipLaunchKernelGGL((k_qf_eb64<true, true>), dim3(nb), dim3(64), lds, s, vdim, ctx->Q, QG, E, src, dst, cks);
                  else hipLaunchKernelGGL((k_qf_eb64<true, false>), dim3(nb), dim3(64), lds, s, vdim, ctx->Q, QG, E, src, dst, cks); }
      else      { if (v2) hipLaunchKernelGGL((k_qf_eb64<false, true>), dim3(nb), dim3(64), lds, s, vdim, ctx->Q, QG, E, src, dst, cks);
                  else hipLaunchKernelGGL((k_qf_eb64<false, false>), dim3(nb), dim3(64), lds, s, vdim, ctx->Q, QG, E, src, dst, cks); }
   } else {
      const int64_t n = (int64_t)vdim * ctx->P;
      const bool v2 = al16 && ((reinterpret_cast<uintptr_t>(pack ? (const double*)src : (const double*)dst) & 15u) == 0);
      const int64_t work = v2 ? (n + 1) / 2 : n;
      const unsigned nb = (unsigned)std::min<int64_t>((work + 255) / 256, 8192);
      if (v2) hipLaunchKernelGGL((k_qf_copy<true>), dim3(nb), dim3(256), 0, s, n, src, dst, cks);
      else hipLaunchKernelGGL((k_qf_copy<false>), dim3(nb), dim3(256), 0, s, n, src, dst, cks);
   }
   EXA_HIP_CHECK(ctx, hipGetLastError());
   return EXA_OK;
}

}  // namespace

int exa_launch_qf_pack(exa_ctx* ctx, int vdim, const double* src, double* dst, unsigned long long* cks, hipStream_t s) { return launch(ctx, true, vdim, src, dst, cks, s); }
int exa_launch_qf_unpack(exa_ctx* ctx, int vdim, const double* src, double* dst, unsigned long long* cks, hipStream_t s) { return launch(ctx, false, vdim, src, dst, cks, s); }
