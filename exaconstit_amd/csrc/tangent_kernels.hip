// Kernels of the homogenised tangent of a periodic RVE (gfx950), DESIGN 4.13:
//   k_grad_apply_p1_cols   the p = 1 hexahedron L-vector record action of pa_kernels.hip (k_grad_apply_p1, GEO forms) applied to NCH column
//                          vectors per pass over the record stream - the nine fluctuation solves of the tangent share one operator
//   k_affine_columns       the nine affine nodal fields a_m = E_m (x - origin), E_m the unit 3 x 3 matrices row by row
//   k_macro_contract       per column the 3 x 3 sum over the nodes of y (x) (x - origin), block partials combined in block order
// The record stream is most of what the action moves (208 of 248 B per point with the compact record); a pass over it that serves NCH columns
// reads it once for all of them.  A lane owns an element; per column it keeps the 24 outputs in registers and the 24 gathered inputs in LDS.
#include "exa_internal.hpp"
#include <algorithm>
#include <type_traits>

namespace {

// ---- p = 1 reference table as compile-time constants (the table of pa_kernels.hip) -----------------------------------------------------
constexpr double GL0 = 0.21132486540518713, GL1 = 0.78867513459481287;   // (1 -/+ 1/sqrt 3)/2
constexpr double gl_pt(int i) { return i == 0 ? GL0 : GL1; }
constexpr int VX[8] = { 0, 1, 1, 0, 0, 1, 1, 0 }, VY[8] = { 0, 0, 1, 1, 0, 0, 1, 1 }, VZ[8] = { 0, 0, 0, 0, 1, 1, 1, 1 };
constexpr double n1(int v, double x) { return v ? x : 1.0 - x; }
constexpr double d1(int v) { return v ? 1.0 : -1.0; }
constexpr double G1(int a, int j, int q) {
   const double x = gl_pt(q & 1), y = gl_pt((q >> 1) & 1), z = gl_pt((q >> 2) & 1);
   return j == 0 ? d1(VX[a]) * n1(VY[a], y) * n1(VZ[a], z) : (j == 1 ? n1(VX[a], x) * d1(VY[a]) * n1(VZ[a], z) : n1(VX[a], x) * n1(VY[a], y) * d1(VZ[a]));
}
__device__ __forceinline__ void adj_det(const double* Jq, double adj[9], double& detJ) {
   const double J11 = Jq[0], J21 = Jq[1], J31 = Jq[2], J12 = Jq[3], J22 = Jq[4], J32 = Jq[5], J13 = Jq[6], J23 = Jq[7], J33 = Jq[8];
   adj[0] = J22 * J33 - J23 * J32; adj[1] = J32 * J13 - J12 * J33; adj[2] = J12 * J23 - J22 * J13;
   adj[3] = J31 * J23 - J21 * J33; adj[4] = J11 * J33 - J13 * J31; adj[5] = J21 * J13 - J11 * J23;
   adj[6] = J21 * J32 - J31 * J22; adj[7] = J31 * J12 - J11 * J32; adj[8] = J11 * J22 - J12 * J21;
   detJ = J11 * adj[0] + J21 * adj[1] + J31 * adj[2];
}

template <int NCH> struct ColGates { const double* g[NCH]; };

// CMP: compact record (13 pairs: D, K), otherwise the first 18 pairs of the 46-double record (the scaled tangent); adj(J) is recomputed from the
// nodal coordinates in both forms.  TRANS: C^T (element-assembly contexts on the full record; compact records are stored in the orientation
// the action needs).  Column k reads x + k ldx and adds into y + k ldy.  gates.g[k] (nullable): device flag of column k - a non-zero value
// leaves the column out of the pass: it is neither gathered nor scattered; a block whose columns are all gated returns before the first load.
// The arithmetic of a column is that of k_grad_apply_p1, statement by statement, and does not depend on NCH or on the other columns of the pass.
template <int NCH, bool CMP, bool TRANS, bool NT>
__global__ __launch_bounds__(PA_BLK) void k_grad_apply_p1_cols(const int E, const double* __restrict__ pa, const double* __restrict__ x, const int64_t ldx,
                                                               double* __restrict__ y, const int64_t ldy, const int32_t* __restrict__ conn, const int nnodes,
                                                               const uint8_t* __restrict__ mask, const ColGates<NCH> gates, const double* __restrict__ coords) {
   const int lane = threadIdx.x; const int64_t blk = xcd_block(blockIdx.x, gridDim.x); const int64_t e = blk * PA_BLK + lane;
   if (e >= E) return;
   bool on[NCH]; bool any = false;
#pragma unroll
   for (int k = 0; k < NCH; k++) { on[k] = gates.g[k] == nullptr || gates.g[k][0] == 0.0; any = any || on[k]; }   // (block-uniform)
   if (!any) return;
   // The gathered inputs are parked in LDS (24 doubles per column and lane, lane-contiguous rows: conflict-free 8-byte reads, and a lane reads
   // only what it wrote - no barrier); the outputs, the element's coordinates and two records stay in registers.  With inputs AND outputs in
   // registers two columns already spill (96 registers per column next to the 90 of a record and the 48 of the coordinates).
   __shared__ double sX[NCH * 24 * PA_BLK];
   double Y[NCH][3][8];
   double XC[3][8];
   int g[8];
#pragma unroll
   for (int a = 0; a < 8; a++) g[a] = conn[a + 8 * e];
#pragma unroll
   for (int c = 0; c < 3; c++)
#pragma unroll
      for (int a = 0; a < 8; a++) XC[c][a] = coords[g[a] + (int64_t)nnodes * c];
   {
      // every value and every mask byte is requested before the first one is looked at (k_grad_apply_p1)
      double X[NCH][3][8];
#pragma unroll
      for (int k = 0; k < NCH; k++) {
         if (on[k]) {
#pragma unroll
            for (int c = 0; c < 3; c++)
#pragma unroll
               for (int a = 0; a < 8; a++) X[k][c][a] = x[k * ldx + g[a] + (int64_t)nnodes * c];
         } else {
#pragma unroll
            for (int c = 0; c < 3; c++)
#pragma unroll
               for (int a = 0; a < 8; a++) X[k][c][a] = 0.0;
         }
      }
      if (mask != nullptr) {
         uint8_t mk[3][8];
#pragma unroll
         for (int c = 0; c < 3; c++)
#pragma unroll
            for (int a = 0; a < 8; a++) mk[c][a] = mask[g[a] + (int64_t)nnodes * c];
         __builtin_amdgcn_sched_barrier(0);
#pragma unroll
         for (int k = 0; k < NCH; k++)
#pragma unroll
            for (int c = 0; c < 3; c++)
#pragma unroll
               for (int a = 0; a < 8; a++) X[k][c][a] = mk[c][a] ? 0.0 : X[k][c][a];
      }
#pragma unroll
      for (int k = 0; k < NCH; k++)
#pragma unroll
         for (int c = 0; c < 3; c++)
#pragma unroll
            for (int a = 0; a < 8; a++) sX[((k * 3 + c) * 8 + a) * PA_BLK + lane] = X[k][c][a];
   }
#pragma unroll
   for (int k = 0; k < NCH; k++)
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
         for (int a = 0; a < 8; a++) Y[k][c][a] = 0.0;
   constexpr int NPR = CMP ? PAC_PAIRS : 18;
   auto rec_of = [&](int q) { return reinterpret_cast<const double2*>(pa + (CMP ? pac_off<PAC_PAIRS>(blk, 8, q, 0) : (((blk * 8 + q) * PA_PAIRS) * PA_BLK) * 2)) + lane; };
   // the record of point q + 1 is requested before point q is worked on; the scheduling barrier at the end of a point keeps the compiler from
   // requesting the later ones as well (all eight at once are 4.6 KB per lane)
   double2 nxt[NPR];
   { const double2* rec = rec_of(0);
#pragma unroll
     for (int pr = 0; pr < NPR; pr++) nxt[pr] = ld_rec<NT>(&rec[pr * PA_BLK]); }
#pragma unroll
   for (int q = 0; q < 8; q++) {
      double v[PA_SLOTS];
#pragma unroll
      for (int pr = 0; pr < NPR; pr++) { v[2 * pr] = nxt[pr].x; v[2 * pr + 1] = nxt[pr].y; }
      if (q < 7) {
         const double2* rec = rec_of(q + 1);
#pragma unroll
         for (int pr = 0; pr < NPR; pr++) nxt[pr] = ld_rec<NT>(&rec[pr * PA_BLK]);
      }
      {   // J(i,j) = sum_a x_a,i dN_a/dxi_j, then adj(J) exactly as grad_setup stored it
         double Jl[9];
#pragma unroll
         for (int j = 0; j < 3; j++)
#pragma unroll
            for (int i = 0; i < 3; i++) { double t = 0; for (int a = 0; a < 8; a++) t += G1(a, j, q) * XC[i][a]; Jl[i + 3 * j] = t; }
         double dj; adj_det(Jl, v + 36, dj);
      }
      const double* Ct = v; const double* adj = v + 36;
      // (the parked inputs are the same at every point: an offset the compiler cannot see through keeps it from reading them once and holding them
      //  in registers after all)
      int sl = lane; asm volatile("" : "+v"(sl));
#pragma unroll
      for (int k = 0; k < NCH; k++) {
         double gx[3][3];
#pragma unroll
         for (int c = 0; c < 3; c++) {
            double xk[8];
#pragma unroll
            for (int a = 0; a < 8; a++) xk[a] = sX[((k * 3 + c) * 8 + a) * PA_BLK + sl];
#pragma unroll
            for (int j = 0; j < 3; j++) { double s = 0; for (int a = 0; a < 8; a++) s += G1(a, j, q) * xk[a]; gx[c][j] = s; }
         }
         double h[3][3];
#pragma unroll
         for (int c = 0; c < 3; c++)
#pragma unroll
            for (int t = 0; t < 3; t++) h[c][t] = gx[c][0] * adj[t] + gx[c][1] * adj[3 + t] + gx[c][2] * adj[6 + t];
         const double eps[6] = { h[0][0], h[1][1], h[2][2], h[1][2] + h[2][1], h[0][2] + h[2][0], h[0][1] + h[1][0] };
         double sg[6];
         static_assert(!(CMP && TRANS), "compact records are stored in the orientation the action needs");
         if (CMP) d55_apply(v, v[25], eps, sg);
         else {
#pragma unroll
            for (int i = 0; i < 6; i++) { double s = 0; for (int j = 0; j < 6; j++) s += (TRANS ? Ct[j + 6 * i] : Ct[i + 6 * j]) * eps[j]; sg[i] = s; }
         }
         const double S[3][3] = { { sg[0], sg[5], sg[4] }, { sg[5], sg[1], sg[3] }, { sg[4], sg[3], sg[2] } };
         double T[3][3];
#pragma unroll
         for (int j = 0; j < 3; j++)
#pragma unroll
            for (int c = 0; c < 3; c++) T[j][c] = adj[3 * j] * S[0][c] + adj[3 * j + 1] * S[1][c] + adj[3 * j + 2] * S[2][c];
#pragma unroll
         for (int c = 0; c < 3; c++)
#pragma unroll
            for (int a = 0; a < 8; a++) Y[k][c][a] += G1(a, 0, q) * T[0][c] + G1(a, 1, q) * T[1][c] + G1(a, 2, q) * T[2][c];
      }
      // (one basic block holds all eight points, and nothing but the scatter at its end consumes the sums: without a use here the instruction selector
      //  sinks the arithmetic of every point below the last record load and keeps all eight records alive for it)
#pragma unroll
      for (int k = 0; k < NCH; k++)
#pragma unroll
         for (int c = 0; c < 3; c++)
#pragma unroll
            for (int a = 0; a < 8; a++) asm volatile("" : "+v"(Y[k][c][a]));
      __builtin_amdgcn_sched_barrier(0);
   }
#pragma unroll
   for (int k = 0; k < NCH; k++) {
      if (!on[k]) continue;
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
         for (int a = 0; a < 8; a++) atomicAdd(&y[k * ldy + g[a] + (int64_t)nnodes * c], Y[k][c][a]);
   }
}

// out[m ld + g + nn c], m = 3 i + j: component i of a_m is x_j - o_j, the other two are zero.  One thread per node.
struct double3v { double a[3]; };
__global__ __launch_bounds__(256) void k_affine_columns(const int nn, const double* __restrict__ xc, const double3v org, double* __restrict__ out, const int64_t ld) {
   const int g = blockIdx.x * blockDim.x + threadIdx.x;
   if (g >= nn) return;
   const double d[3] = { xc[g] - org.a[0], xc[g + (int64_t)nn] - org.a[1], xc[g + 2 * (int64_t)nn] - org.a[2] };
#pragma unroll
   for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++)
#pragma unroll
         for (int c = 0; c < 3; c++) out[(3 * i + j) * ld + g + (int64_t)nn * c] = c == i ? d[j] : 0.0;
}

// part[(b NC + m) 9 + 3 k + l] = sum over the nodes of block b of y_m(g, k) (x(g, l) - o_l).  A block walks its nodes with the grid stride, so a
// coordinate and a column value are read once per launch; the 256 lanes are summed by shuffles within a wave and the four waves through LDS in
// wave order.  k_macro_combine adds the block partials in block order: a fixed order and no atomics - the same bits in every run (the
// arrangement of the face resultants, periodic_kernels.hip).
template <int NC>
__global__ __launch_bounds__(256) void k_macro_contract(const int nn, const double* __restrict__ y, const int64_t ldy, const double* __restrict__ xc, const double3v org,
                                                        double* __restrict__ part) {
   __shared__ double lds[4][9 * NC];
   double acc[NC][9];
#pragma unroll
   for (int m = 0; m < NC; m++)
#pragma unroll
      for (int t = 0; t < 9; t++) acc[m][t] = 0.0;
   for (int g = blockIdx.x * 256 + threadIdx.x; g < nn; g += gridDim.x * 256) {
      const double d[3] = { xc[g] - org.a[0], xc[g + (int64_t)nn] - org.a[1], xc[g + 2 * (int64_t)nn] - org.a[2] };
#pragma unroll
      for (int m = 0; m < NC; m++)
#pragma unroll
         for (int k = 0; k < 3; k++) {
            const double yk = y[m * ldy + g + (int64_t)nn * k];
#pragma unroll
            for (int l = 0; l < 3; l++) acc[m][3 * k + l] += yk * d[l];
         }
   }
   const int w = threadIdx.x >> 6;
#pragma unroll
   for (int m = 0; m < NC; m++)
#pragma unroll
      for (int t = 0; t < 9; t++) {
         double s = acc[m][t];
         for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
         if ((threadIdx.x & 63) == 0) lds[w][9 * m + t] = s;
      }
   __syncthreads();
   if (threadIdx.x < 9 * NC) part[(int64_t)blockIdx.x * 9 * NC + threadIdx.x] = ((lds[0][threadIdx.x] + lds[1][threadIdx.x]) + lds[2][threadIdx.x]) + lds[3][threadIdx.x];
}
__global__ void k_macro_combine(const int nb, const int n, const double* __restrict__ part, double* __restrict__ out) {
   const int t = threadIdx.x;
   if (t >= n) return;
   double s = 0.0;
   for (int b = 0; b < nb; b++) s += part[(int64_t)b * n + t];
   out[t] = s;
}

inline unsigned nblk(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

template <int NCH>
int launch_cols(exa_ctx* ctx, const double* x, int64_t ldx, double* y, int64_t ldy, const uint8_t* mask, const double* const* gates, bool trans, hipStream_t s) {
   const unsigned nb = exa_nblocks(ctx);
   if (nb == 0) return EXA_OK;
   ColGates<NCH> G;
   for (int k = 0; k < NCH; k++) G.g[k] = gates ? gates[k] : nullptr;
   const bool cmp = exa_has_compact(ctx);
   if constexpr (NCH == 3) { if (!cmp) { ctx->err = "three columns per pass are built for the compact record"; return EXA_ERR_ARG; } }
   // (the hint follows the size of the record stream, as in exa_launch_grad_apply_p1)
   const bool nt = exa_stream_nt((size_t)ctx->P * 16 * (cmp ? PAC_PAIRS : 18));
   auto go = [&](auto cm, auto t, auto n) {
      hipLaunchKernelGGL((k_grad_apply_p1_cols<NCH, cm.value, t.value, n.value>), dim3(nb), dim3(PA_BLK), 0, s, ctx->E, cm.value ? ctx->pa_c : ctx->pa, x, ldx, y, ldy, ctx->conn, ctx->nnodes, mask, G, ctx->coords_lvec);
   };
   if (cmp) exa_dispatch([&](auto n) { go(EXA_YES, EXA_NO, n); }, nt);   // D or D^T in the record
   else if constexpr (NCH < 3) exa_dispatch([&](auto t, auto n) { go(EXA_NO, t, n); }, trans, nt);   // (no three-column instantiation on the 46-double record)
   return exa_launched(ctx);
}

}  // namespace

// columns [0, ncols) in passes of `nch` (1 .. 3) columns and a remainder of single-column passes: the same arithmetic per column either way
// (the caller has checked that the records this reads exist: exa_grad_apply_lvec_cols, capi.hip)
int exa_launch_grad_apply_p1_cols(exa_ctx* ctx, int ncols, const double* x, int64_t ldx, double* y, int64_t ldy, const uint8_t* mask, const double* const* gates, bool trans,
                                  int nch, hipStream_t s) {
   // (the 36-double record and its successor next to three columns' sums do not fit the register file: two columns per pass there)
   if (nch > 2 && !exa_has_compact(ctx)) nch = 2;
   int k = 0;
   while (k < ncols) {
      const int left = ncols - k;
      const int w = (nch >= 3 && left >= 3) ? 3 : ((nch == 2 && left >= 2) ? 2 : 1);
      const double* const* gk = gates ? gates + k : nullptr;
      int rc;
      if (w == 3) rc = launch_cols<3>(ctx, x + k * ldx, ldx, y + k * ldy, ldy, mask, gk, trans, s);
      else if (w == 2) rc = launch_cols<2>(ctx, x + k * ldx, ldx, y + k * ldy, ldy, mask, gk, trans, s);
      else rc = launch_cols<1>(ctx, x + k * ldx, ldx, y + k * ldy, ldy, mask, gk, trans, s);
      if (rc) return rc;
      k += w;
   }
   return EXA_OK;
}

int exa_launch_affine_columns(exa_ctx* ctx, int nn, const double* xc, const double* org3, double* out, int64_t ld, hipStream_t s) {
   double3v o; for (int i = 0; i < 3; i++) o.a[i] = org3[i];
   if (nn > 0) hipLaunchKernelGGL(k_affine_columns, dim3(nblk(nn, 256)), dim3(256), 0, s, nn, xc, o, out, ld);
   return exa_launched(ctx);
}

// out[9 m + 3 k + l], m < ncols; work: >= EXA_MACRO_BLOCKS * 9 * 9 doubles
constexpr int EXA_MACRO_BLOCKS = 256;
int exa_launch_macro_contract(exa_ctx* ctx, int nn, int ncols, const double* y, int64_t ldy, const double* xc, const double* org3, double* work, double* out, hipStream_t s) {
   double3v o; for (int i = 0; i < 3; i++) o.a[i] = org3[i];
   const unsigned nb = std::max(1u, std::min((unsigned)EXA_MACRO_BLOCKS, nblk(nn, 256)));
   int m = 0;
   while (m < ncols) {   // nine columns per launch (the tangent's case), single columns otherwise
      if (ncols - m >= 9) {
         hipLaunchKernelGGL(k_macro_contract<9>, dim3(nb), dim3(256), 0, s, nn, y + m * ldy, ldy, xc, o, work);
         hipLaunchKernelGGL(k_macro_combine, dim3(1), dim3(128), 0, s, (int)nb, 81, work, out + 9 * m);
         m += 9;
      } else {
         hipLaunchKernelGGL(k_macro_contract<1>, dim3(nb), dim3(256), 0, s, nn, y + m * ldy, ldy, xc, o, work);
         hipLaunchKernelGGL(k_macro_combine, dim3(1), dim3(128), 0, s, (int)nb, 9, work, out + 9 * m);
         m += 1;
      }
   }
   return exa_launched(ctx);
}

// private (scratch) bytes per lane of the kernels of this file in the loaded code object: out8 = { k_grad_apply_p1_cols<1>, <2>, <3> (the largest
// over their record forms), k_affine_columns, k_macro_contract<9>, k_macro_contract<1>, k_macro_combine, 0 }; returns 0, or -1 without a device
extern "C" int exa_tangent_scratch_bytes(int* out8) {
   hipFuncAttributes a;
   auto get = [&](const void* f) -> int { if (hipFuncGetAttributes(&a, f) != hipSuccess) { (void)hipGetLastError(); return -1; } return (int)a.localSizeBytes; };
   auto cols = [&](auto nch) -> int {
      constexpr int N = decltype(nch)::value; constexpr int M = N < 3 ? N : 2;   // (three columns: compact record only)
      const void* f[6] = { reinterpret_cast<const void*>(k_grad_apply_p1_cols<N, true, false, true>), reinterpret_cast<const void*>(k_grad_apply_p1_cols<N, true, false, false>),
                           reinterpret_cast<const void*>(k_grad_apply_p1_cols<M, false, false, true>), reinterpret_cast<const void*>(k_grad_apply_p1_cols<M, false, false, false>),
                           reinterpret_cast<const void*>(k_grad_apply_p1_cols<M, false, true, true>), reinterpret_cast<const void*>(k_grad_apply_p1_cols<M, false, true, false>) };
      int worst = 0;
      for (const void* p : f) { const int b = get(p); if (b < 0) return -1; worst = std::max(worst, b); }
      return worst;
   };
   out8[0] = cols(std::integral_constant<int, 1>()); out8[1] = cols(std::integral_constant<int, 2>()); out8[2] = cols(std::integral_constant<int, 3>());
   out8[3] = get(reinterpret_cast<const void*>(k_affine_columns));
   out8[4] = get(reinterpret_cast<const void*>(k_macro_contract<9>)); out8[5] = get(reinterpret_cast<const void*>(k_macro_contract<1>));
   out8[6] = get(reinterpret_cast<const void*>(k_macro_combine)); out8[7] = 0;
   for (int k = 0; k < 7; k++) if (out8[k] < 0) return -1;
   return 0;
}
