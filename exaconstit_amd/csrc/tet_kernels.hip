// Tetrahedron operator kernels (gfx950), DESIGN 4.9: the fused L-vector gradient action of straight-sided tetrahedra at p = 1 and p = 2.
//   AddMultGradPA / element-assembly mat-vec of the reference for any MFEM element   reference src/mechanics_integrators.cpp:562-622, 1195-1604
// Every tetrahedron here is straight-sided (file meshes are read with H1_3D_P1 geometry, the p = 2 nodes sit at the edge midpoints), so J is
// constant in the element.  At p = 1 the strain-displacement matrix B is constant as well and the Q = 5 point tangents contract exactly into one
// element tangent  Cbar = dt detJ sum_q W_q C_q  (W_q includes the negative centroid weight of the degree-3 rule):
//   y_e = B^T Cbar B x_e   (EA contexts: Cbar^T, the operator the assembled element matrices apply, k_ea_apply_rt)
// which is the reference's per-point action up to round-off.  Record of an element (p = 1): Cbar (36, column-major Voigt, engineering shear) +
// J^-1 (9, row-major) + 1 spare = 23 16-byte pairs, [block of 64 elements][pair][64 lanes][2] like every record stream of the library.
// p = 2: the 46-double point records of exa_grad_setup (pa_kernels.hip, k_grad_setup_pa) are streamed; the 10 x 3 x 14 shape-gradient table
// sits in LDS.  One lane per element, one wave per 64-element block, scatter with FP64 atomics (as k_grad_apply_p1).
#include "exa_internal.hpp"

namespace {

constexpr int TET_PAIRS = 23;
__device__ __forceinline__ int64_t tet_off(int64_t blk, int pair) { return ((blk * TET_PAIRS + pair) * PA_BLK) * 2; }
__device__ __forceinline__ int64_t pa_off_t(int64_t blk, int Q, int q, int pair) { return (((blk * Q + q) * PA_PAIRS + pair) * PA_BLK) * 2; }

// element record at p = 1 from the Jacobian and tangent fields; TRD: Cbar^T (element-assembly contexts)
template <bool QB, bool TRD>
__global__ __launch_bounds__(PA_BLK) void k_tet_setup_p1(const int E, const double dt, const double* __restrict__ W, const double* __restrict__ J,
                                                         const double* __restrict__ C, double* __restrict__ rec) {
   constexpr int Q = 5;
   const int lane = threadIdx.x; const int64_t blk = blockIdx.x; const int64_t e = blk * PA_BLK + lane;
   if (e >= E) return;
   // J is the same at every point of an affine element (the p = 1 shape gradients are constants): point 0's
   const QView vj = qview<QB>(9, Q, e, 0);
   const double* Jq = J + vj.base; const int64_t st = vj.stride;
   const double J11 = Jq[0], J21 = Jq[st], J31 = Jq[2 * st], J12 = Jq[3 * st], J22 = Jq[4 * st], J32 = Jq[5 * st], J13 = Jq[6 * st], J23 = Jq[7 * st], J33 = Jq[8 * st];
   double adj[9];
   adj[0] = J22 * J33 - J23 * J32; adj[1] = J32 * J13 - J12 * J33; adj[2] = J12 * J23 - J22 * J13;
   adj[3] = J31 * J23 - J21 * J33; adj[4] = J11 * J33 - J13 * J31; adj[5] = J21 * J13 - J11 * J23;
   adj[6] = J21 * J32 - J31 * J22; adj[7] = J31 * J12 - J11 * J32; adj[8] = J11 * J22 - J12 * J21;
   const double detJ = J11 * adj[0] + J21 * adj[1] + J31 * adj[2], di = 1.0 / detJ;
   double v[2 * TET_PAIRS];
#pragma unroll
   for (int i = 0; i < 36; i++) v[i] = 0.0;
   for (int q = 0; q < Q; q++) {
      const QView vc = qview<QB>(36, Q, e, q);
      const double wq = W[q];
#pragma unroll
      for (int i = 0; i < 36; i++) v[i] += wq * C[vc.base + (int64_t)i * vc.stride];
   }
   const double sc = dt * detJ;
   if (TRD) {
#pragma unroll
      for (int i = 0; i < 6; i++)
#pragma unroll
         for (int j = 0; j < i; j++) { const double t = v[i + 6 * j]; v[i + 6 * j] = v[j + 6 * i]; v[j + 6 * i] = t; }
   }
#pragma unroll
   for (int i = 0; i < 36; i++) v[i] *= sc;
#pragma unroll
   for (int i = 0; i < 9; i++) v[36 + i] = adj[i] * di;
   v[45] = 0.0;
   double2* r = reinterpret_cast<double2*>(rec + tet_off(blk, 0)) + lane;
#pragma unroll
   for (int pr = 0; pr < TET_PAIRS; pr++) r[pr * PA_BLK] = make_double2(v[2 * pr], v[2 * pr + 1]);
}

// gather of an element's N nodes (all values and mask bytes requested before the first is used, as k_grad_apply_p1)
template <int N>
__device__ __forceinline__ void tet_gather(const int64_t e, const int32_t* __restrict__ conn, const int nnodes, const double* __restrict__ x,
                                           const uint8_t* __restrict__ mask, int (&g)[N], double (&X)[3][N]) {
#pragma unroll
   for (int a = 0; a < N; a++) g[a] = conn[a + N * e];
#pragma unroll
   for (int c = 0; c < 3; c++)
#pragma unroll
      for (int a = 0; a < N; a++) X[c][a] = x[g[a] + (int64_t)nnodes * c];
   if (mask != nullptr) {
      uint8_t mk[3][N];
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
         for (int a = 0; a < N; a++) mk[c][a] = mask[g[a] + (int64_t)nnodes * c];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
         for (int a = 0; a < N; a++) X[c][a] = mk[c][a] ? 0.0 : X[c][a];
   }
}

// s = C eps with C column-major 6 x 6 (TRANS: C^T)
template <bool TRANS>
__device__ __forceinline__ void c_apply(const double* Ct, const double eps[6], double sg[6]) {
#pragma unroll
   for (int i = 0; i < 6; i++) {
      double t = 0.0;
#pragma unroll
      for (int j = 0; j < 6; j++) t += (TRANS ? Ct[j + 6 * i] : Ct[i + 6 * j]) * eps[j];
      sg[i] = t;
   }
}

// p = 1: y_e += B^T Cbar B x_e.  Reference gradients dN_0 = (-1,-1,-1), dN_{1+s} = e_s.
// GEO: J^-1 recomputed from the four vertex coordinates (gathered through the same connectivity, L2-resident node rows) instead of read from
// the record: 18 instead of 23 record pairs per element (the formula of k_tet_setup_p1).
template <bool NT, bool GEO>
__global__ __launch_bounds__(PA_BLK) void k_tet_apply_p1(const int E, const double* __restrict__ rec, const double* __restrict__ x, double* __restrict__ y,
                                                         const int32_t* __restrict__ conn, const int nnodes, const uint8_t* __restrict__ mask,
                                                         const double* __restrict__ gate, const double* __restrict__ coords) {
   const int lane = threadIdx.x; const int64_t blk = xcd_block(blockIdx.x, gridDim.x); const int64_t e = blk * PA_BLK + lane;
   if (e >= E) return;
   if (gate != nullptr && gate[0] != 0.0) return;
   int g[4]; double X[3][4];
   tet_gather<4>(e, conn, nnodes, x, mask, g, X);
   constexpr int NPR = GEO ? 18 : TET_PAIRS;
   double v[2 * TET_PAIRS];
   const double2* r = reinterpret_cast<const double2*>(rec + tet_off(blk, 0)) + lane;
#pragma unroll
   for (int pr = 0; pr < NPR; pr++) { const double2 t = ld_rec<NT>(&r[pr * PA_BLK]); v[2 * pr] = t.x; v[2 * pr + 1] = t.y; }
   if constexpr (GEO) {
      double XC[3][4];
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
         for (int a = 0; a < 4; a++) XC[c][a] = coords[g[a] + (int64_t)nnodes * c];
      // J(i, j) = dx_i / dxi_j = x_{j+1, i} - x_{0, i} (k_jacobians sums -x_0 + x_{j+1} + 0 + 0: the same value)
      const double J11 = -XC[0][0] + XC[0][1], J21 = -XC[1][0] + XC[1][1], J31 = -XC[2][0] + XC[2][1];
      const double J12 = -XC[0][0] + XC[0][2], J22 = -XC[1][0] + XC[1][2], J32 = -XC[2][0] + XC[2][2];
      const double J13 = -XC[0][0] + XC[0][3], J23 = -XC[1][0] + XC[1][3], J33 = -XC[2][0] + XC[2][3];
      double adj[9];
      adj[0] = J22 * J33 - J23 * J32; adj[1] = J32 * J13 - J12 * J33; adj[2] = J12 * J23 - J22 * J13;
      adj[3] = J31 * J23 - J21 * J33; adj[4] = J11 * J33 - J13 * J31; adj[5] = J21 * J13 - J11 * J23;
      adj[6] = J21 * J32 - J31 * J22; adj[7] = J31 * J12 - J11 * J32; adj[8] = J11 * J22 - J12 * J21;
      const double di = 1.0 / (J11 * adj[0] + J21 * adj[1] + J31 * adj[2]);
#pragma unroll
      for (int i = 0; i < 9; i++) v[36 + i] = adj[i] * di;
   }
   const double* Ji = v + 36;
   double h[3][3];   // h[c][t] = du_c / dx_t
#pragma unroll
   for (int c = 0; c < 3; c++) {
      const double g0 = X[c][1] - X[c][0], g1 = X[c][2] - X[c][0], g2 = X[c][3] - X[c][0];
#pragma unroll
      for (int t = 0; t < 3; t++) h[c][t] = g0 * Ji[t] + g1 * Ji[3 + t] + g2 * Ji[6 + t];
   }
   const double eps[6] = { h[0][0], h[1][1], h[2][2], h[1][2] + h[2][1], h[0][2] + h[2][0], h[0][1] + h[1][0] };
   double sg[6]; c_apply<false>(v, eps, sg);
   const double Sm[3][3] = { { sg[0], sg[5], sg[4] }, { sg[5], sg[1], sg[3] }, { sg[4], sg[3], sg[2] } };
#pragma unroll
   for (int c = 0; c < 3; c++) {
      double T[3];
#pragma unroll
      for (int j = 0; j < 3; j++) T[j] = Ji[3 * j] * Sm[0][c] + Ji[3 * j + 1] * Sm[1][c] + Ji[3 * j + 2] * Sm[2][c];
      atomicAdd(&y[g[0] + (int64_t)nnodes * c], -(T[0] + T[1] + T[2]));
#pragma unroll
      for (int j = 0; j < 3; j++) atomicAdd(&y[g[1 + j] + (int64_t)nnodes * c], T[j]);
   }
}

// p = 2: 14 points of the 46-double records (Ct = C dt W / detJ, adj(J), W detJ); TRANS: Ct^T (element-assembly contexts)
template <bool TRANS, bool NT>
__global__ __launch_bounds__(PA_BLK) void k_tet_apply_p2(const int E, const double* __restrict__ pa, const double* __restrict__ G, const double* __restrict__ x,
                                                         double* __restrict__ y, const int32_t* __restrict__ conn, const int nnodes,
                                                         const uint8_t* __restrict__ mask, const double* __restrict__ gate) {
   constexpr int N = 10, Q = 14;
   __shared__ double sG[N * 3 * Q];
   for (int i = threadIdx.x; i < N * 3 * Q; i += PA_BLK) sG[i] = G[i];
   __syncthreads();
   const int lane = threadIdx.x; const int64_t blk = xcd_block(blockIdx.x, gridDim.x); const int64_t e = blk * PA_BLK + lane;
   if (e >= E) return;
   if (gate != nullptr && gate[0] != 0.0) return;
   int g[N]; double X[3][N], Y[3][N];
   tet_gather<N>(e, conn, nnodes, x, mask, g, X);
#pragma unroll
   for (int c = 0; c < 3; c++)
#pragma unroll
      for (int a = 0; a < N; a++) Y[c][a] = 0.0;
   for (int q = 0; q < Q; q++) {
      const double* Gq = sG + 3 * N * q;
      const double2* r = reinterpret_cast<const double2*>(pa + pa_off_t(blk, Q, q, 0)) + lane;
      double v[PA_SLOTS];
#pragma unroll
      for (int pr = 0; pr < PA_PAIRS; pr++) { const double2 t = ld_rec<NT>(&r[pr * PA_BLK]); v[2 * pr] = t.x; v[2 * pr + 1] = t.y; }
      const double* adj = v + 36;
      double gx[3][3];
#pragma unroll
      for (int c = 0; c < 3; c++) {
         double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
         for (int a = 0; a < N; a++) { s0 += Gq[a] * X[c][a]; s1 += Gq[a + N] * X[c][a]; s2 += Gq[a + 2 * N] * X[c][a]; }
         gx[c][0] = s0; gx[c][1] = s1; gx[c][2] = s2;
      }
      double h[3][3];
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
         for (int t = 0; t < 3; t++) h[c][t] = gx[c][0] * adj[t] + gx[c][1] * adj[3 + t] + gx[c][2] * adj[6 + t];
      const double eps[6] = { h[0][0], h[1][1], h[2][2], h[1][2] + h[2][1], h[0][2] + h[2][0], h[0][1] + h[1][0] };
      double sg[6]; c_apply<TRANS>(v, eps, sg);
      const double Sm[3][3] = { { sg[0], sg[5], sg[4] }, { sg[5], sg[1], sg[3] }, { sg[4], sg[3], sg[2] } };
#pragma unroll
      for (int c = 0; c < 3; c++) {
         double T[3];
#pragma unroll
         for (int j = 0; j < 3; j++) T[j] = adj[3 * j] * Sm[0][c] + adj[3 * j + 1] * Sm[1][c] + adj[3 * j + 2] * Sm[2][c];
#pragma unroll
         for (int a = 0; a < N; a++) Y[c][a] += Gq[a] * T[0] + Gq[a + N] * T[1] + Gq[a + 2 * N] * T[2];
      }
   }
#pragma unroll
   for (int c = 0; c < 3; c++)
#pragma unroll
      for (int a = 0; a < N; a++) atomicAdd(&y[g[a] + (int64_t)nnodes * c], Y[c][a]);
}


}  // namespace

// element records of the p = 1 action (p = 2 streams the point records of exa_grad_setup: nothing to do)
int exa_launch_tet_setup(exa_ctx* ctx, double dt, const double* J, const double* C, hipStream_t s) {
   if (ctx->geom != EXA_GEOM_TET) { ctx->err = "tetrahedron set-up on a hexahedron context"; return EXA_ERR_STATE; }
   if (ctx->p != 1) return EXA_OK;
   const size_t bytes = (size_t)exa_nblocks(ctx) * TET_PAIRS * 2 * PA_BLK * sizeof(double);
   if (!ctx->tet_rec) { EXA_HIP_CHECK(ctx, hipMalloc(&ctx->tet_rec, bytes)); EXA_HIP_CHECK(ctx, hipMemsetAsync(ctx->tet_rec, 0, bytes, s)); }
   exa_dispatch([&](auto qb, auto trd) { hipLaunchKernelGGL((k_tet_setup_p1<qb.value, trd.value>), dim3(exa_nblocks(ctx)), dim3(PA_BLK), 0, s, ctx->E, dt, ctx->W_dev, J, C, ctx->tet_rec); },
                ctx->qblk, ctx->cfg.assembly == EXA_ASSEMBLY_EA);
   return exa_launched(ctx);
}

// driver-internal: whether exa_grad_setup builds the element records of the fused p = 1 action (off: the action is not going to run - table-driven
// route, EXA_TET_ACTION=generic - and a later exa_grad_apply_lvec builds them itself)
int exa_tet_set_fused_action(exa_ctx* ctx, int on) {
   if (!ctx) return EXA_ERR_ARG;
   ctx->tet_fused = on != 0; return EXA_OK;
}

// fused L-vector action (atomic scatter); mask: essential dofs of x read as zero; gate: device flag, non-zero = no-op.
// p = 1 with nodal coordinates registered (exa_grad_set_coords): J^-1 recomputed from them (GEO)
int exa_launch_tet_apply(exa_ctx* ctx, const double* x, double* y, const uint8_t* mask, const double* gate, hipStream_t s) {
   if (ctx->geom != EXA_GEOM_TET) { ctx->err = "tetrahedron action on a hexahedron context"; return EXA_ERR_STATE; }
   const unsigned nb = exa_nblocks(ctx);
   if (nb == 0) return EXA_OK;
   if (ctx->p == 1) {
      // (records the set-up did not build; never inside the driver's captured PCG chunk, whose set-up builds them)
      if (int rc = exa_build_pending(ctx, ctx->tet_pending, exa_launch_tet_setup, s)) return rc;
      if (!ctx->tet_rec) { ctx->err = "tetrahedron action: no element records (exa_grad_setup)"; return EXA_ERR_STATE; }
      const bool geo = ctx->coords_lvec != nullptr;
      exa_dispatch([&](auto nt, auto g) { hipLaunchKernelGGL((k_tet_apply_p1<nt.value, g.value>), dim3(nb), dim3(PA_BLK), 0, s, ctx->E, ctx->tet_rec, x, y, ctx->conn, ctx->nnodes, mask, gate, ctx->coords_lvec); },
                   exa_stream_nt((size_t)nb * PA_BLK * (geo ? 18 : TET_PAIRS) * 16), geo);
   } else {
      if (ctx->n != 10 || ctx->Q != 14) { ctx->err = "tetrahedron action: p = 1 or 2"; return EXA_ERR_UNSUPPORTED; }
      exa_dispatch([&](auto tr, auto nt) { hipLaunchKernelGGL((k_tet_apply_p2<tr.value, nt.value>), dim3(nb), dim3(PA_BLK), 0, s, ctx->E, ctx->pa, ctx->G_dev, x, y, ctx->conn, ctx->nnodes, mask, gate); },
                   ctx->cfg.assembly == EXA_ASSEMBLY_EA, exa_stream_nt((size_t)ctx->P * PA_PAIRS * 16));
   }
   return exa_launched(ctx);
}
