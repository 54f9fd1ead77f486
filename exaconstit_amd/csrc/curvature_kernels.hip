// Intragranular misorientation and lattice curvature (gfx950): GROD, KAM, the curvature kappa = d omega / d x of the rotation
// vector about the grain mean and the norm of the Nye tensor, from the per-element rows of exa_element_fields (include/exaconstit_hip.h).
//   launch 1 (elements): omega_e = rotation vector of s q_e (x) conj(qbar_g) (sample frame, sign-folded) -> record (omega (3), V, g) per element
//   launch 2 (nodes):    per node the 9 sums over the elements that hold it as a vertex: V omega (3), V, count, and the sums and sums of
//                        squares of the two 16-bit halves of the grain ids - integers, so that "all holders carry one id" is decided exactly
//                        after any further summation over ranks and periodic images (count * sum g^2 == (sum g)^2 for both halves)
//   launch 3 (elements): vertex values Omega_a = sum V omega / sum V (the element's own omega_e at a mixed node) -> kappa at the centroid through
//                        the trilinear / linear vertex functions on the current vertex coordinates, alpha_ij = kappa_ji - delta_ij kappa_kk,
//                        KAM = mean |Omega_a - omega_e| over the unmixed vertices -> rows [E][EXA_NCURV]
//   launch 4 + 5 (summary): sum V, sum V GROD, sum V KAM, sum V GND and the three maxima: the two-launch summary of analysis_device.hpp
// Design.  None of the launches is compute-bound; what matters is how the bytes move (staging, write-out and summary: analysis_device.hpp):
//   1: the rows are 296 bytes each and 5 of their 37 doubles are needed (volume, orientation).  A block of 64 lanes stages the leading 31 columns of
//      its 64 rows through LDS with wave-wide loads (stage_rows, dense: every load instruction reads 512 bytes that are contiguous row by
//      row); the records go back through the same LDS (store_tile) as one contiguous run of 64 x 5 doubles.
//   2: one lane per node walks the context's node -> (element, local node) table in its stored order (ascending element): a gather of 40-byte
//      records that neighbouring nodes share (L2), planar stores.  No atomics, a fixed order of every sum.
//   3: lane = element gathers 9 nodal values and 3 coordinates per vertex (the nodal planes are shared by the 8 elements of a node and stay in
//      L2; the coordinates are the element's own 3 n doubles of the E-vector), and the 16 results go out through an LDS tile (rows padded to 17)
//      as one contiguous run of 64 x 16 doubles.
//   4: lane = element reads V of its field row and 3 of the 16 doubles of its result row (one 128-byte line).
// Every launch gives the same bits on every call.
#include "analysis_device.hpp"
#include <cmath>

int exa_det_prepare(exa_ctx* ctx);   // capi.hip: builds the node -> element table on first use

using namespace exa_analysis;

namespace {

constexpr int NF = EXA_NFIELDS, NCV = EXA_NCURV;
constexpr int CH = 64;                               // elements per block of the two element launches
constexpr int NC1 = EXA_F_ORIENTATION + 4;           // launch 1 stages columns 0 .. 30 (volume .. orientation)
constexpr int REC = 5;                               // record: omega (3), V, grain id (as a double: exact for any int32)
constexpr int NPL = 9;                               // nodal planes: three nodal 3-vectors
constexpr int LDO = NCV + 1;                         // padded row of the output tile in LDS
constexpr int S_THREADS = 256, S_WAVES = S_THREADS / 64, S_MAX_BLOCKS = 960;

__global__ __launch_bounds__(CH) void k_curv_rotvec(const int64_t E, const double* __restrict__ F, const int32_t* __restrict__ grain, const int G,
                                                    const double* __restrict__ qbar, double* __restrict__ rec) {
   __shared__ double sm[NC1 * CH];
   const BlockView bv(E);
   const int lane = bv.lane, nv = bv.nv;
   const int64_t base = bv.base;
   const int32_t g = lane < nv ? grain[base + lane] : 0;
   double qr[4] = { 1.0, 0.0, 0.0, 0.0 };            // an id outside 1 .. G reads no mean: the identity stands in
   if (g >= 1 && g <= G) for (int k = 0; k < 4; k++) qr[k] = qbar[4 * (int64_t)(g - 1) + k];
   stage_rows<NC1, NC1>(sm, nv, lane, F, [&](int r) { return (base + r) * NF; }, IdentityCol());
   __syncthreads();
   double v[REC] = { 0.0, 0.0, 0.0, 0.0, 0.0 };
   if (lane < nv) {
      const double* f = sm + lane * NC1;
      const double q0 = f[EXA_F_ORIENTATION], q1 = f[EXA_F_ORIENTATION + 1], q2 = f[EXA_F_ORIENTATION + 2], q3 = f[EXA_F_ORIENTATION + 3];
      // d = q (x) conj(qbar): d_0 = q . qbar, d_vec = qbar_0 q_v - q_0 qbar_v - q_v x qbar_v
      double d0 = q0 * qr[0] + q1 * qr[1] + q2 * qr[2] + q3 * qr[3];
      double d1 = qr[0] * q1 - q0 * qr[1] - (q2 * qr[3] - q3 * qr[2]);
      double d2 = qr[0] * q2 - q0 * qr[2] - (q3 * qr[1] - q1 * qr[3]);
      double d3 = qr[0] * q3 - q0 * qr[3] - (q1 * qr[2] - q2 * qr[1]);
      if (d0 < 0.0) { d0 = -d0; d1 = -d1; d2 = -d2; d3 = -d3; }
      const double nrm = sqrt(d1 * d1 + d2 * d2 + d3 * d3);
      const double sc = nrm > 0.0 ? 2.0 * atan2(nrm, d0) / nrm : 0.0;
      v[0] = sc * d1; v[1] = sc * d2; v[2] = sc * d3; v[3] = f[EXA_F_VOLUME]; v[4] = (double)g;
   }
   __syncthreads();   // every lane has read its staged row before the record tile overwrites the staging area
   if (lane < nv) {
#pragma unroll
      for (int k = 0; k < REC; k++) sm[lane * REC + k] = v[k];
   }
   __syncthreads();
   store_tile<REC, REC>(rec, base, sm, nv, lane);
}

__global__ __launch_bounds__(256) void k_curv_nodal(const int n, const int nvert, const int nnodes, const int32_t* __restrict__ off,
                                                    const int32_t* __restrict__ idx, const double* __restrict__ rec, double* __restrict__ out) {
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= nnodes) return;
   double s[NPL];
#pragma unroll
   for (int p = 0; p < NPL; p++) s[p] = 0.0;
   for (int k = off[i]; k < off[i + 1]; k++) {
      const int code = idx[k]; const int64_t e = code / n; const int a = code - (int)e * n;
      if (a >= nvert) continue;   // a high-order node of this element
      const double* r = rec + e * REC;
      const double V = r[3];
      const uint32_t g = (uint32_t)(int32_t)r[4];
      const double lo = (double)(g & 0xffffu), hi = (double)(g >> 16);
      s[0] += V * r[0]; s[1] += V * r[1]; s[2] += V * r[2];
      s[3] += V; s[4] += 1.0; s[5] += lo;
      s[6] += lo * lo; s[7] += hi; s[8] += hi * hi;
   }
#pragma unroll
   for (int p = 0; p < NPL; p++) out[(int64_t)p * nnodes + i] = s[p];
}

// NV = 8: hexahedron, vertices in the order (0,0,0) (1,0,0) (1,1,0) (0,1,0) (0,0,1) (1,0,1) (1,1,1) (0,1,1); NV = 4: tetrahedron (0,0,0) (1,0,0) (0,1,0) (0,0,1)
template <int NV>
__global__ __launch_bounds__(CH) void k_curv_elements(const int64_t E, const int n, const int nnodes, const int32_t* __restrict__ conn,
                                                      const double* __restrict__ rec, const double* __restrict__ nodal, const double* __restrict__ xe,
                                                      const double inv_b, double* __restrict__ out) {
   __shared__ double sm[CH * LDO];
   const BlockView bv(E);
   const int lane = bv.lane, nv = bv.nv;
   const int64_t base = bv.base, e = base + lane;
   if (lane < nv) {
      const double* r = rec + e * REC;
      const double w[3] = { r[0], r[1], r[2] };
      double W[3][3] = { { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } }, J[3][3] = { { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } };
      double kam = 0.0; int nun = 0;
#pragma unroll
      for (int a = 0; a < NV; a++) {
         const int64_t nd = conn[a + (int64_t)n * e];
         double t[NPL];
#pragma unroll
         for (int p = 0; p < NPL; p++) t[p] = nodal[(int64_t)p * nnodes + nd];
         const uint64_t c = (uint64_t)t[4], sl = (uint64_t)t[5], sl2 = (uint64_t)t[6], sh = (uint64_t)t[7], sh2 = (uint64_t)t[8];
         const bool mixed = c * sl2 != sl * sl || c * sh2 != sh * sh;
         const double iv = 1.0 / t[3];
         double wt[3] = { t[0] * iv, t[1] * iv, t[2] * iv };
         if (mixed) { wt[0] = w[0]; wt[1] = w[1]; wt[2] = w[2]; }
         else {
            const double a0 = wt[0] - w[0], a1 = wt[1] - w[1], a2 = wt[2] - w[2];
            kam += sqrt(a0 * a0 + a1 * a1 + a2 * a2); nun++;
         }
         double d[3];   // d N_a / d xi at the centroid
         if (NV == 8) {
            d[0] = ((a ^ (a >> 1)) & 1) ? 0.25 : -0.25; d[1] = (a & 2) ? 0.25 : -0.25; d[2] = (a & 4) ? 0.25 : -0.25;
         } else {
            d[0] = a == 0 ? -1.0 : (a == 1 ? 1.0 : 0.0); d[1] = a == 0 ? -1.0 : (a == 2 ? 1.0 : 0.0); d[2] = a == 0 ? -1.0 : (a == 3 ? 1.0 : 0.0);
         }
#pragma unroll
         for (int i = 0; i < 3; i++) {
            const double x = xe[a + (int64_t)n * (i + 3 * e)];
#pragma unroll
            for (int k = 0; k < 3; k++) { W[i][k] += wt[i] * d[k]; J[i][k] += x * d[k]; }
         }
      }
      // J^-1 = adj(J) / det J, kappa = W J^-1
      double A[3][3];
      A[0][0] = J[1][1] * J[2][2] - J[1][2] * J[2][1]; A[0][1] = J[0][2] * J[2][1] - J[0][1] * J[2][2]; A[0][2] = J[0][1] * J[1][2] - J[0][2] * J[1][1];
      A[1][0] = J[1][2] * J[2][0] - J[1][0] * J[2][2]; A[1][1] = J[0][0] * J[2][2] - J[0][2] * J[2][0]; A[1][2] = J[0][2] * J[1][0] - J[0][0] * J[1][2];
      A[2][0] = J[1][0] * J[2][1] - J[1][1] * J[2][0]; A[2][1] = J[0][1] * J[2][0] - J[0][0] * J[2][1]; A[2][2] = J[0][0] * J[1][1] - J[0][1] * J[1][0];
      const double idet = 1.0 / (J[0][0] * A[0][0] + J[0][1] * A[1][0] + J[0][2] * A[2][0]);
      double kp[3][3];
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
         for (int j = 0; j < 3; j++) kp[i][j] = (W[i][0] * A[0][j] + W[i][1] * A[1][j] + W[i][2] * A[2][j]) * idet;
      const double tr = kp[0][0] + kp[1][1] + kp[2][2];
      double nye2 = 0.0;
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
         for (int j = 0; j < 3; j++) { const double al = kp[j][i] - (i == j ? tr : 0.0); nye2 += al * al; }
      const double nye = sqrt(nye2);
      double* o = sm + lane * LDO;
      o[EXA_C_ROTVEC] = w[0]; o[EXA_C_ROTVEC + 1] = w[1]; o[EXA_C_ROTVEC + 2] = w[2];
      o[EXA_C_GROD] = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]) * RAD2DEG;
      o[EXA_C_KAM] = nun > 0 ? kam / nun * RAD2DEG : 0.0;
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
         for (int j = 0; j < 3; j++) o[EXA_C_CURVATURE + 3 * i + j] = kp[i][j];
      o[EXA_C_NYENORM] = nye; o[EXA_C_GND] = nye * inv_b;
   }
   __syncthreads();
   store_tile<NCV, LDO>(out, base, sm, nv, lane);
}

// sum V, sum V GROD, sum V KAM, sum V GND | max GROD, max KAM, max GND.  The three are >= 0: 0 is the neutral element of the maxima
struct CurvSummary {
   static constexpr int N = 7;
   static __device__ __forceinline__ void init(double* v) {
#pragma unroll
      for (int k = 0; k < N; k++) v[k] = 0.0;
   }
   static __device__ __forceinline__ void merge(double* v, const double* y) {
#pragma unroll
      for (int k = 0; k < 4; k++) v[k] += y[k];
#pragma unroll
      for (int k = 4; k < N; k++) v[k] = fmax(v[k], y[k]);
   }
};
constexpr int NSUM = CurvSummary::N;

__global__ __launch_bounds__(S_THREADS) void k_curv_partial(const int64_t E, const double* __restrict__ F, const double* __restrict__ C, double* __restrict__ partial) {
   __shared__ double sm[S_WAVES][NSUM];
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   double acc[NSUM];
   CurvSummary::init(acc);
   const int64_t nblk = (E + 63) / 64, stride = (int64_t)gridDim.x * S_WAVES;
   for (int64_t b = (int64_t)blockIdx.x * S_WAVES + wave; b < nblk; b += stride) {
      const int64_t e = b * 64 + lane;
      if (e >= E) continue;
      const double V = F[e * NF + EXA_F_VOLUME];
      const double* c = C + e * NCV;
      const double gr = c[EXA_C_GROD], ka = c[EXA_C_KAM], gn = c[EXA_C_GND];
      acc[0] += V; acc[1] += V * gr; acc[2] += V * ka; acc[3] += V * gn;
      acc[4] = fmax(acc[4], gr); acc[5] = fmax(acc[5], ka); acc[6] = fmax(acc[6], gn);
   }
   summary_block_partial<CurvSummary>(acc, sm, partial);
}

__global__ __launch_bounds__(64) void k_curv_reduce(const int nb, const double* __restrict__ partial, double* __restrict__ out) {
   summary_reduce<CurvSummary>(nb, partial, out);
}

int check_common(exa_ctx* ctx, const char* who, bool ok) {
   if (!ok) { ctx->err = std::string(who) + ": a required pointer is NULL"; return EXA_ERR_ARG; }
   if (!ctx->conn) { ctx->err = std::string(who) + ": call exa_set_connectivity first"; return EXA_ERR_STATE; }
   return EXA_OK;
}

}  // namespace

extern "C" int exa_curvature_sizes(int64_t E, int64_t* work_doubles, int* nodal_planes) {
   if (E < 0) return EXA_ERR_ARG;
   if (work_doubles) *work_doubles = (int64_t)REC * E;
   if (nodal_planes) *nodal_planes = NPL;
   return EXA_OK;
}

extern "C" int exa_curvature_nodal(exa_ctx* ctx, const double* fields_dev, const int32_t* grain_of_elem_dev, int G, const double* qbar_dev, double* work_dev,
                                   double* nodal_dev, exa_stream str) {
   if (!ctx) return EXA_ERR_ARG;
   if (int rc = check_common(ctx, "exa_curvature_nodal", nodal_dev && (ctx->E == 0 || (fields_dev && grain_of_elem_dev && qbar_dev && work_dev)))) return rc;
   if (G < 1) { ctx->err = "exa_curvature_nodal: G >= 1 is required"; return EXA_ERR_ARG; }
   hipStream_t s = reinterpret_cast<hipStream_t>(str);
   if (ctx->E == 0) { EXA_HIP_CHECK(ctx, hipMemsetAsync(nodal_dev, 0, sizeof(double) * NPL * (size_t)ctx->nnodes, s)); return EXA_OK; }
   if (int rc = exa_det_prepare(ctx)) return rc;
   const int nvert = exa_is_hex(ctx) ? 8 : 4;
   hipLaunchKernelGGL(k_curv_rotvec, dim3((unsigned)(((int64_t)ctx->E + CH - 1) / CH)), dim3(CH), 0, s, (int64_t)ctx->E, fields_dev, grain_of_elem_dev, G, qbar_dev, work_dev);
   hipLaunchKernelGGL(k_curv_nodal, dim3((unsigned)((ctx->nnodes + 255) / 256)), dim3(256), 0, s, ctx->n, nvert, ctx->nnodes, (const int32_t*)ctx->n2e_off,
                      (const int32_t*)ctx->n2e_idx, (const double*)work_dev, nodal_dev);
   EXA_HIP_CHECK(ctx, hipGetLastError());
   return EXA_OK;
}

extern "C" int exa_curvature_elements(exa_ctx* ctx, const double* fields_dev, const int32_t* grain_of_elem_dev, int G, const double* qbar_dev, const double* work_dev,
                                      const double* nodal_dev, const double* xe_dev, double burgers, double* out_dev, exa_stream str) {
   if (!ctx) return EXA_ERR_ARG;
   if (int rc = check_common(ctx, "exa_curvature_elements", ctx->E == 0 || (fields_dev && grain_of_elem_dev && qbar_dev && work_dev && nodal_dev && xe_dev && out_dev))) return rc;
   if (G < 1 || !(burgers > 0.0) || !std::isfinite(burgers)) { ctx->err = "exa_curvature_elements: G >= 1 and a finite Burgers vector length > 0 are required"; return EXA_ERR_ARG; }
   if (ctx->E == 0) return EXA_OK;
   hipStream_t s = reinterpret_cast<hipStream_t>(str);
   const dim3 grid((unsigned)(((int64_t)ctx->E + CH - 1) / CH));
   if (exa_is_hex(ctx)) hipLaunchKernelGGL(k_curv_elements<8>, grid, dim3(CH), 0, s, (int64_t)ctx->E, ctx->n, ctx->nnodes, ctx->conn, work_dev, nodal_dev, xe_dev, 1.0 / burgers, out_dev);
   else hipLaunchKernelGGL(k_curv_elements<4>, grid, dim3(CH), 0, s, (int64_t)ctx->E, ctx->n, ctx->nnodes, ctx->conn, work_dev, nodal_dev, xe_dev, 1.0 / burgers, out_dev);
   EXA_HIP_CHECK(ctx, hipGetLastError());
   return EXA_OK;
}

extern "C" int exa_curvature_summary(exa_ctx* ctx, const double* fields_dev, const double* curv_dev, double* out_dev, exa_stream str) {
   if (!ctx) return EXA_ERR_ARG;
   if (!out_dev || (ctx->E > 0 && (!fields_dev || !curv_dev))) { ctx->err = "exa_curvature_summary: fields, curvature rows and an output are required"; return EXA_ERR_ARG; }
   hipStream_t s = reinterpret_cast<hipStream_t>(str);
   if (ctx->E == 0) { EXA_HIP_CHECK(ctx, hipMemsetAsync(out_dev, 0, sizeof(double) * NSUM, s)); return EXA_OK; }
   int nb;
   if (int rc = summary_grid(ctx, "exa_curvature_summary", S_THREADS, S_MAX_BLOCKS, NSUM, &nb)) return rc;
   hipLaunchKernelGGL(k_curv_partial, dim3(nb), dim3(S_THREADS), 0, s, (int64_t)ctx->E, fields_dev, curv_dev, ctx->scratch_dev);
   hipLaunchKernelGGL(k_curv_reduce, dim3(1), dim3(64), 0, s, nb, (const double*)ctx->scratch_dev, out_dev);
   EXA_HIP_CHECK(ctx, hipGetLastError());
   return EXA_OK;
}
