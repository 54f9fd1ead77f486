// Per-element output fields (gfx950): the element averages of the quadrature state behind the reference's SystemDriver::Project* calls
//   CalcElementAvg / ProjectModelStress / ProjectVolume       reference src/system_driver.cpp:560-640
//   ProjectCentroid, ProjectVonMisesStress, ProjectHydroStress, ProjectDpEff, ProjectEffPlasticStrain, ProjectShearRate, ProjectH,
//   ProjectOrientation, ProjectElasticStrains                 reference src/system_driver.cpp:640-870
// One launch writes the EXA_NFIELDS columns of every element (include/exaconstit_hip.h).  Design (HBM-bound, one wave per 64-element block,
// lane = element): every point value is read once and summed into per-lane registers in a fixed order (q ascending), so the result has the
// same bits from run to run without atomics.  Element-blocked quadrature functions are read directly (each (q, component) access of a wave is one
// contiguous 512-byte row); AOS ones are staged per point index q through LDS (the 64 rows of q are 64 contiguous 224 / 48 / 72-byte segments).
// The [E][EXA_NFIELDS] rows leave through LDS as contiguous wave stores.  At p = 1 the 24 node coordinates the centroid needs are staged
// through LDS as well and det J is recomputed from them when no Jacobian field is given (72 B per point less traffic).
#include "exa_internal.hpp"
#include <cmath>

namespace {

constexpr int NF = EXA_NFIELDS;
constexpr int SV = 28;            // state variables per point (include/exaconstit_hip.h, "State layout")
constexpr int XPAD = 25;          // LDS row of a staged element: 24 node coordinates (p = 1) + 1
constexpr int SPAD = SV + 1;      // ... 28 state values (AOS) + 1
constexpr int LDS_DOUBLES = 64 * NF;
static_assert(64 * SPAD <= LDS_DOUBLES && 64 * XPAD <= LDS_DOUBLES && 64 * 16 <= LDS_DOUBLES, "LDS staging buffer too small");

// one-dimensional nodal basis of order p at the p + 1 Gauss points and the lexicographic -> native node map, passed by value (kernel arguments):
// N_a(xi_q) = B[qx][i] B[qy][j] B[qz][k] with a = nat[i + np (j + np k)]
struct Basis1D {
   double B[7 * 7];
   int16_t nat[343];
};

// p = 1 reference hexahedron (vertex order of the native numbering = VTK_HEXAHEDRON), quadrature point q = x + 2 y + 4 z
constexpr double GL0 = 0.21132486540518713, GL1 = 0.78867513459481287;
constexpr double gl_pt(int i) { return i == 0 ? GL0 : GL1; }
constexpr int VX[8] = { 0, 1, 1, 0, 0, 1, 1, 0 }, VY[8] = { 0, 0, 1, 1, 0, 0, 1, 1 }, VZ[8] = { 0, 0, 0, 0, 1, 1, 1, 1 };
constexpr double n1(int v, double x) { return v ? x : 1.0 - x; }
constexpr double d1(int v) { return v ? 1.0 : -1.0; }
constexpr double N1(int a, int q) { return n1(VX[a], gl_pt(q & 1)) * n1(VY[a], gl_pt((q >> 1) & 1)) * n1(VZ[a], gl_pt((q >> 2) & 1)); }
constexpr double G1(int a, int j, int q) {
   const double x = gl_pt(q & 1), y = gl_pt((q >> 1) & 1), z = gl_pt((q >> 2) & 1);
   return j == 0 ? d1(VX[a]) * n1(VY[a], y) * n1(VZ[a], z) : (j == 1 ? n1(VX[a], x) * d1(VY[a]) * n1(VZ[a], z) : n1(VX[a], x) * n1(VY[a], y) * d1(VZ[a]));
}

// det of J(i,j) = dx_i/dxi_j stored column-major at stride st (the cofactor expansion of adj_det, pa_kernels.hip)
__device__ __forceinline__ double det3(const double* Jq, const int st) {
   const double J11 = Jq[0], J21 = Jq[st], J31 = Jq[2 * st], J12 = Jq[3 * st], J22 = Jq[4 * st], J32 = Jq[5 * st], J13 = Jq[6 * st], J23 = Jq[7 * st], J33 = Jq[8 * st];
   return J11 * (J22 * J33 - J23 * J32) + J21 * (J32 * J13 - J12 * J33) + J31 * (J12 * J23 - J22 * J13);
}

// the state slots that are averaged, in accumulator order: 0, 1 (DpEff, EffPlasticStrain), 4..8 (elastic strain), 9..12 (orientation),
// 13 (hardness), 14..25 (slip rates), 26 (relative volume) -> accumulator k = slot for slot <= 1, slot - 2 above (slots 2, 3, 27 are not read)
constexpr int NACC = 25;
__device__ __forceinline__ constexpr int acc_slot(int k) { return k < 2 ? k : k + 2; }

// TET: straight-sided tetrahedra: volume = sum_q W_q detJ from the Jacobian field, centroid = mean of the four vertices
template <bool QB, bool P1, bool HAVE_J, bool TET = false>
__global__ __launch_bounds__(64) void k_element_fields(const int64_t E, const int Q, const int n, const int np, const double* __restrict__ W,
                                                       const double* __restrict__ J, const double* __restrict__ S, const double* __restrict__ X,
                                                       const double* __restrict__ xe, double* __restrict__ out, const Basis1D basis) {
   __shared__ double sh[LDS_DOUBLES];
   const int t = threadIdx.x;
   const int64_t e0 = (int64_t)blockIdx.x * 64, e = e0 + t;
   const int nvalid = (int)((E - e0) < 64 ? (E - e0) : 64);
   const bool live = t < nvalid;
   // p = 1: the block's 64 x 24 node coordinates are one contiguous E-vector segment
   double x8[P1 ? 24 : 1];
   if constexpr (P1) {
      for (int i = t; i < 24 * nvalid; i += 64) sh[(i / 24) * XPAD + i % 24] = xe[24 * e0 + i];
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 24; i++) x8[i] = live ? sh[t * XPAD + i] : 0.0;
      __syncthreads();
   }
   double vol = 0.0, cx = 0.0, cy = 0.0, cz = 0.0, s[6] = { 0, 0, 0, 0, 0, 0 }, a[NACC];
#pragma unroll
   for (int k = 0; k < NACC; k++) a[k] = 0.0;
   // (p = 1: eight points, unrolled, so that the shape values and derivatives above are constants)
   constexpr int QUNROLL = P1 ? 8 : 1;
#pragma unroll QUNROLL
   for (int q = 0; q < (P1 ? 8 : Q); q++) {
      // ---- AOS: rows of point q of the block's elements staged through LDS (state first, then stress + Jacobian)
      if constexpr (!QB) {
         for (int i = t; i < SV * nvalid; i += 64) { const int r = i / SV, c = i - r * SV; sh[r * SPAD + c] = X[((e0 + r) * Q + q) * SV + c]; }
         __syncthreads();
      }
      double w = 0.0, xq[3] = { 0, 0, 0 };
      double sv[NACC];
      if (live) {
         const QView vs = qview<QB>(SV, Q, e, q);
         if constexpr (QB) {
#pragma unroll
            for (int k = 0; k < NACC; k++) sv[k] = X[vs.base + (int64_t)acc_slot(k) * vs.stride];
         } else {
#pragma unroll
            for (int k = 0; k < NACC; k++) sv[k] = sh[t * SPAD + acc_slot(k)];
         }
      }
      if constexpr (!QB) {
         __syncthreads();
         const int NR = HAVE_J ? 15 : 6;   // stress (6) + Jacobian (9) of point q per element
         for (int i = t; i < NR * nvalid; i += 64) {
            const int r = i / NR, c = i - r * NR;
            sh[r * 16 + c] = c < 6 ? S[((e0 + r) * Q + q) * 6 + c] : J[((e0 + r) * Q + q) * 9 + (c - 6)];
         }
         __syncthreads();
      }
      if (live) {
         double sq[6];
         double detJ;
         const QView vq = qview<QB>(6, Q, e, q);
         if constexpr (QB) {
#pragma unroll
            for (int k = 0; k < 6; k++) sq[k] = S[vq.base + (int64_t)k * vq.stride];
         } else {
#pragma unroll
            for (int k = 0; k < 6; k++) sq[k] = sh[t * 16 + k];
         }
         if constexpr (HAVE_J) {
            if constexpr (QB) { const QView vj = qview<QB>(9, Q, e, q); detJ = det3(J + vj.base, vj.stride); }
            else detJ = det3(sh + t * 16 + 6, 1);
         }
         if constexpr (P1) {
            double Jl[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
#pragma unroll
            for (int b = 0; b < 8; b++) {
               const double x0 = x8[b], x1 = x8[b + 8], x2 = x8[b + 16], nb = N1(b, q);
               xq[0] += nb * x0; xq[1] += nb * x1; xq[2] += nb * x2;
               if constexpr (!HAVE_J) {
                  const double g0 = G1(b, 0, q), g1 = G1(b, 1, q), g2 = G1(b, 2, q);
                  Jl[0] += x0 * g0; Jl[1] += x1 * g0; Jl[2] += x2 * g0;
                  Jl[3] += x0 * g1; Jl[4] += x1 * g1; Jl[5] += x2 * g1;
                  Jl[6] += x0 * g2; Jl[7] += x1 * g2; Jl[8] += x2 * g2;
               }
            }
            if constexpr (!HAVE_J) detJ = det3(Jl, 1);
         } else if constexpr (!TET) {
            // x(xi_q) = sum_a N_a(xi_q) x_a, lexicographic node walk
            const int qx = q % np, qy = (q / np) % np, qz = q / (np * np);
            const double* xel = xe + (int64_t)3 * n * e;
            int lex = 0;
            for (int k = 0; k < np; k++)
               for (int j = 0; j < np; j++) {
                  const double byz = basis.B[qy * np + j] * basis.B[qz * np + k];
                  for (int i = 0; i < np; i++, lex++) {
                     const int nd = basis.nat[lex];
                     const double nb = basis.B[qx * np + i] * byz;
                     xq[0] += nb * xel[nd]; xq[1] += nb * xel[nd + n]; xq[2] += nb * xel[nd + 2 * n];
                  }
               }
         }
         w = W[q] * detJ;
         vol += w; cx += w * xq[0]; cy += w * xq[1]; cz += w * xq[2];
#pragma unroll
         for (int k = 0; k < 6; k++) s[k] += w * sq[k];
#pragma unroll
         for (int k = 0; k < NACC; k++) a[k] += w * sv[k];
      }
      if constexpr (!QB) __syncthreads();
   }
   // ---- element values (reference src/system_driver.cpp:560-870)
   if (live) {
      const double iv = 1.0 / vol;
      double* o = sh + t * NF;
      o[EXA_F_VOLUME] = vol;
      o[EXA_F_CENTROID] = cx * iv; o[EXA_F_CENTROID + 1] = cy * iv; o[EXA_F_CENTROID + 2] = cz * iv;
      if constexpr (TET) {
         const double* xel = xe + (int64_t)3 * n * e;
#pragma unroll
         for (int d = 0; d < 3; d++) o[EXA_F_CENTROID + d] = 0.25 * (xel[n * d] + xel[1 + n * d] + xel[2 + n * d] + xel[3 + n * d]);
      }
#pragma unroll
      for (int k = 0; k < 6; k++) s[k] *= iv;
#pragma unroll
      for (int k = 0; k < 6; k++) o[EXA_F_STRESS + k] = s[k];
      const double d01 = s[0] - s[1], d12 = s[1] - s[2], d20 = s[2] - s[0];
      o[EXA_F_VONMISES] = sqrt(0.5 * (d01 * d01 + d12 * d12 + d20 * d20 + 6.0 * (s[3] * s[3] + s[4] * s[4] + s[5] * s[5])));
      o[EXA_F_HYDROSTATIC] = (s[0] + s[1] + s[2]) * (1.0 / 3.0);
#pragma unroll
      for (int k = 0; k < NACC; k++) a[k] *= iv;
      o[EXA_F_DPEFF] = a[0];              // slot 0
      o[EXA_F_EFFPLASTICSTRAIN] = a[1];   // slot 1
      o[EXA_F_HARDNESS] = a[11];          // slot 13
#pragma unroll
      for (int k = 0; k < 12; k++) o[EXA_F_SHEARRATE + k] = a[12 + k];   // slots 14..25
      const double qn = 1.0 / sqrt(a[7] * a[7] + a[8] * a[8] + a[9] * a[9] + a[10] * a[10]);   // slots 9..12
#pragma unroll
      for (int k = 0; k < 4; k++) o[EXA_F_ORIENTATION + k] = a[7 + k] * qn;
      // ProjectElasticStrains: deviatoric 5-vector (slots 4..8) + volumetric part ln(rel_vol) (slot 26) -> Voigt (11,22,33,23,13,12)
      const double t1 = C_SQR2I * a[2], t2 = C_SQR6I * a[3], v = log(a[24]);
      o[EXA_F_XTALELASTICSTRAIN + 0] = t1 - t2 + v;
      o[EXA_F_XTALELASTICSTRAIN + 1] = -t1 - t2 + v;
      o[EXA_F_XTALELASTICSTRAIN + 2] = 0.81649658092772603273 * a[3] + v;   // sqrt(2/3)
      o[EXA_F_XTALELASTICSTRAIN + 3] = C_SQR2I * a[6];
      o[EXA_F_XTALELASTICSTRAIN + 4] = C_SQR2I * a[5];
      o[EXA_F_XTALELASTICSTRAIN + 5] = C_SQR2I * a[4];
   }
   __syncthreads();
   // the block's rows are one contiguous segment of out
   double* ob = out + e0 * NF;
   for (int i = t; i < NF * nvalid; i += 64) ob[i] = sh[i];
}

template <bool QB, bool P1, bool HAVE_J, bool TET = false>
void launch(const exa_ctx* ctx, const double* J, const double* S, const double* X, const double* xe, double* out, const Basis1D& b, hipStream_t s) {
   const unsigned nb = (unsigned)((ctx->E + 63) / 64);
   hipLaunchKernelGGL((k_element_fields<QB, P1, HAVE_J, TET>), dim3(nb), dim3(64), 0, s, (int64_t)ctx->E, ctx->Q, ctx->n, ctx->p + 1, ctx->W_dev, J, S, X, xe, out, b);
}

}  // namespace

extern "C" int exa_element_fields(exa_ctx* ctx, const double* J, const double* S, const double* X, const double* xe, double* out, exa_stream str) {
   if (!ctx) return EXA_ERR_ARG;
   if (!S || !X || !xe || !out) { ctx->err = "exa_element_fields: stress, state, coordinates and output are required"; return EXA_ERR_ARG; }
   if (!J && (ctx->p != 1 || !exa_is_hex(ctx))) { ctx->err = "exa_element_fields: a Jacobian field is required at p > 1 and for tetrahedra (only the p = 1 hexahedron recomputes det J from the coordinates)"; return EXA_ERR_ARG; }
   if (ctx->nstatev != SV) { ctx->err = "exa_element_fields: the fields read a 28-variable state"; return EXA_ERR_UNSUPPORTED; }
   if (ctx->p < 1 || ctx->p > 6) { ctx->err = "exa_element_fields: order out of range"; return EXA_ERR_UNSUPPORTED; }
   if (ctx->E == 0) return EXA_OK;
   Basis1D b{};
   hipStream_t s = reinterpret_cast<hipStream_t>(str);
   if (!exa_is_hex(ctx)) {
      if (ctx->qblk) launch<true, false, true, true>(ctx, J, S, X, xe, out, b, s); else launch<false, false, true, true>(ctx, J, S, X, xe, out, b, s);
      EXA_HIP_CHECK(ctx, hipGetLastError());
      return EXA_OK;
   }
   if (ctx->p > 1) {
      std::vector<double> T1; std::vector<int> nat;
      exa_build_1d_tables(ctx->p, T1, nat);
      const int np = ctx->p + 1;
      for (int q = 0; q < np; q++) for (int i = 0; i < np; i++) b.B[q * np + i] = T1[2 * np * q + i];
      for (size_t i = 0; i < nat.size(); i++) b.nat[i] = (int16_t)nat[i];
   }
   const bool p1 = ctx->p == 1;
   if (ctx->qblk) {
      if (p1) { if (J) launch<true, true, true>(ctx, J, S, X, xe, out, b, s); else launch<true, true, false>(ctx, J, S, X, xe, out, b, s); }
      else launch<true, false, true>(ctx, J, S, X, xe, out, b, s);
   } else {
      if (p1) { if (J) launch<false, true, true>(ctx, J, S, X, xe, out, b, s); else launch<false, true, false>(ctx, J, S, X, xe, out, b, s); }
      else launch<false, false, true>(ctx, J, S, X, xe, out, b, s);
   }
   EXA_HIP_CHECK(ctx, hipGetLastError());
   return EXA_OK;
}
