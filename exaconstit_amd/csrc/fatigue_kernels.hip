// Slip-system activity and the Fatemi-Socie fatigue indicator parameter (gfx950) on the per-element rows of exa_element_fields
// (include/exaconstit_hip.h).  The accumulators persist across the steps of a run: 60 doubles per element, planar [EXA_NSLIPACC][E_pad] with
// E_pad = E rounded up to 64, planes Gamma (12) | A (12) | Gamma_min (12) | Gamma_max (12) | N_max (12).
//   launch 1 (every committed step): Gamma_a += dt g_a, A_a += dt |g_a|, window minimum / maximum of Gamma_a and maximum of the normal stress
//                        sigma_n,a = n_a^T sigma n_a on the slip plane, n_a = R(q) m_a; RESET: the window restarts from the values of this call
//   launch 2 (evaluation): planar accumulators -> rows [E][EXA_NFIP]
//   launch 3 + 4 (summary): sum V, sum V FIP, sum V AccumulatedSlip, the three maxima and the global id of the element of the largest FIP (ties: the
//                        smallest id): the two-launch summary of analysis_device.hpp
// Design.  Launch 1 is the hot path and moves bytes: per element one 296-byte row, of which 22 doubles are needed (stress, shear rates,
// orientation), and 480 bytes of accumulators read and written.
//   1: a block of 64 lanes stages the 22 columns of its 64 rows through LDS with wave-wide loads (stage_rows with the column map field_col: every
//      load instruction walks the rows contiguously, 48 + 128 bytes per row), rows padded to 23 in LDS (odd stride: lane = row reads hit distinct
//      banks).  Lane = element then reads and writes each accumulator plane at [plane][base + lane]: one 512-byte run per wave and instruction.  The 12 unit
//      plane normals arrive by value (kernel arguments: scalar registers under the unrolled system loop).  RESET reads 24 planes instead of 60.
//   2: lane = element reads its 60 planar values, the 6 results go out through an LDS tile (store_tile, rows padded to 7) as one contiguous
//      run of 64 x 6 doubles.
//   3: lane = element reads V of its field row and its 48-byte result row.
// No atomics, fixed summation orders: every launch gives the same bits on every call.
#include "analysis_device.hpp"
#include <cmath>
#include <limits>

using namespace exa_analysis;

namespace {

constexpr int NF = EXA_NFIELDS, NFP = EXA_NFIP, NS = 12;
constexpr int CH = 64;                               // elements per block of the two element launches
constexpr int NCOL = 6 + NS + 4;                     // staged columns: stress | shear rates | orientation
constexpr int LDR = NCOL + 1;                        // padded row of the staging tile
constexpr int C_SIG = 0, C_RATE = 6, C_Q = 6 + NS;   // their places in a staged row
constexpr int P_GAM = EXA_ACC_SLIP, P_ABS = EXA_ACC_ABS, P_MIN = EXA_ACC_MIN, P_MAX = EXA_ACC_MAX, P_NMX = EXA_ACC_NMAX;   // accumulator planes
constexpr int S_THREADS = 256, S_WAVES = S_THREADS / 64, S_MAX_BLOCKS = 960;

struct Normals { double m[NS][3]; };

__host__ __device__ constexpr int field_col(int c) { return c < 6 ? EXA_F_STRESS + c : (c < 6 + NS ? EXA_F_SHEARRATE + (c - 6) : EXA_F_ORIENTATION + (c - 6 - NS)); }

template <bool RESET>
__global__ __launch_bounds__(CH) void k_slip_accumulate(const int64_t E, const int64_t Epad, const double* __restrict__ F, const Normals nrm, const double dt,
                                                        double* __restrict__ acc) {
   __shared__ double sm[LDR * CH];
   const BlockView bv(E);
   const int lane = bv.lane, nv = bv.nv;
   const int64_t base = bv.base;
   stage_rows<NCOL, LDR>(sm, nv, lane, F, [&](int r) { return (base + r) * NF; }, [](int c) { return field_col(c); });
   __syncthreads();
   if (lane >= nv) return;   // lanes beyond E store nothing
   const double* f = sm + lane * LDR;
   const double q[4] = { f[C_Q], f[C_Q + 1], f[C_Q + 2], f[C_Q + 3] };
   double R[9]; ecmdev::quat_to_mat(q, R);
   const double s0 = f[C_SIG], s1 = f[C_SIG + 1], s2 = f[C_SIG + 2], s3 = f[C_SIG + 3], s4 = f[C_SIG + 4], s5 = f[C_SIG + 5];
   double* a0 = acc + base + lane;
#pragma unroll
   for (int a = 0; a < NS; a++) {
      const double m0 = nrm.m[a][0], m1 = nrm.m[a][1], m2 = nrm.m[a][2];
      const double n0 = R[0] * m0 + R[1] * m1 + R[2] * m2, n1 = R[3] * m0 + R[4] * m1 + R[5] * m2, n2 = R[6] * m0 + R[7] * m1 + R[8] * m2;
      const double sn = s0 * n0 * n0 + s1 * n1 * n1 + s2 * n2 * n2 + 2.0 * (s3 * n1 * n2 + s4 * n0 * n2 + s5 * n0 * n1);
      const double g = f[C_RATE + a];
      const double gam = a0[(P_GAM + a) * Epad] + dt * g;
      const double ab = a0[(P_ABS + a) * Epad] + dt * fabs(g);
      double lo = gam, hi = gam, nm = sn;
      if (!RESET) {
         lo = fmin(a0[(P_MIN + a) * Epad], gam); hi = fmax(a0[(P_MAX + a) * Epad], gam); nm = fmax(a0[(P_NMX + a) * Epad], sn);
      }
      a0[(P_GAM + a) * Epad] = gam; a0[(P_ABS + a) * Epad] = ab;
      a0[(P_MIN + a) * Epad] = lo; a0[(P_MAX + a) * Epad] = hi; a0[(P_NMX + a) * Epad] = nm;
   }
}

__global__ __launch_bounds__(CH) void k_fip_rows(const int64_t E, const int64_t Epad, const double* __restrict__ acc, const double k_over_sy, double* __restrict__ out) {
   __shared__ double sm[CH * (NFP + 1)];
   const BlockView bv(E);
   const int lane = bv.lane, nv = bv.nv;
   const int64_t base = bv.base;
   if (lane < nv) {
      const double* a0 = acc + base + lane;
      double best = 0.0, brange = 0.0, bn = 0.0, asum = 0.0, net = 0.0; int bsys = 0;
#pragma unroll
      for (int a = 0; a < NS; a++) {
         const double gam = a0[(P_GAM + a) * Epad], ab = a0[(P_ABS + a) * Epad];
         const double lo = a0[(P_MIN + a) * Epad], hi = a0[(P_MAX + a) * Epad], nm = a0[(P_NMX + a) * Epad];
         const double range = 0.5 * (hi - lo);
         const double fip = range * (1.0 + k_over_sy * nm);
         if (a == 0 || fip > best) { best = fip; bsys = a; brange = range; bn = nm; }   // the smallest system that attains the maximum
         asum += ab; net = fmax(net, fabs(gam));
      }
      double* o = sm + lane * (NFP + 1);
      o[EXA_FIP_FIP] = best; o[EXA_FIP_SYSTEM] = (double)bsys; o[EXA_FIP_SHEARRANGE] = brange; o[EXA_FIP_NORMALSTRESSMAX] = bn;
      o[EXA_FIP_ACCUMULATEDSLIP] = asum; o[EXA_FIP_NETSLIPMAX] = net;
   }
   __syncthreads();
   store_tile<NFP, NFP + 1>(out, base, sm, nv, lane);
}

// the pair (largest FIP, id): the larger FIP, on a tie the smaller id
__device__ __forceinline__ void best_of(double& f, double& id, const double f2, const double id2) {
   if (f2 > f || (f2 == f && id2 < id)) { f = f2; id = id2; }
}
constexpr double NEG_INF = -std::numeric_limits<double>::infinity();
constexpr double NO_ID = 9007199254740992.0;   // 2^53: above every element id

// sum V, sum V FIP, sum V AccumulatedSlip | max FIP, max ShearRange, max AccumulatedSlip | id of max FIP.  FIP carries no clamp and may be
// negative: -inf is the neutral element of the maxima
struct FipSummary {
   static constexpr int N = 7;
   static __device__ __forceinline__ void init(double* v) { v[0] = v[1] = v[2] = 0.0; v[3] = v[4] = v[5] = NEG_INF; v[6] = NO_ID; }
   static __device__ __forceinline__ void merge(double* v, const double* y) {
      v[0] += y[0]; v[1] += y[1]; v[2] += y[2];
      best_of(v[3], v[6], y[3], y[6]);
      v[4] = fmax(v[4], y[4]); v[5] = fmax(v[5], y[5]);
   }
};
constexpr int NSUM = FipSummary::N;

__global__ __launch_bounds__(S_THREADS) void k_fip_partial(const int64_t E, const double* __restrict__ F, const double* __restrict__ P, const int64_t* __restrict__ gid,
                                                           double* __restrict__ partial) {
   __shared__ double sm[S_WAVES][NSUM];
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   double v[NSUM];
   FipSummary::init(v);
   const int64_t nblk = (E + 63) / 64, stride = (int64_t)gridDim.x * S_WAVES;
   for (int64_t b = (int64_t)blockIdx.x * S_WAVES + wave; b < nblk; b += stride) {
      const int64_t e = b * 64 + lane;
      if (e >= E) continue;
      const double V = F[e * NF + EXA_F_VOLUME];
      const double* p = P + e * NFP;
      const double fip = p[EXA_FIP_FIP], rg = p[EXA_FIP_SHEARRANGE], as = p[EXA_FIP_ACCUMULATEDSLIP];
      v[0] += V; v[1] += V * fip; v[2] += V * as;
      best_of(v[3], v[6], fip, (double)gid[e]);
      v[4] = fmax(v[4], rg); v[5] = fmax(v[5], as);
   }
   summary_block_partial<FipSummary>(v, sm, partial);
}

__global__ __launch_bounds__(64) void k_fip_reduce(const int nb, const double* __restrict__ partial, double* __restrict__ out) {
   summary_reduce<FipSummary>(nb, partial, out);
}

inline int64_t pad64(int64_t E) { return (E + 63) / 64 * 64; }

}  // namespace

extern "C" int exa_slip_activity_sizes(int64_t E, int64_t* acc_doubles) {
   if (E < 0) return EXA_ERR_ARG;
   if (acc_doubles) *acc_doubles = (int64_t)EXA_NSLIPACC * pad64(E);
   return EXA_OK;
}

extern "C" int exa_slip_accumulate(exa_ctx* ctx, const double* fields_dev, const double* normals12x3, double dt, int reset, double* acc_dev, exa_stream str) {
   if (!ctx) return EXA_ERR_ARG;
   if (!normals12x3 || (ctx->E > 0 && (!fields_dev || !acc_dev))) { ctx->err = "exa_slip_accumulate: fields, plane normals and accumulators are required"; return EXA_ERR_ARG; }
   if (!std::isfinite(dt) || dt < 0.0) { ctx->err = "exa_slip_accumulate: dt must be a finite number >= 0"; return EXA_ERR_ARG; }
   Normals n;
   for (int a = 0; a < NS; a++) {
      const double* m = normals12x3 + 3 * a;
      const double len = std::sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]);
      if (!(len > 0.0) || !std::isfinite(len)) { ctx->err = "exa_slip_accumulate: a plane normal is zero or not finite"; return EXA_ERR_ARG; }
      for (int i = 0; i < 3; i++) n.m[a][i] = m[i] / len;
   }
   if (ctx->E == 0) return EXA_OK;
   hipStream_t s = reinterpret_cast<hipStream_t>(str);
   const int64_t E = ctx->E, Epad = pad64(E);
   const dim3 grid((unsigned)(Epad / CH));
   if (reset) hipLaunchKernelGGL(k_slip_accumulate<true>, grid, dim3(CH), 0, s, E, Epad, fields_dev, n, dt, acc_dev);
   else hipLaunchKernelGGL(k_slip_accumulate<false>, grid, dim3(CH), 0, s, E, Epad, fields_dev, n, dt, acc_dev);
   EXA_HIP_CHECK(ctx, hipGetLastError());
   return EXA_OK;
}

extern "C" int exa_fip_rows(exa_ctx* ctx, const double* acc_dev, double k_fs, double sigma_y, double* out_dev, exa_stream str) {
   if (!ctx) return EXA_ERR_ARG;
   if (ctx->E > 0 && (!acc_dev || !out_dev)) { ctx->err = "exa_fip_rows: accumulators and an output are required"; return EXA_ERR_ARG; }
   if (!(k_fs >= 0.0) || !std::isfinite(k_fs) || !(sigma_y > 0.0) || !std::isfinite(sigma_y)) { ctx->err = "exa_fip_rows: k_fs >= 0 and sigma_y > 0 (finite) are required"; return EXA_ERR_ARG; }
   if (ctx->E == 0) return EXA_OK;
   hipStream_t s = reinterpret_cast<hipStream_t>(str);
   const int64_t E = ctx->E, Epad = pad64(E);
   hipLaunchKernelGGL(k_fip_rows, dim3((unsigned)(Epad / CH)), dim3(CH), 0, s, E, Epad, acc_dev, k_fs / sigma_y, out_dev);
   EXA_HIP_CHECK(ctx, hipGetLastError());
   return EXA_OK;
}

extern "C" int exa_fip_summary(exa_ctx* ctx, const double* fields_dev, const double* fip_dev, const int64_t* elem_gid_dev, double* out7_dev, exa_stream str) {
   if (!ctx) return EXA_ERR_ARG;
   if (!out7_dev || (ctx->E > 0 && (!fields_dev || !fip_dev || !elem_gid_dev))) { ctx->err = "exa_fip_summary: fields, FIP rows, element ids and an output are required"; return EXA_ERR_ARG; }
   hipStream_t s = reinterpret_cast<hipStream_t>(str);
   int nb;   // (no rows: nb = 0, the reduce launch alone writes the neutral elements)
   if (int rc = summary_grid(ctx, "exa_fip_summary", S_THREADS, S_MAX_BLOCKS, NSUM, &nb)) return rc;
   if (nb > 0) hipLaunchKernelGGL(k_fip_partial, dim3(nb), dim3(S_THREADS), 0, s, (int64_t)ctx->E, fields_dev, fip_dev, elem_gid_dev, ctx->scratch_dev);
   hipLaunchKernelGGL(k_fip_reduce, dim3(1), dim3(64), 0, s, nb, (const double*)ctx->scratch_dev, out7_dev);
   EXA_HIP_CHECK(ctx, hipGetLastError());
   return EXA_OK;
}

extern "C" int exa_slip_plane_normals(int model, double* out12x3) {
   if (!out12x3) return EXA_ERR_ARG;
   // {111} planes of the 12 FCC systems and {110} planes of the 12 BCC systems, in the order of the slip rates (state slots 14 .. 25)
   static const int fcc[NS][3] = { { 1, 1, 1 }, { 1, 1, 1 }, { 1, 1, 1 }, { -1, 1, 1 }, { -1, 1, 1 }, { -1, 1, 1 },
                                   { -1, -1, 1 }, { -1, -1, 1 }, { -1, -1, 1 }, { 1, -1, 1 }, { 1, -1, 1 }, { 1, -1, 1 } };
   static const int bcc[NS][3] = { { 0, 1, -1 }, { -1, 0, 1 }, { 1, -1, 0 }, { -1, 0, -1 }, { 0, -1, 1 }, { 1, 1, 0 },
                                   { 0, -1, -1 }, { 1, 0, 1 }, { -1, 1, 0 }, { 1, 0, -1 }, { 0, 1, 1 }, { -1, -1, 0 } };
   const bool is_fcc = model == EXA_FCC_VOCE || model == EXA_FCC_VOCE_NL || model == EXA_FCC_KMDD;
   const bool is_bcc = model == EXA_BCC_VOCE || model == EXA_BCC_VOCE_NL || model == EXA_BCC_KMDD;
   if (!is_fcc && !is_bcc) return EXA_ERR_ARG;
   const int (*t)[3] = is_fcc ? fcc : bcc;
   for (int a = 0; a < NS; a++) {
      const double len = std::sqrt((double)(t[a][0] * t[a][0] + t[a][1] * t[a][1] + t[a][2] * t[a][2]));
      for (int i = 0; i < 3; i++) out12x3[3 * a + i] = t[a][i] / len;
   }
   return EXA_OK;
}

// private (scratch) bytes per lane of the kernels of this file in the loaded code object: out8 = { k_slip_accumulate<false>, <true>, k_fip_rows, k_fip_partial,
// k_fip_reduce, 0, 0, 0 }; returns 0, or -1 without a device
extern "C" int exa_fatigue_scratch_bytes(int* out8) {
   if (!out8) return -1;
   hipFuncAttributes a;
   auto get = [&](const void* f) -> int { if (hipFuncGetAttributes(&a, f) != hipSuccess) { (void)hipGetLastError(); return -1; } return (int)a.localSizeBytes; };
   out8[0] = get(reinterpret_cast<const void*>(k_slip_accumulate<false>)); out8[1] = get(reinterpret_cast<const void*>(k_slip_accumulate<true>));
   out8[2] = get(reinterpret_cast<const void*>(k_fip_rows)); out8[3] = get(reinterpret_cast<const void*>(k_fip_partial));
   out8[4] = get(reinterpret_cast<const void*>(k_fip_reduce)); out8[5] = out8[6] = out8[7] = 0;
   for (int k = 0; k < 5; k++) if (out8[k] < 0) return -1;
   return 0;
}
