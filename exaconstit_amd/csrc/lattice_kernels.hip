// In-situ lattice strains of {hkl} fibres (gfx950): the analysis of the reference's light-up post-processing chain
//   scripts/postprocessing/adios2_extraction.py -> strain_Xtal_to_Sample.py -> calc_lattice_strain.py (math at lines 121-180)
// evaluated on the per-element rows of exa_element_fields (include/exaconstit_hip.h).  Per element e (V_e, unit quaternion q_e, crystal-frame
// elastic strain eps_e) and family j with the unit axes c of its cubic orbit (folded by sign, exa_cubic_fiber_axes):
//   u_e = R(q_e)^T s                          sample direction in the crystal frame (R = quat_to_mat, ecm_device.hpp: crystal -> sample)
//   e in fibre j  <=>  max_c |u_e . c| > cos_tol
//   eps_s = u_e^T eps_e u_e                   = s^T (R eps_e R^T) s
// and the launch leaves the 2H + 1 local sums  sum_{e in j} V_e eps_s, sum_{e in j} V_e (j = 0 .. H-1), sum_e V_e  in out_dev.
// Design (HBM-bound: each lane reads 11 of the 37 doubles of its own row, a wave's loads cover the 64 rows of its block): lane = element,
// 64-element blocks dealt to the waves of a fixed grid in a grid-stride loop, then the two-launch summary of analysis_device.hpp (wave tree ->
// the block's waves in wave order -> partials per block -> one wave), written out here because the number of values, 2H + 1, is a run-time
// count and the per-lane sums acc[2 MAXH + 1] are compacted on the way to LDS; lanes k < 2H + 1 combine the waves, one value each.  No atomics,
// the grid depends on E alone: every launch on the same data gives the same bits.
#include "analysis_device.hpp"
#include <cmath>

using namespace exa_analysis;

namespace {

constexpr int NF = EXA_NFIELDS;
constexpr int MAXH = EXA_LATTICE_MAX_HKL, MAXAX = 24 * MAXH, MAXV = 2 * MAXH + 1;
constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int MAX_BLOCKS = 960;   // partial sums: MAX_BLOCKS x MAXV doubles of ctx->scratch_dev (32768 doubles, capi.hip)

// The axes of a family travel by value as the signed-permutation codes of its first axis (perm_code / perm_apply, analysis_device.hpp): ~0.9 KB
// of kernel arguments instead of 9 KB of doubles
struct LatArgs {
   double v[MAXH][3];
   uint16_t code[MAXAX];
   int16_t off[MAXH + 1];
   double s[3];
   double cos_tol;
   int nhkl;
};

__global__ __launch_bounds__(THREADS) void k_lattice_partial(const int64_t E, const double* __restrict__ F, double* __restrict__ partial, const LatArgs A) {
   __shared__ double sm[WAVES][MAXV];
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   const int H = A.nhkl, nv = 2 * H + 1;
   double acc[MAXV];
#pragma unroll
   for (int k = 0; k < MAXV; k++) acc[k] = 0.0;
   const int64_t nblk = (E + 63) / 64, stride = (int64_t)gridDim.x * WAVES;
   for (int64_t b = (int64_t)blockIdx.x * WAVES + wave; b < nblk; b += stride) {
      const int64_t e = b * 64 + lane;
      if (e >= E) continue;
      const double* r = F + e * NF;
      const double V = r[EXA_F_VOLUME];
      const double q[4] = { r[EXA_F_ORIENTATION], r[EXA_F_ORIENTATION + 1], r[EXA_F_ORIENTATION + 2], r[EXA_F_ORIENTATION + 3] };
      double eps[6];
#pragma unroll
      for (int k = 0; k < 6; k++) eps[k] = r[EXA_F_XTALELASTICSTRAIN + k];
      double R[9]; ecmdev::quat_to_mat(q, R);   // row-major, = ExaModel::Quat2RMat; u = R^T s
      const double u0 = R[0] * A.s[0] + R[3] * A.s[1] + R[6] * A.s[2];
      const double u1 = R[1] * A.s[0] + R[4] * A.s[1] + R[7] * A.s[2];
      const double u2 = R[2] * A.s[0] + R[5] * A.s[1] + R[8] * A.s[2];
      // eps (11, 22, 33, 23, 13, 12), tensor components
      const double es = u0 * u0 * eps[0] + u1 * u1 * eps[1] + u2 * u2 * eps[2] + 2.0 * (u1 * u2 * eps[3] + u0 * u2 * eps[4] + u0 * u1 * eps[5]);
      const double Ves = V * es;
      acc[2 * MAXH] += V;
#pragma unroll
      for (int j = 0; j < MAXH; j++) {
         if (j >= H) continue;   // kernel-uniform (no break: the loop is unrolled so that acc stays in registers)
         double m = 0.0;
         for (int a = A.off[j]; a < A.off[j + 1]; a++) {
            // perm_apply's three lines in place: as a call the launch measured 8.06 us against the parent's 7.22 .. 7.76 (profiles/analysis_helpers_speed.txt)
            const int c = A.code[a];
            const double c0 = ((c >> 6) & 1) ? -A.v[j][c & 3] : A.v[j][c & 3];
            const double c1 = ((c >> 7) & 1) ? -A.v[j][(c >> 2) & 3] : A.v[j][(c >> 2) & 3];
            const double c2 = ((c >> 8) & 1) ? -A.v[j][(c >> 4) & 3] : A.v[j][(c >> 4) & 3];
            m = fmax(m, fabs(u0 * c0 + u1 * c1 + u2 * c2));
         }
         const bool in = m > A.cos_tol;
         acc[2 * j] += in ? Ves : 0.0;
         acc[2 * j + 1] += in ? V : 0.0;
      }
   }
   // wave, then the block's waves in order; value k of the output is acc[k] for k < 2H and acc[2 MAXH] (total volume) for k = 2H
#pragma unroll
   for (int k = 0; k < MAXV; k++) {
      if (k < 2 * H || k == 2 * MAXH) {
         const double w = wave_sum(acc[k]);
         if (lane == 0) sm[wave][k == 2 * MAXH ? 2 * H : k] = w;
      }
   }
   __syncthreads();
   if (threadIdx.x < nv) {
      double t = sm[0][threadIdx.x];
#pragma unroll
      for (int w = 1; w < WAVES; w++) t += sm[w][threadIdx.x];
      partial[(int64_t)blockIdx.x * nv + threadIdx.x] = t;
   }
}

// one wave: out[k] = sum over the nb blocks of partial[b][k], lanes over blocks in a fixed stride, then the shuffle tree
__global__ __launch_bounds__(64) void k_lattice_reduce(const int nb, const int nv, const double* __restrict__ partial, double* __restrict__ out) {
   const int lane = threadIdx.x;
   for (int k = 0; k < nv; k++) {
      double t = 0.0;
      for (int b = lane; b < nb; b += 64) t += partial[(int64_t)b * nv + k];
      t = wave_sum(t);
      if (lane == 0) out[k] = t;
   }
}

}  // namespace

extern "C" int exa_lattice_strains(exa_ctx* ctx, const double* fields_dev, int nhkl, const double* axes, const int* axis_offsets, const double* s_dir,
                                   double cos_tol, double* out_dev, exa_stream str) {
   if (!ctx) return EXA_ERR_ARG;
   if (!fields_dev || !axes || !axis_offsets || !s_dir || !out_dev) { ctx->err = "exa_lattice_strains: fields, axes, offsets, direction and output are required"; return EXA_ERR_ARG; }
   if (nhkl < 1 || nhkl > MAXH) { ctx->err = "exa_lattice_strains: 1 to 16 families"; return EXA_ERR_ARG; }
   LatArgs A{};
   A.nhkl = nhkl; A.cos_tol = cos_tol;
   for (int i = 0; i < 3; i++) A.s[i] = s_dir[i];
   if (axis_offsets[0] != 0) { ctx->err = "exa_lattice_strains: axis_offsets[0] must be 0"; return EXA_ERR_ARG; }
   for (int j = 0; j < nhkl; j++) {
      const int a0 = axis_offsets[j], a1 = axis_offsets[j + 1];
      if (a1 <= a0 || a1 - a0 > 24 || a1 > MAXAX) { ctx->err = "exa_lattice_strains: every family needs 1 to 24 axes"; return EXA_ERR_ARG; }
      A.off[j] = (int16_t)a0; A.off[j + 1] = (int16_t)a1;
      const double* v = axes + 3 * (size_t)a0;
      for (int i = 0; i < 3; i++) A.v[j][i] = v[i];
      for (int a = a0; a < a1; a++) {
         const int code = perm_code(v, axes + 3 * (size_t)a);
         if (code < 0) { ctx->err = "exa_lattice_strains: the axes of a family must be signed permutations of its first axis (a cubic orbit)"; return EXA_ERR_ARG; }
         A.code[a] = (uint16_t)code;
      }
   }
   const int nv = 2 * nhkl + 1;
   hipStream_t s = reinterpret_cast<hipStream_t>(str);
   if (ctx->E == 0) { EXA_HIP_CHECK(ctx, hipMemsetAsync(out_dev, 0, sizeof(double) * nv, s)); return EXA_OK; }
   int nb;
   if (int rc = summary_grid(ctx, "exa_lattice_strains", THREADS, MAX_BLOCKS, nv, &nb)) return rc;
   hipLaunchKernelGGL(k_lattice_partial, dim3(nb), dim3(THREADS), 0, s, (int64_t)ctx->E, fields_dev, ctx->scratch_dev, A);
   hipLaunchKernelGGL(k_lattice_reduce, dim3(1), dim3(64), 0, s, nb, nv, (const double*)ctx->scratch_dev, out_dev);
   EXA_HIP_CHECK(ctx, hipGetLastError());
   return EXA_OK;
}

// the 24 proper rotations of the cubic group are the signed permutation matrices of determinant +1; applied to (h, k, l) / |(h, k, l)| they
// give signed permutations of it, and folding c ~ -c (first non-zero component positive) leaves 4 / 3 / 6 / 12 / 24 axes for 111 / 200 / 220 / 311 / 123
extern "C" int exa_cubic_fiber_axes(int h, int k, int l, double* out, int max) {
   if (h == 0 && k == 0 && l == 0) return -1;
   const double n = std::sqrt((double)h * h + (double)k * k + (double)l * l);
   const double c[3] = { h / n, k / n, l / n };
   uint16_t rot[24];
   cubic_proper_rotations(rot);
   int cnt = 0;
   std::vector<double> ax;
   for (int r = 0; r < 24; r++) {   // in the order of the rotations: the axis order is part of the output
      double a[3];
      perm_apply(c, rot[r], a[0], a[1], a[2]);
      const double lead = a[0] != 0.0 ? a[0] : (a[1] != 0.0 ? a[1] : a[2]);
      if (lead < 0.0) for (double& x : a) x = -x;
      for (double& x : a) if (x == 0.0) x = 0.0;   // no -0
      bool dup = false;
      for (int i = 0; i < cnt && !dup; i++) dup = ax[3 * i] == a[0] && ax[3 * i + 1] == a[1] && ax[3 * i + 2] == a[2];
      if (dup) continue;
      ax.insert(ax.end(), a, a + 3); cnt++;
   }
   if (out) for (int i = 0; i < cnt && i < max; i++) for (int d = 0; d < 3; d++) out[3 * i + d] = ax[3 * i + d];
   return cnt;
}
