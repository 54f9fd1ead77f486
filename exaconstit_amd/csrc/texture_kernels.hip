// In-situ texture (gfx950): pole figures of {hkl} families and inverse pole figures of sample directions on the per-element rows of
// exa_element_fields (include/exaconstit_hip.h), binned on an (alpha, beta) grid of the upper hemisphere.  Per element e
// (V = EXA_F_VOLUME, unit quaternion q = EXA_F_ORIENTATION, R = quat_to_mat(q): crystal -> sample, as lattice_kernels.hip):
//   pole figure of family j:           poles p = R c for the N_j axes c of the family's cubic orbit, each of weight V / N_j
//   inverse pole figure of direction d: u = R^T d, images p = S_k u for the 24 proper cubic rotations S_k, each of weight V / 24
// Every pole is folded onto the upper hemisphere and binned by texture_bin (below: the one statement of the binning rules, host and device).
// Exact, order-independent sums: a pole's weight is quantized to the unsigned 64-bit integer rint(V 2^-quantum_log2 / N); the counts are
// summed as integers (LDS atomics per workgroup, then one integer atomic add per non-empty bin and workgroup into the output), so the
// result has the same bits for any grid, element order or rank split of the same rows.  No float atomics.
// Design: lane = element, 64-element blocks dealt to the waves of a fixed grid (lattice_kernels.hip); each element's 5 doubles are read
// once per launch for all the sets whose histograms share the workgroup's LDS: the sets are cut into chunks of at most 64 KiB of counters
// (blockIdx.y = chunk); at the default 5 degrees every set up to 6 fits in one chunk.
#include "exa_internal.hpp"
#include <cmath>

namespace {

constexpr int NF = EXA_NFIELDS;
constexpr int MAXSET = EXA_TEXTURE_MAX_HKL + EXA_TEXTURE_MAX_DIRS, MAXCODE = 24 * MAXSET;
constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int LDS_BINS = 8192;     // 64 KiB of 64-bit counters per workgroup: one set at 2 degrees (45 x 180 = 8100 bins)
constexpr int MAX_BLOCKS = 512;    // per chunk; each workgroup adds its non-empty bins to the output once

// component i of the image of a vector b under signed-permutation code c: ((c >> (6 + i)) & 1 ? -1 : 1) * b[(c >> 2 i) & 3]
// (the fibre-axis codes of lattice_kernels.hip; a sign flip and a permutation are exact)
struct TexArgs {
   double v[MAXSET][3];      // pole figure: the family's first unit axis (crystal frame); inverse pole figure: the unit direction (sample frame)
   double wscale[MAXSET];    // 2^-quantum_log2 / N_set: count of a pole = rint(V wscale)
   uint16_t code[MAXCODE];
   int16_t off[MAXSET + 1];
   int8_t chunk[MAXSET + 1]; // chunk c holds the sets chunk[c] .. chunk[c + 1] - 1
   int npf, na, nb;
   double res_deg;
};

}  // namespace

// The binning rules (the contract of DESIGN 4.8): fold p onto the upper hemisphere (p_z < 0, or p_z = 0 and (p_y < 0, or p_y = 0 and p_x < 0):
// p -> -p), alpha = atan2(sqrt(p_x^2 + p_y^2), p_z) in [0, 90] degrees, beta = atan2(p_y, p_x) mapped into [0, 360) (0 at the pole itself);
// ring i = min(floor(alpha / res), n_alpha - 1), sector k = floor(beta / res) mod n_beta.
__host__ __device__ inline void texture_bin(double x, double y, double z, double res_deg, int na, int nb, int& i, int& k) {
   if (z < 0.0 || (z == 0.0 && (y < 0.0 || (y == 0.0 && x < 0.0)))) { x = -x; y = -y; z = -z; }
   double a = atan2(sqrt(x * x + y * y), z) * (180.0 / M_PI);
   if (!(a >= 0.0)) a = 0.0;   // NaN (a non-finite orientation): ring 0, never outside the grid
   const int ia = (int)floor(a / res_deg);
   i = ia < na - 1 ? ia : na - 1;
   double b = (x != 0.0 || y != 0.0) ? atan2(y, x) * (180.0 / M_PI) : 0.0;
   if (b < 0.0) b += 360.0;
   if (!(b >= 0.0)) b = 0.0;
   int kb = (int)floor(b / res_deg);
   if (kb >= nb) kb -= nb;   // b rounded up to 360
   k = kb < nb ? kb : nb - 1;
}

namespace {

__device__ __forceinline__ void perm(const double* b, int c, double& p0, double& p1, double& p2) {
   p0 = ((c >> 6) & 1) ? -b[c & 3] : b[c & 3];
   p1 = ((c >> 7) & 1) ? -b[(c >> 2) & 3] : b[(c >> 2) & 3];
   p2 = ((c >> 8) & 1) ? -b[(c >> 4) & 3] : b[(c >> 4) & 3];
}

__global__ __launch_bounds__(THREADS) void k_texture(const int64_t E, const double* __restrict__ F, unsigned long long* __restrict__ out, const TexArgs A) {
   extern __shared__ unsigned long long hist[];
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   const int s0 = A.chunk[blockIdx.y], s1 = A.chunk[blockIdx.y + 1];
   const int nbins = A.na * A.nb, tot = (s1 - s0) * nbins;
   for (int t = threadIdx.x; t < tot; t += THREADS) hist[t] = 0ull;
   __syncthreads();
   const int64_t nblk = (E + 63) / 64, stride = (int64_t)gridDim.x * WAVES;
   for (int64_t blk = (int64_t)blockIdx.x * WAVES + wave; blk < nblk; blk += stride) {
      const int64_t e = blk * 64 + lane;
      if (e >= E) continue;
      const double* r = F + e * NF;
      const double V = r[EXA_F_VOLUME];
      const double x0 = r[EXA_F_ORIENTATION], x1 = r[EXA_F_ORIENTATION + 1], x2 = r[EXA_F_ORIENTATION + 2], x3 = r[EXA_F_ORIENTATION + 3];
      // R(q) row-major (quat_to_mat, ecm_device.hpp)
      const double R0 = x0 * x0 + x1 * x1 - x2 * x2 - x3 * x3, R1 = 2.0 * (x1 * x2 - x0 * x3), R2 = 2.0 * (x1 * x3 + x0 * x2);
      const double R3 = 2.0 * (x1 * x2 + x0 * x3), R4 = x0 * x0 - x1 * x1 + x2 * x2 - x3 * x3, R5 = 2.0 * (x2 * x3 - x0 * x1);
      const double R6 = 2.0 * (x1 * x3 - x0 * x2), R7 = 2.0 * (x2 * x3 + x0 * x1), R8 = x0 * x0 - x1 * x1 - x2 * x2 + x3 * x3;
      for (int j = s0; j < s1; j++) {   // kernel-uniform bounds
         const unsigned long long w = (unsigned long long)rint(V * A.wscale[j]);
         unsigned long long* h = hist + (j - s0) * nbins;
         double u[3];
         if (j >= A.npf) {   // inverse pole figure: u = R^T d, images S_k u
            const double* d = A.v[j];
            u[0] = R0 * d[0] + R3 * d[1] + R6 * d[2];
            u[1] = R1 * d[0] + R4 * d[1] + R7 * d[2];
            u[2] = R2 * d[0] + R5 * d[1] + R8 * d[2];
         }
         for (int a = A.off[j]; a < A.off[j + 1]; a++) {
            double c0, c1, c2, p0, p1, p2;
            if (j < A.npf) {   // pole figure: p = R c
               perm(A.v[j], A.code[a], c0, c1, c2);
               p0 = R0 * c0 + R1 * c1 + R2 * c2;
               p1 = R3 * c0 + R4 * c1 + R5 * c2;
               p2 = R6 * c0 + R7 * c1 + R8 * c2;
            } else perm(u, A.code[a], p0, p1, p2);
            int i, k;
            texture_bin(p0, p1, p2, A.res_deg, A.na, A.nb, i, k);
            atomicAdd(&h[i * A.nb + k], w);
         }
      }
   }
   __syncthreads();
   unsigned long long* o = out + (int64_t)s0 * nbins;
   for (int t = threadIdx.x; t < tot; t += THREADS) {
      const unsigned long long c = hist[t];
      if (c) atomicAdd(&o[t], c);
   }
}

// largest EXA_F_VOLUME of the rows: per-block maxima in scratch, then one wave (max is exact: any order gives the same value)
__global__ __launch_bounds__(THREADS) void k_vmax_partial(const int64_t E, const double* __restrict__ F, double* __restrict__ partial) {
   __shared__ double sm[WAVES];
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   double m = 0.0;
   for (int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x; e < E; e += (int64_t)gridDim.x * THREADS) m = fmax(m, F[e * NF + EXA_F_VOLUME]);
#pragma unroll
   for (int d = 32; d > 0; d >>= 1) m = fmax(m, __shfl_down(m, d));
   if (lane == 0) sm[wave] = m;
   __syncthreads();
   if (threadIdx.x == 0) {
      double t = sm[0];
      for (int w = 1; w < WAVES; w++) t = fmax(t, sm[w]);
      partial[blockIdx.x] = t;
   }
}

__global__ __launch_bounds__(64) void k_vmax_reduce(const int nb, const double* __restrict__ partial, double* __restrict__ out) {
   double m = 0.0;
   for (int b = threadIdx.x; b < nb; b += 64) m = fmax(m, partial[b]);
#pragma unroll
   for (int d = 32; d > 0; d >>= 1) m = fmax(m, __shfl_down(m, d));
   if (threadIdx.x == 0) out[0] = m;
}

// the signed-permutation code taking v to c, or -1
int perm_code(const double* v, const double* c) {
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

}  // namespace

extern "C" int exa_texture_grid(double res_deg, int* n_alpha, int* n_beta) {
   if (!(res_deg >= 2.0 && res_deg <= 30.0)) return -1;
   const double n = 90.0 / res_deg, nr = std::nearbyint(n);
   if (std::fabs(n - nr) > 1e-9 * nr) return -1;
   if (n_alpha) *n_alpha = (int)nr;
   if (n_beta) *n_beta = 4 * (int)nr;
   return 0;
}

extern "C" int exa_texture_bin(const double* p3, double res_deg, int* i, int* k) {
   int na, nb;
   if (!p3 || !i || !k || exa_texture_grid(res_deg, &na, &nb) != 0) return -1;
   texture_bin(p3[0], p3[1], p3[2], res_deg, na, nb, *i, *k);
   return 0;
}

extern "C" int exa_texture_quantum_log2(double vmax, int64_t n_elements) {
   if (!(vmax > 0.0) || !std::isfinite(vmax) || n_elements < 1) return 0;
   int e;
   std::frexp(vmax * (double)n_elements, &e);   // 2^(e - 1) <= vmax n < 2^e
   return e - 61;                              // every set sums to at most ~2^61 counts over all elements of all ranks
}

extern "C" int exa_texture_volume_max(exa_ctx* ctx, const double* fields_dev, double* out_dev, exa_stream str) {
   if (!ctx) return EXA_ERR_ARG;
   if (!fields_dev || !out_dev) { ctx->err = "exa_texture_volume_max: fields and output are required"; return EXA_ERR_ARG; }
   hipStream_t s = reinterpret_cast<hipStream_t>(str);
   if (ctx->E == 0) { EXA_HIP_CHECK(ctx, hipMemsetAsync(out_dev, 0, sizeof(double), s)); return EXA_OK; }
   const int64_t need = ((int64_t)ctx->E + THREADS - 1) / THREADS;
   const int nb = (int)(need < 1024 ? need : 1024);
   if (sizeof(double) * (size_t)nb > ctx->scratch_bytes) { ctx->err = "exa_texture_volume_max: reduction scratch too small"; return EXA_ERR_UNSUPPORTED; }
   hipLaunchKernelGGL(k_vmax_partial, dim3(nb), dim3(THREADS), 0, s, (int64_t)ctx->E, fields_dev, ctx->scratch_dev);
   hipLaunchKernelGGL(k_vmax_reduce, dim3(1), dim3(64), 0, s, nb, (const double*)ctx->scratch_dev, out_dev);
   EXA_HIP_CHECK(ctx, hipGetLastError());
   return EXA_OK;
}

extern "C" int exa_texture_weights(exa_ctx* ctx, const double* fields_dev, int npf, const double* pf_axes, const int* pf_axis_offsets, int nipf,
                                   const double* ipf_dirs, double res_deg, int quantum_log2, int64_t* out_dev, exa_stream str) {
   if (!ctx) return EXA_ERR_ARG;
   if (!fields_dev || !out_dev || (npf > 0 && (!pf_axes || !pf_axis_offsets)) || (nipf > 0 && !ipf_dirs)) {
      ctx->err = "exa_texture_weights: fields, output, the axes of every family and the directions are required"; return EXA_ERR_ARG;
   }
   if (npf < 0 || npf > EXA_TEXTURE_MAX_HKL || nipf < 0 || nipf > EXA_TEXTURE_MAX_DIRS || npf + nipf < 1) {
      ctx->err = "exa_texture_weights: 0 to 16 families and 0 to 3 directions, at least one set"; return EXA_ERR_ARG;
   }
   TexArgs A{};
   if (exa_texture_grid(res_deg, &A.na, &A.nb) != 0) { ctx->err = "exa_texture_weights: res_deg must divide 90 and lie in [2, 30]"; return EXA_ERR_ARG; }
   if (quantum_log2 < -1000 || quantum_log2 > 1000) { ctx->err = "exa_texture_weights: quantum_log2 out of range"; return EXA_ERR_ARG; }
   A.npf = npf; A.res_deg = res_deg;
   const double scale = std::ldexp(1.0, -quantum_log2);
   int ncode = 0;
   if (npf > 0 && pf_axis_offsets[0] != 0) { ctx->err = "exa_texture_weights: pf_axis_offsets[0] must be 0"; return EXA_ERR_ARG; }
   for (int j = 0; j < npf; j++) {
      const int a0 = pf_axis_offsets[j], a1 = pf_axis_offsets[j + 1];
      if (a0 != ncode || a1 <= a0 || a1 - a0 > 24) { ctx->err = "exa_texture_weights: every family needs 1 to 24 axes"; return EXA_ERR_ARG; }
      const double* v = pf_axes + 3 * (size_t)a0;
      for (int i = 0; i < 3; i++) A.v[j][i] = v[i];
      for (int a = a0; a < a1; a++) {
         const int cd = perm_code(v, pf_axes + 3 * (size_t)a);
         if (cd < 0) { ctx->err = "exa_texture_weights: the axes of a family must be signed permutations of its first axis (a cubic orbit)"; return EXA_ERR_ARG; }
         A.code[ncode++] = (uint16_t)cd;
      }
      A.off[j] = (int16_t)a0; A.off[j + 1] = (int16_t)a1;
      A.wscale[j] = scale / (a1 - a0);
   }
   // the 24 proper rotations of the cubic group: the signed permutations of determinant +1
   uint16_t rot[24]; int nrot = 0;
   {
      static const int P[6][3] = { { 0, 1, 2 }, { 1, 2, 0 }, { 2, 0, 1 }, { 0, 2, 1 }, { 2, 1, 0 }, { 1, 0, 2 } };   // even permutations first
      for (int p = 0; p < 6; p++)
         for (int sg = 0; sg < 8; sg++) {
            const int par = p < 3 ? 1 : -1, sgn = ((sg & 1) ? -1 : 1) * ((sg & 2) ? -1 : 1) * ((sg & 4) ? -1 : 1);
            if (par * sgn == 1) rot[nrot++] = (uint16_t)(P[p][0] | (P[p][1] << 2) | (P[p][2] << 4) | (sg << 6));
         }
   }
   for (int m = 0; m < nipf; m++) {
      const int j = npf + m;
      const double* d = ipf_dirs + 3 * (size_t)m;
      const double n = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
      if (!(n > 0.0) || !std::isfinite(n)) { ctx->err = "exa_texture_weights: an inverse pole figure direction is zero"; return EXA_ERR_ARG; }
      for (int i = 0; i < 3; i++) A.v[j][i] = d[i] / n;
      A.off[j] = (int16_t)ncode;
      for (int r = 0; r < 24; r++) A.code[ncode++] = rot[r];
      A.off[j + 1] = (int16_t)ncode;
      A.wscale[j] = scale / 24.0;
   }
   // chunks of sets whose counters fit the workgroup's LDS together
   const int nset = npf + nipf, nbins = A.na * A.nb, per = LDS_BINS / nbins;
   int nchunk = 0, maxper = 0;
   for (int j = 0; j < nset; j += per) {
      A.chunk[nchunk++] = (int8_t)j;
      maxper = std::max(maxper, std::min(per, nset - j));
   }
   A.chunk[nchunk] = (int8_t)nset;
   hipStream_t s = reinterpret_cast<hipStream_t>(str);
   EXA_HIP_CHECK(ctx, hipMemsetAsync(out_dev, 0, sizeof(int64_t) * (size_t)nset * nbins, s));
   if (ctx->E == 0) return EXA_OK;
   const int64_t need = ((int64_t)ctx->E + 4 * THREADS - 1) / (4 * THREADS);   // at least 4 elements per lane
   const int nb = (int)(need < MAX_BLOCKS ? need : MAX_BLOCKS);
   hipLaunchKernelGGL(k_texture, dim3(nb, nchunk), dim3(THREADS), sizeof(unsigned long long) * (size_t)maxper * nbins, s, (int64_t)ctx->E, fields_dev,
                      reinterpret_cast<unsigned long long*>(out_dev), A);
   EXA_HIP_CHECK(ctx, hipGetLastError());
   return EXA_OK;
}
