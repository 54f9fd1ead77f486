// In-situ texture (gfx950): pole figures of {hkl} families and inverse pole figures of sample directions on the per-element rows of
// exa_element_fields (include/exaconstit_hip.h), binned on an (alpha, beta) grid of the upper hemisphere.  Per element e
// (V = EXA_F_VOLUME, unit quaternion q = EXA_F_ORIENTATION, R = quat_to_mat(q): crystal -> sample):
//   pole figure of family j:           poles p = R c for the N_j axes c of the family's cubic orbit, each of weight V / N_j
//   inverse pole figure of direction d: u = R^T d, images p = S_k u for the 24 proper cubic rotations S_k, each of weight V / 24
// Every pole is folded onto the upper hemisphere and binned by texture_bin (below: the one statement of the binning rules, host and device).
// Exact, order-independent sums: a pole's weight is quantized to the unsigned 64-bit integer rint(V 2^-quantum_log2 / N); the counts are
// summed as integers (LDS atomics per workgroup, then one integer atomic add per non-empty bin and workgroup into the output), so the
// result has the same bits for any grid, element order or rank split of the same rows.  No float atomics.
// Design: lane = element, 64-element blocks dealt to the waves of a fixed grid in a grid-stride loop; each element's 5 doubles are read
// once per launch for all the sets whose histograms share the workgroup's LDS: the sets are cut into chunks of at most 64 KiB of counters
// (blockIdx.y = chunk); at the default 5 degrees every set up to 6 fits in one chunk.  The largest volume, which sizes the quantum, comes
// from the two-launch summary of analysis_device.hpp; the axes and rotations travel as its signed-permutation codes.
#include "analysis_device.hpp"
#include <cmath>

using namespace exa_analysis;

namespace {

constexpr int NF = EXA_NFIELDS;
constexpr int MAXSET = EXA_TEXTURE_MAX_HKL + EXA_TEXTURE_MAX_DIRS, MAXCODE = 24 * MAXSET;
constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int LDS_BINS = 8192;     // 64 KiB of 64-bit counters per workgroup: one set at 2 degrees (45 x 180 = 8100 bins)
constexpr int MAX_BLOCKS = 512;    // per chunk; each workgroup adds its non-empty bins to the output once
constexpr int VMAX_BLOCKS = 1024;  // the volume maximum's summary grid

struct TexArgs {
   double v[MAXSET][3];      // pole figure: the family's first unit axis (crystal frame); inverse pole figure: the unit direction (sample frame)
   double wscale[MAXSET];    // 2^-quantum_log2 / N_set: count of a pole = rint(V wscale)
   uint16_t code[MAXCODE];   // perm_apply: a family's axes from its first axis, the 24 cubic images of u
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
      const double q[4] = { r[EXA_F_ORIENTATION], r[EXA_F_ORIENTATION + 1], r[EXA_F_ORIENTATION + 2], r[EXA_F_ORIENTATION + 3] };
      double R[9]; ecmdev::quat_to_mat(q, R);   // row-major
      for (int j = s0; j < s1; j++) {   // kernel-uniform bounds
         const unsigned long long w = (unsigned long long)rint(V * A.wscale[j]);
         unsigned long long* h = hist + (j - s0) * nbins;
         double u[3];
         if (j >= A.npf) {   // inverse pole figure: u = R^T d, images S_k u
            const double* d = A.v[j];
            u[0] = R[0] * d[0] + R[3] * d[1] + R[6] * d[2];
            u[1] = R[1] * d[0] + R[4] * d[1] + R[7] * d[2];
            u[2] = R[2] * d[0] + R[5] * d[1] + R[8] * d[2];
         }
         for (int a = A.off[j]; a < A.off[j + 1]; a++) {
            double c0, c1, c2, p0, p1, p2;
            if (j < A.npf) {   // pole figure: p = R c
               perm_apply(A.v[j], A.code[a], c0, c1, c2);
               p0 = R[0] * c0 + R[1] * c1 + R[2] * c2;
               p1 = R[3] * c0 + R[4] * c1 + R[5] * c2;
               p2 = R[6] * c0 + R[7] * c1 + R[8] * c2;
            } else perm_apply(u, A.code[a], p0, p1, p2);
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

// largest EXA_F_VOLUME of the rows (max is exact: any order gives the same value); volumes are > 0: 0 is the neutral element
struct VolumeMax {
   static constexpr int N = 1;
   static __device__ __forceinline__ void init(double* v) { v[0] = 0.0; }
   static __device__ __forceinline__ void merge(double* v, const double* y) { v[0] = fmax(v[0], y[0]); }
};

__global__ __launch_bounds__(THREADS) void k_vmax_partial(const int64_t E, const double* __restrict__ F, double* __restrict__ partial) {
   __shared__ double sm[WAVES][1];
   double m[1];
   VolumeMax::init(m);
   for (int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x; e < E; e += (int64_t)gridDim.x * THREADS) m[0] = fmax(m[0], F[e * NF + EXA_F_VOLUME]);
   summary_block_partial<VolumeMax>(m, sm, partial);
}

__global__ __launch_bounds__(64) void k_vmax_reduce(const int nb, const double* __restrict__ partial, double* __restrict__ out) {
   summary_reduce<VolumeMax>(nb, partial, out);
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
   int nb;
   if (int rc = summary_grid(ctx, "exa_texture_volume_max", THREADS, VMAX_BLOCKS, VolumeMax::N, &nb)) return rc;
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
   uint16_t rot[24];
   cubic_proper_rotations(rot);
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
