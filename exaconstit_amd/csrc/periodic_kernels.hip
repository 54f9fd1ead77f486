// Periodic boundary conditions: the vector kernels that keep the images of a degree of freedom consistent on one rank.
// A periodic group is the set of local nodes with one canonical id (host/mesh.hpp, Partition::make_periodic); its first member is the
// representative.  These are bandwidth kernels over surface dofs: one thread per (group, component), int32 indices, plain loads and stores.
//
// Device table (PeriodicTable): the groups sorted by size - n2 groups of 2 images (the face interiors: the bulk of the table), n4 of 4 (edges),
// n8 of 8 (corners) - and, within a size class of n groups, member-major: image j of group g at idx[base + j n + g].  Neighbouring threads read
// neighbouring table entries, and the face groups are one contiguous block.  Vectors are byNODES: dof = node + nn * component.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "host/device_utils.hpp"

namespace {

struct double9 { double a[9]; };

// group g of the table: image count m, stride n between its images, pointer to its representative's entry
__device__ __forceinline__ const int32_t* group_of(const exa_host::PeriodicTable& T, int g, int& m, int& n) {
   if (g < T.n2) { m = 2; n = T.n2; return T.idx + g; }
   g -= T.n2;
   if (g < T.n4) { m = 4; n = T.n4; return T.idx + 2 * T.n2 + g; }
   g -= T.n4;
   m = 8; n = T.n8; return T.idx + 2 * T.n2 + 4 * T.n4 + g;
}

// y(image) <- sum over the images of its group, added in table order: the same bits in every run and on every image.  No atomics: a dof
// belongs to one group.  bcast: y(image) <- y(representative) instead (after an exchange between ranks, which carries the representative only).
// flag: the PCG's done flag - the launch is a no-op once it is set, like the action it follows.
__device__ __forceinline__ void periodic_sum_entry(const exa_host::PeriodicTable& T, int nn, double* __restrict__ y, int bcast, int t) {
   const int G = T.n2 + T.n4 + T.n8;
   if (t >= 3 * G) return;
   const int c = t / G;
   int m, n; const int32_t* p = group_of(T, t - c * G, m, n);
   const int off = c * nn;
   double sum = y[p[0] + off];
   if (!bcast) for (int j = 1; j < m; j++) sum += y[p[j * n] + off];
   for (int j = bcast ? 1 : 0; j < m; j++) y[p[j * n] + off] = sum;
}
__global__ void __launch_bounds__(256) k_periodic_sum(exa_host::PeriodicTable T, int nn, double* __restrict__ y, const double* __restrict__ flag, int bcast) {
   if (flag && flag[0] != 0.0) return;
   periodic_sum_entry(T, nn, y, bcast, blockIdx.x * blockDim.x + threadIdx.x);
}

// ---- mixed loading: the corner differences H_id = v_i(c_d) - v_i(c_0) are unknowns of the system --------------------------------
// expand (P): the stored vector holds the group value on every image and the control values H_id in the slots (c_d, i); the full nodal field is
// out(image) = in(image) + sum_d n_d H_d with the image's 3-bit code n, and out(corner) = in(c_0) + sum_d n_d H_d (bit 3 of the code).  One thread
// per (image, component), out of place: out holds a copy of `in` (masked, when constrained) everywhere else.  constrained: the essential entries of
// the input count as zero - c_0 and the prescribed H_id (the input-side mask of a corner image follows: it is zero only if every H_id it adds is).
// h12: { in(c_0) (3), H row by row (9) } gathered and summed over the ranks; nullptr (one rank): read from `in` at the control nodes.
__global__ void __launch_bounds__(256) k_periodic_expand(exa_host::MixedTable M, int nn, const double* __restrict__ in, const double* __restrict__ h12,
                                                         double* __restrict__ out, const double* __restrict__ flag, int constrained) {
   if (flag && flag[0] != 0.0) return;
   const int t = blockIdx.x * blockDim.x + threadIdx.x;
   if (t >= 3 * M.nimg) return;
   const int c = t / M.nimg, e = t - c * M.nimg;
   const int node = M.img[e], code = M.code[e], off = c * nn;
   double v;
   if (code & 8) v = constrained ? 0.0 : (h12 ? h12[c] : in[M.ctrl[0] + off]);
   else v = in[node + off];
   for (int d = 0; d < 3; d++) if ((code >> d) & 1) {
      if (constrained && !((M.free_bits >> (3 * c + d)) & 1)) continue;
      v += h12 ? h12[3 + 3 * c + d] : in[M.ctrl[1 + d] + off];
   }
   out[node + off] = v;
}

// out[k] = src[idx[k]] (0 where idx[k] < 0): the corner values a rank holds, for the sum over the ranks
struct int24 { int32_t a[24]; };
__global__ void k_gather_slots(int24 idx, int n, const double* __restrict__ src, double* __restrict__ out) {
   const int k = threadIdx.x;
   if (k < n) out[k] = idx.a[k] >= 0 ? src[idx.a[k]] : 0.0;
}

// face resultants, stage 1: F_id = sum over the nodes of top face d of component i of the raw element contributions y (before any sum over images
// or ranks: the contributions of the ranks are disjoint).  Block b works on 256 nodes of one face (M.fblk: first block of each face) and writes
// its three partial sums to part[3 b + i]: shuffles within a wave, the four waves through LDS in wave order - a fixed order, no atomics.
__global__ void __launch_bounds__(256) k_face_resultants(exa_host::MixedTable M, int nn, const double* __restrict__ y, const double* __restrict__ flag, double* __restrict__ part) {
   if (flag && flag[0] != 0.0) return;
   __shared__ double lds[4][3];
   const int b = blockIdx.x;
   const int d = b >= M.fblk[2] ? 2 : (b >= M.fblk[1] ? 1 : 0);
   const int k = (b - M.fblk[d]) * 256 + threadIdx.x;
   double s0 = 0.0, s1 = 0.0, s2 = 0.0;
   if (k < M.foff[d + 1] - M.foff[d]) { const int node = M.face[M.foff[d] + k]; s0 = y[node]; s1 = y[node + nn]; s2 = y[node + 2 * nn]; }
   for (int o = 32; o > 0; o >>= 1) { s0 += __shfl_down(s0, o, 64); s1 += __shfl_down(s1, o, 64); s2 += __shfl_down(s2, o, 64); }
   const int w = threadIdx.x >> 6;
   if ((threadIdx.x & 63) == 0) { lds[w][0] = s0; lds[w][1] = s1; lds[w][2] = s2; }
   __syncthreads();
   if (threadIdx.x < 3) part[3 * b + threadIdx.x] = ((lds[0][threadIdx.x] + lds[1][threadIdx.x]) + lds[2][threadIdx.x]) + lds[3][threadIdx.x];
}
// stage 2, inside the consumer: thread k = 3 i + d adds the partial sums of face d in block order -> f9[k], and writes the free ones to their control slots
__device__ __forceinline__ void face_combine(const exa_host::MixedTable& M, int nn, const double* __restrict__ part, double* __restrict__ f9, double* __restrict__ y, int k) {
   const int i = k / 3, d = k - 3 * i;
   double s = 0.0;
   for (int b = M.fblk[d]; b < M.fblk[d + 1]; b++) s += part[3 * b + i];
   if (f9) f9[k] = s;
   if (y && ((M.free_bits >> k) & 1) && M.ctrl[1 + d] >= 0) y[M.ctrl[1 + d] + i * nn] = s;
}
// one rank: the sum over the periodic images, and one more block that finishes the resultants (the corners are in no group: the two do not meet)
__global__ void __launch_bounds__(256) k_periodic_sum_controls(exa_host::PeriodicTable T, exa_host::MixedTable M, int nn, double* __restrict__ y, const double* __restrict__ flag,
                                                               const double* __restrict__ part, double* __restrict__ f9) {
   if (flag && flag[0] != 0.0) return;
   if (blockIdx.x + 1 == gridDim.x) { if (threadIdx.x < 9) face_combine(M, nn, part, f9, y, threadIdx.x); return; }
   periodic_sum_entry(T, nn, y, 0, blockIdx.x * blockDim.x + threadIdx.x);
}
// several ranks: combine (y = nullptr) before the all-reduce of f9; control write after it (part = nullptr: f9 holds the sums of all ranks)
__global__ void k_face_combine(exa_host::MixedTable M, int nn, const double* __restrict__ part, double* __restrict__ f9, double* __restrict__ y, const double* __restrict__ flag) {
   if (flag && flag[0] != 0.0) return;
   const int k = threadIdx.x;
   if (k >= 9) return;
   if (part) { face_combine(M, nn, part, f9, y, k); return; }
   const int i = k / 3, d = k - 3 * i;
   if (((M.free_bits >> k) & 1) && M.ctrl[1 + d] >= 0) y[M.ctrl[1 + d] + i * nn] = f9[k];
}

// v(image) = v(representative) + L (x(image) - x(representative)): the affine jump of the velocity between the images of a node
__global__ void __launch_bounds__(256) k_periodic_jump(exa_host::PeriodicTable T, int nn, const double* __restrict__ x, double9 L, double* __restrict__ v) {
   const int G = T.n2 + T.n4 + T.n8;
   const int t = blockIdx.x * blockDim.x + threadIdx.x;
   if (t >= 3 * G) return;
   const int c = t / G;
   int m, n; const int32_t* p = group_of(T, t - c * G, m, n);
   const int r = p[0];
   const double x0 = x[r], x1 = x[r + nn], x2 = x[r + 2 * nn], vr = v[r + c * nn];
   for (int j = 1; j < m; j++) {
      const int a = p[j * n];
      v[a + c * nn] = vr + L.a[3 * c] * (x[a] - x0) + L.a[3 * c + 1] * (x[a + nn] - x1) + L.a[3 * c + 2] * (x[a + 2 * nn] - x2);
   }
}

// Several ranks: the images of a node may sit on different ranks, so the jump is imposed through the fluctuation w = v - L x, which is the same
// on all images.  k_periodic_fluct writes t = rep_w (v - L x) - rep_w = 1 / (ranks holding the node) on the node whose grid index is its canonical
// id, 0 on the other images - the summation over images and ranks (SumLVector) turns t into that node's fluctuation on every image, and
// k_periodic_unfluct sets v = t + L x on the nodes of the box surface.
__global__ void __launch_bounds__(256) k_periodic_fluct(int nn, const double* __restrict__ rep_w, const double* __restrict__ x, double9 L, const double* __restrict__ v, double* __restrict__ t) {
   const int g = blockIdx.x * blockDim.x + threadIdx.x;
   if (g >= nn) return;
   const double w = rep_w[g], x0 = x[g], x1 = x[g + nn], x2 = x[g + 2 * nn];
   for (int c = 0; c < 3; c++) t[g + c * nn] = w * (v[g + c * nn] - (L.a[3 * c] * x0 + L.a[3 * c + 1] * x1 + L.a[3 * c + 2] * x2));
}
__global__ void __launch_bounds__(256) k_periodic_unfluct(int nn, const uint8_t* __restrict__ surf, const double* __restrict__ x, double9 L, const double* __restrict__ t, double* __restrict__ v) {
   const int g = blockIdx.x * blockDim.x + threadIdx.x;
   if (g >= nn || !surf[g]) return;
   const double x0 = x[g], x1 = x[g + nn], x2 = x[g + 2 * nn];
   for (int c = 0; c < 3; c++) v[g + c * nn] = t[g + c * nn] + (L.a[3 * c] * x0 + L.a[3 * c + 1] * x1 + L.a[3 * c + 2] * x2);
}

// v += dL (x - origin) on every node: a change of the macroscopic velocity gradient keeps the fluctuation and swaps the affine part
__global__ void __launch_bounds__(256) k_periodic_affine_add(int nn, const double* __restrict__ x, const double* __restrict__ org, double9 L, double* __restrict__ v) {
   const int g = blockIdx.x * blockDim.x + threadIdx.x;
   if (g >= nn) return;
   const double d0 = x[g] - org[0], d1 = x[g + nn] - org[1], d2 = x[g + 2 * nn] - org[2];
   for (int c = 0; c < 3; c++) v[g + c * nn] += L.a[3 * c] * d0 + L.a[3 * c + 1] * d1 + L.a[3 * c + 2] * d2;
}

// v += t on every node: a rigid translation (mixed loading: the pinned corner follows the realised gradient, SystemDriver::MixedStepEnd)
__global__ void __launch_bounds__(256) k_translate(int nn, double t0, double t1, double t2, double* __restrict__ v) {
   const int g = blockIdx.x * blockDim.x + threadIdx.x;
   if (g >= nn) return;
   v[g] += t0; v[g + nn] += t1; v[g + 2 * nn] += t2;
}

inline unsigned nblk(int64_t n) { return (unsigned)((n + 255) / 256); }
inline double9 mat9(const double* L9) { double9 L; for (int i = 0; i < 9; i++) L.a[i] = L9[i]; return L; }

}  // namespace

namespace exa_host {

void vk_periodic_sum(const PeriodicTable& T, int64_t nn, double* y, const double* flag, bool bcast, hipStream_t s) {
   const int64_t n = 3 * (int64_t)T.groups();
   if (n > 0) hipLaunchKernelGGL(k_periodic_sum, dim3(nblk(n)), dim3(256), 0, s, T, (int)nn, y, flag, bcast ? 1 : 0);
}
void vk_periodic_expand(const MixedTable& M, int64_t nn, const double* in, const double* h12, double* out, const double* flag, bool constrained, hipStream_t s) {
   const int64_t n = 3 * (int64_t)M.nimg;
   if (n > 0) hipLaunchKernelGGL(k_periodic_expand, dim3(nblk(n)), dim3(256), 0, s, M, (int)nn, in, h12, out, flag, constrained ? 1 : 0);
}
void vk_gather_slots(const int32_t* idx_host, int n, const double* src, double* out, hipStream_t s) {
   int24 a; for (int k = 0; k < 24; k++) a.a[k] = k < n ? idx_host[k] : -1;
   hipLaunchKernelGGL(k_gather_slots, dim3(1), dim3(64), 0, s, a, n, src, out);
}
void vk_face_resultants(const MixedTable& M, int64_t nn, const double* y, const double* flag, double* part, hipStream_t s) {
   if (M.fblk[3] > 0) hipLaunchKernelGGL(k_face_resultants, dim3(M.fblk[3]), dim3(256), 0, s, M, (int)nn, y, flag, part);
}
void vk_periodic_sum_controls(const PeriodicTable& T, const MixedTable& M, int64_t nn, double* y, const double* flag, const double* part, double* f9, hipStream_t s) {
   const int64_t n = 3 * (int64_t)T.groups();
   hipLaunchKernelGGL(k_periodic_sum_controls, dim3(nblk(n) + 1), dim3(256), 0, s, T, M, (int)nn, y, flag, part, f9);
}
void vk_face_combine(const MixedTable& M, int64_t nn, const double* part, double* f9, double* y, const double* flag, hipStream_t s) {
   hipLaunchKernelGGL(k_face_combine, dim3(1), dim3(64), 0, s, M, (int)nn, part, f9, y, flag);
}
void vk_translate(int64_t nn, const double* t3_host, double* v, hipStream_t s) {
   if (nn > 0) hipLaunchKernelGGL(k_translate, dim3(nblk(nn)), dim3(256), 0, s, (int)nn, t3_host[0], t3_host[1], t3_host[2], v);
}
void vk_periodic_jump(const PeriodicTable& T, int64_t nn, const double* x, const double* L9_host, double* v, hipStream_t s) {
   const int64_t n = 3 * (int64_t)T.groups();
   if (n > 0) hipLaunchKernelGGL(k_periodic_jump, dim3(nblk(n)), dim3(256), 0, s, T, (int)nn, x, mat9(L9_host), v);
}
void vk_periodic_affine_add(int64_t nn, const double* x, const double* org3_dev, const double* L9_host, double* v, hipStream_t s) {
   if (nn > 0) hipLaunchKernelGGL(k_periodic_affine_add, dim3(nblk(nn)), dim3(256), 0, s, (int)nn, x, org3_dev, mat9(L9_host), v);
}
void vk_periodic_fluct(int64_t nn, const double* rep_w, const double* x, const double* L9_host, const double* v, double* t, hipStream_t s) {
   if (nn > 0) hipLaunchKernelGGL(k_periodic_fluct, dim3(nblk(nn)), dim3(256), 0, s, (int)nn, rep_w, x, mat9(L9_host), v, t);
}
void vk_periodic_unfluct(int64_t nn, const uint8_t* surf, const double* x, const double* L9_host, const double* t, double* v, hipStream_t s) {
   if (nn > 0) hipLaunchKernelGGL(k_periodic_unfluct, dim3(nblk(nn)), dim3(256), 0, s, (int)nn, surf, x, mat9(L9_host), t, v);
}

}  // namespace exa_host

// the same of the two kernels of mixed loading: out2 = { k_periodic_expand, k_face_resultants }
extern "C" int exa_periodic_mixed_scratch_bytes(int* out2) {
   hipFuncAttributes a;
   if (hipFuncGetAttributes(&a, reinterpret_cast<const void*>(k_periodic_expand)) != hipSuccess) { (void)hipGetLastError(); return -1; }
   out2[0] = (int)a.localSizeBytes;
   if (hipFuncGetAttributes(&a, reinterpret_cast<const void*>(k_face_resultants)) != hipSuccess) { (void)hipGetLastError(); return -1; }
   out2[1] = (int)a.localSizeBytes;
   return 0;
}

// bytes of private (scratch) memory per lane of k_periodic_sum in the loaded code object (hipFuncGetAttributes); -1 without a device
extern "C" int exa_periodic_sum_scratch_bytes(void) {
   hipFuncAttributes a;
   if (hipFuncGetAttributes(&a, reinterpret_cast<const void*>(k_periodic_sum)) != hipSuccess) { (void)hipGetLastError(); return -1; }
   return (int)a.localSizeBytes;
}
