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
__global__ void __launch_bounds__(256) k_periodic_sum(exa_host::PeriodicTable T, int nn, double* __restrict__ y, const double* __restrict__ flag, int bcast) {
   if (flag && flag[0] != 0.0) return;
   const int G = T.n2 + T.n4 + T.n8;
   const int t = blockIdx.x * blockDim.x + threadIdx.x;
   if (t >= 3 * G) return;
   const int c = t / G;
   int m, n; const int32_t* p = group_of(T, t - c * G, m, n);
   const int off = c * nn;
   double sum = y[p[0] + off];
   if (!bcast) for (int j = 1; j < m; j++) sum += y[p[j * n] + off];
   for (int j = bcast ? 1 : 0; j < m; j++) y[p[j * n] + off] = sum;
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

inline unsigned nblk(int64_t n) { return (unsigned)((n + 255) / 256); }
inline double9 mat9(const double* L9) { double9 L; for (int i = 0; i < 9; i++) L.a[i] = L9[i]; return L; }

}  // namespace

namespace exa_host {

void vk_periodic_sum(const PeriodicTable& T, int64_t nn, double* y, const double* flag, bool bcast, hipStream_t s) {
   const int64_t n = 3 * (int64_t)T.groups();
   if (n > 0) hipLaunchKernelGGL(k_periodic_sum, dim3(nblk(n)), dim3(256), 0, s, T, (int)nn, y, flag, bcast ? 1 : 0);
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

// bytes of private (scratch) memory per lane of k_periodic_sum in the loaded code object (hipFuncGetAttributes); -1 without a device
extern "C" int exa_periodic_sum_scratch_bytes(void) {
   hipFuncAttributes a;
   if (hipFuncGetAttributes(&a, reinterpret_cast<const void*>(k_periodic_sum)) != hipSuccess) { (void)hipGetLastError(); return -1; }
   return (int)a.localSizeBytes;
}
