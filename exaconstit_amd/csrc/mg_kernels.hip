// Kernels of the geometric multigrid preconditioner (host/multigrid.hip) on generated p = 1 meshes.
//
// Every level is a structured box of nodes: level l of a rank holds (ne >> l) + 1 nodes per direction, and its node (i, j, k) is node
// (2i, 2j, 2k) of level l - 1 (the vertices nest).  Vectors are laid out like the fine L-vector, dof = node + NN * component, node =
// i + n0 (j + n1 k).  A coarse operator is a 27-point stencil of 3 x 3 blocks per node: 243 doubles per node, structure of arrays,
// S[(o * 9 + 3 r + c) * NN + node] with neighbour offset o = (dx + 1) + 3 (dy + 1) + 9 (dz + 1), row component r, column component c.
//
// One thread per node everywhere; every sum runs in a fixed order and nothing is added atomically, so each launch gives the same bits
// for the same input.  Colours (probing of the Galerkin product) are taken from GLOBAL node coordinates, so every rank agrees on them.
#include "host/multigrid.hpp"

namespace exa_host {
namespace {

constexpr int MG_BS = 256;
__host__ __device__ inline int64_t grid_nn(const MgGrid& G) { return (int64_t)G.n[0] * G.n[1] * G.n[2]; }
__device__ inline int pmod(int a, int m) { const int r = a % m; return r < 0 ? r + m : r; }
__device__ inline int colour_of(const MgGrid& G, int i, int j, int k, int m) {
   return pmod(G.g0[0] + i, m) + m * (pmod(G.g0[1] + j, m) + m * pmod(G.g0[2] + k, m));
}

// y_f = beta y_f + P x_c: trilinear interpolation, weights 1, 1/2, 1/4, 1/8 (F = level l - 1, C = level l)
__global__ __launch_bounds__(MG_BS) void k_mg_prolong(const MgGrid F, const MgGrid C, const double* __restrict__ xc, double* __restrict__ yf, const double beta) {
   const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
   const int64_t nnf = grid_nn(F), nnc = grid_nn(C);
   if (t >= nnf) return;
   const int i = (int)(t % F.n[0]), j = (int)((t / F.n[0]) % F.n[1]), k = (int)(t / ((int64_t)F.n[0] * F.n[1]));
   const int f[3] = { i, j, k };
   int lo[3], cnt[3];
#pragma unroll
   for (int d = 0; d < 3; d++) { lo[d] = f[d] >> 1; cnt[d] = (f[d] & 1) ? 2 : 1; }
   const double w1 = 1.0, wh = 0.5;
   double s[3] = { 0.0, 0.0, 0.0 };
   for (int c2 = 0; c2 < cnt[2]; c2++)
      for (int c1 = 0; c1 < cnt[1]; c1++)
         for (int c0 = 0; c0 < cnt[0]; c0++) {
            const double w = (cnt[0] == 2 ? wh : w1) * (cnt[1] == 2 ? wh : w1) * (cnt[2] == 2 ? wh : w1);
            const int64_t v = (lo[0] + c0) + (int64_t)C.n[0] * ((lo[1] + c1) + (int64_t)C.n[1] * (lo[2] + c2));
#pragma unroll
            for (int c = 0; c < 3; c++) s[c] += w * xc[v + nnc * c];
         }
#pragma unroll
   for (int c = 0; c < 3; c++) yf[t + nnf * c] = (beta == 0.0 ? 0.0 : beta * yf[t + nnf * c]) + s[c];
}

// r_c(I) = sum_j w_j P_jI r_f(j) over the fine nodes j of the 3 x 3 x 3 neighbourhood of I (w = NULL: w_j = 1)
__global__ __launch_bounds__(MG_BS) void k_mg_restrict(const MgGrid F, const MgGrid C, const double* __restrict__ w, const double* __restrict__ rf, double* __restrict__ rc) {
   const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
   const int64_t nnf = grid_nn(F), nnc = grid_nn(C);
   if (t >= nnc) return;
   const int I = (int)(t % C.n[0]), J = (int)((t / C.n[0]) % C.n[1]), K = (int)(t / ((int64_t)C.n[0] * C.n[1]));
   double s[3] = { 0.0, 0.0, 0.0 };
   for (int dz = -1; dz <= 1; dz++) {
      const int fk = 2 * K + dz; if (fk < 0 || fk >= F.n[2]) continue;
      for (int dy = -1; dy <= 1; dy++) {
         const int fj = 2 * J + dy; if (fj < 0 || fj >= F.n[1]) continue;
         for (int dx = -1; dx <= 1; dx++) {
            const int fi = 2 * I + dx; if (fi < 0 || fi >= F.n[0]) continue;
            const int64_t v = fi + (int64_t)F.n[0] * (fj + (int64_t)F.n[1] * fk);
            const double wt = (dx ? 0.5 : 1.0) * (dy ? 0.5 : 1.0) * (dz ? 0.5 : 1.0) * (w ? w[v] : 1.0);
#pragma unroll
            for (int c = 0; c < 3; c++) s[c] += wt * rf[v + nnf * c];
         }
      }
   }
#pragma unroll
   for (int c = 0; c < 3; c++) rc[t + nnc * c] = s[c];
}

// y = A x with the 27-point block stencil (rows of this rank's part of the operator; the caller adds the other ranks' parts)
__global__ __launch_bounds__(MG_BS) void k_mg_stencil_apply(const MgGrid C, const double* __restrict__ S, const double* __restrict__ x, double* __restrict__ y) {
   const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
   const int64_t nn = grid_nn(C);
   if (t >= nn) return;
   const int i = (int)(t % C.n[0]), j = (int)((t / C.n[0]) % C.n[1]), k = (int)(t / ((int64_t)C.n[0] * C.n[1]));
   double s[3] = { 0.0, 0.0, 0.0 };
   for (int dz = -1; dz <= 1; dz++) {
      if (k + dz < 0 || k + dz >= C.n[2]) continue;
      for (int dy = -1; dy <= 1; dy++) {
         if (j + dy < 0 || j + dy >= C.n[1]) continue;
         for (int dx = -1; dx <= 1; dx++) {
            if (i + dx < 0 || i + dx >= C.n[0]) continue;
            const int o = (dx + 1) + 3 * (dy + 1) + 9 * (dz + 1);
            const int64_t v = t + dx + (int64_t)C.n[0] * (dy + (int64_t)C.n[1] * dz);
            const double xv[3] = { x[v], x[v + nn], x[v + 2 * nn] };
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
               for (int c = 0; c < 3; c++) s[r] += S[(o * 9 + 3 * r + c) * nn + t] * xv[c];
         }
      }
   }
#pragma unroll
   for (int r = 0; r < 3; r++) y[t + nn * r] = s[r];
}

// probe vector: 1 on component comp of the free nodes of colour `colour` (colour = global coordinates mod m), 0 elsewhere
__global__ __launch_bounds__(MG_BS) void k_mg_probe(const MgGrid C, const int m, const int colour, const int comp, const uint8_t* __restrict__ mask, double* __restrict__ x) {
   const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
   const int64_t nn = grid_nn(C);
   if (t >= nn) return;
   const int i = (int)(t % C.n[0]), j = (int)((t / C.n[0]) % C.n[1]), k = (int)(t / ((int64_t)C.n[0] * C.n[1]));
   const bool on = colour_of(C, i, j, k, m) == colour;
#pragma unroll
   for (int c = 0; c < 3; c++) x[t + nn * c] = (on && c == comp && !mask[t + nn * c]) ? 1.0 : 0.0;
}

// column `comp` of the stencil blocks whose neighbour has colour `colour` (mod 3) from the probe result y; neighbours outside the box get 0
__global__ __launch_bounds__(MG_BS) void k_mg_extract(const MgGrid C, const int colour, const int comp, const double* __restrict__ y, double* __restrict__ S) {
   const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
   const int64_t nn = grid_nn(C);
   if (t >= nn) return;
   const int i = (int)(t % C.n[0]), j = (int)((t / C.n[0]) % C.n[1]), k = (int)(t / ((int64_t)C.n[0] * C.n[1]));
   for (int o = 0; o < 27; o++) {
      const int dx = o % 3 - 1, dy = (o / 3) % 3 - 1, dz = o / 9 - 1;
      if (colour_of(C, i + dx, j + dy, k + dz, 3) != colour) continue;
      const bool in = i + dx >= 0 && i + dx < C.n[0] && j + dy >= 0 && j + dy < C.n[1] && k + dz >= 0 && k + dz < C.n[2];
#pragma unroll
      for (int r = 0; r < 3; r++) S[(o * 9 + 3 * r + comp) * nn + t] = in ? y[t + nn * r] : 0.0;
   }
}

// diagonal entries of component comp at the nodes of colour `colour` (mod m) from a probe result
__global__ __launch_bounds__(MG_BS) void k_mg_diag_probe(const MgGrid C, const int m, const int colour, const int comp, const double* __restrict__ y, double* __restrict__ diag) {
   const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
   const int64_t nn = grid_nn(C);
   if (t >= nn) return;
   const int i = (int)(t % C.n[0]), j = (int)((t / C.n[0]) % C.n[1]), k = (int)(t / ((int64_t)C.n[0] * C.n[1]));
   if (colour_of(C, i, j, k, m) == colour) diag[t + nn * comp] = y[t + nn * comp];
}

__global__ __launch_bounds__(MG_BS) void k_mg_stencil_diag(const MgGrid C, const double* __restrict__ S, double* __restrict__ diag) {
   const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
   const int64_t nn = grid_nn(C);
   if (t >= nn) return;
#pragma unroll
   for (int r = 0; r < 3; r++) diag[t + nn * r] = S[(13 * 9 + 4 * r) * nn + t];
}

// D^-1: zero on essential dofs (and where the diagonal vanishes)
__global__ __launch_bounds__(MG_BS) void k_mg_dinv(const int64_t n, const uint8_t* __restrict__ mask, const double* __restrict__ diag, double* __restrict__ dinv) {
   const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
   if (t < n) dinv[t] = (mask[t] || diag[t] == 0.0) ? 0.0 : 1.0 / diag[t];
}

// level-l essential mask = level l - 1 mask at the surviving nodes
__global__ __launch_bounds__(MG_BS) void k_mg_mask_coarsen(const MgGrid F, const MgGrid C, const uint8_t* __restrict__ mf, uint8_t* __restrict__ mc) {
   const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
   const int64_t nnf = grid_nn(F), nnc = grid_nn(C);
   if (t >= nnc) return;
   const int I = (int)(t % C.n[0]), J = (int)((t / C.n[0]) % C.n[1]), K = (int)(t / ((int64_t)C.n[0] * C.n[1]));
   const int64_t v = 2 * I + (int64_t)F.n[0] * (2 * J + (int64_t)F.n[1] * 2 * K);
#pragma unroll
   for (int c = 0; c < 3; c++) mc[t + nnc * c] = mf[v + nnf * c];
}

// Chebyshev step (Saad, Iterative Methods, Alg. 12.1, preconditioned by D^-1): first: d = c2 D^-1 r, x = d;
// otherwise r -= A d, d = c1 d + c2 D^-1 r, x += d
__global__ __launch_bounds__(MG_BS) void k_mg_cheb(const int64_t n, double* __restrict__ x, double* __restrict__ r, double* __restrict__ d, const double* __restrict__ Ad,
                                                   const double* __restrict__ dinv, const double c1, const double c2, const int first) {
   const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
   if (t >= n) return;
   if (first) { const double dd = c2 * dinv[t] * r[t]; d[t] = dd; x[t] = dd; return; }
   const double rr = r[t] - Ad[t];
   const double dd = c1 * d[t] + c2 * dinv[t] * rr;
   r[t] = rr; d[t] = dd; x[t] += dd;
}

// r = b - y, zero on essential dofs
__global__ __launch_bounds__(MG_BS) void k_mg_resid(const int64_t n, const uint8_t* __restrict__ mask, const double* __restrict__ b, const double* __restrict__ y, double* __restrict__ r) {
   const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
   if (t < n) r[t] = mask[t] ? 0.0 : b[t] - y[t];
}

// start vector of the power iteration: a hash of the GLOBAL dof index in (0, 1], zero on essential dofs (the same vector on every decomposition)
__global__ __launch_bounds__(MG_BS) void k_mg_seed(const MgGrid C, const int ng0, const int ng1, const int ng2, const uint8_t* __restrict__ mask, double* __restrict__ v) {
   const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
   const int64_t nn = grid_nn(C);
   if (t >= nn) return;
   const int i = (int)(t % C.n[0]), j = (int)((t / C.n[0]) % C.n[1]), k = (int)(t / ((int64_t)C.n[0] * C.n[1]));
   const uint64_t g = (uint64_t)(C.g0[0] + i) + (uint64_t)ng0 * ((uint64_t)(C.g0[1] + j) + (uint64_t)ng1 * (uint64_t)(C.g0[2] + k));
   (void)ng2;
#pragma unroll
   for (int c = 0; c < 3; c++) {
      uint64_t z = (3 * g + c) + 0x9E3779B97F4A7C15ull;   // splitmix64
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
      v[t + nn * c] = mask[t + nn * c] ? 0.0 : (double)((z >> 11) + 1) * (1.0 / 9007199254740992.0);
   }
}

// level-l vector <-> the level-0 positions of its nodes (stride 2^l): the coarse halo sums run on the fine exchange plan
__global__ __launch_bounds__(MG_BS) void k_mg_to_fine(const MgGrid F0, const MgGrid C, const int stride, const double* __restrict__ xc, double* __restrict__ x0) {
   const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
   const int64_t nn0 = grid_nn(F0), nnc = grid_nn(C);
   if (t >= nnc) return;
   const int I = (int)(t % C.n[0]), J = (int)((t / C.n[0]) % C.n[1]), K = (int)(t / ((int64_t)C.n[0] * C.n[1]));
   const int64_t v = (int64_t)stride * I + (int64_t)F0.n[0] * ((int64_t)stride * J + (int64_t)F0.n[1] * stride * K);
#pragma unroll
   for (int c = 0; c < 3; c++) x0[v + nn0 * c] = xc[t + nnc * c];
}
__global__ __launch_bounds__(MG_BS) void k_mg_from_fine(const MgGrid F0, const MgGrid C, const int stride, const double* __restrict__ x0, double* __restrict__ xc) {
   const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
   const int64_t nn0 = grid_nn(F0), nnc = grid_nn(C);
   if (t >= nnc) return;
   const int I = (int)(t % C.n[0]), J = (int)((t / C.n[0]) % C.n[1]), K = (int)(t / ((int64_t)C.n[0] * C.n[1]));
   const int64_t v = (int64_t)stride * I + (int64_t)F0.n[0] * ((int64_t)stride * J + (int64_t)F0.n[1] * stride * K);
#pragma unroll
   for (int c = 0; c < 3; c++) xc[t + nnc * c] = x0[v + nn0 * c];
}

inline unsigned blocks(int64_t n) { return (unsigned)((n + MG_BS - 1) / MG_BS); }
inline void launched(const char* what) { hip_check(hipGetLastError(), what); }

}  // namespace

void mg_prolong(const MgGrid& F, const MgGrid& C, const double* xc, double* yf, double beta, hipStream_t s) {
   hipLaunchKernelGGL(k_mg_prolong, dim3(blocks(grid_nn(F))), dim3(MG_BS), 0, s, F, C, xc, yf, beta); launched("k_mg_prolong");
}
void mg_restrict(const MgGrid& F, const MgGrid& C, const double* w, const double* rf, double* rc, hipStream_t s) {
   hipLaunchKernelGGL(k_mg_restrict, dim3(blocks(grid_nn(C))), dim3(MG_BS), 0, s, F, C, w, rf, rc); launched("k_mg_restrict");
}
void mg_stencil_apply(const MgGrid& C, const double* S, const double* x, double* y, hipStream_t s) {
   hipLaunchKernelGGL(k_mg_stencil_apply, dim3(blocks(grid_nn(C))), dim3(MG_BS), 0, s, C, S, x, y); launched("k_mg_stencil_apply");
}
void mg_probe(const MgGrid& C, int m, int colour, int comp, const uint8_t* mask, double* x, hipStream_t s) {
   hipLaunchKernelGGL(k_mg_probe, dim3(blocks(grid_nn(C))), dim3(MG_BS), 0, s, C, m, colour, comp, mask, x); launched("k_mg_probe");
}
void mg_extract(const MgGrid& C, int colour, int comp, const double* y, double* S, hipStream_t s) {
   hipLaunchKernelGGL(k_mg_extract, dim3(blocks(grid_nn(C))), dim3(MG_BS), 0, s, C, colour, comp, y, S); launched("k_mg_extract");
}
void mg_diag_probe(const MgGrid& C, int m, int colour, int comp, const double* y, double* diag, hipStream_t s) {
   hipLaunchKernelGGL(k_mg_diag_probe, dim3(blocks(grid_nn(C))), dim3(MG_BS), 0, s, C, m, colour, comp, y, diag); launched("k_mg_diag_probe");
}
void mg_stencil_diag(const MgGrid& C, const double* S, double* diag, hipStream_t s) {
   hipLaunchKernelGGL(k_mg_stencil_diag, dim3(blocks(grid_nn(C))), dim3(MG_BS), 0, s, C, S, diag); launched("k_mg_stencil_diag");
}
void mg_dinv(int64_t n, const uint8_t* mask, const double* diag, double* dinv, hipStream_t s) {
   hipLaunchKernelGGL(k_mg_dinv, dim3(blocks(n)), dim3(MG_BS), 0, s, n, mask, diag, dinv); launched("k_mg_dinv");
}
void mg_mask_coarsen(const MgGrid& F, const MgGrid& C, const uint8_t* mf, uint8_t* mc, hipStream_t s) {
   hipLaunchKernelGGL(k_mg_mask_coarsen, dim3(blocks(grid_nn(C))), dim3(MG_BS), 0, s, F, C, mf, mc); launched("k_mg_mask_coarsen");
}
void mg_cheb(int64_t n, double* x, double* r, double* d, const double* Ad, const double* dinv, double c1, double c2, bool first, hipStream_t s) {
   hipLaunchKernelGGL(k_mg_cheb, dim3(blocks(n)), dim3(MG_BS), 0, s, n, x, r, d, Ad, dinv, c1, c2, first ? 1 : 0); launched("k_mg_cheb");
}
void mg_resid(int64_t n, const uint8_t* mask, const double* b, const double* y, double* r, hipStream_t s) {
   hipLaunchKernelGGL(k_mg_resid, dim3(blocks(n)), dim3(MG_BS), 0, s, n, mask, b, y, r); launched("k_mg_resid");
}
void mg_seed(const MgGrid& C, const int ng[3], const uint8_t* mask, double* v, hipStream_t s) {
   hipLaunchKernelGGL(k_mg_seed, dim3(blocks(grid_nn(C))), dim3(MG_BS), 0, s, C, ng[0], ng[1], ng[2], mask, v); launched("k_mg_seed");
}
void mg_to_fine(const MgGrid& F0, const MgGrid& C, int stride, const double* xc, double* x0, hipStream_t s) {
   hipLaunchKernelGGL(k_mg_to_fine, dim3(blocks(grid_nn(C))), dim3(MG_BS), 0, s, F0, C, stride, xc, x0); launched("k_mg_to_fine");
}
void mg_from_fine(const MgGrid& F0, const MgGrid& C, int stride, const double* x0, double* xc, hipStream_t s) {
   hipLaunchKernelGGL(k_mg_from_fine, dim3(blocks(grid_nn(C))), dim3(MG_BS), 0, s, F0, C, stride, x0, xc); launched("k_mg_from_fine");
}

}  // namespace exa_host
