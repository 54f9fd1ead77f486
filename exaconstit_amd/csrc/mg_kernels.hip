// Kernels of the geometric multigrid preconditioner (host/multigrid.hip) on generated meshes of order p = 1 and 2.
//
// Every level is a structured box of nodes: level l of a rank holds ((ne p) >> l) + 1 nodes per direction, and its node (i, j, k) is node
// (2i, 2j, 2k) of level l - 1 (the vertices nest; at p = 2 level 0 is the p = 2 node grid and level 1 the element vertices, whose stencil and the
// fine diagonal gen_kernels.hip reads off the point records).  Vectors are laid out like the fine L-vector, dof = node + NN * component, node =
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

// Periodic cell on one rank ("periodic cells"): in every direction index 0 and index n - 1 are images of each other, at every level.
// y = G (S x), G the sum over the images of a node written to every image, in ONE launch: the thread of a surface node evaluates the stored rows
// of all local images of its node (2 on a face, 4 on an edge, 8 at a corner), each exactly as k_mg_stencil_apply evaluates it (no wrap inside a
// row: S holds the operator of nodes taken as distinct), and adds the row sums in ascending local index of the image.  Every image of a node runs
// the same instructions on the same data, so all of them carry the same bits: no atomics, no second launch, no group table.  Interior threads do
// what k_mg_stencil_apply does.  The loops run over image counts (1 or 2 per direction), never over an array: nothing is spilled.
__global__ __launch_bounds__(MG_BS) void k_mg_stencil_apply_periodic(const MgGrid C, const double* __restrict__ S, const double* __restrict__ x, double* __restrict__ y) {
   const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
   const int64_t nn = grid_nn(C);
   if (t >= nn) return;
   const int i = (int)(t % C.n[0]), j = (int)((t / C.n[0]) % C.n[1]), k = (int)(t / ((int64_t)C.n[0] * C.n[1]));
   const int ci = (i == 0 || i == C.n[0] - 1) ? 2 : 1, cj = (j == 0 || j == C.n[1] - 1) ? 2 : 1, ck = (k == 0 || k == C.n[2] - 1) ? 2 : 1;
   double acc[3] = { 0.0, 0.0, 0.0 };
   for (int mk = 0; mk < ck; mk++) {
      const int kk = ck == 2 ? mk * (C.n[2] - 1) : k;
      for (int mj = 0; mj < cj; mj++) {
         const int jj = cj == 2 ? mj * (C.n[1] - 1) : j;
         for (int mi = 0; mi < ci; mi++) {
            const int ii = ci == 2 ? mi * (C.n[0] - 1) : i;
            const int64_t u = ii + (int64_t)C.n[0] * (jj + (int64_t)C.n[1] * kk);   // the image whose row this is
            // One row: the neighbours free of branches - one outside the box reads the image itself and counts as 0 - and unrolled by the nine of a
            // plane, so that the loads of a plane are in flight together (all 27 at once would spill).  A corner thread walks 8 rows one after the other: with k_mg_stencil_apply's loop (a
            // round trip to memory per neighbour) it would hold every launch of every level for 8 x 27 round trips instead of 8 x 3, and the coarse levels are
            // nothing but latency.  The order of the sum is k_mg_stencil_apply's.
            double s[3] = { 0.0, 0.0, 0.0 };
#pragma unroll 1
            for (int dz = -1; dz <= 1; dz++)
#pragma unroll
            for (int q = 0; q < 9; q++) {
               const int dx = q % 3 - 1, dy = q / 3 - 1, o = q + 9 * (dz + 1);
               const bool in = (unsigned)(ii + dx) < (unsigned)C.n[0] && (unsigned)(jj + dy) < (unsigned)C.n[1] && (unsigned)(kk + dz) < (unsigned)C.n[2];
               const int64_t v = in ? u + dx + (int64_t)C.n[0] * (dy + (int64_t)C.n[1] * dz) : u;
               const double x0 = x[v], x1 = x[v + nn], x2 = x[v + 2 * nn];
               const double xv[3] = { in ? x0 : 0.0, in ? x1 : 0.0, in ? x2 : 0.0 };
#pragma unroll
               for (int r = 0; r < 3; r++)
#pragma unroll
                  for (int c = 0; c < 3; c++) s[r] += S[(o * 9 + 3 * r + c) * nn + u] * xv[c];
            }
#pragma unroll
            for (int r = 0; r < 3; r++) acc[r] += s[r];
         }
      }
   }
#pragma unroll
   for (int r = 0; r < 3; r++) y[t + nn * r] = acc[r];
}

// Reduced restriction of the periodic cell on one rank: r_c(I) = sum_j P_jI r_f(j) over the fine nodes within one step of I WITH wrap-around
// (fine index -1 is index n - 2, index n is index 1), from an assembled r_f (equal on the images of a node).  The wrapped neighbourhood holds
// every canonical fine node once, so no weights are needed; every image of I gathers the same values in the same order and so writes the same bits.
__global__ __launch_bounds__(MG_BS) void k_mg_restrict_periodic(const MgGrid F, const MgGrid C, const double* __restrict__ rf, double* __restrict__ rc) {
   const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
   const int64_t nnf = grid_nn(F), nnc = grid_nn(C);
   if (t >= nnc) return;
   const int I = (int)(t % C.n[0]), J = (int)((t / C.n[0]) % C.n[1]), K = (int)(t / ((int64_t)C.n[0] * C.n[1]));
   double s[3] = { 0.0, 0.0, 0.0 };
   for (int dz = -1; dz <= 1; dz++) {
      int fk = 2 * K + dz; if (fk < 0) fk += F.n[2] - 1; else if (fk >= F.n[2]) fk -= F.n[2] - 1;
      for (int dy = -1; dy <= 1; dy++) {
         int fj = 2 * J + dy; if (fj < 0) fj += F.n[1] - 1; else if (fj >= F.n[1]) fj -= F.n[1] - 1;
         for (int dx = -1; dx <= 1; dx++) {
            int fi = 2 * I + dx; if (fi < 0) fi += F.n[0] - 1; else if (fi >= F.n[0]) fi -= F.n[0] - 1;
            const int64_t v = fi + (int64_t)F.n[0] * (fj + (int64_t)F.n[1] * fk);
            const double wt = (dx ? 0.5 : 1.0) * (dy ? 0.5 : 1.0) * (dz ? 0.5 : 1.0);
#pragma unroll
            for (int c = 0; c < 3; c++) s[c] += wt * rf[v + nnf * c];
         }
      }
   }
#pragma unroll
   for (int c = 0; c < 3; c++) rc[t + nnc * c] = s[c];
}

// control block of the preconditioner under mixed loading: z = r / d on this rank's free control slots (at most 8; not hot)
__global__ void k_mg_control_block(const int n, const int32_t* __restrict__ slot, const double* __restrict__ dinv, const double* __restrict__ r, double* __restrict__ z) {
   const int t = threadIdx.x;
   if (t < n) z[slot[t]] = dinv[t] * r[slot[t]];
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

// is the level-l mask closed under P?  flag[0] <- 1 by every thread whose free coarse dof interpolates onto a masked fine dof (all write the same value)
__global__ __launch_bounds__(MG_BS) void k_mg_mask_closed(const MgGrid F, const MgGrid C, const uint8_t* __restrict__ mf, const uint8_t* __restrict__ mc, int32_t* __restrict__ flag) {
   const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
   const int64_t nnf = grid_nn(F), nnc = grid_nn(C);
   if (t >= nnc) return;
   const int I = (int)(t % C.n[0]), J = (int)((t / C.n[0]) % C.n[1]), K = (int)(t / ((int64_t)C.n[0] * C.n[1]));
   bool bad = false;
   for (int dz = -1; dz <= 1; dz++) {
      const int fk = 2 * K + dz; if (fk < 0 || fk >= F.n[2]) continue;
      for (int dy = -1; dy <= 1; dy++) {
         const int fj = 2 * J + dy; if (fj < 0 || fj >= F.n[1]) continue;
         for (int dx = -1; dx <= 1; dx++) {
            const int fi = 2 * I + dx; if (fi < 0 || fi >= F.n[0]) continue;
            const int64_t v = fi + (int64_t)F.n[0] * (fj + (int64_t)F.n[1] * fk);
#pragma unroll
            for (int c = 0; c < 3; c++) bad = bad || (!mc[t + nnc * c] && mf[v + nnf * c]);
         }
      }
   }
   if (bad) flag[0] = 1;
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

// start vector of the power iteration: a hash of the GLOBAL dof index in (0, 1], zero on essential dofs (the same vector on every decomposition).
// periodic: of the canonical coordinate (the last index of a direction is index 0), so that the images of a node start equal
__global__ __launch_bounds__(MG_BS) void k_mg_seed(const MgGrid C, const int ng0, const int ng1, const int ng2, const int periodic, const uint8_t* __restrict__ mask, double* __restrict__ v) {
   const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
   const int64_t nn = grid_nn(C);
   if (t >= nn) return;
   const int i = (int)(t % C.n[0]), j = (int)((t / C.n[0]) % C.n[1]), k = (int)(t / ((int64_t)C.n[0] * C.n[1]));
   int gi = C.g0[0] + i, gj = C.g0[1] + j, gk = C.g0[2] + k;
   if (periodic) { gi %= ng0 - 1; gj %= ng1 - 1; gk %= ng2 - 1; }
   const uint64_t g = (uint64_t)gi + (uint64_t)ng0 * ((uint64_t)gj + (uint64_t)ng1 * (uint64_t)gk);
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
void mg_stencil_apply_periodic(const MgGrid& C, const double* S, const double* x, double* y, hipStream_t s) {
   hipLaunchKernelGGL(k_mg_stencil_apply_periodic, dim3(blocks(grid_nn(C))), dim3(MG_BS), 0, s, C, S, x, y); launched("k_mg_stencil_apply_periodic");
}
void mg_restrict_periodic(const MgGrid& F, const MgGrid& C, const double* rf, double* rc, hipStream_t s) {
   hipLaunchKernelGGL(k_mg_restrict_periodic, dim3(blocks(grid_nn(C))), dim3(MG_BS), 0, s, F, C, rf, rc); launched("k_mg_restrict_periodic");
}
void mg_control_block(int n, const int32_t* slot, const double* dinv, const double* r, double* z, hipStream_t s) {
   if (n < 1) return;
   hipLaunchKernelGGL(k_mg_control_block, dim3(1), dim3(64), 0, s, n, slot, dinv, r, z); launched("k_mg_control_block");
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
void mg_mask_closed(const MgGrid& F, const MgGrid& C, const uint8_t* mf, const uint8_t* mc, int32_t* flag, hipStream_t s) {
   hipLaunchKernelGGL(k_mg_mask_closed, dim3(blocks(grid_nn(C))), dim3(MG_BS), 0, s, F, C, mf, mc, flag); launched("k_mg_mask_closed");
}
void mg_cheb(int64_t n, double* x, double* r, double* d, const double* Ad, const double* dinv, double c1, double c2, bool first, hipStream_t s) {
   hipLaunchKernelGGL(k_mg_cheb, dim3(blocks(n)), dim3(MG_BS), 0, s, n, x, r, d, Ad, dinv, c1, c2, first ? 1 : 0); launched("k_mg_cheb");
}
void mg_resid(int64_t n, const uint8_t* mask, const double* b, const double* y, double* r, hipStream_t s) {
   hipLaunchKernelGGL(k_mg_resid, dim3(blocks(n)), dim3(MG_BS), 0, s, n, mask, b, y, r); launched("k_mg_resid");
}
void mg_seed(const MgGrid& C, const int ng[3], bool periodic, const uint8_t* mask, double* v, hipStream_t s) {
   hipLaunchKernelGGL(k_mg_seed, dim3(blocks(grid_nn(C))), dim3(MG_BS), 0, s, C, ng[0], ng[1], ng[2], periodic ? 1 : 0, mask, v); launched("k_mg_seed");
}
void mg_to_fine(const MgGrid& F0, const MgGrid& C, int stride, const double* xc, double* x0, hipStream_t s) {
   hipLaunchKernelGGL(k_mg_to_fine, dim3(blocks(grid_nn(C))), dim3(MG_BS), 0, s, F0, C, stride, xc, x0); launched("k_mg_to_fine");
}
void mg_from_fine(const MgGrid& F0, const MgGrid& C, int stride, const double* x0, double* xc, hipStream_t s) {
   hipLaunchKernelGGL(k_mg_from_fine, dim3(blocks(grid_nn(C))), dim3(MG_BS), 0, s, F0, C, stride, x0, xc); launched("k_mg_from_fine");
}

}  // namespace exa_host

// private-memory bytes per lane of the two periodic kernels as the loaded code object reports them (both must be 0: nothing is spilled)
extern "C" int exa_mg_periodic_scratch_bytes(int* out2) {
   const void* f[2] = { reinterpret_cast<const void*>(exa_host::k_mg_stencil_apply_periodic), reinterpret_cast<const void*>(exa_host::k_mg_restrict_periodic) };
   for (int k = 0; k < 2; k++) {
      hipFuncAttributes a;
      if (hipFuncGetAttributes(&a, f[k]) != hipSuccess) { (void)hipGetLastError(); return -1; }
      out2[k] = (int)a.localSizeBytes;
   }
   return 0;
}
