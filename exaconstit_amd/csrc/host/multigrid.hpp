// Geometric multigrid V-cycle used as the PCG preconditioner on generated p = 1 meshes (Solvers.Krylov.preconditioner = "multigrid").
//
// Level 0 is the fine mesh and its operator is the constrained gradient action the PCG applies (NonlinearMechOperator::GradMult).  Level
// l >= 1 keeps every second node of level l - 1 in each direction of the rank's structured box (host/mesh.hpp).  P_l (level l -> l - 1) is
// trilinear interpolation, the level-l mask is the level l - 1 mask at the surviving nodes, and the coarse operator is the Galerkin product
// A_l = M_l P_l^T A_{l-1} P_l M_l, stored as a 27-point stencil of 3 x 3 blocks per node (mg_kernels.hip).
//
// The stencil of level l is obtained by probing the product: for each of the 27 node colours (global coordinates mod 3) and 3 components,
// the coloured coarse unit vector is interpolated, the level l - 1 operator is applied without the halo exchange, and the result is
// restricted.  Coarse nodes of one colour are at least 3 apart, so every stencil entry is read off exactly once.  Without the exchange the
// result is this rank's part of each row (the elements it holds), the same pattern as the fine action, and the stencil apply is followed by
// a halo sum.  Probing works on any gradient form the driver builds (compact records, 46-double records, element assembly), needs nothing
// but the action, and is exact: it evaluates the product, it does not approximate it.
//
// Smoother: Chebyshev on D^-1 A (the same polynomial before and after the coarse correction, so the V-cycle is symmetric), interval
// [0.3 * 1.2 lmax, 1.2 lmax], lmax from 10 power iterations started from a hash of the global dof index (the same vector on every
// decomposition), D^-1 = 0 on essential dofs.  The coarsest level runs the same smoother at degree 16 instead of a direct solve.
//
// Periodic cells ("periodic cells"): an image pair is a rank interface with oneself, so the stencils, probes and transfers of the
// build stay what they are (nodes taken as distinct, rows summed afterwards) and only the sums change.  One rank: the V-cycle runs the fused
// kernels mg_stencil_apply_periodic / mg_restrict_periodic (the sum over the images inside the launch).  Several ranks: the unfused kernels and
// NonlinearMechOperator::SumLVector at the fine positions (PeriodicCell::Sum), never both.  Mixed loading: the hierarchy is that of the fluctuation
// block (level-0 mask = essential set + every control slot), and Apply adds the control block z = r / d on the free control slots.
//
// p = 2 ("p = 2"; opt-in, Solvers.Krylov.mg_p2): the p = 2 node grid (2 ne + 1 nodes per direction) is level 0, the element vertices -
// every second node - are level 1, and the trilinear interpolation between them is the embedding Q1 in Q2, so the hierarchy is the one above with
// n = ((ne p) >> l) + 1.  The fine operator reaches two nodes: its diagonal is probed with the 27 colours mod 3.  Because Q1 in Q2, the level-1
// product is the trilinear rediscretisation on the p = 2 rule, and Build reads it - and the fine diagonal - off the point records of the action in
// one pass each (exa_grad_mg_p2_build) where those records exist and the essential set is closed under P; otherwise it probes as everywhere else.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>
#include "device_utils.hpp"
#include "mesh.hpp"

namespace exa_host {

struct MgGrid { int n[3]; int g0[3]; };   // local nodes per direction, global index of the first one (at this level)

// kernels (mg_kernels.hip)
void mg_prolong(const MgGrid& F, const MgGrid& C, const double* xc, double* yf, double beta, hipStream_t s);            // y_f = beta y_f + P x_c
void mg_restrict(const MgGrid& F, const MgGrid& C, const double* w, const double* rf, double* rc, hipStream_t s);        // r_c = P^T (w .* r_f)
void mg_stencil_apply(const MgGrid& C, const double* S, const double* x, double* y, hipStream_t s);
void mg_probe(const MgGrid& C, int m, int colour, int comp, const uint8_t* mask, double* x, hipStream_t s);
void mg_extract(const MgGrid& C, int colour, int comp, const double* y, double* S, hipStream_t s);
void mg_diag_probe(const MgGrid& C, int m, int colour, int comp, const double* y, double* diag, hipStream_t s);
void mg_stencil_diag(const MgGrid& C, const double* S, double* diag, hipStream_t s);
void mg_dinv(int64_t n, const uint8_t* mask, const double* diag, double* dinv, hipStream_t s);
void mg_mask_coarsen(const MgGrid& F, const MgGrid& C, const uint8_t* mf, uint8_t* mc, hipStream_t s);
void mg_cheb(int64_t n, double* x, double* r, double* d, const double* Ad, const double* dinv, double c1, double c2, bool first, hipStream_t s);
void mg_resid(int64_t n, const uint8_t* mask, const double* b, const double* y, double* r, hipStream_t s);
void mg_seed(const MgGrid& C, const int ng[3], bool periodic, const uint8_t* mask, double* v, hipStream_t s);   // periodic: hash of the canonical coordinate
// periodic cell on one rank: y = (sum over the images)(S x) written to every image, and the reduced restriction with wrap-around, one launch each
void mg_stencil_apply_periodic(const MgGrid& C, const double* S, const double* x, double* y, hipStream_t s);
void mg_restrict_periodic(const MgGrid& F, const MgGrid& C, const double* rf, double* rc, hipStream_t s);
void mg_control_block(int n, const int32_t* slot, const double* dinv, const double* r, double* z, hipStream_t s);                // z[slot] = dinv r[slot]
// flag[0] = 1 when a free dof of C has a masked dof of F in the support of its interpolation (flag zeroed by the caller): M_F P M_C = P M_C fails
void mg_mask_closed(const MgGrid& F, const MgGrid& C, const uint8_t* mf, const uint8_t* mc, int32_t* flag, hipStream_t s);
void mg_to_fine(const MgGrid& F0, const MgGrid& C, int stride, const double* xc, double* x0, hipStream_t s);
void mg_from_fine(const MgGrid& F0, const MgGrid& C, int stride, const double* x0, double* xc, hipStream_t s);

constexpr int MG_STENCIL = 243;        // doubles per node of a coarse operator
constexpr int MG_POWER_ITERS = 10;
constexpr int MG_COARSE_DEGREE = 16;

// Number of coarse levels of an N0 x N1 x N2 element box split over nranks (Partition::build): levels are added while every rank's local
// box stays divisible by 2^l and keeps at least 2 elements per direction; cap > 0 limits the count.  The same on every rank.
inline int mg_level_count(const int N[3], int nranks, int cap) {
   const auto pg = Partition::grid_for(nranks);
   int L = 1 << 20;
   for (int d = 0; d < 3; d++)
      for (int r = 0; r < pg[d]; r++) {
         int st = 0, ne = 0; Partition::split(N[d], pg[d], r, st, ne);
         int l = 0;
         while (ne % (2 << l) == 0 && ne / (2 << l) >= 2) l++;
         L = std::min(L, l);
      }
   return cap > 0 ? std::min(L, cap) : L;
}

// ... at polynomial order 2: level 1 is the trilinear space on the element vertices (every second node of the p = 2 node grid), which needs no
// evenness, and the levels below it are those of order 1; cap > 0 limits the count of coarse levels as before.  Order 1: mg_level_count.
inline int mg_level_count_order(const int N[3], int nranks, int cap, int order) {
   if (order == 1) return mg_level_count(N, nranks, cap);
   const int L = 1 + mg_level_count(N, nranks, 0);
   return cap > 0 ? std::min(L, cap) : L;
}

class NonlinearMechOperator;

class Multigrid {
 public:
   // throws when not even one coarse level can be built
   Multigrid(NonlinearMechOperator& op, int levels_cap, int degree);
   ~Multigrid();
   void Build();                                           // after every gradient set-up
   void Apply(const double* b, double* x);                 // x = B b, one V-cycle
   int levels() const { return (int)lv_.size() - 1; }       // coarse levels
   int degree() const { return degree_; }
   int levels_cap() const { return levels_cap_; }           // as asked for at construction (0: as many as the mesh allows)
   bool periodic() const { return periodic_; }
   int control_dofs() const { return control_dofs_; }      // free control entries of the control block (all ranks' count; 0 before the first Build)
   bool built() const { return built_; }
   // test hooks (level l of the hierarchy of the last Build): y = A_l x (level 0: the constrained fine operator), the diagonal, transfers
   void LevelApply(int l, const double* x, double* y);
   void LevelDiag(int l, double* out);                     // (mixed loading, level 0: d on the free control slots this rank holds)
   void Prolong(int l, const double* xc, double* xf);      // level l + 1 -> l
   void Restrict(int l, const double* rf, double* rc);     // level l -> l + 1: halo_sum(sum_local w_j P_jI r(j))
   int64_t level_dofs(int l) const { return lv_[l].nd; }
   const MgGrid& grid(int l) const { return lv_[l].g; }
   double lmax(int l) const { return lv_[l].lmax; }
   double setup_ms = 0.0;
   double vcycle_ms();
   const double* stencil(int l) const { return lv_[l].S.p; }
   int order(int l) const { return l == 0 ? p_ : 1; }       // polynomial order of level l
   bool bbar() const { return bbar_; }                      // the fine operator is the B-bar one (Solvers.Krylov.mg_bbar)
   int level1_build() const { return level1_build_; }       // p = 2, last Build: 1 level 1 and the fine diagonal from the point records, 0 probed; -1 at p = 1 / before
 private:
   bool BuildFromRecords();                                 // p = 2: false (nothing written) where the records cannot serve, see Build
   struct Level {
      MgGrid g{}; int64_t nn = 0, nd = 0; int stride = 1;
      DevBuf<double> S, diag, dinv, w, b, x, r, d, t, u, v;
      DevBuf<uint8_t> mask_own; const uint8_t* mask = nullptr; const double* wp = nullptr;
      double lmax = 0.0; int deg = 2;
   };
   void A(int l, const double* x, double* y);              // A_l x, halo-summed
   void ALocal(int l, const double* x, double* y);         // this rank's part
   void halo(int l, double* y);
   void BuildControlBlock();                               // mixed loading: the level-0 mask and the diagonal of the free control slots
   double dot(int l, const double* a, const double* b);
   void smooth(int l, const double* b, double* x);
   void vcycle(int l, const double* b, double* x);
   NonlinearMechOperator& op_;
   std::vector<Level> lv_;
   int degree_ = 2, levels_cap_ = 0; bool built_ = false;
   bool periodic_ = false, fused_ = false, mixed_ = false;  // fused_: periodic on one rank (the image sums run inside the coarse kernels)
   DevBuf<uint8_t> mask0_;                                  // mixed loading: essential set + the free control slots
   DevBuf<int32_t> ctrl_slot_; DevBuf<double> ctrl_dinv_; int ctrl_local_ = 0, control_dofs_ = 0;   // this rank's free control slots and 1 / d
   int64_t ctrl_at_[8] = {}; double ctrl_d_[8] = {};
   bool bbar_ = false;
   int p_ = 1, level1_build_ = -1;                          // order of level 0 (1 or 2)
   DevBuf<int32_t> elem_at_, closed_flag_;                  // p = 2: local element at every position of the element box; result of the mask check
   int ng_[3] = { 0, 0, 0 };                                // global elements per direction at level 0
   DevBuf<double> fine_tmp_, partial_, scal_;
   hipEvent_t ev0_ = nullptr, ev1_ = nullptr; bool ev_pending_ = false; double vcycle_ms_ = 0.0;
};

}  // namespace exa_host
