// Geometric multigrid preconditioner: hierarchy build and V-cycle (see multigrid.hpp; kernels in mg_kernels.hip).
#include "multigrid.hpp"
#include "driver.hpp"
#include <chrono>
#include <cmath>
#include <stdexcept>

namespace exa_host {

Multigrid::Multigrid(NonlinearMechOperator& op, int levels_cap, int degree) : op_(op), degree_(degree), levels_cap_(levels_cap) {
   const Partition& part = op.part();
   periodic_ = part.periodic; mixed_ = part.periodic && part.mixed; fused_ = part.periodic && !op.comm().active();
   // (p = 2: opt-in, the operator was told - SystemDriver::SetPreconditioner; without it the refusal of every order but 1 stands)
   if (part.from_file || part.geom != 0 || !(part.p == 1 || (part.p == 2 && op.mg_p2_allowed)))
      throw std::runtime_error("Solvers.Krylov.preconditioner = \"multigrid\" needs a generated mesh (Mesh.type = \"auto\") at p_refinement = 1");
   if (part.p == 2 && part.periodic) throw std::runtime_error(ExaOptions::mg_p2_no_periodic());
   // (B-bar: opt-in as well, Solvers.Krylov.mg_bbar; the hierarchy itself is built the same way - DESIGN 4.6, "B-bar")
   bbar_ = op.cfg_used.integ == EXA_INTEG_BBAR;
   if (bbar_ && !op.mg_bbar_allowed) throw std::runtime_error(ExaOptions::mg_no_bbar());
   if (bbar_ && part.periodic) throw std::runtime_error(ExaOptions::mg_bbar_no_periodic());
   p_ = part.p;
   if (degree < 1 || degree > 8) throw std::runtime_error("Solvers.Krylov.mg_smoother_degree must lie in 1 ... 8");
   if (levels_cap < 0) throw std::runtime_error("Solvers.Krylov.mg_levels must be >= 0 (0: as many as the mesh allows)");
   const int L = mg_level_count_order(part.N, part.nranks, levels_cap, p_);
   if (L < 1)
      throw std::runtime_error("Solvers.Krylov.preconditioner = \"multigrid\": no coarse level can be built for " + std::to_string(part.N[0]) + " x " + std::to_string(part.N[1]) + " x " +
                               std::to_string(part.N[2]) + " elements on " + std::to_string(part.nranks) + " rank(s) (every rank's element box must be even, with at least 2 elements per direction after coarsening)");
   for (int d = 0; d < 3; d++) ng_[d] = part.N[d];
   hipStream_t s = op.stream();
   lv_.resize(L + 1);
   for (int l = 0; l <= L; l++) {
      Level& v = lv_[l];
      v.stride = 1 << l;
      for (int d = 0; d < 3; d++) { v.g.n[d] = ((part.ne[d] * p_) >> l) + 1; v.g.g0[d] = (part.e0[d] * p_) >> l; }
      v.nn = (int64_t)v.g.n[0] * v.g.n[1] * v.g.n[2]; v.nd = 3 * v.nn;
      v.deg = l == L ? MG_COARSE_DEGREE : degree;
      v.diag.alloc(v.nd); v.dinv.alloc(v.nd); v.r.alloc(v.nd); v.d.alloc(v.nd); v.t.alloc(v.nd); v.u.alloc(v.nd); v.v.alloc(v.nd);
      if (l > 0) {
         v.S.alloc((size_t)MG_STENCIL * v.nn); v.b.alloc(v.nd); v.x.alloc(v.nd); v.mask_own.alloc(v.nd);
         v.mask = v.mask_own.p;
         std::vector<double> w((size_t)v.nn);      // node multiplicity weight = the fine node's
         for (int k = 0; k < v.g.n[2]; k++) for (int j = 0; j < v.g.n[1]; j++) for (int i = 0; i < v.g.n[0]; i++)
            w[i + (size_t)v.g.n[0] * (j + (size_t)v.g.n[1] * k)] = part.weight[(size_t)v.stride * i + (size_t)part.nn[0] * ((size_t)v.stride * j + (size_t)part.nn[1] * v.stride * k)];
         v.w.upload(w, s); v.wp = v.w.p;
      }
   }
   if ((int64_t)lv_[0].nn != part.NN) throw std::runtime_error("multigrid: the partition is not a structured box of its order");
   if (p_ == 2) {   // where every element of the box sits in the rank's element order (its first native node is its lowest vertex)
      std::vector<int32_t> at((size_t)part.E, -1);
      for (int e = 0; e < part.E; e++) {
         const int g = part.conn[(size_t)part.n * e];
         const int i = g % part.nn[0], j = (g / part.nn[0]) % part.nn[1], k = g / (part.nn[0] * part.nn[1]);
         if ((i | j | k) & 1) throw std::runtime_error("multigrid: the partition is not a structured p = 2 box");
         at[(size_t)(i >> 1) + (size_t)part.ne[0] * ((j >> 1) + (size_t)part.ne[1] * (k >> 1))] = e;
      }
      for (int32_t e : at) if (e < 0) throw std::runtime_error("multigrid: the partition is not a structured p = 2 box");
      elem_at_.upload(at, s); closed_flag_.alloc(1);
   }
   fine_tmp_.alloc(lv_[0].nd); partial_.alloc(DOT_BLOCKS * 4); scal_.alloc(4);
   if (mixed_) { mask0_.alloc(lv_[0].nd); ctrl_slot_.alloc(8); ctrl_dinv_.alloc(8); }
   EXA_HC(hipEventCreate(&ev0_)); EXA_HC(hipEventCreate(&ev1_));
}

Multigrid::~Multigrid() {
   if (ev0_) (void)hipEventDestroy(ev0_);
   if (ev1_) (void)hipEventDestroy(ev1_);
}

// coarse halo sum on the fine exchange plan: the level-l nodes are level-0 nodes, and the fine neighbour lists hold every shared one
void Multigrid::halo(int l, double* y) {
   Comm& comm = op_.comm();
   hipStream_t s = op_.stream();
   if (periodic_) {
      // Periodic partition: the sum over the local images, the ranks and back to the images is the cell's (PeriodicCell::Sum through SumLVector,
      // raw = false: no resultants).  On one rank this detour through a zeroed fine vector serves the build only (the diagonals): the V-cycle
      // runs the fused kernels and never comes here, so it is not hot.  On several ranks it is today's cost model of every coarse sum.
      if (l == 0) { op_.SumLVector(y, nullptr, false); return; }
      fine_tmp_.zero(s);
      mg_to_fine(lv_[0].g, lv_[l].g, lv_[l].stride, y, fine_tmp_.p, s);
      op_.SumLVector(fine_tmp_.p, nullptr, false);
      mg_from_fine(lv_[0].g, lv_[l].g, lv_[l].stride, fine_tmp_.p, y, s);
      return;
   }
   if (!comm.active()) return;
   if (l == 0) { comm.halo_sum(y, s); return; }
   fine_tmp_.zero(s);
   mg_to_fine(lv_[0].g, lv_[l].g, lv_[l].stride, y, fine_tmp_.p, s);
   comm.halo_sum(fine_tmp_.p, s);
   mg_from_fine(lv_[0].g, lv_[l].g, lv_[l].stride, fine_tmp_.p, y, s);
}

void Multigrid::ALocal(int l, const double* x, double* y) {
   if (l == 0 && mixed_) { op_.GradMultRaw(x, y, mask0_.p); vk_mask_zero(lv_[0].nd, mask0_.p, y, op_.stream()); }
   else if (l == 0) op_.GradMultLocal(x, y);
   else mg_stencil_apply(lv_[l].g, lv_[l].S.p, x, y, op_.stream());   // (periodic cells too: the probes act on the operator of distinct nodes)
}

void Multigrid::A(int l, const double* x, double* y) {
   if (l == 0 && mixed_) {
      // Fluctuation block M0 K M0 of a mixed partition: with every control slot masked the masked vector is its own expansion, so
      // the raw action on M0 x followed by the plain sums is NonlinearMechOperator::GradMult(M0 x) without its expansion and resultant launches
      op_.GradMultRaw(x, y, mask0_.p); op_.SumLVector(y, nullptr, false); vk_mask_zero(lv_[0].nd, mask0_.p, y, op_.stream());
      return;
   }
   if (l == 0) { op_.GradMult(x, y, true); return; }
   if (fused_) { mg_stencil_apply_periodic(lv_[l].g, lv_[l].S.p, x, y, op_.stream()); return; }
   mg_stencil_apply(lv_[l].g, lv_[l].S.p, x, y, op_.stream());
   halo(l, y);
}

// Mixed loading: the level-0 mask of the fluctuation block, and d = the diagonal entry of the reduced operator on every free
// control slot, read off one constrained action on its unit vector (at most 8 actions per build; the rank that holds the slot keeps 1 / d).
void Multigrid::BuildControlBlock() {
   hipStream_t s = op_.stream();
   const Partition& part = op_.part();
   Level& f = lv_[0];
   const uint32_t bits = op_.cell()->free_bits();
   EXA_HC(hipMemcpyAsync(mask0_.p, op_.ess_mask.p, f.nd, hipMemcpyDeviceToDevice, s));
   int32_t slot[8]; double dinv[8]; ctrl_local_ = 0; control_dofs_ = 0;
   for (int i = 0; i < 3; i++) for (int d = 0; d < 3; d++) {
      if (!(bits >> (3 * i + d) & 1u) || control_dofs_ == 8) continue;
      control_dofs_++;
      const int64_t at = part.ctrl_node[1 + d] >= 0 ? part.ctrl_node[1 + d] + f.nn * i : -1;   // (-1: another rank's)
      f.t.zero(s);
      const double one = 1.0; double dd = 0.0;
      if (at >= 0) EXA_HC(hipMemcpyAsync(f.t.p + at, &one, sizeof(double), hipMemcpyHostToDevice, s));
      op_.GradMult(f.t.p, f.u.p, true);
      if (at < 0) continue;
      EXA_HC(hipMemcpyAsync(&dd, f.u.p + at, sizeof(double), hipMemcpyDeviceToHost, s)); EXA_HC(hipStreamSynchronize(s));
      slot[ctrl_local_] = (int32_t)at; dinv[ctrl_local_] = dd > 0.0 ? 1.0 / dd : 0.0; ctrl_at_[ctrl_local_] = at; ctrl_d_[ctrl_local_] = dd; ctrl_local_++;
      EXA_HC(hipMemsetAsync(mask0_.p + at, 1, 1, s));
   }
   if (ctrl_local_ > 0) { ctrl_slot_.upload(slot, ctrl_local_, s); ctrl_dinv_.upload(dinv, ctrl_local_, s); EXA_HC(hipStreamSynchronize(s)); }
}

double Multigrid::dot(int l, const double* a, const double* b) {
   if (l == 0) return op_.dot(a, b);
   hipStream_t s = op_.stream();
   vk_dot(lv_[l].nd, lv_[l].nn, lv_[l].wp, a, b, nullptr, partial_.p, scal_.p, s);
   op_.comm().allreduce_sum(scal_.p, 1, s);
   double h; EXA_HC(hipMemcpyAsync(&h, scal_.p, sizeof(double), hipMemcpyDeviceToHost, s)); EXA_HC(hipStreamSynchronize(s));
   return h;
}

// p = 2: this rank's part of A_1 = M_1 P^T A_0 P M_1 and of diag(A_0) read off the point records of the action (exa_grad_mg_p2_build), the halo sums
// as after the probes.  Q1 in Q2 makes the product the trilinear rediscretisation, but only P^T K P: it equals P^T (M_0 K M_0) P on the free level-1
// dofs when none of them interpolates onto an essential fine dof, which is checked here on every rank (whole box faces pass: they sit at even
// indices).  False - nothing written, the caller probes - when the test hook asks for the probes, the action does not run from records
// (deterministic mode, EXA_TANGENT_RECORDS=off, assembled element matrices), the check fails on any rank, or the library has no such records.
bool Multigrid::BuildFromRecords() {
   if (op_.mg_p2_build == 0 || !op_.p2_records_readable()) return false;
   hipStream_t s = op_.stream();
   Level& f = lv_[0]; Level& c = lv_[1];
   closed_flag_.zero(s);
   mg_mask_closed(f.g, c.g, f.mask, c.mask, closed_flag_.p, s);
   int32_t open = 0; closed_flag_.download(&open, 1, s);
   if (op_.comm().max_over_ranks(open ? 1.0 : 0.0) != 0.0) return false;
   const Partition& part = op_.part();
   exa_ctx* ctx = op_.GetModel()->ctx();
   const int rc = exa_grad_mg_p2_build(ctx, part.ne, elem_at_.p, f.mask, c.mask, c.S.p, f.diag.p, s);
   // (a property of the context, the same on every rank)
   if (rc == EXA_ERR_UNSUPPORTED) return false;
   if (rc < 0) throw std::runtime_error(std::string("exa_grad_mg_p2_build: ") + exa_last_error(ctx));
   halo(0, f.diag.p);
   mg_stencil_diag(c.g, c.S.p, c.diag.p, s);
   halo(1, c.diag.p);
   return true;
}

void Multigrid::Build() {
   const auto t0 = std::chrono::steady_clock::now();
   hipStream_t s = op_.stream();
   const int L = levels();
   lv_[0].mask = op_.ess_mask.p; lv_[0].wp = op_.weight.p;
   if (mixed_) { BuildControlBlock(); lv_[0].mask = mask0_.p; }
   for (int l = 1; l <= L; l++) mg_mask_coarsen(lv_[l - 1].g, lv_[l].g, lv_[l - 1].mask, lv_[l].mask_own.p, s);
   // p = 2: level 1 and the fine diagonal in one pass each over the point records, where they can serve
   const bool from_records = p_ == 2 && BuildFromRecords();
   if (p_ == 2) level1_build_ = from_records ? 1 : 0;
   // fine diagonal: the fine operator couples nodes at most p apart, so probes of the (p + 1)^3 colours mod p + 1 (per component) read it off
   if (!from_records) {
      Level& f = lv_[0];
      const int m = p_ + 1;
      f.diag.zero(s);
      for (int colour = 0; colour < m * m * m; colour++)
         for (int c = 0; c < 3; c++) {
            mg_probe(f.g, m, colour, c, f.mask, f.t.p, s);
            A(0, f.t.p, f.u.p);
            mg_diag_probe(f.g, m, colour, c, f.u.p, f.diag.p, s);
         }
   }
   // Galerkin stencils, level by level: probe, interpolate, this rank's part of the level l - 1 action, restrict, mask, read off
   for (int l = 1; l <= L; l++) {
      Level& c = lv_[l]; Level& f = lv_[l - 1];
      if (l == 1 && from_records) continue;
      for (int colour = 0; colour < 27; colour++)
         for (int k = 0; k < 3; k++) {
            mg_probe(c.g, 3, colour, k, c.mask, c.x.p, s);
            mg_prolong(f.g, c.g, c.x.p, f.t.p, 0.0, s);
            ALocal(l - 1, f.t.p, f.u.p);
            mg_restrict(f.g, c.g, nullptr, f.u.p, c.r.p, s);
            vk_mask_zero(c.nd, c.mask, c.r.p, s);
            mg_extract(c.g, colour, k, c.r.p, c.S.p, s);
         }
      mg_stencil_diag(c.g, c.S.p, c.diag.p, s);
      halo(l, c.diag.p);
   }
   // D^-1 and the largest eigenvalue of D^-1 A per level (power iteration from the same start vector on every decomposition)
   for (int l = 0; l <= L; l++) {
      Level& v = lv_[l];
      mg_dinv(v.nd, v.mask, v.diag.p, v.dinv.p, s);
      int ng[3]; for (int d = 0; d < 3; d++) ng[d] = ((ng_[d] * p_) >> l) + 1;
      mg_seed(v.g, ng, periodic_, v.mask, v.v.p, s);
      double lam = 0.0;
      for (int it = 0; it < MG_POWER_ITERS; it++) {
         const double nrm = std::sqrt(dot(l, v.v.p, v.v.p));
         if (!(nrm > 0.0)) break;
         vk_axpby(v.nd, 0.0, v.v.p, 1.0 / nrm, v.v.p, s);
         A(l, v.v.p, v.t.p);
         vk_pointwise(v.nd, v.dinv.p, v.t.p, v.u.p, s);
         lam = dot(l, v.v.p, v.u.p);
         v.v.swap(v.u);
      }
      v.lmax = lam;
   }
   EXA_HC(hipStreamSynchronize(s));
   setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
   built_ = true;
}

// Chebyshev smoother with zero initial guess: x = p(D^-1 A) D^-1 b, degree lv_[l].deg (Saad, Iterative Methods, Alg. 12.1)
void Multigrid::smooth(int l, const double* b, double* x) {
   Level& v = lv_[l];
   hipStream_t s = op_.stream();
   const double hi = 1.2 * v.lmax, lo = 0.3 * hi;
   const double theta = 0.5 * (hi + lo), delta = 0.5 * (hi - lo), sigma = theta / delta;
   double rho = 1.0 / sigma;
   EXA_HC(hipMemcpyAsync(v.r.p, b, sizeof(double) * v.nd, hipMemcpyDeviceToDevice, s));
   if (!(v.lmax > 0.0)) { EXA_HC(hipMemsetAsync(x, 0, sizeof(double) * v.nd, s)); return; }
   mg_cheb(v.nd, x, v.r.p, v.d.p, nullptr, v.dinv.p, 0.0, 1.0 / theta, true, s);
   for (int k = 1; k < v.deg; k++) {
      A(l, v.d.p, v.t.p);
      const double rho1 = 1.0 / (2.0 * sigma - rho);
      mg_cheb(v.nd, x, v.r.p, v.d.p, v.t.p, v.dinv.p, rho1 * rho, 2.0 * rho1 / delta, false, s);
      rho = rho1;
   }
}

void Multigrid::vcycle(int l, const double* b, double* x) {
   Level& v = lv_[l];
   hipStream_t s = op_.stream();
   if (l == levels()) { smooth(l, b, x); return; }
   Level& c = lv_[l + 1];
   smooth(l, b, x);                                        // pre-smoothing
   A(l, x, v.t.p); mg_resid(v.nd, v.mask, b, v.t.p, v.u.p, s);
   Restrict(l, v.u.p, c.b.p);
   vk_mask_zero(c.nd, c.mask, c.b.p, s);                   // (M P)^T r: the transpose of the masked prolongation below
   vcycle(l + 1, c.b.p, c.x.p);                            // coarse correction
   mg_prolong(v.g, c.g, c.x.p, x, 1.0, s);
   vk_mask_zero(v.nd, v.mask, x, s);
   A(l, x, v.t.p); mg_resid(v.nd, v.mask, b, v.t.p, v.u.p, s);
   smooth(l, v.u.p, v.v.p);                                // post-smoothing: the same polynomial
   vk_axpby(v.nd, 1.0, v.v.p, 1.0, x, s);
}

void Multigrid::Apply(const double* b, double* x) {
   if (!built_) throw std::runtime_error("multigrid: the hierarchy has not been built (no gradient set-up yet)");
   hipStream_t s = op_.stream();
   EXA_HC(hipEventRecord(ev0_, s));
   vcycle(0, b, x);
   if (mixed_) mg_control_block(ctrl_local_, ctrl_slot_.p, ctrl_dinv_.p, b, x, s);   // block-diagonal: z = r / d on the free control slots
   EXA_HC(hipEventRecord(ev1_, s));
   ev_pending_ = true;
}

double Multigrid::vcycle_ms() {
   if (ev_pending_) {
      EXA_HC(hipEventSynchronize(ev1_));
      float ms = 0; EXA_HC(hipEventElapsedTime(&ms, ev0_, ev1_)); vcycle_ms_ = ms; ev_pending_ = false;
   }
   return vcycle_ms_;
}

void Multigrid::LevelApply(int l, const double* x, double* y) {
   if (l < 0 || l > levels()) throw std::runtime_error("multigrid: no level " + std::to_string(l));
   if (l > 0 && !built_) throw std::runtime_error("multigrid: the hierarchy has not been built (no gradient set-up yet)");
   A(l, x, y);
}
void Multigrid::LevelDiag(int l, double* out) {
   if (l < 0 || l > levels()) throw std::runtime_error("multigrid: no level " + std::to_string(l));
   if (!built_) throw std::runtime_error("multigrid: the hierarchy has not been built (no gradient set-up yet)");
   EXA_HC(hipMemcpyAsync(out, lv_[l].diag.p, sizeof(double) * lv_[l].nd, hipMemcpyDeviceToDevice, op_.stream()));
   // mixed loading: the diagonal of the control block on this rank's free control slots (the fluctuation block has zeros there)
   if (l == 0 && mixed_) {
      for (int k = 0; k < ctrl_local_; k++) EXA_HC(hipMemcpyAsync(out + ctrl_at_[k], &ctrl_d_[k], sizeof(double), hipMemcpyHostToDevice, op_.stream()));
      EXA_HC(hipStreamSynchronize(op_.stream()));
   }
}
void Multigrid::Prolong(int l, const double* xc, double* xf) {
   if (l < 0 || l >= levels()) throw std::runtime_error("multigrid: no transfer below level " + std::to_string(l));
   mg_prolong(lv_[l].g, lv_[l + 1].g, xc, xf, 0.0, op_.stream());
}
void Multigrid::Restrict(int l, const double* rf, double* rc) {
   if (l < 0 || l >= levels()) throw std::runtime_error("multigrid: no transfer below level " + std::to_string(l));
   const Level& f = lv_[l];
   if (fused_) { mg_restrict_periodic(f.g, lv_[l + 1].g, rf, rc, op_.stream()); return; }
   mg_restrict(f.g, lv_[l + 1].g, !(periodic_ || op_.comm().active()) ? nullptr : (l == 0 ? op_.weight.p : f.wp), rf, rc, op_.stream());
   halo(l + 1, rc);
}

}  // namespace exa_host
