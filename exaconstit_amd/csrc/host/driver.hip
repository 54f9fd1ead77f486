// Implementation of the stand-alone host driver (see driver.hpp for the reference classes each part follows).
#include "driver.hpp"
#include "multigrid.hpp"
#include "roctx.hpp"
#include <chrono>
#include <memory>
#include <sys/stat.h>
#include <algorithm>
#include <cmath>
#include <limits>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <iostream>

extern "C" const int* exa_model_fail_counter_dev(exa_ctx* ctx);
extern "C" int exa_grad_apply_lvec_blocks(exa_ctx* ctx, const double* x, double* y, const uint8_t* mask, const double* gate, int blk0, int nblk, exa_stream s);
int exa_grad_refresh_bbar(exa_ctx* ctx, const double* J, hipStream_t s);   // gen_kernels.hip (driver-internal)
int exa_tet_set_fused_action(exa_ctx* ctx, int on);                        // tet_kernels.hip (driver-internal)
extern "C" int exa_grad_apply_lvec_gated(exa_ctx* ctx, const double* x, double* y, const uint8_t* mask, const double* gate, exa_stream s);
extern "C" int exa_grad_apply_lvec_cols_w(exa_ctx* ctx, int nch, int ncols, const double* x, int64_t ldx, double* y, int64_t ldy, const uint8_t* mask, const double* const* gates, exa_stream s);


namespace exa_host {

// =====================================================================================================================
// model seam
// =====================================================================================================================
static void abi_check(exa_ctx* ctx, int rc, const char* what) { if (rc < 0) throw std::runtime_error(std::string(what) + ": " + exa_last_error(ctx)); }

void ExaCMechModel::ModelSetupLVec(const double* x_lvec, const double* v_lvec, double* jacobian_out, hipStream_t s) {
   abi_check(ctx_, exa_model_setup_lvec(ctx_, dt_, x_lvec, v_lvec, stress0_->p, matVars0_->p, stress1_->p, matVars1_->p, matGrad_->p, jacobian_out, s), "exa_model_setup_lvec");
}
void ExaCMechModel::ModelSetupLVecRecords(const double* x_lvec, const double* v_lvec, double* jacobian_out, hipStream_t s) {
   abi_check(ctx_, exa_model_setup_lvec_records(ctx_, dt_, x_lvec, v_lvec, stress0_->p, matVars0_->p, stress1_->p, matVars1_->p, jacobian_out, s), "exa_model_setup_lvec_records");
}
void ExaCMechModel::calcDpMat(double* dp, hipStream_t s) const { abi_check(ctx_, exa_calc_dp(ctx_, matVars1_->p, dp, s), "exa_calc_dp"); }

// =====================================================================================================================
// NonlinearMechOperator
// =====================================================================================================================
static bool is_bbar(const ExaOptions& o) { return ExaOptions::lower(o.integ_model) == "bbar"; }
// what the route decision (host/routes.hpp) needs from options, partition and transport
static RouteFacts route_facts(const ExaOptions& o, const Partition& part, const Comm& comm) {
   RouteFacts f;
   f.geom = part.geom; f.order = part.p; f.bbar = is_bbar(o); f.ea = o.assembly == Assembly::EA;
   f.slip = o.slip == SlipType::POWERVOCE ? RouteFacts::VOCE : (o.slip == SlipType::POWERVOCENL ? RouteFacts::VOCE_NL : RouteFacts::KMDD);
   f.several_ranks = comm.nranks > 1; f.rccl = comm.kind() == Comm::RCCL;
   f.has_bdr_blocks = part.E_bdr > 0; f.has_nbrs = !part.nbrs.empty(); f.periodic = part.periodic;
   return f;
}
static int model_id(const ExaOptions& o) {
   const bool bcc = o.xtal == XtalType::BCC;
   switch (o.slip) {
      case SlipType::POWERVOCE: return bcc ? EXA_BCC_VOCE : EXA_FCC_VOCE;
      case SlipType::POWERVOCENL: return bcc ? EXA_BCC_VOCE_NL : EXA_FCC_VOCE_NL;
      default: return bcc ? EXA_BCC_KMDD : EXA_FCC_KMDD;
   }
}

NonlinearMechOperator::NonlinearMechOperator(const ExaOptions& opt, const Partition& part, Comm& comm, const std::vector<double>& props,
                                             const std::vector<double>& quats_per_elem)
   : opt_(opt), part_(part), comm_(comm), routes_(decide_routes(route_facts(opt, part, comm), RouteSwitches::from_env())) {
   EXA_HC(hipStreamCreate(&stream_)); EXA_HC(hipEventCreate(&ev0_)); EXA_HC(hipEventCreate(&ev1_));
   const bool bbar = is_bbar(opt);
   const bool tet = part.geom == 1;
   if (tet && bbar) throw std::runtime_error("integ_model = \"BBAR\" is built for hexahedral meshes only (this mesh has tetrahedra)");
   exa_config cfg; cfg.model = model_id(opt); cfg.nprops = (int)props.size(); cfg.props = props.data(); cfg.temp_k = opt.temp_k; cfg.order = part.p;
   cfg.nelems = part.E; cfg.assembly = opt.assembly == Assembly::PA ? EXA_ASSEMBLY_PA : EXA_ASSEMBLY_EA; cfg.integ = bbar ? EXA_INTEG_BBAR : EXA_INTEG_FULL; cfg.device = -1;
   int err = 0; ctx_ = exa_create_geom(&cfg, tet ? EXA_GEOM_TET : EXA_GEOM_HEX, &err);
   if (!ctx_) throw std::runtime_error("exa_create failed (" + std::to_string(err) + ")");
   this->props = props; cfg_used = cfg; cfg_used.props = nullptr;
   nn_ = part.NN; nd_ = 3 * nn_; E_ = part.E; npe_ = part.n;
   const OperatorRoutes& r = routes_;
   compact_tangent_ = r.compact_tangent; newton_cap_ = r.newton_cap; newton_cap2_ = r.newton_cap2;
   if (r.ea_matrix_free) abi_check(ctx_, exa_set_ea_matrix_free(ctx_, 1), "exa_set_ea_matrix_free");
   if (tet) abi_check(ctx_, exa_tet_set_fused_action(ctx_, r.tet_fused ? 1 : 0), "exa_tet_set_fused_action");
   if (r.compact_tangent) abi_check(ctx_, exa_set_tangent_form(ctx_, EXA_TANGENT_DEV5_BULK), "exa_set_tangent_form");
   if (r.det) { abi_check(ctx_, exa_set_deterministic(ctx_, 1), "exa_set_deterministic"); comm_.deterministic = true; }
   abi_check(ctx_, exa_set_newton_caps(ctx_, newton_cap_, newton_cap2_, r.tail_resume ? 1 : 0), "exa_set_newton_caps");   // A/B switch for measurements; the fused launch is the product path
   abi_check(ctx_, exa_set_lean_state(ctx_, r.lean_state ? 1 : 0), "exa_set_lean_state");
   if (r.qlayout_eb64) abi_check(ctx_, exa_set_quadrature_layout(ctx_, EXA_QLAYOUT_EB64), "exa_set_quadrature_layout");
   auto qf = [&](int vdim) { return (size_t)exa_qf_size(ctx_, vdim); };
   conn.upload(part.conn); abi_check(ctx_, exa_set_connectivity(ctx_, conn.p, nn_), "exa_set_connectivity");
   x_ref.upload(part.X); x_beg.upload(part.X); x_cur.upload(part.X);
   weight.upload(part.weight);
   el_x.alloc(3 * (size_t)npe_ * E_); el_y_.alloc(3 * (size_t)npe_ * E_); el_jac.alloc(qf(9));
   stress0.alloc(qf(6)); stress1.alloc(qf(6)); matVars0.alloc(qf(28)); matVars1.alloc(qf(28));
   if (!r.records_setup) { matGrad.alloc(qf(36)); matGrad.zero(); }   // (allocated on demand if the records route is left, see SetPrecond)
   stress0.zero(); stress1.zero(); matVars1.zero();
   diag.alloc(nd_); dinv.alloc(nd_); tmp_l_.alloc(nd_); tmp_r_.alloc(nd_); el_x2_.alloc(3 * (size_t)npe_ * E_); ess_mask.alloc(nd_); ess_mask.zero();
   partial.alloc(DOT_BLOCKS * 4); scal.alloc(SCAL_LEN); scal.zero();
   { DevBuf<double> q; q.upload(quats_per_elem); abi_check(ctx_, exa_init_state(ctx_, matVars0.p, q.p, stream_), "exa_init_state"); EXA_HC(hipStreamSynchronize(stream_)); }
   model_.reset(new ExaCMechModel(ctx_, &stress0, &stress1, &matGrad, &matVars0, &matVars1));
   comm_.setup_halo(part);
   // the overlapped halo exchange is decided collectively: every rank runs the same form (a partition in which one rank has no boundary block
   // would otherwise put its exchange on another stream than its peers')
   overlap_ = r.overlap_wish;
   if (comm.nranks > 1) overlap_ = comm.max_over_ranks(overlap_ ? 0.0 : 1.0) == 0.0;
   nblk_bdr_ = (part.E_bdr + 63) / 64;
   if (part.periodic) SetupPeriodic();
}

// Periodic partition (Partition::make_periodic): the weights and the halo lists of the partition as it is now, and the cell's tables
void NonlinearMechOperator::SetupPeriodic() {
   weight.upload(part_.weight);
   comm_.setup_halo(part_);
   overlap_ = false;
   if (!cell_) cell_.reset(new PeriodicCell(part_, comm_, stream_));
   cell_->Build();
}

void NonlinearMechOperator::SumLVector(double* y, const double* flag, bool raw) {
   if (!part_.periodic) { comm_.halo_sum(y, stream_); return; }
   cell_->Sum(y, flag, raw);
}

void NonlinearMechOperator::UpdateEndCoords(const double* k) { vk_update_coords(nd_, x_beg.p, k, dt_, x_cur.p, stream_); }

void NonlinearMechOperator::ensure_mat_grad() { if (matGrad.n == 0) { matGrad.alloc((size_t)exa_qf_size(ctx_, 36)); matGrad.zero(stream_); } }

NonlinearMechOperator::~NonlinearMechOperator() {
   exa_destroy(ctx_); (void)hipEventDestroy(ev0_); (void)hipEventDestroy(ev1_);
   for (EvPair& e : ev_ring_) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
   (void)hipStreamDestroy(stream_);
}

void NonlinearMechOperator::SetCapState(int cap, int cap2) {
   if (!routes_.cap_auto) return;   // a fixed cap (EXA_NEWTON_CAP) or none: nothing follows the run
   newton_cap_ = cap; newton_cap2_ = cap2;
   abi_check(ctx_, exa_set_newton_caps(ctx_, newton_cap_, newton_cap2_, routes_.tail_resume ? 1 : 0), "exa_set_newton_caps");
}

void NonlinearMechOperator::UpdateEssTDofs(const std::vector<uint8_t>& mask) { ess_mask.upload(mask); }

template <bool upd_crds>
void NonlinearMechOperator::Setup(const double* k) {
   if (upd_crds) vk_update_coords(nd_, x_beg.p, k, dt_, x_cur.p, stream_);   // ExaModel::UpdateEndCoords (halo copies stay consistent)
   ProfRegion prof("ecmech_kernel");   // reference: CALI_MARK_BEGIN("ecmech_kernel"), src/mechanics_ecmech.cpp:237
   // No host synchronisation in here: the launch is timed by a ring of event pairs that is read back lazily (FlushModelTimers) and a failed
   // local solve poisons the residual norm ON THE DEVICE (ResidualNorm), which is also where the count reaches the host.  At 64^3 elements
   // per rank the launch is 0.6 ms: an event wait plus a status read-back per evaluation (round 2) was ~10 % of it.
   EvPair& ev = NextModelTimer();
   EXA_HC(hipEventRecord(ev.a, stream_));
   // ... and AssembleGradPA: the launch writes the action's point records.  With the L-vector residual both integrator actions take the geometry
   // from x_cur, so no Jacobian field is written (72 of 848 B per point); UpdateModel refreshes it once per step for the volume averages
   if (use_records()) { model_->ModelSetupLVecRecords(x_cur.p, k, routes_.geo_resid ? nullptr : el_jac.p, stream_); jac_stale_ = routes_.geo_resid; MarkRates(matVars1.p, exa_get_lean_state(ctx_) == 1); }
   else { ensure_mat_grad(); model_->ModelSetupLVec(x_cur.p, k, el_jac.p, stream_); jac_stale_ = false; MarkRates(matVars1.p, false); }   // L->E of x and v + SetupJacobianTerms inside the constitutive launch
   EXA_HC(hipEventRecord(ev.b, stream_)); ev.pending = true;
   timers.qpt_updates += (int64_t)E_ * exa_qpts_per_elem(ctx_); model_calls++;
   model_status_pending_ = true;
   if (routes_.nfev_log) {
      int h[64]; abi_check(ctx_, exa_model_nfev_hist(ctx_, matVars1.p, h, stream_), "exa_model_nfev_hist");
      std::fprintf(stderr, "nfev_hist call %ld dt %.4g cap %d tail %d:", (long)model_calls, dt_, newton_cap_, newton_cap_ > 0 ? exa_model_tail_count(ctx_, stream_) : 0);
      for (int i = 0; i < 64; i++) if (h[i]) std::fprintf(stderr, " %d:%d", i, h[i]);
      std::fprintf(stderr, "\n");
   }
   if (routes_.cap_auto && (model_calls <= 4 || model_calls % 4 == 0)) {   // tail split: next cap from the evaluation counts of this launch (the distribution drifts slowly)
      int h[64]; abi_check(ctx_, exa_model_nfev_hist(ctx_, matVars1.p, h, stream_), "exa_model_nfev_hist");
      // (one dense launch: measured at 128^3, a second level loses - FCC 5: 18.0 ms, 5+11: 19.0, 4+6: 21.1; BCC 4: 9.7, 3+5: 13.1 - because
      //  the dense launches pay for scattered 8-byte accesses into the blocked rows, not for idle lanes; EXA_NEWTON_CAP=K,K2 runs two levels)
      newton_cap_ = choose_newton_cap(h, routes_.tail_cost); newton_cap2_ = 0;
      abi_check(ctx_, exa_set_newton_caps(ctx_, newton_cap_, newton_cap2_, routes_.tail_resume ? 1 : 0), "exa_set_newton_caps");
   }
}
template void NonlinearMechOperator::Setup<true>(const double*);
template void NonlinearMechOperator::Setup<false>(const double*);

void NonlinearMechOperator::MarkRates(const double* p, bool pending) {
   for (const double*& r : rates_pending_) if (r == p) r = nullptr;
   if (!pending) return;
   for (const double*& r : rates_pending_) if (!r) { r = p; return; }
   throw std::runtime_error("lean state: more than two state arrays wait for their slip rates");
}
void NonlinearMechOperator::EnsureSlipRates(const DevBuf<double>& buf) {
   if (!RatesPending(buf)) return;
   abi_check(ctx_, exa_slip_rates_from_state(ctx_, buf.p, stream_), "exa_slip_rates_from_state");
   MarkRates(buf.p, false); rate_launches++;
}

NonlinearMechOperator::EvPair& NonlinearMechOperator::NextModelTimer() {
   if (ev_ring_.empty()) { ev_ring_.resize(64); for (EvPair& e : ev_ring_) { EXA_HC(hipEventCreate(&e.a)); EXA_HC(hipEventCreate(&e.b)); } }
   EvPair& e = ev_ring_[ev_head_]; ev_head_ = (ev_head_ + 1) % (int)ev_ring_.size();
   if (e.pending) ReadTimer(e);
   e.call = model_calls + 1;
   return e;
}
void NonlinearMechOperator::ReadTimer(EvPair& e) {
   EXA_HC(hipEventSynchronize(e.b)); float ms = 0; EXA_HC(hipEventElapsedTime(&ms, e.a, e.b)); timers.t_model_ms += ms; e.pending = false;
   if (routes_.model_times) std::fprintf(stderr, "model_launch call %ld: %.4f ms\n", e.call, ms);
}
// adds the launches timed since the last call to timers.t_model_ms (waits for the last of them)
void NonlinearMechOperator::FlushModelTimers() {
   for (EvPair& e : ev_ring_) if (e.pending) ReadTimer(e);
}
// failed local solves of the last constitutive launch, for callers that do not go through ResidualNorm (one 4-byte read-back + sync)
void NonlinearMechOperator::ReadModelStatus() {
   if (!model_status_pending_) return;
   model_fail = exa_model_status(ctx_, stream_);
   if (model_fail < 0) abi_check(ctx_, model_fail, "exa_model_status");
   model_fail_total += model_fail; model_status_pending_ = false;
}

void NonlinearMechOperator::ResidualAction(double* y) {
   EXA_HC(hipMemsetAsync(y, 0, sizeof(double) * nd_, stream_));
   if (routes_.lvec_resid && jac_stale_) {   // geometry from the nodes of the configuration the stress belongs to
      abi_check(ctx_, exa_grad_set_coords(ctx_, x_cur.p), "exa_grad_set_coords");
      abi_check(ctx_, exa_residual_lvec(ctx_, nullptr, stress1.p, y, stream_), "exa_residual_lvec");
   } else if (routes_.lvec_resid) abi_check(ctx_, exa_residual_lvec(ctx_, el_jac.p, stress1.p, y, stream_), "exa_residual_lvec");
   else {   // Hform->Setup() = AssemblePA, Hform->Mult = L->E, AddMultPA, E->L
      abi_check(ctx_, exa_residual_setup(ctx_, el_jac.p, stress1.p, stream_), "exa_residual_setup");
      el_y_.zero(stream_);
      abi_check(ctx_, exa_residual_apply(ctx_, el_y_.p, stream_), "exa_residual_apply");
      abi_check(ctx_, exa_restrict_transpose_add(ctx_, el_y_.p, y, stream_), "exa_restrict_transpose_add");
   }
   SumLVector(y);
   if (cell_) { cell_->OwnerBits(y); cell_->KeepResultants(); }   // several ranks: one copy of every entry; mixed loading: the resultants of this residual
   vk_mask_zero(nd_, ess_mask.p, y, stream_);
}

void NonlinearMechOperator::Mult(const double* k, double* y) { Setup<true>(k); ResidualAction(y); }

// Jacobians of the current configuration when the constitutive launch did not write them (record route): L->E of x_cur + SetupJacobianTerms
void NonlinearMechOperator::RefreshJacobians() {
   if (!jac_stale_) return;
   abi_check(ctx_, exa_restrict(ctx_, x_cur.p, el_x.p, stream_), "exa_restrict");
   abi_check(ctx_, exa_jacobians(ctx_, el_x.p, el_jac.p, stream_), "exa_jacobians");
   jac_stale_ = false;
}

void NonlinearMechOperator::GetGradient() {
   if (use_records()) {   // the constitutive launch of the last residual evaluation wrote the records of this state; the action recomputes the geometry from x_cur
      abi_check(ctx_, exa_grad_set_coords(ctx_, x_cur.p), "exa_grad_set_coords");
      // (B-bar, p = 2: the element-average gradients the action reads; the residual refreshes them as well, but GetUpdateBCsAction applies the gradient first)
      if (!routes_.fast_p1) abi_check(ctx_, exa_grad_refresh_bbar(ctx_, el_jac.p, stream_), "exa_grad_refresh_bbar");
      vk_jacobi_setup(nd_, ess_mask.p, diag.p, 1, dinv.p, stream_);
      // (B-bar multigrid at p = 2: the records build reads eDS next to the records - refreshed two lines up, on the same stream, for the state the
      //  records belong to; the probes go through the action, which reads the same eDS.  The tangent-field routes below refresh it in exa_grad_setup)
      if (precond == Precond::MULTIGRID) mg->Build();
      return;
   }
   // compact tangent form of the p = 1 PA action (include/exaconstit_hip.h): valid for ExaCMech tangents; verified on the data of
   // every call (one pass over the tangent field, one 8-byte read-back per Newton iteration) and dropped for good if it ever fails
   if (compact_tangent_) {
      double defect = 0.0;
      abi_check(ctx_, exa_grad_tangent_defect(ctx_, matGrad.p, &defect, stream_), "exa_grad_tangent_defect");
      if (!(defect < 1e-11)) {
         compact_tangent_ = false;
         abi_check(ctx_, exa_set_tangent_form(ctx_, EXA_TANGENT_FULL), "exa_set_tangent_form");
         if (comm_.rank == 0) std::cerr << "tangent is not of the deviatoric-block + bulk form (defect " << defect << "): streaming the full tangent\n";
      }
   }
   abi_check(ctx_, exa_grad_setup(ctx_, dt_, el_jac.p, matGrad.p, stream_), "exa_grad_setup");
   // geometry of the action recomputed from x_cur (unchanged until the next residual evaluation); EXA_APPLY_GEO=off streams it instead
   if (routes_.grad_set_coords) abi_check(ctx_, exa_grad_set_coords(ctx_, x_cur.p), "exa_grad_set_coords");   // read by the record-based actions (PA, matrix-free EA) only
   // The reference assembles the operator diagonal here on every call, but its Jacobi smoother never reads it (dinv is built once
   // from diag = 1).  With that default the assembly is skipped: no result depends on it, and for p = 2 element
   // assembly it would be the only consumer of the 81 x 81 matrices.
   if (precond == Precond::JACOBI) {
      el_y_.zero(stream_);
      abi_check(ctx_, exa_grad_diagonal(ctx_, el_y_.p, stream_), "exa_grad_diagonal");
      diag.zero(stream_);
      abi_check(ctx_, exa_restrict_transpose_add(ctx_, el_y_.p, diag.p, stream_), "exa_restrict_transpose_add");
      SumLVector(diag.p);
      vk_mask_one(nd_, ess_mask.p, diag.p, stream_);
   }
   vk_jacobi_setup(nd_, ess_mask.p, diag.p, precond == Precond::JACOBI ? 0 : 1, dinv.p, stream_);
   if (precond == Precond::MULTIGRID) mg->Build();
}

// generic-order partial assembly, added into y: mask, L->E, AddMultGradPA, E->L (spec reference src/mechanics_operator_ext.cpp:143-157)
void NonlinearMechOperator::ElementAction(const double* x, const uint8_t* in_mask, double* y) {
   EXA_HC(hipMemcpyAsync(tmp_l_.p, x, sizeof(double) * nd_, hipMemcpyDeviceToDevice, stream_));
   if (in_mask) vk_mask_zero(nd_, in_mask, tmp_l_.p, stream_);
   abi_check(ctx_, exa_restrict(ctx_, tmp_l_.p, el_x2_.p, stream_), "exa_restrict");
   el_y_.zero(stream_);
   abi_check(ctx_, exa_grad_apply(ctx_, el_x2_.p, el_y_.p, stream_), "exa_grad_apply");
   abi_check(ctx_, exa_restrict_transpose_add(ctx_, el_y_.p, y, stream_), "exa_restrict_transpose_add");
}

void NonlinearMechOperator::GradMultLocal(const double* x, double* y) {
   GradMultRaw(x, y, ess_mask.p);
   vk_mask_zero(nd_, ess_mask.p, y, stream_);
}

// y = this rank's element contributions of K x as they stand: no expansion, no sum over images or ranks, no output mask
void NonlinearMechOperator::GradMultRaw(const double* x, double* y, const uint8_t* in_mask) {
   EXA_HC(hipMemsetAsync(y, 0, sizeof(double) * nd_, stream_));
   if (routes_.lvec_grad) abi_check(ctx_, exa_grad_apply_lvec_gated(ctx_, x, y, in_mask, nullptr, stream_), "exa_grad_apply_lvec");
   else ElementAction(x, in_mask, y);
}

// the raw action on nc columns in one call (exa_grad_apply_lvec_cols): false when the context has no such kernel - y is then untouched
bool NonlinearMechOperator::GradMultRawCols(int nch, int nc, const double* x, int64_t ldx, double* y, int64_t ldy, const uint8_t* in_mask, const double* const* gates) {
   if (!routes_.lvec_grad) return false;
   const int rc = exa_grad_apply_lvec_cols_w(ctx_, nch, nc, x, ldx, y, ldy, in_mask, gates, stream_);
   if (rc == EXA_ERR_UNSUPPORTED) return false;
   abi_check(ctx_, rc, "exa_grad_apply_lvec_cols");
   return true;
}

void NonlinearMechOperator::GradMult(const double* x, double* y, bool constrained, const double* done_flag, bool y_prezeroed, bool skip_out_mask) {
   if (!y_prezeroed) vk_fill_if(nd_, done_flag, 0.0, y, stream_);
   if (routes_.lvec_grad && overlap_) {
      // blocks that touch shared nodes, exchange of the shared dofs on the communication stream, interior blocks meanwhile, unpack last
      const uint8_t* m = constrained ? ess_mask.p : nullptr;
      const int nball = (E_ + 63) / 64;
      const int rc0 = exa_grad_apply_lvec_blocks(ctx_, x, y, m, done_flag, 0, nblk_bdr_, stream_);
      // (the context cannot run block ranges - a property of the configuration, the same on every rank; nothing has been added to y: whole action + halo_sum from now on)
      if (rc0 == EXA_ERR_UNSUPPORTED) overlap_ = false;
      else {
         abi_check(ctx_, rc0, "exa_grad_apply_lvec_blocks");
         comm_.halo_begin(y, stream_);
         abi_check(ctx_, exa_grad_apply_lvec_blocks(ctx_, x, y, m, done_flag, nblk_bdr_, nball - nblk_bdr_, stream_), "exa_grad_apply_lvec_blocks");
         comm_.halo_end(y, stream_);
         if (constrained && !skip_out_mask) vk_mask_zero(nd_, ess_mask.p, y, stream_);
         return;
      }
   }
   // Mixed loading: the action sees P x.  The essential entries of the reduced vector are masked before the expansion (a corner image stays free in
   // every component that a free H_id reaches), so the action itself runs without an input mask.
   const bool mix = mixed();
   if (mix) x = cell_->Expand(x, done_flag, constrained ? ess_mask.p : nullptr);
   const uint8_t* in_mask = constrained && !mix ? ess_mask.p : nullptr;
   if (routes_.lvec_grad) abi_check(ctx_, exa_grad_apply_lvec_gated(ctx_, x, y, in_mask, done_flag, stream_), "exa_grad_apply_lvec");
   else ElementAction(x, in_mask, y);
   SumLVector(y, done_flag);
   if (constrained && !skip_out_mask) vk_mask_zero(nd_, ess_mask.p, y, stream_);
}

void NonlinearMechOperator::GetUpdateBCsAction(const double* k, const double* x, double* y) {
   Setup<false>(k);
   ReadModelStatus();                          // (no residual norm follows this evaluation)
   GetGradient();                              // Hform->Setup + gradient data
   GradMult(x, y, false);                      // local action without essential constraints
   ResidualAction(tmp_r_.p);                   // Hform->Mult(k, resid), essential rows zeroed
   vk_mask_zero(nd_, ess_mask.p, y, stream_);
   vk_axpby(nd_, 1.0, tmp_r_.p, 1.0, y, stream_);
}

double NonlinearMechOperator::dot(const double* a, const double* b) {
   double* sum = scal.p + SCAL_DOT;
   vk_dot(nd_, nn_, weight.p, a, b, nullptr, partial.p, sum, stream_);
   comm_.allreduce_sum(sum, 1, stream_);
   double h; EXA_HC(hipMemcpyAsync(&h, sum, sizeof(double), hipMemcpyDeviceToHost, stream_)); EXA_HC(hipStreamSynchronize(stream_));
   return h;
}

// ||r|| over all ranks; +inf everywhere if any rank saw an unconverged constitutive point in the launch that produced r
double NonlinearMechOperator::ResidualNorm(const double* r) {
   double* sum = scal.p + SCAL_DOT;
   vk_dot(nd_, nn_, weight.p, r, r, nullptr, partial.p, sum, stream_);
   // device side: fail count of the launch that produced r -> SCAL_FAILED; a non-zero count turns the local sum into +inf before the all-reduce
   if (model_status_pending_) vk_poison_if_failed(exa_model_fail_counter_dev(ctx_), sum, scal.p + SCAL_FAILED, stream_);
   comm_.allreduce_sum(sum, 1, stream_);
   double h[SCAL_FAILED - SCAL_DOT + 1]; EXA_HC(hipMemcpyAsync(h, sum, sizeof(h), hipMemcpyDeviceToHost, stream_)); EXA_HC(hipStreamSynchronize(stream_));
   if (model_status_pending_) { model_fail = (int)h[SCAL_FAILED - SCAL_DOT]; model_fail_total += model_fail; model_status_pending_ = false; }
   FlushModelTimers();   // everything on the stream has finished: no wait
   return std::sqrt(h[0]);
}

void NonlinearMechOperator::UpdateModel() { model_->UpdateModelVars(); model_->UpdateStress(); model_->UpdateStateVars(); }
void NonlinearMechOperator::SwapCoords() { x_beg.copy_from(x_cur, stream_); }

// =====================================================================================================================
// SystemDriver
// =====================================================================================================================
static void load_case_data(const ExaOptions& opt, const Partition& part, std::vector<double>& props, std::vector<double>& quats_local, std::vector<int32_t>& attr,
                           std::vector<double>& ori) {
   props = ExaOptions::load_numbers(opt.resolve(opt.props_file));
   if ((int)props.size() != opt.nprops) throw std::runtime_error("Properties file does not hold num_props values");
   ori = ExaOptions::load_numbers(opt.resolve(opt.ori_file));
   quats_local.resize((size_t)4 * part.E); attr.resize((size_t)part.E);
   if (part.from_file) {   // grain id = element attribute (reference src/mechanics_driver.cpp:1117-1125)
      for (int e = 0; e < part.E; e++) {
         const int grain = part.elem_attr[e] - 1;
         if (grain < 0 || 4 * (grain + 1) > (int)ori.size()) throw std::runtime_error("Element attribute outside the orientation file");
         attr[e] = grain + 1;
         for (int q = 0; q < 4; q++) quats_local[4 * (size_t)e + q] = ori[4 * (size_t)grain + q];
      }
      return;
   }
   std::vector<double> gmap = ExaOptions::load_numbers(opt.resolve(opt.grain_file));
   const int f = 1 << opt.ref_ser;
   const int c0 = opt.ncuts[0], c1 = opt.ncuts[1], c2 = opt.ncuts[2];
   if ((int)gmap.size() < c0 * c1 * c2) throw std::runtime_error("Grain map is smaller than the mesh");
   quats_local.resize((size_t)4 * part.E);
   for (int e = 0; e < part.E; e++) {
      const int64_t g = part.elem_gid[e];
      const int i = (int)(g % part.N[0]), j = (int)((g / part.N[0]) % part.N[1]), k = (int)(g / ((int64_t)part.N[0] * part.N[1]));
      // uniform refinement: children inherit the parent's grain id (setElementGrainIDs, src/mechanics_driver.cpp:1257-1270)
      const int grain = (int)gmap[(i / f) + c0 * ((j / f) + c1 * (k / f))] - 1;
      if (grain < 0 || 4 * (grain + 1) > (int)ori.size()) throw std::runtime_error("Grain id outside the orientation file");
      attr[e] = grain + 1;
      for (int q = 0; q < 4; q++) quats_local[4 * (size_t)e + q] = ori[4 * (size_t)grain + q];
   }
}

SystemDriver::~SystemDriver() = default;

static void normalise_quats(std::vector<double>& q) {
   for (size_t i = 0; i + 3 < q.size(); i += 4) {
      const double n = std::sqrt(q[i] * q[i] + q[i + 1] * q[i + 1] + q[i + 2] * q[i + 2] + q[i + 3] * q[i + 3]);
      if (n > 0.0 && std::isfinite(n)) for (int k = 0; k < 4; k++) q[i + k] /= n;
   }
}

// EXA_HALO_SELFTEST (Comm::init): the one rank lists itself as neighbour with the dofs of the nodes on its x-max face - (N + 1)^2 nodes x 3 components, the
// size of a face exchange of a block decomposition - so that every halo_sum / halo_begin of a solve runs a real grouped send / receive (of zeros) over RCCL
static void add_selftest_neighbour(Partition& part, const Comm& comm) {
   if (!comm.selftest() || !part.nbrs.empty()) return;
   double xmax = -1e300; for (int g = 0; g < part.NN; g++) xmax = std::max(xmax, part.X[g]);
   Neighbor nb; nb.rank = comm.rank;
   for (int c = 0; c < 3; c++) for (int g = 0; g < part.NN; g++) if (part.X[g] >= xmax - 1e-12) nb.dofs.push_back(g + part.NN * c);
   part.nbrs.push_back(nb);
}

SystemDriver::SystemDriver(const ExaOptions& opt, int rank, int nranks, const void* uid) : opt_(opt) {
   comm.init(rank, nranks, uid);
   if (opt.mesh_type == "auto") {
      const int f = 1 << opt.ref_ser; const int N[3] = { opt.ncuts[0] * f, opt.ncuts[1] * f, opt.ncuts[2] * f };
      part.build(N, opt.length, rank, nranks, opt.order);
   } else part.build_from_mfem_mesh(opt.resolve(opt.mesh_file), rank, nranks, opt.order);
   add_selftest_neighbour(part, comm);
   if (opt.order == 1) part.order_boundary_first();   // several ranks: elements at shared nodes first (exchange overlapped with the interior, GradMult)
   if (opt.periodic) part.make_periodic(opt.periodic_mixed);            // (after the element order: it rewrites weights, neighbour lists and the group table only)
   std::vector<double> props, quats, qref; load_case_data(opt, part, props, quats, elem_attr, qref);
   qref.resize(qref.size() / 4 * 4);
   normalise_quats(qref);   // grain g: row g - 1 of the orientation file
   init(props, quats, std::move(qref));
}

SystemDriver::SystemDriver(const ExaOptions& opt, const std::vector<double>& props, const std::vector<double>& quats_global, int rank, int nranks, const void* uid) : opt_(opt) {
   comm.init(rank, nranks, uid);
   const int f = 1 << opt.ref_ser; const int N[3] = { opt.ncuts[0] * f, opt.ncuts[1] * f, opt.ncuts[2] * f };
   part.build(N, opt.length, rank, nranks, opt.order);
   add_selftest_neighbour(part, comm);
   if (opt.order == 1) part.order_boundary_first();
   std::vector<double> quats((size_t)4 * part.E);
   for (int e = 0; e < part.E; e++) for (int q = 0; q < 4; q++) quats[4 * (size_t)e + q] = quats_global[4 * (size_t)part.elem_gid[e] + q];
   elem_attr.resize((size_t)part.E);   // one grain per element (SetGrains: a grain map)
   for (int e = 0; e < part.E; e++) elem_attr[e] = (int32_t)(part.elem_gid[e] + 1);
   synthetic_ = true;
   std::vector<double> qref(quats_global.begin(), quats_global.begin() + 4 * part.E_global());
   normalise_quats(qref);
   init(props, quats, std::move(qref));
}

void SystemDriver::init(const std::vector<double>& props, const std::vector<double>& quats_local, std::vector<double> grain_qref) {
   oper_.reset(new NonlinearMechOperator(opt_, part, comm, props, quats_local));
   if (opt_.periodic && opt_.periodic_mixed) set_free(opt_.periodic_free);
   const int nd = oper_->Height();
   v_sol.alloc(nd); v_sol.zero(); r_.alloc(nd); c_.alloc(nd); xt_.alloc(nd); ess_val_.alloc(nd);
   ess_host_.assign(nd, 0); ess_val_host_.assign(nd, 0.0);
   dt_class = opt_.dt;
   PCGSolver::Settings ks;
   ks.rel_tol = opt_.krylov_rel; ks.abs_tol = opt_.krylov_abs; ks.max_iter = opt_.krylov_iter;
   if (const char* g = std::getenv("EXA_PCG_GRAPH")) { if (std::string(g) == "0") ks.graph_max_dofs = 0; else if (std::string(g) == "all") ks.graph_max_dofs = INT64_MAX; }
   if (opt_.krylov_solver == "gmres") { ks.kdim = opt_.gmres_kdim; krylov_.reset(new GMRESSolver(*oper_, ks)); }
   else krylov_.reset(new PCGSolver(*oper_, ks));
   analyses_.reset(new StepAnalyses(*oper_, comm, part, opt_, elem_attr, std::move(grain_qref)));
}

// BCManager::updateBCData + UpdateEssTDofs; component codes reference src/BCData.cpp:25-116
void SystemDriver::UpdateEssBdr(const BCEntry& bc) {
   const int nn = part.NN;
   std::fill(ess_host_.begin(), ess_host_.end(), 0); std::fill(ess_val_host_.begin(), ess_val_host_.end(), 0.0);
   std::vector<uint8_t> vel(ess_host_.size(), 0), vg(ess_host_.size(), 0);
   have_vel_ = have_vgrad_ = false;
   for (int k = 0; k < 9; k++) vgrad_[k] = bc.vgrad[k];
   if (part.periodic) {   // the eight corners, all components, as velocity-gradient dofs: v = L (x - origin) pins the rigid translation
      for (int g = 0; g < nn; g++) {
         const bool corner = part.is_corner(g);
         if (corner) for (int k = 0; k < 3; k++) { ess_host_[g + nn * k] = 1; vg[g + nn * k] = 1; }
         // mixed loading: the slot (c_d, i) holds the unknown H_id where it is free
         if (corner && mix_.on) for (int d = 0; d < 3; d++) if (g == part.ctrl_node[1 + d]) for (int k = 0; k < 3; k++) if (mix_.free[3 * k + d]) ess_host_[g + nn * k] = 0;
      }
      have_vgrad_ = true;
   }
   for (size_t b = 0; b < bc.ids.size(); b++) {   // (periodic: no ids)
      bool c[3] = { false, false, false };
      const bool is_vg = bc.comps[b] < 0;
      if (bc.ids[b] < 1 || bc.ids[b] > part.num_bdr_attr())
         throw std::runtime_error("BCs.essential_ids: boundary attribute " + std::to_string(bc.ids[b]) + " does not exist (the mesh has " + std::to_string(part.num_bdr_attr()) + ")");
      if (std::abs(bc.comps[b]) > 7) throw std::runtime_error("BCs.essential_comps: component code " + std::to_string(bc.comps[b]) + " is not one of 0..7 (negative: velocity gradient)");
      switch (std::abs(bc.comps[b])) { case 1: c[0] = true; break; case 2: c[1] = true; break; case 3: c[2] = true; break; case 4: c[0] = c[1] = true; break;
                                       case 5: c[1] = c[2] = true; break; case 6: c[0] = c[2] = true; break; case 7: c[0] = c[1] = c[2] = true; break; default: break; }
      for (int g = 0; g < nn; g++) if (part.on_face(g, bc.ids[b])) for (int k = 0; k < 3; k++) if (c[k]) {
         ess_host_[g + nn * k] = 1;
         if (is_vg) { vg[g + nn * k] = 1; vel[g + nn * k] = 0; have_vgrad_ = true; }
         else { vel[g + nn * k] = 1; vg[g + nn * k] = 0; ess_val_host_[g + nn * k] = bc.vals[3 * b + k]; have_vel_ = true; }
      }
   }
   oper_->UpdateEssTDofs(ess_host_);
   ess_val_.upload(ess_val_host_); vel_mask_.upload(vel); vg_mask_.upload(vg);
}

// origin of the velocity-gradient conditions, left in the operator's scal[SCAL_ORIGIN]: Problem.vgrad_origin when it is given, otherwise the
// componentwise minimum of the current coordinates over all ranks
const double* SystemDriver::VgradOrigin() {
   NonlinearMechOperator& op = *oper_;
   hipStream_t s = op.stream();
   double* org = op.scal.p + NonlinearMechOperator::SCAL_ORIGIN;
   if (opt_.vgrad_origin_flag) EXA_HC(hipMemcpyAsync(org, opt_.vgrad_origin, 3 * sizeof(double), hipMemcpyHostToDevice, s));
   else { vk_min3(part.NN, op.x_cur.p, op.partial.p, org, s); comm.allreduce_min(org, 3, s); }
   return org;
}

// SystemDriver::UpdateVelocity (reference src/system_driver.cpp:326-426): velocity conditions, then the velocity-gradient
// conditions v = L (x - x_min) evaluated on the current mesh nodes (end of the previous step) for their own essential dofs.
void SystemDriver::UpdateVelocity(double* v) {
   NonlinearMechOperator& op = *oper_;
   hipStream_t s = op.stream();
   const double* L = mix_.on ? mix_.L_eff : vgrad_;
   if (have_vel_) vk_mask_set(op.Height(), vel_mask_.p, ess_val_.p, v, s);
   if (have_vgrad_) {
      const double* org = VgradOrigin();
      vk_vgrad_velocity(part.NN, vg_mask_.p, op.x_cur.p, org, L, v, s);
   }
   if (part.periodic) op.cell()->Jump(L, op.x_cur.p, v, xt_.p);
}

void SystemDriver::set_free(const uint8_t* f) {
   oper_->cell()->set_free_bits(mix_.set_free(f, opt_.bcs.empty() ? nullptr : opt_.bcs.front().vgrad));
}

// Three stages: the corner values from the cell, the step algebra of host/mixed_loading.hpp, the launches that follow from it.
void SystemDriver::MixedStepStart() {
   NonlinearMechOperator& op = *oper_;
   hipStream_t s = op.stream();
   double cx[12], cv[12], A[9], Hp[9], H[9];
   op.cell()->CornerValues(op.x_cur.p, cx); op.cell()->CornerValues(v_sol.p, cv);
   corner_differences(cx, A); corner_differences(cv, Hp);
   const std::string refusal = mixed_free_refusal(mix_.free, A);
   if (!refusal.empty()) throw std::runtime_error(refusal);
   mixed_choose_H(mix_.free, steps_done == 0 && !restarted_, vgrad_, A, Hp, H);
   mixed_gradient(H, A, mix_.L_eff);
   if (mix_.bc_changed) {   // the affine part of the prescribed entries: v += (H - H_prev) A^-1 (x - origin)
      double dL[9];
      mixed_bc_dL(mix_.L_eff, Hp, A, dL);
      const double* org = VgradOrigin();
      vk_periodic_affine_add(part.NN, op.x_cur.p, org, dL, v_sol.p, s);
      mix_.bc_changed = false;
   }
   for (int k = 0; k < 9; k++) mix_.A[k] = A[k];
   // c_0 relative to the origin of the velocity-gradient conditions (UpdateVelocity pins v(c_0) = L (x(c_0) - origin)): MixedStepEnd
   double org[3];
   if (opt_.vgrad_origin_flag) for (int k = 0; k < 3; k++) org[k] = opt_.vgrad_origin[k];
   else {
      const double* org_dev = VgradOrigin();
      EXA_HC(hipMemcpyAsync(org, org_dev, 3 * sizeof(double), hipMemcpyDeviceToHost, s)); EXA_HC(hipStreamSynchronize(s));
   }
   for (int k = 0; k < 3; k++) mix_.w0[k] = cx[k] - org[k];
}

void SystemDriver::MixedStepEnd() {
   double cv[12], H[9], t[3];
   oper_->cell()->CornerValues(v_sol.p, cv);
   oper_->cell()->ReadResultants(mix_.F);
   corner_differences(cv, H);
   mixed_gradient(H, mix_.A, mix_.L);
   mix_.solved = true;
   // The step pinned c_0 at L (x(c_0) - origin) with the gradient it started from.  A rigid translation of the converged field (the residual does
   // not see it) moves the pin to the realised gradient: the run is then the one the fully prescribed route makes of that gradient, node by node.
   mixed_pin_translation(mix_.L, mix_.L_eff, mix_.w0, t);
   if (t[0] != 0.0 || t[1] != 0.0 || t[2] != 0.0) { vk_translate(part.NN, t, v_sol.p, oper_->stream()); oper_->UpdateEndCoords(v_sol.p); }
}

// A new velocity gradient under periodic conditions (the first step included, from L = 0).  The corrector of the prescribed-face model
// (SolveInit) moves the essential dofs and solves for the rest; here the essential dofs are the eight corners only, while the change of L
// changes the jump of every image - a corrector that knows the corners alone returns a field whose images no longer fit their
// neighbours once the jump is imposed.  The periodic counterpart keeps the fluctuation and swaps the affine part:
// v += (L_new - L_old) (x - origin) on every node, which satisfies the new jump and the new corner values where v satisfied the old ones.
void SystemDriver::PeriodicBCChange(const BCEntry& bc) {
   NonlinearMechOperator& op = *oper_;
   hipStream_t s = op.stream();
   double dL[9];
   for (int k = 0; k < 9; k++) dL[k] = bc.vgrad[k] - (bc_index_ >= 0 ? vgrad_[k] : 0.0);
   bc_index_ = (int)(&bc - opt_.bcs.data());
   UpdateEssBdr(bc);
   if (mix_.on) { mix_.bc_changed = true; return; }   // (MixedStepStart swaps the affine part of the prescribed entries)
   const double* org = VgradOrigin();
   vk_periodic_affine_add(part.NN, op.x_cur.p, org, dL, v_sol.p, s);
}

void SystemDriver::SetPreconditioner(int kind, int levels, int degree) {
   if (kind < 0 || kind > 2) throw std::runtime_error("preconditioner kind must be 0 (identity), 1 (jacobi) or 2 (multigrid)");
   NonlinearMechOperator& op = *oper_;
   if (kind == 2) {
      const bool bbar = ExaOptions::lower(opt_.integ_model) == "bbar";
      if (bbar && opt_.mg_bbar && part.periodic) throw std::runtime_error(ExaOptions::mg_bbar_no_periodic());   // (with or without mg_periodic)
      if (part.periodic && !opt_.mg_periodic) throw std::runtime_error(ExaOptions::periodic_no_multigrid());
      if (bbar && !opt_.mg_bbar) throw std::runtime_error(ExaOptions::mg_no_bbar());
      // p = 2 is opt-in (Solvers.Krylov.mg_p2); what stays refused with it says why, everything else keeps the constructor's message
      if (opt_.mg_p2 && !part.from_file && part.geom == 0 && part.p > 2) throw std::runtime_error(ExaOptions::mg_p2_no_higher_order());
      if (opt_.mg_p2 && part.p == 2 && part.periodic) throw std::runtime_error(ExaOptions::mg_p2_no_periodic());
      op.mg_p2_allowed = opt_.mg_p2; op.mg_bbar_allowed = opt_.mg_bbar;
      op.mg.reset(new Multigrid(op, levels, degree));   // throws where no hierarchy can be built
   } else op.mg.reset();
   krylov_->DropGraph();
   op.precond = kind == 0 ? Precond::IDENTITY : (kind == 1 ? Precond::JACOBI : Precond::MULTIGRID);
}

void SystemDriver::SetKrylov(const std::string& solver, int kdim) {
   const std::string k = ExaOptions::lower(solver);
   KrylovSolver::Settings ks = krylov_->set;
   std::unique_ptr<KrylovSolver> next;
   if (k == "gmres") {
      if (kdim < 1 || kdim > 100) throw std::runtime_error(ExaOptions::gmres_kdim_range());
      ks.kdim = kdim;
      next.reset(new GMRESSolver(*oper_, ks));
      opt_.gmres_kdim = kdim;
   } else if (k == "pcg") next.reset(new PCGSolver(*oper_, ks));
   else throw std::runtime_error("set_krylov: the solver is \"pcg\" or \"gmres\"");
   // the diagnostics and totals are the run's, not the object's: they go on counting
   next->diag = krylov_->diag; next->krylov_ms = krylov_->krylov_ms; next->krylov_iters = krylov_->krylov_iters;
   krylov_ = std::move(next);
   opt_.krylov_solver = k;
}

void SystemDriver::SetPeriodic(const double* L9, const uint8_t* free9) {
   if (steps_done > 0 || !stats.empty() || restarted_) throw std::runtime_error("set_periodic: periodic boundary conditions can only be set before the first step");
   if (!L9) throw std::runtime_error("set_periodic: a 3 x 3 velocity gradient is required");
   for (int k = 0; k < 9; k++) if (!std::isfinite(L9[k])) throw std::runtime_error("set_periodic: the velocity gradient must be finite");
   if (part.from_file || part.geom != 0) throw std::runtime_error(ExaOptions::periodic_needs_generated_mesh());
   if (oper_->precond == Precond::MULTIGRID && part.p == 2) throw std::runtime_error(ExaOptions::mg_p2_no_periodic());   // (with or without mg_periodic)
   if (oper_->precond == Precond::MULTIGRID && ExaOptions::lower(opt_.integ_model) == "bbar") throw std::runtime_error(ExaOptions::mg_bbar_no_periodic());
   if (oper_->precond == Precond::MULTIGRID && !opt_.mg_periodic) throw std::runtime_error(ExaOptions::periodic_no_multigrid());
   uint8_t f[9];
   const bool any = free_mask_bits(free9, f) != 0;
   if (free9) if (const char* why = ExaOptions::periodic_free_refusal(f)) throw std::runtime_error(why);
   part.make_periodic(any);
   BCEntry e; e.step = 1; for (int k = 0; k < 9; k++) e.vgrad[k] = L9[k];
   opt_.bcs.assign(1, e); opt_.periodic = true; opt_.periodic_mixed = any;
   for (int k = 0; k < 9; k++) opt_.periodic_free[k] = f[k];
   oper_->SetupPeriodic();
   set_free(opt_.periodic_free);   // (after the set-up: the bits live in the cell)
   // a hierarchy made for the prescribed-face cell took its weights and its sums from the partition as it was: make it again
   if (oper_->mg) oper_->mg.reset(new Multigrid(*oper_, oper_->mg->levels_cap(), oper_->mg->degree()));
   krylov_->DropGraph();
}

// ExaNewtonSolver::Mult / ExaNewtonLSSolver::Mult with b = 0 (reference src/mechanics_solver.cpp:39-143,155-281)
bool SystemDriver::NewtonSolve(double* x, SolverStats& st) {
   NonlinearMechOperator& op = *oper_;
   hipStream_t s = op.stream();
   const int64_t nd = op.Height();
   const int calls0 = op.model_calls;
   ProfRegion prof("newton_solver");
   op.Mult(x, r_.p);
   double norm = op.ResidualNorm(r_.p), norm_prev;
   const double norm_max = std::max(opt_.newton_rel * norm, opt_.newton_abs);
   double scale = 1.0; bool converged = false; int it;
   for (it = 0; true; it++) {
      if (!std::isfinite(norm)) { converged = false; break; }
      if (norm <= norm_max) { converged = true; break; }
      if (it >= opt_.newton_iter) { converged = false; break; }
      op.GetGradient();
      st.krylov_iters += krylov_->Solve(r_.p, c_.p);
      if (mix_.on) op.cell()->ExpandCorrection(c_.p, op.ess_mask.p);   // the correction of the reduced unknowns -> of the nodal velocities
      if (opt_.nl_solver == NLSolver::NRLS) {
         const double q1 = norm;
         EXA_HC(hipMemcpyAsync(xt_.p, x, sizeof(double) * nd, hipMemcpyDeviceToDevice, s)); vk_axpby(nd, -1.0, c_.p, 1.0, xt_.p, s);
         op.Mult(xt_.p, r_.p); const double q3 = op.ResidualNorm(r_.p);
         EXA_HC(hipMemcpyAsync(xt_.p, x, sizeof(double) * nd, hipMemcpyDeviceToDevice, s)); vk_axpby(nd, -0.5, c_.p, 1.0, xt_.p, s);
         op.Mult(xt_.p, r_.p); const double q2 = op.ResidualNorm(r_.p);
         const double eps = (3.0 * q1 - 4.0 * q2 + q3) / (4.0 * (q1 - 2.0 * q2 + q3));
         if ((q1 - 2.0 * q2 + q3) > 0 && eps > 0 && eps < 1) scale = eps; else if (q3 < q1) scale = 1.0; else scale = 0.05;
      }
      if (scale == 0.0) { converged = false; break; }
      vk_axpby(nd, -scale, c_.p, 1.0, x, s);
      op.Mult(x, r_.p);
      norm_prev = norm; norm = op.ResidualNorm(r_.p);
      if (opt_.nl_solver == NLSolver::NR) scale = (norm / norm_prev > 0.5) ? 0.5 : 1.0;
   }
   st.newton_iters = it; st.converged = converged; st.model_calls += op.model_calls - calls0;
   last_newton_norm = norm; last_newton_bound = norm_max;
   return converged;
}

// reference src/system_driver.cpp:293-319
void SystemDriver::SolveInit(const double* xprev, double* x) {
   NonlinearMechOperator& op = *oper_;
   hipStream_t s = op.stream(); const int64_t nd = op.Height();
   DevBuf<double> deltaF(nd), b(nd);
   deltaF.zero(s);
   // deltaF[ess] = x[ess] - xprev[ess]
   EXA_HC(hipMemcpyAsync(xt_.p, x, sizeof(double) * nd, hipMemcpyDeviceToDevice, s)); vk_axpby(nd, -1.0, xprev, 1.0, xt_.p, s);
   vk_mask_set(nd, op.ess_mask.p, xt_.p, deltaF.p, s);
   op.GetUpdateBCsAction(xprev, deltaF.p, b.p);
   SolverStats dummy; (void)dummy;
   const int it = krylov_->Solve(b.p, x);
   if (!stats.empty()) stats.back().krylov_iters += it;
   vk_axpby(nd, 1.0, xprev, -1.0, x, s);   // x = -x + xprev
}

// reference src/system_driver.cpp:221-288 (auto time stepping included)
bool SystemDriver::Solve(double* x) {
   NonlinearMechOperator& op = *oper_;
   SolverStats& st = stats.back();
   if (!opt_.dt_auto) return NewtonSolve(x, st);
   const int64_t nd = op.Height();
   DevBuf<double> xprev(nd); xprev.copy_from(v_sol, op.stream());
   const double dt_old = dt_class;
   bool ok = NewtonSolve(x, st);
   int iter = 0;
   while (!ok && iter < 2) {
      EXA_HC(hipMemcpyAsync(x, xprev.p, sizeof(double) * nd, hipMemcpyDeviceToDevice, op.stream()));
      dt_class *= opt_.dt_scale; if (dt_class < opt_.dt_min) dt_class = opt_.dt_min;
      op.SetDt(dt_class);
      ok = NewtonSolve(x, st); iter++;
   }
   if (iter > 0) time = time - dt_old + dt_class;
   last_dt_ = dt_class; step_dt_ = dt_class;   // (the size the step was solved with, after any cut-back: dt_class becomes the next step's proposal below)
   if (ok) auto_dt_rows_.push_back(dt_class);
   if (ok && write_files && comm.rank == 0) { std::ofstream f(out_dir + "/" + opt_.auto_dt_fname, std::ios_base::app); f << std::setprecision(12) << dt_class << std::endl; }
   const double niter_scale = (double)opt_.newton_iter * opt_.dt_scale;
   const double nr_iter = std::max(1, st.newton_iters);
   dt_class *= niter_scale / nr_iter; if (dt_class < opt_.dt_min) dt_class = opt_.dt_min;
   return ok;
}

// reference src/system_driver.cpp:429-558
void SystemDriver::UpdateModel() {
   NonlinearMechOperator& op = *oper_;
   hipStream_t s = op.stream();
   exa_ctx* ctx = op.GetModel()->ctx();
   op.RefreshJacobians();   // the averages weight with det J of the converged configuration (reference: the determinants cached by the last Setup)
   op.UpdateModel();
   auto vol_avg = [&](const double* qf, int vdim, bool normalise, double* out) {
      std::vector<double> h(vdim + 1);
      abi_check(ctx, exa_vol_avg(ctx, op.el_jac.p, qf, vdim, 0, h.data(), s), "exa_vol_avg");
      if (comm.nranks > 1) { DevBuf<double> t(vdim + 1); t.upload(h.data(), vdim + 1, s); comm.allreduce_sum(t.p, vdim + 1, s); t.download(h.data(), vdim + 1, s); }
      for (int i = 0; i < vdim; i++) out[i] = normalise ? h[i] / h[vdim] : h[i];
   };
   double a[28];
   vol_avg(op.stress0.p, 6, true, a);
   avg_stress.insert(avg_stress.end(), a, a + 6);
   const bool root = comm.rank == 0 && write_files;
   if (root) append_row(out_dir + "/" + opt_.avg_stress_fname, a, 6);
   if (opt_.additional_avgs) {
      op.EnsureSlipRates(op.matVars0);
      vol_avg(op.matVars0.p, 28, false, a);
      avg_pl_work.push_back(a[2]);
      if (root) append_row(out_dir + "/" + opt_.avg_pl_work_fname, a + 2, 1);
      // CalculateDeformationGradient: gradient of the current coordinates on the reference configuration
      const size_t nq9 = (size_t)exa_qf_size(ctx, 9);
      DevBuf<double> jref(nq9), F(nq9), xe(3 * (size_t)part.n * part.E);
      abi_check(ctx, exa_restrict(ctx, op.x_ref.p, xe.p, s), "exa_restrict");
      abi_check(ctx, exa_jacobians(ctx, xe.p, jref.p, s), "exa_jacobians");
      abi_check(ctx, exa_restrict(ctx, op.x_cur.p, op.el_x.p, s), "exa_restrict");   // x_true -> E-vector (reference src/mechanics_operator.cpp:411-414)
      abi_check(ctx, exa_grad_calc(ctx, jref.p, op.el_x.p, F.p, s), "exa_grad_calc");
      vol_avg(F.p, 9, true, a);
      avg_def_grad.insert(avg_def_grad.end(), a, a + 9);
      if (root) append_row(out_dir + "/" + opt_.avg_def_grad_fname, a, 9);
      op.EnsureSlipRates(op.matVars1);
      op.GetModel()->calcDpMat(F.p, s);
      vol_avg(F.p, 9, true, a);
      const double dpv[6] = { a[0], a[4], a[8], a[5], a[2], a[1] };
      avg_dp_tensor.insert(avg_dp_tensor.end(), dpv, dpv + 6);
      if (root) append_row(out_dir + "/" + opt_.avg_dp_tensor_fname, dpv, 6);
   }
}

// one pass of the reference's time-step loop body (src/mechanics_driver.cpp:837-907)
bool SystemDriver::Step(int ti, bool commit) {
   NonlinearMechOperator& op = *oper_;
   hipStream_t s = op.stream(); const int64_t nd = op.Height();
   analyses_->BeforeFirstStep(state(), commit);   // accumulators, ParaView cycle 0 and texture 0 of the initial state, outside the timed region
   double dt_real;
   if (opt_.dt_cust) dt_real = opt_.cust_dt[ti - 1];
   else if (opt_.dt_auto) dt_real = std::min(dt_class, opt_.t_final - time);
   else dt_real = std::min(opt_.dt, opt_.t_final - time);
   time += dt_real; dt_class = dt_real; step_dt_ = dt_real;
   op.SetDt(dt_real);
   stats.emplace_back();
   step_solved_ = false;
   const auto wall0 = std::chrono::steady_clock::now();   // reference: t1 = MPI_Wtime() ... times[ti - 1] = t2 - t1 (src/mechanics_driver.cpp:865,891-892)
   hipEvent_t e0, e1; EXA_HC(hipEventCreate(&e0)); EXA_HC(hipEventCreate(&e1)); EXA_HC(hipEventRecord(e0, s));
   for (const BCEntry& bc : opt_.bcs) if (bc.step == ti) {
      if (part.periodic) { PeriodicBCChange(bc); continue; }
      DevBuf<double> v_prev(nd); v_prev.copy_from(v_sol, s);
      bc_index_ = (int)(&bc - opt_.bcs.data());
      UpdateEssBdr(bc);
      UpdateVelocity(v_sol.p);
      SolveInit(v_prev.p, v_sol.p);
   }
   if (mix_.on) MixedStepStart();
   UpdateVelocity(v_sol.p);
   const bool ok = Solve(v_sol.p);
   EXA_HC(hipEventRecord(e1, s)); EXA_HC(hipEventSynchronize(e1));
   float ms = 0; EXA_HC(hipEventElapsedTime(&ms, e0, e1)); (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
   op.timers.t_solve_ms += ms;
   step_wall_s.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count());
   if (!ok) return false;
   if (mix_.on) MixedStepEnd();
   step_solved_ = true;
   if (!commit) return true;   // the converged state stays the END-of-step state: the next constitutive pass repeats this step's last residual evaluation
   CommitStep();
   // the output schedule of the analyses; the macroscopic tangent, which reads the state and leaves it alone, follows on the same cadence
   if (analyses_->AfterCommit(state(), ti) && opt_.macro_tangent) WriteMacroTangent(ti);
   return true;
}
// end-of-step update of a solved step (also called later for a step solved with commit = false, as long as only residual evaluations at the
// converged velocity - bench passes - have run in between: they rewrite the same end-of-step state)
void SystemDriver::CommitStep() {
   UpdateModel();
   oper_->SwapCoords();
   steps_done++;
   analyses_->Committed(state());
}

int SystemDriver::RunAll() {
   // (a restarted run that already stands at the end of the schedule has nothing to do)
   bool finished = false;
   if (restarted_ && !opt_.dt_cust) { const double dtl = opt_.dt_auto ? last_dt_ : opt_.dt; finished = std::fabs(time - opt_.t_final) <= std::fabs(1e-3 * dtl); }
   for (int ti = steps_done + 1; ti <= opt_.nsteps && !finished; ti++) {
      if (!Step(ti)) {
         if (comm.rank == 0) std::cerr << "Newton Solver did not converge" << (oper_->model_fail > 0 ? " (the constitutive update failed at quadrature points of the last evaluation)" : "") << ".\n";
         return -ti;
      }
      if (!opt_.dt_cust) { const double dtl = opt_.dt_auto ? last_dt_ : opt_.dt; finished = std::fabs(time - opt_.t_final) <= std::fabs(1e-3 * dtl); }
      // [Checkpoint]: every Checkpoint.steps steps and after the last one; older files are removed once the new one is in place
      if (opt_.ckpt_write && write_files && (finished || ti == opt_.nsteps || ti % opt_.ckpt_steps == 0)) { SaveCheckpoint(checkpoint_path(ti)); PruneCheckpoints(ti); }
   }
   WriteStepTimes();
   return steps_done;
}

void SystemDriver::SetGrains(const int32_t* grain, int64_t n_global, const double* grain_quats, int G) {
   if (!synthetic_) throw std::runtime_error("set_grains: only a synthetic driver takes a grain map (a file-driven one has its grains from the options)");
   if (steps_done > 0 || !stats.empty()) throw std::runtime_error("set_grains: the grain map can only be set before the first step");
   if (n_global != part.E_global()) throw std::runtime_error("set_grains: one grain id per global element is required");
   if (G < 1 || !grain || !grain_quats) throw std::runtime_error("set_grains: at least one grain, its orientation and a grain id per element are required");
   for (int64_t e = 0; e < n_global; e++) if (grain[e] < 1 || grain[e] > G) throw std::runtime_error("set_grains: grain ids must lie in 1 .. G");
   std::vector<double> q(grain_quats, grain_quats + 4 * (size_t)G);
   for (double x : q) if (!std::isfinite(x)) throw std::runtime_error("set_grains: orientations must be finite");
   for (int g = 0; g < G; g++) if (q[4 * g] == 0.0 && q[4 * g + 1] == 0.0 && q[4 * g + 2] == 0.0 && q[4 * g + 3] == 0.0) throw std::runtime_error("set_grains: an orientation is zero");
   normalise_quats(q);
   std::vector<double> ql((size_t)4 * part.E);
   for (int e = 0; e < part.E; e++) {
      const int32_t g = grain[part.elem_gid[e]];
      elem_attr[e] = g;
      for (int k = 0; k < 4; k++) ql[4 * (size_t)e + k] = q[4 * (size_t)(g - 1) + k];
   }
   NonlinearMechOperator& op = *oper_;
   hipStream_t s = op.stream();
   exa_ctx* ctx = op.GetModel()->ctx();
   { DevBuf<double> d; d.upload(ql, s); abi_check(ctx, exa_init_state(ctx, op.matVars0.p, d.p, s), "exa_init_state"); EXA_HC(hipStreamSynchronize(s)); }
   analyses_->GrainsChanged(std::move(q));   // (exa_init_state is no constitutive launch: the stamp of the element rows would still match)
}

// per-rank wall time of every step's solve, one value per line with 8 digits: ./time/time_solve.<rank>.txt of the reference
// (src/mechanics_driver.cpp:982-998; every rank writes its own file, appended like the reference's)
void SystemDriver::WriteStepTimes() {
   if (!write_files || step_wall_s.empty()) return;
   const std::string dir = out_dir + "/time";
   (void)::mkdir(dir.c_str(), 0755);
   std::ofstream f(dir + "/time_solve." + std::to_string(comm.rank) + ".txt", std::ios::out | std::ios::app);
   for (double v : step_wall_s) f << std::setprecision(8) << v << "\n";
   step_wall_s.clear();   // written once: a second RunAll / WriteStepTimes appends only its own steps
}

}  // namespace exa_host
