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

// Periodic partition (Partition::make_periodic): the weights and the halo lists of the partition as it is now, the group table in the layout of
// periodic_kernels.hip and, for several ranks, the two nodal arrays of the jump through the fluctuation (PeriodicJump)
void NonlinearMechOperator::SetupPeriodic() {
   const Partition& part = part_;
   weight.upload(part.weight);
   comm_.setup_halo(part);
   overlap_ = false;
   const int n2 = part.grp_count[0], n4 = part.grp_count[1], n8 = part.grp_count[2];
   std::vector<int32_t> idx(part.grp_nodes.size());
   size_t base = 0; int g0 = 0;
   for (int cls = 0; cls < 3; cls++) {   // CSR (group-major) -> member-major within each size class
      const int m = 2 << cls, n = part.grp_count[cls];
      for (int g = 0; g < n; g++) for (int j = 0; j < m; j++) idx[base + (size_t)j * n + g] = part.grp_nodes[(size_t)part.grp_off[g0 + g] + j];
      base += (size_t)m * n; g0 += n;
   }
   per_idx_.release(); if (!idx.empty()) per_idx_.upload(idx);
   per_tab_.idx = per_idx_.p; per_tab_.n2 = n2; per_tab_.n4 = n4; per_tab_.n8 = n8;
   if (comm_.nranks > 1) {
      std::vector<double> rw((size_t)nn_, 0.0); std::vector<uint8_t> surf((size_t)nn_, 0);
      for (int g = 0; g < nn_; g++) { if (part.node_gid[g] == part.canon[g]) rw[g] = part.weight_node[g]; surf[g] = part.on_box_surface(g) ? 1 : 0; }
      if (part.mixed) for (int g = 0; g < nn_; g++) if (part.is_corner(g)) { rw[g] = 0.0; surf[g] = 0; }   // (the corners take their velocity from the control values: UpdateVelocity)
      per_repw_.upload(rw); per_surf_.upload(surf);
      // the owner of a canonical id: its representative on the lowest rank that holds the id (ResidualAction)
      std::vector<uint8_t> notown((size_t)nd_, 1), lower((size_t)nn_, 0);
      for (const Neighbor& nb : part.nbrs) if (nb.rank < comm_.rank) for (int32_t d : nb.dofs) lower[(size_t)(d % nn_)] = 1;
      std::vector<uint8_t> image((size_t)nn_, 0);      // local images other than the representative
      for (size_t g = 0; g + 1 < part.grp_off.size(); g++) for (int32_t k = part.grp_off[g] + 1; k < part.grp_off[g + 1]; k++) image[(size_t)part.grp_nodes[k]] = 1;
      for (int g = 0; g < nn_; g++) if (!lower[g] && !image[g]) for (int c = 0; c < 3; c++) notown[g + (size_t)nn_ * c] = 0;
      per_notown_.upload(notown);
   }
   if (part.mixed) {
      const uint32_t fb = mix_tab_.free_bits;
      mix_tab_ = MixedTable(); mix_tab_.free_bits = fb;
      mix_img_.release(); mix_code_.release(); mix_face_.release();
      if (!part.img_nodes.empty()) { mix_img_.upload(part.img_nodes); mix_code_.upload(part.img_code); }
      std::vector<int32_t> face;
      for (int d = 0; d < 3; d++) {
         face.insert(face.end(), part.face_nodes[d].begin(), part.face_nodes[d].end());
         mix_tab_.foff[d + 1] = (int)face.size();
         mix_tab_.fblk[d + 1] = mix_tab_.fblk[d] + (int)((part.face_nodes[d].size() + 255) / 256);
      }
      if (!face.empty()) mix_face_.upload(face);
      mix_tab_.img = mix_img_.p; mix_tab_.code = mix_code_.p; mix_tab_.nimg = (int)part.img_nodes.size(); mix_tab_.face = mix_face_.p;
      for (int k = 0; k < 4; k++) mix_tab_.ctrl[k] = part.ctrl_node[k];
      if (mix_x_.n == 0) { mix_x_.alloc(nd_); mix_h_.alloc(12); mix_f_.alloc(9); mix_res_.alloc(9); mix_f_.zero(stream_); mix_res_.zero(stream_); }
      mix_part_.release(); mix_part_.alloc((size_t)std::max(1, 3 * mix_tab_.fblk[3]));
   }
}

void NonlinearMechOperator::SumLVector(double* y, const double* flag, bool raw) {
   if (!part_.periodic) { comm_.halo_sum(y, stream_); return; }
   const bool one = !comm_.active();
   const bool mix = part_.mixed && raw;
   if (mix) vk_face_resultants(mix_tab_, nn_, y, flag, mix_part_.p, stream_);
   if (mix && one) { vk_periodic_sum_controls(per_tab_, mix_tab_, nn_, y, flag, mix_part_.p, mix_f_.p, stream_); return; }
   if (mix) { vk_face_combine(mix_tab_, nn_, mix_part_.p, mix_f_.p, nullptr, flag, stream_); comm_.allreduce_sum(mix_f_.p, 9, stream_); }
   vk_periodic_sum(per_tab_, nn_, y, flag, false, stream_);
   if (!one) {
      // the exchange carries the representative of a group: its local sum out, the other ranks' sums added to it, then back to its local images
      comm_.halo_sum(y, stream_);
      vk_periodic_sum(per_tab_, nn_, y, flag, true, stream_);
   }
   if (mix) vk_face_combine(mix_tab_, nn_, nullptr, mix_f_.p, y, flag, stream_);
}

// x -> P x.  One rank reads the control values from x itself; several ranks gather { x(c_0), H } where they hold them and add them up
// (the first of the two small all-reduces of an action).
const double* NonlinearMechOperator::MixedExpand(const double* x, const double* flag, bool constrained) {
   // (the copy is not gated by the flag: a finished PCG never reads it)
   EXA_HC(hipMemcpyAsync(mix_x_.p, x, sizeof(double) * nd_, hipMemcpyDeviceToDevice, stream_));
   if (constrained) vk_mask_zero(nd_, ess_mask.p, mix_x_.p, stream_);
   const double* h12 = nullptr;
   if (comm_.nranks > 1) {
      int32_t idx[12];
      for (int c = 0; c < 3; c++) {
         idx[c] = mix_tab_.ctrl[0] >= 0 ? mix_tab_.ctrl[0] + nn_ * c : -1;
         for (int d = 0; d < 3; d++) idx[3 + 3 * c + d] = mix_tab_.ctrl[1 + d] >= 0 ? mix_tab_.ctrl[1 + d] + nn_ * c : -1;
      }
      vk_gather_slots(idx, 12, x, mix_h_.p, stream_);
      comm_.allreduce_sum(mix_h_.p, 12, stream_);
      h12 = mix_h_.p;
   }
   vk_periodic_expand(mix_tab_, nn_, x, h12, mix_x_.p, flag, constrained, stream_);
   return mix_x_.p;
}

void NonlinearMechOperator::ExpandCorrection(double* c) {
   const double* f = MixedExpand(c, nullptr, true);
   EXA_HC(hipMemcpyAsync(c, f, sizeof(double) * nd_, hipMemcpyDeviceToDevice, stream_));
}

void NonlinearMechOperator::UpdateEndCoords(const double* k) { vk_update_coords(nd_, x_beg.p, k, dt_, x_cur.p, stream_); }

void NonlinearMechOperator::ReadResultants(double* f9_host) {
   EXA_HC(hipMemcpyAsync(f9_host, mix_res_.p, 9 * sizeof(double), hipMemcpyDeviceToHost, stream_)); EXA_HC(hipStreamSynchronize(stream_));
}

void NonlinearMechOperator::CornerValues(const double* v, double* out12_host) {
   int32_t idx[12];
   for (int k = 0; k < 4; k++) for (int c = 0; c < 3; c++) idx[3 * k + c] = mix_tab_.ctrl[k] >= 0 ? mix_tab_.ctrl[k] + nn_ * c : -1;
   vk_gather_slots(idx, 12, v, mix_h_.p, stream_);
   comm_.allreduce_sum(mix_h_.p, 12, stream_);
   EXA_HC(hipMemcpyAsync(out12_host, mix_h_.p, 12 * sizeof(double), hipMemcpyDeviceToHost, stream_)); EXA_HC(hipStreamSynchronize(stream_));
}

void NonlinearMechOperator::PeriodicJump(const double* L9, double* v) {
   if (comm_.nranks == 1) { vk_periodic_jump(per_tab_, nn_, x_cur.p, L9, v, stream_); return; }
   // several ranks: the images of a node sit on different ranks - the node that carries the canonical id hands its fluctuation v - L x to all of them
   vk_periodic_fluct(nn_, per_repw_.p, x_cur.p, L9, v, tmp_l_.p, stream_);
   SumLVector(tmp_l_.p, nullptr, false);
   vk_periodic_unfluct(nn_, per_surf_.p, x_cur.p, L9, tmp_l_.p, v, stream_);
}

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
   // Several ranks, periodic: three or more holders add their contributions in different orders, so their copies of a residual entry differ in
   // the last bits of the element forces - which is far above the last bits of a residual near equilibrium, and a part of the right-hand side
   // that differs between the copies of a dof is out of the PCG's reach (tight Krylov tolerances then stop at the cap).  Every holder takes the
   // owner's bits: all other copies are zeroed and summed again - one non-zero term per dof, an exact sum.
   if (part_.periodic && comm_.nranks > 1) { vk_mask_zero(nd_, per_notown_.p, y, stream_); SumLVector(y, nullptr, false); }
   if (mixed()) EXA_HC(hipMemcpyAsync(mix_res_.p, mix_f_.p, 9 * sizeof(double), hipMemcpyDeviceToDevice, stream_));
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
   if (mix) x = MixedExpand(x, done_flag, constrained);
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
   krylov_.reset(new PCGSolver(*oper_, ks));
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
         const int l[3] = { g % part.nn[0], (g / part.nn[0]) % part.nn[1], g / (part.nn[0] * part.nn[1]) };
         bool corner = true;
         for (int d = 0; d < 3; d++) { const int gi = part.e0[d] * part.p + l[d]; corner = corner && (gi == 0 || gi == part.N[d] * part.p); }
         if (corner) for (int k = 0; k < 3; k++) { ess_host_[g + nn * k] = 1; vg[g + nn * k] = 1; }
         // mixed loading: the slot (c_d, i) holds the unknown H_id where it is free
         if (corner && mixed_) for (int d = 0; d < 3; d++) if (g == part.ctrl_node[1 + d]) for (int k = 0; k < 3; k++) if (free_[3 * k + d]) ess_host_[g + nn * k] = 0;
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
   if (have_vel_) vk_mask_set(op.Height(), vel_mask_.p, ess_val_.p, v, s);
   if (have_vgrad_) {
      const double* org = VgradOrigin();
      vk_vgrad_velocity(part.NN, vg_mask_.p, op.x_cur.p, org, mixed_ ? vgrad_eff_ : vgrad_, v, s);
   }
   if (part.periodic) op.PeriodicJump(mixed_ ? vgrad_eff_ : vgrad_, v);
}

namespace {
void inv3(const double* A, double* B) {
   const double c0 = A[4] * A[8] - A[5] * A[7], c1 = A[5] * A[6] - A[3] * A[8], c2 = A[3] * A[7] - A[4] * A[6];
   const double det = A[0] * c0 + A[1] * c1 + A[2] * c2;
   B[0] = c0 / det; B[1] = (A[2] * A[7] - A[1] * A[8]) / det; B[2] = (A[1] * A[5] - A[2] * A[4]) / det;
   B[3] = c1 / det; B[4] = (A[0] * A[8] - A[2] * A[6]) / det; B[5] = (A[2] * A[3] - A[0] * A[5]) / det;
   B[6] = c2 / det; B[7] = (A[1] * A[6] - A[0] * A[7]) / det; B[8] = (A[0] * A[4] - A[1] * A[3]) / det;
}
void mul3(const double* A, const double* B, double* C) {
   for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
// A (column d = a_d) and H (column d = h_d) from the values of a field at c_0 .. c_3
void corner_differences(const double* c12, double* M) { for (int d = 0; d < 3; d++) for (int i = 0; i < 3; i++) M[3 * i + d] = c12[3 * (d + 1) + i] - c12[i]; }
}  // namespace

void SystemDriver::set_free(const uint8_t* f) {
   uint32_t bits = 0; mixed_ = false;
   for (int k = 0; k < 9; k++) { free_[k] = f[k] ? 1 : 0; if (free_[k]) { bits |= 1u << k; mixed_ = true; } }
   oper_->SetMixedFree(bits);
   for (int k = 0; k < 9; k++) vgrad_eff_[k] = opt_.bcs.empty() ? 0.0 : opt_.bcs.front().vgrad[k];
}

void SystemDriver::MixedStepStart() {
   NonlinearMechOperator& op = *oper_;
   hipStream_t s = op.stream();
   double cx[12], cv[12], A[9], Hp[9], H[9], Ai[9], LA[9];
   op.CornerValues(op.x_cur.p, cx); op.CornerValues(v_sol.p, cv);
   corner_differences(cx, A); corner_differences(cv, Hp);
   for (int d = 0; d < 3; d++) {
      const double len = std::sqrt(A[d] * A[d] + A[3 + d] * A[3 + d] + A[6 + d] * A[6 + d]);
      for (int i = 0; i < 3; i++) if (!free_[3 * i + d]) for (int j = 0; j < 3; j++) if (free_[3 * i + j] && std::fabs(A[3 * j + d]) > 1e-12 * len) {
         char m[320];
         std::snprintf(m, sizeof(m), "periodic_free: entry (%d,%d) of the velocity gradient is free and entry (%d,%d) is prescribed, but period vector %d has the component %.3e "
                       "along direction %d - the prescribed entry is no condition on one corner difference alone (DESIGN 4.12)", i + 1, j + 1, i + 1, d + 1, d + 1, A[3 * j + d], j + 1);
         throw std::runtime_error(m);
      }
   }
   mul3(vgrad_, A, LA);
   const bool first = steps_done == 0 && !restarted_;
   for (int k = 0; k < 9; k++) H[k] = (!free_[k] || first) ? LA[k] : Hp[k];
   inv3(A, Ai);
   mul3(H, Ai, vgrad_eff_);
   if (mix_bc_changed_) {   // the affine part of the prescribed entries: v += (H - H_prev) A^-1 (x - origin)
      double Lold[9], dL[9];
      mul3(Hp, Ai, Lold);
      for (int k = 0; k < 9; k++) dL[k] = vgrad_eff_[k] - Lold[k];
      const double* org = VgradOrigin();
      vk_periodic_affine_add(part.NN, op.x_cur.p, org, dL, v_sol.p, s);
      mix_bc_changed_ = false;
   }
   for (int k = 0; k < 9; k++) mac_A_[k] = A[k];
   // c_0 relative to the origin of the velocity-gradient conditions (UpdateVelocity pins v(c_0) = L (x(c_0) - origin)): MixedStepEnd
   double org[3];
   if (opt_.vgrad_origin_flag) for (int k = 0; k < 3; k++) org[k] = opt_.vgrad_origin[k];
   else {
      const double* org_dev = VgradOrigin();
      EXA_HC(hipMemcpyAsync(org, org_dev, 3 * sizeof(double), hipMemcpyDeviceToHost, s)); EXA_HC(hipStreamSynchronize(s));
   }
   for (int k = 0; k < 3; k++) mac_w0_[k] = cx[k] - org[k];
}

void SystemDriver::MixedStepEnd() {
   double cv[12], H[9], Ai[9];
   oper_->CornerValues(v_sol.p, cv);
   corner_differences(cv, H);
   inv3(mac_A_, Ai);
   mul3(H, Ai, mac_L_);
   oper_->ReadResultants(mac_F_);
   mac_have_ = true;
   // The step pinned c_0 at L (x(c_0) - origin) with the gradient it started from.  A rigid translation of the converged field (the residual does
   // not see it) moves the pin to the realised gradient: the run is then the one the fully prescribed route makes of that gradient, node by node.
   double t[3];
   for (int i = 0; i < 3; i++) { t[i] = 0.0; for (int j = 0; j < 3; j++) t[i] += (mac_L_[3 * i + j] - vgrad_eff_[3 * i + j]) * mac_w0_[j]; }
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
   if (mixed_) { mix_bc_changed_ = true; return; }   // (MixedStepStart swaps the affine part of the prescribed entries)
   const double* org = VgradOrigin();
   vk_periodic_affine_add(part.NN, op.x_cur.p, org, dL, v_sol.p, s);
}

void SystemDriver::SetPreconditioner(int kind, int levels, int degree) {
   if (kind < 0 || kind > 2) throw std::runtime_error("preconditioner kind must be 0 (identity), 1 (jacobi) or 2 (multigrid)");
   NonlinearMechOperator& op = *oper_;
   if (kind == 2) {
      if (part.periodic) throw std::runtime_error(ExaOptions::periodic_no_multigrid());
      if (ExaOptions::lower(opt_.integ_model) == "bbar") throw std::runtime_error("Solvers.Krylov.preconditioner = \"multigrid\" is not built for integ_model = \"BBAR\"");
      op.mg.reset(new Multigrid(op, levels, degree));   // throws where no hierarchy can be built
   } else op.mg.reset();
   krylov_->DropGraph();
   op.precond = kind == 0 ? Precond::IDENTITY : (kind == 1 ? Precond::JACOBI : Precond::MULTIGRID);
}

void SystemDriver::SetPeriodic(const double* L9, const uint8_t* free9) {
   if (steps_done > 0 || !stats.empty() || restarted_) throw std::runtime_error("set_periodic: periodic boundary conditions can only be set before the first step");
   if (!L9) throw std::runtime_error("set_periodic: a 3 x 3 velocity gradient is required");
   for (int k = 0; k < 9; k++) if (!std::isfinite(L9[k])) throw std::runtime_error("set_periodic: the velocity gradient must be finite");
   if (part.from_file || part.geom != 0) throw std::runtime_error(ExaOptions::periodic_needs_generated_mesh());
   if (oper_->precond == Precond::MULTIGRID) throw std::runtime_error(ExaOptions::periodic_no_multigrid());
   bool any = false;
   if (free9) {
      uint8_t f[9]; for (int k = 0; k < 9; k++) { f[k] = free9[k] ? 1 : 0; any = any || f[k]; }
      if (const char* why = ExaOptions::periodic_free_refusal(f)) throw std::runtime_error(why);
   }
   part.make_periodic(any);
   BCEntry e; e.step = 1; for (int k = 0; k < 9; k++) e.vgrad[k] = L9[k];
   opt_.bcs.assign(1, e); opt_.periodic = true; opt_.periodic_mixed = any;
   for (int k = 0; k < 9; k++) opt_.periodic_free[k] = any && free9[k] ? 1 : 0;
   set_free(opt_.periodic_free);
   oper_->SetupPeriodic();
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
      if (mixed_) op.ExpandCorrection(c_.p);   // the correction of the reduced unknowns -> of the nodal velocities
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
   if (mixed_) MixedStepStart();
   UpdateVelocity(v_sol.p);
   const bool ok = Solve(v_sol.p);
   EXA_HC(hipEventRecord(e1, s)); EXA_HC(hipEventSynchronize(e1));
   float ms = 0; EXA_HC(hipEventElapsedTime(&ms, e0, e1)); (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
   op.timers.t_solve_ms += ms;
   step_wall_s.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count());
   if (!ok) return false;
   if (mixed_) MixedStepEnd();
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
