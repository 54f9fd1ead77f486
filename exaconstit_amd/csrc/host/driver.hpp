// Stand-alone host driver above the C ABI: the reference's operator / solver / system-driver classes re-expressed for
// device-resident data (MFEM is not available in this image, so the data containers are plain device buffers; the class
// and method names, argument meaning and control flow follow the reference so that its regression cases run unchanged).
//   ExaModel / ExaCMechModel            reference src/mechanics_model.hpp:17-241, src/mechanics_ecmech.hpp:12-109
//   ExaNLFIntegrator                     reference src/mechanics_integrators.hpp:14-76
//   NonlinearMechOperator                reference src/mechanics_operator.hpp:18-100, src/mechanics_operator.cpp:288-483
//   MechOperatorJacobiSmoother           reference src/mechanics_operator_ext.cpp:11-55
//   ExaNewtonSolver / ExaNewtonLSSolver  reference src/mechanics_solver.cpp:39-281
//   PCGSolver (host/krylov.hpp)          MFEM CGSolver, set up at reference src/system_driver.cpp:166-177
//   GMRESSolver (host/krylov.hpp)        MFEM GMRESSolver, set up at reference src/system_driver.cpp:152-164
//   SystemDriver                         reference src/system_driver.cpp:221-558
//   Comm (host/comm.hpp)               MPI in the reference (src/mechanics_driver.cpp:312, src/system_driver.cpp:167, src/mechanics_kernels.hpp:119,124)
//   OperatorRoutes (host/routes.hpp)     the operator's EXA_* switches and which kernels it runs for them (no counterpart in the reference)
//   PeriodicCell (host/periodic.hpp)     periodic images, their sums and mixed loading on the device; MixedLoading (host/mixed_loading.hpp): its step algebra (no counterpart)
//   StepAnalyses (host/analyses.hpp)     reference src/system_driver.cpp:560-870 (the Project* outputs) and what this project adds to them
//   time-step loop                       reference src/mechanics_driver.cpp:837-907
#pragma once
#include <map>
#include <memory>
#include <string>
#include <vector>
#include "../../../include/exaconstit_hip.h"
#include "analyses.hpp"
#include "comm.hpp"
#include "device_utils.hpp"
#include "krylov.hpp"
#include "mesh.hpp"
#include "mixed_loading.hpp"
#include "options.hpp"
#include "periodic.hpp"
#include "routes.hpp"

namespace exa_host {

class Multigrid;

// macroscopic tangent of a periodic cell: T[9 (3 k + l) + m] / V = d sigma_bar_kl / d L_bar_m, m = 3 i + j the entry (i, j) of L_bar
struct MacroTangentResult {
   double T[81]; double V = 0.0, dt = 0.0;
   int iters[9]; int flag[9];                       // per column: PCG iterations, the solver's flag (1 converged, 2 max_iter, -1 breakdown)
   double reduction[9], b_norm[9], res_norm[9];     // the solver's own reduction sqrt((r, M^-1 r) / (r0, M^-1 r0)); |b_m|, |b_m - K_uu w_m| recomputed by one more action
   double w_over_a[9];                              // max |w_m| / max |a_m|: size of the fluctuation against the affine field
   int batched = 0, nch = 0;                        // route taken: nine columns in lockstep through the multi-column action (nch columns per pass), or one by one
};
// C_pp - C_pf C_ff^-1 C_fp of the 9 x 9 c[9 (kl) + (mn)] for the free mask (row by row): out81 holds it in the prescribed rows / columns and zeros in
// the free ones; false when C_ff is singular.  Host code.
bool macro_tangent_condense(const double* c81, const uint8_t* free9, double* out81);
// one row (step, time, dt, V, 81 values of d sigma_bar / d L_bar, 17 significant digits) per evaluation
void write_macro_tangent_rows(const std::string& path, const std::vector<double>& rows, bool append);
constexpr int MACRO_TANGENT_ROW = 85;

struct SolverStats { int newton_iters = 0; int krylov_iters = 0; int model_calls = 0; bool converged = false; };

struct Timers { double t_model_ms = 0, t_solve_ms = 0; int64_t qpt_updates = 0; };   // (the Krylov totals are the solver's: host/krylov.hpp)

// Per-quadrature-point model seam (ExaModel): owns nothing but scratch; the driver owns the quadrature functions.
class ExaCMechModel {
 public:
   ExaCMechModel(exa_ctx* ctx, DevBuf<double>* stress0, DevBuf<double>* stress1, DevBuf<double>* matGrad, DevBuf<double>* matVars0, DevBuf<double>* matVars1)
      : ctx_(ctx), stress0_(stress0), stress1_(stress1), matGrad_(matGrad), matVars0_(matVars0), matVars1_(matVars1) {}
   void SetModelDt(double dt) { dt_ = dt; }
   double GetModelDt() const { return dt_; }
   // ExaCMechModel::ModelSetup (reference src/mechanics_ecmech.cpp:192-258) with the operator's L->E restrictions and Jacobian refresh fused in (writes the Jacobians)
   void ModelSetupLVec(const double* x_lvec, const double* v_lvec, double* jacobian_out, hipStream_t s);
   // ... and with AssembleGradPA fused in too: writes the compact gradient records instead of the tangent field (p = 1 fast path)
   void ModelSetupLVecRecords(const double* x_lvec, const double* v_lvec, double* jacobian_out, hipStream_t s);
   void UpdateModelVars() {}
   void UpdateStress() { stress0_->swap(*stress1_); }        // reference src/mechanics_model.cpp:435-438
   void UpdateStateVars() { matVars0_->swap(*matVars1_); }   // reference src/mechanics_model.cpp:440-443
   void calcDpMat(double* dp, hipStream_t s) const;          // reads matVars1 (reference src/mechanics_ecmech.hpp:309)
   DevBuf<double>* GetStress0() { return stress0_; } DevBuf<double>* GetStress1() { return stress1_; }
   DevBuf<double>* GetMatVars0() { return matVars0_; } DevBuf<double>* GetMatVars1() { return matVars1_; } DevBuf<double>* GetMatGrad() { return matGrad_; }
   exa_ctx* ctx() const { return ctx_; }
 private:
   exa_ctx* ctx_; double dt_ = 1.0;
   DevBuf<double>*stress0_, *stress1_, *matGrad_, *matVars0_, *matVars1_;
};

class NonlinearMechOperator {
 public:
   NonlinearMechOperator(const ExaOptions& opt, const Partition& part, Comm& comm, const std::vector<double>& props, const std::vector<double>& quats_per_elem);
   ~NonlinearMechOperator();
   int Height() const { return nd_; }
   void SetDt(double dt) { dt_ = dt; model_->SetModelDt(dt); }
   void UpdateEssTDofs(const std::vector<uint8_t>& mask);
   // y = F(k): residual with essential rows zeroed (reference src/mechanics_operator.cpp:288-308)
   void Mult(const double* k, double* y);
   template <bool upd_crds> void Setup(const double* k);
   // Jacobian set-up + Jacobi diagonal (reference src/mechanics_operator.cpp:436-443)
   void GetGradient();
   // y = K x with essential columns/rows masked (constrained) or the plain local action
   // y_prezeroed / skip_out_mask: the PCG loop folds the zero fill into its direction update and the output mask into its dot product
   void GradMult(const double* x, double* y, bool constrained, const double* done_flag = nullptr, bool y_prezeroed = false, bool skip_out_mask = false);
   // this rank's part of the constrained action (no halo exchange): what the multigrid hierarchy probes (host/multigrid.hpp)
   void GradMultLocal(const double* x, double* y);
   // macroscopic tangent (host/tangent.hip): the element contributions of K x as they stand - no expansion, no sum over images or
   // ranks, no output mask; in_mask (nullable): entries of x read as zero
   void GradMultRaw(const double* x, double* y, const uint8_t* in_mask = nullptr);
   // ... of nc columns at once, ADDED into y, nch columns per pass over the records (0: the library's default); gates: one device flag per column
   // (nullable).  false: the context has no multi-column kernel (y untouched) and the caller goes column by column
   bool GradMultRawCols(int nch, int nc, const double* x, int64_t ldx, double* y, int64_t ldy, const uint8_t* in_mask, const double* const* gates);
   bool deterministic() const { return comm_.deterministic; }
   // reference src/mechanics_operator.cpp:446-483
   void GetUpdateBCsAction(const double* k, const double* x, double* y);
   void ResidualAction(double* y);
   // The one place where an L-vector of element contributions becomes the assembled vector: the sum over the ranks, on a periodic partition the
   // cell's sum over images and ranks (PeriodicCell::Sum, DESIGN 4.11 / 4.12, which explains flag and raw).
   void SumLVector(double* y, const double* flag = nullptr, bool raw = true);
   bool mixed() const { return part_.periodic && part_.mixed; }
   void UpdateEndCoords(const double* k);    // x_cur = x_beg + dt k, as the residual evaluation at k computes it
   // weights, halo lists and the cell of a partition that has (just) become periodic
   void SetupPeriodic();
   PeriodicCell* cell() { return cell_.get(); }   // null on a partition that is not periodic
   void RefreshJacobians();                // el_jac of x_cur when the record route left it unwritten (volume averages)
   void UpdateModel();                     // swap begin/end state, x_beg <- x_cur
   void SwapCoords();
   ExaCMechModel* GetModel() { return model_.get(); }
   hipStream_t stream() const { return stream_; }
   const Partition& part() const { return part_; }
   Comm& comm() { return comm_; }
   // route of the Krylov action (Driver.mesh_info): 0 hexahedron kernels, 1 fused tetrahedron action, 2 table-driven E-vector PA, 3 table-driven EA on L-vectors
   int action_route() const { return routes_.action_route; }
   // state of the automatic Newton cap (checkpoint files carry it: the cap in force decides how the next constitutive launch is split)
   void GetCapState(int& cap, int& cap2) const { cap = newton_cap_; cap2 = newton_cap2_; }
   void SetCapState(int cap, int cap2);
   bool halo_overlap() const { return overlap_; }      // the gradient action overlaps the halo exchange with its interior blocks
   // Lean end-of-step state (include/exaconstit_hip.h exa_set_lean_state): the element-blocked record launches leave the inputs of the 12
   // slip rates in state slots 14..19 instead of the rates, and the buffer they wrote is marked "rates pending".  The mark belongs to the device
   // array, so it follows matVars0 / matVars1 through their swaps.  Every reader of slots 14..25 calls EnsureSlipRates on its buffer first: one
   // bandwidth-bound launch (exa_slip_rates_from_state) when the mark is set, nothing otherwise.  EXA_LEAN_STATE=off: full state from every launch.
   void EnsureSlipRates(const DevBuf<double>& buf);
   bool RatesPending(const DevBuf<double>& buf) const { return buf.p && (rates_pending_[0] == buf.p || rates_pending_[1] == buf.p); }
   void ForgetPendingRates() { rates_pending_[0] = rates_pending_[1] = nullptr; }   // the state arrays have been replaced (checkpoint load)
   int64_t rate_launches = 0;                          // materialisation launches so far (Driver.diagnostics)
   // data (device)
   DevBuf<double> x_ref, x_beg, x_cur, el_x, el_jac, diag, dinv, weight;
   DevBuf<double> stress0, stress1, matVars0, matVars1, matGrad;
   DevBuf<uint8_t> ess_mask;
   DevBuf<int32_t> conn;
   Precond precond = Precond::IDENTITY;   // (SystemDriver::SetPreconditioner is its only writer)
   std::unique_ptr<Multigrid> mg;   // precond == MULTIGRID: rebuilt after every gradient set-up
   // multigrid at p = 2 (host/multigrid.hpp; SystemDriver::SetPreconditioner writes the first, exa_driver_set_mg_p2_build the second)
   bool mg_p2_allowed = false;      // Solvers.Krylov.mg_p2: Multigrid's constructor accepts a p = 2 partition
   bool mg_bbar_allowed = false;    // Solvers.Krylov.mg_bbar: Multigrid's constructor accepts a B-bar operator (written by SetPreconditioner too)
   int mg_p2_build = 1;             // 1: level 1 and the fine diagonal from the point records where they can serve; 0: always probed
   // The p = 2 matrix-free action reads point records this Newton iteration's set-up left, in the form the run streams: the compact records of the
   // constitutive launch (record route), or the 46-double records of exa_grad_setup when the compact form is switched off (EXA_TANGENT_FORM=full).
   // EXA_TANGENT_RECORDS=off, the deterministic mode and EXA_EA_ASSEMBLED=1 take the tangent-field routes: nothing is read off records there.
   bool p2_records_readable() const {
      return part_.p == 2 && part_.geom == 0 && routes_.lvec_grad && !routes_.det && (use_records() || !routes_.compact_tangent) &&
             (opt_.assembly == Assembly::PA || routes_.ea_matrix_free);
   }
   Timers timers;
   int model_calls = 0;
   std::vector<double> props;     // material parameters the context was created with (the adapter-route bench creates a second, AOS context from them)
   exa_config cfg_used;           // ... and its configuration (props pointer not valid after construction)
   double dt() const { return dt_; }
   // quadrature points whose local (ExaCMech) solve did not converge in the last constitutive launch.  The library fails the run
   // in that case (ECMECH_FAIL in getResponseSngl); here a non-zero count poisons the next residual norm on every rank, so that
   // Newton reports non-convergence: Time.Auto then cuts dt, otherwise the run stops.
   int model_fail = 0; int64_t model_fail_total = 0;
   bool model_status_pending_ = false;       // a constitutive launch whose failure count has not reached the host yet (ResidualNorm / ReadModelStatus)
   struct EvPair { hipEvent_t a = nullptr, b = nullptr; bool pending = false; long call = 0; };
   void ReadTimer(EvPair& e);   // adds a finished launch to timers.t_model_ms (EXA_MODEL_TIMES=1: and prints it)
   EvPair& NextModelTimer(); void FlushModelTimers(); void ReadModelStatus();
   double ResidualNorm(const double* r);
   double dot(const double* a, const double* b);   // weighted, all-reduced, synchronising
   // scal: the operator's own device scalars - the sum of dot / ResidualNorm, the origin of the velocity-gradient conditions (3 doubles), the failed-point
   // count of the constitutive launch behind a residual (ResidualNorm reads SCAL_DOT .. SCAL_FAILED back in one copy)
   enum { SCAL_DOT = 9, SCAL_ORIGIN = 12, SCAL_FAILED = 15, SCAL_LEN = 32 };
   DevBuf<double> partial, scal;
 private:
   ExaOptions opt_; const Partition& part_; Comm& comm_;
   // Which kernels run (host/routes.hpp), decided once at construction.  What changes afterwards is held by the members below: overlap_ (agreed over
   // the ranks, demoted when the context cannot run block ranges, off on periodic partitions), compact_tangent_ (dropped when the defect check
   // fails), jac_stale_, the caps of the tail-split controller (newton_cap_, newton_cap2_) and the pending-rates marks (rates_pending_).
   const OperatorRoutes routes_;
   exa_ctx* ctx_ = nullptr; std::unique_ptr<ExaCMechModel> model_;
   hipStream_t stream_ = nullptr; hipEvent_t ev0_, ev1_;
   std::vector<EvPair> ev_ring_; int ev_head_ = 0;   // event pairs around the constitutive launches, read back lazily
   int nn_, nd_, E_, npe_ = 8; double dt_ = 1.0;
   bool use_records() const { return routes_.records_setup && precond != Precond::JACOBI; }   // gradient records written by the constitutive launch
   bool jac_stale_ = false;       // the record route left the Jacobian field unwritten (RefreshJacobians)
   void ensure_mat_grad();
   bool overlap_ = false; int nblk_bdr_ = 0;   // halo exchange overlapped with the interior element blocks (several ranks, atomic p = 1 record action)
   bool compact_tangent_ = false;
   const double* rates_pending_[2] = { nullptr, nullptr };   // state arrays whose slots 14..25 wait for EnsureSlipRates
   void MarkRates(const double* p, bool pending);
   int newton_cap_ = 0, newton_cap2_ = 0;
   void ElementAction(const double* x, const uint8_t* in_mask, double* y);   // the generic E-vector action, added into y (in_mask nullable)
   DevBuf<double> tmp_l_, tmp_r_, el_y_, el_x2_;
   std::unique_ptr<PeriodicCell> cell_;
};

class SystemDriver {
 public:
   SystemDriver(const ExaOptions& opt, int rank, int nranks, const void* nccl_uid);
   ~SystemDriver();
   // synthetic RVE without files (bench): N^3 elements, one grain per element, seeded orientations
   SystemDriver(const ExaOptions& opt, const std::vector<double>& props, const std::vector<double>& quats_per_global_elem, int rank, int nranks, const void* nccl_uid);
   void UpdateEssBdr(const BCEntry& bc);
   void UpdateVelocity(double* v);
   void PeriodicBCChange(const BCEntry& bc);   // periodic counterpart of UpdateEssBdr + SolveInit when the velocity gradient changes
   void SolveInit(const double* xprev, double* x);
   bool Solve(double* x);
   void UpdateModel();
   // one time step of the reference's loop (src/mechanics_driver.cpp:837-907); returns false if Newton failed
   // commit = false (bench): solve the step but leave begin-of-step state, coordinates and outputs untouched
   bool Step(int ti, bool commit = true);
   void CommitStep();                      // end-of-step update of a step solved with commit = false
   int RunAll();
   bool NewtonSolve(double* x, SolverStats& st);
   // preconditioner of the PCG (set before the first step; takes effect at the next gradient set-up): kind 0 identity, 1 Jacobi, 2 multigrid with at most `levels` coarse levels (0: as
   // many as the mesh allows) and a Chebyshev smoother of `degree`; refuses multigrid where no hierarchy can be built
   void SetPreconditioner(int kind, int levels, int degree);
   // multigrid on a periodic cell is opt-in (Solvers.Krylov.mg_periodic; DESIGN 4.6, "periodic cells"): without it SetPreconditioner and SetPeriodic
   // refuse the combination with the options reader's message, as they always did
   void AllowPeriodicMultigrid(bool on) { opt_.mg_periodic = on; }
   // ... and so is multigrid at p_refinement = 2 (Solvers.Krylov.mg_p2; DESIGN 4.6, "p = 2"): without it SetPreconditioner refuses the order as it always did
   void AllowP2Multigrid(bool on) { opt_.mg_p2 = on; }
   // ... and multigrid under integ_model = "BBAR" (Solvers.Krylov.mg_bbar; DESIGN 4.6, "B-bar"); the key permits, a FULL run does not read it
   void AllowBbarMultigrid(bool on) { opt_.mg_bbar = on; }
   // periodic boundary conditions under the macroscopic velocity gradient L9 (row by row) on a freshly created driver before its first step,
   // like SetPreconditioner: rebuilds the partition tables, weights, essential set and halo lists (every rank calls it).  Refuses file meshes
   // and, without AllowPeriodicMultigrid, the multigrid preconditioner with the messages of the options reader; a hierarchy that exists is made again.  The boundary-condition schedule becomes one entry: L from step 1.
   // free9 (row by row, may be null: all prescribed): the entries of L that are unknowns, their mean tractions zero (mixed loading)
   void SetPeriodic(const double* L9, const uint8_t* free9 = nullptr);
   // (mixed loading: the realised gradient H A^-1 of the last solved step, once there is one)
   const double* vgrad_in_force() const { return mix_.on && mix_.solved ? mix_.L : (bc_index_ >= 0 ? vgrad_ : opt_.bcs.front().vgrad); }
   // Mixed loading, start of a step: period vectors A and corner differences H from the fields, the run-time check that "prescribed L_id" is a
   // condition on H_id alone, the prescribed H_id = (L a_d)_i (step 1: all of them), the gradient L = H A^-1 that UpdateVelocity imposes; when the
   // options' L has just changed, the affine part of the velocity is swapped for the prescribed entries
   void MixedStepStart();
   void MixedStepEnd();   // realised gradient and face resultants of the converged step
   const MixedLoading& mixed_loading() const { return mix_; }
   double last_newton_norm = 0.0, last_newton_bound = 0.0;   // final residual norm and max(rel |r0|, abs) of the last Newton solve
   KrylovSolver& krylov() { return *krylov_; }   // the run's linear solver: PCG or GMRES
   // the run's linear solver anew (exa_driver_set_krylov): "pcg", or "gmres" with its Krylov dimension; before the first step or between steps.
   // Tolerances, cap and chunk stay, and the run's diagnostics and totals (solves not converged, worst reduction, Krylov ms and iterations) go on
   // counting; the restarts and second passes of krylov_info are the new GMRES object's.
   void SetKrylov(const std::string& solver, int kdim);
   StepAnalyses& analyses() { return *analyses_; }   // the run's in-situ analyses (host/analyses.hpp) ...
   StepState state() const { return { steps_done, time, step_dt_, out_dir, write_files, v_sol }; }   // ... and where the run stands, for their calls
   // Homogenised tangent d sigma_bar / d L_bar of the last solved step of a periodic cell (host/tangent.hip), every rank calls it.
   // rel_tol / max_iter <= 0: the Krylov options.  batched: -1 the automatic route, 0 column by column through PCGSolver::Solve, 1 the nine columns in
   // lockstep through the multi-column action (one rank, non-deterministic mode, a context exa_grad_apply_lvec_cols serves; refused elsewhere).
   // Refuses a driver that is not periodic or has no step solved in this process.  Leaves the run as it found it.
   void MacroTangent(double rel_tol, int max_iter, int batched, MacroTangentResult& out);
   // probe of the operator (exa_driver_grad_apply_columns): y_m = K x_m for nc host columns of local dofs (byNODES).  assembled: the operator of the
   // tangent's solves (periodic and rank sums, the run's essential set plus the control slots, input and output); otherwise the raw element action.
   // gated (nullable): columns with a non-zero entry are left out - their y stays as passed in.
   void GradApplyColumns(int nc, const double* x, double* y, bool assembled, bool batched, const int* gated);
   // probe of the linear solver (exa_driver_pcg_solve): K_uu x_m = b_m for nc host columns of local dofs (byNODES), the operator and the scope of
   // GradApplyColumns(assembled), in a PCGSolver of the probe's own built from the run's settings with rel_tol, abs_tol, max_iter, check_every
   // (0: the run's) and graph (-1 the run's limit, 0 no replay, 1 replay at any size).  mode 0: Solve for each column in turn into one fixed device
   // buffer (a later column replays the chunk the first one captured and starts from the record it left); mode 1: SolveColumns on all of them
   // (tangent_nch columns per pass).  Per column: x, iterations, flag, the solver's reduction, indefinite iterations, sc[2 m] = (r0, z0) and
   // sc[2 m + 1] = the last (r, z).  Every rank calls it.  Leaves the run as it found it.
   void PcgSolveProbe(int nc, const double* b, double rel_tol, double abs_tol, int max_iter, int check_every, int graph, int mode, double* x, int* iters, int* flag,
                      double* reduction, int* indefinite, double* sc);
   // probe of GMRES (exa_driver_gmres_solve), as PcgSolveProbe: a GMRESSolver of the probe's own, the columns in turn.  ortho: -1 EXA_GMRES_ORTHO,
   // 0 ... 3 GMRESSolver::Ortho.  Per column sc[4 m ...] = beta0, the last residual norm, restarts, second Gram-Schmidt passes.
   void GmresSolveProbe(int nc, const double* b, double rel_tol, double abs_tol, int max_iter, int kdim, int check_every, int ortho, double* x, int* iters, int* flag,
                        double* reduction, double* sc);
   int tangent_nch = 0;                 // columns per pass of the multi-column action (0: the library's default; EXA_TANGENT_NCH)
   bool tangent_auto_batched = true;    // what batched = -1 picks where the batched route is available (EXA_TANGENT_BATCHED=0 | 1)
   std::vector<double> macro_tangent_rows;   // Visualizations.macro_tangent: MACRO_TANGENT_ROW values per written evaluation
   NonlinearMechOperator& oper() { return *oper_; }
   const ExaOptions& options() const { return opt_; }
   std::vector<double> avg_stress, avg_def_grad, avg_pl_work, avg_dp_tensor;   // one row per completed step (rank 0 view, all ranks identical)
   std::vector<SolverStats> stats;
   DevBuf<double> v_sol;
   double time = 0.0, dt_class = 0.0; int steps_done = 0;
   bool write_files = true; std::string out_dir = ".";
   std::vector<double> step_wall_s;            // wall time of each step (solve part), written to time/time_solve.<rank>.txt by RunAll
   void WriteStepTimes();
   // Checkpoint and restart.  SaveCheckpoint: everything that defines where the run is, into one file written as <path>.tmp and
   // renamed (every rank calls it).  LoadCheckpoint: legal only on a freshly created driver before its first step; refuses a file that does not
   // belong to this mesh / model / property set, naming the mismatch; rewrites the avg_* and light-up files from the stored rows.
   void SaveCheckpoint(const std::string& path);
   void LoadCheckpoint(const std::string& path);
   std::string checkpoint_path(int step) const;   // <out_dir>/<Checkpoint.floc>_<step %06d>.ckpt
   // grain map of a synthetic driver before its first step: grain (1..G) of every global element and the orientation of every grain (normalised
   // here); the elements' initial orientations and states become their grain's; the analyses are told (GrainsChanged)
   void SetGrains(const int32_t* grain_of_global_elem, int64_t n_global, const double* grain_quats, int G);
   std::vector<int32_t> elem_attr;             // grain id (element attribute) of every local element
   Partition part;
   Comm comm;
 private:
   void init(const std::vector<double>& props, const std::vector<double>& quats_local, std::vector<double> grain_qref);
   ExaOptions opt_;
   std::unique_ptr<NonlinearMechOperator> oper_;
   std::unique_ptr<KrylovSolver> krylov_;
   std::unique_ptr<StepAnalyses> analyses_;
   DevBuf<double> r_, c_, xt_, ess_val_;
   std::vector<uint8_t> ess_host_; std::vector<double> ess_val_host_;
   DevBuf<uint8_t> vel_mask_, vg_mask_; bool have_vel_ = false, have_vgrad_ = false; double vgrad_[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
   double last_dt_ = 0.0, step_dt_ = 0.0;      // step_dt_: size of the step last solved: Time.Auto after any cut-back, otherwise the dt Step took (StepState::dt)
   // accepted dt of Time.Auto: rows that exist only in an append-mode file otherwise (checkpoint host section)
   std::vector<double> auto_dt_rows_;
   MixedLoading mix_;
   void set_free(const uint8_t* f);             // the free mask into mix_ and the cell's free bits
   const double* VgradOrigin();                 // leaves the origin of the velocity-gradient conditions in the operator's scal[SCAL_ORIGIN]
   int bc_index_ = -1;                          // index in opt_.bcs of the essential-boundary entry in force
   bool synthetic_ = false, restarted_ = false;
   bool step_solved_ = false;                   // the last Step of this process converged and no constitutive launch has run since (MacroTangent)
   struct TangentScope;                         // host/tangent.hip: the essential set of the tangent's solves and what an evaluation puts back
   void WriteMacroTangent(int step);
   // shared-node copies of a checkpoint written on another rank count (host/checkpoint.hip): carried along untouched and written back as long as
   // no constitutive launch has run since the load, so that load + save reproduces the file on any rank count
   std::vector<unsigned char> ckpt_foreign_copies_[2]; long ckpt_foreign_calls_ = -1;
   void PruneCheckpoints(int step);
};

}  // namespace exa_host
