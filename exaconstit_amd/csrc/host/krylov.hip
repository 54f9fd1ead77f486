// The linear solvers (host/krylov.hpp).  PCGSolver: three loops for one system - device scalars, single reduction, multigrid - and the lockstep
// loop for several; GMRESSolver: one loop; all between one prologue (Frame) and one epilogue (Finish).
#include "driver.hpp"
#include "multigrid.hpp"
#include "roctx.hpp"
#include "../pcg_slots.hpp"
#include "../gmres_slots.hpp"
#include "../gmres_small.hpp"
#include <cmath>
#include <iostream>

namespace exa_host {

static_assert(sizeof(KrylovSolver::last) / sizeof(KrylovSolver::Last) == EXA_GRAD_COLS_MAX, "one entry per column of the lockstep solve");
static_assert(gmres::F_RUNNING == pcg::RUNNING && gmres::F_CONVERGED == pcg::CONVERGED && gmres::F_MAX_ITER == pcg::MAX_ITER && gmres::F_BREAKDOWN == pcg::BREAKDOWN, "one set of flags");

KrylovSolver::KrylovSolver(NonlinearMechOperator& op, const Settings& set_, const char* name) : set(set_), op_(op), comm_(op.comm()), name_(name) {}

PCGSolver::PCGSolver(NonlinearMechOperator& op, const Settings& set_) : KrylovSolver(op, set_, "PCG") {
   const size_t nd = (size_t)op.Height();
   r_.alloc(nd); z_.alloc(nd); d_.alloc(nd);
   S_.alloc((size_t)EXA_GRAD_COLS_MAX * pcg::LEN); S_.zero(op.stream());
}

double* PCGSolver::record(int m) const { return S_.p + (size_t)m * pcg::LEN; }

void PCGSolver::DropGraph() {
   if (graph_) { (void)hipGraphExecDestroy((hipGraphExec_t)graph_); graph_ = nullptr; }
   graph_key_ = GraphKey();
}

struct KrylovSolver::Frame {
   ProfRegion prof; hipStream_t s; hipEvent_t e0 = nullptr, e1 = nullptr;
   explicit Frame(hipStream_t s_) : prof("krylov_solver"), s(s_) { EXA_HC(hipEventCreate(&e0)); EXA_HC(hipEventCreate(&e1)); EXA_HC(hipEventRecord(e0, s)); }
   float stop() { EXA_HC(hipEventRecord(e1, s)); EXA_HC(hipEventSynchronize(e1)); float ms = 0; EXA_HC(hipEventElapsedTime(&ms, e0, e1)); return ms; }
   ~Frame() { (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); }
};

// in_flight: a solve with consumer-side reductions, whose iteration count travels in ITERS_NEXT between the direction and the update kernel - after a
// chunk ITERS is one behind (pcg_slots.hpp)
void PCGSolver::ReadRecords(int n, bool in_flight, Outcome* out) {
   double h[EXA_GRAD_COLS_MAX * pcg::LEN];
   S_.download(h, (size_t)(n - 1) * pcg::LEN + pcg::USED, op_.stream());
   for (int m = 0; m < n; m++) {
      const double* S = h + (size_t)m * pcg::LEN;
      out[m].flag = (int)S[pcg::FLAG]; out[m].iters = (int)S[in_flight ? pcg::ITERS_NEXT : pcg::ITERS]; out[m].indefinite = (int)S[pcg::INDEFINITE];
      out[m].betanom = S[pcg::BETANOM]; out[m].r0z0 = S[pcg::R0Z0];
   }
}

void KrylovSolver::Finish(Frame& f, const Outcome* o, int n) {
   krylov_ms += f.stop();
   for (int m = 0; m < n; m++) {
      const bool converged = o[m].flag == (int)pcg::CONVERGED;
      krylov_iters += o[m].iters;
      last[m] = Last{ o[m].iters, o[m].flag, o[m].indefinite, o[m].r0z0, o[m].betanom };
      diag.last_flag = o[m].flag; diag.indefinite_iters += o[m].indefinite;
      if (!converged) diag.not_converged++;
      diag.last_reduction = o[m].reduction();
      if (!converged) diag.worst_capped_reduction = std::max(diag.worst_capped_reduction, diag.last_reduction);
      // what MFEM prints (CGSolver::Mult): breakdown, indefinite operator, no convergence within max_iter
      if (comm_.rank == 0 && (set.verbose || std::getenv("EXA_VERBOSE"))) {
         if (o[m].indefinite > 0) std::cerr << name_ << ": The operator is not positive definite. (Ad, d) < 0 in " << o[m].indefinite << " iteration(s)\n";
         if (o[m].flag == (int)pcg::BREAKDOWN) std::cerr << name_ << (gmres() ? ": breakdown, stopping after " : ": (Ad, d) = 0, stopping after ") << o[m].iters << " iterations\n";
         else if (!converged) std::cerr << name_ << ": No convergence! (" << o[m].iters << " iterations)\n";
      }
   }
}

int PCGSolver::Solve(const double* b, double* x) {
   if (op_.precond == Precond::MULTIGRID) return SolveMultigrid(b, x);
   if (comm_.active() && std::getenv("EXA_PCG_TWO_REDUCTIONS") == nullptr) return SolveSingleReduction(b, x);
   return SolveDeviceScalars(b, x);
}

// PCG on more than one rank: the Chronopoulos-Gear arrangement of the same recurrence needs ONE fused reduction per iteration - the pair
// gamma = (r, u), delta = (A u, u) in a single 16-byte all-reduce - instead of the two 8-byte ones of MFEM's loop:
//    u = M^-1 r,  s = A u,  beta = gamma / gamma_old,  alpha = gamma / (delta - beta gamma / alpha_old),
//    p = u + beta p,  q = s + beta q (= A p),  x += alpha p,  r -= alpha q.
// Same iterates in exact arithmetic, same stopping test on (r, M^-1 r) after each update, same iteration cap.  EXA_PCG_TWO_REDUCTIONS=1
// keeps the two-reduction loop on several ranks (A/B switch).
int PCGSolver::SolveSingleReduction(const double* b, double* x) {
   NonlinearMechOperator& op = op_;
   hipStream_t s = op.stream();
   const int64_t nd = op.Height(), nn = op.part().NN;
   double* S = record();
   Frame frame(s);
   if (s_.n < (size_t)nd) { s_.alloc(nd); q_.alloc(nd); }
   const bool ident = op.precond == Precond::IDENTITY;
   EXA_HC(hipMemsetAsync(x, 0, sizeof(double) * nd, s));
   EXA_HC(hipMemcpyAsync(r_.p, b, sizeof(double) * nd, hipMemcpyDeviceToDevice, s));
   if (!ident) vk_pointwise(nd, op.dinv.p, r_.p, z_.p, s);
   const double* u = ident ? r_.p : z_.p;
   EXA_HC(hipMemsetAsync(d_.p, 0, sizeof(double) * nd, s)); EXA_HC(hipMemsetAsync(q_.p, 0, sizeof(double) * nd, s));
   EXA_HC(hipMemsetAsync(s_.p, 0, sizeof(double) * nd, s));
   EXA_HC(hipMemsetAsync(S, 0, sizeof(double) * pcg::CLEARED, s));
   op.GradMult(u, s_.p, true, S + pcg::FLAG, true, true);
   vk_cg2_dots(nd, nn, op.weight.p, op.ess_mask.p, r_.p, z_.p, s_.p, S + pcg::FLAG, op.partial.p, S + pcg::RED0, ident, s);
   comm_.allreduce_sum(S + pcg::RED0, 2, s);
   vk_cg2_init(S, set.rel_tol, set.abs_tol, s);
   Outcome o; int launched = 0; bool done = false;
   while (!done) {
      for (int k = 0; k < set.check_every && launched < set.max_iter; k++, launched++) {
         vk_cg2_update(nd, S, op.dinv.p, x, r_.p, z_.p, d_.p, s_.p, q_.p, ident, s);
         op.GradMult(u, s_.p, true, S + pcg::FLAG, true, true);
         vk_cg2_dots(nd, nn, op.weight.p, op.ess_mask.p, r_.p, z_.p, s_.p, S + pcg::FLAG, op.partial.p, S + pcg::RED0, ident, s);
         comm_.allreduce_sum(S + pcg::RED0, 2, s);
         vk_cg2_scalars(S, set.max_iter, s);
      }
      ReadRecords(1, false, &o);
      done = o.flag != (int)pcg::RUNNING || launched >= set.max_iter;
   }
   Finish(frame, &o, 1);
   return o.iters;
}

// device PCG (MFEM CGSolver::Mult with iterative_mode = false); all scalars stay on the device, the host only polls the
// done-flag every check_every iterations.
#ifndef EXA_PCG_CONSUMER_REDUCE_MAX_DOFS
#define EXA_PCG_CONSUMER_REDUCE_MAX_DOFS INT64_MAX   // consumer-side reductions of the PCG scalars up to this many local dofs (EXA_PCG_REDUCE_LAUNCH=1: never, =<n>: up to n)
#endif
int PCGSolver::SolveDeviceScalars(const double* b, double* x) {
   NonlinearMechOperator& op = op_;
   hipStream_t s = op.stream();
   const int64_t nd = op.Height(), nn = op.part().NN;
   double* S = record();
   Frame frame(s);
   EXA_HC(hipMemsetAsync(x, 0, sizeof(double) * nd, s));
   EXA_HC(hipMemcpyAsync(r_.p, b, sizeof(double) * nd, hipMemcpyDeviceToDevice, s));
   vk_pointwise(nd, op.dinv.p, r_.p, z_.p, s);
   EXA_HC(hipMemcpyAsync(d_.p, z_.p, sizeof(double) * nd, hipMemcpyDeviceToDevice, s));
   EXA_HC(hipMemsetAsync(S, 0, sizeof(double) * pcg::CLEARED, s));
   vk_dot(nd, nn, op.weight.p, d_.p, r_.p, nullptr, op.partial.p, S + pcg::RED0, s);
   comm_.allreduce_sum(S + pcg::RED0, 1, s);
   vk_cg_init(S, set.rel_tol, set.abs_tol, s);
   // One rank: the scalar updates ride in the reductions (no all-reduce in between).  (Summing the denominator d.(K d) element-wise
   // inside the action, with its scatter skipping the essential rows, was measured too: the pass it saves costs what it adds to the
   // action kernel, +0.8 %.)
   const bool one = comm_.nranks == 1;
   // Consumer-side reductions (vec_kernels.hip): one rank.  An iteration is then four launches instead of six - update / direction / action / masked dot - and
   // the blocks of the update and direction kernels sum the <= 1024 partial sums themselves.  Same bits as the one-block reduction launches (EXA_PCG_REDUCE_LAUNCH=1).
   const char* red_env = std::getenv("EXA_PCG_REDUCE_LAUNCH");      // (read per solve: the tests switch it between drivers of one process)
   const int64_t red_max_dofs = red_env ? (std::atoll(red_env) == 1 ? (int64_t)0 : (int64_t)std::atoll(red_env)) : (int64_t)EXA_PCG_CONSUMER_REDUCE_MAX_DOFS;
   const bool red = !comm_.active() && nd <= red_max_dofs;
   double* partD = op.partial.p + 2 * DOT_BLOCKS;      // partial sums of the denominator (the (r, z) ones use the front of the buffer)
   op.GradMult(d_.p, z_.p, true, S + pcg::FLAG);
   if (red) vk_dot_partial(nd, nn, op.weight.p, z_.p, d_.p, S + pcg::FLAG, partD, s);      // the first update kernel turns them into alpha
   else {
      vk_dot(nd, nn, op.weight.p, z_.p, d_.p, S + pcg::FLAG, op.partial.p, S + pcg::RED0, s);
      comm_.allreduce_sum(S + pcg::RED0, 1, s);
      vk_cg_den(S, s);
   }
   const bool ident = op.precond == Precond::IDENTITY;      // z == r is never materialised
   auto iteration = [&]() {
      if (red) {
         vk_cg_step1(nd, nn, S, op.weight.p, op.dinv.p, d_.p, x, r_.p, z_.p, op.partial.p, ident, false, set.max_iter, s, partD);      // alpha from partD; (r, z) partial sums
         vk_cg_step2z(nd, S, z_.p, r_.p, d_.p, ident, s, op.partial.p, set.max_iter);      // beta from them; d = z + beta d; z = 0
         op.GradMult(d_.p, z_.p, true, S + pcg::FLAG, true, true);
         vk_mask_dot(nd, nn, op.weight.p, op.ess_mask.p, d_.p, z_.p, S + pcg::FLAG, partD, nullptr, s, nullptr);
         return;
      }
      vk_cg_step1(nd, nn, S, op.weight.p, op.dinv.p, d_.p, x, r_.p, z_.p, op.partial.p, ident, one, set.max_iter, s);
      if (!one) { comm_.allreduce_sum(S + pcg::RED0, 1, s); vk_cg_beta(S, set.max_iter, s); }
      vk_cg_step2z(nd, S, z_.p, r_.p, d_.p, ident, s);               // d = z + beta d; z = 0
      op.GradMult(d_.p, z_.p, true, S + pcg::FLAG, true, true);      // z += K d (input masked in the kernel, output mask folded into the dot)
      vk_mask_dot(nd, nn, op.weight.p, op.ess_mask.p, d_.p, z_.p, S + pcg::FLAG, op.partial.p, S + pcg::RED0, s, one ? S : nullptr);
      if (!one) { comm_.allreduce_sum(S + pcg::RED0, 1, s); vk_cg_den(S, s); }
   };
   // Small systems are launch-bound (16^3: 6 kernels of 2-3 us per iteration): the check_every iterations between two polls of the
   // done-flag are captured once in a hipGraph and replayed.  Every kernel of an iteration takes its scalars from the device record and is
   // a no-op once the flag is set or max_iter is reached, so the graph always holds the full chunk.  One rank only (no collective inside
   // the capture); above graph_max_dofs the kernels are long enough to hide their launches (measured).
   // The capture bakes in every kernel argument: the solution pointer, the preconditioner variant, the iteration cap (an argument of
   // k_cg_step1 / the reductions) and the chunk length - all of them are part of the key.
   const GraphKey key{ x, op.precond, red, set.check_every, set.max_iter };
   bool use_graph = !comm_.active() && nd <= set.graph_max_dofs && set.check_every > 1;
   if (use_graph && !(graph_ && graph_key_ == key)) {
      DropGraph();
      // whatever happens between begin and end, the stream must leave capture mode and the graph must not leak
      hipGraph_t g = nullptr; hipGraphExec_t ge = nullptr; std::string cap_err;
      EXA_HC(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
      try { for (int k = 0; k < set.check_every; k++) iteration(); } catch (const std::exception& e) { cap_err = e.what(); }
      const hipError_t ec = hipStreamEndCapture(s, &g);
      if (cap_err.empty() && ec == hipSuccess && g && hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) == hipSuccess) {
         graph_ = ge; graph_key_ = key;
      } else {
         (void)hipGetLastError();   // clear the sticky capture error; the plain launch loop below does the work
         use_graph = false; set.graph_max_dofs = 0;
         if (comm_.rank == 0) std::cerr << "PCG: hipGraph capture failed (" << (cap_err.empty() ? "capture/instantiate" : cap_err) << "), using stream launches\n";
      }
      if (g) (void)hipGraphDestroy(g);
   }
   Outcome o; int launched = 0; bool done = false;
   while (!done) {
      if (use_graph) { EXA_HC(hipGraphLaunch((hipGraphExec_t)graph_, s)); launched += set.check_every; }
      else for (int k = 0; k < set.check_every && launched < set.max_iter; k++, launched++) iteration();
      ReadRecords(1, red, &o);
      done = o.flag != (int)pcg::RUNNING || launched >= set.max_iter;
   }
   Finish(frame, &o, 1);
   return o.iters;
}

// PCG preconditioned by one multigrid V-cycle per iteration (host/multigrid.hpp): MFEM CGSolver::Mult with iterative_mode = false, its order of
// operations and stopping test (r, z) <= max(rel^2 (r0, z0), abs^2), on one rank and on several.  The host reads every scalar (the V-cycle
// synchronises for nothing else); no graph capture, no device record: the loop hands its scalars to the epilogue itself.
int PCGSolver::SolveMultigrid(const double* b, double* x) {
   NonlinearMechOperator& op = op_;
   hipStream_t s = op.stream();
   const int64_t nd = op.Height();
   Frame frame(s);
   double* r = r_.p; double* z = z_.p; double* d = d_.p;
   EXA_HC(hipMemsetAsync(x, 0, sizeof(double) * nd, s));
   EXA_HC(hipMemcpyAsync(r, b, sizeof(double) * nd, hipMemcpyDeviceToDevice, s));
   op.mg->Apply(r, z);
   EXA_HC(hipMemcpyAsync(d, z, sizeof(double) * nd, hipMemcpyDeviceToDevice, s));
   double nom0 = op.dot(d, r), nom = nom0, betanom = nom0;
   Outcome o; o.r0z0 = nom0; o.flag = (int)pcg::MAX_ITER;
   int it = 0;
   const double r0 = std::max(nom0 * set.rel_tol * set.rel_tol, set.abs_tol * set.abs_tol);
   if (nom0 < 0.0) o.flag = (int)pcg::MAX_ITER;                      // the preconditioner is not positive definite: MFEM stops, not converged
   else if (nom0 <= r0) o.flag = (int)pcg::CONVERGED;
   else {
      op.GradMult(d, z, true);
      double den = op.dot(z, d);
      if (den <= 0.0 && op.dot(d, d) > 0.0) o.indefinite++;
      if (den == 0.0) o.flag = (int)pcg::BREAKDOWN;
      else
         for (it = 1; true; it++) {
            const double alpha = nom / den;
            vk_axpby(nd, alpha, d, 1.0, x, s);
            vk_axpby(nd, -alpha, z, 1.0, r, s);
            op.mg->Apply(r, z);
            betanom = op.dot(r, z);
            if (betanom < 0.0) { o.flag = (int)pcg::MAX_ITER; break; }
            if (betanom <= r0) { o.flag = (int)pcg::CONVERGED; break; }
            if (it >= set.max_iter) { o.flag = (int)pcg::MAX_ITER; break; }
            const double beta = betanom / nom;
            vk_axpby(nd, 1.0, z, beta, d, s);      // d = z + beta d
            op.GradMult(d, z, true);
            den = op.dot(d, z);
            if (den <= 0.0 && op.dot(d, d) > 0.0) o.indefinite++;
            if (den == 0.0) { o.flag = (int)pcg::BREAKDOWN; break; }
            nom = betanom;
         }
   }
   o.betanom = betanom; o.iters = it;
   Finish(frame, &o, 1);
   return it;
}

void PCGSolver::SolveColumns(int nc, const double* B, double* X, int64_t ld, int nch, int* iters, double* reduction, int* flag) {
   if (nc < 1 || nc > EXA_GRAD_COLS_MAX) throw std::runtime_error("SolveColumns: between 1 and 16 columns");
   if (comm_.active() || op_.deterministic() || op_.precond == Precond::MULTIGRID)
      throw std::runtime_error("the batched tangent solve is built for one rank in non-deterministic mode with the identity or Jacobi preconditioner");
   NonlinearMechOperator& op = op_;
   hipStream_t s = op.stream();
   const int64_t nd = op.Height(), nn = op.part().NN;
   if (ld < nd) throw std::runtime_error("SolveColumns: column stride shorter than the vectors");
   Frame frame(s);
   DevBuf<double> R((size_t)nc * nd), Z((size_t)nc * nd), D((size_t)nc * nd);
   EXA_HC(hipMemsetAsync(record(), 0, sizeof(double) * nc * pcg::LEN, s));
   const bool ident = op.precond == Precond::IDENTITY;
   std::vector<const double*> gates(nc);
   for (int m = 0; m < nc; m++) {
      double* S = record(m); gates[m] = S + pcg::FLAG;
      double* r = R.p + (size_t)m * nd; double* z = Z.p + (size_t)m * nd; double* d = D.p + (size_t)m * nd;
      EXA_HC(hipMemsetAsync(X + (size_t)m * ld, 0, sizeof(double) * nd, s));
      EXA_HC(hipMemcpyAsync(r, B + (size_t)m * ld, sizeof(double) * nd, hipMemcpyDeviceToDevice, s));
      vk_pointwise(nd, op.dinv.p, r, z, s);
      EXA_HC(hipMemcpyAsync(d, z, sizeof(double) * nd, hipMemcpyDeviceToDevice, s));
      vk_dot(nd, nn, op.weight.p, d, r, nullptr, op.partial.p, S + pcg::RED0, s);
      vk_cg_init(S, set.rel_tol, set.abs_tol, s);
   }
   // Z += K_uu D on the columns still running: one pass over the records per nch columns, then the periodic sum of every column (the control
   // slots are essential in every solve of the tangent, so the masked direction is its own expansion: no PeriodicCell::Expand); the output mask rides
   // in the dot product that follows
   auto action = [&]() {
      if (!op.GradMultRawCols(nch, nc, D.p, nd, Z.p, nd, op.ess_mask.p, gates.data()))
         throw std::runtime_error("the batched tangent solve needs the p = 1 hexahedron L-vector record action with atomic scatter (exa_grad_apply_lvec_cols)");
      for (int m = 0; m < nc; m++) op.SumLVector(Z.p + (size_t)m * nd, gates[m], false);
      for (int m = 0; m < nc; m++) { double* S = record(m); vk_mask_dot(nd, nn, op.weight.p, op.ess_mask.p, D.p + (size_t)m * nd, Z.p + (size_t)m * nd, S + pcg::FLAG, op.partial.p, S + pcg::RED0, s, S); }
   };
   for (int m = 0; m < nc; m++) vk_fill_if(nd, gates[m], 0.0, Z.p + (size_t)m * nd, s);
   action();
   auto iteration = [&]() {
      for (int m = 0; m < nc; m++) {
         double* S = record(m);
         double* r = R.p + (size_t)m * nd; double* z = Z.p + (size_t)m * nd; double* d = D.p + (size_t)m * nd;
         vk_cg_step1(nd, nn, S, op.weight.p, op.dinv.p, d, X + (size_t)m * ld, r, z, op.partial.p, ident, true, set.max_iter, s);
         vk_cg_step2z(nd, S, z, r, d, ident, s);
      }
      action();
   };
   Outcome o[EXA_GRAD_COLS_MAX];
   int launched = 0; bool done = false;
   while (!done) {
      for (int k = 0; k < set.check_every && launched < set.max_iter; k++, launched++) iteration();
      ReadRecords(nc, false, o);
      done = launched >= set.max_iter;
      bool all = true;
      for (int m = 0; m < nc; m++) all = all && o[m].flag != (int)pcg::RUNNING;
      done = done || all;
   }
   Finish(frame, o, nc);
   for (int m = 0; m < nc; m++) {
      iters[m] = o[m].iters;
      reduction[m] = o[m].reduction();
      flag[m] = o[m].flag == (int)pcg::RUNNING ? (int)pcg::MAX_ITER : o[m].flag;
   }
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// GMRES(kdim).  One Arnoldi step at column i is a fixed sequence of launches on the device record S: action (+ preconditioner), multi-dot against
// v_0 ... v_i with |w|^2 as one more column, scalar kernel (column of H, coefficients), multi-axpy with the partial sums of the new |w|^2, scalar
// kernel (second pass or not; else h_i+1,i, rotations, residual, flag), the four launches of the second pass (they leave at once when it was
// not decided), normalisation.  w lives where v_i+1 will: the normalisation is in place.  The host polls the head of the record every check_every
// steps (multigrid: every step) and at the end of a cycle, and enqueues the back-substitution and x += V y when it sees a stop.
GMRESSolver::GMRESSolver(NonlinearMechOperator& op, const Settings& set_) : KrylovSolver(op, set_, "GMRES") {
   if (set.kdim < 1 || set.kdim > gmres::MAXK) throw std::runtime_error("GMRES: the Krylov dimension (gmres_kdim) is a whole number in 1 ... 100");
   S_.alloc(gmres::LEN); S_.zero(op.stream());
}

bool GMRESSolver::parse_ortho(const char* name, Ortho* out) {
   const std::string v = name ? name : "";
   if (v.empty() || v == "ifneeded") *out = Ortho::IFNEEDED; else if (v == "always") *out = Ortho::ALWAYS; else if (v == "never") *out = Ortho::NEVER;
   else if (v == "mgs") *out = Ortho::MGS; else return false;
   return true;
}

// (Several ranks: the launch that only reduces and the all-reduce are enqueued by the host, so they also run for the launches that leave at once -
//  after a stop, up to the next poll, and for a second pass that was not decided.  The stale sums they move are never read: needless collectives,
//  at most check_every steps' worth per stop, the price of not asking the device before every one.)
void GMRESSolver::Scalar(GmStage a, int cols) {
   hipStream_t s = op_.stream();
   if (comm_.active() && cols > 0) {
      GmStage r; r.stage = GmStage::REDUCE; r.reduce_cols = cols; r.force = a.force; r.gate_reorth = a.gate_reorth;
      gm_scalar(S_.p, table_.p, nb_, r, s);
      comm_.allreduce_sum(S_.p + gmres::RED, cols, s);
      a.reduce_cols = 0;
   } else a.reduce_cols = cols;
   gm_scalar(S_.p, table_.p, nb_, a, s);
}

namespace {
// the orthogonalisation of w against v_0 ... v_i, for the solver and for the probe: scalar(stage, columns of the table to sum first)
template <typename ScalarFn>
void gm_orthogonalise(int64_t n, int64_t nn, const double* wgt, const double* V, int64_t stride, int i, double* w, double* S, double* table, GMRESSolver::Ortho mode, int max_iter,
                      bool column_update, hipStream_t s, ScalarFn&& scalar) {
   GmStage coef; coef.stage = GmStage::COEF; coef.col = i;
   GmStage norm; norm.stage = GmStage::NORM; norm.col = i; norm.max_iter = max_iter; norm.column_update = column_update ? 1 : 0;
   if (mode == GMRESSolver::Ortho::MGS) {   // MFEM's order: one basis vector at a time through the same two kernels
      for (int j = 0; j <= i; j++) {
         gm_multidot(n, nn, wgt, V, stride, j, 1, w, false, S, 0, table, s);
         coef.j0 = j; coef.k = 1; scalar(coef, 1);
         gm_multiaxpy(n, nn, wgt, V, stride, j, 1, S, gmres::COEF, -1.0, w, 0, j == i ? table : nullptr, s);
      }
      scalar(norm, 1);
      return;
   }
   const int k = i + 1;
   gm_multidot(n, nn, wgt, V, stride, 0, k, w, true, S, 0, table, s);
   coef.k = k; coef.with_norm = 1; scalar(coef, k + 1);
   gm_multiaxpy(n, nn, wgt, V, stride, 0, k, S, gmres::COEF, -1.0, w, 0, table, s);
   norm.decide = mode == GMRESSolver::Ortho::IFNEEDED ? 1 : (mode == GMRESSolver::Ortho::ALWAYS ? 2 : 0);
   scalar(norm, 1);
   if (mode == GMRESSolver::Ortho::NEVER) return;
   // the second pass: c = V^T W w, w -= V c, h += c.  Always enqueued; every launch leaves at once unless the decision was taken.
   gm_multidot(n, nn, wgt, V, stride, 0, k, w, false, S, 1, table, s);
   coef.with_norm = 0; coef.accumulate = 1; coef.gate_reorth = 1; scalar(coef, k);
   gm_multiaxpy(n, nn, wgt, V, stride, 0, k, S, gmres::COEF, -1.0, w, 1, table, s);
   norm.decide = 0; norm.gate_reorth = 1; scalar(norm, 1);
}
}  // namespace

void GMRESSolver::Step(int i, Ortho mode, bool mg, bool ident) {
   NonlinearMechOperator& op = op_;
   hipStream_t s = op.stream();
   double* S = S_.p;
   const double* vi = V_.p + (size_t)i * stride_;
   double* w = V_.p + (size_t)(i + 1) * stride_;
   // w = M^-1 K v_i, the input masked and the output zero on essential rows
   if (mg) { op.GradMult(vi, t_.p, true, S + gmres::FLAG); op.mg->Apply(t_.p, w); }
   else if (ident) op.GradMult(vi, w, true, S + gmres::FLAG);
   else { op.GradMult(vi, t_.p, true, S + gmres::FLAG); gm_scale(nd_, w, t_.p, op.dinv.p, S, -1, s); }
   gm_orthogonalise(nd_, nn_, op.weight.p, V_.p, stride_, i, w, S, table_.p, mode, set.max_iter, true, s, [&](const GmStage& a, int cols) { Scalar(a, cols); });
   gm_scale(nd_, w, w, nullptr, S, gmres::SCALE, s);   // v_i+1 = w / h_i+1,i
}

int GMRESSolver::Solve(const double* b, double* x) {
   NonlinearMechOperator& op = op_;
   hipStream_t s = op.stream();
   const int64_t nd = op.Height();
   const int kdim = set.kdim;
   if (kdim < 1 || kdim > gmres::MAXK) throw std::runtime_error("GMRES: the Krylov dimension (gmres_kdim) is a whole number in 1 ... 100");
   if ((reinterpret_cast<uintptr_t>(x) & 15) != 0 || (reinterpret_cast<uintptr_t>(b) & 15) != 0) throw std::runtime_error("GMRES: the vectors must start at multiples of 16 bytes");
   Ortho mode = ortho;
   if (!ortho_forced && !parse_ortho(std::getenv("EXA_GMRES_ORTHO"), &mode)) throw std::runtime_error("EXA_GMRES_ORTHO is one of ifneeded, always, never, mgs");
   // (kdim + 2) nd doubles, at the first solve: the basis with the vector at work as its last column, and K v
   const int64_t stride = (nd + 31) / 32 * 32;
   if (nd_ != nd || V_.n < (size_t)(kdim + 1) * stride) {
      nd_ = nd; nn_ = op.part().NN; stride_ = stride; nb_ = (int)gm_blocks(nd);
      V_.alloc((size_t)(kdim + 1) * stride); t_.alloc(nd); table_.alloc((size_t)(gmres::MAXK + 2) * GM_BLOCKS);
   }
   Frame frame(s);
   double* S = S_.p; double* V0 = V_.p;
   const bool mg = op.precond == Precond::MULTIGRID, ident = op.precond == Precond::IDENTITY;
   EXA_HC(hipMemsetAsync(x, 0, sizeof(double) * nd, s));
   EXA_HC(hipMemsetAsync(S, 0, sizeof(double) * gmres::LEN, s));
   // r = M^-1 b, beta = |r|
   if (mg) op.mg->Apply(b, V0); else gm_scale(nd, V0, b, ident ? nullptr : op.dinv.p, S, -1, s);
   gm_multidot(nd, nn_, op.weight.p, V_.p, stride_, 0, 0, V0, true, S, 0, table_.p, s);
   { GmStage a; a.stage = GmStage::START; a.force = 1; a.rel_tol = set.rel_tol; a.abs_tol = set.abs_tol; Scalar(a, 1); }
   gm_scale(nd, V0, V0, nullptr, S, gmres::SCALE, s);
   const int every = mg ? 1 : std::max(1, set.check_every);
   double head[gmres::HEAD];
   int i = 0, launched = 0, since_poll = 0;
   for (;;) {
      if (launched < set.max_iter && i < kdim) { Step(i, mode, mg, ident); i++; launched++; since_poll++; }
      if (launched < set.max_iter && i < kdim && since_poll < every) continue;
      S_.download(head, gmres::HEAD, s); since_poll = 0;
      if (head[gmres::FLAG] != pcg::RUNNING) break;
      if (launched >= set.max_iter) { head[gmres::FLAG] = pcg::MAX_ITER; break; }   // (a cap of 0: the device never saw a column)
      if (i == kdim) {
         // end of a cycle: x += V y, r = M^-1 (b - K x), beta = |r|.  The flag was just seen RUNNING, so nothing here needs its gate.
         { GmStage a; a.stage = GmStage::SOLVE; Scalar(a, 0); }
         gm_multiaxpy(nd, nn_, op.weight.p, V_.p, stride_, 0, kdim, S, gmres::Y, 1.0, x, 0, nullptr, s);
         op.GradMult(x, t_.p, true, S + gmres::FLAG);
         if (mg) { vk_axpby(nd, 1.0, b, -1.0, t_.p, s); op.mg->Apply(t_.p, V0); }
         else gm_resid(nd, V0, b, t_.p, ident ? nullptr : op.dinv.p, S, s);
         gm_multidot(nd, nn_, op.weight.p, V_.p, stride_, 0, 0, V0, true, S, 0, table_.p, s);
         { GmStage a; a.stage = GmStage::RESTART; Scalar(a, 1); }
         gm_scale(nd, V0, V0, nullptr, S, gmres::SCALE, s);
         i = 0;
      }
   }
   // the iterate of the columns that are complete (none after a stop at the start of a cycle)
   if ((int)head[gmres::NCOL] > 0) {
      { GmStage a; a.stage = GmStage::SOLVE; a.force = 1; Scalar(a, 0); }
      gm_multiaxpy(nd, nn_, op.weight.p, V_.p, stride_, 0, (int)head[gmres::NCOL], S, gmres::Y, 1.0, x, 2, nullptr, s);
   }
   Outcome o; o.flag = (int)head[gmres::FLAG]; o.iters = (int)head[gmres::ITERS];
   o.r0z0 = head[gmres::BETA0] * head[gmres::BETA0]; o.betanom = head[gmres::RESID] * head[gmres::RESID];
   if (!std::isfinite(o.betanom)) o.betanom = 0.0;
   last_beta0 = head[gmres::BETA0]; last_resid = head[gmres::RESID]; last_restarts = (int)head[gmres::RESTARTS]; last_reorth = (int)head[gmres::REORTH_PASSES];
   restarts += last_restarts; reorth_passes += last_reorth;
   Finish(frame, &o, 1);
   return o.iters;
}

void gmres_ortho_probe(int64_t n, int k, const double* weight, const double* V, const double* w, double flag, int mode, double* h, double* w_out, double* wnorm2, int* passes) {
   if (n < 1 || k < 1 || k > gmres::MAXK) throw std::runtime_error("gmres_ortho_probe: n >= 1 and 1 <= k <= 100");
   if (mode < 0 || mode > 3) throw std::runtime_error("gmres_ortho_probe: mode 0 (ifneeded), 1 (always), 2 (never) or 3 (mgs)");
   hipStream_t s = nullptr;
   const int64_t stride = (n + 31) / 32 * 32;
   const int nb = (int)gm_blocks(n);
   DevBuf<double> dV((size_t)(k + 1) * stride), dwgt((size_t)n), S((size_t)gmres::LEN), table((size_t)(gmres::MAXK + 2) * GM_BLOCKS);
   dV.zero(s); S.zero(s);
   for (int j = 0; j < k; j++) EXA_HC(hipMemcpyAsync(dV.p + (size_t)j * stride, V + (size_t)j * n, sizeof(double) * n, hipMemcpyHostToDevice, s));
   double* dw = dV.p + (size_t)k * stride;
   EXA_HC(hipMemcpyAsync(dw, w, sizeof(double) * n, hipMemcpyHostToDevice, s));
   EXA_HC(hipMemcpyAsync(dwgt.p, weight, sizeof(double) * n, hipMemcpyHostToDevice, s));
   EXA_HC(hipMemcpyAsync(S.p + gmres::FLAG, &flag, sizeof(double), hipMemcpyHostToDevice, s));
   EXA_HC(hipStreamSynchronize(s));
   gm_orthogonalise(n, n, dwgt.p, dV.p, stride, k - 1, dw, S.p, table.p, (GMRESSolver::Ortho)mode, 0, false, s,
                    [&](GmStage a, int cols) { a.reduce_cols = cols; gm_scalar(S.p, table.p, nb, a, s); });
   std::vector<double> rec = S.to_host(s);
   EXA_HC(hipMemcpyAsync(w_out, dw, sizeof(double) * n, hipMemcpyDeviceToHost, s)); EXA_HC(hipStreamSynchronize(s));
   for (int j = 0; j < k; j++) h[j] = rec[gmres::H + (k - 1) * gmres::LDH + j];
   *wnorm2 = rec[gmres::HNEXT] * rec[gmres::HNEXT];
   *passes = flag != 0.0 ? 0 : 1 + (int)rec[gmres::REORTH_PASSES];
}

double gmres_ortho_bench(int64_t n, int col, int mode, int reps) {
   if (n < 1 || col < 0 || col >= gmres::MAXK || reps < 1 || mode < 0 || mode > 3) throw std::runtime_error("gmres_ortho_bench: n >= 1, 0 <= col < 100, reps >= 1, mode 0 ... 3");
   hipStream_t s = nullptr;
   const int64_t stride = (n + 31) / 32 * 32;
   const int nb = (int)gm_blocks(n), k = col + 1;
   DevBuf<double> V((size_t)(k + 1) * stride), wgt((size_t)n), S((size_t)gmres::LEN), table((size_t)(gmres::MAXK + 2) * GM_BLOCKS);
   // constant vectors of unit norm in the span of one direction: the first pass leaves w = 0 and every later one keeps it there - plain numbers, the same traffic
   vk_fill_if((int64_t)(k + 1) * stride, nullptr, 1.0 / std::sqrt((double)n * k), V.p, s);
   vk_fill_if(n, nullptr, 1.0, wgt.p, s);
   S.zero(s);
   double* w = V.p + (size_t)k * stride;
   auto once = [&]() {
      gm_orthogonalise(n, n, wgt.p, V.p, stride, col, w, S.p, table.p, (GMRESSolver::Ortho)mode, 0, false, s, [&](GmStage a, int cols) { a.reduce_cols = cols; gm_scalar(S.p, table.p, nb, a, s); });
      gm_scale(n, w, w, nullptr, S.p, gmres::SCALE, s);
   };
   once(); once();
   hipEvent_t e0, e1; EXA_HC(hipEventCreate(&e0)); EXA_HC(hipEventCreate(&e1));
   EXA_HC(hipEventRecord(e0, s));
   for (int r = 0; r < reps; r++) once();
   EXA_HC(hipEventRecord(e1, s)); EXA_HC(hipEventSynchronize(e1));
   float ms = 0; EXA_HC(hipEventElapsedTime(&ms, e0, e1));
   (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
   return (double)ms / reps;
}

}  // namespace exa_host
