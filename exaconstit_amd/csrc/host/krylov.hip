// PCGSolver (host/krylov.hpp): three loops for one system - device scalars, single reduction, multigrid - and the lockstep loop for several,
// between one prologue (Frame) and one epilogue (Finish).
#include "driver.hpp"
#include "multigrid.hpp"
#include "roctx.hpp"
#include "../pcg_slots.hpp"
#include <cmath>
#include <iostream>

namespace exa_host {

static_assert(sizeof(PCGSolver::last) / sizeof(PCGSolver::Last) == EXA_GRAD_COLS_MAX, "one entry per column of the lockstep solve");

PCGSolver::PCGSolver(NonlinearMechOperator& op, const Settings& set_) : set(set_), op_(op), comm_(op.comm()) {
   const size_t nd = (size_t)op.Height();
   r_.alloc(nd); z_.alloc(nd); d_.alloc(nd);
   S_.alloc((size_t)EXA_GRAD_COLS_MAX * pcg::LEN); S_.zero(op.stream());
}

double* PCGSolver::record(int m) const { return S_.p + (size_t)m * pcg::LEN; }

void PCGSolver::DropGraph() {
   if (graph_) { (void)hipGraphExecDestroy((hipGraphExec_t)graph_); graph_ = nullptr; }
   graph_key_ = GraphKey();
}

struct PCGSolver::Frame {
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

void PCGSolver::Finish(Frame& f, const Outcome* o, int n) {
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
         if (o[m].indefinite > 0) std::cerr << "PCG: The operator is not positive definite. (Ad, d) < 0 in " << o[m].indefinite << " iteration(s)\n";
         if (o[m].flag == (int)pcg::BREAKDOWN) std::cerr << "PCG: (Ad, d) = 0, stopping after " << o[m].iters << " iterations\n";
         else if (!converged) std::cerr << "PCG: No convergence! (" << o[m].iters << " iterations)\n";
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

}  // namespace exa_host
