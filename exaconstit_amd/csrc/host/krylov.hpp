// Linear solver of the Newton correction: MFEM's CGSolver (linalg/solvers.cpp, CGSolver::Mult with iterative_mode = false; set up at reference
// src/system_driver.cpp:166-177) on device-resident vectors and scalars.  One object owns everything a solve needs besides the operator: work
// vectors, the device scalar record (../pcg_slots.hpp), the captured chunk of iterations, settings, diagnostics and totals.  Whoever needs solves
// with other settings builds a second object (host/tangent.hip, the benchmark hook of host/driver_capi.hip) and leaves the run's alone.
#pragma once
#include <cmath>
#include <cstdint>
#include "device_utils.hpp"

namespace exa_host {

class NonlinearMechOperator;
class Comm;
enum class Precond { IDENTITY, JACOBI, MULTIGRID };

class PCGSolver {
 public:
   struct Settings {
      double rel_tol = 1e-10, abs_tol = 1e-30; int max_iter = 200;   // Solvers.Krylov.rel_tol / abs_tol / iter
      int check_every = 16;                                          // iterations between two polls of the done flag (the chunk a graph holds)
      // iterations replayed from a hipGraph up to this many local dofs (32^3 elements at p = 1: +9 % at 16^3, +3 % at 32^3, a loss from 48^3 on);
      // EXA_PCG_GRAPH=0 | all (SystemDriver::init); 0 after a capture that failed
      int64_t graph_max_dofs = 3 * 33 * 33 * 33;
      bool verbose = false;                                          // MFEM's messages on rank 0 (EXA_VERBOSE prints them too)
   };
   // what MFEM's CGSolver prints: flag of the last solve (pcg::CONVERGED / MAX_ITER / BREAKDOWN), solves that did not converge, iterations that saw
   // (Ad, d) < 0; |r|_M / |r0|_M of the last solve and the worst among the solves that did not converge
   struct Diagnostics { int last_flag = 1; int64_t not_converged = 0, indefinite_iters = 0; double last_reduction = 0.0, worst_capped_reduction = 0.0; };

   PCGSolver(NonlinearMechOperator& op, const Settings& set);
   ~PCGSolver() { DropGraph(); }
   PCGSolver(const PCGSolver&) = delete; PCGSolver& operator=(const PCGSolver&) = delete;

   // x = K_uu^-1 b from x = 0; returns the iterations.  Multigrid preconditioner: the host-scalar loop; several ranks or a forced communicator:
   // the single-reduction loop (EXA_PCG_TWO_REDUCTIONS=1: the next one); else the device-scalar loop with graph replay and consumer-side reductions
   int Solve(const double* b, double* x);
   // nc <= 16 systems K_uu x_m = b_m in lockstep: recurrence and stopping test of the device-scalar loop with one record per column, the multi-column
   // action (nch columns per pass, 0: the library's default) in the middle; B, X: columns at stride ld.  No graph capture, no consumer-side
   // reductions.  One rank, non-deterministic mode, identity or Jacobi preconditioner.
   void SolveColumns(int nc, const double* B, double* X, int64_t ld, int nch, int* iters, double* reduction, int* flag);
   // forget the captured chunk: its solution buffer, or a table the operator's launches take by value, is about to change
   void DropGraph();

   Settings set;
   Diagnostics diag;
   // what the last solve left per column (a single solve: column 0): iterations, flag, iterations that saw (Ad, d) < 0, (r0, z0) and the last (r, z)
   // as the read-back of the device record gave them (multigrid: as the host loop had them)
   struct Last { int iters = 0, flag = 0, indefinite = 0; double r0z0 = 0.0, rz = 0.0; };
   Last last[16];   // EXA_GRAD_COLS_MAX columns
   double krylov_ms = 0.0; int64_t krylov_iters = 0;   // totals over all solves since ResetTotals
   void ResetTotals() { krylov_ms = 0.0; krylov_iters = 0; }

 private:
   struct Frame;      // prologue of a solve: profiler range and start event
   // what the epilogue needs of a solved system; reduction: sqrt((r, M^-1 r) / (r0, M^-1 r0)), what a solve that stopped at max_iter reached
   struct Outcome {
      int flag = 0, iters = 0, indefinite = 0; double betanom = 0.0, r0z0 = 0.0;
      double reduction() const { return r0z0 > 0.0 ? std::sqrt(std::fmax(betanom, 0.0) / r0z0) : 0.0; }
   };
   // everything a captured chunk bakes in
   struct GraphKey {
      const double* x = nullptr; Precond precond = Precond::IDENTITY; bool consumer_side = false; int check_every = 0, max_iter = 0;
      bool operator==(const GraphKey& o) const { return x == o.x && precond == o.precond && consumer_side == o.consumer_side && check_every == o.check_every && max_iter == o.max_iter; }
   };
   int SolveDeviceScalars(const double* b, double* x);
   int SolveSingleReduction(const double* b, double* x);
   int SolveMultigrid(const double* b, double* x);
   void ReadRecords(int n, bool in_flight, Outcome* out);   // the one place the device records come back to the host
   void Finish(Frame& f, const Outcome* o, int n);          // the one epilogue: time, totals, diagnostics, messages
   double* record(int m = 0) const;                          // device record of column m (a single solve uses column 0)

   NonlinearMechOperator& op_; Comm& comm_;
   DevBuf<double> r_, z_, d_, s_, q_;   // s, q: single-reduction loop only (allocated on first use)
   DevBuf<double> S_;                   // pcg::LEN doubles per column
   void* graph_ = nullptr; GraphKey graph_key_;   // hipGraphExec_t of check_every iterations
};

}  // namespace exa_host
