// Linear solvers of the Newton correction: MFEM's CGSolver and GMRESSolver (linalg/solvers.cpp, Mult with iterative_mode = false; set up at reference
// src/system_driver.cpp:152-177) on device-resident vectors and scalars, behind one base class.  One object owns everything a solve needs besides the operator: work
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

// What the run, the diagnostics and the timers see of a linear solver, whichever it is: settings, one Solve, the counters of MFEM's messages and
// the totals.  The prologue (Frame) and the epilogue (Finish) of a solve are shared too.
class KrylovSolver {
 public:
   struct Settings {
      double rel_tol = 1e-10, abs_tol = 1e-30; int max_iter = 200;   // Solvers.Krylov.rel_tol / abs_tol / iter
      int check_every = 16;                                          // iterations between two polls of the done flag (the chunk a graph holds)
      // iterations replayed from a hipGraph up to this many local dofs (32^3 elements at p = 1: +9 % at 16^3, +3 % at 32^3, a loss from 48^3 on);
      // EXA_PCG_GRAPH=0 | all (SystemDriver::init); 0 after a capture that failed
      int64_t graph_max_dofs = 3 * 33 * 33 * 33;
      bool verbose = false;                                          // MFEM's messages on rank 0 (EXA_VERBOSE prints them too)
      int kdim = 50;                                                 // GMRES: Krylov dimension of a cycle (Solvers.Krylov.gmres_kdim)
   };
   // what MFEM's CGSolver prints: flag of the last solve (pcg::CONVERGED / MAX_ITER / BREAKDOWN), solves that did not converge, iterations that saw
   // (Ad, d) < 0; |r|_M / |r0|_M of the last solve and the worst among the solves that did not converge
   struct Diagnostics { int last_flag = 1; int64_t not_converged = 0, indefinite_iters = 0; double last_reduction = 0.0, worst_capped_reduction = 0.0; };

   KrylovSolver(NonlinearMechOperator& op, const Settings& set, const char* name);
   virtual ~KrylovSolver() = default;
   KrylovSolver(const KrylovSolver&) = delete; KrylovSolver& operator=(const KrylovSolver&) = delete;

   virtual int Solve(const double* b, double* x) = 0;   // x = K_uu^-1 b from x = 0; returns the iterations
   virtual void DropGraph() {}                          // forget whatever bakes in a buffer or a table that is about to change
   virtual bool gmres() const { return false; }

   Settings set;
   Diagnostics diag;
   // what the last solve left per column (a single solve: column 0): iterations, flag, iterations that saw (Ad, d) < 0, (r0, z0) and the last (r, z)
   // as the read-back of the device record gave them (multigrid: as the host loop had them; GMRES: the squares of beta0 and of the last residual)
   struct Last { int iters = 0, flag = 0, indefinite = 0; double r0z0 = 0.0, rz = 0.0; };
   Last last[16];   // EXA_GRAD_COLS_MAX columns
   double krylov_ms = 0.0; int64_t krylov_iters = 0;   // totals over all solves since ResetTotals
   void ResetTotals() { krylov_ms = 0.0; krylov_iters = 0; }

 protected:
   struct Frame;      // prologue of a solve: profiler range and start event
   // what the epilogue needs of a solved system; reduction: sqrt((r, M^-1 r) / (r0, M^-1 r0)), what a solve that stopped at max_iter reached
   struct Outcome {
      int flag = 0, iters = 0, indefinite = 0; double betanom = 0.0, r0z0 = 0.0;
      double reduction() const { return r0z0 > 0.0 ? std::sqrt(std::fmax(betanom, 0.0) / r0z0) : 0.0; }
   };
   void Finish(Frame& f, const Outcome* o, int n);          // the one epilogue: time, totals, diagnostics, messages

   NonlinearMechOperator& op_; Comm& comm_;
   const char* name_;   // "PCG" / "GMRES" in the messages
};

class PCGSolver : public KrylovSolver {
 public:
   PCGSolver(NonlinearMechOperator& op, const Settings& set);
   ~PCGSolver() override { DropGraph(); }

   // x = K_uu^-1 b from x = 0; returns the iterations.  Multigrid preconditioner: the host-scalar loop; several ranks or a forced communicator:
   // the single-reduction loop (EXA_PCG_TWO_REDUCTIONS=1: the next one); else the device-scalar loop with graph replay and consumer-side reductions
   int Solve(const double* b, double* x) override;
   // nc <= 16 systems K_uu x_m = b_m in lockstep: recurrence and stopping test of the device-scalar loop with one record per column, the multi-column
   // action (nch columns per pass, 0: the library's default) in the middle; B, X: columns at stride ld.  No graph capture, no consumer-side
   // reductions.  One rank, non-deterministic mode, identity or Jacobi preconditioner.
   void SolveColumns(int nc, const double* B, double* X, int64_t ld, int nch, int* iters, double* reduction, int* flag);
   // forget the captured chunk: its solution buffer, or a table the operator's launches take by value, is about to change
   void DropGraph() override;

 private:
   // everything a captured chunk bakes in
   struct GraphKey {
      const double* x = nullptr; Precond precond = Precond::IDENTITY; bool consumer_side = false; int check_every = 0, max_iter = 0;
      bool operator==(const GraphKey& o) const { return x == o.x && precond == o.precond && consumer_side == o.consumer_side && check_every == o.check_every && max_iter == o.max_iter; }
   };
   int SolveDeviceScalars(const double* b, double* x);
   int SolveSingleReduction(const double* b, double* x);
   int SolveMultigrid(const double* b, double* x);
   void ReadRecords(int n, bool in_flight, Outcome* out);   // the one place the device records come back to the host
   double* record(int m = 0) const;                          // device record of column m (a single solve uses column 0)

   DevBuf<double> r_, z_, d_, s_, q_;   // s, q: single-reduction loop only (allocated on first use)
   DevBuf<double> S_;                   // pcg::LEN doubles per column
   void* graph_ = nullptr; GraphKey graph_key_;   // hipGraphExec_t of check_every iterations
};

// MFEM's GMRESSolver::Mult with iterative_mode = false (restarted GMRES(kdim), preconditioner on the left; reference src/system_driver.cpp:152-164)
// on the same operator, weights and preconditioners as PCGSolver: classical Gram-Schmidt by a multi-dot and a multi-axpy kernel with a second pass
// on the Daniel-Gragg-Kaufman-Stewart criterion, all scalars in a device record (../gmres_slots.hpp), DESIGN 4.16.  At the iteration cap the
// iterate of the columns done so far is returned as it is: no further residual evaluation.
class GMRESSolver : public KrylovSolver {
 public:
   enum class Ortho { IFNEEDED, ALWAYS, NEVER, MGS };   // EXA_GMRES_ORTHO, read once per solve
   static bool parse_ortho(const char* name, Ortho* out);
   GMRESSolver(NonlinearMechOperator& op, const Settings& set);
   int Solve(const double* b, double* x) override;
   bool gmres() const override { return true; }
   bool ortho_forced = false; Ortho ortho = Ortho::IFNEEDED;      // forced: the probe's argument instead of the environment
   // of the last solve: |M^-1 b|, the last residual norm, restarts and second Gram-Schmidt passes; totals over all solves
   double last_beta0 = 0.0, last_resid = 0.0; int last_restarts = 0, last_reorth = 0;
   int64_t restarts = 0, reorth_passes = 0;
   size_t basis_bytes() const { return sizeof(double) * (V_.n + t_.n); }
 private:
   void Step(int i, Ortho mode, bool mg, bool ident);
   void Scalar(GmStage a, int cols);   // partial sums of cols columns -> record, all-reduce on several ranks, then the stage
   int64_t nd_ = 0, nn_ = 0, stride_ = 0; int nb_ = 0;
   DevBuf<double> V_, t_, table_, S_;   // kdim + 1 basis vectors (allocated at the first solve), K v, the partial-sum table, the record
};

// The orthogonalisation of one column on shapes a driver cannot produce (exa_gmres_ortho_probe): host arrays in and out, V k vectors of n entries,
// mode 0 ... 3 = Ortho; passes: 0 when the flag was set, else 1 + second passes
void gmres_ortho_probe(int64_t n, int k, const double* weight, const double* V, const double* w, double flag, int mode, double* h, double* w_out, double* wnorm2, int* passes);
// ms per orthogonalisation of column col (col + 1 basis vectors of n entries) with its normalisation, device buffers of the call's own (exa_gmres_ortho_bench)
double gmres_ortho_bench(int64_t n, int col, int mode, int reps);

}  // namespace exa_host
