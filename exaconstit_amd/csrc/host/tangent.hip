// Homogenised tangent of a periodic RVE: d sigma_bar / d L_bar of the converged step from nine fluctuation solves with the
// operator, the periodic sum and the PCG the step itself used.
//
//   K        the operator of the Krylov action in force (d f / d v, with the dt factor the gradient set-up folds in) at the state of the last
//            residual evaluation of the last solved step; K_raw: its element action on a field as it stands - no essential mask, no expansion
//            of control values, no sum over periodic images or ranks
//   a_m      the affine nodal field E_m (x_cur - origin), m = 1 .. 9, E_m the unit 3 x 3 matrices row by row (not periodic)
//   b_m      the assembled form of - K_raw a_m: periodic and rank sums (SumLVector, raw = false), then the essential mask - the run's own set
//            plus, on a mixed partition, all nine control slots: the eight corners, every component
//   w_m      K_uu w_m = b_m by the run's PCG: a fluctuation of the periodic space, zero on the corners
//   T        T_(kl),m = sum over the local nodes of (K_raw (a_m + w_m))_k (x_l - o_l), summed over the ranks;  T / V = d sigma_bar_kl / d L_bar_m
//            by Hill-Mandel (V the current cell volume).  Every column of a raw action sums to zero over the nodes, so the origin drops out.
//
// Two routes for the nine solves, both through a PCGSolver (host/krylov.hpp) built for the evaluation with its tolerance and cap.  Batched (one rank,
// non-deterministic mode, a context exa_grad_apply_lvec_cols serves): SolveColumns runs the columns in lockstep around the multi-column action of
// tangent_kernels.hip.  Everywhere else - several ranks, EXA_DETERMINISTIC=1, p >= 2, assembled element matrices, B-bar - the columns go one by one
// through Solve into one fixed solution buffer.
#include "driver.hpp"
#include <cmath>
#include <cstring>
#include <fstream>
#include <iomanip>

int exa_launch_affine_columns(exa_ctx* ctx, int nn, const double* xc, const double* org3, double* out, int64_t ld, hipStream_t s);   // tangent_kernels.hip
int exa_launch_macro_contract(exa_ctx* ctx, int nn, int ncols, const double* y, int64_t ldy, const double* xc, const double* org3, double* work, double* out, hipStream_t s);

namespace exa_host {

namespace {
constexpr int MACRO_WORK = 256 * 81;   // block partials of the contraction (tangent_kernels.hip, EXA_MACRO_BLOCKS)
void abi(exa_ctx* ctx, int rc, const char* what) { if (rc < 0) throw std::runtime_error(std::string(what) + ": " + exa_last_error(ctx)); }
int env_int(const char* k, int dflt) { const char* e = std::getenv(k); return e ? std::atoi(e) : dflt; }
}

// What an evaluation shares with the run and puts back: the essential mask and the free bits (mixed partitions: the solves fix all nine control
// slots) and the operator's own scalars.  The solves run in a PCGSolver of the evaluation's own, so the run's Krylov settings, diagnostics, totals
// and captured chunk are never touched; the records, the Newton cap state, stats and the model timers are never written: no constitutive launch runs.
struct SystemDriver::TangentScope {
   SystemDriver& sd; NonlinearMechOperator& op;
   double scal[NonlinearMechOperator::SCAL_LEN]; uint32_t free_bits = 0; bool mask_changed = false; bool closed = false;
   TangentScope(SystemDriver& d) : sd(d), op(*d.oper_) {
      op.scal.download(scal, NonlinearMechOperator::SCAL_LEN, op.stream());
      if (sd.mix_.on) {
         free_bits = op.cell()->free_bits();
         std::vector<uint8_t> m = sd.ess_host_;
         const int nn = sd.part.NN;
         for (int d3 = 0; d3 < 3; d3++) if (sd.part.ctrl_node[1 + d3] >= 0) for (int k = 0; k < 3; k++) m[(size_t)sd.part.ctrl_node[1 + d3] + (size_t)nn * k] = 1;
         op.UpdateEssTDofs(m); op.cell()->set_free_bits(0);
         mask_changed = true;
      }
   }
   void close() {
      if (closed) return;
      closed = true;
      hipStream_t s = op.stream();
      (void)hipStreamSynchronize(s);
      if (mask_changed) {
         op.UpdateEssTDofs(sd.ess_host_); op.cell()->set_free_bits(free_bits);
         op.GetGradient();   // (the inverse diagonal follows the mask: back to the run's)
      }
      op.scal.upload(scal, NonlinearMechOperator::SCAL_LEN, s);
   }
   ~TangentScope() { try { close(); } catch (...) {} }
};

void SystemDriver::MacroTangent(double rel_tol, int max_iter, int batched, MacroTangentResult& out) {
   if (!part.periodic) throw std::runtime_error("macro_tangent: the driver is not periodic (set_periodic / BCs.periodic = true) - the homogenised tangent is that of a periodic cell");
   if (!step_solved_)
      throw std::runtime_error(restarted_ ? "macro_tangent: no step has been solved in this process since the restart - the records of the converged iterate are not part of a checkpoint; solve a step first"
                                          : "macro_tangent: no solved step - the tangent is taken at the converged iterate of the last step; solve a step first");
   NonlinearMechOperator& op = *oper_;
   hipStream_t s = op.stream();
   exa_ctx* ctx = op.GetModel()->ctx();
   const int64_t nd = op.Height(); const int nn = part.NN;
   const double rel = rel_tol > 0.0 ? rel_tol : opt_.krylov_rel;
   const int mi = max_iter > 0 ? max_iter : opt_.krylov_iter;
   const bool can_batch = !comm.active() && !op.deterministic() && op.precond != Precond::MULTIGRID;
   if (batched == 1 && !can_batch) throw std::runtime_error("macro_tangent: the batched route is built for one rank in non-deterministic mode; use batched = 0 or the automatic route");
   const int auto_env = env_int("EXA_TANGENT_BATCHED", tangent_auto_batched ? 1 : 0);
   bool want = batched < 0 ? (can_batch && auto_env != 0) : batched == 1;
   const int nch = tangent_nch > 0 ? tangent_nch : env_int("EXA_TANGENT_NCH", 0);
   if (nch < 0 || nch > 3) throw std::runtime_error("macro_tangent: 1, 2 or 3 columns per pass");
   TangentScope scope(*this);
   PCGSolver::Settings ks = krylov_->set;   // (chunk length and graph limit as the run has them: a capture that failed is not tried again)
   ks.rel_tol = rel; ks.max_iter = mi;
   PCGSolver pcg(op, ks);
   op.GetGradient();
   DevBuf<double> A((size_t)9 * nd), W((size_t)9 * nd), Bv((size_t)9 * nd), tmp((size_t)nd), small(3 + 81), work((size_t)MACRO_WORK);
   double org[3];
   vk_min3(nn, op.x_cur.p, op.partial.p, small.p, s); comm.allreduce_min(small.p, 3, s);
   small.download(org, 3, s);
   abi(ctx, exa_launch_affine_columns(ctx, nn, op.x_cur.p, org, A.p, nd, s), "k_affine_columns");
   // nine raw actions: in one call where the context has the multi-column kernel, one by one elsewhere
   auto raw9 = [&](const double* X, double* Y) {
      if (want) {
         EXA_HC(hipMemsetAsync(Y, 0, sizeof(double) * 9 * nd, s));
         if (op.GradMultRawCols(nch, 9, X, nd, Y, nd, nullptr, nullptr)) return;
         if (batched == 1) throw std::runtime_error("macro_tangent: the batched route needs the p = 1 hexahedron L-vector record action with atomic scatter; use batched = 0 or the automatic route");
         want = false;
      }
      for (int m = 0; m < 9; m++) op.GradMultRaw(X + (size_t)m * nd, Y + (size_t)m * nd);
   };
   raw9(A.p, Bv.p);
   vk_axpby(9 * nd, 0.0, Bv.p, -1.0, Bv.p, s);
   for (int m = 0; m < 9; m++) {
      double* b = Bv.p + (size_t)m * nd;
      op.SumLVector(b, nullptr, false);
      vk_mask_zero(nd, op.ess_mask.p, b, s);
      out.b_norm[m] = std::sqrt(std::fmax(op.dot(b, b), 0.0));
   }
   if (want) pcg.SolveColumns(9, Bv.p, W.p, nd, nch, out.iters, out.reduction, out.flag);
   else {
      // one fixed solution buffer (tmp): the PCG chunk is captured once for it and replayed by all nine solves
      for (int m = 0; m < 9; m++) {
         out.iters[m] = pcg.Solve(Bv.p + (size_t)m * nd, tmp.p);
         out.reduction[m] = pcg.diag.last_reduction; out.flag[m] = pcg.diag.last_flag;
         EXA_HC(hipMemcpyAsync(W.p + (size_t)m * nd, tmp.p, sizeof(double) * nd, hipMemcpyDeviceToDevice, s));
      }
   }
   out.batched = want ? 1 : 0; out.nch = want ? (nch ? nch : EXA_GRAD_COLS_DEFAULT) : 0;
   // true residual |b - K_uu w| by one more action, and the size of the fluctuation
   for (int m = 0; m < 9; m++) {
      op.GradMult(W.p + (size_t)m * nd, tmp.p, true);
      vk_axpby(nd, 1.0, Bv.p + (size_t)m * nd, -1.0, tmp.p, s);
      out.res_norm[m] = std::sqrt(std::fmax(op.dot(tmp.p, tmp.p), 0.0));
      vk_max_abs_diff(nd, W.p + (size_t)m * nd, W.p + (size_t)m * nd, small.p, s);   // (out[1] = max |w|)
      double h3[3]; small.download(h3, 3, s); const double wmax = comm.max_over_ranks(h3[1]);
      vk_max_abs_diff(nd, A.p + (size_t)m * nd, A.p + (size_t)m * nd, small.p, s);
      small.download(h3, 3, s); const double amax = comm.max_over_ranks(h3[1]);
      out.w_over_a[m] = amax > 0.0 ? wmax / amax : 0.0;
   }
   // T = sum over the nodes of K_raw (a + w) (x) (x - o)
   vk_axpby(9 * nd, 1.0, W.p, 1.0, A.p, s);
   raw9(A.p, Bv.p);
   abi(ctx, exa_launch_macro_contract(ctx, nn, 9, Bv.p, nd, op.x_cur.p, org, work.p, small.p + 3, s), "k_macro_contract");
   comm.allreduce_sum(small.p + 3, 81, s);
   double t81[81]; EXA_HC(hipMemcpyAsync(t81, small.p + 3, sizeof(t81), hipMemcpyDeviceToHost, s)); EXA_HC(hipStreamSynchronize(s));
   for (int m = 0; m < 9; m++) for (int kl = 0; kl < 9; kl++) out.T[9 * kl + m] = t81[9 * m + kl];
   // current cell volume: sum of W det J of the current configuration (the Jacobians of x_cur, as the volume averages of the step take them)
   op.RefreshJacobians();
   { double h[7]; abi(ctx, exa_vol_avg(ctx, op.el_jac.p, op.stress0.p, 6, 0, h, s), "exa_vol_avg");
     if (comm.nranks > 1) { small.upload(h + 6, 1, s); comm.allreduce_sum(small.p, 1, s); small.download(h + 6, 1, s); }
     out.V = h[6]; }
   out.dt = op.dt();
   scope.close();
}

void SystemDriver::GradApplyColumns(int nc, const double* x, double* y, bool assembled, bool batched, const int* gated) {
   if (nc < 1 || nc > EXA_GRAD_COLS_MAX) throw std::runtime_error("grad_apply_columns: between 1 and 16 columns");
   if (!step_solved_) throw std::runtime_error("grad_apply_columns: no solved step - the operator is that of the converged iterate of the last step");
   NonlinearMechOperator& op = *oper_;
   hipStream_t s = op.stream();
   const int64_t nd = op.Height();
   if (batched && comm.active()) throw std::runtime_error("grad_apply_columns: the batched route is built for one rank");
   const int nch = tangent_nch > 0 ? tangent_nch : env_int("EXA_TANGENT_NCH", 0);
   TangentScope scope(*this);
   op.GetGradient();
   DevBuf<double> X((size_t)nc * nd), Y((size_t)nc * nd), G((size_t)nc);
   X.upload(x, (size_t)nc * nd, s);
   std::vector<double> gh(nc, 0.0); std::vector<const double*> gp(nc, nullptr);
   if (gated) { Y.upload(y, (size_t)nc * nd, s); for (int m = 0; m < nc; m++) { gh[m] = gated[m] ? 1.0 : 0.0; gp[m] = G.p + m; } G.upload(gh.data(), nc, s); }
   const uint8_t* mask = assembled ? op.ess_mask.p : nullptr;
   if (batched) {
      for (int m = 0; m < nc; m++) if (gh[m] == 0.0) EXA_HC(hipMemsetAsync(Y.p + (size_t)m * nd, 0, sizeof(double) * nd, s));
      if (!op.GradMultRawCols(nch, nc, X.p, nd, Y.p, nd, mask, gated ? gp.data() : nullptr))
         throw std::runtime_error("grad_apply_columns: this context has no multi-column action (exa_grad_apply_lvec_cols: p = 1 hexahedra, L-vector record action, atomic scatter)");
      if (assembled) for (int m = 0; m < nc; m++) if (gh[m] == 0.0) { op.SumLVector(Y.p + (size_t)m * nd, nullptr, false); vk_mask_zero(nd, op.ess_mask.p, Y.p + (size_t)m * nd, s); }
   } else {
      for (int m = 0; m < nc; m++) {
         if (gh[m] != 0.0) continue;
         if (assembled) op.GradMult(X.p + (size_t)m * nd, Y.p + (size_t)m * nd, true);
         else op.GradMultRaw(X.p + (size_t)m * nd, Y.p + (size_t)m * nd);
      }
   }
   Y.download(y, (size_t)nc * nd, s);
   scope.close();
}

void SystemDriver::PcgSolveProbe(int nc, const double* b, double rel_tol, double abs_tol, int max_iter, int check_every, int graph, int mode, double* x, int* iters, int* flag,
                                 double* reduction, int* indefinite, double* sc) {
   if (nc < 1 || nc > EXA_GRAD_COLS_MAX) throw std::runtime_error("pcg_solve: between 1 and 16 columns");
   if (!step_solved_) throw std::runtime_error("pcg_solve: no solved step - the operator is that of the converged iterate of the last step");
   if (mode != 0 && mode != 1) throw std::runtime_error("pcg_solve: mode 0 (Solve, column by column) or 1 (SolveColumns)");
   if (graph < -1 || graph > 1) throw std::runtime_error("pcg_solve: graph -1 (as the run), 0 (off) or 1 (on)");
   if (max_iter < 0 || check_every < 0 || !(rel_tol >= 0.0) || !(abs_tol >= 0.0)) throw std::runtime_error("pcg_solve: tolerances, max_iter and check_every must not be negative");
   NonlinearMechOperator& op = *oper_;
   hipStream_t s = op.stream();
   const int64_t nd = op.Height();
   const int nch = tangent_nch > 0 ? tangent_nch : env_int("EXA_TANGENT_NCH", 0);
   TangentScope scope(*this);
   op.GetGradient();
   PCGSolver::Settings ks = krylov_->set;
   ks.rel_tol = rel_tol; ks.abs_tol = abs_tol; ks.max_iter = max_iter;
   if (check_every > 0) ks.check_every = check_every;
   if (graph == 0) ks.graph_max_dofs = 0; else if (graph == 1) ks.graph_max_dofs = INT64_MAX;
   PCGSolver pcg(op, ks);
   DevBuf<double> B((size_t)nc * nd), X((size_t)nc * nd);
   B.upload(b, (size_t)nc * nd, s);
   DevBuf<double> tmp((size_t)nd);   // mode 0: one fixed solution buffer, as the tangent's column-by-column route has it
   if (mode == 1) {
      std::vector<int> it(nc), fl(nc); std::vector<double> red(nc);
      pcg.SolveColumns(nc, B.p, X.p, nd, nch, it.data(), red.data(), fl.data());
      for (int m = 0; m < nc; m++) {
         const PCGSolver::Last& l = pcg.last[m];
         iters[m] = it[m]; flag[m] = fl[m]; reduction[m] = red[m]; indefinite[m] = l.indefinite; sc[2 * m] = l.r0z0; sc[2 * m + 1] = l.rz;
      }
   } else {
      for (int m = 0; m < nc; m++) {
         iters[m] = pcg.Solve(B.p + (size_t)m * nd, tmp.p);
         const PCGSolver::Last& l = pcg.last[0];
         flag[m] = pcg.diag.last_flag; reduction[m] = pcg.diag.last_reduction; indefinite[m] = l.indefinite; sc[2 * m] = l.r0z0; sc[2 * m + 1] = l.rz;
         EXA_HC(hipMemcpyAsync(X.p + (size_t)m * nd, tmp.p, sizeof(double) * nd, hipMemcpyDeviceToDevice, s));
      }
   }
   X.download(x, (size_t)nc * nd, s);
   scope.close();
}

void SystemDriver::GmresSolveProbe(int nc, const double* b, double rel_tol, double abs_tol, int max_iter, int kdim, int check_every, int ortho, double* x, int* iters, int* flag,
                                   double* reduction, double* sc) {
   if (nc < 1 || nc > EXA_GRAD_COLS_MAX) throw std::runtime_error("gmres_solve: between 1 and 16 columns");
   if (!step_solved_) throw std::runtime_error("gmres_solve: no solved step - the operator is that of the converged iterate of the last step");
   if (kdim < 1 || kdim > 100) throw std::runtime_error("gmres_solve: " + std::string(ExaOptions::gmres_kdim_range()));
   if (ortho < -1 || ortho > 3) throw std::runtime_error("gmres_solve: ortho -1 (EXA_GMRES_ORTHO), 0 ifneeded, 1 always, 2 never or 3 mgs");
   if (max_iter < 0 || check_every < 0 || !(rel_tol >= 0.0) || !(abs_tol >= 0.0)) throw std::runtime_error("gmres_solve: tolerances, max_iter and check_every must not be negative");
   NonlinearMechOperator& op = *oper_;
   hipStream_t s = op.stream();
   const int64_t nd = op.Height();
   TangentScope scope(*this);
   op.GetGradient();
   KrylovSolver::Settings ks = krylov_->set;
   ks.rel_tol = rel_tol; ks.abs_tol = abs_tol; ks.max_iter = max_iter; ks.kdim = kdim;
   if (check_every > 0) ks.check_every = check_every;
   GMRESSolver gm(op, ks);
   if (ortho >= 0) { gm.ortho_forced = true; gm.ortho = (GMRESSolver::Ortho)ortho; }
   DevBuf<double> B((size_t)nc * nd), X((size_t)nc * nd), tmp((size_t)nd), bm((size_t)nd);
   B.upload(b, (size_t)nc * nd, s);
   for (int m = 0; m < nc; m++) {
      EXA_HC(hipMemcpyAsync(bm.p, B.p + (size_t)m * nd, sizeof(double) * nd, hipMemcpyDeviceToDevice, s));
      iters[m] = gm.Solve(bm.p, tmp.p);
      flag[m] = gm.diag.last_flag; reduction[m] = gm.diag.last_reduction;
      sc[4 * m] = gm.last_beta0; sc[4 * m + 1] = gm.last_resid; sc[4 * m + 2] = gm.last_restarts; sc[4 * m + 3] = gm.last_reorth;
      EXA_HC(hipMemcpyAsync(X.p + (size_t)m * nd, tmp.p, sizeof(double) * nd, hipMemcpyDeviceToDevice, s));
   }
   X.download(x, (size_t)nc * nd, s);
   scope.close();
}

void SystemDriver::WriteMacroTangent(int step) {
   MacroTangentResult r;
   MacroTangent(opt_.macro_tangent_rel_tol, opt_.macro_tangent_max_iter, -1, r);
   double row[MACRO_TANGENT_ROW] = { (double)step, time, r.dt, r.V };
   for (int k = 0; k < 81; k++) row[4 + k] = r.T[k] / r.V;
   macro_tangent_rows.insert(macro_tangent_rows.end(), row, row + MACRO_TANGENT_ROW);
   if (comm.rank == 0) write_macro_tangent_rows(out_dir + "/" + opt_.macro_tangent_fname, std::vector<double>(row, row + MACRO_TANGENT_ROW), true);
}

void write_macro_tangent_rows(const std::string& path, const std::vector<double>& rows, bool append) {
   std::ofstream f(path, append ? std::ios_base::app : std::ios_base::trunc);
   if (!f) throw std::runtime_error("macro_tangent: cannot write " + path);
   f << std::setprecision(17);
   for (size_t i = 0; i + MACRO_TANGENT_ROW <= rows.size(); i += MACRO_TANGENT_ROW) {
      f << (long)rows[i];
      for (int k = 1; k < MACRO_TANGENT_ROW; k++) f << ' ' << rows[i + k];
      f << '\n';
   }
}

bool macro_tangent_condense(const double* c, const uint8_t* free9, double* out) {
   int fi[9], nf = 0;
   for (int k = 0; k < 9; k++) if (free9 && free9[k]) fi[nf++] = k;
   for (int k = 0; k < 81; k++) out[k] = 0.0;
   // X = C_ff^-1 C_f. by Gaussian elimination with partial pivoting on [C_ff | C_f.]
   double M[9][18];
   for (int a = 0; a < nf; a++) { for (int b = 0; b < nf; b++) M[a][b] = c[9 * fi[a] + fi[b]]; for (int n = 0; n < 9; n++) M[a][nf + n] = c[9 * fi[a] + n]; }
   for (int col = 0; col < nf; col++) {
      int piv = col;
      for (int a = col + 1; a < nf; a++) if (std::fabs(M[a][col]) > std::fabs(M[piv][col])) piv = a;
      if (M[piv][col] == 0.0 || !std::isfinite(M[piv][col])) return false;
      if (piv != col) for (int b = 0; b < nf + 9; b++) std::swap(M[piv][b], M[col][b]);
      for (int a = 0; a < nf; a++) if (a != col) {
         const double f = M[a][col] / M[col][col];
         if (f != 0.0) for (int b = col; b < nf + 9; b++) M[a][b] -= f * M[col][b];
      }
   }
   for (int k = 0; k < 9; k++) {
      if (free9 && free9[k]) continue;
      for (int n = 0; n < 9; n++) {
         if (free9 && free9[n]) continue;
         double v = c[9 * k + n];
         for (int a = 0; a < nf; a++) v -= c[9 * k + fi[a]] * (M[a][nf + n] / M[a][a]);
         out[9 * k + n] = v;
      }
   }
   return true;
}

}  // namespace exa_host
