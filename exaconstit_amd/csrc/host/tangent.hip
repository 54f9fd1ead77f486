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
// Two routes for the nine solves.  Batched (one rank, non-deterministic mode, a context exa_grad_apply_lvec_cols serves): CGSolveColumns runs
// the columns in lockstep around the multi-column action of tangent_kernels.hip.  Everywhere else - several ranks, EXA_DETERMINISTIC=1, p >= 2,
// assembled element matrices, B-bar - the columns go one by one through CGSolve into one fixed solution buffer.
#include "driver.hpp"
#include <cmath>
#include <cstring>
#include <fstream>
#include <iomanip>

int exa_launch_affine_columns(exa_ctx* ctx, int nn, const double* xc, const double* org3, double* out, int64_t ld, hipStream_t s);   // tangent_kernels.hip
int exa_launch_macro_contract(exa_ctx* ctx, int nn, int ncols, const double* y, int64_t ldy, const double* xc, const double* org3, double* work, double* out, hipStream_t s);

namespace exa_host {

namespace {
constexpr int SB = 24;                 // doubles per scalar block of a column (the PCG scalars of vec_kernels.hip use 18)
constexpr int MACRO_WORK = 256 * 81;   // block partials of the contraction (tangent_kernels.hip, EXA_MACRO_BLOCKS)
void abi(exa_ctx* ctx, int rc, const char* what) { if (rc < 0) throw std::runtime_error(std::string(what) + ": " + exa_last_error(ctx)); }
int env_int(const char* k, int dflt) { const char* e = std::getenv(k); return e ? std::atoi(e) : dflt; }
}

// Everything an evaluation changes and puts back: the essential mask and the free bits (mixed partitions: the solves fix all nine control slots),
// the Krylov options CGSolve reads, scal, the timers, the PCG diagnostics and the captured PCG chunk of the run (set aside, so that the solves
// of the tangent capture and drop their own).  The records, the Newton cap state and stats are never written: no constitutive launch runs.
struct SystemDriver::TangentScope {
   SystemDriver& sd; NonlinearMechOperator& op;
   double krylov_rel; int krylov_iter; Timers timers; int last_flag; int64_t not_conv, indef; double last_red, worst_red;
   void* graph; const double* graph_x; int64_t graph_key;
   double scal[32]; uint32_t free_bits; bool mask_changed = false; bool closed = false;
   TangentScope(SystemDriver& d) : sd(d), op(*d.oper_) {
      hipStream_t s = op.stream();
      krylov_rel = sd.opt_.krylov_rel; krylov_iter = sd.opt_.krylov_iter; timers = op.timers;
      last_flag = sd.last_cg_flag; not_conv = sd.cg_not_converged; indef = sd.cg_indefinite_iters; last_red = sd.last_cg_reduction; worst_red = sd.worst_capped_cg_reduction;
      graph = sd.cg_graph_; graph_x = sd.cg_graph_x_; graph_key = sd.cg_graph_key_;
      sd.cg_graph_ = nullptr; sd.cg_graph_x_ = nullptr; sd.cg_graph_key_ = -1;
      op.scal.download(scal, 32, s);
      free_bits = op.MixedFree();
      if (sd.mixed_) {
         std::vector<uint8_t> m = sd.ess_host_;
         const int nn = sd.part.NN;
         for (int d3 = 0; d3 < 3; d3++) if (sd.part.ctrl_node[1 + d3] >= 0) for (int k = 0; k < 3; k++) m[(size_t)sd.part.ctrl_node[1 + d3] + (size_t)nn * k] = 1;
         op.UpdateEssTDofs(m); op.SetMixedFree(0);
         mask_changed = true;
      }
   }
   void close() {
      if (closed) return;
      closed = true;
      hipStream_t s = op.stream();
      (void)hipStreamSynchronize(s);
      sd.drop_cg_graph();
      sd.cg_graph_ = graph; sd.cg_graph_x_ = graph_x; sd.cg_graph_key_ = graph_key;
      sd.opt_.krylov_rel = krylov_rel; sd.opt_.krylov_iter = krylov_iter; op.timers = timers;
      sd.last_cg_flag = last_flag; sd.cg_not_converged = not_conv; sd.cg_indefinite_iters = indef; sd.last_cg_reduction = last_red; sd.worst_capped_cg_reduction = worst_red;
      if (mask_changed) {
         op.UpdateEssTDofs(sd.ess_host_); op.SetMixedFree(free_bits);
         op.GetGradient();   // (the inverse diagonal follows the mask: back to the run's)
      }
      op.scal.upload(scal, 32, s);
   }
   ~TangentScope() { try { close(); } catch (...) {} }
};

void SystemDriver::CGSolveColumns(int nc, const double* B, double* X, int64_t ld, double rel_tol, int max_iter, int nch, int* iters, double* reduction, int* flag) {
   if (nc < 1 || nc > EXA_GRAD_COLS_MAX) throw std::runtime_error("CGSolveColumns: between 1 and 16 columns");
   if (comm.nranks > 1 || comm.forced() || oper_->deterministic() || oper_->precond == Precond::MULTIGRID)
      throw std::runtime_error("the batched tangent solve is built for one rank in non-deterministic mode with the identity or Jacobi preconditioner");
   NonlinearMechOperator& op = *oper_;
   hipStream_t s = op.stream();
   const int64_t nd = op.Height(), nn = part.NN;
   if (ld < nd) throw std::runtime_error("CGSolveColumns: column stride shorter than the vectors");
   DevBuf<double> R((size_t)nc * nd), Z((size_t)nc * nd), D((size_t)nc * nd), Sb((size_t)nc * SB);
   Sb.zero(s);
   const bool ident = op.precond == Precond::IDENTITY;
   std::vector<const double*> gates(nc);
   for (int m = 0; m < nc; m++) {
      double* S = Sb.p + (size_t)m * SB; gates[m] = S + 6;
      double* r = R.p + (size_t)m * nd; double* z = Z.p + (size_t)m * nd; double* d = D.p + (size_t)m * nd;
      EXA_HC(hipMemsetAsync(X + (size_t)m * ld, 0, sizeof(double) * nd, s));
      EXA_HC(hipMemcpyAsync(r, B + (size_t)m * ld, sizeof(double) * nd, hipMemcpyDeviceToDevice, s));
      vk_pointwise(nd, op.dinv.p, r, z, s);
      EXA_HC(hipMemcpyAsync(d, z, sizeof(double) * nd, hipMemcpyDeviceToDevice, s));
      vk_dot(nd, nn, op.weight.p, d, r, nullptr, op.partial.p, S + 8, s);
      vk_cg_init(S, rel_tol, opt_.krylov_abs, s);
   }
   // Z += K_uu D on the columns still running: one pass over the records per nch columns, then the periodic sum of every column (the control
   // slots are essential in every solve of the tangent, so the masked direction is its own expansion: no MixedExpand); the output mask rides
   // in the dot product that follows
   auto action = [&]() {
      if (!op.GradMultRawCols(nch, nc, D.p, nd, Z.p, nd, op.ess_mask.p, gates.data()))
         throw std::runtime_error("the batched tangent solve needs the p = 1 hexahedron L-vector record action with atomic scatter (exa_grad_apply_lvec_cols)");
      for (int m = 0; m < nc; m++) op.SumLVector(Z.p + (size_t)m * nd, gates[m], false);
   };
   for (int m = 0; m < nc; m++) vk_fill_if(nd, gates[m], 0.0, Z.p + (size_t)m * nd, s);
   action();
   for (int m = 0; m < nc; m++) { double* S = Sb.p + (size_t)m * SB; vk_mask_dot(nd, nn, op.weight.p, op.ess_mask.p, D.p + (size_t)m * nd, Z.p + (size_t)m * nd, S + 6, op.partial.p, S + 8, s, S); }
   auto iteration = [&]() {
      for (int m = 0; m < nc; m++) {
         double* S = Sb.p + (size_t)m * SB;
         double* r = R.p + (size_t)m * nd; double* z = Z.p + (size_t)m * nd; double* d = D.p + (size_t)m * nd;
         vk_cg_step1(nd, nn, S, op.weight.p, op.dinv.p, d, X + (size_t)m * ld, r, z, op.partial.p, ident, true, max_iter, s);
         vk_cg_step2z(nd, S, z, r, d, ident, s);
      }
      action();
      for (int m = 0; m < nc; m++) { double* S = Sb.p + (size_t)m * SB; vk_mask_dot(nd, nn, op.weight.p, op.ess_mask.p, D.p + (size_t)m * nd, Z.p + (size_t)m * nd, S + 6, op.partial.p, S + 8, s, S); }
   };
   std::vector<double> hS((size_t)nc * SB);
   int launched = 0; bool done = false;
   while (!done) {
      for (int k = 0; k < cg_check_every && launched < max_iter; k++, launched++) iteration();
      Sb.download(hS.data(), hS.size(), s);
      done = launched >= max_iter;
      bool all = true;
      for (int m = 0; m < nc; m++) all = all && hS[(size_t)m * SB + 6] != 0.0;
      done = done || all;
   }
   for (int m = 0; m < nc; m++) {
      const double* S = &hS[(size_t)m * SB];
      iters[m] = (S[6] == 1.0 && S[7] == 0.0) ? 0 : (int)S[7];
      reduction[m] = S[11] > 0.0 ? std::sqrt(std::fmax(S[2], 0.0) / S[11]) : 0.0;
      flag[m] = S[6] == 0.0 ? 2 : (int)S[6];
   }
}

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
   const bool can_batch = comm.nranks == 1 && !comm.forced() && !op.deterministic() && op.precond != Precond::MULTIGRID;
   if (batched == 1 && !can_batch) throw std::runtime_error("macro_tangent: the batched route is built for one rank in non-deterministic mode; use batched = 0 or the automatic route");
   const int auto_env = env_int("EXA_TANGENT_BATCHED", tangent_auto_batched ? 1 : 0);
   bool want = batched < 0 ? (can_batch && auto_env != 0) : batched == 1;
   const int nch = tangent_nch > 0 ? tangent_nch : env_int("EXA_TANGENT_NCH", 0);
   if (nch < 0 || nch > 3) throw std::runtime_error("macro_tangent: 1, 2 or 3 columns per pass");
   TangentScope scope(*this);
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
   if (want) CGSolveColumns(9, Bv.p, W.p, nd, rel, mi, nch, out.iters, out.reduction, out.flag);
   else {
      // one fixed solution buffer: the PCG chunk is captured once for it and replayed by all nine solves
      if (tangent_x_.n != (size_t)nd) tangent_x_.alloc((size_t)nd);
      opt_.krylov_rel = rel; opt_.krylov_iter = mi;
      for (int m = 0; m < 9; m++) {
         out.iters[m] = CGSolve(Bv.p + (size_t)m * nd, tangent_x_.p);
         out.reduction[m] = last_cg_reduction; out.flag[m] = last_cg_flag;
         EXA_HC(hipMemcpyAsync(W.p + (size_t)m * nd, tangent_x_.p, sizeof(double) * nd, hipMemcpyDeviceToDevice, s));
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
   if (batched && (comm.nranks > 1 || comm.forced())) throw std::runtime_error("grad_apply_columns: the batched route is built for one rank");
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
