// The small dense algebra of GMRES (MFEM linalg/solvers.cpp: GeneratePlaneRotation, ApplyPlaneRotation, Update), host and device: the scalar
// kernel of gmres_kernels.hip and the host probe exa_gmres_column_probe run this very code.  Nothing here divides by zero.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define EXA_GMRES_HD __host__ __device__
#else
#define EXA_GMRES_HD
#endif

namespace gmres {

// values of the solver's flag, the same numbers as pcg::RUNNING / CONVERGED / MAX_ITER / BREAKDOWN
constexpr double F_RUNNING = 0.0, F_CONVERGED = 1.0, F_MAX_ITER = 2.0, F_BREAKDOWN = -1.0;

// the overflow-safe form: the quotient taken is the one of magnitude <= 1.  A column that is zero from the diagonal down (dx = dy = 0) gets the
// swap instead of MFEM's identity: the residual |s_i+1| then stays what it was, as the least-squares problem says, instead of dropping to 0.
EXA_GMRES_HD inline void generate_rotation(double dx, double dy, double& cs, double& sn) {
   if (dy == 0.0) { cs = dx == 0.0 ? 0.0 : 1.0; sn = dx == 0.0 ? 1.0 : 0.0; }
   else if (std::fabs(dy) > std::fabs(dx)) { const double t = dx / dy; sn = 1.0 / std::sqrt(1.0 + t * t); cs = t * sn; }
   else { const double t = dy / dx; cs = 1.0 / std::sqrt(1.0 + t * t); sn = t * cs; }
}

EXA_GMRES_HD inline void apply_rotation(double& dx, double& dy, double cs, double sn) {
   const double t = cs * dx + sn * dy;
   dy = -sn * dx + cs * dy; dx = t;
}

// column i of H as Gram-Schmidt left it - h[0 .. i] and h[i + 1] = |w| - under the rotations 0 .. i - 1, then the new rotation on the column and on
// s (s[i + 1] is 0 on entry).  Returns |s[i + 1]|: the residual norm of the least-squares problem with i + 1 columns.
EXA_GMRES_HD inline double column_update(int i, double* h, double* cs, double* sn, double* s) {
   for (int k = 0; k < i; k++) apply_rotation(h[k], h[k + 1], cs[k], sn[k]);
   generate_rotation(h[i], h[i + 1], cs[i], sn[i]);
   apply_rotation(h[i], h[i + 1], cs[i], sn[i]);
   apply_rotation(s[i], s[i + 1], cs[i], sn[i]);
   return std::fabs(s[i + 1]);
}

// what a finished column decides.  hnext = h_i+1,i before the rotations: at 0 the Krylov space is exhausted, which is convergence when the residual
// says so and a breakdown otherwise.
EXA_GMRES_HD inline double step_flag(double resid, double final_norm, double hnext, double iters, double max_iter) {
   if (!std::isfinite(resid) || !std::isfinite(hnext)) return F_BREAKDOWN;
   if (resid <= final_norm) return F_CONVERGED;
   if (hnext == 0.0) return F_BREAKDOWN;
   if (iters >= max_iter) return F_MAX_ITER;
   return F_RUNNING;
}

// R y = s for the k leading columns of the rotated H (upper triangular, leading dimension ldh).  A zero pivot gives y_i = 0; a non-finite entry
// gives y = 0.  false when either happened.
EXA_GMRES_HD inline bool back_substitute(int k, const double* H, int ldh, const double* s, double* y) {
   bool ok = true;
   for (int i = k - 1; i >= 0; i--) {
      double t = s[i];
      for (int j = i + 1; j < k; j++) t -= H[i + j * ldh] * y[j];
      const double p = H[i + i * ldh];
      if (p == 0.0) { y[i] = 0.0; ok = false; } else y[i] = t / p;
   }
   bool finite = true;
   for (int i = 0; i < k; i++) finite = finite && std::isfinite(y[i]);
   if (!finite) { for (int i = 0; i < k; i++) y[i] = 0.0; ok = false; }
   return ok;
}

}  // namespace gmres
