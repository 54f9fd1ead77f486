// The device record of one GMRES solve (host/krylov.hip, gmres_kernels.hip), beside the PCG one (pcg_slots.hpp): a head of scalars that
// the host reads back when it polls, then the reduction results, the coefficients of the next multi-axpy, the rotations, the right-hand side s of
// the least-squares problem and the Hessenberg matrix.  FLAG takes the values of pcg::RUNNING / CONVERGED / MAX_ITER / BREAKDOWN and is the gate
// of every kernel of an iteration, the operator's included.
#pragma once

namespace gmres {

constexpr int MAXK = 100;          // largest Krylov dimension (Solvers.Krylov.gmres_kdim)
constexpr int LDH = MAXK + 1;      // leading dimension of H (column-major: column i holds h_0i ... h_i+1,i)
constexpr int PAD = 104;           // an array of up to MAXK + 2 entries

enum Slot : int {
   FLAG = 0,            // RUNNING until the scalar kernel decides
   ITERS = 1,           // Arnoldi steps done
   RESID = 2,           // |s_i+1| of the last column (after a restart: beta)
   FINAL = 3,           // max(rel_tol beta0, abs_tol)
   BETA0 = 4,           // |M^-1 b|
   BETA = 5,            // |M^-1 (b - K x)| at the start of the cycle
   REORTH = 6,          // 1 between the decision for a second Gram-Schmidt pass and its end
   RESTARTS = 7,
   REORTH_PASSES = 8,   // second passes taken
   WN2_BEFORE = 9,      // |w|^2 before the first pass (one more column of the first multi-dot)
   HNEXT = 10,          // h_i+1,i = |w| after orthogonalisation
   SCALE = 11,          // 1 / HNEXT (1 / beta at the start of a cycle): what the normalisation multiplies by
   NCOL = 12,           // columns of the cycle that are complete: what the back-substitution solves for
};
constexpr int HEAD = 16;           // slots a poll fetches
constexpr int RED = HEAD;          // sums of the partial-sum table, in place for the all-reduce (up to MAXK + 2)
constexpr int COEF = RED + PAD;    // coefficients of the multi-axpy of the orthogonalisation
constexpr int Y = COEF + PAD;      // solution of the triangular system
constexpr int CS = Y + PAD;
constexpr int SN = CS + PAD;
constexpr int SVEC = SN + PAD;     // MAXK + 1 entries
constexpr int H = SVEC + PAD;
constexpr int LEN = H + LDH * MAXK;

}  // namespace gmres
