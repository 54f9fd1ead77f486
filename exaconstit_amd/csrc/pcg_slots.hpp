// The device scalar record of one PCG solve: which double lives where.  The vector kernels (vec_kernels.hip) keep every scalar of the recurrence
// in it, the operator kernels take its FLAG slot as their gate, and the host reads it back every few iterations (host/krylov.hip).
#pragma once

namespace pcg {

enum Slot : int {
   NOM = 0,          // (r, z) of the iterate the direction was built from
   DEN = 1,          // (A d, d)
   BETANOM = 2,      // latest (r, z): the achieved reduction is reported from it
   THRESHOLD = 3,    // max(rel^2 (r0, z0), abs^2)
   ALPHA = 4,
   BETA = 5,
   FLAG = 6,         // RUNNING until a kernel decides; every kernel of an iteration, the operator's included, is a no-op once it is set
   ITERS = 7,
   RED0 = 8,         // where a reduction (and the all-reduce behind it) leaves its sum ...
   RED1 = 9,         // ... and the second of a pair (single-reduction loop: gamma, delta)
   INDEFINITE = 10,  // iterations that saw (A d, d) < 0
   R0Z0 = 11,        // (r0, z0)
   // consumer-side reductions: what all blocks of a kernel read is never written by that kernel, so the direction kernel leaves the next
   // (NOM, ITERS) here and the update kernel commits them.  Between the two, ITERS is one behind ITERS_NEXT.
   NOM_NEXT = 16,
   ITERS_NEXT = 17,
};
constexpr int USED = 18;      // slots a read-back has to fetch
constexpr int LEN = 24;       // doubles per record (the lockstep solve keeps one record per column at this stride)
constexpr int CLEARED = 11;   // slots [0, CLEARED) are zeroed before a solve; the init kernels set what they need beyond
static_assert(CLEARED == INDEFINITE + 1 && USED == ITERS_NEXT + 1 && USED <= LEN, "record layout");

// values of FLAG (MFEM's CGSolver: converged, no convergence within max_iter, (A d, d) = 0 or a negative (r0, z0))
constexpr double RUNNING = 0.0, CONVERGED = 1.0, MAX_ITER = 2.0, BREAKDOWN = -1.0;

}  // namespace pcg
