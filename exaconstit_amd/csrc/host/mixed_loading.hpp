// Mixed stress / velocity-gradient loading of a periodic cell: what SystemDriver keeps of it between steps and the 3 x 3 algebra of
// MixedStepStart / MixedStepEnd.  Pure functions of host numbers (no HIP include): the driver reads the corner values from the PeriodicCell
// (host/periodic.hpp), calls these and launches; tests/mixed_loading_check.cpp runs them without a GPU and under the sanitizers.
// Matrices are 3 x 3, row by row.  A: column d = period vector a_d; H: column d = h_d = v(c_d) - v(c_0); L = H A^-1.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

namespace exa_host {

inline void inv3(const double* A, double* B) {
   const double c0 = A[4] * A[8] - A[5] * A[7], c1 = A[5] * A[6] - A[3] * A[8], c2 = A[3] * A[7] - A[4] * A[6];
   const double det = A[0] * c0 + A[1] * c1 + A[2] * c2;
   B[0] = c0 / det; B[1] = (A[2] * A[7] - A[1] * A[8]) / det; B[2] = (A[1] * A[5] - A[2] * A[4]) / det;
   B[3] = c1 / det; B[4] = (A[0] * A[8] - A[2] * A[6]) / det; B[5] = (A[2] * A[3] - A[0] * A[5]) / det;
   B[6] = c2 / det; B[7] = (A[1] * A[6] - A[0] * A[7]) / det; B[8] = (A[0] * A[4] - A[1] * A[3]) / det;
}
inline void mul3(const double* A, const double* B, double* C) {
   for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
// A (column d = a_d) and H (column d = h_d) from the values of a field at c_0 .. c_3
inline void corner_differences(const double* c12, double* M) { for (int d = 0; d < 3; d++) for (int i = 0; i < 3; i++) M[3 * i + d] = c12[3 * (d + 1) + i] - c12[i]; }

// free mask of any integer type (row by row; null: nothing free) as 0 / 1 bytes; returns MixedTable::free_bits (bit 3 i + d = entry (i, d) is free)
template <class T>
inline uint32_t free_mask_bits(const T* f9, uint8_t* out9) {
   uint32_t bits = 0;
   for (int k = 0; k < 9; k++) { out9[k] = f9 && f9[k] ? 1 : 0; if (out9[k]) bits |= 1u << k; }
   return bits;
}

// The run-time check of the free mask against the cell: a prescribed L_id is a condition on H_id alone only when a_d has no component along a
// direction j whose L_ij is free.  Returns the refusal, or nothing when the mask is well posed on A.
inline std::string mixed_free_refusal(const uint8_t* free9, const double* A) {
   for (int d = 0; d < 3; d++) {
      const double len = std::sqrt(A[d] * A[d] + A[3 + d] * A[3 + d] + A[6 + d] * A[6 + d]);
      for (int i = 0; i < 3; i++) if (!free9[3 * i + d]) for (int j = 0; j < 3; j++) if (free9[3 * i + j] && std::fabs(A[3 * j + d]) > 1e-12 * len) {
         char m[320];
         std::snprintf(m, sizeof(m), "periodic_free: entry (%d,%d) of the velocity gradient is free and entry (%d,%d) is prescribed, but period vector %d has the component %.3e "
                       "along direction %d - the prescribed entry is no condition on one corner difference alone (DESIGN 4.12)", i + 1, j + 1, i + 1, d + 1, d + 1, A[3 * j + d], j + 1);
         return m;
      }
   }
   return std::string();
}
// the corner differences a step starts from: the prescribed H_id = (L a_d)_i (first step: all of them), the free ones as the last step left them
inline void mixed_choose_H(const uint8_t* free9, bool first, const double* L, const double* A, const double* H_prev, double* H) {
   double LA[9];
   mul3(L, A, LA);
   for (int k = 0; k < 9; k++) H[k] = (!free9[k] || first) ? LA[k] : H_prev[k];
}
// L = H A^-1: the gradient UpdateVelocity imposes (H of the start of a step) or the one a step realised (H of its converged field)
inline void mixed_gradient(const double* H, const double* A, double* L) { double Ai[9]; inv3(A, Ai); mul3(H, Ai, L); }
// a changed boundary condition: what the affine part of the velocity gains, (H - H_prev) A^-1, as L_eff - H_prev A^-1
inline void mixed_bc_dL(const double* L_eff, const double* H_prev, const double* A, double* dL) {
   double Lold[9];
   mixed_gradient(H_prev, A, Lold);
   for (int k = 0; k < 9; k++) dL[k] = L_eff[k] - Lold[k];
}
// The step pinned c_0 at L_eff w0 (w0 = x(c_0) - origin).  The rigid translation that moves the pin to the realised gradient; exactly zero when
// the two gradients are equal.
inline void mixed_pin_translation(const double* L_real, const double* L_eff, const double* w0, double* t) {
   for (int i = 0; i < 3; i++) { t[i] = 0.0; for (int j = 0; j < 3; j++) t[i] += (L_real[3 * i + j] - L_eff[3 * i + j]) * w0[j]; }
}

// what the driver keeps of mixed loading between its calls
struct MixedLoading {
   bool on = false;           // some entry of L is free
   bool solved = false;       // L and F are those of a solved step
   bool bc_changed = false;   // the options' L has changed: the next MixedStepStart swaps the affine part of the prescribed entries
   uint8_t free[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
   double L_eff[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };   // gradient the step in progress imposes
   double A[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };       // A of the start of the last step
   double L[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };       // realised gradient of the last solved step
   double F[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };       // face resultants F_id of its last residual
   double w0[3] = { 0, 0, 0 };                        // c_0 relative to the origin of the velocity-gradient conditions
   // takes the mask, with L0 (null: zero) the gradient in force until the first step starts; returns the bits for the cell
   uint32_t set_free(const uint8_t* f9, const double* L0) {
      const uint32_t bits = free_mask_bits(f9, free);
      on = bits != 0;
      for (int k = 0; k < 9; k++) L_eff[k] = L0 ? L0[k] : 0.0;
      return bits;
   }
};

}  // namespace exa_host
