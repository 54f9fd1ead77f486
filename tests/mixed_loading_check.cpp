// Stand-alone check of the step algebra of mixed loading (exaconstit_amd/csrc/host/mixed_loading.hpp): the 3 x 3 helpers, the run-time
// check of the free mask against the period vectors, the choice of H, L = H A^-1, the dL of a changed boundary condition and the pin translation.
// No GPU, no Python.  scripts/mixed_loading_sanitize.sh builds it with -fsanitize=address,undefined and runs it.
#include "../exaconstit_amd/csrc/host/mixed_loading.hpp"
#include <cstring>

using namespace exa_host;

static int nbad = 0;
static void expect(bool ok, const char* what) { if (!ok) { nbad++; std::printf("mixed_loading_check: wrong: %s\n", what); } }
static double maxdiff(const double* a, const double* b, int n = 9) { double m = 0.0; for (int k = 0; k < n; k++) m = std::fmax(m, std::fabs(a[k] - b[k])); return m; }

int main() {
   const double I[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };
   // a sheared, non-symmetric cell: a_1 = (1.1, 0.05, -0.02), a_2 = (0.3, 0.9, 0.01), a_3 = (-0.2, 0.4, 1.3) in the columns
   const double A[9] = { 1.1, 0.3, -0.2, 0.05, 0.9, 0.4, -0.02, 0.01, 1.3 };
   double Ai[9], P[9];
   inv3(A, Ai);
   mul3(A, Ai, P); expect(maxdiff(P, I) < 4e-16, "A A^-1 = 1");
   mul3(Ai, A, P); expect(maxdiff(P, I) < 4e-16, "A^-1 A = 1");
   {  // mul3 is row by row: (A B)_01 by hand
      const double B[9] = { 1, 2, 3, 4, 5, 6, 7, 8, 10 };
      mul3(A, B, P);
      expect(P[1] == A[0] * B[1] + A[1] * B[4] + A[2] * B[7] && P[6] == A[6] * B[0] + A[7] * B[3] + A[8] * B[6], "mul3 entries");
   }
   // corner differences of the affine field f(x) = f0 + G x at c_0 = o, c_d = o + a_d: column d of the result is G a_d
   const double G[9] = { 0.5, -1.0, 2.0, 0.25, 3.0, -0.5, 1.5, 0.125, -2.0 }, f0[3] = { 7.0, -3.0, 0.5 }, o[3] = { 0.25, -0.5, 2.0 };
   double c12[12], M[9], GA[9];
   for (int k = 0; k < 4; k++) for (int i = 0; i < 3; i++) {
      double x[3]; for (int j = 0; j < 3; j++) x[j] = o[j] + (k ? A[3 * j + (k - 1)] : 0.0);
      c12[3 * k + i] = f0[i] + G[3 * i] * x[0] + G[3 * i + 1] * x[1] + G[3 * i + 2] * x[2];
   }
   corner_differences(c12, M); mul3(G, A, GA);
   expect(maxdiff(M, GA) < 1e-14, "corner differences of an affine field");
   {  // ... and of the coordinates themselves: A
      double cx[12]; for (int k = 0; k < 4; k++) for (int i = 0; i < 3; i++) cx[3 * k + i] = o[i] + (k ? A[3 * i + (k - 1)] : 0.0);
      corner_differences(cx, M); expect(maxdiff(M, A) < 1e-15, "corner differences of the coordinates");
   }
   // the free mask: any integer type, null, bits
   uint8_t f[9]; const int fi[9] = { 1, 0, 0, 0, -7, 0, 0, 0, 0 }; const uint8_t none[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
   expect(free_mask_bits(fi, f) == ((1u << 0) | (1u << 4)) && f[0] == 1 && f[4] == 1 && f[1] == 0 && f[8] == 0, "free bits of ints");
   expect(free_mask_bits((const int*)nullptr, f) == 0 && std::memcmp(f, none, 9) == 0, "null mask");
   const uint8_t all[9] = { 1, 2, 3, 4, 5, 6, 7, 8, 255 };
   expect(free_mask_bits(all, f) == 0x1ffu && f[8] == 1, "all free");
   // the check: uniaxial mask (xx and yy free) on an axis-aligned cell, then a_2 leaning along x by more / less than 1e-12 |a_2|
   const uint8_t uni[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 0 };
   double B[9] = { 1.5, 0, 0, 0, 2.0, 0, 0, 0, 0.75 };
   expect(mixed_free_refusal(uni, B).empty(), "uniaxial mask on an axis-aligned cell");
   expect(mixed_free_refusal(none, A).empty(), "nothing free on a sheared cell");
   B[1] = 2.0 * 0.5e-12; expect(mixed_free_refusal(uni, B).empty(), "a_2 leaning by 0.5e-12 |a_2| passes");
   B[1] = -2.0 * 0.5e-12; expect(mixed_free_refusal(uni, B).empty(), "a_2 leaning by -0.5e-12 |a_2| passes");
   B[1] = 2.0 * 2e-12;
   const std::string why = mixed_free_refusal(uni, B);
   expect(why == "periodic_free: entry (1,1) of the velocity gradient is free and entry (1,2) is prescribed, but period vector 2 has the component 4.000e-12 "
                 "along direction 1 - the prescribed entry is no condition on one corner difference alone (DESIGN 4.12)", "the refusal and its text");
   B[1] = 0.0; B[5] = 0.1; expect(mixed_free_refusal(uni, B).find("entry (2,2) of the velocity gradient is free and entry (2,3) is prescribed, but period vector 3") != std::string::npos, "a_3 leaning along y");
   B[5] = 0.0; B[6] = 0.3; expect(mixed_free_refusal(uni, B).empty(), "a_1 leaning along z: no free entry in row 3");
   // the choice of H: the first step takes L A everywhere, later steps keep the free entries of the last step
   const double L[9] = { 1e-3, 2e-4, 0, -1e-4, 5e-4, 3e-4, 0, 1e-4, -2e-3 };
   double H[9], LA[9], Hp[9], Lb[9];
   mul3(L, A, LA);
   for (int k = 0; k < 9; k++) Hp[k] = 10.0 + k;
   mixed_choose_H(uni, true, L, A, Hp, H); expect(maxdiff(H, LA) == 0.0, "first step: H = L A");
   mixed_choose_H(uni, false, L, A, Hp, H);
   for (int k = 0; k < 9; k++) expect(H[k] == (uni[k] ? Hp[k] : LA[k]), "later steps: free entries from the last step");
   // nothing free: H A^-1 gives the prescribed L back
   mixed_choose_H(none, false, L, A, Hp, H); mixed_gradient(H, A, Lb);
   expect(maxdiff(Lb, L) < 1e-18 + 4e-16 * 2e-3, "H A^-1 reproduces the prescribed L");
   {  // a changed boundary condition: dL = (H - H_prev) A^-1
      double dL[9], D[9], want[9];
      mixed_bc_dL(Lb, Hp, A, dL);
      for (int k = 0; k < 9; k++) D[k] = H[k] - Hp[k];
      mul3(D, Ai, want);
      expect(maxdiff(dL, want) < 1e-13, "dL of a changed boundary condition");
      mixed_bc_dL(Lb, H, A, dL); for (int k = 0; k < 9; k++) expect(dL[k] == 0.0, "no change: dL exactly zero");
   }
   // the pin translation: exactly zero for equal gradients, (L - L_eff) w0 otherwise
   const double w0[3] = { 0.3, -1.7, 2.9 };
   double t[3];
   mixed_pin_translation(Lb, Lb, w0, t); expect(t[0] == 0.0 && t[1] == 0.0 && t[2] == 0.0, "equal gradients: no translation");
   mixed_pin_translation(L, I, w0, t);
   expect(std::fabs(t[0] - ((L[0] - 1) * w0[0] + L[1] * w0[1] + L[2] * w0[2])) < 1e-15 && std::fabs(t[2] - (L[6] * w0[0] + L[7] * w0[1] + (L[8] - 1) * w0[2])) < 1e-15, "pin translation");
   // the struct: the mask, the flag and the gradient in force before the first step
   MixedLoading m;
   expect(!m.on && !m.solved && !m.bc_changed && maxdiff(m.A, I) == 0.0, "defaults");
   expect(m.set_free(uni, L) == 0x11u && m.on && maxdiff(m.L_eff, L) == 0.0 && std::memcmp(m.free, uni, 9) == 0, "set_free");
   expect(m.set_free(none, nullptr) == 0 && !m.on && m.L_eff[0] == 0.0 && m.L_eff[8] == 0.0, "set_free with nothing free");
   std::printf("mixed_loading_check: %d wrong values\n", nbad);
   return nbad == 0 ? 0 : 1;
}
