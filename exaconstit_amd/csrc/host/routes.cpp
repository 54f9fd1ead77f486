// The operator's switches, its route decision and the cost model of the tail split (see routes.hpp).  Host code only.
#include "routes.hpp"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace exa_host {

// the one string test: the variable is set and spells exactly v
static bool env_is(const char* k, const char* v) { const char* e = std::getenv(k); return e && std::strcmp(e, v) == 0; }

RouteSwitches RouteSwitches::from_env() {
   RouteSwitches s;
   s.tet_action_generic = env_is("EXA_TET_ACTION", "generic");
   s.deterministic = env_is("EXA_DETERMINISTIC", "1");
   if (const char* nc = std::getenv("EXA_NEWTON_CAP")) {
      if (std::strcmp(nc, "auto") == 0) s.newton_cap_mode = Cap::AUTO;
      else {   // "off", "<K>" or "<K>,<K2>" (second level)
         s.newton_cap_mode = Cap::FIXED; s.newton_cap = std::strcmp(nc, "off") == 0 ? 0 : std::atoi(nc);
         if (const char* c2 = std::strchr(nc, ',')) s.newton_cap2 = std::atoi(c2 + 1);
      }
   }
   s.tail_resume_off = env_is("EXA_TAIL_RESUME", "off");
   s.ea_assembled = env_is("EXA_EA_ASSEMBLED", "1");
   s.tet_apply_geo_off = env_is("EXA_TET_APPLY_GEO", "off");
   s.tangent_form_full = env_is("EXA_TANGENT_FORM", "full");
   s.apply_geo_off = env_is("EXA_APPLY_GEO", "off");
   s.p2_prepass_off = env_is("EXA_P2_PREPASS", "off");
   s.tangent_records_off = env_is("EXA_TANGENT_RECORDS", "off");
   s.qlayout_aos = env_is("EXA_QLAYOUT", "aos");
   s.jac_field_on = env_is("EXA_JAC_FIELD", "on");
   s.lean_state_off = env_is("EXA_LEAN_STATE", "off");
   if (const char* ho = std::getenv("EXA_HALO_OVERLAP")) s.halo_overlap = (std::strcmp(ho, "off") == 0 || std::strcmp(ho, "0") == 0) ? Overlap::OFF : Overlap::ON;
   s.nfev_log = std::getenv("EXA_NFEV_LOG") != nullptr;         // measurement aid: evaluation-count histogram of every launch on stderr (synchronises)
   s.model_times = std::getenv("EXA_MODEL_TIMES") != nullptr;   // per-launch durations on stderr (measurement aid)
   return s;
}

OperatorRoutes decide_routes(const RouteFacts& f, const RouteSwitches& sw) {
   OperatorRoutes r;
   const bool tet = f.geom == 1;   // tetrahedra: table-driven kernels + the fused action of tet_kernels.hip, never a hexahedron fast path
   const bool pa = !f.ea, kmdd = f.slip == RouteFacts::KMDD;
   r.fast_p1 = f.order == 1 && !f.bbar && !tet;          // fused L-vector kernels exist for p = 1 full integration
   const bool hex_p2 = f.order == 2 && !tet;
   // EXA_TET_ACTION=generic: tetrahedra keep the table-driven PA (E-vector) / EA action (A/B switch)
   const bool tet_wants_fused = tet && !sw.tet_action_generic;
   // EXA_DETERMINISTIC=1: ordered E->L sums and halo additions instead of FP64 atomics: bit-reproducible residuals, CG iterates and results.
   // The fused kernels are ordered for p = 1 full integration; the other contexts take the E-vector entries + the ordered E->L sum.
   r.det = sw.deterministic;
   r.det_unfused = r.det && !r.fast_p1;
   r.lvec_grad = !r.det_unfused && (r.fast_p1 || f.ea || hex_p2 || tet_wants_fused);   // p = 2: matrix-free action from the point records (PA and EA)
   // tail split of the constitutive launch (include/exaconstit_hip.h): EXA_NEWTON_CAP=off | <K> | unset (chosen from the evaluation-count histogram of the previous launch)
   // The controller runs for the Kocks-Mecking family only: for the Voce kernels the model never finds a paying cap in steady state and
   // a stale histogram costs 20 % in the elastic-plastic transition passes (measured).  EXA_NEWTON_CAP=auto forces it on.
   r.cap_auto = sw.newton_cap_mode == RouteSwitches::Cap::UNSET ? kmdd : sw.newton_cap_mode == RouteSwitches::Cap::AUTO;
   r.tail_resume = !sw.tail_resume_off;   // A/B switch: the dense launch starts its points over (round 2) instead of resuming them
   r.newton_cap = sw.newton_cap;
   r.newton_cap2 = r.tail_resume ? sw.newton_cap2 : 0;
   r.tail_cost = kmdd ? 1.5 : 4.0;   // (Kocks-Mecking: re-measured on the final round-3 kernels - resumed tail points, rejecting points handed over: w = 1.2 ... 2 picks cap 6 for FCC, 16.6 instead of 16.9 ms at cap 5 (w <= 1); BCC 4 either way)
   // element assembly: the element matrices are 2x (p = 1) to 5x (p = 2) the bytes of the records they are built from, so the action is
   // computed from the records and the matrices only exist if somebody asks for them (diagonal, export); EXA_EA_ASSEMBLED=1 streams them instead
   r.ea_matrix_free = !r.det_unfused && f.ea && (hex_p2 || r.fast_p1 || tet_wants_fused) && !sw.ea_assembled;
   // tetrahedra: the fused kernel runs for PA and for matrix-free EA, in atomic mode; assembled EA matrices (EXA_EA_ASSEMBLED=1) take the
   // table-driven L-vector kernel, and the records of the fused action are then not built per Newton iteration
   r.tet_fused = tet_wants_fused && !(r.det_unfused || (f.ea && !r.ea_matrix_free));
   // p = 1 fused action: J^-1 recomputed from the current coordinates (EXA_TET_APPLY_GEO=off: read from the element record)
   r.tet_geo = r.tet_fused && f.order == 1 && !sw.tet_apply_geo_off;
   // compact tangent records wherever a record-based action runs: p = 1 PA / matrix-free EA with the geometry recomputed, p = 2 matrix-free
   const bool ea_streamed = f.ea && sw.ea_assembled;
   r.compact_tangent = !r.det_unfused && !sw.tangent_form_full && !ea_streamed && ((r.fast_p1 && !sw.apply_geo_off) || hex_p2);
   // Gradient records straight from the constitutive launch (p = 1, compact form, identity "Jacobi" of the reference): no tangent field, no
   // defect check, no AssembleGradPA pass per Newton iteration.  EXA_TANGENT_RECORDS=off keeps the tangent field + exa_grad_setup (A/B switch);
   // true Jacobi needs the 46-double records for the diagonal and takes that route as well (SetPrecond).
   // p = 2 (round 6): the same behind the geometry pre-pass - the launch writes the 18-pair records of the matrix-free action (plain or B-bar, PA or EA)
   const bool p2_records = hex_p2 && !r.det && (pa || !sw.ea_assembled) && !sw.p2_prepass_off;
   // (p = 1: on either layout - the reference layout through the staged launch; p = 2: element-blocked only)
   r.records_setup = (r.fast_p1 || p2_records) && r.compact_tangent && !r.det && !sw.tangent_records_off && (r.fast_p1 || !sw.qlayout_aos);
   r.lvec_resid = r.fast_p1 || (hex_p2 && !r.det);      // fused L-vector residual kernels (p = 1 full integration; p = 2 plain and B-bar)
   // record route + L-vector residual: no Jacobian field is written, both actions recompute the geometry; EXA_JAC_FIELD=on is the A/B switch: the
   // record route writes and reads the Jacobian field as before (p = 2: the field is written by the geometry pre-pass and read by the residual)
   r.geo_resid = !sw.jac_field_on && r.lvec_resid && r.fast_p1;
   // slip rates on demand (EnsureSlipRates): the element-blocked record launches write 56 B per point less (Kocks-Mecking: 48); EXA_LEAN_STATE=off is the A/B switch
   r.lean_state = !sw.lean_state_off;
   // internal quadrature-function layout: element-blocked on the fused p = 1 and p = 2 paths (EXA_QLAYOUT=aos switches back for A/B runs)
   r.qlayout_eb64 = r.lvec_resid && !sw.qlayout_aos;
   // geometry of the tangent-field action recomputed from x_cur (unchanged until the next residual evaluation); EXA_APPLY_GEO=off streams it instead
   r.grad_set_coords = (r.fast_p1 && !sw.apply_geo_off) || r.tet_geo;
   // Halo exchange overlapped with the interior blocks: several ranks, the atomic p = 1 record-based action (PA, and EA computed from the
   // records).  The deterministic mode keeps the plain sequence (its ordered E->L gather runs over all elements at once); EXA_HALO_OVERLAP=off
   // is the A/B switch.  E_bdr > 0 only after Partition::order_boundary_first (SystemDriver).
   // Over RCCL the overlapped form is OPT-IN (EXA_HALO_OVERLAP=on).  Round 6 ran it on the hardware a one-GPU box has - the forced one-rank communicator
   // exchanging a face of the real size with itself (EXA_HALO_SELFTEST, tests/test_gpu_rccl.py): the grouped send/recv on the second stream between the
   // all-reduces of the main stream works, but at 64^3 per rank it costs 162 us per PCG iteration against 141 us in line (profiles/r06_rccl_self_exchange.txt):
   // two launches of the action and two cross-stream waits to hide a 24 us exchange.  A box with real xGMI neighbours has to show where the balance tips.
   const bool want = sw.halo_overlap == RouteSwitches::Overlap::UNSET ? !f.rccl : sw.halo_overlap == RouteSwitches::Overlap::ON;
   const bool ea_rec = f.ea && !sw.ea_assembled;
   // (periodic partitions keep the plain sequence: the elements at the box surface touch shared dofs too, and the boundary-first order does not know them)
   r.overlap_wish = r.fast_p1 && r.lvec_grad && !r.det && f.has_bdr_blocks && f.has_nbrs && (pa || ea_rec) && want && !f.periodic;
   r.action_route = !tet ? 0 : (r.lvec_grad && r.tet_fused ? 1 : (r.lvec_grad ? 3 : 2));
   r.nfev_log = sw.nfev_log; r.model_times = sw.model_times;
   return r;
}

void OperatorRoutes::to_ints(int* o) const {
   const int v[QUERY_FIELDS] = { fast_p1, lvec_grad, lvec_resid, compact_tangent, records_setup, geo_resid, tet_fused, tet_geo, overlap_wish, cap_auto, qlayout_eb64,
                                 lean_state, ea_matrix_free, det, det_unfused, grad_set_coords, newton_cap, newton_cap2, tail_resume, (int)std::lround(10.0 * tail_cost),
                                 action_route, nfev_log, model_times };
   std::copy(v, v + QUERY_FIELDS, o);
}

// Cost model of the tail split in units of one residual evaluation per point.  A wave costs the largest evaluation count among its 64
// lanes: E[max of 64 draws].  With cap K the first launch draws from min(n, K) and the dense second launch from {n > K} (plus ~2
// evaluations' worth of set-up / tangent / I/O per redone point):  C(K) = Emax64(min(n,K)) + 0.2 + f_tail w (Emax64(n | n > K) + 2).
// w = measured cost of a point in the second launch relative to the first (its lanes are scattered points: 8-byte accesses into the
// blocked rows): 4 for the Voce kernels, whose first launch is close to the memory system's limits, 1.5 for the compute-heavy
// Kocks-Mecking kernel; 0.2 = the second launch's fixed cost.  Measured at 128^3: BCC KM-DD 31.6 -> 16.0 ms, FCC KM-DD 70.9 -> 55.9 ms,
// Voce stays uncapped (6.9 ms; K = 5 would cost 10.2 ms, which the model reproduces).  Round 3: w = 1.0 at mid-round, 1.5 again on the final kernels.
// Returns the K minimising C, or 0 (off) when it does not beat the uncapped launch by 3 %.
// With resumed tail points (exa_set_newton_caps) a listed point does not repeat its K evaluations: the dense launch pays the point set-up again
// (~0.7 evaluations), one evaluation that restores (r, J), and the evaluations beyond K.  A second cap K2 splits the dense launch once more:
//   C(K, K2) = Emax64(min(n,K)) + 0.2 + f1 w (Emax64(min(n,K2) | n > K) - K + 1.7) + [0.2 + f2 w (Emax64(n | n > K2) - K2 + 1.7)]
// The pair (K, K2) minimising C is returned (K2 = 0: one dense launch), or (0, 0) when it does not beat the uncapped launch by 3 %.
void choose_newton_caps_resume(const int* hist, double w, int& k1, int& k2) {
   k1 = k2 = 0;
   double tot = 0; for (int i = 0; i < 64; i++) tot += hist[i];
   if (tot <= 0) return;
   // E[max of 64 draws] of min(n, hi) over the population n > lo
   auto emax = [&](int lo, int hi) {
      double n = 0; for (int m = lo + 1; m < 64; m++) n += hist[m];
      if (n <= 0) return 0.0;
      double F = 0, prev = 0, e = 0;
      for (int m = lo + 1; m <= hi; m++) {
         double pm = hist[m]; if (m == hi) for (int j = hi + 1; j < 64; j++) pm += hist[j];
         F += pm / n; const double f64 = std::pow(std::min(F, 1.0), 64.0); e += m * (f64 - prev); prev = f64;
      }
      return e;
   };
   auto above = [&](int k) { double n = 0; for (int m = k + 1; m < 64; m++) n += hist[m]; return n / tot; };
   const double c_inf = emax(-1, 63);
   double best = c_inf;
   for (int K = 3; K < 40; K++) {
      const double f1 = above(K);
      if (f1 == 0) break;
      const double first = emax(-1, K) + 0.2;
      {  const double c = first + f1 * w * (emax(K, 63) - K + 1.7);
         if (c < best) { best = c; k1 = K; k2 = 0; } }
      for (int K2 = K + 2; K2 < 48; K2++) {
         const double f2 = above(K2);
         if (f2 == 0) break;
         const double c = first + f1 * w * (emax(K, K2) - K + 1.7) + 0.2 + f2 * w * (emax(K2, 63) - K2 + 1.7);
         if (c < best) { best = c; k1 = K; k2 = K2; }
      }
   }
   if (!(best < 0.97 * c_inf)) k1 = k2 = 0;
}

int choose_newton_cap(const int* hist, double tail_cost_) {
   double tot = 0; for (int i = 0; i < 64; i++) tot += hist[i];
   if (tot <= 0) return 0;
   auto emax = [&](int lo, int hi, double n) {   // E[max of 64 draws] of the histogram restricted to bins lo..hi (n = its population)
      if (n <= 0) return 0.0;
      double F = 0, prev = 0, e = 0;
      for (int m = lo; m <= hi; m++) { F += hist[m] / n; const double f64 = std::pow(std::min(F, 1.0), 64.0); e += m * (f64 - prev); prev = f64; }
      return e;
   };
   const double c_inf = emax(0, 63, tot);
   double best = c_inf; int bestk = 0;
   for (int K = 3; K < 40; K++) {
      double ntail = 0; for (int m = K + 1; m < 64; m++) ntail += hist[m];
      if (ntail == 0) break;
      // first launch: bins above K collapse onto K
      double F = 0, prev = 0, e = 0;
      for (int m = 0; m <= K; m++) { F += (m < K ? hist[m] : tot - [&] { double a = 0; for (int j = 0; j < K; j++) a += hist[j]; return a; }()) / tot;
                                     const double f64 = std::pow(std::min(F, 1.0), 64.0); e += m * (f64 - prev); prev = f64; }
      const double c = e + 0.2 + ntail / tot * tail_cost_ * (emax(K + 1, 63, ntail) + 2.0);
      if (c < best) { best = c; bestk = K; }
   }
   return (best < 0.97 * c_inf) ? bestk : 0;
}

}  // namespace exa_host
