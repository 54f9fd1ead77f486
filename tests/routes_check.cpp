// Stand-alone check of the operator's route code (exaconstit_amd/csrc/host/routes.hpp, routes.cpp): RouteSwitches::from_env over awkward values of
// the variables it parses by hand, decide_routes on what comes out, and the two cap choosers over empty, single-bin and saturated histograms.
// No GPU, no Python.  scripts/routes_sanitize.sh builds it with -fsanitize=address,undefined and runs it.
#include "../exaconstit_amd/csrc/host/routes.hpp"
#include "../exaconstit_amd/csrc/host/routes.cpp"
#include <climits>
#include <cstdio>
#include <string>

using namespace exa_host;

static int nbad = 0;
static void expect(bool ok, const char* what) { if (!ok) { nbad++; std::printf("routes_check: wrong: %s\n", what); } }

static RouteSwitches with(const char* k, const char* v) { setenv(k, v, 1); RouteSwitches s = RouteSwitches::from_env(); unsetenv(k); return s; }

int main() {
   using Cap = RouteSwitches::Cap; using Ov = RouteSwitches::Overlap;
   const std::string longx(1 << 20, 'x'), long9(1 << 16, '9'), longc = std::string(1 << 16, ',') + "5";
   for (const char* k : { "EXA_TET_ACTION", "EXA_DETERMINISTIC", "EXA_NEWTON_CAP", "EXA_TAIL_RESUME", "EXA_EA_ASSEMBLED", "EXA_TET_APPLY_GEO", "EXA_TANGENT_FORM", "EXA_APPLY_GEO",
                          "EXA_P2_PREPASS", "EXA_TANGENT_RECORDS", "EXA_QLAYOUT", "EXA_JAC_FIELD", "EXA_LEAN_STATE", "EXA_HALO_OVERLAP", "EXA_NFEV_LOG", "EXA_MODEL_TIMES" }) unsetenv(k);
   {  RouteSwitches s = RouteSwitches::from_env();
      expect(s.newton_cap_mode == Cap::UNSET && s.halo_overlap == Ov::UNSET && !s.deterministic && !s.nfev_log && !s.qlayout_aos, "nothing set"); }
   struct { const char* v; Cap mode; int k1, k2; } caps[] = {
      { "", Cap::FIXED, 0, 0 }, { ",", Cap::FIXED, 0, 0 }, { "4,", Cap::FIXED, 4, 0 }, { "auto,3", Cap::FIXED, 0, 3 }, { "auto", Cap::AUTO, 0, 0 }, { "off", Cap::FIXED, 0, 0 },
      { "-5", Cap::FIXED, -5, 0 }, { "-5,-2", Cap::FIXED, -5, -2 }, { "4,7", Cap::FIXED, 4, 7 }, { " 6 , 9", Cap::FIXED, 6, 9 }, { "4,7,9", Cap::FIXED, 4, 7 }, { "off,7", Cap::FIXED, 0, 7 },
      { longx.c_str(), Cap::FIXED, 0, 0 }, { longc.c_str(), Cap::FIXED, 0, 0 } };
   for (const auto& c : caps) {
      const RouteSwitches s = with("EXA_NEWTON_CAP", c.v);
      expect(s.newton_cap_mode == c.mode && s.newton_cap == c.k1 && s.newton_cap2 == c.k2, std::string(c.v).substr(0, 16).c_str());
   }
   (void)with("EXA_NEWTON_CAP", long9.c_str());   // (out of atoi's range: any value, no fault)
   {  // EXA_TAIL_RESUME=off zeroes the second cap; the Kocks-Mecking family alone runs the controller when nothing is set
      setenv("EXA_TAIL_RESUME", "off", 1);
      const RouteSwitches s = with("EXA_NEWTON_CAP", "4,7");
      unsetenv("EXA_TAIL_RESUME");
      RouteFacts f; OperatorRoutes r = decide_routes(f, s);
      expect(!r.cap_auto && r.newton_cap == 4 && r.newton_cap2 == 0 && !r.tail_resume && r.tail_cost == 4.0, "4,7 with the resume off");
      f.slip = RouteFacts::KMDD; r = decide_routes(f, RouteSwitches());
      expect(r.cap_auto && r.newton_cap == 0 && r.tail_resume && r.tail_cost == 1.5, "Kocks-Mecking default");
   }
   struct { const char* v; Ov o; } ovs[] = { { "off", Ov::OFF }, { "0", Ov::OFF }, { "", Ov::ON }, { "on", Ov::ON }, { "OFF", Ov::ON }, { "00", Ov::ON }, { longx.c_str(), Ov::ON } };
   for (const auto& c : ovs) expect(with("EXA_HALO_OVERLAP", c.v).halo_overlap == c.o, "EXA_HALO_OVERLAP");
   // exact spellings only; "set" is enough for the two measurement aids
   expect(!with("EXA_DETERMINISTIC", "").deterministic && !with("EXA_DETERMINISTIC", "11").deterministic && !with("EXA_DETERMINISTIC", longx.c_str()).deterministic &&
          with("EXA_DETERMINISTIC", "1").deterministic, "EXA_DETERMINISTIC");
   expect(!with("EXA_QLAYOUT", "AOS").qlayout_aos && !with("EXA_QLAYOUT", "aos ").qlayout_aos && with("EXA_QLAYOUT", "aos").qlayout_aos, "EXA_QLAYOUT");
   expect(with("EXA_NFEV_LOG", "").nfev_log && with("EXA_MODEL_TIMES", longx.c_str()).model_times, "measurement aids");
   {  // every combination of facts decides without a fault and gives a route in range
      for (int m = 0; m < 1 << 9; m++) for (int order = 1; order <= 3; order++) {
         RouteFacts f; f.geom = m & 1; f.order = order; f.bbar = m & 2; f.ea = m & 4; f.slip = (m >> 3) % 3; f.several_ranks = m & 32; f.rccl = m & 64;
         f.has_bdr_blocks = f.has_nbrs = m & 128; f.periodic = m & 256;
         int o[OperatorRoutes::QUERY_FIELDS]; const OperatorRoutes r = decide_routes(f, RouteSwitches()); r.to_ints(o);
         expect(r.action_route >= 0 && r.action_route <= 3 && (f.geom == 1) == (r.action_route != 0) && o[20] == r.action_route, "action route");
      }
   }
   // the cap choosers: empty, one bin, saturated counts
   int h[64]; int k1 = -1, k2 = -1;
   auto fill = [&](int v) { for (int& x : h) x = v; };
   auto sane = [&]() { return (k1 == 0 && k2 == 0) || (k1 >= 3 && k1 < 40 && (k2 == 0 || (k2 >= k1 + 2 && k2 < 48))); };
   for (double w : { 1.0, 1.5, 4.0 }) {
      fill(0);
      choose_newton_caps_resume(h, w, k1, k2); expect(choose_newton_cap(h, w) == 0 && k1 == 0 && k2 == 0, "empty histogram");
      for (int b : { 0, 4, 63 }) {
         fill(0); h[b] = 1000; choose_newton_caps_resume(h, w, k1, k2); expect(choose_newton_cap(h, w) == 0 && k1 == 0 && k2 == 0, "one bin");
         h[b] = INT_MAX; choose_newton_caps_resume(h, w, k1, k2); expect(choose_newton_cap(h, w) == 0 && k1 == 0 && k2 == 0, "one saturated bin");
      }
      fill(INT_MAX);
      const int k = choose_newton_cap(h, w); choose_newton_caps_resume(h, w, k1, k2);
      expect((k == 0 || (k >= 3 && k < 40)) && sane(), "all bins saturated");
      fill(0); h[3] = INT_MAX; h[63] = INT_MAX;
      const int kb = choose_newton_cap(h, w); choose_newton_caps_resume(h, w, k1, k2);
      expect((kb == 0 || (kb >= 3 && kb < 40)) && sane(), "two saturated bins");
   }
   std::printf("routes_check: %d wrong values\n", nbad);
   return nbad == 0 ? 0 : 1;
}
