// Which kernels the operator runs: the EXA_* switches NonlinearMechOperator reads, what the decision needs from options, partition and transport,
// and the decision itself - one expression per flag.  Pure host code (no HIP include): exa_operator_routes_query evaluates it without a device,
// tests/test_host_logic.py pins the table, tests/routes_check.cpp runs it under the sanitizers.
#pragma once

namespace exa_host {

// The parsed environment: one field per variable, each compared once (routes.cpp).  from_env() is the only place the operator reads the
// environment; it is called once per operator construction and never cached (the tests switch variables between drivers of one process).
struct RouteSwitches {
   bool tet_action_generic = false;    // EXA_TET_ACTION=generic
   bool deterministic = false;         // EXA_DETERMINISTIC=1
   enum class Cap { UNSET, AUTO, FIXED };
   Cap newton_cap_mode = Cap::UNSET;   // EXA_NEWTON_CAP: unset | auto | anything else ("off", "<K>", "<K>,<K2>")
   int newton_cap = 0, newton_cap2 = 0;   // FIXED: "off" -> 0, otherwise atoi of the value and of what follows its first comma
   bool tail_resume_off = false;       // EXA_TAIL_RESUME=off
   bool ea_assembled = false;          // EXA_EA_ASSEMBLED=1
   bool tet_apply_geo_off = false;     // EXA_TET_APPLY_GEO=off
   bool tangent_form_full = false;     // EXA_TANGENT_FORM=full
   bool apply_geo_off = false;         // EXA_APPLY_GEO=off
   bool p2_prepass_off = false;        // EXA_P2_PREPASS=off
   bool tangent_records_off = false;   // EXA_TANGENT_RECORDS=off
   bool qlayout_aos = false;           // EXA_QLAYOUT=aos
   bool jac_field_on = false;          // EXA_JAC_FIELD=on
   bool lean_state_off = false;        // EXA_LEAN_STATE=off
   enum class Overlap { UNSET, OFF, ON };
   Overlap halo_overlap = Overlap::UNSET;   // EXA_HALO_OVERLAP: unset | "off", "0" | anything else
   bool nfev_log = false;              // EXA_NFEV_LOG set
   bool model_times = false;           // EXA_MODEL_TIMES set
   static RouteSwitches from_env();
};

// what the decision needs from options, partition and transport (exa_operator_routes_query takes them as ints in this order)
struct RouteFacts {
   enum { VOCE = 0, VOCE_NL = 1, KMDD = 2 };
   int geom = 0;                 // 0 hexahedra, 1 tetrahedra
   int order = 1;
   bool bbar = false;
   bool ea = false;              // element assembly (otherwise partial assembly)
   int slip = VOCE;              // slip family
   bool several_ranks = false;   // NOT read by decide_routes: carried so that the query's fact vector names the whole situation.  What several ranks
                                 // change is the constructor's step after the decision: overlap_wish becomes the flag through the agreement of all ranks
   bool rccl = false;            // the transport is RCCL
   bool has_bdr_blocks = false;  // Partition::E_bdr > 0
   bool has_nbrs = false;
   bool periodic = false;
   enum { COUNT = 10 };
};

struct OperatorRoutes {
   bool fast_p1, lvec_grad, lvec_resid, compact_tangent, records_setup, geo_resid;
   bool tet_fused, tet_geo;
   bool overlap_wish;            // this rank's wish for the overlapped halo exchange
   bool cap_auto;
   bool qlayout_eb64, lean_state, ea_matrix_free, det, det_unfused;
   bool grad_set_coords;         // GetGradient (tangent-field route) hands x_cur to the action
   int newton_cap, newton_cap2;  // initial caps
   bool tail_resume;
   double tail_cost;
   int action_route;             // Driver.mesh_info: 0 hexahedron kernels, 1 fused tetrahedron action, 2 table-driven E-vector PA, 3 table-driven EA on L-vectors
   bool nfev_log, model_times;   // measurement aids (stderr)
   enum { QUERY_FIELDS = 23 };   // exa_operator_routes_query writes them in the order above, tail_cost in tenths
   void to_ints(int* out) const;
};

// (tetrahedra with B-bar are refused by the operator's constructor before it asks)
OperatorRoutes decide_routes(const RouteFacts& f, const RouteSwitches& sw);

// tail-split controller (see routes.cpp): cap on local-solver evaluations from a 64-bin histogram of their counts; 0 = no cap
int choose_newton_cap(const int* hist64, double tail_cost);
void choose_newton_caps_resume(const int* hist64, double tail_cost, int& k1, int& k2);

}  // namespace exa_host
