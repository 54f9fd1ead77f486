/* exaconstit_hip.h — C ABI of libexaconstit_hip.so (MI355X / gfx950).
 *
 * The reference (LLNL/ExaConstit v0.7.0) has no C ABI: its replaceable seam for the hot path is two C++ class
 * interfaces.  Each entry point below cites the reference interface it stands in for; INTEGRATION.md shows the
 * MFEM-side adapters (HipExaModel : ExaModel, HipExaNLFIntegrator : ExaNLFIntegrator) that bind them.
 *
 * Conventions
 *   - every pointer marked "dev" is a device pointer owned by the caller; "host" pointers are host memory;
 *   - every array is FP64 and uses the reference's layouts (column-major = first index fastest):
 *       E-vector        (node, comp, elem)            reference src/mechanics_kernels.cpp:28-29
 *       Jacobians       (3, 3, Q, E), J(i,j)=dx_i/dxi_j   reference src/mechanics_operator.cpp:379-390
 *       shape table     (node, dir, qpt)              reference src/mechanics_operator.cpp:249-260
 *       quadrature data (vdim, Q, E)                  reference src/mechanics_model.cpp:209-214
 *       tangent         (6, 6, Q, E) column-major, Voigt (11,22,33,23,13,12), engineering shear
 *   - every function returns int: 0 ok, <0 invalid argument / HIP error (see exa_last_error), and the work is
 *     enqueued on the given stream without host synchronisation unless stated otherwise;
 *   - no global state; one exa_ctx per (mesh partition, material); re-entrant per context.
 */
#ifndef EXACONSTIT_HIP_H
#define EXACONSTIT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct exa_ctx exa_ctx;
typedef void* exa_stream;   /* hipStream_t */

/* model ids: reference src/mechanics_ecmech.hpp:407-414 (Voce), :460-463 (KM-DD); chosen in
 * reference src/mechanics_operator.cpp:49-210 from Model.ExaCMech.{xtal_type,slip_type} */
enum { EXA_FCC_VOCE = 0, EXA_FCC_VOCE_NL = 1, EXA_BCC_VOCE = 2, EXA_BCC_VOCE_NL = 3, EXA_FCC_KMDD = 4, EXA_BCC_KMDD = 5 };
/* reference src/option_types.hpp Assembly / IntegrationType */
enum { EXA_ASSEMBLY_PA = 0, EXA_ASSEMBLY_EA = 1 };
enum { EXA_INTEG_FULL = 0, EXA_INTEG_BBAR = 1 };

enum { EXA_OK = 0, EXA_ERR_ARG = -1, EXA_ERR_HIP = -2, EXA_ERR_STATE = -3, EXA_ERR_UNSUPPORTED = -4 };
/* Which entry points are legal in which context (everything else returns EXA_ERR_UNSUPPORTED with a message in exa_last_error):
 *
 *   route                         layout   entry points                                                               orders / integrators
 *   ----------------------------  -------  -------------------------------------------------------------------------  ----------------------------------
 *   A  E-vector (MFEM adapters)   AOS      exa_jacobians[_from_geom], exa_model_setup, exa_residual_setup/apply,      p = 1..6, full and B-bar (B-bar:
 *                                          exa_grad_setup, exa_grad_apply, exa_grad_diagonal, exa_grad_get_ea,        element assembly only, like the
 *                                          exa_restrict / exa_restrict_transpose_add, exa_calc_dp, exa_vol_avg        reference)
 *   B  fused L-vector             AOS or   A's set-up calls + exa_set_connectivity, exa_model_setup_lvec,             p = 1 full integration; p = 2 full
 *                                 EB64     exa_residual_lvec, exa_grad_apply_lvec (PA, EA from matrices or - with     and B-bar (EB64: L-vector entries
 *                                          exa_set_ea_matrix_free - from the point records), exa_grad_set_coords,     only, exa_residual_setup/apply stay
 *                                          exa_set_tangent_form                                                       AOS); p >= 3: exa_grad_apply_lvec
 *                                                                                                                     for element assembly only
 *   C  record route (driver)      EB64     exa_model_setup_lvec_records + exa_grad_set_coords + exa_grad_apply_lvec   p = 1 full integration, PA or
 *                                          + exa_residual_lvec (Jacobian field optional)                              matrix-free EA, compact tangent form
 *
 *   exa_set_deterministic: ordered sums for route B / C at p = 1 full integration; elsewhere the fused entries refuse and route A + exa_restrict_transpose_add is
 *   the reproducible path.  An adapter that does not care about any of this uses route A and never sees EXA_ERR_UNSUPPORTED. */

typedef struct {
   int model;            /* EXA_* model id */
   int nprops;           /* 17 (Voce), 18 (Voce NL), 24 (KM-DD) — reference src/option_parser.cpp:396-478 */
   const double* props;  /* host; parameter order of reference src/mechanics_ecmech.hpp:395-405,444-458 */
   double temp_k;        /* Properties.temperature (the library overrides it with its EOS temperature, as ExaCMech does) */
   int order;            /* H1 order p: n = Q = (p+1)^3 */
   int nelems;           /* elements of this partition */
   int assembly;         /* EXA_ASSEMBLY_* */
   int integ;            /* EXA_INTEG_* */
   int device;           /* HIP device ordinal; -1 = current */
} exa_config;

/* lifetime -------------------------------------------------------------------------------------------------- */
exa_ctx* exa_create(const exa_config* cfg, int* err);          /* ECMechXtalModel ctor, src/mechanics_ecmech.hpp:126-262 */
void     exa_destroy(exa_ctx* ctx);
const char* exa_last_error(const exa_ctx* ctx);                /* MFEM_ABORT text equivalent */
const char* exa_build_id(void);                                /* 12 hex digits: hash of the library's sources at build time */
const char* exa_kernel_build_id(void);                         /* ... of the device code and its compile flags alone: stamped into the counter files under profiles/ */
int exa_num_state_vars(const exa_ctx* ctx);                    /* numHist + ne + 1 = 28, src/mechanics_ecmech.hpp:136-141 */
int exa_nodes_per_elem(const exa_ctx* ctx);
int exa_qpts_per_elem(const exa_ctx* ctx);

/* reference-element tables built on the host once: src/mechanics_operator.cpp:237-261, src/mechanics_integrators.cpp:184-197 */
int exa_shape_table(const exa_ctx* ctx, double* G_host /*(n,3,Q)*/, double* W_host /*(Q)*/);

/* Element geometry.  exa_create makes hexahedron contexts; exa_create_geom takes the geometry explicitly (same config).
 * Tetrahedra: straight-sided, p = 1 (n = 4, Q = 5) or p = 2 (n = 10, Q = 14), MFEM's node order (vertices, then the edge midpoints of
 * edges (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)) and the rules of IntRules.Get(TETRAHEDRON, 2p + 1) on the unit tetrahedron.  A tetrahedron
 * context refuses EXA_INTEG_BBAR (at creation), exa_model_setup_lvec_records and exa_grad_apply_lvec_blocks (EXA_ERR_UNSUPPORTED). */
enum { EXA_GEOM_HEX = 0, EXA_GEOM_TET = 1 };
exa_ctx* exa_create_geom(const exa_config* cfg, int geometry, int* err);
int exa_element_geometry(const exa_ctx* ctx);                  /* EXA_GEOM_* */
/* Host only (no device needed): the reference-element tables of (geometry, order): G (n,3,Q), W (Q), N (n,Q) shape values (may be NULL).
 * Returns n * 1000 + Q, or EXA_ERR_ARG (hexahedra: order 1 ... 6, tetrahedra: 1 or 2). */
int exa_ref_elem_tables(int geometry, int order, double* G, double* W, double* N);

/* Layout of every quadrature function passed to this context (jacobian, stress, state, ddsdde, dp, any exa_vol_avg field):
 *   EXA_QLAYOUT_AOS  (default) the reference's QuadratureFunction layout (vdim, Q, E), first index fastest;
 *   EXA_QLAYOUT_EB64 [block of 64 elements][q][component][lane = element], exa_qf_size(ctx, vdim) doubles per field.  It is the
 *                    internal layout of the stand-alone driver (every per-value access of a wave is one contiguous 512-byte row:
 *                    the constitutive launch is 1.4x faster at 128^3); p = 1 full integration and p = 2 (plain or B-bar) with
 *                    the L-vector entry points only (exa_residual_setup / exa_residual_apply stay AOS).  An MFEM adapter keeps AOS. */
enum { EXA_QLAYOUT_AOS = 0, EXA_QLAYOUT_EB64 = 1 };
int exa_set_quadrature_layout(exa_ctx* ctx, int layout);
/* EXA_QLAYOUT_AOS, constitutive launches (exa_model_setup, exa_model_setup_lvec): the 64 points of a wave are 64 x 28 / 6 / 9 / 36 CONTIGUOUS doubles of
 * the state / stress / Jacobian / tangent arrays, so the wave moves them with coalesced 16-byte accesses and transposes them through the per-lane LDS
 * stash the kernel owns anyway (inputs once, outputs in three rounds: two tangent halves, then state + stress) instead of 8-byte accesses at a
 * 224 / 288-byte lane stride - the reference's layout at the element-blocked layout's speed, same bits out.  On by default; 0 restores the
 * per-lane strided accesses (A/B runs).  exa_get_aos_staging: the setting (the staged kernels exist for every order and model; the dense
 * launches of a tail split keep strided accesses - their lanes are scattered points). */
int exa_set_aos_staging(exa_ctx* ctx, int on);
int exa_get_aos_staging(const exa_ctx* ctx);
int exa_get_quadrature_layout(const exa_ctx* ctx);               /* EXA_QLAYOUT_* currently selected */
int64_t exa_qf_size(const exa_ctx* ctx, int vdim);

/* ExaModel seam ------------------------------------------------------------------------------------------------ */
/* getHistInfo + init_state_vars (src/mechanics_ecmech.hpp:248-300) with setStateVarData's quaternion splice
 * (src/mechanics_driver.cpp:1058-1154): fills state0 (28,Q,E) from one quaternion per element. */
int exa_init_state(exa_ctx* ctx, double* state0_dev, const double* quats_per_elem_dev /*(4,E)*/, exa_stream s);

/* State layout ------------------------------------------------------------------------------------------------- */
/* The 28 state variables of a quadrature point, all six models (index table of src/mechanics_ecmech.hpp:165-185; numHist + ne + 1,
 * :136-141).  Slot = offset inside the (28, Q, E) quadrature function:
 *
 *    0        shrateEff   effective shear rate of the step, sum_a |gdot_a|            (ecmech::evptn::iHistA_shrateEff, "shrateEff")
 *    1        shrEff      accumulated effective shear, slot 1 += slot 0 * dt          (iHistA_shrEff, "shrEff")
 *    2        flowStr     ExaCMech's flow strength; ExaConstit stores the accumulated plastic work there ("pl_work",
 *                         src/mechanics_ecmech.cpp:154-160) - so does this library
 *    3        nFEval      residual evaluations the local Newton solve (SNLS trust-region dog-leg) of this point took in this step
 *                         (iHistA_nFEval); 2 for an elastic point
 *    4 .. 8   deviatoric elastic strain in the lattice frame, 5-vector              (iHistLbE, "elas_strain")
 *    9 .. 12  lattice orientation, unit quaternion, scalar first                    (iHistLbQ, "quats")
 *    13       hardness: slip-system strength g (Voce kinds) or dislocation density rho (Kocks-Mecking kinds)   (iHistLbH, "hardness")
 *    14 .. 25 the 12 slip rates gdot_a of the converged step                          (iHistLbGdot, "gdot")
 *    26       relative volume                                                         ("rel_vol")
 *    27       internal energy per reference volume                                    ("int_eng")
 *
 * Two slots carry more than a value:
 *    slot 0  is an INPUT of the next step: the hardness update takes the begin-of-step effective shear rate from it instead of
 *            re-reading the 12 slip rates (88 B per point less traffic).  Invariant a caller-supplied state0 must satisfy:
 *            slot 0 == sum_a |slot 14+a|.  It holds for every state this library wrote and for exa_init_state; a state that
 *            comes from elsewhere (restart file, another code) is brought into this form by exa_state_normalize.
 *    slot 3  follows the iteration PATH of the local solve, not only its result.  The library reproduces the reference solver's
 *            path: against a CPU restatement of that solver the count is equal at >= 99.9 % of the points and never differs by more than one
 *            (ulp-level ties of the trust-region acceptance tests; asserted by tests/test_gpu_parity.py, test_gpu_point_fixtures.py,
 *            test_gpu_fullsize.py; measured 99.999 %, profiles/r04_nfev_agreement.txt).  The tail split (exa_set_newton_cap) does not
 *            change it. */
/* state[0] = sum_a |state[14+a]| at every point of a state array in the context's layout (see above) */
int exa_state_normalize(exa_ctx* ctx, double* state_dev, exa_stream s);

/* Checkpoint support.  exa_qf_pack: a quadrature function of vdim values per point in the context's layout -> the canonical
 * (vdim, Q, E) rows of a checkpoint file (EXA_QLAYOUT_AOS order, local element order, vdim Q E doubles); exa_qf_unpack: the reverse (the
 * padding lanes of the last element block keep what they held).  1 <= vdim <= 96.  checksum_dev may be NULL; otherwise it receives, in the
 * same pass, the sum of the bit patterns of the vdim Q E values as unsigned 64-bit integers modulo 2^64 - a value that does not depend on
 * the layout, on the order of the elements or on how they are spread over ranks (partial sums of ranks simply add). */
int exa_qf_pack(exa_ctx* ctx, int vdim, const double* src_dev, double* dst_dev, uint64_t* checksum_dev, exa_stream s);
int exa_qf_unpack(exa_ctx* ctx, int vdim, const double* src_dev, double* dst_dev, uint64_t* checksum_dev, exa_stream s);

/* ExaCMechModel::ModelSetup (src/mechanics_ecmech.cpp:192-258), i.e. StressSetup/StateVarsSetup, grad_calc,
 * kernel_setup, getResponseECM, kernel_postprocessing fused into one launch.  On return (stream order) stress1, state1
 * and the column-major tangent d sigma/d eps hold end-of-step values.  Points whose local solve did not converge are
 * counted; read the count with exa_model_status. */
int exa_model_setup(exa_ctx* ctx, double dt, const double* jacobian_dev /*(3,3,Q,E)*/, const double* vel_evec_dev /*(n,3,E)*/,
                    const double* stress0_dev, const double* state0_dev,
                    double* stress1_dev, double* state1_dev, double* ddsdde_dev, exa_stream s);
/* exa_model_setup + exa_model_status in one call, with the return value the model seam is specified with: < 0 error, 0 every local
 * solve converged, > 0 the number of quadrature points whose ExaCMech solve failed (the reference aborts the run on one: ECMECH_FAIL behind
 * getResponseECM, src/mechanics_ecmech.cpp:176-186).  Synchronises the stream (one 4-byte read-back); the MFEM adapter's ModelSetup uses it. */
int exa_model_setup_checked(exa_ctx* ctx, double dt, const double* jacobian_dev, const double* vel_evec_dev,
                            const double* stress0_dev, const double* state0_dev,
                            double* stress1_dev, double* state1_dev, double* ddsdde_dev, exa_stream s);
/* Same update driven from L-vectors (needs exa_set_connectivity): gathers nodal coordinates / velocities itself and also
 * WRITES the Jacobians (3,3,Q,E) the integrator calls need, i.e. NonlinearMechOperator::Setup's two L->E restrictions and
 * SetupJacobianTerms (src/mechanics_operator.cpp:310-391) fused into the constitutive launch. */
int exa_model_setup_lvec(exa_ctx* ctx, double dt, const double* coords_lvec_dev /*(nnodes,3) byNODES*/, const double* vel_lvec_dev,
                         const double* stress0_dev, const double* state0_dev,
                         double* stress1_dev, double* state1_dev, double* ddsdde_dev, double* jacobian_out_dev, exa_stream s);
/* The same launch with AssembleGradPA (src/mechanics_integrators.cpp:331-414) fused in as well: instead of the 36 tangent entries it
 * writes, for every point, the compact record the L-vector gradient action streams (EXA_TANGENT_DEV5_BULK: the tangent's 5 x 5
 * deviatoric block and bulk term times dt W_q / detJ; D^T in element-assembly contexts), so that neither a tangent field nor a
 * separate exa_grad_setup pass exists on this path.  After it exa_grad_apply_lvec is valid once exa_grad_set_coords has named the
 * coordinates (the same coords_lvec).  Preconditions: p = 1 full integration, EXA_QLAYOUT_EB64, exa_set_connectivity,
 * exa_set_tangent_form(EXA_TANGENT_DEV5_BULK), partial assembly or matrix-free element assembly.  The entry points that read the
 * full 46-double records (exa_grad_apply on E-vectors, exa_grad_diagonal, exa_grad_get_ea) still need exa_grad_setup.
 * jacobian_out_dev may be NULL: the Jacobians are then not written at all (72 B per point less traffic) - on this route both integrator
 * actions can take the geometry from the nodal coordinates (exa_grad_set_coords + exa_residual_lvec with a NULL Jacobian field); a
 * caller that wants volume averages afterwards fills a Jacobian field once with exa_restrict + exa_jacobians. */
int exa_model_setup_lvec_records(exa_ctx* ctx, double dt, const double* coords_lvec_dev, const double* vel_lvec_dev,
                                 const double* stress0_dev, const double* state0_dev,
                                 double* stress1_dev, double* state1_dev, double* jacobian_out_dev, exa_stream s);
/* Lean end-of-step state (0 = off, the default).  With it on, exa_model_setup_lvec_records on an EXA_QLAYOUT_EB64 context - p = 1 and p = 2, the dense
 * launches of a tail split included - does not write the 12 slip rates into state1 slots 14..25.  It leaves what they are a function of instead: the
 * hardness is in slot 13 anyway, the lattice-frame elastic strain of the converged point goes to slots 14..18 and, for the Kocks-Mecking kinds, the
 * thermal factor of the kinetics to slot 19 (40 / 48 B per point instead of 96, and no extra kinetics pass for the Kocks-Mecking kinds); slots
 * 20..25 are not written.  Nothing in a constitutive launch reads slots 14..25 of state0.  exa_slip_rates_from_state turns such an array into the
 * full state in place, with the bits the full launch writes; it must run before anything reads slots 14..25 of it (exa_calc_dp, exa_element_fields,
 * a 28-wide exa_vol_avg, a copy for a checkpoint).  The caller keeps track of which arrays are lean: running it on a full state destroys the rates.
 * The kinetics are those of the LAST lean launch of the context.  Every other launch writes all 28 slots, whatever the switch says.
 * The stand-alone driver turns it on for its own record launches (EXA_LEAN_STATE=off keeps the full state) and materialises on demand. */
int exa_set_lean_state(exa_ctx* ctx, int on);
int exa_get_lean_state(exa_ctx* ctx);   /* 1: the next exa_model_setup_lvec_records of this context leaves a lean state1 */
int exa_slip_rates_from_state(exa_ctx* ctx, double* state_dev, exa_stream s);
/* Tail split of the constitutive launch (0 = off, the default).  The local Newton solve needs 3-6 evaluations at most points and
 * 10-19 at a few per cent of them, and a wave waits for its slowest lane (measured wave max / mean = 1.2 ... 2.7).  With max_evals = K
 * the launch stops a point after K residual evaluations and a second, dense launch of the same kernel redoes exactly those points from
 * scratch without a cap, so every output - the evaluation count in state slot 3 included - is the one of the uncapped solve.
 * exa_model_tail_count (synchronises) returns how many points the last launch handed over. */
int exa_set_newton_cap(exa_ctx* ctx, int max_evals);
/* The same with the dense launch resuming instead of starting over (resume = 1, the default of a context): a point that is cut off leaves
 * its solver state - accepted iterate, trust radius, evaluation count; 80 bytes, stored by list slot - and the dense launch restores (r, J)
 * with one evaluation at that iterate and carries on, bit for bit the uncapped iteration.  max_evals_2 > max_evals (0 = off) adds a second
 * level: the dense launch stops at max_evals_2 evaluations and a third launch finishes what is left (the evaluation counts of a
 * Kocks-Mecking RVE have a second mode near 10 and a thin tail up to 20: two dense launches waste fewer idle lanes than one).
 * With resume on, the capped launch of a Kocks-Mecking model also lists a point at the moment one of its trial steps is rejected (such a
 * point sits at its accepted iterate with a smaller trust radius - a resumable state - and would be listed a few evaluations later anyway),
 * so that no wave of the full launch pays the re-evaluation of the accepted point; same bits again.
 * exa_set_newton_cap(ctx, K) is exa_set_newton_caps(ctx, K, 0, <current resume setting>). */
int exa_set_newton_caps(exa_ctx* ctx, int max_evals, int max_evals_2, int resume);
int exa_model_tail_count(exa_ctx* ctx, exa_stream s);
/* Element-blocked p = 1 record launches (exa_model_setup_lvec_records) of this context so far: out2[0] through the kernel entry that has the tail-split
 * arguments compiled out - Voce kinds, no cap in force, no Jacobian field asked for -, out2[1] through the generic kernel (a sequence of capped and dense
 * launches counts once).  EXA_MODEL_POLICY=off in the environment (read per launch) keeps every launch generic: an A/B switch, the bits are the same. */
int exa_model_record_launches(exa_ctx* ctx, long long* out2);
/* Let the library choose max_evals itself (what the stand-alone driver does for its own launches, host/driver.hip): after the first four launches
 * of exa_model_setup / _lvec / _lvec_records and after every fourth one from then on, the evaluation counts the launch left in state1 are binned
 * (exa_model_nfev_hist: one small launch and a 256-byte read-back that waits for the stream) and the cap of the next launches is the K that
 * minimises  E[max of 64 draws of min(n, K)] + 0.2 + (share of points above K) * tail_cost * (E[max of 64 draws | n > K] + 2)  - or no cap when that
 * does not beat the uncapped launch by 3 %.  mode: 0 = off (and the cap is cleared), 1 = for the Kocks-Mecking models only - the driver's default:
 * at 128^3 the BCC launch takes 7.2 ms with it and 17.3 ms without; the Voce launches never find a paying cap in steady state -, 2 = every model.
 * tail_cost <= 0: the measured defaults (1.5 Kocks-Mecking, 4 Voce).  Results do not depend on the cap (see above), only the launch time does.
 * The MFEM adapters (include/exaconstit_mfem_adapters.hpp) switch mode 1 on. */
int exa_set_newton_cap_auto(exa_ctx* ctx, int mode, double tail_cost);
int exa_get_newton_cap(exa_ctx* ctx);   /* the cap in force (0 = none) */
/* histogram (64 bins, last bin = 63 and more) of the evaluation counts stored in slot 3 of a state array; synchronises.  The driver
 * picks max_evals from it (host/routes.cpp, choose_newton_cap). */
int exa_model_nfev_hist(exa_ctx* ctx, const double* state_dev, int* hist64_host, exa_stream s);
/* synchronises the stream; returns the number of non-converged points of the last exa_model_setup (>= 0) */
int exa_model_status(exa_ctx* ctx, exa_stream s);

/* calcDpMat (src/mechanics_ecmech.hpp:303-357): dp (3,3,Q,E) from the slip rates and orientation stored in state */
int exa_calc_dp(exa_ctx* ctx, const double* state_dev, double* dp_dev, exa_stream s);

/* geometry helpers (MFEM GeometricFactors + re-layout, src/mechanics_operator.cpp:350-391; grad_calc on any field,
 * src/mechanics_kernels.cpp:7-78, used for the deformation gradient src/mechanics_operator.cpp:393-427) */
int exa_jacobians(exa_ctx* ctx, const double* coords_evec_dev /*(n,3,E)*/, double* jacobian_dev, exa_stream s);
/* Re-layout of mfem::GeometricFactors::J (Q,3,3,E) into the (3,3,Q,E) Jacobian array (src/mechanics_operator.cpp:377-391,
 * src/mechanics_integrators.cpp:225-238): what an MFEM-side adapter calls instead of exa_jacobians. */
int exa_jacobians_from_geom(exa_ctx* ctx, const double* geom_J_dev /*(Q,3,3,E)*/, double* jacobian_dev, exa_stream s);
int exa_grad_calc(exa_ctx* ctx, const double* jacobian_dev, const double* field_evec_dev, double* grad_dev /*(3,3,Q,E), overwritten*/, exa_stream s);

/* ExaNLFIntegrator seam ---------------------------------------------------------------------------------------- */
/* AssemblePA (src/mechanics_integrators.cpp:160-314): D = W sigma adj(J)^T kept inside the context */
int exa_residual_setup(exa_ctx* ctx, const double* jacobian_dev, const double* stress1_dev, exa_stream s);
/* AddMultPA (src/mechanics_integrators.cpp:518-557): y_evec += G^T D */
int exa_residual_apply(exa_ctx* ctx, double* y_evec_dev, exa_stream s);
/* PA: TransformMatGradTo4D + AssembleGradPA (src/mechanics_model.cpp:949-1061, src/mechanics_integrators.cpp:331-513)
 * EA: AssembleEA (src/mechanics_integrators.cpp:756-1017).  The tangent is the column-major matGrad of exa_model_setup. */
int exa_grad_setup(exa_ctx* ctx, double dt, const double* jacobian_dev, const double* ddsdde_dev, exa_stream s);
/* AddMultGradPA (src/mechanics_integrators.cpp:562-622) | element mat-vec (spec src/mechanics_operator_ext.cpp:303-314):
 * y_evec += K_e x_evec */
int exa_grad_apply(exa_ctx* ctx, const double* x_evec_dev, double* y_evec_dev, exa_stream s);
/* AssembleGradDiagonalPA (src/mechanics_integrators.cpp:625-748) | EA diagonal (spec src/mechanics_operator_ext.cpp:246-252):
 * diag_evec += diag(K_e) */
int exa_grad_diagonal(exa_ctx* ctx, double* diag_evec_dev, exa_stream s);
/* EA only: copy the element matrices out in the reference layout (3n,3n,E) column-major, dof = node + n*comp */
int exa_grad_get_ea(exa_ctx* ctx, double* emat_dev, exa_stream s);

/* L-vector conveniences for callers without MFEM (element restriction, spec src/mechanics_operator_ext.cpp:149-157) -- */
/* connectivity (n,E) of local node -> L-vector node; L-vectors are byNODES: [x0..xN, y0.., z0..] with nnodes entries per comp */
int exa_set_connectivity(exa_ctx* ctx, const int32_t* conn_dev /*(n,E)*/, int nnodes);
int exa_restrict(exa_ctx* ctx, const double* lvec_dev, double* evec_dev, exa_stream s);                 /* L -> E */
int exa_restrict_transpose_add(exa_ctx* ctx, const double* evec_dev, double* lvec_dev, exa_stream s);   /* L += E^T */
/* fused gather / apply / scatter-add of the gradient action on L-vectors (the PCG inner kernel): y_L += K x_L.
 * mask_dev (nullable, 3*nnodes bytes): essential dofs — x is read as 0 there (spec src/mechanics_operator_ext.cpp:143-146). */
int exa_grad_apply_lvec(exa_ctx* ctx, const double* x_lvec_dev, double* y_lvec_dev, const uint8_t* mask_dev, exa_stream s);
/* The same action on `ncols` (1 .. EXA_GRAD_COLS_MAX) column vectors in one call: column k reads x_dev + k ldx and adds into y_dev + k ldy
 * (ldx, ldy in doubles, >= 3 nnodes).  The record of a point is loaded once per pass and applied to up to three columns, so the record
 * stream - most of what the action moves - is shared among them; every column's result is what exa_grad_apply_lvec gives for it, up to the
 * order of the atomic addends, whatever the other columns are.  mask_dev as above (one mask for all columns).  gates (host array of ncols
 * device pointers; the array and every entry may be NULL): a non-zero double at gates[k] leaves column k out - it is neither read nor
 * written.  Built for ONE configuration: hexahedra at p = 1 full integration with nodal coordinates named (exa_grad_set_coords), partial
 * assembly or element assembly from the point records, atomic scatter.  Every other context - p >= 2, tetrahedra, B-bar, assembled element
 * matrices, deterministic mode, no coordinates - returns EXA_ERR_UNSUPPORTED without touching y: loop exa_grad_apply_lvec there. */
enum { EXA_GRAD_COLS_MAX = 16, EXA_GRAD_COLS_DEFAULT = 3 };
int exa_grad_apply_lvec_cols(exa_ctx* ctx, int ncols, const double* x_dev, int64_t ldx, double* y_dev, int64_t ldy, const uint8_t* mask_dev,
                             const double* const* gates, exa_stream s);
/* private (scratch) bytes per lane of the kernels behind exa_grad_apply_lvec_cols and the macroscopic tangent in the loaded code object:
 * out8 = { column action at 1, 2, 3 columns per pass, affine columns, contraction (9 columns, 1 column), its combine, 0 }; 0, or -1 without a device */
int exa_tangent_scratch_bytes(int* out8);
/* p = 2 multigrid (generated hexahedral box of ne[0] x ne[1] x ne[2] local elements, nodes numbered x fastest on the (2 ne + 1)^3 grid): this
 * rank's part of the trilinear Galerkin product P^T K P on the element vertices and of the diagonal of K, both from the point records
 * exa_grad_apply_lvec reads (compact records with geometry or 46-double records, the transposed tangent under element assembly), in one pass
 * each, gathered in a fixed order (no atomics: the same bits for the same records).
 *   elem_at_dev  local element index at position ex + ne[0] (ey + ne[1] ez) of the box
 *   S_dev        (nullable) 243 doubles per vertex, [(o * 9 + 3 r + c) * NV + vertex], o = (dx+1) + 3 (dy+1) + 9 (dz+1), NV = prod (ne + 1); rows
 *                and columns of the dofs marked in mask1_dev (3 NV bytes) are zero
 *   diag_dev     (nullable) 3 nnodes doubles, zero on the dofs marked in mask0_dev (3 nnodes bytes)
 * B-bar contexts: the same two products of the B-bar operator, with the element-average gradients the action reads (those of the
 * last exa_grad_setup, or of the driver's refresh on the record route; EXA_ERR_STATE where there are none yet)
 * (a small per-element pre-pass contracts them onto the eight embedded trilinear functions first).
 * EXA_ERR_UNSUPPORTED, nothing written, where the L-vector action does not run from such records (deterministic mode, assembled element
 * matrices, other orders, tetrahedra). */
int exa_grad_mg_p2_build(exa_ctx* ctx, const int* ne, const int32_t* elem_at_dev, const uint8_t* mask0_dev, const uint8_t* mask1_dev, double* S_dev,
                         double* diag_dev, exa_stream s);
/* private (scratch) bytes per lane of its kernels in the loaded code object: out8 = { vertex stencil: 46-double records plain, transposed, compact
 * records plain, transposed; diagonal: the same four }; 0, or -1 without a device */
int exa_mg_p2_scratch_bytes(int* out8);
/* ... and of the B-bar forms of the same kernels, in the same order, then of the pre-pass: out9; 0, or -1 without a device */
int exa_mg_p2_bbar_scratch_bytes(int* out9);
/* Optional (p = 1 partial assembly, L-vector action): the nodal coordinates (nnodes,3 byNODES) the Jacobians given to exa_grad_setup
 * were computed from.  When set, exa_grad_apply_lvec recomputes adj(J) from them instead of streaming it from its per-point record
 * (36 instead of 46 doubles per point from HBM); the array must stay unchanged until the next exa_grad_setup.  NULL switches it off. */
int exa_grad_set_coords(exa_ctx* ctx, const double* coords_lvec_dev);
/* Form of the tangent the p = 1 partial-assembly action streams when the geometry is recomputed (exa_grad_set_coords):
 *   EXA_TANGENT_FULL       (default) the 36 entries of ddsdde;
 *   EXA_TANGENT_DEV5_BULK  ddsdde = V65 D V65^T + K m m^T, m = (1,1,1,0,0,0): a 5 x 5 block in the deviatoric vector basis of ExaCMech
 *                          plus a bulk term - what every ExaCMech evptn model returns (26 numbers, 13 instead of 18 16-byte loads per point).
 *                          exa_grad_setup projects ddsdde onto that form; the projection is exact only if the tangent has the form, which
 *                          exa_grad_tangent_defect measures (max over the points of |C - projection|_max / |C|_max; ~1e-16 for ExaCMech
 *                          tangents).  The caller is responsible for checking it; the stand-alone driver does on every GetGradient.
 *                          p = 1 partial assembly: exa_grad_setup then writes the compact records only (71 instead of 117 doubles moved per point); the
 *                          46-double records that exa_grad_diagonal, exa_grad_apply on E-vectors and an L-vector action without exa_grad_set_coords
 *                          read are built when one of them is first called, from the jacobian_dev / ddsdde_dev arrays of that exa_grad_setup - which
 *                          must therefore stay unchanged until then (they do within a Newton iteration).
 *   EXA_TANGENT_DEV5_BULK_GEO  the same compact tangent with adj(J) and W detJ kept in the record (36 numbers, 18 pairs): for the E-vector action
 *                          exa_grad_apply at p = 1 partial assembly, which has no nodal coordinates to recompute the geometry from - 360 instead of 440 bytes per
 *                          point and action (what HipExaNLFIntegrator selects after the same defect check); the 46-double records are built on demand as above. */
enum { EXA_TANGENT_FULL = 0, EXA_TANGENT_DEV5_BULK = 1, EXA_TANGENT_DEV5_BULK_GEO = 2 };
int exa_set_tangent_form(exa_ctx* ctx, int form);
int exa_grad_tangent_defect(exa_ctx* ctx, const double* ddsdde_dev, double* defect_host, exa_stream s);
/* Element assembly without the element matrices: with `on` != 0 exa_grad_setup stops after the per-point records (and the
 * element-average gradients of the B-bar integrator) and exa_grad_apply_lvec computes the action of the element matrices from them -
 * the same operator (y_j += sum_i A_ij x_i, A = B^T C B, i.e. B^T C^T B x), from 0.3-0.4 KB per point instead of 4.6 KB (p = 1,
 * 24 x 24) or 52 KB (p = 2, 81 x 81) per element.  Built for p = 1 full integration and for p = 2 (plain and B-bar); other
 * contexts keep the assembled path.  The matrices themselves are assembled on the first call that needs them (exa_grad_apply on
 * E-vectors, exa_grad_diagonal, exa_grad_get_ea).  Default: off. */
int exa_set_ea_matrix_free(exa_ctx* ctx, int on);
/* self-test hook (tests/test_gpu_point_fixtures.py): the Kocks-Mecking kinetics' own exp and near-1 log evaluated on the device,
 * out[0..n) = exp(x), out[n..2n) = log(x) (the latter meaningful for x in [0.75, 1.25]); no context needed */
int exa_selftest_km_math(const double* x_dev, double* out_dev, int n, exa_stream s);
/* self-test hook (tests/test_gpu_offpath_constitutive.py): the rotation arithmetic of the point update evaluated on the device.
 * out[2 i], out[2 i + 1] = sine, cosine of x[i] by the kernel's own sincos (i < n); then, for each whole triple
 * (x[3 t], x[3 t + 1], x[3 t + 2]), t < n / 3, taken as a rotation vector, out[2 n + 18 t ...] = the exponential map's rotation matrix A
 * (9 numbers, row-major) and right Jacobian Tr (9 numbers).  out_dev holds 2 n + 18 (n / 3) doubles; no context needed */
int exa_selftest_rot_math(const double* x_dev, double* out_dev, int n, exa_stream s);
/* Bit-reproducible E->L sums (reference: mfem::ElementRestriction::MultTranspose; the fused kernels here scatter with FP64 atomics, whose
 * order - and therefore the last bits of the L-vector, and from there every CG iterate - changes from run to run).  With `on` != 0
 * exa_residual_lvec, exa_grad_apply_lvec (partial assembly and element assembly from the point records) and exa_restrict_transpose_add
 * write per-element outputs and add them node by node in ascending element order (node -> element table built once per connectivity).
 * Costs one extra write + read of the element outputs (24 doubles per element).  The fused L-vector entries are ordered for p = 1 full
 * integration; in other contexts they return EXA_ERR_UNSUPPORTED while the mode is on and the E-vector entries + exa_restrict_transpose_add
 * are the reproducible route (what the stand-alone driver then takes).  Default off. */
int exa_set_deterministic(exa_ctx* ctx, int on);
/* fused AssemblePA + AddMultPA + E->L: y_L += B^T sigma (p = 1 full integration; p = 2 full integration and B-bar, where the
 * element-average gradients are refreshed from the Jacobians first: ICExaNLFIntegrator::AssemblePA + AddMultPA).
 * p = 1 full integration: jacobian_dev may be NULL when exa_grad_set_coords has named the nodal coordinates of the configuration -
 * adj(J) is then recomputed from them (the scatter gathers the connectivity anyway) instead of read from a Jacobian field. */
int exa_residual_lvec(exa_ctx* ctx, const double* jacobian_dev, const double* stress1_dev, double* y_lvec_dev, exa_stream s);
/* Per-element output fields: the element averages behind the reference's SystemDriver::Project* calls (src/system_driver.cpp:560-870), one row
 * of EXA_NFIELDS doubles per element, out_dev [E][EXA_NFIELDS] row-major.  With w_q = W_q det J_q of the configuration the Jacobians / coordinates
 * describe (the stand-alone driver passes the converged one, like its volume averages):
 *   EXA_F_VOLUME               1   ElementVolume       sum_q w_q
 *   EXA_F_CENTROID             3   ElemCentroid        sum_q w_q x(xi_q) / vol, x interpolated from xe_dev (ProjectCentroid)
 *   EXA_F_STRESS               6   Stress              sum_q w_q sigma_q / vol, Voigt (11,22,33,23,13,12) (ProjectModelStress = CalcElementAvg)
 *   EXA_F_VONMISES             1   VonMisesStress      of the averaged stress, sqrt(((s0-s1)^2 + (s1-s2)^2 + (s2-s0)^2 + 6 (s3^2 + s4^2 + s5^2)) / 2)
 *   EXA_F_HYDROSTATIC          1   HydrostaticStress   (s0 + s1 + s2) / 3 of the averaged stress
 *   EXA_F_DPEFF                1   DpEff               average of state slot 0 (shrateEff)
 *   EXA_F_EFFPLASTICSTRAIN     1   EffPlasticStrain    average of state slot 1 (shrEff)
 *   EXA_F_HARDNESS             1   Hardness            average of state slot 13
 *   EXA_F_SHEARRATE           12   ShearRate           averages of state slots 14..25
 *   EXA_F_ORIENTATION          4   LatticeOrientation  averages of state slots 9..12 normalised to unit length (ProjectOrientation)
 *   EXA_F_XTALELASTICSTRAIN    6   XtalElasticStrain   ProjectElasticStrains from the averaged slots 4..8 (e) and 26 (rel_vol): t1 = e0/sqrt 2,
 *                                                      t2 = e1/sqrt 6, v = ln rel_vol -> (t1-t2+v, -t1-t2+v, sqrt(2/3) e1+v, e4/sqrt 2, e3/sqrt 2, e2/sqrt 2)
 * Both quadrature layouts, p = 1..6.  jacobian_dev may be NULL at p = 1: det J is then recomputed from the 24 node coordinates of xe_dev
 * (the current nodal coordinates as an E-vector (n,3,E), needed for the centroid in any case).  One launch, no atomics, fixed summation order:
 * every call on the same data gives the same bits. */
enum { EXA_NFIELDS = 37, EXA_F_VOLUME = 0, EXA_F_CENTROID = 1, EXA_F_STRESS = 4, EXA_F_VONMISES = 10, EXA_F_HYDROSTATIC = 11, EXA_F_DPEFF = 12,
       EXA_F_EFFPLASTICSTRAIN = 13, EXA_F_HARDNESS = 14, EXA_F_SHEARRATE = 15, EXA_F_ORIENTATION = 27, EXA_F_XTALELASTICSTRAIN = 31 };
int exa_element_fields(exa_ctx* ctx, const double* jacobian_dev, const double* stress_dev, const double* state_dev, const double* xe_dev,
                       double* out_dev, exa_stream s);
/* Lattice strains of {hkl} fibres (the light-up analysis; reference scripts/postprocessing/calc_lattice_strain.py) on the rows of
 * exa_element_fields: fields_dev [E][EXA_NFIELDS] (device).  axes [naxes][3] (host) are unit axes grouped by family: family j owns
 * axes[axis_offsets[j] .. axis_offsets[j + 1]) (host offsets, axis_offsets[0] = 0), 1 to 24 axes that are signed permutations of the family's
 * first axis - the cubic orbit of exa_cubic_fiber_axes.  s_dir (host) is the unit sample direction.  Per element, with u = R(q)^T s
 * (R = quat_to_mat of EXA_F_ORIENTATION, crystal -> sample) and eps the EXA_F_XTALELASTICSTRAIN tensor: the element is in fibre j iff
 * max_c |u . c| > cos_tol, and eps_s = u^T eps u.  out_dev (device) receives 2 nhkl + 1 local sums: out[2j] = sum_{e in j} V_e eps_s,
 * out[2j + 1] = sum_{e in j} V_e, out[2 nhkl] = sum_e V_e (V = EXA_F_VOLUME).  1 <= nhkl <= EXA_LATTICE_MAX_HKL.  Two launches (partial sums
 * per block in the context's scratch, then one block), no atomics: every call on the same data gives the same bits.  Does not synchronise. */
enum { EXA_LATTICE_MAX_HKL = 16 };
int exa_lattice_strains(exa_ctx* ctx, const double* fields_dev, int nhkl, const double* axes, const int* axis_offsets, const double* s_dir,
                        double cos_tol, double* out_dev, exa_stream s);
/* host only: the distinct fibre axes of the plane family {hkl} of a cubic crystal - the orbit of (h, k, l) / |(h, k, l)| under the 24 proper
 * rotations, a direction and its negative counted once (first non-zero component positive).  Writes min(count, max) axes to out [.][3]
 * (out may be NULL) and returns the count (4 for 111, 3 for 200, 6 for 220, 12 for 311, 24 for 123), or -1 for (0, 0, 0). */
int exa_cubic_fiber_axes(int h, int k, int l, double* out, int max);
/* Per-grain sums of the rows of exa_element_fields (fields_dev [E][EXA_NFIELDS], device), the reductions behind the grain averages.
 * plan (int32) describes a grain map of the context's E elements; exa_grain_plan builds it on the host once per map, and the caller keeps the
 * host copy (plan_host) and a device copy (plan_dev).  Grain ids are 1-based; row g - 1 of the outputs belongs to grain g, 1 <= g <= G.
 *   pass 1: out_dev [G][EXA_GRAIN_NSUMS] receives, for every grain with local elements, the sums over them of
 *           V, 1, V sigma (6), V eps_s (6), V eps_x (6), V EffPlasticStrain, V DpEff, V Hardness, V ShearRate (12), V s q (4)
 *           (V = EXA_F_VOLUME, sigma = EXA_F_STRESS, eps_x = EXA_F_XTALELASTICSTRAIN, eps_s = R(q) eps_x R(q)^T with R = quat_to_mat of
 *           q = EXA_F_ORIENTATION (crystal -> sample), tensor components in Voigt order 11 22 33 23 13 12; s = +1 if q . q_ref >= 0, else -1),
 *           quats_dev [G][4] (device) = the reference orientations q_ref.
 *   pass 2: quats_dev [G][4] = the unit grain means qbar; out_dev is planar [2][G]: out[g - 1] = sum V theta, out[G + g - 1] = max theta, with
 *           theta = 2 atan2(|d_vec|, |d_0|) in degrees, d = conj(qbar) (x) q.
 * Rows of grains without local elements are not written: the caller zero-fills out_dev.  work_dev (device) holds work_doubles doubles
 * (exa_grain_plan).  Grain-sorted 64-element chunks, levels of boundary partials, no atomics: every call on the same data gives the same bits.
 * Does not synchronise. */
enum { EXA_GRAIN_NSUMS = 39 };
int exa_grain_sums(exa_ctx* ctx, int pass, const double* fields_dev, const int32_t* plan_host, const int32_t* plan_dev, int G, const double* quats_dev,
                   double* work_dev, double* out_dev, exa_stream s);
/* host only: the plan of exa_grain_sums for E elements with 1-based grain ids grain_of_elem[E] (elements sorted by grain, stable in element
 * index, cut into 64-element chunks, and the levels of the chunks' boundary partials).  Reports its length in *plan_len and the workspace in
 * *work_doubles (either may be NULL) and writes it to plan when plan_cap suffices (plan may be NULL: a size query).  Returns 0, or
 * EXA_ERR_ARG for an id < 1 or a too small plan_cap. */
int exa_grain_plan(int64_t E, const int32_t* grain_of_elem, int32_t* plan, int64_t plan_cap, int64_t* plan_len, int64_t* work_doubles);
/* Texture: pole-figure and inverse-pole-figure weights of the rows of exa_element_fields (fields_dev [E][EXA_NFIELDS], device) on
 * the equal-angle grid of resolution res_deg (exa_texture_grid).  Sets 0 .. npf - 1 are pole figures: family j owns the unit crystal axes
 * pf_axes[pf_axis_offsets[j] .. pf_axis_offsets[j + 1]) [3] (host; 1 to 24 signed permutations of its first axis - the cubic orbit of
 * exa_cubic_fiber_axes), and each element adds its N_j poles p = R(q) c.  Sets npf .. npf + nipf - 1 are inverse pole figures of the sample
 * directions ipf_dirs [nipf][3] (host, normalised here): u = R(q)^T d and its 24 images S_k u under the proper cubic rotations.  R = quat_to_mat of
 * EXA_F_ORIENTATION (crystal -> sample).  Every pole is binned by exa_texture_bin and carries the count rint(V 2^-quantum_log2 / N) (N = N_j or
 * 24, V = EXA_F_VOLUME); out_dev [npf + nipf][n_alpha][n_beta] (device, int64) receives the summed counts.  Integer sums only: every call on
 * the same rows gives the same bits in any element order and on any split of the rows.  0 <= npf <= EXA_TEXTURE_MAX_HKL, 0 <= nipf <=
 * EXA_TEXTURE_MAX_DIRS, npf + nipf >= 1; the caller picks quantum_log2 so that the counts cannot overflow (exa_texture_quantum_log2).
 * Does not synchronise. */
enum { EXA_TEXTURE_MAX_HKL = 16, EXA_TEXTURE_MAX_DIRS = 3 };
int exa_texture_weights(exa_ctx* ctx, const double* fields_dev, int npf, const double* pf_axes, const int* pf_axis_offsets, int nipf,
                        const double* ipf_dirs, double res_deg, int quantum_log2, int64_t* out_dev, exa_stream s);
/* out_dev[0] (device) = the largest EXA_F_VOLUME of the rows (0 without rows).  Does not synchronise. */
int exa_texture_volume_max(exa_ctx* ctx, const double* fields_dev, double* out_dev, exa_stream s);
/* host only: the quantum exponent for rows whose largest volume over all ranks is vmax and whose element count over all ranks is n_elements:
 * the q with 2^(q + 60) <= vmax n_elements < 2^(q + 61), so that every set sums to at most about 2^61 counts (0 when vmax <= 0). */
int exa_texture_quantum_log2(double vmax, int64_t n_elements);
/* host only: the grid of resolution res_deg, n_alpha = 90 / res_deg rings and n_beta = 360 / res_deg sectors.  res_deg must lie in [2, 30]
 * and divide 90.  Returns 0, or -1 for any other res_deg. */
int exa_texture_grid(double res_deg, int* n_alpha, int* n_beta);
/* host only: the bin (ring *i, sector *k) of the direction p3 [3] - the code the kernel runs: p -> -p when p_z < 0, or p_z = 0 and (p_y < 0, or
 * p_y = 0 and p_x < 0); alpha = atan2(sqrt(p_x^2 + p_y^2), p_z), beta = atan2(p_y, p_x) in [0, 360) degrees (0 at the pole);
 * i = min(floor(alpha / res_deg), n_alpha - 1), k = floor(beta / res_deg) mod n_beta.  Returns 0, or -1 for a bad res_deg. */
int exa_texture_bin(const double* p3, double res_deg, int* i, int* k);
/* Intragranular misorientation and lattice curvature on the rows of exa_element_fields (fields_dev [E][EXA_NFIELDS], device), for
 * any context with connectivity (exa_set_connectivity): hexahedra p = 1..6, tetrahedra p = 1, 2, both quadrature layouts.  grain_of_elem_dev [E]
 * (device, int32) are 1-based grain ids and qbar_dev [G][4] (device) the unit grain means; an id outside 1 .. G takes the identity as its mean.
 * Per element: delta = s q (x) conj(qbar_g) with s = +-1 so that delta_0 >= 0, omega = 2 atan2(|delta_vec|, delta_0) delta_vec / |delta_vec|
 * (radians, sample frame; 0 when delta_vec = 0).  The recovery runs over the vertex nodes only (the first 8 / 4 entries of an element's
 * connectivity).  Three calls, so that the caller can add up the copies of a shared node in between:
 *   exa_curvature_nodal     writes the per-element record (omega (3), V, g) to work_dev and the sums over the holders of every node to nodal_dev,
 *                           planar [planes][nnodes]: V omega (3) | V, holder count, sum g_lo | sum g_lo^2, sum g_hi, sum g_hi^2 (g_lo, g_hi the
 *                           16-bit halves of the id).  Every triple of planes is a byNODES nodal 3-vector: sum it over ranks and periodic images
 *                           like any assembled L-vector.  The last five planes are integers below 2^53, exact in any summation order.  One lane
 *                           per node walks the node -> element table of the deterministic E->L sums in its stored order (built, with one
 *                           device -> host copy of the connectivity, by the first call on a connectivity); no atomics.
 *   exa_curvature_elements  reads work_dev as exa_curvature_nodal left it (same fields_dev, ids and means: they are not read again) and the summed
 *                           nodal_dev.  A node is mixed when its holders do not all carry one id: count x sum g^2 != (sum g)^2 for either half.
 *                           omega~_a = (sum V omega / sum V)_a at an unmixed vertex, the element's own omega at a mixed one;
 *                           kappa_ij = sum_a omega~_a,i dN_a/dx_j at the centroid, N_a the trilinear / linear vertex functions on the vertex
 *                           coordinates of xe_dev (current coordinates as an E-vector (n,3,E)); alpha_ij = kappa_ji - delta_ij kappa_kk
 *                           (elastic-strain gradients neglected).  out_dev [E][EXA_NCURV]: EXA_C_ROTVEC omega (3, radians), EXA_C_GROD |omega|
 *                           (degrees), EXA_C_KAM mean over the unmixed vertices of |Omega_a - omega| (degrees; 0 without one), EXA_C_CURVATURE
 *                           kappa row-major (9, radians per length), EXA_C_NYENORM |alpha|_F, EXA_C_GND |alpha|_F / burgers (burgers > 0 in
 *                           the mesh's length unit).
 *   exa_curvature_summary   out_dev [7] (device) = local sum V, sum V GROD, sum V KAM, sum V GND, max GROD, max KAM, max GND over the rows curv_dev
 *                           of exa_curvature_elements (V = EXA_F_VOLUME of fields_dev); partial sums per block in the context's scratch, then
 *                           one block.
 * No atomics, fixed summation orders: every call on the same data gives the same bits.  None of them synchronises. */
enum { EXA_NCURV = 16, EXA_C_ROTVEC = 0, EXA_C_GROD = 3, EXA_C_KAM = 4, EXA_C_CURVATURE = 5 /* 9, row-major kappa_ij */, EXA_C_NYENORM = 14, EXA_C_GND = 15 };
int exa_curvature_nodal(exa_ctx* ctx, const double* fields_dev, const int32_t* grain_of_elem_dev, int G, const double* qbar_dev, double* work_dev,
                        double* nodal_dev, exa_stream s);
int exa_curvature_elements(exa_ctx* ctx, const double* fields_dev, const int32_t* grain_of_elem_dev, int G, const double* qbar_dev, const double* work_dev,
                           const double* nodal_dev, const double* xe_dev, double burgers, double* out_dev, exa_stream s);
int exa_curvature_summary(exa_ctx* ctx, const double* fields_dev, const double* curv_dev, double* out_dev /* 7 */, exa_stream s);
/* host only: doubles of work_dev for E elements and the plane count of nodal_dev (a multiple of 3; nodal_dev holds planes x nnodes doubles);
 * either output may be NULL.  Returns 0, or EXA_ERR_ARG for E < 0. */
int exa_curvature_sizes(int64_t E, int64_t* work_doubles, int* nodal_planes);
/* Slip-system activity and the Fatemi-Socie fatigue indicator parameter on the rows of exa_element_fields (fields_dev
 * [E][EXA_NFIELDS], device), for any context: they read rows only.  Slip system a = 0 .. 11 in the order of the slip rates (state slots 14 .. 25).
 * acc_dev (device) holds the accumulators that persist across the steps of a run, planar [EXA_NSLIPACC][E_pad] with E_pad = E rounded up to 64
 * (exa_slip_activity_sizes), 12 planes each of: Gamma (EXA_ACC_SLIP), A (EXA_ACC_ABS), Gamma_min (EXA_ACC_MIN), Gamma_max (EXA_ACC_MAX), N_max
 * (EXA_ACC_NMAX); the caller zero-fills it at the start of a run.  Entries [.][E .. E_pad) are never read or written.
 *   exa_slip_accumulate  one committed step of size dt >= 0: with g_a = EXA_F_SHEARRATE + a, n_a = R(q) m_a (R = quat_to_mat of EXA_F_ORIENTATION, crystal ->
 *                        sample; m_a = normals12x3 [12][3], host, normalised here: exa_slip_plane_normals) and sigma_n,a = n_a^T sigma n_a (sigma =
 *                        EXA_F_STRESS): Gamma_a += dt g_a, A_a += dt |g_a|, then Gamma_min_a = min(Gamma_min_a, Gamma_a), Gamma_max_a = max(Gamma_max_a,
 *                        Gamma_a), N_max_a = max(N_max_a, sigma_n,a).  reset != 0 restarts the window in the same pass: Gamma_min_a = Gamma_max_a =
 *                        Gamma_a and N_max_a = sigma_n,a after the update (dt = 0 with reset: the reset alone, Gamma and A keep their bits).
 *   exa_fip_rows         out_dev [E][EXA_NFIP] from the accumulators, read-only on them: FIP_a = (Gamma_max_a - Gamma_min_a) / 2 (1 + k_fs N_max_a /
 *                        sigma_y) without a clamp (k_fs >= 0, sigma_y > 0 in the stress unit of the rows); EXA_FIP_FIP max_a FIP_a, EXA_FIP_SYSTEM the
 *                        smallest a that attains it (as a double), EXA_FIP_SHEARRANGE and EXA_FIP_NORMALSTRESSMAX the half range and N_max of that
 *                        system, EXA_FIP_ACCUMULATEDSLIP sum_a A_a, EXA_FIP_NETSLIPMAX max_a |Gamma_a|.
 *   exa_fip_summary      out7_dev [7] (device) = local sum V, sum V FIP, sum V AccumulatedSlip, max FIP, max ShearRange, max AccumulatedSlip and the
 *                        global id of the element of max FIP as a double (V = EXA_F_VOLUME of fields_dev, fip_dev the rows of exa_fip_rows,
 *                        elem_gid_dev [E] int64 on the device; ties go to the smallest id).  Without rows: zeros, -inf for the maxima, 2^53 for the id.
 *                        Partials per block in the context's scratch, then one block.
 * No atomics, fixed summation orders: every call on the same data gives the same bits.  None of them synchronises. */
enum { EXA_NSLIPACC = 60, EXA_ACC_SLIP = 0, EXA_ACC_ABS = 12, EXA_ACC_MIN = 24, EXA_ACC_MAX = 36, EXA_ACC_NMAX = 48 };
enum { EXA_NFIP = 6, EXA_FIP_FIP = 0, EXA_FIP_SYSTEM = 1, EXA_FIP_SHEARRANGE = 2, EXA_FIP_NORMALSTRESSMAX = 3, EXA_FIP_ACCUMULATEDSLIP = 4, EXA_FIP_NETSLIPMAX = 5 };
int exa_slip_accumulate(exa_ctx* ctx, const double* fields_dev, const double* normals12x3, double dt, int reset, double* acc_dev, exa_stream s);
int exa_fip_rows(exa_ctx* ctx, const double* acc_dev, double k_fs, double sigma_y, double* out_dev, exa_stream s);
int exa_fip_summary(exa_ctx* ctx, const double* fields_dev, const double* fip_dev, const int64_t* elem_gid_dev, double* out7_dev, exa_stream s);
/* host only: doubles of acc_dev for E elements (may be NULL).  Returns 0, or EXA_ERR_ARG for E < 0. */
int exa_slip_activity_sizes(int64_t E, int64_t* acc_doubles);
/* host only: the unit slip-plane normals [12][3] in the crystal frame of the model's 12 systems, in the order of the slip rates: {111} for the FCC
 * models, {110} for the BCC models.  Returns 0, or EXA_ERR_ARG for an unknown model. */
int exa_slip_plane_normals(int model, double* out12x3);
/* private (scratch) bytes per lane of the kernels behind the three calls above in the loaded code object: out8 = { k_slip_accumulate, k_slip_accumulate
 * with the fused reset, k_fip_rows, k_fip_partial, k_fip_reduce, 0, 0, 0 }; returns 0, or -1 without a device */
int exa_fatigue_scratch_bytes(int* out8);
/* volume average  sum_q W detJ val / sum_q W detJ  (src/mechanics_kernels.hpp:19-134); out_host[vdim] (+ volume in out_host[vdim]).
 * Synchronises the stream. */
int exa_vol_avg(exa_ctx* ctx, const double* jacobian_dev, const double* qf_dev, int vdim, int normalise, double* out_host, exa_stream s);

#ifdef __cplusplus
}
#endif
#endif
