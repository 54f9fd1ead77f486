/* exaconstit_driver.h — C entry points of the stand-alone driver inside libexaconstit_hip.so.
 *
 * Run-time surface of the reference's `mechanics -opt options.toml` executable (reference src/mechanics_driver.cpp:112-1022) and
 * of its SystemDriver (reference src/system_driver.hpp:101-143) for callers without MFEM: the `mechanics` binary of this repo,
 * the tests and bench.py.  Multi-GPU: one process per GPU; rank 0 obtains a RCCL unique id (exa_rccl_unique_id), the launcher
 * distributes the 128 bytes (bench.py uses torch.distributed), every rank passes them to exa_driver_create*.
 */
#ifndef EXA_DRIVER_CAPI_H
#define EXA_DRIVER_CAPI_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef struct exa_driver exa_driver;

typedef struct {
   int N;                      /* N^3 elements on the unit cube, p = 1 */
   int bcc;                    /* 0 fcc, 1 bcc */
   int slip;                   /* 0 powervoce, 1 powervocenl, 2 mtsdd */
   int nprops; const double* props; double temp_k;
   const double* quats;        /* (4, N^3) one orientation per element, x fastest */
   int assembly;               /* 0 PA, 1 EA */
   int nrls, jacobi;
   int newton_iter; double newton_rel, newton_abs;
   int krylov_iter; double krylov_rel, krylov_abs;
   int nsteps; const double* dts;
   double vz;                  /* z-velocity of the top face */
   int order;                  /* H1 order p (1 or 2; 0 = 1) */
   int bbar;                   /* 1: B-bar integrator (element assembly only) */
   int nrev; const int* rev_steps;   /* load reversals: the top-face velocity changes sign at these steps (the cyclic schedule of the reference's
                                * voce_full_cyclic.toml: update_steps 11, 31, 51, 71); each one is a boundary-condition change with its corrector solve */
} exa_synth_config;

int exa_rccl_unique_id(void* out128);
/* the id rank 0 hands to a group of nranks: a RCCL unique id, or the id of the inter-process shared-device transport when RCCL cannot serve
 * the launch (more ranks than visible devices - RCCL refuses two ranks on one device - or EXA_TRANSPORT=ipc).  bench.py and exa_bootstrap use it. */
int exa_comm_unique_id(void* out128, int nranks);
/* PCI bus id of the current device ("0000:c1:00.0"): lets a launcher tell one rank per physical GPU from several ranks on one GPU */
int exa_device_identity(char* out, int len);
/* out2 = { rank count the transport itself reports (ncclCommCount for RCCL), kind: 0 none, 1 rccl, 2 ipc, 3 in-process loopback } */
int exa_driver_comm_info(exa_driver* d, int* out2);
/* out8 = { local elements, elements in 64-blocks that touch shared nodes, neighbour ranks, doubles sent (= received) per halo exchange,
 *          halo exchange overlapped with the interior blocks (0 / 1; over RCCL opt-in with EXA_HALO_OVERLAP=on), transport kind, ranks the
 *          transport reports, 0 } - what bench.py prints per rank of a multi-rank run */
int exa_driver_comm_details(exa_driver* d, int64_t* out8);
/* The transport on its own, for the tests; in place, every rank of the group calls it.  what 0 / 1 / 2: all-reduce (sum / min / max) of n host
 * doubles on the driver's stream; what 3: halo sum of a host L-vector of the local dofs (n = exa_driver_local_dofs, dof = node + local nodes * component) */
int exa_driver_comm_probe(exa_driver* d, int what, double* host_vec, int n);
/* host only: the rank-ordered fold every host-synchronous reduction uses - out[i] = ((c[0][i] op c[1][i]) op c[2][i]) ..., a left fold from rank 0 over
 * contributions[nranks][n]; op 0 sum, 1 min, 2 max.  Returns 0, or -1 for another op or nranks < 1 */
int exa_comm_rank_fold(int op, int nranks, int n, const double* contributions, double* out);
/* host only: which kernels an operator would run for these facts under the EXA_* switches of the environment as it is now (host/routes.hpp).
 * facts[10] = { geometry (0 hexahedra, 1 tetrahedra), order, B-bar, element assembly, slip family (0 Voce, 1 Voce NL, 2 Kocks-Mecking), several ranks,
 *               the transport is RCCL, the partition has boundary blocks (E_bdr > 0), it has neighbours, it is periodic }
 * out[23]   = { fused p = 1 kernels, L-vector action, L-vector residual, compact tangent form, records from the constitutive launch, no Jacobian field,
 *               fused tetrahedron action, its geometry from the coordinates, this rank's wish for the overlapped halo exchange, cap controller,
 *               element-blocked layout, lean state, matrix-free EA, deterministic, deterministic on the E-vector route, GetGradient hands the coordinates
 *               to the tangent-field action, first cap, second cap, resumed tail, tail cost weight in tenths, action route (exa_driver_mesh_info),
 *               EXA_NFEV_LOG, EXA_MODEL_TIMES }
 * ("several ranks" changes no field: with several ranks the live flag of the overlapped exchange is the agreement of all ranks' wishes.)
 * Returns 23, or -1 for nfacts != 10, nout < 23 or facts an operator refuses (geometry, slip family, order < 1, B-bar on tetrahedra) */
int exa_operator_routes_query(const int* facts, int nfacts, int* out, int nout);
/* latency floor of the RCCL calls of one PCG iteration on this device (one-rank communicator): out2 = { us per 16-byte all-reduce,
 * us per grouped send/recv of n doubles to the own rank } */
int exa_rccl_microbench(int iters, int n, double* out2, char* err, int errlen);
/* Launcher-agnostic process-group bootstrap of the `mechanics` executable (reference: MPI_Init / MPI_Comm_rank / MPI_Comm_size,
 * src/mechanics_driver.cpp:119-150).  exa_bootstrap_env reads rank / size / local rank from the environment of mpirun (MPICH PMI_*,
 * Open MPI OMPI_COMM_WORLD_*), srun (SLURM_*), torchrun-style launchers (RANK / WORLD_SIZE / LOCAL_RANK) or EXA_RANK / EXA_NRANKS;
 * exa_bootstrap_bcast copies rank 0's buffer to every rank over a TCP rendez-vous on [EXA_]MASTER_ADDR:[EXA_]MASTER_PORT (default
 * 127.0.0.1:29517); exa_bootstrap = both + device selection (local rank mod visible devices) + the RCCL unique id in uid128. */
int exa_bootstrap_env(int* rank, int* nranks, int* local_rank);
int exa_bootstrap_bcast(int rank, int nranks, void* buf, int nbytes, double timeout_s, char* err, int errlen);
/* The rendez-vous in its general form: every rank contributes nbytes, rank 0 turns the table of all contributions (rank order) into the
 * reply every rank receives (fn runs on rank 0 only; 0 = ok).  exa_bootstrap uses it to decide the transport from the IDENTITY of the
 * ranks' devices (host name + PCI bus id): RCCL when every rank has a GPU of its own - on one node or several -, the shared-device
 * inter-process transport only when ranks of ONE host share a device; ranks that share a device across hosts cannot exist, and the
 * shared-device transport is refused for a group that spans hosts. */
typedef int (*exa_bootstrap_reply_fn)(const void* all, int nranks, int nbytes, void* reply, int reply_bytes, void* user);
int exa_bootstrap_gather_reply(int rank, int nranks, const void* mine, int nbytes, void* reply, int reply_bytes, exa_bootstrap_reply_fn fn, void* user,
                               double timeout_s, char* err, int errlen);
/* the decision itself, exposed for the tests: ids = nranks records of 96 bytes (host name[64], PCI bus id[32], zero padded);
 * returns 1 = RCCL, 2 = shared-device transport, -1 = impossible (reason in err) - EXA_TRANSPORT=rccl|ipc overrides where it can */
int exa_transport_from_identities(const void* ids, int nranks, char* err, int errlen);
int exa_bootstrap(int* rank, int* nranks, void* uid128, char* err, int errlen);
/* Test transport: `nranks` drivers on ONE device, one host thread each, exchanging through an in-process group instead of RCCL
 * (RCCL refuses two ranks on one device).  Pass the 128 bytes as the unique id of every rank; destroy after the drivers. */
int exa_loopback_group_create(int nranks, void* out128);
void exa_loopback_group_destroy(const void* id128);
exa_driver* exa_driver_create(const char* toml_path, const char* out_dir, int rank, int nranks, const void* uid, int jacobi, int write_files, char* err, int errlen);
exa_driver* exa_driver_create_synthetic(const exa_synth_config* c, int rank, int nranks, const void* uid, char* err, int errlen);
/* Checkpoint and restart.  A checkpoint is one self-describing file that does not depend on the decomposition, the quadrature
 * layout or the rank count: a run resumes from it on any number of ranks.  Every rank of the group calls save / load.
 *   exa_driver_save_checkpoint  writes <path>.tmp and renames it, so an interrupted write leaves the previous checkpoint intact
 *   exa_driver_load_checkpoint  legal only on a freshly created driver before its first step; a file of another mesh, order, geometry, model,
 *                               property set or grain map, a truncated file and a checksum mismatch are refused with a message that names the
 *                               mismatch; the avg_* and light-up files are rewritten from the stored rows; exa_driver_run continues at the
 *                               step after the stored one.  Nothing of the driver is changed before every section's checksum has been
 *                               verified: after a refused load (-1) the driver is still the freshly created one and may load another file
 *                               or run from the start
 *   exa_driver_create_restart   exa_driver_create + load: restart_path NULL = Checkpoint.restart_from of the options file (if any),
 *                               "" = no restart, otherwise the checkpoint to resume from
 *   exa_checkpoint_info         header and section table only, no GPU needed: out20 = { version, global elements, global nodes, points per element,
 *                               geometry, order, model, nprops, nstatev, steps_done, BC entry in force, writer's rank count, flags, sections,
 *                               model_calls, newton_cap, newton_cap2, writer, 0, 0 }, outd3 = { time, dt_class, last_dt }, hashes3 = { property,
 *                               grain-map, connectivity hash }, sec_names = 24 bytes per section, sec_info = { offset, nbytes, checksum } per
 *                               section (any of them may be NULL); returns the number of sections or -1 (err) */
exa_driver* exa_driver_create_restart(const char* toml_path, const char* out_dir, int rank, int nranks, const void* uid, int jacobi, int write_files,
                                      const char* restart_path, char* err, int errlen);
int exa_driver_save_checkpoint(exa_driver* d, const char* path, char* err, int errlen);
int exa_driver_load_checkpoint(exa_driver* d, const char* path, char* err, int errlen);
int exa_checkpoint_info(const char* path, int64_t* out20, double* outd3, uint64_t* hashes3, char* sec_names, uint64_t* sec_info, int max_sections, char* err, int errlen);
void exa_driver_destroy(exa_driver* d);
/* Preconditioner of the PCG (Solvers.Krylov.preconditioner in an options file; this call overrides it), valid before the first step (so
 * synthetic and exa_driver_bench_prepare'd drivers can use it): kind 0 identity, 1 Jacobi, 2 geometric multigrid V-cycle (generated p = 1
 * meshes, p = 2 after exa_driver_set_mg_p2, B-bar after exa_driver_set_mg_bbar) with at most `levels` coarse levels (0: as many as the mesh allows) and a Chebyshev smoother of `degree` (1 ... 8).
 * Refused (-1, err) where no coarse level can be built for the decomposition. */
int exa_driver_set_preconditioner(exa_driver* d, int kind, int levels, int degree, char* err, int errlen);
/* out (>= 6 + 4 (L + 1) doubles) = { coarse levels L, ms of the last hierarchy set-up, ms of the last V-cycle, smoother degree, then per level
 * l = 0 ... L: local elements per direction (3), lmax estimate of D^-1 A_l; then 1 on a periodic cell, the free control entries of mixed loading
 * in the preconditioner's control block }.  Returns 0 or -1 (no multigrid preconditioner). */
int exa_driver_mg_info(exa_driver* d, double* out);
/* Multigrid on a periodic cell is opt-in ([Solvers.Krylov] mg_periodic = true in an options file): on != 0 before exa_driver_set_preconditioner(2) /
 * exa_driver_set_periodic lets the two meet, in either order; without it either call refuses the other, as before.  Returns 0. */
int exa_driver_set_mg_periodic(exa_driver* d, int on);
/* Multigrid at p_refinement = 2 is opt-in ([Solvers.Krylov] mg_p2 = true): on != 0 before exa_driver_set_preconditioner(2) makes a generated
 * p = 2 mesh legal (level 1 = the trilinear space on the element vertices); without it the call refuses p = 2 as before.  B-bar, file and
 * tetrahedral meshes, p >= 3 and periodic cells at p = 2 stay refused.  Returns 0. */
int exa_driver_set_mg_p2(exa_driver* d, int on);
/* Multigrid under integ_model = "BBAR" is opt-in ([Solvers.Krylov] mg_bbar = true): on != 0 before exa_driver_set_preconditioner(2) makes a B-bar
 * run on a generated mesh legal at p = 1, and at p = 2 together with exa_driver_set_mg_p2; without it the call refuses B-bar as before.  The key
 * permits, it does not require: a FULL run is not changed by it.  Periodic cells stay refused under B-bar multigrid (either call order, with or
 * without exa_driver_set_mg_periodic), and so does everything multigrid refuses without B-bar.  Returns 0. */
int exa_driver_set_mg_bbar(exa_driver* d, int on);
/* How the p = 2 hierarchy builds level 1 and the fine diagonal from the next set-up on: 1 (default) from the point records in one pass each
 * (exa_grad_mg_p2_build) where the action runs from records and the essential set is closed under the interpolation, by probing otherwise;
 * 0 always by probing (what the tests compare the records build against).  Returns 0. */
int exa_driver_set_mg_p2_build(exa_driver* d, int from_records);
/* out (>= 2 + L + 1 ints) = { coarse levels L, level-1 build of the last set-up (0 probe, 1 records; -1 before the first set-up or at p = 1),
 * then the polynomial order of every level l = 0 ... L }.  Returns 0 or -1 (no multigrid preconditioner). */
int exa_driver_mg_info_order(exa_driver* d, int* out);
/* 1 where the hierarchy stands on the B-bar operator (exa_driver_set_mg_bbar), 0 otherwise; -1 (no multigrid preconditioner) */
int exa_driver_mg_bbar(exa_driver* d);
/* Test hooks on the hierarchy of the last gradient set-up; host arrays of exa_driver_mg_level_dofs(level) doubles (node-major per component,
 * node = i + n0 (j + n1 k) of the rank's local box at that level).  Level 0 is the constrained operator the PCG applies. */
int64_t exa_driver_mg_level_dofs(exa_driver* d, int level);
/* gradient set-up of the current state and the hierarchy build after it: a residual evaluation after the last set-up (the one that ends a
 * Newton solve) renews the fine operator, this makes the hierarchy match it again */
int exa_driver_mg_setup(exa_driver* d, char* err, int errlen);
int exa_driver_mg_apply(exa_driver* d, int level, const double* x, double* y);
int exa_driver_mg_diag(exa_driver* d, int level, double* out);
/* dir 0: out (level l) = P_{l+1} in (level l + 1), trilinear interpolation; dir 1: out (level l + 1) = restriction of in (level l) */
int exa_driver_mg_transfer(exa_driver* d, int level, int dir, const double* in, double* out);
/* stored coarse operator of level >= 1: 243 doubles per node, [(o * 9 + 3 r + c) * NN + node], o = (dx+1) + 3 (dy+1) + 9 (dz+1) */
int exa_driver_mg_stencil(exa_driver* d, int level, double* out);
/* z = B r: one application of the multigrid preconditioner (level-0 sized host arrays) */
int exa_driver_precond_apply(exa_driver* d, const double* r, double* z);
int exa_driver_num_steps(exa_driver* d);
int64_t exa_driver_local_qpts(exa_driver* d);
/* out8 = { element geometry (EXA_GEOM_HEX 0 / EXA_GEOM_TET 1), H1 order, nodes per element, quadrature points per element, local elements,
 *          local nodes, route of the Krylov action (0 hexahedron kernels, 1 fused tetrahedron action, 2 table-driven E-vector action,
 *          3 table-driven element-assembly action on L-vectors), 0 } */
int exa_driver_mesh_info(exa_driver* d, int64_t* out8);
int64_t exa_driver_local_dofs(exa_driver* d);
int exa_driver_step(exa_driver* d, int ti, char* err, int errlen);
/* solve step ti but do not commit it (no begin/end swap, no coordinate update, no output row): the state bench.py times its passes on */
int exa_driver_step_nocommit(exa_driver* d, int ti, char* err, int errlen);
/* end-of-step update of a step solved by exa_driver_step_nocommit, valid while only residual evaluations at the converged velocity
 * (exa_driver_bench_model / exa_driver_bench_pcg) have run since */
int exa_driver_commit_step(exa_driver* d, char* err, int errlen);
int exa_driver_run(exa_driver* d, char* err, int errlen);
int exa_driver_get_avgs(exa_driver* d, int which, double* out, int maxrows);
int exa_driver_get_stats(exa_driver* d, int* newton, int* krylov, int* model_calls, int maxrows);
void exa_driver_get_timers(exa_driver* d, double* out5);
void exa_driver_reset_timers(exa_driver* d);
/* Solver diagnostics the reference prints or aborts on: out4[0] quadrature points whose ExaCMech solve did not converge (the
 * library's ECMECH_FAIL; here Newton reports non-convergence), [1] PCG solves without convergence, [2] PCG iterations with
 * (Ad, d) < 0 (MFEM: "The operator is not positive definite"), [3] flag of the last PCG solve (1 ok, 2 max_iter, -1 (Ad, d) = 0). */
void exa_driver_get_diagnostics(exa_driver* d, int64_t* out4);
/* Launches of exa_slip_rates_from_state so far.  The driver's element-blocked record launches leave a lean end-of-step state (include/exaconstit_hip.h,
 * exa_set_lean_state; EXA_LEAN_STATE=off at creation: the full state) and the 12 slip rates are written when a reader of state slots 14..25 asks:
 * the additional averages, the element fields, a checkpoint, exa_driver_get_qf_component of those slots.  A run that asks for none of them stays at 0. */
int64_t exa_driver_get_rate_launches(exa_driver* d);
/* p = 1 record launches of the driver's context so far (include/exaconstit_hip.h, exa_model_record_launches): out2[0] through the entry without tail-split
 * arguments, out2[1] through the generic kernel; both 0 on the other routes. */
void exa_driver_get_record_launches(exa_driver* d, int64_t* out2);
/* Launches of exa_element_fields so far.  Every analysis of the element rows (fields, lattice strains, grain averages, texture, curvature, slip
 * activity, the ParaView save) takes them from one accessor, which launches only when the rows it holds are not those of the state at hand:
 * analyses asked for in a row on one state share one launch (exa_driver_element_fields itself always launches). */
int64_t exa_driver_get_field_launches(exa_driver* d);
/* Residual reduction |r|_M / |r0|_M the PCG reached: out2[0] last solve, out2[1] the worst among the solves that stopped at max_iter
 * (MFEM's CGSolver prints "No convergence!" with the final norms, linalg/solvers.cpp; the reference's Newton loop goes on regardless). */
void exa_driver_get_pcg_reduction(exa_driver* d, double* out2);
/* 64-bin histogram of the local-solver evaluation counts (ExaCMech's nFEval state variable) of the last constitutive launch */
int exa_driver_nfev_hist(exa_driver* d, int* hist64, char* err, int errlen);
/* the same of the begin-of-step state (which = 0: after a completed step, the launch that step converged with) or the end-of-step state (1) */
int exa_driver_nfev_hist_of(exa_driver* d, int which, int* hist64, char* err, int errlen);
/* one component of a quadrature function of the operator, de-blocked on the host: which = 0 begin-of-step state, 1 end-of-step state (28),
 * 2 begin stress, 3 end stress (6); out receives E * Q doubles ordered [element][point] (diagnostics: nFEval maps, parity tools) */
int exa_driver_get_qf_component(exa_driver* d, int which, int comp, double* out, char* err, int errlen);
/* Per-element output fields of the current begin-of-step state (after a completed step: the converged one) on this rank, without any file:
 * out [E][EXA_NFIELDS] (column table at exa_element_fields, include/exaconstit_hip.h), elem_gid [E] global element index, attribute [E] grain id;
 * every pointer may be NULL.  Local element order of the driver.  Returns E (>= 0) or -1 (err). */
int exa_driver_element_fields(exa_driver* d, double* out, int64_t* elem_gid, int32_t* attribute, char* err, int errlen);
/* ParaView save of those fields on demand: <dir>/Cycle%06d/proc%06d.vtu (every rank), data.pvtu and <dir>/<basename(dir)>.pvd (rank 0; the
 * collection lists the cycles saved to dir through this driver).  Every rank of the group calls it.  Returns 0 or -1 (err). */
int exa_driver_write_fields(exa_driver* d, const char* dir, int cycle, double t, char* err, int errlen);
/* Lattice strains of nhkl (1..16) plane families {hkl} (hkl3: 3 integers each) along the sample direction s_dir3 (normalised here) with fibre
 * tolerance tol_deg in (0, 90], on the current begin-of-step state (after a completed step: the converged one), summed over all ranks (every rank
 * of the group calls it): strain_out[j] = volume-weighted mean of s^T eps s over the elements whose <hkl> lies within tol_deg of s (NaN for an
 * empty fibre), volfrac_out[j] = their volume fraction (exa_lattice_strains, include/exaconstit_hip.h).  Returns 0 or -1 (err). */
int exa_driver_lattice_strains(exa_driver* d, int nhkl, const int* hkl3, const double* s_dir3, double tol_deg, double* strain_out, double* volfrac_out,
                               char* err, int errlen);
/* Per-grain averages of the current begin-of-step state (after a completed step: the converged one), over all ranks (every rank
 * of the group calls it).  Grains are the element attributes (1-based); only grains with elements are reported, in ascending id.  Writes, when
 * the row count n <= cap, grain_ids[n] and vals[n][EXA_GRAIN_NVALS]: n_elements, volume, volume_fraction, Stress (6), VonMisesStress,
 * HydrostaticStress, ElasticStrainSample (6), XtalElasticStrain (6), EffPlasticStrain, DpEff, Hardness, ShearRate (12), LatticeOrientation (4),
 * MisorientationMean, MisorientationMax, GrainRotation (degrees).  Either pointer may be NULL.  Returns n or -1 (err). */
enum { EXA_GRAIN_NVALS = 45 };
int exa_driver_grain_averages(exa_driver* d, int32_t* grain_ids, double* vals, int64_t cap, char* err, int errlen);
/* Intragranular misorientation and lattice curvature of the current begin-of-step state (after a completed step: the converged
 * one); every rank of the group calls it.  Grains are the element attributes and their means the LatticeOrientation of exa_driver_grain_averages;
 * the nodal recovery sums over the ranks and, on a periodic cell, over the periodic images of a node.  burgers > 0: Burgers vector length in the
 * mesh's length unit.  out [E][EXA_NCURV] (column table at exa_curvature_elements, include/exaconstit_hip.h) in the local element order of the
 * driver, elem_gid [E] and attribute [E] as exa_driver_element_fields; summary7 (all ranks) = { mean GROD, max GROD, mean KAM, max KAM (degrees),
 * mean GNDDensity, max GNDDensity, total volume }, means weighted by element volume.  Every pointer may be NULL (all NULL: no launch, the row
 * count only).  Returns E (>= 0) or -1 (err). */
int exa_driver_lattice_curvature(exa_driver* d, double burgers, double* out, int64_t* elem_gid, int32_t* attribute, double* summary7, char* err, int errlen);
/* Grain map of a synthetic driver (exa_driver_create_synthetic), before its first step: grain_of_global_element[n_global] in 1..G (n_global =
 * N^3, global element index x fastest) and grain_quats[G][4] (scalar first, normalised here).  Every element's initial orientation and state
 * become its grain's, and the grain's orientation is its reference q_ref.  Every rank of the group calls it with the same map.  Returns 0 or -1 (err). */
int exa_driver_set_grains(exa_driver* d, const int32_t* grain_of_global_element, const double* grain_quats, int G, int64_t n_global, char* err, int errlen);
/* Texture of the current begin-of-step state (after a completed step: the converged one), over all ranks (every rank of the group
 * calls it): pole figures of the nhkl families hkl3 [nhkl][3] and inverse pole figures of the ndir sample directions dirs3 [ndir][3] (normalised
 * here) on the grid of res_deg (exa_texture_grid), in multiples of random distribution: mrd_out [nhkl + ndir][n_alpha][n_beta] receives
 * MRD_ik = (W_ik / W_tot) 2 pi / dOmega_i, dOmega_i = res (cos i res - cos (i + 1) res) (res in radians), from the integer weights of
 * exa_texture_weights summed exactly over the ranks: the same bits for any rank count.  0 <= nhkl <= 16, 0 <= ndir <= 3, nhkl + ndir >= 1.
 * Returns 0 or -1 (err). */
int exa_driver_pole_figures(exa_driver* d, int nhkl, const int* hkl3, int ndir, const double* dirs3, double res_deg, double* mrd_out, char* err, int errlen);
/* Periodic boundary conditions in all three directions under the macroscopic velocity gradient vel_grad9 (row by row), on a freshly
 * created driver before its first step - also one made by exa_driver_create_synthetic, whose prescribed faces it replaces: the velocity satisfies
 * v(image) - v(node) = L (x(image) - x(node)) between the images of a surface node, the eight corners carry v = L (x - origin).  Rebuilds the
 * partition tables, weights, essential set and halo lists; every rank of the group calls it.  Refuses meshes read from a file and, unless
 * exa_driver_set_mg_periodic allowed it, the multigrid preconditioner, like the options reader ([BCs] periodic = true); a multigrid hierarchy
 * that exists already is made again for the periodic partition.  Returns 0 or -1 (err). */
int exa_driver_set_periodic(exa_driver* d, const double* vel_grad9, char* err, int errlen);
/* Mixed stress / velocity-gradient loading of a periodic cell: like exa_driver_set_periodic, with free9[3 i + d] != 0 making entry
 * (i, d) of the velocity gradient an unknown whose conjugate mean traction (component i on face pair d) is zero; the other entries stay
 * prescribed at vel_grad9, the free ones start from it.  Refused: both entries of an off-diagonal pair free, all nine free.  free9 NULL or all
 * zero is exa_driver_set_periodic.  Returns 0 or -1 (err). */
int exa_driver_set_periodic_mixed(exa_driver* d, const double* vel_grad9, const int* free9, char* err, int errlen);
/* free9 = the mask; vel_grad9 = the gradient H A^-1 the last solved step realised (zeros before it); period9 = the period vectors at the start of
 * that step (column d = a_d, row by row); resultants9 = the face resultants F_id of the last converged residual (row by row, summed over the
 * ranks).  Returns 1 with mixed loading on, 0 without it (all outputs zero), -1 on error. */
int exa_driver_macro_info(exa_driver* d, int* free9, double* vel_grad9, double* period9, double* resultants9);
/* Homogenised tangent d sigma_bar / d L_bar of the last solved step of a periodic cell: nine fluctuation solves with the operator, the
 * periodic sum and the PCG of the step, then dsig81[9 (3 k + l) + (3 m + n)] = d sigma_bar_kl / d L_bar_mn by Hill-Mandel.  rel_tol / max_iter <= 0:
 * the Krylov options.  batched: -1 the automatic route, 0 column by column, 1 the nine columns in lockstep through exa_grad_apply_lvec_cols (one
 * rank, non-deterministic mode, p = 1 hexahedron L-vector record action; refused elsewhere).  out2 = { current cell volume V, dt }.  info (9 x 6,
 * may be NULL): per column { PCG iterations, solver flag (1 converged, 2 max_iter, -1 breakdown), the solver's own reduction, |b_m|, the TRUE residual
 * |b_m - K_uu w_m| recomputed by one more action, max |w_m| / max |a_m| }.  route2 (may be NULL) = { batched, columns per pass }.  Refused: a driver
 * that is not periodic; a driver without a step solved in this process (a freshly restarted one included).  The run is left as it was: essential
 * mask, PCG scalars and captured graph, records, timers, Newton cap state, statistics.  Every rank calls it.  Returns 0 or -1 (err). */
int exa_driver_macro_tangent(exa_driver* d, double rel_tol, int max_iter, int batched, double* dsig81, double* out2, double* info, int* route2, char* err, int errlen);
/* Probe of the operator behind the tangent (cf. exa_driver_mg_apply): y_m = K x_m for ncols <= 16 host columns of local dofs, byNODES (dof = node +
 * local nodes * component), column m at m * local dofs.  flags bit 0: assembled and masked - the operator K_uu of the tangent's solves (periodic and
 * rank sums; the run's essential set plus the control slots) - instead of the raw element action; bit 1: batched instead of one by one.  gated (may
 * be NULL): columns with a non-zero entry are left out and keep the y passed in.  nch: 1 .. 3 columns per pass of the batched route from now on
 * (0: unchanged).  Needs a solved step. */
int exa_driver_grad_apply_columns(exa_driver* d, int ncols, const double* x, double* y, int flags, const int* gated, int nch, char* err, int errlen);
/* Probe of the linear solver next to the one of its operator: K_uu x_m = b_m from x = 0 for nrhs <= 16 host columns of local dofs (byNODES, column m at
 * m * local dofs), K_uu the assembled, masked operator of exa_driver_grad_apply_columns (flags bit 0), in a PCG solver of the probe's own: the run's
 * settings with rel_tol, abs_tol, max_iter, check_every (0: the run's) and graph (-1: replay of captured chunks as the run decides, 0: never, 1: at any
 * size).  mode 0: the single-system solve for each column in turn, into one fixed device buffer by one solver object; mode 1: all columns in lockstep
 * (columns per pass: exa_driver_set_tangent_route).  Per column: x, iterations, flag (1 converged, 2 max_iter, -1 breakdown), the solver's own
 * reduction sqrt((r, z) / (r0, z0)), iterations that saw (Ad, d) < 0, scalars2[2 m] = (r0, z0), scalars2[2 m + 1] = the last (r, z).  Needs a solved
 * step; every rank calls it.  The run's solver, captured chunk, diagnostics and totals are not touched. */
int exa_driver_pcg_solve(exa_driver* d, int nrhs, const double* b, double rel_tol, double abs_tol, int max_iter, int check_every, int graph, int mode, double* x, int* iters,
                         int* flags, double* reduction, int* indefinite, double* scalars2, char* err, int errlen);
/* The run's linear solver: solver "pcg" or "gmres" (any case), kdim the Krylov dimension of restarted GMRES (1 ... 100, MFEM's default
 * is 50; ignored for PCG).  Legal before the first step and between steps; tolerances and cap stay, and the run's diagnostics and totals
 * (exa_driver_get_diagnostics, _get_pcg_reduction, _get_timers) go on counting.  Every rank calls it.  Returns 0 or -1 (err). */
int exa_driver_set_krylov(exa_driver* d, const char* solver, int kdim, char* err, int errlen);
/* out3i = { 0 PCG / 1 GMRES, kdim (0 for PCG), chunk of the multi-dot kernel }; out3 = { restarts, second Gram-Schmidt passes (both over all solves of
 * the run's solver), bytes of the basis (0 before the first GMRES solve) } */
int exa_driver_krylov_info(exa_driver* d, int* out3i, int64_t* out3);
int exa_gmres_multidot_chunk(void);   /* basis vectors per pass of the multi-dot kernel, a compile-time constant (8 ... 16) */
/* Probe of GMRES, mirroring exa_driver_pcg_solve: K_uu x_m = b_m from x = 0 for nrhs <= 16 host columns in turn, in a GMRES(kdim) solver of the probe's
 * own with the run's preconditioner and chunk (check_every 0: the run's).  ortho: -1 as EXA_GMRES_ORTHO says, 0 ifneeded, 1 always, 2 never, 3 mgs.
 * Per column: x, Arnoldi steps, flag (1 converged, 2 max_iter, -1 breakdown), reduction = last residual / beta0, scalars4[4 m ...] = { beta0 = |M^-1 b|,
 * last residual norm, restarts, second Gram-Schmidt passes }.  Needs a solved step; every rank calls it; the run's solver is not touched. */
int exa_driver_gmres_solve(exa_driver* d, int nrhs, const double* b, double rel_tol, double abs_tol, int max_iter, int kdim, int check_every, int ortho, double* x, int* iters,
                           int* flags, double* reduction, double* scalars4, char* err, int errlen);
/* The two bandwidth kernels of the orthogonalisation on any shape (host arrays in and out, one GPU): w (n) against the k <= 100 vectors V (k x n, row j
 * = v_j) in the product weighted by weight (n); flag != 0: the kernels' gate is closed.  mode 0 ifneeded, 1 always, 2 never, 3 mgs.  h (k): the column
 * of H; w_out (n); wnorm2 = |w_out|^2 from the partial sums of the subtraction kernel; passes: 0 with the gate closed, else 1 + second passes. */
int exa_gmres_ortho_probe(int64_t n, int k, const double* weight, const double* V, const double* w, double flag, int mode, double* h, double* w_out, double* wnorm2,
                          int* passes, char* err, int errlen);
/* measurement hook of scripts/gmres_compare.py, no part of a run (as exa_driver_bench_pcg is for bench.py): timing of the same launches on device
 * buffers of the call's own, ms per orthogonalisation and normalisation of column col (col + 1 basis vectors of n
 * entries), the mean of reps back-to-back repetitions after two warm-up ones */
int exa_gmres_ortho_bench(int64_t n, int col, int mode, int reps, double* ms, char* err, int errlen);
/* Host only, no GPU call: the small algebra of the scalar kernel.  Hbar: ncols <= 100 columns at leading dimension ncols + 1, column i holding
 * h_0i ... h_i+1,i as Gram-Schmidt leaves them; beta: the first residual norm.  resid (ncols): |s_i+1| after column i; flags (ncols): what the solver
 * decides after that column with the bound final_norm and no iteration cap (0 running, 1 converged, -1 breakdown); y (ncols): the back-substitution
 * over all columns.  Returns 1, 0 when the back-substitution met a zero pivot (those y_i are 0), -1 on a bad ncols. */
int exa_gmres_column_probe(int ncols, const double* Hbar, double beta, double final_norm, double* resid, int* flags, double* y);
/* columns per pass of the batched route (1 .. 3, 0: the default) and whether the automatic route takes it where it exists */
int exa_driver_set_tangent_route(exa_driver* d, int nch, int auto_batched);
/* host only: the condensed tangent of the prescribed entries, C_pp - C_pf C_ff^-1 C_fp, of the 9 x 9 c81[9 (kl) + (mn)] for the free mask of a mixed
 * run (row by row); zeros in the free rows and columns.  0, or -1 when C_ff is singular. */
int exa_macro_tangent_condense(const double* c81, const int* free9, double* out81);
/* [Visualizations] macro_tangent, macro_tangent_max_iter -> out2; macro_tangent_rel_tol; macro_tangent_fname (0: the Solvers.Krylov value) */
int exa_options_macro_tangent(const char* toml_path, int* out2, double* rel_tol, char* fname, int fnamelen, char* err, int errlen);
/* private (scratch) bytes per lane of k_periodic_expand and k_face_resultants in the loaded code object: out2; returns 0, or -1 without a device */
int exa_periodic_mixed_scratch_bytes(int* out2);
/* the same of the multigrid kernels of a periodic cell on one rank: out2 = { k_mg_stencil_apply_periodic, k_mg_restrict_periodic } */
int exa_mg_periodic_scratch_bytes(int* out2);
/* out8 = { periodic (0 / 1), local periodic groups of 2, of 4, of 8 images, canonical ids exchanged with other ranks, neighbours, 0, 0 };
 * vel_grad9 = the macroscopic velocity gradient in force (zeros when the driver is not periodic).  Returns 0 or -1. */
int exa_driver_periodic_info(exa_driver* d, int64_t* out8, double* vel_grad9);
/* private (scratch) bytes per lane of k_periodic_sum in the loaded code object (the launch that follows every periodic operator action); -1 without a device */
int exa_periodic_sum_scratch_bytes(void);
/* A nodal field of this rank: which = 0 velocity, 1 current coordinates (after a completed step: its end), 2 reference coordinates; out
 * [local nodes][3] or NULL.  Row g belongs to the node exa_partition_query_nodes numbers node_gid[g].  Returns the local node count or -1 (err). */
int exa_driver_get_nodal(exa_driver* d, int which, double* out, char* err, int errlen);
/* out2 = { residual norm the last Newton solve of the last step ended with, its bound max(rel_tol |r0|, abs_tol) }.  Returns 0. */
int exa_driver_newton_info(exa_driver* d, double* out2);
int exa_driver_bench_prepare(exa_driver* d, int nsteps, const double* dts, double perturb, char* err, int errlen);
int exa_driver_bench_model(exa_driver* d, int steps, double* out3, char* err, int errlen);
int exa_driver_bench_pcg(exa_driver* d, int iters, double* out3, char* err, int errlen);
/* the drop-in route (the calls of include/exaconstit_mfem_adapters.hpp: AOS exa_model_setup, exa_grad_setup, E-vector exa_grad_apply between the element
 * restriction and its transpose - and the L-vector pair's exa_model_setup_lvec / exa_grad_apply_lvec) timed on a second context that is given this driver's state;
 * out24 documented at the definition (host/driver_capi.hip) */
int exa_driver_bench_adapter_route(exa_driver* d, int steps, int iters, double* out24, char* err, int errlen);

/* host-logic queries that need no GPU (used by the CPU tests) ------------------------------------------------------------ */
/* options.toml reader (reference src/option_parser.cpp:26-932): fills out[0..19] =
 * {temp_k, nprops, num_grains, xtal, slip, dt_cust, dt_auto, nsteps, assembly(0 PA,1 EA), nl_solver(0 NR,1 NRLS), newton_iter, newton_rel,
 *  newton_abs, krylov_iter, krylov_rel, krylov_abs, ref_ser, ncuts0, additional_avgs, number of BC change steps}; returns 0 or -1 (err) */
int exa_options_query(const char* toml_path, double* out20, char* err, int errlen);
/* [BCs] table: out2 = { periodic (default 0), boundary-condition entries }, vel_grad = essential_vel_grad of every entry (9 values each, row by
 * row; at most max_entries entries are copied; may be NULL); returns 0 or -1 (err) */
int exa_options_query_bcs(const char* toml_path, int* out2, double* vel_grad, int max_entries, char* err, int errlen);
/* Solvers.Krylov keys of the multigrid preconditioner: out3 = { 0 key absent (the jacobi flag of exa_driver_create decides), 1 "jacobi",
 * 2 "multigrid"; mg_levels (default 0 = as many as the mesh allows); mg_smoother_degree (default 2) }; returns 0 or -1 (err) */
int exa_options_query_solver(const char* toml_path, int* out3, char* err, int errlen);
/* number of coarse multigrid levels of an N0 x N1 x N2 element grid on nranks block ranks (0: multigrid refused), capped by cap > 0 */
int exa_mg_level_count(const int* N, int nranks, int cap);
/* ... at polynomial order 1 (the same) or 2: one more level, the element vertices, which needs no evenness (never 0); -1 for other orders */
int exa_mg_level_count_order(const int* N, int nranks, int cap, int order);
/* [Solvers.Krylov] mg_p2 of an options file (0 / 1; read next to preconditioner = "multigrid" only); returns 0 or -1 (err) */
int exa_options_query_mg_p2(const char* toml_path, int* out1, char* err, int errlen);
/* [Solvers.Krylov] mg_bbar of an options file, likewise */
int exa_options_query_mg_bbar(const char* toml_path, int* out1, char* err, int errlen);
/* Visualizations table (reference src/option_parser.cpp:540-570): paraview (default 0), steps (1), light_up (0), floc ("results/exaconstit",
 * relative to the driver's output directory); returns 0 or -1 (err) */
int exa_options_query_vis(const char* toml_path, int* paraview, int* steps, int* light_up, char* floc, int floclen, char* err, int errlen);
/* light-up analysis keys of the Visualizations table: enabled = light_up and light_up_hkl given; nhkl families in hkl48 (3 integers each, room for
 * 48); s_dir3 the normalised light_up_s_dir (default 0 0 1); tol_deg light_up_dist_tol_deg (5); light_up_strain_fname ("lattice_strains.txt") and
 * light_up_volume_fname ("lattice_volumes.txt") into buffers of fnamelen bytes.  Every pointer may be NULL.  Returns 0 or -1 (err). */
int exa_options_query_lightup(const char* toml_path, int* enabled, int* nhkl, int* hkl48, double* s_dir3, double* tol_deg, char* strain_fname,
                              char* volume_fname, int fnamelen, char* err, int errlen);
/* per-grain averages keys of the Visualizations table: enabled = grain_avgs (default 0), grain_avgs_fname ("grain_avgs") into a buffer of
 * fnamelen bytes.  Either pointer may be NULL.  Returns 0 or -1 (err). */
/* texture keys of the Visualizations table: enabled = texture (default 0); texture_hkl (default [[1,1,1],[2,0,0],[2,2,0]]) as *nhkl triples
 * into hkl48; texture_ipf_dirs (default [[0,0,1]]), normalised, as *ndir directions into dirs9; texture_res_deg (5); texture_fname ("texture")
 * into a buffer of fnamelen bytes.  Every pointer may be NULL.  Returns 0 or -1 (err). */
int exa_options_query_texture(const char* toml_path, int* enabled, int* nhkl, int* hkl48, int* ndir, double* dirs9, double* res_deg, char* fname, int fnamelen,
                              char* err, int errlen);
int exa_options_query_grains(const char* toml_path, int* enabled, char* fname, int fnamelen, char* err, int errlen);
/* lattice-curvature keys of the Visualizations table: enabled = lattice_curvature (default 0), burgers = lattice_curvature_burgers (1.0; refused
 * unless > 0), lattice_curvature_fname ("lattice_curvature.txt"; refused if empty or with a '/') into a buffer of fnamelen bytes.  Every pointer
 * may be NULL.  Returns 0 or -1 (err). */
int exa_options_query_lattice_curvature(const char* toml_path, int* enabled, double* burgers, char* fname, int fnamelen, char* err, int errlen);
/* fatigue keys of the Visualizations table: out2 = { fatigue (default 0), fatigue_cycle_steps (0; refused if < 0) }, out2d = { fatigue_k (0.5;
 * refused if < 0), fatigue_sigma_y (0 when absent; refused unless > 0, and required with fatigue = true) }, fatigue_fname ("fatigue.txt"; refused if empty or
 * with a '/') into a buffer of fnamelen bytes.  Every pointer may be NULL.  Returns 0 or -1 (err). */
int exa_options_query_fatigue(const char* toml_path, int* out2, double* out2d, char* fname, int fnamelen, char* err, int errlen);
/* Slip-system activity and the Fatemi-Socie fatigue indicator parameter of a run (kernels: exa_slip_accumulate, exa_fip_rows, exa_fip_summary of
 * exaconstit_hip.h).  exa_driver_enable_slip_activity switches the accumulators on before the first step (an options file does with Visualizations.fatigue):
 * every committed step then adds itself, whether committed by exa_driver_step or by exa_driver_commit_step.  exa_driver_reset_fatigue_window asks for a new
 * window: it starts with the next committed step (before step 1 the window is the initial state already).  exa_driver_slip_activity evaluates the committed
 * state with k_fs >= 0 and sigma_y > 0, read-only on the accumulators; every rank of a group calls it with the same pointers NULL.  acc_out [E][60] (Gamma,
 * A, Gamma_min, Gamma_max, N_max, 12 systems each) and fip_out [E][EXA_NFIP] of the local elements in local order, elem_gid / attribute as
 * exa_driver_element_fields; summary8 = over all ranks { volume, mean FIP, max FIP, global element of the max (ties: the smallest), mean AccumulatedSlip, max
 * AccumulatedSlip, max ShearRange, first step of the window }; per grain with elements over all ranks, ascending id: grain_ids and grain_vals3 [.][3] =
 * volume, volume-weighted mean FIP, max FIP, copied when their count *n_grains <= grain_cap.  All outputs NULL: no evaluation.  Returns E or -1 (err). */
int exa_driver_enable_slip_activity(exa_driver* d, char* err, int errlen);
int exa_driver_reset_fatigue_window(exa_driver* d, char* err, int errlen);
int exa_driver_slip_activity(exa_driver* d, double k_fs, double sigma_y, double* acc_out, double* fip_out, int64_t* elem_gid, int32_t* attribute, double* summary8,
                             int32_t* grain_ids, double* grain_vals3, int64_t grain_cap, int64_t* n_grains, char* err, int errlen);
/* the writers of the fatigue files (host only).  exa_fatigue_write: nrows rows of 9 doubles { step, time, first step of the window, mean FIP, max FIP, global
 * element of the max, mean AccumulatedSlip, max AccumulatedSlip, max ShearRange } (the three counts as integers, the rest with 17 significant digits); append = 0
 * starts the file anew with its '#' header, otherwise the rows are appended.  exa_fatigue_grains_write: a '#' header and n rows grain id, volume, mean FIP, max FIP.
 * Return 0 or -1 (err). */
int exa_fatigue_write(const char* path, int nrows, const double* rows9, int append, char* err, int errlen);
int exa_fatigue_grains_write(const char* path, int n, const int32_t* grain_ids, const double* vals3, char* err, int errlen);
/* [Checkpoint] table (all keys optional): out3 = { write (default 0), steps (1), keep (2) }, floc (default "checkpoint"), restart_from (default "") */
int exa_options_query_checkpoint(const char* toml_path, int* out3, char* floc, int floclen, char* restart_from, int restartlen, char* err, int errlen);
/* the grain_avgs file writer (host only): a '#' header naming the 46 columns, then n rows of grain_ids[i] and vals[i][EXA_GRAIN_NVALS] (the
 * element count as an integer, the rest with 17 significant digits).  Returns 0 or -1 (err). */
int exa_grain_avgs_write(const char* path, int n, const int32_t* grain_ids, const double* vals, char* err, int errlen);
/* the ParaView writer on a fixed two-hexahedron piece (host only): fields = 2 rows of EXA_NFIELDS doubles, saved under dir as cycles 0 (t = 0)
 * and 1 (t = 0.5); mesh and point data documented at the definition (host/driver_capi.hip) */
int exa_vtu_selftest(const char* dir, const double* fields, int light_up, char* err, int errlen);
/* the driver's tail-split controller as a pure function (host logic; tests): cap on local-solver evaluations chosen from a 64-bin
 * histogram of evaluation counts, 0 = leave the launch uncapped.  tail_cost = relative cost of a point in the second launch. */
int exa_choose_newton_cap(const int* hist64, double tail_cost);
/* the same for resumed tail points (exa_set_newton_caps): first cap and second cap (0 = one dense launch) */
int exa_choose_newton_caps(const int* hist64, double tail_cost, int* k1, int* k2);

/* block decomposition of an N0 x N1 x N2 element grid (reference: ParMesh/METIS, src/mechanics_driver.cpp:312): sizes first
 * (info[0..7] = {E, NN, nneighbors, pg0, pg1, pg2, total shared dofs, n}; info[7] is in/out: H1 order p on input (0 or 1 -> 1, 2 -> 2),
 * nodes per element n = (p+1)^3 on output), then the arrays when the pointers are non-null:
 * conn (n,E) native node order, X (NN,3 byNODES), elem_gid (E), weight (NN), nbr_rank (nneighbors), nbr_count (nneighbors), nbr_dofs (concatenated) */
int exa_partition_query(const int* N, int rank, int nranks, int64_t* info8, int32_t* conn, double* X, int64_t* elem_gid, double* weight,
                        int32_t* nbr_rank, int32_t* nbr_count, int32_t* nbr_dofs);
/* the same view of the partition of an MFEM mesh v1.0 file (Mesh.type = "other"): every rank reads the file, elements are split by
 * recursive coordinate bisection of their centroids (reference: METIS through ParMesh, src/mechanics_driver.cpp:312), elem_gid = index
 * of the element in the file, nodes renumbered per rank in ascending global order.  Returns 0 or -1 (err). */
/* The element order the driver runs with on several ranks: elements touching a node shared with another rank first (their 64-element
 * blocks are computed before the halo exchange starts, the interior ones while it is on the wire).  out2 = { E, E_bdr }. */
int exa_partition_query_boundary_first(const int* N, int rank, int nranks, int order, int64_t* out2, int32_t* conn, int64_t* elem_gid);
/* [BCs] periodic_free: out10 = { mixed loading on (0 / 1), the 3 x 3 mask row by row }; returns 0 or -1 (err) */
int exa_options_query_periodic_free(const char* toml_path, int* out10, char* err, int errlen);
/* The tables of mixed loading of a rank's block: info8 = { local nodes, top-face nodes of direction 0, 1, 2, image entries,
 * neighbours, neighbour dofs in all, local groups }, then the arrays whose pointers are non-null: weight (local nodes), face_nodes (the three
 * lists back to back), ctrl4 (local ids of c_0 .. c_3, -1 where another rank holds the node), img_nodes / img_code (image entries; bit d of the
 * code: one period up in direction d, bit 3: a corner), canon (local nodes), nbr_dofs (concatenated) */
int exa_partition_query_periodic_mixed(const int* N, int rank, int nranks, int order, int64_t* info8, double* weight, int32_t* face_nodes, int32_t* ctrl4,
                                       int32_t* img_nodes, uint8_t* img_code, int64_t* canon, int32_t* nbr_dofs);
/* The periodic view of a rank's block of the generated mesh: info8 = { local nodes, neighbours, neighbour dofs in all, local
 * groups, their members in all, groups of 2, of 4, of 8 images }, then the arrays whose pointers are non-null: canon (local nodes; the
 * canonical id: global grid index with index N p mapped to 0 in every direction, numbered like node_gid), weight (local nodes; 1 / holders of the
 * canonical id over all ranks), nbr_rank / nbr_count (neighbours), nbr_dofs (concatenated; component by component, ascending canonical id,
 * identical on both sides), grp_off (local groups + 1) and grp_nodes: CSR of the canonical ids with >= 2 local images, by size, then by id. */
int exa_partition_query_periodic(const int* N, int rank, int nranks, int order, int64_t* info8, int64_t* canon, double* weight, int32_t* nbr_rank,
                                 int32_t* nbr_count, int32_t* nbr_dofs, int32_t* grp_off, int32_t* grp_nodes);
/* local -> global node numbers of a rank's partition: info2 = { local nodes, global nodes }; node_gid (local nodes) may be NULL.  Ranks that hold
 * the same node give it the same number (generated meshes: the (N p + 1)^3 grid, x fastest; file meshes: the reader's numbering after elevation) */
int exa_partition_query_nodes(const int* N, int rank, int nranks, int order, int64_t* info2, int64_t* node_gid);
int exa_mesh_partition_query_nodes(const char* mesh_path, int rank, int nranks, int order, int64_t* info2, int64_t* node_gid, char* err, int errlen);
int exa_mesh_partition_query(const char* mesh_path, int rank, int nranks, int64_t* info8, int32_t* conn, double* X, int64_t* elem_gid, double* weight,
                             int32_t* nbr_rank, int32_t* nbr_count, int32_t* nbr_dofs, char* err, int errlen);
/* ... at p_refinement = order: 1, or 2 = one node added per edge, face and element of the trilinear file mesh (what the reference's order
 * elevation of the nodal space gives for straight-sided hexahedra, src/mechanics_driver.cpp:300-306); higher orders: generated meshes only. */
int exa_mesh_partition_query_order(const char* mesh_path, int rank, int nranks, int order, int64_t* info8, int32_t* conn, double* X, int64_t* elem_gid,
                                   double* weight, int32_t* nbr_rank, int32_t* nbr_count, int32_t* nbr_dofs, char* err, int errlen);
#ifdef __cplusplus
}
#endif
#endif
