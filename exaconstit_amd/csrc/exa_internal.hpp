// Internal definitions of libexaconstit_hip.so (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include <type_traits>
#include <cstdint>
#include <cstdlib>
#include "../../include/exaconstit_hip.h"
#include "ecm_device.hpp"

#define EXA_HIP_CHECK(ctx, call)                                                                 \
   do {                                                                                          \
      hipError_t e_ = (call);                                                                    \
      if (e_ != hipSuccess) { (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_); return EXA_ERR_HIP; } \
   } while (0)

// Internal layout of the partial-assembly gradient data ("pa data"), one record per quadrature point:
//   36 doubles  Ct(i,j) = C(i,j) * dt * W_q / detJ      (column-major 6x6, Voigt, engineering shear)
//    9 doubles  adj(J)(r,c) at slot 36 + 3 r + c
//    1 double   W_q * detJ (quadrature weight in the current configuration)
// stored as [block of 64 elements][qpt][23 slot-pairs][64 lanes][2] so that lane = element reads 16 B and a wave reads
// 1 KiB contiguous per instruction.  (The reference stores 81 + 81 doubles per point: src/mechanics_integrators.cpp:395-414.)
constexpr int PA_SLOTS = 46;
constexpr int PA_PAIRS = 23;
constexpr int PA_BLK = 64;
// who wrote the gradient data a context holds
enum exa_grad_source { EXA_GRAD_NONE = 0, EXA_GRAD_FROM_SETUP, EXA_GRAD_FROM_MODEL_RECORDS };   // nobody yet | exa_grad_setup | exa_model_setup_lvec_records

struct exa_ctx {
   exa_config cfg;
   ecmdev::MatParams mp;
   int p, n, Q, E;
   int64_t P;               // E * Q
   int geom = EXA_GEOM_HEX; // EXA_GEOM_*: tetrahedra take the table-driven kernels and the fused action of tet_kernels.hip, never a hexahedron fast path
   double* tet_rec = nullptr;               // tetrahedra, p = 1: element records of the fused action (tet_kernels.hip)
   bool tet_fused = true;                   // tetrahedra: exa_grad_setup builds the element records for the fused action (exa_tet_set_fused_action)
   int nstatev;
   int device;
   std::string err;
   std::vector<double> G_host, W_host;      // (n,3,Q), (Q)
   double* G_dev = nullptr; double* W_dev = nullptr;
   // residual PA data (D of AssemblePA), gradient PA data / EA matrices
   double* dmat = nullptr;                  // (3,3,Q,E)
   double* pa = nullptr;                    // see layout above
   double* emat = nullptr;                  // EA: p=1 full integration [block][24][12 pairs][64][2]; otherwise [block][3n][3n][64]
   double* T1_dev = nullptr;                // p = 2 matrix-free action: one-dimensional basis tables (3 x 6)
   double* eDS = nullptr;                   // B-bar: element-average shape gradient [block][n x 3][64 lanes]
   double* eDSP = nullptr;                  // B-bar, p = 2 multigrid: average gradients of the eight embedded trilinear functions [block][8 x 3][64 lanes]
   double* tbuf = nullptr;                  // generic PA action: per-point T (3,3,Q,E)
   double* vgrad_ref = nullptr;             // p = 2 element-blocked constitutive launch: reference-space velocity gradients of its geometry pre-pass (3,3,Q,E)
   const double* resid_J = nullptr; const double* resid_S = nullptr;   // B-bar residual reads J and sigma at apply time, like the reference
   bool ea_matfree = false;                 // EA: L-vector action computed from the point records, matrices assembled on demand (exa_set_ea_matrix_free)
   bool qblk = false;                       // quadrature functions in the element-blocked layout (see QView below)
   bool aos_stage = true;                   // AOS layout: constitutive launches move a wave's contiguous point rows coalesced and transpose them through LDS (exa_set_aos_staging)
   bool have_resid = false;
   // ---- gradient data: which exist, and who builds the rest (the buffers are pa, pa_c, emat, tet_rec above and below) ----
   int grad_src = EXA_GRAD_NONE;            // exa_grad_source.  FROM_MODEL_RECORDS: the compact records alone - no 46-double records, no element matrices, no geometry
   // what the last exa_grad_setup was given.  Borrowed: the caller leaves J and C untouched until the next set-up, because a record set marked pending
   // below is built from them by the first call that reads it (they do stay in a Newton iteration: the reference calls AssembleGradDiagonalPA right after
   // AssembleGradPA, src/mechanics_operator.cpp:436-443)
   const double* setup_J = nullptr; const double* setup_C = nullptr; double setup_dt = 0.0;
   bool pa_pending = false;                 // the set-up wrote the compact records only: `pa` waits for the diagonal, the E-vector action or an action without coordinates
   bool tet_pending = false;                // the set-up did not expect the fused tetrahedron action: `tet_rec` waits for the first exa_grad_apply_lvec
   bool emat_valid = false;                 // EA: `emat` holds the matrices of the last set-up (assembled in it, or on demand in matrix-free contexts)
   bool ea_generic = false;                 // EA: the matrices have the generic layout (B-bar, p != 1, tetrahedra), not the p = 1 one
   int tangent_form = 0;                    // EXA_TANGENT_*: the form the next set-up writes
   int pac_pairs = 0;                       // 16-byte pairs per point of the records in pa_c: PAC_PAIRS (D, K) or PAC_PAIRS_GEO (+ geometry); 0 without pa_c
   const double* coords_lvec = nullptr;     // optional: nodal coordinates the Jacobians of the set-up came from (geometry recomputed in the apply; exa_grad_set_coords)
   // L-vector support
   const int32_t* conn = nullptr; int nnodes = 0;
   double* pa_c = nullptr;                  // compact tangent records (25 + 1 per point, + 10 of geometry in the 18-pair shape); allocated when the form is first set up
   // deterministic E->L (exa_set_deterministic): node -> (element, local node) table in element order + per-element output scratch
   int det = 0; int32_t* n2e_off = nullptr; int32_t* n2e_idx = nullptr; double* ev_det = nullptr; int det_nnodes = 0; const int32_t* det_conn = nullptr;
   // status
   int* fail_count_dev = nullptr;
   int newton_cap = 0; int* tail_dev = nullptr;   // tail split of the constitutive launch: [0] = count, [1..] = deferred point ids
   int newton_cap2 = 0; int* tail2_dev = nullptr; // second level (exa_set_newton_caps): list of the points the first tail launch cuts off
   int tail_resume = 1; double* resume_dev[2] = { nullptr, nullptr };   // solver states of the listed points, [RS_N][P] by list slot
   int cap_auto = 0; double cap_tail_cost = 0.0; long cap_calls = 0;   // exa_set_newton_cap_auto: the library picks newton_cap from the evaluation counts of its own launches
   // exa_set_lean_state: the element-blocked record launches leave the inputs of the slip rates in state slots 14..19 instead of the 12 rates;
   // lean_kin: kernel kind (ecmdev::KIN_* with its flags) of the last such launch, which exa_slip_rates_from_state instantiates the kinetics with
   bool lean_state = false; int lean_kin = -1;
   // element-blocked p = 1 record launches so far: through the entry without tail-split arguments (k_model_setup_rec_nt) / through the generic kernel (exa_model_record_launches)
   int64_t rec_policy_launches = 0, rec_generic_launches = 0;
   double* scratch_dev = nullptr; size_t scratch_bytes = 0;   // reductions
   double hist_init[ecmdev::NUM_HIST];
};

// host-side reference element (H1 hex of order p at (p+1)^3 Gauss-Legendre points), src/mechanics_operator.cpp:237-261
int exa_ensure_p2_tables(struct exa_ctx* ctx);   // gen_kernels.hip
void exa_build_ref_elem(int p, std::vector<double>& G, std::vector<double>& W);
// reference tetrahedron of order p = 1, 2; false for other orders.  N (n, Q) shape values, may be null
bool exa_build_ref_elem_tet(int p, std::vector<double>& G, std::vector<double>& W, std::vector<double>* N);
static inline bool exa_is_hex(const exa_ctx* ctx) { return ctx->geom == EXA_GEOM_HEX; }
// one-dimensional tables [1D Gauss point][B_0..B_p, D_0..D_p] of the order-p nodal basis and the lexicographic -> native node map
void exa_build_1d_tables(int p, std::vector<double>& T1, std::vector<int>& nat);
bool exa_fill_mat_params(const exa_config& cfg, ecmdev::MatParams& mp, double* hist_init, std::string& err);

// Quadrature-function addressing.  AOS is the reference's QuadratureFunction layout (vdim values of a point contiguous, points of an
// element consecutive).  EB64 is the internal layout of the stand-alone driver: [block of 64 elements][point q][value k][lane = element],
// the same blocking as the PA record, so that a wave whose lanes are 64 consecutive elements reads or writes one contiguous 512-byte
// row per value — the per-lane 224/288-byte strides of AOS cost the constitutive kernel 5 of its 7.5 ms at 128^3.
struct QView { int64_t base; int stride; };
template <bool QB>
__device__ __forceinline__ QView qview(int W, int Q, int64_t e, int q) {
   if (QB) return { ((((e >> 6) * Q + q) * (int64_t)W) << 6) + (e & 63), 64 };
   return { (int64_t)W * (q + (int64_t)Q * e), 1 };
}
// Shape-derivative table (n,3,Q) of the reference element: the kernels that walk it stage it in LDS when it is small (p = 1: 1.5 KB, p = 2:
// 17 KB) and read it from global memory at the orders the reference's unit tests also run (p = 3: 96 KB ... p = 6: 2.8 MB); one rule for
// the kernel (stage_shape) and for the launch (exa_g_lds_bytes)
constexpr int64_t EXA_G_LDS_MAX_DOUBLES = 6144;
static inline __host__ __device__ bool exa_g_in_lds(int n, int Q) { return (int64_t)n * 3 * Q <= EXA_G_LDS_MAX_DOUBLES; }
static inline size_t exa_g_lds_bytes(int n, int Q) { return exa_g_in_lds(n, Q) ? sizeof(double) * (size_t)n * 3 * Q : 0; }
#ifdef __HIPCC__
__device__ __forceinline__ const double* stage_shape(double* lds, const double* __restrict__ G, int n, int Q) {
   if (!exa_g_in_lds(n, Q)) return G;      // kernel-uniform
   for (int i = threadIdx.x; i < n * 3 * Q; i += blockDim.x) lds[i] = G[i];
   __syncthreads();
   return lds;
}
#endif
static inline size_t exa_qf_doubles(const exa_ctx* ctx, int vdim) {
   return ctx->qblk ? (size_t)vdim * 64 * ctx->Q * ((ctx->E + 63) / 64) : (size_t)vdim * ctx->P;
}

#ifdef __HIPCC__
// Point records and element matrices are streams: a launch of an operator action reads each 16-byte pair exactly once, gigabytes per launch (3.5 GB of
// compact records at 128^3), and the next launch reads them again from HBM whatever the caches held.  With the non-temporal hint they pass through
// without displacing the node rows (x, coordinates, the atomically updated y) that neighbouring waves share in L2: p = 1 action 0.712 -> 0.664 ms,
// PCG 1 169 -> 1 232 it/s at 128^3 in one call (round 5).  EXA_APPLY_NT=0: plain loads (A/B switch).
#ifndef EXA_APPLY_NT
#define EXA_APPLY_NT 1
#endif
template <bool NT = (EXA_APPLY_NT != 0)>
__device__ __forceinline__ double2 ld_rec(const double2* p) {
   if constexpr (NT) {
      typedef double vd2 __attribute__((ext_vector_type(2)));
      const vd2 v = __builtin_nontemporal_load(reinterpret_cast<const vd2*>(p));
      return make_double2(v.x, v.y);
   } else return *p;
}
// ... when the stream is larger than the caches can hold from one launch to the next.  Round 6, same call, PCG iterations/s with the hints | without: 16^3 (7 MB of
// compact records) 40 226 | 42 137, 32^3 (54 MB) 30 469 | 31 393, 64^3 (436 MB) 8 494 | 7 738: a small partition's records and vectors live in L2 / MALL across
// iterations and the hint throws that away.  The p = 1 action and the PCG vector kernels therefore carry it only above this size (EXA_NT_MIN_MB overrides; 0 = always)
static inline bool exa_stream_nt(size_t bytes_per_launch) {
   static const double min_mb = [] { const char* e = std::getenv("EXA_NT_MIN_MB"); return e ? std::atof(e) : 128.0; }();
   return EXA_APPLY_NT != 0 && (double)bytes_per_launch >= min_mb * 1048576.0;
}
// Workgroups are dealt round-robin to the 8 XCDs (each with its own L2).  Remapped, XCD x works on one contiguous eighth of the element blocks, so the node rows
// neighbouring blocks share (gathers of x / coordinates, scatter atomics) stay within one L2 (p = 1 action since round 4; p = 2 action / residual / pre-pass: round 6)
#ifndef EXA_XCD_REMAP
#define EXA_XCD_REMAP 1
#endif
__device__ __forceinline__ int64_t xcd_block(const unsigned b, const unsigned nb) {
   if (!EXA_XCD_REMAP) return b;
   const unsigned q = nb >> 3, r = nb & 7u, x = b & 7u, i = b >> 3;
   return x < r ? (int64_t)x * (q + 1) + i : (int64_t)r * (q + 1) + (int64_t)(x - r) * q + i;
}
// ---- compact tangent form (include/exaconstit_hip.h, EXA_TANGENT_DEV5_BULK) ----------------------------------------------------
// d sigma / d eps = V65 D V65^T + K m m^T: a 5 x 5 block in ExaCMech's deviatoric vector basis plus the bulk term, m = (1,1,1,0,0,0).
constexpr int PAC_PAIRS = 13;       // compact record of the p = 1 action: 25 D entries + K, scaled by dt W / detJ
constexpr int PAC_PAIRS_GEO = 18;   // compact record of the p = 2 action: the same + adj(J) (9) + W detJ
template <int NP>
__device__ __forceinline__ int64_t pac_off(int64_t blk, int Q, int q, int pair) { return (((blk * Q + q) * NP + pair) * PA_BLK) * 2; }
constexpr double C_SQR2I = 0.70710678118654752440, C_SQR6I = 0.40824829046386301637;
__device__ __forceinline__ void v65t(const double c0, const double c1, const double c2, const double c3, const double c4, const double c5, double o[5]) {
   o[0] = C_SQR2I * (c0 - c1); o[1] = C_SQR6I * (2.0 * c2 - c0 - c1); o[2] = C_SQR2I * c5; o[3] = C_SQR2I * c4; o[4] = C_SQR2I * c3;
}
// D = L^-1 V65^T C V65 L^-1 with L = V65^T V65 = diag(1,1,1/2,1/2,1/2), K = m^T C m / 9 (exact when C has the form above)
__device__ __forceinline__ void tangent_to_d55(const double* c, const int64_t st, double D[25], double& K) {
   double T[5][6];
#pragma unroll
   for (int j = 0; j < 6; j++) {
      double o[5]; v65t(c[(0 + 6 * j) * st], c[(1 + 6 * j) * st], c[(2 + 6 * j) * st], c[(3 + 6 * j) * st], c[(4 + 6 * j) * st], c[(5 + 6 * j) * st], o);
#pragma unroll
      for (int k = 0; k < 5; k++) T[k][j] = o[k];
   }
#pragma unroll
   for (int k = 0; k < 5; k++) {
      double o[5]; v65t(T[k][0], T[k][1], T[k][2], T[k][3], T[k][4], T[k][5], o);
#pragma unroll
      for (int l = 0; l < 5; l++) D[k + 5 * l] = o[l] * ((k < 2 ? 1.0 : 2.0) * (l < 2 ? 1.0 : 2.0));
   }
   double t = 0;
#pragma unroll
   for (int j = 0; j < 3; j++)
#pragma unroll
      for (int i = 0; i < 3; i++) t += c[(i + 6 * j) * st];
   K = t * (1.0 / 9.0);
}
// s = (V65 D V65^T + K m m^T) eps
__device__ __forceinline__ void d55_apply(const double D[25], const double K, const double eps[6], double sg[6]) {
   double e5[5], s5[5];
   v65t(eps[0], eps[1], eps[2], eps[3], eps[4], eps[5], e5);
#pragma unroll
   for (int k = 0; k < 5; k++) s5[k] = D[k] * e5[0] + D[k + 5] * e5[1] + D[k + 10] * e5[2] + D[k + 15] * e5[3] + D[k + 20] * e5[4];
   const double t1 = C_SQR2I * s5[0], t2 = C_SQR6I * s5[1], bk = K * (eps[0] + eps[1] + eps[2]);
   sg[0] = t1 - t2 + bk; sg[1] = -t1 - t2 + bk; sg[2] = 2.0 * C_SQR6I * s5[1] + bk; sg[3] = C_SQR2I * s5[4]; sg[4] = C_SQR2I * s5[3]; sg[5] = C_SQR2I * s5[2];
}
#endif

// ---- forms of the gradient data, named once (host) ------------------------------------------------------------------------------
static inline unsigned exa_nblocks(const exa_ctx* ctx) { return (unsigned)((ctx->E + PA_BLK - 1) / PA_BLK); }   // 64-element blocks
static inline bool exa_p1_full(const exa_ctx* ctx) { return ctx->p == 1 && ctx->cfg.integ == EXA_INTEG_FULL; }
// the L-vector action runs from the point records: partial assembly, or element assembly switched to matrix-free ...
static inline bool exa_acts_from_records(const exa_ctx* ctx) { return ctx->cfg.assembly == EXA_ASSEMBLY_PA || ctx->ea_matfree; }
// ... which on hexahedra has kernels for the transposed tangent at p = 2 and at p = 1 full integration
static inline bool exa_ea_from_records(const exa_ctx* ctx) { return exa_is_hex(ctx) && ctx->ea_matfree && (ctx->n == 27 || exa_p1_full(ctx)); }
static inline bool exa_has_compact(const exa_ctx* ctx) { return ctx->pa_c && ctx->pac_pairs == PAC_PAIRS; }           // compact p = 1 record
static inline bool exa_has_compact_geo(const exa_ctx* ctx) { return ctx->pa_c && ctx->pac_pairs == PAC_PAIRS_GEO; }   // compact record with geometry
// this p = 1 launch streams the compact record (and recomputes the geometry): picks the kernel AND sizes its record stream
static inline bool exa_streams_compact(const exa_ctx* ctx, bool lvec) { return lvec && ctx->coords_lvec && exa_has_compact(ctx); }
static inline size_t exa_pa_bytes(const exa_ctx* ctx) { return (size_t)exa_nblocks(ctx) * ctx->Q * PA_SLOTS * PA_BLK * sizeof(double); }
static inline size_t exa_pac_bytes(const exa_ctx* ctx) { return (size_t)exa_nblocks(ctx) * ctx->Q * 2 * ctx->pac_pairs * PA_BLK * sizeof(double); }
static inline size_t exa_eds_bytes(const exa_ctx* ctx) { return sizeof(double) * 3 * ctx->n * PA_BLK * (size_t)exa_nblocks(ctx); }
static inline size_t exa_emat_bytes(const exa_ctx* ctx) { const size_t nd = 3 * (size_t)ctx->n; return (size_t)exa_nblocks(ctx) * nd * nd * PA_BLK * sizeof(double); }
static inline void exa_forget_grad(exa_ctx* ctx) { ctx->grad_src = EXA_GRAD_NONE; }   // the next action is refused until a set-up
// a record set marked pending, built now from what the last exa_grad_setup was given
template <class Build>
static inline int exa_build_pending(exa_ctx* ctx, bool& pending, Build build, hipStream_t s) {
   if (!pending) return EXA_OK;
   const int rc = build(ctx, ctx->setup_dt, ctx->setup_J, ctx->setup_C, s);
   if (rc == EXA_OK) pending = false;
   return rc;
}

// ---- launching ------------------------------------------------------------------------------------------------------------------
// Run-time flags to template arguments: f is called once, with std::true_type / std::false_type in place of each flag, and holds the one launch line
// (a generic lambda: `[&](auto qb, auto nt) { hipLaunchKernelGGL((k<qb.value, nt.value>), ...); }`).  Every combination of the flags handed in is
// instantiated; where a kernel leaves combinations out, branch before the call and hand in the flags that remain.
template <class F> static inline void exa_dispatch(F&& f) { f(); }
template <class F, class... Bs>
static inline void exa_dispatch(F&& f, bool b, Bs... bs) {
   if (b) exa_dispatch([&](auto... t) { f(std::true_type(), t...); }, bs...);
   else exa_dispatch([&](auto... t) { f(std::false_type(), t...); }, bs...);
}
constexpr std::true_type EXA_YES{}; constexpr std::false_type EXA_NO{};
// the tail of every launcher
static inline int exa_launched(exa_ctx* ctx) { EXA_HIP_CHECK(ctx, hipGetLastError()); return EXA_OK; }
