// The fused constitutive kernel and its launch helpers, shared by the two translation units that instantiate it (model_kernels.hip: the element-blocked
// and per-lane AOS launches; model_kernels_aos.hip: the staged AOS launches).  See model_kernels.hip for the reference functions the launch replaces.
#pragma once
#include "exa_internal.hpp"
#include "p2_basis.hpp"
#include <cstdlib>
#include <cstring>

using namespace ecmdev;

#ifndef EXA_MODEL_OCC
#define EXA_MODEL_OCC 2   // waves per SIMD the register allocator is asked to fit (tuned on MI355X)
#endif
#ifndef EXA_MODEL_BS
#define EXA_MODEL_BS 128   // threads per block of the constitutive launch (4 blocks of 2 waves per CU: 38.9 KB of stash each; a block waits for 2 waves, not 4)
#endif
static_assert(EXA_MODEL_BS % ecmdev::STASH_STRIDE == 0, "a block is a whole number of per-wave stash regions");
constexpr int EXA_STASH_DOUBLES = ecmdev::ST_SLOTS * EXA_MODEL_BS;   // LDS stash of a block

// row pieces of the staged launch: non-temporal loads / stores like the per-lane accesses of the other launches
// (every round stores whole 128-byte lines: with the tangent in 144-byte pieces - rounds of 3 columns - plain stores were the faster ones)
__device__ __forceinline__ double2 ldg2(const double* p) {
   typedef double vd2 __attribute__((ext_vector_type(2)));
   const vd2 v = __builtin_nontemporal_load(reinterpret_cast<const vd2*>(p));
   return make_double2(v.x, v.y);
}
// Row strides (doubles) in the stage: the rows lie there as in memory.  (Measured: rows one double apart - odd strides 29 / 7, no LDS bank conflicts of the lanes'
// 8-byte row accesses, two 8-byte LDS accesses per 16-byte piece - are slower, 4.87 against 4.83 ms at 128^3: the row accesses are not what the launch waits for.)
constexpr int RS_SV = ecmdev::NSTATEV, RS_S = 6, RS_T = 36;
__device__ __forceinline__ void stg2r(double* p, const double a, const double b) { ecmdev::stg2(reinterpret_cast<double2*>(p), a, b); }
// Where one thread's quadrature point lives.  Everything is a function of (block index, thread index) and kernel-uniform data, so nothing
// per-lane has to survive the local Newton solve: locate() derives the point from the thread index, refresh() does it again behind a compiler
// barrier after the solve, and the accessors form the addresses where they are used.  Before, five 64-bit row pointers and two LDS addresses
// were live across the solve; the register allocator spilled some of them and re-loaded them from scratch BEHIND the first output stores,
// where a load waits for the whole store queue of the wave (ecm_device.hpp, epilogue of point_update).
// STG (staged AOS launch, QB = false): a wave owns the 64 CONSECUTIVE points pt0() ... pt0() + 63, whose rows are contiguous in every (vdim, Q, E) array.
// The wave's stash region (ST_SLOTS x 64 doubles of LDS) doubles as its transposition buffer: rows come in through coalesced 16-byte loads and are
// read back by their lanes (model_kernel.hpp, stage_in); outputs are written by their lanes as rows - sv1() / s1() / cm() point into the region - and
// leave through coalesced 16-byte stores (flush_tangent, flush_state).  A lane beyond the last point repeats the last point (live = false) and
// stores nothing: all 64 lanes take part in every round.  The dense launches of a tail split run the SAME kernel (tail_mode, so that a listed point is
// finished with the bits the full launch would have given it): their lanes are scattered points, which read their inputs per lane, write their
// output rows into the stage like everybody and copy them out per lane.
// TAIL = false (launch policy of k_model_setup_rec_nt): never a dense launch - no list, locate() / refresh() keep the one branch of their layout
template <bool QB, bool REC, bool STG = false, int NPAIR = PAC_PAIRS, bool TAIL = true>
struct PointIO {
   const double* state0; const double* stress0; double* state1; double* stress1; double* cmat;   // kernel-uniform array bases
   double* stash0;                  // LDS stash of the block
   const int* tail; int tail_mode;  // dense tail launch: thread t owns point tail[1 + t]
   int Q; int64_t bidx; int wpb;    // points per element, (remapped) block index, waves per block
   int q; int64_t e; int tid;       // this thread's point and its index in the block
   int64_t P; bool live;            // STG: points of the launch; this lane's point exists
   static_assert(!STG || !QB, "staged rows: AOS layout");
   static_assert(TAIL || (QB && !STG), "launch policy without tail split: the element-blocked per-lane launches");
   __device__ __forceinline__ int wave() const { return STG ? __builtin_amdgcn_readfirstlane(tid >> 6) : (tid >> 6); }   // (STG: wave-uniform row addresses in scalar registers)
   __device__ __forceinline__ int64_t pt0() const { return (bidx * wpb + wave()) * 64; }
   __device__ __forceinline__ int nvalid() const { const int64_t r = P - pt0(); return r < 64 ? (int)r : 64; }   // points of this wave that exist (may be <= 0)
   __device__ __forceinline__ void locate(const int tid_) {
      tid = tid_;
      if constexpr (!TAIL) { const int64_t gw = bidx * wpb + (tid >> 6); q = (int)(gw % Q); e = (gw / Q) * 64 + (tid & 63); }
      else if (STG && !tail_mode) { const int64_t ip = pt0() + (tid & 63); live = ip < P; const int64_t ie = live ? ip : P - 1; q = (int)(ie % Q); e = ie / Q; }
      else if (tail_mode) { const int64_t ipt = tail[1 + bidx * (int64_t)(wpb * 64) + tid]; q = (int)(ipt % Q); e = ipt / Q; }
      else if (QB) { const int64_t gw = bidx * wpb + (tid >> 6); q = (int)(gw % Q); e = (gw / Q) * 64 + (tid & 63); }   // wave = (block of 64 elements, q); lane = element
      else { const int64_t ip = bidx * (int64_t)(wpb * 64) + tid; q = (int)(ip % Q); e = ip / Q; }
   }
   // the wave's region of the stash (STG: its stage); row of the point this lane computes on input (the last existing one for a lane beyond the end)
   __device__ __forceinline__ double* wreg() const { return stash0 + wave() * (ecmdev::ST_SLOTS * 64); }
   __device__ __forceinline__ int row_in() const { return (int)(e * Q + q - pt0()); }
   // one round of coalesced row stores: n doubles of the stage at lds -> g (16-byte aligned), 16 bytes per lane and pass
   // (rows of W doubles RS apart in the stage; RS == W: the stage holds them as they lie in memory)
   template <int W, int RS, int NROWS = 64>
   __device__ __forceinline__ void flush_rows(const double* lds, double* g, const int n) const {
      const int lane = tid & 63;
#pragma unroll
      for (int m = 0; m < (NROWS * W / 2 + 63) / 64; m++) {
         const int u = m * 64 + lane;
         const int i0 = (RS == W) ? 2 * u : ((2 * u) / W) * RS + (2 * u) % W;      // (W even when RS != W: both doubles of a piece lie in one row)
         if (2 * u + 1 < n) stg2r(g + 2 * u, lds[i0], lds[i0 + 1]);
         else if (2 * u < n) ecmdev::stg(g + 2 * u, lds[i0]);      // (odd row counts: Jacobian rows of a wave that ends the array at an odd-order element)
      }
   }
   // the 36-double tangent rows of points 32 h ... 32 h + 31 of the wave (staged_tangent, ecm_device.hpp): 9 216 contiguous bytes
   __device__ __forceinline__ int half() const { return (tid >> 5) & 1; }
   __device__ __forceinline__ void flush_tangent(const int h) const {
      if (tail_mode) {   // (uniform) this lane's row to its own point
         if (half() != h) return;
         const double* row = wreg() + (tid & 31) * RS_T; double* g = cmat + (e * Q + q) * 36;
#pragma unroll
         for (int c = 0; c < 18; c++) stg2r(g + 2 * c, row[2 * c], row[2 * c + 1]);
         return;
      }
      const int nv = nvalid() - 32 * h;
      if (nv > 0) flush_rows<36, 36, 32>(wreg(), cmat + (pt0() + 32 * h) * 36, (nv < 32 ? nv : 32) * 36);
   }
   __device__ __forceinline__ void flush_state() const {
      if (tail_mode) {
         const double* row = wreg() + (tid & 63) * RS_SV; double* g = state1 + (e * Q + q) * ecmdev::NSTATEV;
#pragma unroll
         for (int c = 0; c < ecmdev::NSTATEV / 2; c++) ecmdev::stg2(reinterpret_cast<double2*>(g + 2 * c), row[2 * c], row[2 * c + 1]);
         const double* rs = wreg() + 64 * RS_SV + (tid & 63) * RS_S; double* gs = stress1 + (e * Q + q) * 6;
#pragma unroll
         for (int c = 0; c < 3; c++) ecmdev::stg2(reinterpret_cast<double2*>(gs + 2 * c), rs[2 * c], rs[2 * c + 1]);
         return;
      }
      const int nv = nvalid();
      flush_rows<ecmdev::NSTATEV, RS_SV>(wreg(), state1 + pt0() * ecmdev::NSTATEV, nv * ecmdev::NSTATEV);
      flush_rows<6, RS_S>(wreg() + 64 * RS_SV, stress1 + pt0() * 6, nv * 6);
   }
   __device__ __forceinline__ void refresh() { int t = threadIdx.x; asm volatile("" : "+v"(t)); locate(t); }
   __device__ __forceinline__ const double* sv0() const { return state0 + qview<QB>(ecmdev::NSTATEV, Q, e, q).base; }
   __device__ __forceinline__ const double* s0() const { return stress0 + qview<QB>(6, Q, e, q).base; }
   // (STG: the lane's rows of the stage - state 28, stress 6 behind the 64 state rows, tangent half 18)
   __device__ __forceinline__ double* sv1() const { return STG ? wreg() + (tid & 63) * RS_SV : state1 + qview<QB>(ecmdev::NSTATEV, Q, e, q).base; }
   __device__ __forceinline__ double* s1() const { return STG ? wreg() + 64 * RS_SV + (tid & 63) * RS_S : stress1 + qview<QB>(6, Q, e, q).base; }
   // REC: the lane's first 16-byte pair of its compact record ([block][q][13 pairs][64 lanes][2]); else the tangent slot
   __device__ __forceinline__ double* cm() const {
      if (STG && !REC) return wreg() + (tid & 31) * RS_T;      // (lanes l and l + 32 use the row one after the other)
      return REC ? cmat + pac_off<NPAIR>(e >> 6, Q, q, 0) + 2 * (e & 63) : cmat + qview<QB>(36, Q, e, q).base;
   }
   // slot s of this thread at stash()[s * STASH_STRIDE]: the regions of the block's waves, one behind the other
   __device__ __forceinline__ double* stash() const { return stash0 + (tid / ecmdev::STASH_STRIDE) * (ecmdev::ST_SLOTS * ecmdev::STASH_STRIDE) + (tid % ecmdev::STASH_STRIDE); }
   __device__ __forceinline__ int ipt() const { return (int)(e * Q + q); }
};

// LVEC = false: J (3,3,Q,E) and the velocity E-vector (n,3,E) are inputs (the reference's ModelSetup signature).
// LVEC = true : the kernel gathers nodal coordinates and velocities from the L-vectors through the connectivity, computes J itself
//               and WRITES it to Jio for the integrator kernels: NonlinearMechOperator::Setup's L->E restrictions and
//               SetupJacobianTerms (reference src/mechanics_operator.cpp:310-391) ride inside this VALU-bound kernel for free.
// NFIX = 8: trilinear elements, node loops fully unrolled so that all gathers of a point are in flight together (two memory round
// trips instead of one dependent index->value chain per node); NFIX = 0: run-time n.
// QB: quadrature functions (J, stress, state, tangent) in the element-blocked layout; then a wave is (64 consecutive elements, one
// point index q) so that every per-value access of the wave is one contiguous 512-byte row.
// REC (fused p = 1 launch of the stand-alone driver): cmat is the buffer of compact gradient records and the launch writes, instead of the
// 36 tangent entries, the record the gradient action streams (ecm_device.hpp, point_update<.., REC>): AssembleGradPA rides in the launch.
// STG (reference layout only): the staged form - see PointIO.  Input rows (state 28, stress 6; without LVEC also the Jacobians 9, and for trilinear elements
// the velocity E-vector rows of the wave's 8 elements and the shape table) are requested as 16-byte pieces, contiguous across the wave, go through the
// wave's stage and are read back by the lanes that own them; the Jacobians of an LVEC launch and all outputs leave the same way.  No block barrier: a
// wave only ever touches its own region.  Never a tail launch (scattered points: the per-lane form takes those).
// n doubles at g (16-byte aligned) -> registers, 16 bytes per lane and pass, contiguous across the wave; NU = passes (2 * 64 * NU >= total doubles)
template <int NU>
__device__ __forceinline__ void rows_load(const double* __restrict__ g, const int n, const int lane, double2 (&r)[NU]) {
#pragma unroll
   for (int m = 0; m < NU; m++) {
      const int u = m * 64 + lane;
      r[m] = make_double2(0.0, 0.0);
      if (2 * u + 1 < n) r[m] = ldg2(g + 2 * u);
      else if (2 * u < n) r[m].x = ecmdev::ldg(g + 2 * u);
   }
}
// ... -> the stage (TOT = doubles the rows occupy there; pieces beyond are not written)
// (W, RS: rows of W doubles go RS apart; 0, 0: as they lie in memory)
template <int NU, int TOT, int W = 0, int RS = 0>
__device__ __forceinline__ void rows_to_stage(double* lds, const int lane, const double2 (&r)[NU]) {
#pragma unroll
   for (int m = 0; m < NU; m++) {
      const int u = m * 64 + lane;
      if (2 * NU * 64 <= TOT || 2 * u < TOT) {
         if constexpr (RS == W) *reinterpret_cast<double2*>(lds + 2 * u) = r[m];
         else { const int i0 = ((2 * u) / W) * RS + (2 * u) % W; lds[i0] = r[m].x; lds[i0 + 1] = r[m].y; }
      }
   }
}
constexpr int STG_J = 0, STG_V = 576, STG_G = 768;   // stage offsets (doubles) of the prologue: 64 Jacobian rows, 8 velocity E-vector rows, the trilinear shape table

// LEAN (element-blocked record launches, exa_set_lean_state): state slots 14..19 carry the inputs of k_slip_rates_from_state instead of the 12 slip
// rates (ecm_device.hpp, point_update<.., LEAN>); the dense launches of a tail split run the same instantiation, so a listed point parks the same values
// The body of the kernel is model_kernel_body.hpp: one text that both entries below compile - k_model_setup, which takes everything at run time, and
// k_model_setup_rec_nt, which has the tail split compiled out.  (Textual inclusion, not a shared inline function: a function is simplified on its own
// before it is inlined, and that alone gave every k_model_setup instantiation other code - scripts/isa_identity.py.)  The body sees, besides the
// template parameters and kernel arguments of k_model_setup, the launch policy:
// TAIL = false: a launch that is never part of a tail split - no tail_mode, no cap test, no hand-over block and no TailIO in point_update, never a resumed
//               solve; PointIO keeps the one branch of its layout
// WJ: Jacobian output of the LVEC launches: -1 decided at run time (Jio != nullptr), 0 never (no test, no store code), 1 always
template <int KIN, bool LVEC, int NFIX, bool QB, bool REC = false, bool STG = false, bool LEAN = false>
__global__ __launch_bounds__(EXA_MODEL_BS, EXA_MODEL_OCC) void k_model_setup(const MatParams mp, const int Q, const int n_rt, const int64_t P, const double dt,
                                                     double* __restrict__ Jio, const double* __restrict__ G,
                                                     const double* __restrict__ vel, const double* __restrict__ xl, const int32_t* __restrict__ conn, const int nnodes,
                                                     const double* __restrict__ stress0,
                                                     const double* __restrict__ state0, double* __restrict__ stress1,
                                                     double* __restrict__ state1, double* __restrict__ cmat, int* __restrict__ fail,
                                                     const int kcap, int* __restrict__ tail, const int tail_mode_rt,
                                                     const double* __restrict__ Wq = nullptr, const int trd = 0,
                                                     int* __restrict__ tail_out = nullptr, const double* __restrict__ rs_in = nullptr, double* __restrict__ rs_out = nullptr) {
   constexpr bool TAIL = true; constexpr int WJ = -1;
#include "model_kernel_body.hpp"
}

// The element-blocked p = 1 record launch of a Voce kind that is not split (model_kernels.hip, launch_model_rec_l): the policy TAIL = false, WJ = 0, and an
// entry WITHOUT the tail-split arguments - five pointers and three integers less in the kernel-argument segment, which no longer compete with MatParams for
// scalar registers inside the Newton loop.  Same expression graph per evaluation, same bits (tests/test_gpu_record_launch_policy.py).
// (LVEC ... STG: the one launch form this entry exists for - template parameters, so that the body's `if constexpr` branches of the other forms are discarded)
template <int KIN, bool LEAN, bool LVEC = true, int NFIX = 8, bool QB = true, bool REC = true, bool STG = false>
__global__ __launch_bounds__(EXA_MODEL_BS, EXA_MODEL_OCC) void k_model_setup_rec_nt(const MatParams mp, const int Q, const int64_t P, const double dt, const double* __restrict__ G,
                                                     const double* __restrict__ vel, const double* __restrict__ xl, const int32_t* __restrict__ conn, const int nnodes,
                                                     const double* __restrict__ stress0, const double* __restrict__ state0, double* __restrict__ stress1,
                                                     double* __restrict__ state1, double* __restrict__ cmat, int* __restrict__ fail,
                                                     const double* __restrict__ Wq, const int trd) {
   static_assert(LVEC && NFIX == 8 && QB && REC && !STG, "the element-blocked fused p = 1 record launch");
   constexpr bool TAIL = false; constexpr int WJ = 0;
   // what the body names of the arguments this entry does not take
   constexpr int n_rt = 8, kcap = 1 << 30, tail_mode_rt = 0;
   double* const Jio = nullptr; int* const tail = nullptr; int* tail_out = nullptr; const double* rs_in = nullptr; double* const rs_out = nullptr;
#include "model_kernel_body.hpp"
}

// Launch sequence of the tail split (include/exaconstit_hip.h, exa_set_newton_caps): the full launch stops a point after newton_cap evaluations
// and lists it; a dense launch of the same kernel (thread = listed point; its grid covers the worst case, blocks beyond the list leave at
// once) takes the list up - from the saved solver state when the context holds the state buffers, from scratch otherwise - and, with a
// second cap, lists what it cuts off itself for a third launch.
// dynamic LDS of a launch of k_model_setup: shape rows (per wave for the element-blocked full launch, the whole table otherwise) + stash + slip table
// The largest shape table that passes exa_g_in_lds is the p = 2 one (27 * 3 * 27 doubles; p = 3 has 64 * 3 * 64 > EXA_G_LDS_MAX_DOUBLES and stays
// in global memory): with the stash and the slip table it must fit the 64 KB a launch gets without an attribute change.
static_assert(64 * 3 * 64 > EXA_G_LDS_MAX_DOUBLES, "order-3 shape tables must not be staged in LDS by the constitutive launch");
static_assert(sizeof(double) * ((size_t)27 * 3 * 27 + (size_t)EXA_STASH_DOUBLES + 8 * ecmdev::NSLIP) <= 65536, "dynamic LDS of k_model_setup exceeds 64 KB");
static_assert(STG_G + 192 <= ecmdev::ST_SLOTS * 64 && 64 * (RS_SV + RS_S) <= ecmdev::ST_SLOTS * 64 && 32 * RS_T <= 64 * ecmdev::ST_EPI_E, "the staged rows fit a wave's stash region (tangent rows below the parking slots)");
// stg8: staged trilinear launch (k_model_setup, GSTG): the table lives in the waves' stages
static size_t model_lds_bytes(const exa_ctx* ctx, bool km, bool p2f, bool qb, int tail_mode, bool lvec8, bool stg8 = false) {
   const int nrow = (qb && !tail_mode) ? EXA_MODEL_BS / 64 : ctx->Q;
   const bool srow = lvec8 && qb && !tail_mode;      // k_model_setup, SROW: the wave's shape row comes through scalar loads
   const size_t rows = (p2f || srow || stg8 || !exa_g_in_lds(ctx->n, nrow)) ? 0 : (size_t)ctx->n * 3 * nrow;
   return sizeof(double) * (rows + (size_t)EXA_STASH_DOUBLES + (km ? (size_t)8 * ecmdev::NSLIP : (size_t)0));
}

static bool model_split(const exa_ctx* ctx) { return ctx->newton_cap > 0 && ctx->tail_dev != nullptr; }   // the coming launch sequence hands points over
template <typename Go>
static void launch_levels(exa_ctx* ctx, int64_t nb, Go&& go) {
   const int NOCAP = 1 << 30;
   const bool split = model_split(ctx);
   if (!split) { go(nb, NOCAP, ctx->tail_dev, 0, (int*)nullptr, (const double*)nullptr, (double*)nullptr); return; }
   const bool two = ctx->newton_cap2 > ctx->newton_cap && ctx->tail2_dev != nullptr && ctx->resume_dev[0] && ctx->resume_dev[1];
   const int64_t nbt = (ctx->P + EXA_MODEL_BS - 1) / EXA_MODEL_BS;
   go(nb, ctx->newton_cap, ctx->tail_dev, 0, ctx->tail_dev, (const double*)nullptr, ctx->resume_dev[0]);
   go(nbt, two ? ctx->newton_cap2 : NOCAP, ctx->tail_dev, 1, two ? ctx->tail2_dev : ctx->tail_dev, (const double*)ctx->resume_dev[0], two ? ctx->resume_dev[1] : (double*)nullptr);
   if (two) go(nbt, NOCAP, ctx->tail2_dev, 1, ctx->tail2_dev, (const double*)ctx->resume_dev[1], (double*)nullptr);
}

// Kocks-Mecking sets with thermal-activation exponents p == q == 1 (the shipped sets) run the instantiation that has the two exponents
// compiled in (ecmdev::KIN_PQ1: same arithmetic, no pow() code); EXA_KM_PQ1=off keeps the general instantiation for A/B runs
static bool km_pq1(const exa_ctx* ctx) {
   const char* e = std::getenv("EXA_KM_PQ1");   // read per launch: the tests flip it inside one process
   // (the instantiation has the short-series logarithm of the power-law tail compiled in: ecm_device.hpp, kmbald_gdot4)
   return !(e && std::strcmp(e, "off") == 0) && ctx->mp.p == 1.0 && ctx->mp.q == 1.0 && ctx->mp.xn_int == 0 && ctx->mp.t_min >= 0.75 && ctx->mp.t_max <= 1.25;
}

// Voce sets whose power-law exponent 1/m - 1 is 49 (m = 0.02: the shipped sets) run the instantiation with the exponent compiled in
// (ecmdev::KIN_XN49: same multiplication chain, no run-time choice among the power forms inside every evaluation); EXA_VOCE_XN_CT=off keeps the
// general instantiation for A/B runs.  Element-blocked fused launches only (the driver's routes).
static bool voce_xn49(const exa_ctx* ctx) {
   const char* e = std::getenv("EXA_VOCE_XN_CT");
   return !(e && std::strcmp(e, "off") == 0) && ctx->mp.xn_int == 49;
}

// The unsplit Voce record launches run the entry without the tail-split arguments (k_model_setup_rec_nt: same arithmetic, same bits);
// EXA_MODEL_POLICY=off keeps the generic kernel for A/B runs
static bool model_policy() {
   const char* e = std::getenv("EXA_MODEL_POLICY");   // read per launch: the tests flip it inside one process
   return !(e && std::strcmp(e, "off") == 0);
}

