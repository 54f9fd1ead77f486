// Per-grain averages (gfx950): deterministic segmented reductions of the per-element rows of exa_element_fields (include/exaconstit_hip.h)
// over the elements of each grain.
//   pass 1: per grain the 39 sums  V, count, V sigma (6), V eps_s (6), V eps_x (6), V (EffPlasticStrain, DpEff, Hardness), V ShearRate (12),
//           V s q (4), with eps_s = R(q) eps_x R(q)^T (R = quat_to_mat, crystal -> sample) and s = sign(q . q_ref) (+1 at 0)
//   pass 2: given the grain means qbar: sum V theta and max theta, theta = 2 atan2(|d_vec|, |d_0|) (degrees), d = conj(qbar) (x) q
// Design (HBM-bound: the rows are 296 bytes each, read once per pass).  The elements are taken in a grain-sorted order (exa_grain_plan, built
// once per grain map), cut into 64-element chunks, one chunk per 64-lane block:
//   1. the chunk's 64 rows are staged through LDS with wave-wide loads (stage_rows, analysis_device.hpp: the rows' leading columns, dense), so
//      every load instruction reads 512 contiguous-by-row bytes (whole cache lines) instead of one 8-byte piece of 64 different rows;
//   2. lane r turns staged row r into its K values (39 in pass 1, 2 in pass 2) and writes them back to LDS as a [64][K] tile;
//   3. lane k < K walks the tile's rows in order and sums column k per segment (a run of equal grain), flushing at every segment change.
// A segment wholly inside the chunk is final: row gid of the dense output.  A chunk's first and last segment may continue into the
// neighbouring chunks: their partials go to the item list of the next level, in chunk order, where the same kernel reduces them again
// (items instead of gathered rows).  Every item list is at most 2 / 64 of the one before, so the levels stay few (4 at 2M elements) and the
// work is O(E) for any grain sizes: one grain of the whole mesh, one grain per element or anything between.  No atomics, a fixed order of
// every sum given the sorted order: every launch on the same data gives the same bits, whatever the grid.
#include "analysis_device.hpp"
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

using namespace exa_analysis;

namespace {

constexpr int NF = EXA_NFIELDS;
constexpr int K1 = EXA_GRAIN_NSUMS, K2 = 2;
constexpr int CH = 64;                 // elements (items) per chunk = threads per block
constexpr int P2_COLS = EXA_F_ORIENTATION + 4;   // pass 2 reads columns 0 .. 30 (volume .. orientation)

// plan (int32): [0] L levels, [1] the largest grain id, [2 .. 2 + L) n_l items per level (n_0 = E), then order[n_0] and per level
// row_l[n_l] (grain id - 1 of every item: a segment is a run of equal rows) and slots_l[2 nch_l] (item slot of the next level for the chunk's
// first / last segment, -1: final here)
struct PlanView {
   int L = 0, gmax = 0; std::vector<int64_t> n, seg_off, slot_off, work_off; int64_t order_off = 0;
   explicit PlanView(const int32_t* p) {
      L = p[0]; gmax = p[1];
      int64_t o = 2 + L;
      n.resize(L); for (int l = 0; l < L; l++) n[l] = p[2 + l];
      order_off = o; o += L > 0 ? n[0] : 0;
      seg_off.resize(L); slot_off.resize(L); work_off.assign(L + 1, 0);
      for (int l = 0; l < L; l++) { seg_off[l] = o; o += n[l]; slot_off[l] = o; o += 2 * ((n[l] + CH - 1) / CH); }
      for (int l = 1; l < L; l++) work_off[l + 1] = work_off[l] + n[l];   // items of level l start at work_off[l] (x K doubles)
   }
};

__device__ __forceinline__ double qdot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]; }

// PASS 1 / 2; GATHER: level 0 (rows of fields through the sorted order) or a higher level (K-value items, contiguous)
template <int PASS, bool GATHER>
__global__ __launch_bounds__(CH) void k_grain_chunk(const int64_t n, const double* __restrict__ src, const int32_t* __restrict__ order,
                                                    const int32_t* __restrict__ seg, const int32_t* __restrict__ slots,
                                                    const double* __restrict__ quats, const int G, double* __restrict__ items, double* __restrict__ out) {
   constexpr int K = PASS == 1 ? K1 : K2;
   constexpr int NC = GATHER ? (PASS == 1 ? NF : P2_COLS) : K;   // staged columns of every row
   constexpr int SRC_LD = GATHER ? NF : K;
   constexpr int TILE = (NC > K ? NC : K) * CH;
   __shared__ double sm[TILE];
   __shared__ int32_t s_seg[CH], s_row[CH];
   const BlockView bv(n);
   const int lane = bv.lane, nv = bv.nv;
   const int64_t c = blockIdx.x, base = bv.base;
   const int slot_first = slots[2 * c], slot_last = slots[2 * c + 1];   // block-uniform, issued first
   const int my_row = lane < nv ? seg[base + lane] : -1;
   s_seg[lane] = my_row;
   if constexpr (GATHER) s_row[lane] = lane < nv ? order[base + lane] : 0;
   double qr[4] = { 1.0, 0.0, 0.0, 0.0 };   // the grain's reference (pass 1) or mean (pass 2) orientation, loaded beside the staging
   if constexpr (GATHER) {
      if (lane < nv) for (int k = 0; k < 4; k++) qr[k] = quats[4 * (int64_t)my_row + k];
   }
   __syncthreads();
   // 1. stage rows 0 .. nv-1 (NC leading columns each) as the flat [nv][NC] tile: all NC loads are issued before the first LDS write (a load
   //    guarded by r < nv and stored at once would wait for each load in turn); the rows are the gathered order's or the item list's
   stage_rows<NC, NC>(sm, nv, lane, src, [&](int r) { return (GATHER ? (int64_t)s_row[r] : base + r) * SRC_LD; }, IdentityCol());
   __syncthreads();
   // 2. per-element values (level 0 only; items are values already)
   if constexpr (GATHER) {
      double v[K];
      if (lane < nv) {
         const double* f = sm + lane * NC;
         const double V = f[EXA_F_VOLUME];
         const double q[4] = { f[EXA_F_ORIENTATION], f[EXA_F_ORIENTATION + 1], f[EXA_F_ORIENTATION + 2], f[EXA_F_ORIENTATION + 3] };
         if constexpr (PASS == 1) {
            v[0] = V; v[1] = 1.0;
#pragma unroll
            for (int k = 0; k < 6; k++) v[2 + k] = V * f[EXA_F_STRESS + k];
            const double* e = f + EXA_F_XTALELASTICSTRAIN;
            const double T[3][3] = { { e[0], e[5], e[4] }, { e[5], e[1], e[3] }, { e[4], e[3], e[2] } };
            double R[9]; ecmdev::quat_to_mat(q, R);   // row-major
            double M[3][3];   // R T
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
               for (int b = 0; b < 3; b++) M[a][b] = R[3 * a] * T[0][b] + R[3 * a + 1] * T[1][b] + R[3 * a + 2] * T[2][b];
            auto es = [&](int a, int b) { return M[a][0] * R[3 * b] + M[a][1] * R[3 * b + 1] + M[a][2] * R[3 * b + 2]; };   // (R T R^T)_ab
            v[8] = V * es(0, 0); v[9] = V * es(1, 1); v[10] = V * es(2, 2); v[11] = V * es(1, 2); v[12] = V * es(0, 2); v[13] = V * es(0, 1);
#pragma unroll
            for (int k = 0; k < 6; k++) v[14 + k] = V * e[k];
            v[20] = V * f[EXA_F_EFFPLASTICSTRAIN]; v[21] = V * f[EXA_F_DPEFF]; v[22] = V * f[EXA_F_HARDNESS];
#pragma unroll
            for (int k = 0; k < 12; k++) v[23 + k] = V * f[EXA_F_SHEARRATE + k];
            const double sV = qdot(q, qr) >= 0.0 ? V : -V;
#pragma unroll
            for (int k = 0; k < 4; k++) v[35 + k] = sV * q[k];
         } else {
            // d = conj(qbar) (x) q: d_0 = qbar . q, d_vec = qbar_0 q_v - q_0 qbar_v - qbar_v x q_v
            const double d0 = qdot(qr, q);
            const double d1 = qr[0] * q[1] - q[0] * qr[1] - (qr[2] * q[3] - qr[3] * q[2]);
            const double d2 = qr[0] * q[2] - q[0] * qr[2] - (qr[3] * q[1] - qr[1] * q[3]);
            const double d3 = qr[0] * q[3] - q[0] * qr[3] - (qr[1] * q[2] - qr[2] * q[1]);
            const double th = 2.0 * atan2(sqrt(d1 * d1 + d2 * d2 + d3 * d3), fabs(d0)) * RAD2DEG;
            v[0] = V * th; v[1] = th;
         }
      }
      __syncthreads();   // every lane has read its staged row before the [nv][K] tile overwrites the staging area
      if (lane < nv) {
#pragma unroll
         for (int k = 0; k < K; k++) sm[lane * K + k] = v[k];
      }
      __syncthreads();
   }
   // 3. column k, rows in order, one running value per segment; the column is read 8 rows at a time so that the LDS reads overlap
   if (lane < K) {
      const bool is_max = PASS == 2 && lane == 1;
      auto flush = [&](int row, bool first, bool last, double val) {
         int slot = first ? slot_first : -1;
         if (slot < 0 && last) slot = slot_last;
         if (slot >= 0) items[(int64_t)slot * K + lane] = val;
         else if (PASS == 1) out[(int64_t)row * K + lane] = val;
         else out[(int64_t)lane * G + row] = val;   // pass 2: planar [2][G]
      };
      int s = s_seg[0], r0 = 0;
      double acc = 0.0;
      for (int b = 0; b < nv; b += 8) {
         double x[8]; int t[8];
#pragma unroll
         for (int u = 0; u < 8; u++) { x[u] = sm[((b + u) & (CH - 1)) * K + lane]; t[u] = s_seg[(b + u) & (CH - 1)]; }
#pragma unroll
         for (int u = 0; u < 8; u++) {
            const int r = b + u;
            if (r >= nv) break;
            if (t[u] != s) { flush(s, r0 == 0, false, acc); s = t[u]; r0 = r; acc = x[u]; }
            else if (r == 0) acc = x[u];
            else acc = is_max ? fmax(acc, x[u]) : acc + x[u];
         }
      }
      flush(s, r0 == 0, true, acc);
   }
}

template <int PASS>
int launch_levels(exa_ctx* ctx, const PlanView& P, const double* fields, const int32_t* plan_dev, const double* quats, int G, double* work, double* out, hipStream_t s) {
   constexpr int K = PASS == 1 ? K1 : K2;
   for (int l = 0; l < P.L; l++) {
      const int64_t nch = (P.n[l] + CH - 1) / CH;
      const int32_t* seg = plan_dev + P.seg_off[l];
      const int32_t* slots = plan_dev + P.slot_off[l];
      double* items_out = work + K * P.work_off[l + 1];
      if (l == 0)
         hipLaunchKernelGGL((k_grain_chunk<PASS, true>), dim3((unsigned)nch), dim3(CH), 0, s, P.n[0], fields, plan_dev + P.order_off, seg, slots, quats, G,
                            items_out, out);
      else
         hipLaunchKernelGGL((k_grain_chunk<PASS, false>), dim3((unsigned)nch), dim3(CH), 0, s, P.n[l], (const double*)(work + K * P.work_off[l]), (const int32_t*)nullptr,
                            seg, slots, quats, G, items_out, out);
   }
   EXA_HIP_CHECK(ctx, hipGetLastError());
   return EXA_OK;
}

}  // namespace

extern "C" int exa_grain_plan(int64_t E, const int32_t* grain_of_elem, int32_t* plan, int64_t plan_cap, int64_t* plan_len, int64_t* work_doubles) {
   if (E < 0 || (E > 0 && !grain_of_elem) || E > INT32_MAX) return EXA_ERR_ARG;
   for (int64_t e = 0; e < E; e++) if (grain_of_elem[e] < 1) return EXA_ERR_ARG;
   std::vector<int32_t> order((size_t)E);
   std::iota(order.begin(), order.end(), 0);
   std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return grain_of_elem[a] < grain_of_elem[b]; });
   std::vector<int32_t> seg((size_t)E);
   int32_t gmax = 0;
   for (int64_t i = 0; i < E; i++) { seg[i] = grain_of_elem[order[i]] - 1; gmax = std::max(gmax, seg[i] + 1); }
   std::vector<std::vector<int32_t>> segs, slots;
   while (!seg.empty()) {
      const int64_t n = (int64_t)seg.size(), nch = (n + CH - 1) / CH;
      std::vector<int32_t> next, sl((size_t)(2 * nch), -1);
      for (int64_t c = 0; c < nch; c++) {
         const int64_t a = c * CH, b = std::min(n, a + CH) - 1;
         const bool before = a > 0 && seg[a - 1] == seg[a], after = b + 1 < n && seg[b + 1] == seg[b];
         if (seg[a] == seg[b]) {
            if (before || after) { sl[2 * c] = sl[2 * c + 1] = (int32_t)next.size(); next.push_back(seg[a]); }
         } else {
            if (before) { sl[2 * c] = (int32_t)next.size(); next.push_back(seg[a]); }
            if (after) { sl[2 * c + 1] = (int32_t)next.size(); next.push_back(seg[b]); }
         }
      }
      segs.push_back(std::move(seg)); slots.push_back(std::move(sl));
      seg = std::move(next);
   }
   const int L = (int)segs.size();
   std::vector<int32_t> p;
   p.push_back(L); p.push_back(gmax);
   for (int l = 0; l < L; l++) p.push_back((int32_t)segs[l].size());
   p.insert(p.end(), order.begin(), order.end());
   int64_t items = 0;
   for (int l = 0; l < L; l++) {
      p.insert(p.end(), segs[l].begin(), segs[l].end()); p.insert(p.end(), slots[l].begin(), slots[l].end());
      if (l > 0) items += (int64_t)segs[l].size();
   }
   if (plan_len) *plan_len = (int64_t)p.size();
   if (work_doubles) *work_doubles = (int64_t)K1 * items;
   if (plan) {
      if (plan_cap < (int64_t)p.size()) return EXA_ERR_ARG;
      std::copy(p.begin(), p.end(), plan);
   }
   return EXA_OK;
}

extern "C" int exa_grain_sums(exa_ctx* ctx, int pass, const double* fields_dev, const int32_t* plan_host, const int32_t* plan_dev, int G, const double* quats_dev,
                              double* work_dev, double* out_dev, exa_stream str) {
   if (!ctx) return EXA_ERR_ARG;
   if (pass != 1 && pass != 2) { ctx->err = "exa_grain_sums: pass must be 1 or 2"; return EXA_ERR_ARG; }
   if (!plan_host || !plan_dev || !out_dev || G < 1) { ctx->err = "exa_grain_sums: a plan (host and device), G >= 1 and an output are required"; return EXA_ERR_ARG; }
   const PlanView P(plan_host);
   if (P.L == 0) return EXA_OK;   // no local elements: the output stays as the caller filled it
   if (P.n[0] != (int64_t)ctx->E) { ctx->err = "exa_grain_sums: the plan is not one of the context's elements"; return EXA_ERR_ARG; }
   if (!fields_dev || !quats_dev || (P.L > 1 && !work_dev)) { ctx->err = "exa_grain_sums: fields, orientations and (several levels) a workspace are required"; return EXA_ERR_ARG; }
   if (P.gmax > G) { ctx->err = "exa_grain_sums: a grain id of the plan exceeds G"; return EXA_ERR_ARG; }
   hipStream_t s = reinterpret_cast<hipStream_t>(str);
   return pass == 1 ? launch_levels<1>(ctx, P, fields_dev, plan_dev, quats_dev, G, work_dev, out_dev, s)
                    : launch_levels<2>(ctx, P, fields_dev, plan_dev, quats_dev, G, work_dev, out_dev, s);
}
