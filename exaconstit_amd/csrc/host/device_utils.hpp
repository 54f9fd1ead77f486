// Small host-side utilities of the stand-alone driver: RAII device buffers and the vector-kernel launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

namespace exa_host {

constexpr int DOT_BLOCKS = 1024;

inline void hip_check(hipError_t e, const char* what) {
   if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
#define EXA_HC(call) ::exa_host::hip_check((call), #call)

template <typename T>
struct DevBuf {
   T* p = nullptr; size_t n = 0;
   DevBuf() = default;
   explicit DevBuf(size_t n_) { alloc(n_); }
   DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
   DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
   DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; } return *this; }
   ~DevBuf() { release(); }
   void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
   void alloc(size_t n_) { release(); n = n_; if (n) EXA_HC(hipMalloc(&p, sizeof(T) * n)); }
   void zero(hipStream_t s = nullptr) { if (n) EXA_HC(hipMemsetAsync(p, 0, sizeof(T) * n, s)); }
   void upload(const T* h, size_t cnt, hipStream_t s = nullptr) { EXA_HC(hipMemcpyAsync(p, h, sizeof(T) * cnt, hipMemcpyHostToDevice, s)); EXA_HC(hipStreamSynchronize(s)); }
   void upload(const std::vector<T>& h, hipStream_t s = nullptr) { if (n < h.size()) alloc(h.size()); if (!h.empty()) upload(h.data(), h.size(), s); }
   void download(T* h, size_t cnt, hipStream_t s = nullptr) const { EXA_HC(hipMemcpyAsync(h, p, sizeof(T) * cnt, hipMemcpyDeviceToHost, s)); EXA_HC(hipStreamSynchronize(s)); }
   std::vector<T> to_host(hipStream_t s = nullptr) const { std::vector<T> h(n); if (n) download(h.data(), n, s); return h; }
   void copy_from(const DevBuf<T>& o, hipStream_t s = nullptr) { EXA_HC(hipMemcpyAsync(p, o.p, sizeof(T) * o.n, hipMemcpyDeviceToDevice, s)); }
   void swap(DevBuf<T>& o) { std::swap(p, o.p); std::swap(n, o.n); }
};

void vk_poison_if_failed(const int* fail_count, double* sum, double* count_out, hipStream_t s);
void vk_update_coords(int64_t n, const double* xb, const double* v, double dt, double* xe, hipStream_t s);
void vk_mask_zero(int64_t n, const uint8_t* m, double* y, hipStream_t s);
void vk_mask_set(int64_t n, const uint8_t* m, const double* val, double* y, hipStream_t s);
void vk_mask_one(int64_t n, const uint8_t* m, double* y, hipStream_t s);
void vk_axpby(int64_t n, double a, const double* x, double b, double* y, hipStream_t s);
void vk_jacobi_setup(int64_t n, const uint8_t* m, const double* diag, int identity, double* dinv, hipStream_t s);
void vk_pointwise(int64_t n, const double* a, const double* b, double* y, hipStream_t s);
void vk_fill_if(int64_t n, const double* flag, double val, double* y, hipStream_t s);
void vk_dot(int64_t n, int64_t nn, const double* w, const double* a, const double* b, const double* flag, double* partial, double* out, hipStream_t s);
void vk_cg_init(double* S, double rel, double abs_, hipStream_t s);
void vk_cg_den(double* S, hipStream_t s);
void vk_cg_beta(double* S, int max_iter, hipStream_t s);
void vk_cg_step1(int64_t n, int64_t nn, double* S, const double* w, const double* dinv, const double* d, double* x, double* r, double* z, double* partial, bool ident,
                 bool fuse_beta, int max_iter, hipStream_t s, const double* partialD = nullptr);   // partialD: consumer-side reduction of the denominator (vec_kernels.hip)
// single-reduction PCG (more than one rank): see vec_kernels.hip
void vk_cg2_init(double* S, double rel, double abs_, hipStream_t s);
void vk_cg2_scalars(double* S, int max_iter, hipStream_t s);
void vk_cg2_update(int64_t n, const double* S, const double* dinv, double* x, double* r, double* u, double* p, double* sv, double* q, bool ident, hipStream_t s);
void vk_cg2_dots(int64_t n, int64_t nn, const double* w, const uint8_t* m, const double* r, const double* u, double* sv, const double* flag, double* partial, double* out2,
                 bool ident, hipStream_t s);
void vk_cg_step2z(int64_t n, double* S, double* z, const double* r, double* d, bool ident, hipStream_t s, const double* partialN = nullptr, int max_iter = 0);   // ... and z = 0 for the accumulating operator action; partialN: consumer-side reduction of (r, z)
void vk_dot_partial(int64_t n, int64_t nn, const double* w, const double* a, const double* b, const double* flag, double* partial, hipStream_t s);   // partial sums only (their consumer reduces them)
void vk_mask_dot(int64_t n, int64_t nn, const double* w, const uint8_t* m, const double* a, double* b, const double* flag, double* partial, double* out, hipStream_t s,
                 double* fuse_den_S = nullptr);
// GMRES (gmres_kernels.hip, ../gmres_slots.hpp).  S: the device record; V: basis vectors at a fixed stride; vectors and stride at
// multiples of 16 bytes; gate 0: leave when FLAG is set, 1: also unless a second Gram-Schmidt pass was decided, 2: run regardless
constexpr int GM_BLOCKS = 1024;   // most blocks of a multi-dot: rows of its partial-sum table (gmres::MAXK + 2 columns)
struct GmStage {   // what the one-block scalar kernel does after summing reduce_cols columns of the table into the record
   enum Kind : int { REDUCE = 0, START, RESTART, COEF, NORM, SOLVE };
   int stage = REDUCE, reduce_cols = 0;
   int col = 0;                            // column of H at work
   int j0 = 0, k = 0;                      // COEF: RED[0 .. k) are the coefficients against v_j0 ... and go to (accumulate: are added to) rows j0 ... of the column
   int accumulate = 0, with_norm = 0;      // with_norm: RED[k] is |w|^2 before the pass
   int gate_reorth = 0;                    // a launch of the second pass
   int decide = 0;                         // NORM: 0 finish the column, 1 second pass on the criterion, 2 always
   int column_update = 1;                  // NORM: 0 only h_i+1,i (the orthogonalisation probe)
   int max_iter = 0, force = 0;
   double rel_tol = 0.0, abs_tol = 0.0;    // START
};
int gm_chunk();
unsigned gm_blocks(int64_t n);
void gm_multidot(int64_t n, int64_t nn, const double* wgt, const double* V, int64_t stride, int j0, int k, const double* w, bool with_norm, const double* S, int gate,
                 double* table, hipStream_t s);
void gm_multiaxpy(int64_t n, int64_t nn, const double* wgt, const double* V, int64_t stride, int j0, int k, const double* S, int coef, double sign, double* w, int gate,
                  double* table /* may be null */, hipStream_t s);
void gm_scale(int64_t n, double* dst, const double* src, const double* dinv /* may be null */, const double* S, int slot /* < 0: none */, hipStream_t s);
void gm_resid(int64_t n, double* dst, const double* b, const double* t, const double* dinv /* may be null */, const double* S, hipStream_t s);
void gm_scalar(double* S, const double* table, int nb, const GmStage& a, hipStream_t s);
void vk_min3(int64_t nn, const double* x, double* partial /*>= DOT_BLOCKS*/, double* out3, hipStream_t s);
void vk_vgrad_velocity(int64_t nn, const uint8_t* m, const double* x, const double* org3_dev, const double* L9_host, double* v, hipStream_t s);
void vk_qf_eb64_to_aos(int W, int Q, int64_t E, const double* src_eb64, double* dst_aos, hipStream_t s);   // (W, Q, E) <- [block][q][W][lane]
void vk_max_abs_diff(int64_t n, const double* a, const double* b, double* out3_dev /* max |a-b|, max |a|, (u64) differing entries of the skipped component */, hipStream_t s, int W = 0, int skip = -1);
void vk_pack(int64_t n, const int32_t* idx, const double* y, double* buf, hipStream_t s);
void vk_unpack_add(int64_t n, const int32_t* idx, const double* buf, double* y, hipStream_t s);
// periodic boundary conditions (periodic_kernels.hip).  Device table of the local periodic groups, passed by value: n2 / n4 / n8 groups
// of 2 / 4 / 8 images, each size class member-major (image j of group g of a class of n groups at base + j n + g), first image = representative
struct PeriodicTable { const int32_t* idx = nullptr; int n2 = 0, n4 = 0, n8 = 0; int groups() const { return n2 + n4 + n8; } };
void vk_periodic_sum(const PeriodicTable& T, int64_t nn, double* y, const double* flag, bool bcast, hipStream_t s);   // y(image) <- group sum in table order (bcast: <- y(representative))
void vk_periodic_jump(const PeriodicTable& T, int64_t nn, const double* x, const double* L9_host, double* v, hipStream_t s);   // v(image) = v(rep) + L (x(image) - x(rep))
void vk_periodic_affine_add(int64_t nn, const double* x, const double* org3_dev, const double* L9_host, double* v, hipStream_t s);   // v += L (x - org) on every node
void vk_periodic_fluct(int64_t nn, const double* rep_w, const double* x, const double* L9_host, const double* v, double* t, hipStream_t s);      // t = rep_w (v - L x)
// mixed loading.  img / code: the nodes on the top faces with their offset codes (bit d: one period up in direction d, bit 3: a corner);
// face: the three top-face node lists back to back, list d at [foff[d], foff[d + 1]), worked on by the blocks [fblk[d], fblk[d + 1]) of 256 nodes;
// ctrl: local ids of c_0, c_1, c_2, c_3 (-1: another rank's); free_bits: bit 3 i + d = H_id is an unknown
struct MixedTable { const int32_t* img = nullptr; const uint8_t* code = nullptr; int nimg = 0; const int32_t* face = nullptr; int foff[4] = { 0, 0, 0, 0 }, fblk[4] = { 0, 0, 0, 0 };
                    int32_t ctrl[4] = { -1, -1, -1, -1 }; uint32_t free_bits = 0; };
void vk_periodic_expand(const MixedTable& M, int64_t nn, const double* in, const double* h12, double* out, const double* flag, bool constrained, hipStream_t s);
void vk_gather_slots(const int32_t* idx_host, int n /* <= 24 */, const double* src, double* out, hipStream_t s);   // out[k] = src[idx[k]], 0 where idx[k] < 0
void vk_face_resultants(const MixedTable& M, int64_t nn, const double* y, const double* flag, double* part /* 3 fblk[3] */, hipStream_t s);
void vk_periodic_sum_controls(const PeriodicTable& T, const MixedTable& M, int64_t nn, double* y, const double* flag, const double* part, double* f9, hipStream_t s);
void vk_translate(int64_t nn, const double* t3_host, double* v, hipStream_t s);   // v += t on every node
void vk_face_combine(const MixedTable& M, int64_t nn, const double* part, double* f9, double* y, const double* flag, hipStream_t s);
void vk_periodic_unfluct(int64_t nn, const uint8_t* surf, const double* x, const double* L9_host, const double* t, double* v, hipStream_t s);   // v = t + L x where surf

}  // namespace exa_host
