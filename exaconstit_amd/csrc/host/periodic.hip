// PeriodicCell (host/periodic.hpp): tables and launch sequences of the periodic cell and of mixed loading; the kernels are periodic_kernels.hip.
#include "periodic.hpp"
#include <algorithm>

namespace exa_host {

// Periodic partition (Partition::make_periodic): the group table in the layout of periodic_kernels.hip and, for several ranks, the two nodal
// arrays of the jump through the fluctuation (Jump) and the owner mask (OwnerBits)
void PeriodicCell::Build() {
   const Partition& part = part_;
   nn_ = part.NN; nd_ = 3 * nn_;
   const int n2 = part.grp_count[0], n4 = part.grp_count[1], n8 = part.grp_count[2];
   std::vector<int32_t> idx(part.grp_nodes.size());
   size_t base = 0; int g0 = 0;
   for (int cls = 0; cls < 3; cls++) {   // CSR (group-major) -> member-major within each size class
      const int m = 2 << cls, n = part.grp_count[cls];
      for (int g = 0; g < n; g++) for (int j = 0; j < m; j++) idx[base + (size_t)j * n + g] = part.grp_nodes[(size_t)part.grp_off[g0 + g] + j];
      base += (size_t)m * n; g0 += n;
   }
   per_idx_.release(); if (!idx.empty()) per_idx_.upload(idx);
   per_tab_.idx = per_idx_.p; per_tab_.n2 = n2; per_tab_.n4 = n4; per_tab_.n8 = n8;
   if (comm_.nranks > 1) {
      std::vector<double> rw((size_t)nn_, 0.0); std::vector<uint8_t> surf((size_t)nn_, 0);
      for (int g = 0; g < nn_; g++) { if (part.node_gid[g] == part.canon[g]) rw[g] = part.weight_node[g]; surf[g] = part.on_box_surface(g) ? 1 : 0; }
      if (part.mixed) for (int g = 0; g < nn_; g++) if (part.is_corner(g)) { rw[g] = 0.0; surf[g] = 0; }   // (the corners take their velocity from the control values: UpdateVelocity)
      per_repw_.upload(rw); per_surf_.upload(surf);
      // the owner of a canonical id: its representative on the lowest rank that holds the id (OwnerBits)
      std::vector<uint8_t> notown((size_t)nd_, 1), lower((size_t)nn_, 0);
      for (const Neighbor& nb : part.nbrs) if (nb.rank < comm_.rank) for (int32_t d : nb.dofs) lower[(size_t)(d % nn_)] = 1;
      std::vector<uint8_t> image((size_t)nn_, 0);      // local images other than the representative
      for (size_t g = 0; g + 1 < part.grp_off.size(); g++) for (int32_t k = part.grp_off[g] + 1; k < part.grp_off[g + 1]; k++) image[(size_t)part.grp_nodes[k]] = 1;
      for (int g = 0; g < nn_; g++) if (!lower[g] && !image[g]) for (int c = 0; c < 3; c++) notown[g + (size_t)nn_ * c] = 0;
      per_notown_.upload(notown);
   }
   if (part.mixed) {
      const uint32_t fb = mix_tab_.free_bits;
      mix_tab_ = MixedTable(); mix_tab_.free_bits = fb;
      mix_img_.release(); mix_code_.release(); mix_face_.release();
      if (!part.img_nodes.empty()) { mix_img_.upload(part.img_nodes); mix_code_.upload(part.img_code); }
      std::vector<int32_t> face;
      for (int d = 0; d < 3; d++) {
         face.insert(face.end(), part.face_nodes[d].begin(), part.face_nodes[d].end());
         mix_tab_.foff[d + 1] = (int)face.size();
         mix_tab_.fblk[d + 1] = mix_tab_.fblk[d] + (int)((part.face_nodes[d].size() + 255) / 256);
      }
      if (!face.empty()) mix_face_.upload(face);
      mix_tab_.img = mix_img_.p; mix_tab_.code = mix_code_.p; mix_tab_.nimg = (int)part.img_nodes.size(); mix_tab_.face = mix_face_.p;
      for (int k = 0; k < 4; k++) mix_tab_.ctrl[k] = part.ctrl_node[k];
      if (mix_x_.n == 0) { mix_x_.alloc(nd_); mix_h_.alloc(12); mix_f_.alloc(9); mix_res_.alloc(9); mix_f_.zero(stream_); mix_res_.zero(stream_); }
      mix_part_.release(); mix_part_.alloc((size_t)std::max(1, 3 * mix_tab_.fblk[3]));
   }
}

void PeriodicCell::Sum(double* y, const double* flag, bool raw) {
   const bool one = !comm_.active();
   const bool mix = part_.mixed && raw;
   if (mix) vk_face_resultants(mix_tab_, nn_, y, flag, mix_part_.p, stream_);
   if (mix && one) { vk_periodic_sum_controls(per_tab_, mix_tab_, nn_, y, flag, mix_part_.p, mix_f_.p, stream_); return; }
   if (mix) { vk_face_combine(mix_tab_, nn_, mix_part_.p, mix_f_.p, nullptr, flag, stream_); comm_.allreduce_sum(mix_f_.p, 9, stream_); }
   vk_periodic_sum(per_tab_, nn_, y, flag, false, stream_);
   if (!one) {
      // the exchange carries the representative of a group: its local sum out, the other ranks' sums added to it, then back to its local images
      comm_.halo_sum(y, stream_);
      vk_periodic_sum(per_tab_, nn_, y, flag, true, stream_);
   }
   if (mix) vk_face_combine(mix_tab_, nn_, nullptr, mix_f_.p, y, flag, stream_);
}

// Several ranks: three or more holders add their contributions in different orders, so their copies of a residual entry differ in the last bits
// of the element forces - which is far above the last bits of a residual near equilibrium, and a part of the right-hand side that differs between
// the copies of a dof is out of the PCG's reach (tight Krylov tolerances then stop at the cap).  Every holder takes the owner's bits: all other
// copies are zeroed and summed again - one non-zero term per dof, an exact sum.
void PeriodicCell::OwnerBits(double* y) {
   if (comm_.nranks == 1) return;
   vk_mask_zero(nd_, per_notown_.p, y, stream_);
   Sum(y, nullptr, false);
}

// x -> P x.  One rank reads the control values from x itself; several ranks gather { x(c_0), H } where they hold them and add them up
// (the first of the two small all-reduces of an action).
const double* PeriodicCell::Expand(const double* x, const double* flag, const uint8_t* ess_mask) {
   // (the copy is not gated by the flag: a finished PCG never reads it)
   EXA_HC(hipMemcpyAsync(mix_x_.p, x, sizeof(double) * nd_, hipMemcpyDeviceToDevice, stream_));
   if (ess_mask) vk_mask_zero(nd_, ess_mask, mix_x_.p, stream_);
   const double* h12 = nullptr;
   if (comm_.nranks > 1) {
      int32_t idx[12];
      for (int c = 0; c < 3; c++) { idx[c] = slot(0, c); for (int d = 0; d < 3; d++) idx[3 + 3 * c + d] = slot(1 + d, c); }
      vk_gather_slots(idx, 12, x, mix_h_.p, stream_);
      comm_.allreduce_sum(mix_h_.p, 12, stream_);
      h12 = mix_h_.p;
   }
   vk_periodic_expand(mix_tab_, nn_, x, h12, mix_x_.p, flag, ess_mask != nullptr, stream_);
   return mix_x_.p;
}

void PeriodicCell::ExpandCorrection(double* c, const uint8_t* ess_mask) {
   const double* f = Expand(c, nullptr, ess_mask);
   EXA_HC(hipMemcpyAsync(c, f, sizeof(double) * nd_, hipMemcpyDeviceToDevice, stream_));
}

void PeriodicCell::KeepResultants() {
   if (part_.mixed) EXA_HC(hipMemcpyAsync(mix_res_.p, mix_f_.p, 9 * sizeof(double), hipMemcpyDeviceToDevice, stream_));
}

void PeriodicCell::ReadResultants(double* f9_host) {
   EXA_HC(hipMemcpyAsync(f9_host, mix_res_.p, 9 * sizeof(double), hipMemcpyDeviceToHost, stream_)); EXA_HC(hipStreamSynchronize(stream_));
}

void PeriodicCell::CornerValues(const double* v, double* out12_host) {
   int32_t idx[12];
   for (int k = 0; k < 4; k++) for (int c = 0; c < 3; c++) idx[3 * k + c] = slot(k, c);
   vk_gather_slots(idx, 12, v, mix_h_.p, stream_);
   comm_.allreduce_sum(mix_h_.p, 12, stream_);
   EXA_HC(hipMemcpyAsync(out12_host, mix_h_.p, 12 * sizeof(double), hipMemcpyDeviceToHost, stream_)); EXA_HC(hipStreamSynchronize(stream_));
}

void PeriodicCell::Jump(const double* L9, const double* x_cur, double* v, double* scratch) {
   if (comm_.nranks == 1) { vk_periodic_jump(per_tab_, nn_, x_cur, L9, v, stream_); return; }
   // several ranks: the images of a node sit on different ranks - the node that carries the canonical id hands its fluctuation v - L x to all of them
   vk_periodic_fluct(nn_, per_repw_.p, x_cur, L9, v, scratch, stream_);
   Sum(scratch, nullptr, false);
   vk_periodic_unfluct(nn_, per_surf_.p, x_cur, L9, scratch, v, stream_);
}

}  // namespace exa_host
