// The periodic cell of a generated RVE on the device with its mixed stress / velocity-gradient loading: the group table
// in the layout of periodic_kernels.hip, the sum of an L-vector over the images and the ranks, the expansion of the reduced unknowns, the jump of
// the velocity across the cell, the face resultants and the control values at the corners c_0 .. c_3.  NonlinearMechOperator owns one on a
// periodic partition (null otherwise) and is the only one that builds it; it knows the partition, the transport and the stream it was given,
// nothing of the operator: the essential mask, the coordinates and a scratch L-vector arrive with the calls that need them.
#pragma once
#include "comm.hpp"
#include "device_utils.hpp"
#include "mesh.hpp"

namespace exa_host {

class PeriodicCell {
 public:
   PeriodicCell(const Partition& part, Comm& comm, hipStream_t stream) : part_(part), comm_(comm), stream_(stream) {}
   // device tables of the partition as it is now (Partition::make_periodic): the group table and, for several ranks, the nodal arrays of Jump and
   // OwnerBits; mixed partitions: image, face and control tables.  The free bits and the resultants survive a rebuild.
   void Build();
   // The sum over the local periodic images (one launch), then over the ranks.  flag: the PCG's done flag (the launches are no-ops once it is set).
   // Mixed loading, raw = true (y holds raw element contributions): the nine face resultants are taken first and the free ones are written to
   // their control slots after the sums; raw = false: the sums alone.
   void Sum(double* y, const double* flag, bool raw);
   // Several ranks: every holder of a dof takes the owner's bits of an assembled vector (the residual, see periodic.hip); one rank: nothing.
   void OwnerBits(double* y);
   // mixed loading: bit 3 i + d = H_id is an unknown
   uint32_t free_bits() const { return mix_tab_.free_bits; }
   void set_free_bits(uint32_t bits) { mix_tab_.free_bits = bits; }
   // full nodal field P x of the stored vector x in the cell's own L-vector: masked with ess_mask first when it is given (the constrained action)
   const double* Expand(const double* x, const double* flag, const uint8_t* ess_mask);
   void ExpandCorrection(double* c, const uint8_t* ess_mask);   // the same in place: the PCG solution before Newton adds it to the velocity
   void KeepResultants();                    // the resultants of the last Sum(raw = true) become those of the last residual (mixed partitions)
   void ReadResultants(double* f9_host);     // face resultants of the last residual evaluation (all ranks' sum); waits for the stream
   // values of an L-vector at the nodes c_0 .. c_3 (12 numbers, node by node), summed over the ranks; waits for the stream
   void CornerValues(const double* v, double* out12_host);
   // v(image) - v(representative) = L (x_cur(image) - x_cur(representative)) on every periodic group (UpdateVelocity); scratch: an L-vector
   void Jump(const double* L9, const double* x_cur, double* v, double* scratch);
 private:
   const Partition& part_; Comm& comm_; hipStream_t stream_;
   int nn_ = 0, nd_ = 0;
   int32_t slot(int k, int c) const { return mix_tab_.ctrl[k] >= 0 ? mix_tab_.ctrl[k] + nn_ * c : -1; }   // dof of component c of c_k (-1: another rank's)
   // the group table, and for several ranks 1 / holders on the node that carries the canonical id and the box-surface mask
   DevBuf<int32_t> per_idx_; PeriodicTable per_tab_; DevBuf<double> per_repw_; DevBuf<uint8_t> per_surf_, per_notown_;
   // mixed loading: tables, the scratch L-vector of the expanded input, block partials of the resultants, { v(c_0), H } of the input (several ranks),
   // resultants of the last action / of the last residual
   MixedTable mix_tab_; DevBuf<int32_t> mix_img_, mix_face_; DevBuf<uint8_t> mix_code_; DevBuf<double> mix_x_, mix_part_, mix_h_, mix_f_, mix_res_;
};

}  // namespace exa_host
