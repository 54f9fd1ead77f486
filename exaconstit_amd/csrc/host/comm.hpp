// Communication of the stand-alone host driver: all-reduces and the halo sum of the shared dofs over one of three transports (comm.hip) - RCCL over
// xGMI (loaded at run time), the inter-process transport of ranks that share ONE device, the in-process loopback group of the tests - and no-ops on a
// plain one-rank run.  (Reference coupling sites: src/mechanics_driver.cpp:312, src/system_driver.cpp:167, src/mechanics_kernels.hpp:119,124.)
#pragma once
#include <memory>
#include <vector>
#include "device_utils.hpp"
#include "mesh.hpp"

namespace exa_host {

struct Transport;    // comm.hip: what differs between RCCL, the shared-device transport and the loopback group
enum class RankOp;   // rank_sync.hpp: SUM, MIN, MAX

class Comm {
 public:
   enum Kind { NONE = 0, RCCL = 1, IPC = 2, LOOPBACK = 3 };   // the numbers exa_driver_comm_info reports
   int rank = 0, nranks = 1;
   Comm();
   ~Comm();
   // force_rccl: run the RCCL calls on a one-rank communicator too (what EXA_FORCE_RCCL=1 selects from the environment)
   void init(int rank_, int nranks_, const void* nccl_unique_id /*128 bytes, identical on all ranks*/, bool force_rccl = false);
   static void get_unique_id(void* out128);
   // inter-process transport for ranks that share a device: an id of that kind, and whether this launch needs it
   static void ipc_unique_id(void* out128);
   static bool want_ipc_transport(int nranks);
   // in-process loopback transport for tests: several ranks (one host thread each) on ONE device
   static void loopback_create(int nranks, void* out128);
   static void loopback_destroy(const void* id128);
   Kind kind() const;
   const char* transport() const { static const char* const name[] = { "none", "rccl", "ipc", "loopback" }; return name[kind()]; }   // for messages
   int reported_ranks() const;            // what the transport itself says (ncclCommCount for RCCL)
   // Does this run take the multi-rank code paths (halo sums, the single-reduction PCG, no captured graph ...)?  Several ranks, or the one-rank
   // communicator of EXA_FORCE_RCCL=1, which runs them and every RCCL call.  Questions about the DATA - are there other ranks whose contributions
   // or agreement are needed? - ask nranks > 1 instead: a forced one-rank run has nobody to add up with.
   bool active() const { return nranks > 1 || force_; }
   void allreduce_sum(double* dev, int n, hipStream_t s);
   void allreduce_min(double* dev, int n, hipStream_t s);
   void allreduce_max(double* dev, int n, hipStream_t s);
   double max_over_ranks(double v);
   void setup_halo(const Partition& part);   // the neighbours' ranks and shared dofs: the plan of every later exchange
   // y(shared dofs) <- sum over all ranks holding them
   void halo_sum(double* y, hipStream_t s);
   // the same in two halves for overlap with work on stream s: begin = pack + exchange on the communication stream once everything
   // enqueued on s so far has finished; end = s waits for the exchange, then adds the received segments
   void halo_begin(double* y, hipStream_t s);
   void halo_end(double* y, hipStream_t s);
   // us per call of the fused 16-byte all-reduce and of a grouped send/recv of `n` doubles to the own rank (one-rank communicator: latency floor of the RCCL calls)
   void microbench(int iters, int n, double* us_allreduce, double* us_sendrecv);
   bool deterministic = false;               // halo contributions added segment by segment (fixed order) instead of one atomic pass
   size_t halo_dofs() const { return seg_off_.back(); }   // doubles this rank sends (= receives) per exchange, all neighbours
   bool selftest() const { return selftest_zero_; }   // EXA_HALO_SELFTEST: the forced one-rank communicator exchanges zeros with itself (Comm::init)
 private:
   void allreduce(double* dev, int n, RankOp op, hipStream_t s);
   void pack_exchange(double* y, hipStream_t s);   // shared dofs of y -> send buffer -> the neighbours' receive buffers, on stream s
   void unpack(double* y, hipStream_t s);
   std::unique_ptr<Transport> tr_;   // null on a plain one-rank run
   bool force_ = false, selftest_zero_ = false;
   // concatenated neighbour segments (segment i = neighbour i): dof lists, send and receive buffers, one allocation each
   std::vector<int> nbr_rank_; std::vector<size_t> seg_off_{ 0 };
   DevBuf<int32_t> idx_all_; DevBuf<double> sbuf_all_, rbuf_all_;
   DevBuf<double> tmp_;
   hipStream_t cs_ = nullptr; hipEvent_t ev_ready_ = nullptr, ev_done_ = nullptr;   // communication stream of halo_begin / halo_end
};

}  // namespace exa_host
