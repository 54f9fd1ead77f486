// Comm (comm.hpp): what all transports share - the concatenated segment plan, pack / unpack, the communication stream of the overlapped halo - and,
// behind one internal interface, the three transports: RCCL, the inter-process transport of ranks that share one device, the in-process loopback group.
#include "comm.hpp"
#include "rank_sync.hpp"
#include <rccl/rccl.h>
#include <atomic>
#include <chrono>
#include <cstring>
#include <thread>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <dlfcn.h>
#include <link.h>

namespace exa_host {

// One rank's exchange plan as a transport sees it: segment i of the send buffer goes to rank nbr[i], segment i of the receive buffer comes from it
// (same dofs in the same order on both sides)
struct Halo {
   const std::vector<int>& nbr; const std::vector<size_t>& off; double* sbuf; double* rbuf;
   size_t count() const { return nbr.size(); }
   size_t cnt(size_t i) const { return off[i + 1] - off[i]; }
   double* sb(size_t i) const { return sbuf + off[i]; }
   double* rb(size_t i) const { return rbuf + off[i]; }
};

// What differs between the transports.  A new one implements these five and gets a branch in Comm::init; Comm's callers see none of it.
struct Transport {
   virtual ~Transport() = default;
   virtual Comm::Kind kind() const = 0;
   virtual int reported_ranks() const = 0;
   virtual void allreduce(double* dev, int n, RankOp op, hipStream_t s) = 0;   // in place
   virtual void halo_plan(const Halo&) {}                                     // once per Comm::setup_halo, every rank
   virtual void exchange(const Halo& h, hipStream_t s) = 0;                    // send segments -> the neighbours' receive segments, on stream s
};

// =====================================================================================================================
// RCCL, loaded at run time so that single-GPU use has no collective-library dependency
// =====================================================================================================================
namespace {
struct RcclApi {
   void* h = nullptr;
   ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
   ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
   ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
   ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
   ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
   ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
   ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
   ncclResult_t (*GroupStart)() = nullptr;
   ncclResult_t (*GroupEnd)() = nullptr;
   const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
RcclApi& rccl() {
   static RcclApi api;
   if (!api.h) {
      // prefer the RCCL already mapped into the process (PyTorch bundles its own copy next to its HIP runtime): two RCCL builds in
      // one process would each bring their own device state
      std::string loaded;
      dl_iterate_phdr([](struct dl_phdr_info* info, size_t, void* out) -> int {
         if (info->dlpi_name && std::strstr(info->dlpi_name, "librccl")) { *static_cast<std::string*>(out) = info->dlpi_name; return 1; }
         return 0; }, &loaded);
      if (!loaded.empty()) api.h = dlopen(loaded.c_str(), RTLD_NOW | RTLD_GLOBAL);
      if (!api.h) for (const char* name : { "librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1" }) { api.h = dlopen(name, RTLD_NOW | RTLD_GLOBAL); if (api.h) break; }
      if (!api.h) throw std::runtime_error(std::string("cannot load RCCL: ") + dlerror());
      auto sym = [&](const char* n) { void* p = dlsym(api.h, n); if (!p) throw std::runtime_error(std::string("RCCL symbol missing: ") + n); return p; };
      api.GetUniqueId = (decltype(api.GetUniqueId))sym("ncclGetUniqueId");
      api.CommInitRank = (decltype(api.CommInitRank))sym("ncclCommInitRank");
      api.CommDestroy = (decltype(api.CommDestroy))sym("ncclCommDestroy");
      api.CommCount = (decltype(api.CommCount))sym("ncclCommCount");
      api.AllReduce = (decltype(api.AllReduce))sym("ncclAllReduce");
      api.Send = (decltype(api.Send))sym("ncclSend");
      api.Recv = (decltype(api.Recv))sym("ncclRecv");
      api.GroupStart = (decltype(api.GroupStart))sym("ncclGroupStart");
      api.GroupEnd = (decltype(api.GroupEnd))sym("ncclGroupEnd");
      api.GetErrorString = (decltype(api.GetErrorString))sym("ncclGetErrorString");
   }
   return api;
}
void nccl_check(ncclResult_t r, const char* what) { if (r != ncclSuccess) throw std::runtime_error(std::string(what) + ": " + rccl().GetErrorString(r)); }

struct RcclTransport final : Transport {
   ncclComm_t comm = nullptr;
   RcclTransport(const void* uid, int rank, int nranks, bool forced) {
      ncclUniqueId id;
      if (uid) std::memcpy(&id, uid, sizeof(id));
      else if (forced) nccl_check(rccl().GetUniqueId(&id), "ncclGetUniqueId");
      else throw std::runtime_error("Comm::init: a RCCL unique id is required for nranks > 1");
      nccl_check(rccl().CommInitRank(&comm, nranks, id, rank), "ncclCommInitRank");
   }
   ~RcclTransport() override { rccl().CommDestroy(comm); }
   Comm::Kind kind() const override { return Comm::RCCL; }
   int reported_ranks() const override { int n = 0; nccl_check(rccl().CommCount(comm, &n), "ncclCommCount"); return n; }
   void allreduce(double* dev, int n, RankOp op, hipStream_t s) override {
      const ncclRedOp_t o = op == RankOp::SUM ? ncclSum : (op == RankOp::MIN ? ncclMin : ncclMax);
      nccl_check(rccl().AllReduce(dev, dev, n, ncclDouble, o, comm, s), "ncclAllReduce");
   }
   void exchange(const Halo& h, hipStream_t s) override {
      nccl_check(rccl().GroupStart(), "ncclGroupStart");
      for (size_t i = 0; i < h.count(); i++) {
         nccl_check(rccl().Send(h.sb(i), h.cnt(i), ncclDouble, h.nbr[i], comm, s), "ncclSend");
         nccl_check(rccl().Recv(h.rb(i), h.cnt(i), ncclDouble, h.nbr[i], comm, s), "ncclRecv");
      }
      nccl_check(rccl().GroupEnd(), "ncclGroupEnd");
   }
};

// =====================================================================================================================
// Host-synchronous reductions: what the loopback and the shared-device transport have in common.  Every rank downloads its contribution, the ranks
// meet, every rank folds all contributions in rank order (deterministic: rank_sync.hpp), they meet again, every rank uploads the result.  The two
// transports differ only in where the contributions lie and how the ranks meet.
// =====================================================================================================================
struct HostSyncTransport : Transport {
   const int rank_, n_;
   const int piece_;   // doubles a rank's slot holds: longer reductions pass through the slots piece by piece (0: any length at once)
   HostSyncTransport(int rank, int nranks, int piece) : rank_(rank), n_(nranks), piece_(piece) {}
   virtual double* slot(int k, int m) = 0;   // rank k's m doubles of the current piece (k == rank_: with room for them)
   virtual void meet() = 0;
   int reported_ranks() const override { return n_; }
   void allreduce(double* dev, int n, RankOp op, hipStream_t s) final {
      if (n_ == 1) return;
      std::vector<double> v((size_t)n);
      EXA_HC(hipMemcpyAsync(v.data(), dev, sizeof(double) * n, hipMemcpyDeviceToHost, s)); EXA_HC(hipStreamSynchronize(s));
      const int piece = piece_ > 0 ? piece_ : n;
      for (int i0 = 0; i0 < n; i0 += piece) {   // every rank in the same order
         const int m = std::min(piece, n - i0);
         std::copy(v.begin() + i0, v.begin() + i0 + m, slot(rank_, m));
         meet();
         rank_fold(op, n_, m, [&](int k) { return (const double*)slot(k, m); }, v.data() + i0);
         meet();   // everybody has read before the next piece or the next reduction overwrites
      }
      EXA_HC(hipMemcpyAsync(dev, v.data(), sizeof(double) * n, hipMemcpyHostToDevice, s)); EXA_HC(hipStreamSynchronize(s));
   }
};
}  // namespace

// ---- in-process loopback transport (test infrastructure for the multi-rank logic on a one-GPU box) -----------------------------
// Several SystemDrivers, one host thread each, share one device; collectives are host-synchronous exchanges through this group.
// It exercises exactly the code RCCL is used from (partition, pack / unpack-add, weighted dots, reductions); only the RCCL calls
// themselves are replaced.  RCCL cannot be used for this: it refuses two ranks on one device ("Duplicate GPU detected").
struct LoopbackGroup {
   int n; HostBarrier bar;
   std::vector<std::vector<double>> red;                 // per-rank contribution of the current reduction
   std::vector<std::vector<const double*>> sendbuf;      // [rank][neighbour slot] device send buffers of the current halo exchange
   std::vector<std::vector<int>> nbr_rank;               // [rank][slot] neighbour rank
   // stream-asynchronous exchange: "my send buffer is packed" / "I have read my neighbours' send buffers", recorded by every rank
   // on its own stream and waited for by its peers' streams - the host threads only meet to know that the events have been recorded
   std::vector<hipEvent_t> ev_packed, ev_read;
   explicit LoopbackGroup(int n_) : n(n_), bar(n_), red(n_), sendbuf(n_), nbr_rank(n_), ev_packed(n_, nullptr), ev_read(n_, nullptr) {}
   ~LoopbackGroup() { for (hipEvent_t e : ev_packed) if (e) (void)hipEventDestroy(e); for (hipEvent_t e : ev_read) if (e) (void)hipEventDestroy(e); }
};
static const char kLoopMagic[8] = { 'E', 'X', 'A', 'L', 'O', 'O', 'P', '1' };

void Comm::loopback_create(int nranks, void* out128) {
   std::memset(out128, 0, 128);
   std::memcpy(out128, kLoopMagic, 8);
   LoopbackGroup* g = new LoopbackGroup(nranks);
   std::memcpy((char*)out128 + 8, &g, sizeof(g));
}
void Comm::loopback_destroy(const void* id128) {
   if (std::memcmp(id128, kLoopMagic, 8) != 0) return;
   LoopbackGroup* g; std::memcpy(&g, (const char*)id128 + 8, sizeof(g)); delete g;
}

namespace {
struct LoopbackTransport final : HostSyncTransport {
   LoopbackGroup* const g;   // owned by whoever called Comm::loopback_create
   const bool async = std::getenv("EXA_LOOPBACK_SYNC") == nullptr;   // exchanges ordered by events only, no stream is drained
   LoopbackTransport(LoopbackGroup* g_, int rank, int nranks) : HostSyncTransport(rank, nranks, 0), g(g_) {
      if (g->n != nranks) throw std::runtime_error("Comm::init: loopback group size mismatch");
   }
   Comm::Kind kind() const override { return Comm::LOOPBACK; }
   double* slot(int k, int m) override { std::vector<double>& r = g->red[k]; if (k == rank_ && r.size() < (size_t)m) r.resize(m); return r.data(); }
   void meet() override { g->bar.meet(); }
   void exchange(const Halo& h, hipStream_t s) override {
      const size_t nb = h.count(); const int rank = rank_;
      g->sendbuf[rank].resize(nb); g->nbr_rank[rank].resize(nb);
      for (size_t i = 0; i < nb; i++) { g->sendbuf[rank][i] = h.sb(i); g->nbr_rank[rank][i] = h.nbr[i]; }
      auto peer_src = [&](size_t i) {   // my slot i talks to rank r; r's slot that talks to me holds what I receive (same dof order on both sides)
         const int r = h.nbr[i];
         for (size_t k = 0; k < g->nbr_rank[r].size(); k++) if (g->nbr_rank[r][k] == rank) return g->sendbuf[r][k];   // one neighbour entry per pair of ranks
         throw std::runtime_error("loopback halo: asymmetric neighbour lists");
      };
      if (async) {
         // Stream-asynchronous form (default; EXA_LOOPBACK_SYNC=1 keeps the host-synchronous one): NO stream is drained.  Every rank records
         // "packed" on its stream, its peers' streams wait for that event before they copy, every rank records "read" behind its copies and a
         // rank's NEXT pack waits for its neighbours' "read" (the waits at the end of this function, on the stream of this exchange).  The host threads meet twice
         // per exchange only so that an event is recorded before somebody waits for it - the device work of all ranks stays in flight, which is
         // how the overlapped halo (Comm::halo_begin / halo_end: cs_, ev_ready_, ev_done_) runs over RCCL.
         if (!g->ev_packed[rank]) { EXA_HC(hipEventCreateWithFlags(&g->ev_packed[rank], hipEventDisableTiming)); EXA_HC(hipEventCreateWithFlags(&g->ev_read[rank], hipEventDisableTiming)); }
         EXA_HC(hipEventRecord(g->ev_packed[rank], s));
         meet();                                                  // every rank's "packed" is recorded (host side only)
         for (size_t i = 0; i < nb; i++) {
            EXA_HC(hipStreamWaitEvent(s, g->ev_packed[h.nbr[i]], 0));
            EXA_HC(hipMemcpyAsync(h.rb(i), peer_src(i), sizeof(double) * h.cnt(i), hipMemcpyDeviceToDevice, s));
         }
         EXA_HC(hipEventRecord(g->ev_read[rank], s));
         meet();                                                  // every rank's "read" is recorded
         // nobody repacks its send buffer before its readers are done: the stream that packs next is the stream of this exchange or a later one of
         // this rank - ordered behind these waits either way (halo_sum packs on s, halo_begin on cs_, and cs_ waits for ev_ready_ recorded on s)
         for (size_t i = 0; i < nb; i++) EXA_HC(hipStreamWaitEvent(s, g->ev_read[h.nbr[i]], 0));
         return;
      }
      EXA_HC(hipStreamSynchronize(s));
      meet();
      for (size_t i = 0; i < nb; i++) EXA_HC(hipMemcpyAsync(h.rb(i), peer_src(i), sizeof(double) * h.cnt(i), hipMemcpyDeviceToDevice, s));
      EXA_HC(hipStreamSynchronize(s));
      meet();
   }
};
}  // namespace

// ---- inter-process transport for ranks that share ONE device (test / plumbing transport, like the loopback group but across processes) -----
// RCCL refuses two ranks on one device, so `mpirun -np 2 mechanics ...` or `torchrun --nproc-per-node 2 bench.py --gpus 2` could never run
// end to end on a one-GPU box: launcher environment, TCP rendez-vous, local-rank -> device mapping, per-rank files, torch's communicator
// beside this library's.  With EXA_TRANSPORT=ipc (or automatically when there are more ranks than visible devices) rank 0 hands out an id
// of this kind instead of a RCCL id.  Control data lives in a POSIX shared-memory segment named after the id; the halo segments travel
// device-to-device through hipIpcMemHandle mappings of the neighbours' send buffers; reductions go through the segment in rank order.
// Exchanges are host-synchronous (stream sync + barrier), so this is NOT a performance path.
namespace {
constexpr int IPC_MAX_RANKS = 64, IPC_MAX_NBR = 32, IPC_MAX_RED = 32;   // reductions longer than IPC_MAX_RED doubles pass through the slots in pieces
struct IpcShared {
   std::atomic<uint32_t> ready; uint32_t n;
   std::atomic<uint64_t> arrived, generation;
   double red[IPC_MAX_RANKS][IPC_MAX_RED];
   hipIpcMemHandle_t sbuf[IPC_MAX_RANKS]; uint64_t sbuf_len[IPC_MAX_RANKS];
   int32_t nnbr[IPC_MAX_RANKS]; int32_t nbr_rank[IPC_MAX_RANKS][IPC_MAX_NBR]; uint64_t seg_off[IPC_MAX_RANKS][IPC_MAX_NBR + 1];
};
struct IpcGroup {
   IpcShared* sh = nullptr; int n = 0, rank = 0; std::string name;
   std::vector<double*> peer_sbuf;      // neighbours' send buffers mapped into this process (by rank; nullptr: not a neighbour)
   void barrier() {
      const auto t_end = std::chrono::steady_clock::now() + std::chrono::seconds(120);
      const uint64_t g = sh->generation.load(std::memory_order_acquire);
      if (sh->arrived.fetch_add(1, std::memory_order_acq_rel) + 1 == (uint64_t)n) { sh->arrived.store(0, std::memory_order_release); sh->generation.fetch_add(1, std::memory_order_acq_rel); }
      else while (sh->generation.load(std::memory_order_acquire) == g) {
         std::this_thread::yield();
         if (std::chrono::steady_clock::now() > t_end) throw std::runtime_error("ipc transport: a rank did not reach the barrier within 120 s (did a peer fail?)");
      }
   }
   ~IpcGroup() {
      for (double* p : peer_sbuf) if (p) (void)hipIpcCloseMemHandle(p);
      if (sh) ::munmap(sh, sizeof(IpcShared));
   }
};
const char kIpcMagic[8] = { 'E', 'X', 'A', 'I', 'P', 'C', '0', '1' };
std::string ipc_name(const void* uid) {
   static const char* hex = "0123456789abcdef"; std::string s = "/exaipc_";
   for (int i = 8; i < 24; i++) { const unsigned char c = ((const unsigned char*)uid)[i]; s += hex[c >> 4]; s += hex[c & 15]; }
   return s;
}
std::unique_ptr<IpcGroup> ipc_attach(const void* uid, int rank, int nranks) {
   if (nranks > IPC_MAX_RANKS) throw std::runtime_error("ipc transport: too many ranks");
   auto g = std::make_unique<IpcGroup>(); g->n = nranks; g->rank = rank; g->name = ipc_name(uid); g->peer_sbuf.assign((size_t)nranks, nullptr);
   const auto t_end = std::chrono::steady_clock::now() + std::chrono::seconds(60);
   int fd = -1;
   if (rank == 0) {
      ::shm_unlink(g->name.c_str());
      fd = ::shm_open(g->name.c_str(), O_CREAT | O_EXCL | O_RDWR, 0600);
      if (fd < 0 || ::ftruncate(fd, (off_t)sizeof(IpcShared)) != 0) throw std::runtime_error(std::string("ipc transport: shm_open ") + g->name + ": " + std::strerror(errno));
   } else {
      while ((fd = ::shm_open(g->name.c_str(), O_RDWR, 0600)) < 0) {
         if (std::chrono::steady_clock::now() > t_end) throw std::runtime_error("ipc transport: rank 0's segment " + g->name + " did not appear");
         std::this_thread::sleep_for(std::chrono::milliseconds(20));
      }
      struct stat st; while (::fstat(fd, &st) == 0 && (size_t)st.st_size < sizeof(IpcShared)) { if (std::chrono::steady_clock::now() > t_end) throw std::runtime_error("ipc transport: segment not sized"); std::this_thread::sleep_for(std::chrono::milliseconds(5)); }
   }
   void* m = ::mmap(nullptr, sizeof(IpcShared), PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
   ::close(fd);
   if (m == MAP_FAILED) throw std::runtime_error("ipc transport: mmap failed");
   g->sh = (IpcShared*)m;
   if (rank == 0) { g->sh->n = (uint32_t)nranks; g->sh->arrived.store(0); g->sh->generation.store(0); g->sh->ready.store(1, std::memory_order_release); }   // (a fresh segment is zero-filled)
   else while (g->sh->ready.load(std::memory_order_acquire) != 1) { if (std::chrono::steady_clock::now() > t_end) throw std::runtime_error("ipc transport: rank 0 never became ready"); std::this_thread::yield(); }
   if ((int)g->sh->n != nranks) throw std::runtime_error("ipc transport: group size mismatch");
   g->barrier();                                   // everybody is attached: the name can go
   if (rank == 0) ::shm_unlink(g->name.c_str());
   return g;
}

struct IpcTransport final : HostSyncTransport {
   const std::unique_ptr<IpcGroup> g;
   IpcTransport(const void* uid, int rank, int nranks) : HostSyncTransport(rank, nranks, IPC_MAX_RED), g(ipc_attach(uid, rank, nranks)) {}
   Comm::Kind kind() const override { return Comm::IPC; }
   int reported_ranks() const override { return (int)g->sh->n; }
   double* slot(int k, int) override { return g->sh->red[k]; }
   void meet() override { g->barrier(); }
   void halo_plan(const Halo& h) override {   // publish this rank's send buffer and segment table, then map the neighbours' send buffers
      IpcShared* sh = g->sh; const int rank = rank_; const size_t nb = h.count();
      if (nb > (size_t)IPC_MAX_NBR) throw std::runtime_error("ipc transport: too many neighbours");
      for (double*& p : g->peer_sbuf) if (p) { (void)hipIpcCloseMemHandle(p); p = nullptr; }
      sh->nnbr[rank] = (int32_t)nb; sh->sbuf_len[rank] = h.off.back();
      for (size_t i = 0; i < nb; i++) { sh->nbr_rank[rank][i] = h.nbr[i]; sh->seg_off[rank][i] = h.off[i]; }
      sh->seg_off[rank][nb] = h.off.back();
      if (h.off.back() > 0) EXA_HC(hipIpcGetMemHandle(&sh->sbuf[rank], h.sbuf));
      g->barrier();
      for (int r : h.nbr) if (!g->peer_sbuf[r]) {
         void* p = nullptr; EXA_HC(hipIpcOpenMemHandle(&p, sh->sbuf[r], hipIpcMemLazyEnablePeerAccess));
         g->peer_sbuf[r] = (double*)p;
      }
      g->barrier();
   }
   void exchange(const Halo& h, hipStream_t s) override {
      const IpcShared* sh = g->sh; const int rank = rank_;
      EXA_HC(hipStreamSynchronize(s));      // my send buffer is packed
      g->barrier();                         // ... and so is everybody else's
      for (size_t i = 0; i < h.count(); i++) {     // my slot i talks to rank r; r's slot that talks to me holds what I receive (same dof order on both sides)
         const int r = h.nbr[i]; int k = -1;
         for (int j = 0; j < sh->nnbr[r]; j++) if (sh->nbr_rank[r][j] == rank) { k = j; break; }
         if (k < 0 || sh->seg_off[r][k + 1] - sh->seg_off[r][k] != h.cnt(i)) throw std::runtime_error("ipc halo: asymmetric neighbour lists");
         EXA_HC(hipMemcpyAsync(h.rb(i), g->peer_sbuf[r] + sh->seg_off[r][k], sizeof(double) * h.cnt(i), hipMemcpyDeviceToDevice, s));
      }
      EXA_HC(hipStreamSynchronize(s));
      g->barrier();                         // nobody repacks its send buffer before everybody has read it
   }
};
}  // namespace

void Comm::ipc_unique_id(void* out128) {
   std::memset(out128, 0, 128); std::memcpy(out128, kIpcMagic, 8);
   FILE* f = std::fopen("/dev/urandom", "rb");
   if (!f || std::fread((char*)out128 + 8, 1, 16, f) != 16) { const uint64_t t = (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count() ^ ((uint64_t)::getpid() << 32); std::memcpy((char*)out128 + 8, &t, 8); }
   if (f) std::fclose(f);
}
bool Comm::want_ipc_transport(int nranks) {
   if (const char* e = std::getenv("EXA_TRANSPORT")) { if (std::string(e) == "ipc") return true; if (std::string(e) == "rccl") return false; }
   // Without identities (exa_comm_unique_id called by a launcher that did not compare them): ranks of THIS NODE against its visible devices.
   // The node-local count comes from the launcher when it says so; the global count only stands in for it on a one-node launch.
   int local = nranks;
   for (const char* k : { "EXA_LOCAL_NRANKS", "LOCAL_WORLD_SIZE", "OMPI_COMM_WORLD_LOCAL_SIZE", "MPI_LOCALNRANKS", "SLURM_NTASKS_PER_NODE" })
      if (const char* v = std::getenv(k)) { const int n = std::atoi(v); if (n > 0) { local = n; break; } }
   int nd = 0; return nranks > 1 && hipGetDeviceCount(&nd) == hipSuccess && nd > 0 && local > nd;      // more ranks than devices on the node: RCCL cannot serve them
}
void Comm::get_unique_id(void* out128) { ncclUniqueId id; nccl_check(rccl().GetUniqueId(&id), "ncclGetUniqueId"); std::memcpy(out128, &id, sizeof(id)); }

// =====================================================================================================================
// Comm
// =====================================================================================================================
Comm::Comm() = default;
Comm::~Comm() {
   tr_.reset();   // (the shared-device transport unmaps its neighbours' send buffers before the own one is freed)
   if (cs_) { (void)hipStreamDestroy(cs_); (void)hipEventDestroy(ev_ready_); (void)hipEventDestroy(ev_done_); }
}

void Comm::init(int rank_, int nranks_, const void* uid, bool force_rccl) {
   rank = rank_; nranks = nranks_;
   // EXA_FORCE_RCCL=1 routes the one-rank case through RCCL too (plumbing check on a single-GPU box)
   force_ = (nranks == 1 && (force_rccl || std::getenv("EXA_FORCE_RCCL") != nullptr));
   // EXA_HALO_SELFTEST=1 (with the forced one-rank communicator): the rank is its own neighbour across its x-max face (SystemDriver adds the entry) and sends
   // ZEROS of the real halo size to itself - the grouped ncclSend / ncclRecv of an exchange, on the communication stream beside the interior blocks when the
   // overlapped form is on, between the all-reduces of the PCG on the main stream: the two-stream use of one communicator on the hardware there is
   selftest_zero_ = force_ && std::getenv("EXA_HALO_SELFTEST") != nullptr;
   if (uid && std::memcmp(uid, kLoopMagic, 8) == 0) {
      LoopbackGroup* g; std::memcpy(&g, (const char*)uid + 8, sizeof(g));
      tr_ = std::make_unique<LoopbackTransport>(g, rank, nranks);
   } else if (uid && std::memcmp(uid, kIpcMagic, 8) == 0 && nranks > 1) tr_ = std::make_unique<IpcTransport>(uid, rank, nranks);
   else if (active()) tr_ = std::make_unique<RcclTransport>(uid, rank, nranks, force_);
   tmp_.alloc(64);
}

Comm::Kind Comm::kind() const { return tr_ ? tr_->kind() : NONE; }
int Comm::reported_ranks() const { return tr_ ? tr_->reported_ranks() : 1; }

void Comm::allreduce(double* dev, int n, RankOp op, hipStream_t s) { if (tr_) tr_->allreduce(dev, n, op, s); }
void Comm::allreduce_sum(double* dev, int n, hipStream_t s) { allreduce(dev, n, RankOp::SUM, s); }
void Comm::allreduce_min(double* dev, int n, hipStream_t s) { allreduce(dev, n, RankOp::MIN, s); }
void Comm::allreduce_max(double* dev, int n, hipStream_t s) { allreduce(dev, n, RankOp::MAX, s); }

double Comm::max_over_ranks(double v) {
   if (nranks == 1) return v;   // (also on the forced one-rank communicator: there is nobody to agree with)
   EXA_HC(hipMemcpy(tmp_.p, &v, sizeof(double), hipMemcpyHostToDevice));
   allreduce(tmp_.p, 1, RankOp::MAX, nullptr);
   EXA_HC(hipMemcpy(&v, tmp_.p, sizeof(double), hipMemcpyDeviceToHost));
   return v;
}

void Comm::microbench(int iters, int n, double* us_allreduce, double* us_sendrecv) {
   if (kind() != RCCL) throw std::runtime_error("Comm::microbench needs a RCCL communicator (EXA_FORCE_RCCL=1 on one rank)");
   const ncclComm_t comm = static_cast<RcclTransport*>(tr_.get())->comm;
   DevBuf<double> a(2), sb((size_t)n), rb((size_t)n); a.zero(); sb.zero(); rb.zero();
   hipStream_t s; EXA_HC(hipStreamCreate(&s));
   hipEvent_t e0, e1; EXA_HC(hipEventCreate(&e0)); EXA_HC(hipEventCreate(&e1));
   auto timed = [&](auto&& body) {
      for (int i = 0; i < 10; i++) body();
      EXA_HC(hipEventRecord(e0, s));
      for (int i = 0; i < iters; i++) body();
      EXA_HC(hipEventRecord(e1, s)); EXA_HC(hipEventSynchronize(e1));
      float ms = 0; EXA_HC(hipEventElapsedTime(&ms, e0, e1)); return 1e3 * ms / iters;
   };
   *us_allreduce = timed([&] { nccl_check(rccl().AllReduce(a.p, a.p, 2, ncclDouble, ncclSum, comm, s), "ncclAllReduce"); });
   *us_sendrecv = timed([&] {
      nccl_check(rccl().GroupStart(), "ncclGroupStart");
      nccl_check(rccl().Send(sb.p, (size_t)n, ncclDouble, rank, comm, s), "ncclSend");
      nccl_check(rccl().Recv(rb.p, (size_t)n, ncclDouble, rank, comm, s), "ncclRecv");
      nccl_check(rccl().GroupEnd(), "ncclGroupEnd"); });
   (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipStreamDestroy(s);
}

// One pack and one unpack launch per exchange: the neighbours' dof lists are concatenated (segment i = neighbour i), the send /
// receive buffers are one allocation each.  (A launch per neighbour is 14 tiny kernels per operator action on a 2 x 2 x 2 grid -
// more than the exchange itself.)  A dof shared with several neighbours appears in several segments: the unpack adds atomically.
void Comm::setup_halo(const Partition& part) {
   nbr_rank_.clear(); seg_off_.assign(1, 0);
   std::vector<int32_t> all;
   for (const Neighbor& nb : part.nbrs) { nbr_rank_.push_back(nb.rank); all.insert(all.end(), nb.dofs.begin(), nb.dofs.end()); seg_off_.push_back(all.size()); }
   idx_all_.release(); sbuf_all_.release(); rbuf_all_.release();
   if (!all.empty()) { idx_all_.alloc(all.size()); idx_all_.upload(all); sbuf_all_.alloc(all.size()); rbuf_all_.alloc(all.size()); }
   if (tr_) tr_->halo_plan(Halo{ nbr_rank_, seg_off_, sbuf_all_.p, rbuf_all_.p });
}

void Comm::pack_exchange(double* y, hipStream_t s) {
   vk_pack((int64_t)seg_off_.back(), idx_all_.p, y, sbuf_all_.p, s);
   if (selftest_zero_) EXA_HC(hipMemsetAsync(sbuf_all_.p, 0, sizeof(double) * seg_off_.back(), s));
   tr_->exchange(Halo{ nbr_rank_, seg_off_, sbuf_all_.p, rbuf_all_.p }, s);
}

void Comm::halo_sum(double* y, hipStream_t s) {
   if (!active()) return;
   pack_exchange(y, s);
   unpack(y, s);
}

// Overlapped form: everything enqueued on s before halo_begin (the element blocks that touch shared dofs) is waited for by the
// communication stream, which packs and exchanges while s goes on with the interior blocks; halo_end makes s wait for the exchange and
// adds the received segments.  Same arithmetic as halo_sum: only the stream the pack / exchange run on differs.
void Comm::halo_begin(double* y, hipStream_t s) {
   if (!active()) return;
   if (!cs_) { EXA_HC(hipStreamCreateWithFlags(&cs_, hipStreamNonBlocking)); EXA_HC(hipEventCreateWithFlags(&ev_ready_, hipEventDisableTiming)); EXA_HC(hipEventCreateWithFlags(&ev_done_, hipEventDisableTiming)); }
   EXA_HC(hipEventRecord(ev_ready_, s));
   EXA_HC(hipStreamWaitEvent(cs_, ev_ready_, 0));
   pack_exchange(y, cs_);
   EXA_HC(hipEventRecord(ev_done_, cs_));
}
void Comm::halo_end(double* y, hipStream_t s) {
   if (!active()) return;
   EXA_HC(hipStreamWaitEvent(s, ev_done_, 0));
   unpack(y, s);
}

// adds the received segments to y.  A dof on an edge or corner of the block occurs in several segments: one launch over all of them adds
// with atomics in arbitrary order; in deterministic mode the segments are added one after the other (no dof twice within a segment)
void Comm::unpack(double* y, hipStream_t s) {
   if (!deterministic) { vk_unpack_add((int64_t)seg_off_.back(), idx_all_.p, rbuf_all_.p, y, s); return; }
   for (size_t i = 0; i + 1 < seg_off_.size(); i++)
      vk_unpack_add((int64_t)(seg_off_[i + 1] - seg_off_[i]), idx_all_.p + seg_off_[i], rbuf_all_.p + seg_off_[i], y, s);
}

}  // namespace exa_host
