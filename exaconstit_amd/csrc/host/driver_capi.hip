// C entry points of the stand-alone driver (used by the `mechanics` executable, the tests and bench.py through ctypes).
// They expose the reference's run-time surface: `mechanics -opt options.toml` (reference src/mechanics_driver.cpp:139-144),
// the per-step loop, the avg_* outputs (reference src/system_driver.cpp:444-553) and the timing regions the reference marks
// with Caliper (ecmech_kernel, krylov_solver: src/mechanics_ecmech.cpp:237-257, src/mechanics_solver.cpp:99-103).
#include "../gmres_slots.hpp"
#include "../gmres_small.hpp"
#include "driver.hpp"
#include "multigrid.hpp"
#include "rank_sync.hpp"
#include "roctx.hpp"
#include "vtu.hpp"
#include "checkpoint.hpp"
#include "../../../include/exaconstit_driver.h"
#include <unistd.h>
#include <cmath>
#include <cstring>
#include <string>

using namespace exa_host;

struct exa_driver {
   std::unique_ptr<SystemDriver> sd;
   std::vector<double> v_kin;   // kinematic velocity field of the bench (host copy)
};

namespace {
void set_err(char* err, int n, const std::string& m) { if (err && n > 0) { std::strncpy(err, m.c_str(), n - 1); err[n - 1] = 0; } }
}

extern "C" {

// Transport from the identity of the ranks' devices (96-byte records: host name[64], PCI bus id[32]).  RCCL needs one device per rank; the
// shared-device transport (POSIX shm + hipIpc, host/comm.hip) needs every rank on ONE host.  Counting ranks against visible devices cannot
// tell the two apart (16 ranks on 2 x 8 GPUs, or one visible device per rank under srun --gpus-per-task=1), identities can.
int exa_transport_from_identities(const void* ids, int nranks, char* err, int errlen) {
   const char* t = (const char*)ids;
   bool one_host = true, shared = false;
   for (int i = 0; i < nranks; i++) {
      if (std::strncmp(t, t + 96 * (size_t)i, 64) != 0) one_host = false;
      for (int j = 0; j < i; j++) if (std::memcmp(t + 96 * (size_t)i, t + 96 * (size_t)j, 96) == 0) shared = true;
   }
   const char* e = std::getenv("EXA_TRANSPORT");
   const std::string force = e ? e : "";
   if (force == "ipc" || (force != "rccl" && shared)) {
      if (!one_host) { set_err(err, errlen, "exa_bootstrap: the shared-device transport serves ranks of one host only; this group spans hosts (one GPU per rank and RCCL is the multi-node configuration)"); return -1; }
      return 2;
   }
   if (shared) { set_err(err, errlen, "exa_bootstrap: EXA_TRANSPORT=rccl, but two ranks sit on the same device (RCCL refuses that)"); return -1; }
   return 1;
}

namespace {
int bootstrap_reply(const void* all, int nranks, int nbytes, void* reply, int reply_bytes, void* user) {
   if (nbytes != 96 || reply_bytes != 132) return -1;
   char* err = (char*)user;
   const int kind = exa_transport_from_identities(all, nranks, err, 256);
   if (kind < 0) { std::memset(reply, 0, 132); int32_t k = -1; std::memcpy((char*)reply + 128, &k, 4); std::snprintf((char*)reply, 128, "%s", err); return 0; }   // every rank learns why
   try { if (kind == 2) Comm::ipc_unique_id(reply); else Comm::get_unique_id(reply); }
   catch (const std::exception& e) { std::snprintf(err, 256, "exa_bootstrap: %s", e.what()); return -1; }
   const int32_t k = kind; std::memcpy((char*)reply + 128, &k, 4);
   return 0;
}
}

// rank / size from the launcher's environment, device = local rank mod visible devices, then ONE TCP rendez-vous (host/bootstrap.cpp): every
// rank sends the identity of its device, rank 0 decides the transport from them and answers with the unique id of that transport - a RCCL
// id, or the shared-device transport's when ranks of one host share a GPU.  Everything `mechanics` needs before exa_driver_create (reference:
// MPI_Init + MPI_Comm_rank/size, src/mechanics_driver.cpp:119-150)
int exa_bootstrap(int* rank, int* nranks, void* uid128, char* err, int errlen) {
   int lr = 0;
   if (exa_bootstrap_env(rank, nranks, &lr) != 0) { set_err(err, errlen, "exa_bootstrap: inconsistent rank / size in the environment"); return -1; }
   int nd = 0;
   if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) { set_err(err, errlen, "exa_bootstrap: no HIP device"); return -1; }
   if (hipSetDevice(lr % nd) != hipSuccess) { set_err(err, errlen, "exa_bootstrap: hipSetDevice failed"); return -1; }
   std::memset(uid128, 0, 128);
   if (*nranks > 1) {
      char mine[96]; std::memset(mine, 0, sizeof(mine));
      if (::gethostname(mine, 63) != 0) std::snprintf(mine, 64, "unknown-host");
      if (exa_device_identity(mine + 64, 32) != 0) std::snprintf(mine + 64, 32, "device-index-%d-of-%d", lr % nd, nd);
      char reply[132]; char cb_err[256] = "";
      double tmo = 60.0; if (const char* t = std::getenv("EXA_RENDEZVOUS_TIMEOUT")) { const double v = std::atof(t); if (v > 0) tmo = v; }
      if (exa_bootstrap_gather_reply(*rank, *nranks, mine, 96, reply, 132, bootstrap_reply, cb_err, tmo, err, errlen) != 0) {
         if (cb_err[0]) set_err(err, errlen, cb_err);
         return -1;
      }
      int32_t kind = 0; std::memcpy(&kind, reply + 128, 4);
      if (kind < 0) { reply[127] = 0; set_err(err, errlen, reply); return -1; }
      std::memcpy(uid128, reply, 128);
      if (*rank == 0) std::fprintf(stderr, "exa_bootstrap: %d ranks, transport %s (decided from host names and PCI bus ids)\n", *nranks, kind == 2 ? "ipc (ranks share a device)" : "rccl");
   }
   return 0;
}

// latency floor of the two RCCL calls of a PCG iteration on this device (one-rank communicator): out2 = { us per 16-byte all-reduce,
// us per grouped send/recv of n doubles to the own rank }; input of the scaling prediction in DESIGN.md section 7
int exa_rccl_microbench(int iters, int n, double* out2, char* err, int errlen) {
   try {
      Comm c; c.init(0, 1, nullptr, /*force_rccl=*/true);   // (no environment change: later drivers of the process keep their own setting)
      c.microbench(iters, n, out2, out2 + 1);
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

int exa_rccl_unique_id(void* out128) {
   try { Comm::get_unique_id(out128); return 0; } catch (const std::exception& e) { std::fprintf(stderr, "exa_rccl_unique_id: %s\n", e.what()); return -1; }
}

// PCI bus id ("0000:c1:00.0") of the calling thread's current device: what the launchers compare to tell one rank per physical GPU from several
// ranks on one GPU, whatever device numbering each rank sees
int exa_device_identity(char* out, int len) {
   int dev = 0;
   if (!out || len < 16 || hipGetDevice(&dev) != hipSuccess) return -1;
   return hipDeviceGetPCIBusId(out, len, dev) == hipSuccess ? 0 : -1;
}
// the id rank 0 hands out for a group of `nranks` when the caller has NOT compared device identities itself: a RCCL unique id, or - with
// EXA_TRANSPORT=ipc, or when the ranks of this node outnumber its visible devices - the id of the inter-process transport of host/comm.hip
// (class Comm).  bench.py compares identities and sets EXA_TRANSPORT; exa_bootstrap decides from identities (exa_transport_from_identities).
int exa_comm_unique_id(void* out128, int nranks) {
   try { if (Comm::want_ipc_transport(nranks)) Comm::ipc_unique_id(out128); else Comm::get_unique_id(out128); return 0; }
   catch (const std::exception& e) { std::fprintf(stderr, "exa_comm_unique_id: %s\n", e.what()); return -1; }
}
// out2 = { ranks the transport itself reports (ncclCommCount for RCCL), kind: 0 none (one rank), 1 rccl, 2 ipc (shared device), 3 in-process loopback }
int exa_driver_comm_info(exa_driver* d, int* out2) {
   try {
      const Comm& c = d->sd->comm;
      out2[0] = c.reported_ranks(); out2[1] = (int)c.kind();
      return 0;
   } catch (const std::exception& e) { std::fprintf(stderr, "exa_driver_comm_info: %s\n", e.what()); return -1; }
}

// out8 = { local elements, elements in blocks that touch shared nodes, neighbours, doubles sent (= received) per halo exchange, halo exchange
//          overlapped with the interior blocks (0 / 1), transport kind (exa_driver_comm_info), ranks the transport reports, 0 }
int exa_driver_comm_details(exa_driver* d, int64_t* out8) {
   try {
      const SystemDriver& sd = *d->sd; int info[2] = { 1, 0 };
      (void)exa_driver_comm_info(d, info);
      out8[0] = sd.part.E; out8[1] = sd.part.E_bdr; out8[2] = (int64_t)sd.part.nbrs.size(); out8[3] = (int64_t)sd.comm.halo_dofs();
      out8[4] = d->sd->oper().halo_overlap() ? 1 : 0; out8[5] = info[1]; out8[6] = info[0]; out8[7] = 0;
      return 0;
   } catch (const std::exception& e) { std::fprintf(stderr, "exa_driver_comm_details: %s\n", e.what()); return -1; }
}

// The transport on its own (tests): what 0 / 1 / 2 = Comm::allreduce_sum / _min / _max of n host doubles on the operator's stream; 3 = Comm::halo_sum of a
// host L-vector of the local dofs (n = exa_driver_local_dofs, dof = node + local nodes * component).  In place; every rank of the group calls it.
int exa_driver_comm_probe(exa_driver* d, int what, double* host_vec, int n) {
   try {
      SystemDriver& sd = *d->sd; hipStream_t s = sd.oper().stream();
      if (what < 0 || what > 3 || n < 1 || (what == 3 && n != 3 * sd.part.NN)) throw std::runtime_error("what must be 0 .. 3 and n >= 1 (halo sum: the local dofs)");
      DevBuf<double> v((size_t)n); v.upload(host_vec, (size_t)n, s);
      if (what == 0) sd.comm.allreduce_sum(v.p, n, s);
      else if (what == 1) sd.comm.allreduce_min(v.p, n, s);
      else if (what == 2) sd.comm.allreduce_max(v.p, n, s);
      else sd.comm.halo_sum(v.p, s);
      v.download(host_vec, (size_t)n, s);
      return 0;
   } catch (const std::exception& e) { std::fprintf(stderr, "exa_driver_comm_probe: %s\n", e.what()); return -1; }
}

// host only: the fold of the host-synchronous reductions (rank_sync.hpp) over contributions[nranks][n]; op 0 sum, 1 min, 2 max
int exa_comm_rank_fold(int op, int nranks, int n, const double* contributions, double* out) {
   if (op < 0 || op > 2 || nranks < 1) return -1;
   rank_fold((RankOp)op, nranks, n, [&](int k) { return contributions + (size_t)k * n; }, out);
   return 0;
}

// host only: the operator's route decision for the facts under the switches of the environment as it is now (order of facts and out: exaconstit_driver.h)
int exa_operator_routes_query(const int* facts, int nfacts, int* out, int nout) {
   if (!facts || !out || nfacts != RouteFacts::COUNT || nout < OperatorRoutes::QUERY_FIELDS) return -1;
   RouteFacts f;
   f.geom = facts[0]; f.order = facts[1]; f.bbar = facts[2] != 0; f.ea = facts[3] != 0; f.slip = facts[4]; f.several_ranks = facts[5] != 0;
   f.rccl = facts[6] != 0; f.has_bdr_blocks = facts[7] != 0; f.has_nbrs = facts[8] != 0; f.periodic = facts[9] != 0;
   if (f.geom < 0 || f.geom > 1 || f.order < 1 || f.slip < 0 || f.slip > 2 || (f.geom == 1 && f.bbar)) return -1;
   decide_routes(f, RouteSwitches::from_env()).to_ints(out);
   return OperatorRoutes::QUERY_FIELDS;
}

int exa_loopback_group_create(int nranks, void* out128) { try { Comm::loopback_create(nranks, out128); return 0; } catch (...) { return -1; } }
void exa_loopback_group_destroy(const void* id128) { Comm::loopback_destroy(id128); }

exa_driver* exa_driver_create(const char* toml_path, const char* out_dir, int rank, int nranks, const void* uid, int jacobi, int write_files, char* err, int errlen) {
   return exa_driver_create_restart(toml_path, out_dir, rank, nranks, uid, jacobi, write_files, nullptr, err, errlen);
}

// restart_path: NULL = what Checkpoint.restart_from of the options file says (usually nothing), "" = no restart, otherwise the checkpoint to resume from
exa_driver* exa_driver_create_restart(const char* toml_path, const char* out_dir, int rank, int nranks, const void* uid, int jacobi, int write_files,
                                      const char* restart_path, char* err, int errlen) {
   try {
      ExaOptions opt; opt.parse_options(toml_path);
      std::unique_ptr<exa_driver> d(new exa_driver());
      d->sd.reset(new SystemDriver(opt, rank, nranks, uid));
      d->sd->out_dir = out_dir ? out_dir : "."; d->sd->write_files = write_files != 0;
      d->sd->SetPreconditioner(jacobi ? 1 : 0, 0, 0);
      if (opt.precond != 0) d->sd->SetPreconditioner(opt.precond, opt.mg_levels, opt.mg_degree);   // Solvers.Krylov.preconditioner decides when it is present
      const std::string from = restart_path ? std::string(restart_path) : opt.resolve(opt.ckpt_restart_from);
      if (!from.empty()) d->sd->LoadCheckpoint(from);
      return d.release();
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return nullptr; }
}

int exa_driver_save_checkpoint(exa_driver* d, const char* path, char* err, int errlen) {
   try { d->sd->SaveCheckpoint(path); return 0; } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}
int exa_driver_load_checkpoint(exa_driver* d, const char* path, char* err, int errlen) {
   try { d->sd->LoadCheckpoint(path); return 0; } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

// header of a checkpoint file (no GPU needed): out[0..19] = version, E_global, NN_global, Q, geometry, order, model, nprops, nstatev, steps_done, bc_index,
// nranks, flags, nsections, model_calls, newton_cap, newton_cap2, writer, 0, 0; outd[0..2] = time, dt_class, last_dt; hashes[0..2] = property, grain-map,
// connectivity hash.  sec_names (nsections x 24 bytes) and sec_info (nsections x { offset, nbytes, checksum }) may be NULL; at most max_sections are copied.
int exa_checkpoint_info(const char* path, int64_t* out, double* outd, uint64_t* hashes, char* sec_names, uint64_t* sec_info, int max_sections, char* err, int errlen) {
   try {
      exa_ckpt::Header h; std::vector<exa_ckpt::Section> sec;
      exa_ckpt::read_info(path, h, sec);
      const int64_t v[20] = { h.version, h.E_global, h.NN_global, h.Q, h.geom, h.order, h.model, h.nprops, h.nstatev, h.steps_done, h.bc_index, h.nranks, h.flags,
                              h.nsections, h.model_calls, h.newton_cap, h.newton_cap2, h.writer, 0, 0 };
      if (out) std::memcpy(out, v, sizeof(v));
      if (outd) { outd[0] = h.time; outd[1] = h.dt_class; outd[2] = h.last_dt; }
      if (hashes) { hashes[0] = h.props_hash; hashes[1] = h.grain_hash; hashes[2] = h.conn_hash; }
      for (int i = 0; i < (int)sec.size() && i < max_sections; i++) {
         if (sec_names) { std::memset(sec_names + 24 * (size_t)i, 0, 24); std::memcpy(sec_names + 24 * (size_t)i, sec[i].name.c_str(), std::min<size_t>(sec[i].name.size(), 23)); }
         if (sec_info) { sec_info[3 * i] = sec[i].offset; sec_info[3 * i + 1] = sec[i].nbytes; sec_info[3 * i + 2] = sec[i].checksum; }
      }
      return (int)sec.size();
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

// [Checkpoint] table of an options file: out3 = { write, steps, keep }
int exa_options_query_checkpoint(const char* toml_path, int* out3, char* floc, int floclen, char* restart_from, int restartlen, char* err, int errlen) {
   try {
      ExaOptions o; o.parse_options(toml_path);
      if (out3) { out3[0] = o.ckpt_write ? 1 : 0; out3[1] = o.ckpt_steps; out3[2] = o.ckpt_keep; }
      if (floc && floclen > 0) { if ((int)o.ckpt_floc.size() >= floclen) throw std::runtime_error("Checkpoint.floc longer than the buffer"); std::strcpy(floc, o.ckpt_floc.c_str()); }
      if (restart_from && restartlen > 0) { if ((int)o.ckpt_restart_from.size() >= restartlen) throw std::runtime_error("Checkpoint.restart_from longer than the buffer"); std::strcpy(restart_from, o.ckpt_restart_from.c_str()); }
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

// local -> global node map of a rank's partition (Partition::node_gid): info2 = { local nodes, global nodes }; node_gid may be NULL
int exa_partition_query_nodes(const int* N, int rank, int nranks, int order, int64_t* info2, int64_t* node_gid) {
   Partition p; const double L[3] = { 1.0, 1.0, 1.0 };
   p.build(N, L, rank, nranks, (order >= 1 && order <= 6) ? order : 1);
   info2[0] = p.NN; info2[1] = p.NN_glob;
   if (node_gid) std::memcpy(node_gid, p.node_gid.data(), sizeof(int64_t) * p.node_gid.size());
   return 0;
}
int exa_mesh_partition_query_nodes(const char* mesh_path, int rank, int nranks, int order, int64_t* info2, int64_t* node_gid, char* err, int errlen) {
   try {
      Partition p; p.build_from_mfem_mesh(mesh_path, rank, nranks, order);
      info2[0] = p.NN; info2[1] = p.NN_glob;
      if (node_gid) std::memcpy(node_gid, p.node_gid.data(), sizeof(int64_t) * p.node_gid.size());
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

exa_driver* exa_driver_create_synthetic(const exa_synth_config* c, int rank, int nranks, const void* uid, char* err, int errlen) {
   try {
      ExaOptions opt;
      opt.temp_k = c->temp_k;
      opt.xtal = c->bcc ? XtalType::BCC : XtalType::FCC;
      opt.slip = c->slip == 0 ? SlipType::POWERVOCE : (c->slip == 1 ? SlipType::POWERVOCENL : SlipType::MTSDD);
      for (int i = 0; i < 3; i++) { opt.ncuts[i] = c->N; opt.length[i] = 1.0; }
      opt.assembly = c->assembly == 0 ? Assembly::PA : Assembly::EA;
      opt.order = c->order > 0 ? c->order : 1; opt.integ_model = c->bbar ? "BBAR" : "FULL";
      opt.nl_solver = c->nrls ? NLSolver::NRLS : NLSolver::NR;
      opt.newton_iter = c->newton_iter; opt.newton_rel = c->newton_rel; opt.newton_abs = c->newton_abs;
      opt.krylov_iter = c->krylov_iter; opt.krylov_rel = c->krylov_rel; opt.krylov_abs = c->krylov_abs;
      opt.dt_cust = true; opt.nsteps = c->nsteps; opt.cust_dt.assign(c->dts, c->dts + c->nsteps);
      // uniaxial z-tension with three symmetry planes (reference test/data/voce_pa.toml [BCs])
      BCEntry bc; bc.step = 1; bc.ids = { 1, 2, 3, 4 }; bc.comps = { 3, 1, 2, 3 }; bc.vals = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, c->vz };
      opt.bcs.push_back(bc);
      double vz = c->vz;
      for (int i = 0; i < c->nrev; i++) {   // cyclic loading (reference test/data/voce_full_cyclic.toml: changing_ess_bcs with update_steps)
         vz = -vz;
         BCEntry rb = bc; rb.step = c->rev_steps[i]; rb.vals.back() = vz;
         opt.bcs.push_back(rb);
      }
      std::vector<double> props(c->props, c->props + c->nprops);
      const size_t Eg = (size_t)c->N * c->N * c->N;
      std::vector<double> quats(c->quats, c->quats + 4 * Eg);
      auto d = new exa_driver();
      d->sd.reset(new SystemDriver(opt, props, quats, rank, nranks, uid));
      d->sd->write_files = false;
      d->sd->SetPreconditioner(c->jacobi ? 1 : 0, 0, 0);
      return d;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return nullptr; }
}

void exa_driver_destroy(exa_driver* d) { delete d; }

int exa_driver_set_periodic(exa_driver* d, const double* vel_grad9, char* err, int errlen) {
   try { d->sd->SetPeriodic(vel_grad9); return 0; } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

// mixed loading: free9[3 i + d] != 0 makes entry (i, d) of the velocity gradient an unknown with zero mean traction; NULL or all zero = exa_driver_set_periodic
int exa_driver_set_periodic_mixed(exa_driver* d, const double* vel_grad9, const int* free9, char* err, int errlen) {
   try {
      uint8_t f[9]; free_mask_bits(free9, f);
      d->sd->SetPeriodic(vel_grad9, f); return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}
// free9: the mask; vel_grad9: H A^-1 realised by the last solved step (zeros before it); period9: A of the start of that step, column d = a_d, row by
// row; resultants9: F_id of the last converged residual, row by row.  Returns 1 when mixed loading is on (0: all outputs zero), -1 on error.
int exa_driver_macro_info(exa_driver* d, int* free9, double* vel_grad9, double* period9, double* resultants9) {
   try {
      const SystemDriver& sd = *d->sd; const MixedLoading& m = sd.mixed_loading();
      for (int k = 0; k < 9; k++) { free9[k] = 0; vel_grad9[k] = period9[k] = resultants9[k] = 0.0; }
      if (!m.on) return 0;
      for (int k = 0; k < 9; k++) { free9[k] = m.free[k]; period9[k] = m.A[k]; resultants9[k] = m.F[k]; }
      if (m.solved) for (int k = 0; k < 9; k++) vel_grad9[k] = sd.vgrad_in_force()[k];
      return 1;
   } catch (const std::exception& e) { std::fprintf(stderr, "exa_driver_macro_info: %s\n", e.what()); return -1; }
}

// Homogenised tangent of the last solved step of a periodic cell.  rel_tol / max_iter <= 0: the Krylov options; batched: -1 automatic
// route, 0 column by column, 1 the batched multi-column route.  dsig81[9 (3 k + l) + (3 m + n)] = d sigma_bar_kl / d L_bar_mn; out2 = { V, dt };
// info (9 x 6, may be NULL): per column { iterations, solver flag, the solver's own reduction, |b|, |b - K_uu w| recomputed, max |w| / max |a| };
// route2 (may be NULL) = { batched (0 / 1), columns per pass }.  Every rank calls it.  Returns 0 or -1 (err).
int exa_driver_macro_tangent(exa_driver* d, double rel_tol, int max_iter, int batched, double* dsig81, double* out2, double* info, int* route2, char* err, int errlen) {
   try {
      MacroTangentResult r;
      d->sd->MacroTangent(rel_tol, max_iter, batched, r);
      for (int k = 0; k < 81; k++) dsig81[k] = r.T[k] / r.V;
      out2[0] = r.V; out2[1] = r.dt;
      if (info) for (int m = 0; m < 9; m++) {
         info[6 * m] = r.iters[m]; info[6 * m + 1] = r.flag[m]; info[6 * m + 2] = r.reduction[m]; info[6 * m + 3] = r.b_norm[m]; info[6 * m + 4] = r.res_norm[m]; info[6 * m + 5] = r.w_over_a[m];
      }
      if (route2) { route2[0] = r.batched; route2[1] = r.nch; }
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

// Probe of the operator behind the tangent, in the spirit of exa_driver_mg_apply: y_m = K x_m for ncols <= 16 host columns of local dofs (byNODES: dof =
// node + local nodes * component, column m at m * local dofs).  flags bit 0: assembled and masked (the operator K_uu of the tangent's solves) instead of
// the raw element action; bit 1: batched (exa_grad_apply_lvec_cols) instead of one by one.  gated (may be NULL): columns with a non-zero entry are left
// out and keep the y passed in.  nch: columns per pass of the batched route for this and later calls (0: leave as is).  Needs a solved step.
int exa_driver_grad_apply_columns(exa_driver* d, int ncols, const double* x, double* y, int flags, const int* gated, int nch, char* err, int errlen) {
   try {
      if (nch < 0 || nch > 3) throw std::runtime_error("grad_apply_columns: 1, 2 or 3 columns per pass");
      if (nch > 0) d->sd->tangent_nch = nch;
      d->sd->GradApplyColumns(ncols, x, y, (flags & 1) != 0, (flags & 2) != 0, gated);
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

// Probe of the linear solver, next to the one of its operator: K_uu x_m = b_m from x = 0 for nrhs <= 16 host columns of local dofs (byNODES, column m at
// m * local dofs), K_uu the assembled and masked operator of exa_driver_grad_apply_columns (flags bit 0), in a PCG solver of the probe's own: the run's
// settings with rel_tol, abs_tol, max_iter, check_every (0: the run's) and graph (-1: replay as the run decides, 0: never, 1: at any size).  mode 0:
// the single-system solve for each column in turn, into one fixed device buffer by one solver object; mode 1: all columns in lockstep (the columns per
// pass of exa_driver_set_tangent_route).  Per column: x, iterations, flag (1 converged, 2 max_iter, -1 breakdown), the solver's own reduction
// sqrt((r, z) / (r0, z0)), iterations that saw (Ad, d) < 0, scalars2[2 m] = (r0, z0) and scalars2[2 m + 1] = the last (r, z).  Needs a solved step;
// every rank calls it.  The run's solver, captured chunk, diagnostics and totals are not touched.  Returns 0 or -1 (err).
int exa_driver_pcg_solve(exa_driver* d, int nrhs, const double* b, double rel_tol, double abs_tol, int max_iter, int check_every, int graph, int mode, double* x, int* iters,
                         int* flags, double* reduction, int* indefinite, double* scalars2, char* err, int errlen) {
   try {
      d->sd->PcgSolveProbe(nrhs, b, rel_tol, abs_tol, max_iter, check_every, graph, mode, x, iters, flags, reduction, indefinite, scalars2);
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

// The run's linear solver: solver "pcg" or "gmres" (any case), kdim the Krylov dimension of GMRES (1 ... 100; ignored for PCG).  Legal before the
// first step and between steps; tolerances and cap stay, the run's diagnostics and totals go on counting.  Every rank calls it.
int exa_driver_set_krylov(exa_driver* d, const char* solver, int kdim, char* err, int errlen) {
   try { d->sd->SetKrylov(solver ? solver : "", kdim); return 0; } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}
// out3i = { solver: 0 PCG, 1 GMRES; kdim (0 for PCG); chunk of the multi-dot kernel }, out3 = { restarts, second Gram-Schmidt passes - both over all
// solves of the run's solver - and the bytes of its basis (0 before the first GMRES solve) }
int exa_driver_krylov_info(exa_driver* d, int* out3i, int64_t* out3) {
   KrylovSolver& k = d->sd->krylov();
   out3i[0] = k.gmres() ? 1 : 0; out3i[1] = k.gmres() ? k.set.kdim : 0; out3i[2] = gm_chunk();
   out3[0] = out3[1] = out3[2] = 0;
   if (k.gmres()) { const GMRESSolver& g = static_cast<const GMRESSolver&>(k); out3[0] = g.restarts; out3[1] = g.reorth_passes; out3[2] = (int64_t)g.basis_bytes(); }
   return 0;
}
int exa_gmres_multidot_chunk(void) { return gm_chunk(); }   // basis vectors per pass of the multi-dot kernel, a compile-time constant
// Probe of GMRES, mirroring exa_driver_pcg_solve: K_uu x_m = b_m from x = 0 for nrhs <= 16 host columns in turn, in a GMRES solver of the probe's own
// with the run's preconditioner.  ortho: -1 as EXA_GMRES_ORTHO says, 0 ifneeded, 1 always, 2 never, 3 mgs.  Per column: x, Arnoldi steps, flag,
// reduction = last residual / beta0, scalars4[4 m ...] = { beta0, last residual norm, restarts, second Gram-Schmidt passes }.
int exa_driver_gmres_solve(exa_driver* d, int nrhs, const double* b, double rel_tol, double abs_tol, int max_iter, int kdim, int check_every, int ortho, double* x, int* iters,
                           int* flags, double* reduction, double* scalars4, char* err, int errlen) {
   try {
      d->sd->GmresSolveProbe(nrhs, b, rel_tol, abs_tol, max_iter, kdim, check_every, ortho, x, iters, flags, reduction, scalars4);
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}
// The two bandwidth kernels of the orthogonalisation on any shape: w (n) against the k vectors V (k x n, row j = v_j) in the product weighted by
// weight (n); flag != 0: the kernels' gate is closed.  mode as ortho above (>= 0).  h (k): the column of H; w_out (n); wnorm2 = |w_out|^2 from the
// partial sums of the subtraction kernel; passes: 0 with the gate closed, else 1 + second passes.
int exa_gmres_ortho_probe(int64_t n, int k, const double* weight, const double* V, const double* w, double flag, int mode, double* h, double* w_out, double* wnorm2, int* passes,
                          char* err, int errlen) {
   try { gmres_ortho_probe(n, k, weight, V, w, flag, mode, h, w_out, wnorm2, passes); return 0; } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}
// measurement hook of scripts/gmres_compare.py, no part of a run: timing of the same launches on device buffers of the call's own, ms per orthogonalisation (and normalisation) of column col, col + 1 basis vectors
int exa_gmres_ortho_bench(int64_t n, int col, int mode, int reps, double* ms, char* err, int errlen) {
   try { *ms = gmres_ortho_bench(n, col, mode, reps); return 0; } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}
// Host only, no GPU call: the small algebra the scalar kernel runs (gmres_small.hpp).  Hbar: ncols columns at leading dimension ncols + 1, column i
// holding h_0i ... h_i+1,i as Gram-Schmidt leaves them; beta: the first residual norm.  resid (ncols): |s_i+1| after column i; flags (ncols): what
// the solver would decide after that column with the bound final_norm and no iteration cap; y (ncols): the back-substitution over all columns.
// Returns 1 when the back-substitution met no zero pivot, 0 when it did (those y_i are 0).
int exa_gmres_column_probe(int ncols, const double* Hbar, double beta, double final_norm, double* resid, int* flags, double* y) {
   if (ncols < 1 || ncols > gmres::MAXK) return -1;
   const int ld = ncols + 1;
   std::vector<double> H(Hbar, Hbar + (size_t)ld * ncols), cs(ncols), sn(ncols), s(ncols + 1, 0.0);
   s[0] = beta;
   for (int i = 0; i < ncols; i++) {
      const double hn = H[(size_t)i * ld + i + 1];
      resid[i] = gmres::column_update(i, H.data() + (size_t)i * ld, cs.data(), sn.data(), s.data());
      flags[i] = (int)gmres::step_flag(resid[i], final_norm, hn, i + 1.0, 1e300);
   }
   return gmres::back_substitute(ncols, H.data(), ld, s.data(), y) ? 1 : 0;
}

// columns per pass of the batched route (1 .. 3; 0: the library's default) and what the automatic route picks where both exist (batched != 0)
int exa_driver_set_tangent_route(exa_driver* d, int nch, int auto_batched) {
   if (nch < 0 || nch > 3) return -1;
   d->sd->tangent_nch = nch; d->sd->tangent_auto_batched = auto_batched != 0;
   return 0;
}

// host only: C_pp - C_pf C_ff^-1 C_fp of c81[9 (kl) + (mn)] for the free mask free9 (row by row); out81: the condensed tangent in the prescribed rows /
// columns, zeros in the free ones.  Returns 0, or -1 when C_ff is singular.
int exa_macro_tangent_condense(const double* c81, const int* free9, double* out81) {
   uint8_t f[9]; free_mask_bits(free9, f);
   return macro_tangent_condense(c81, f, out81) ? 0 : -1;
}

// [Visualizations] macro_tangent keys of an options file: out2 = { macro_tangent (0 / 1), macro_tangent_max_iter (0: the Krylov value) },
// rel_tol (0: the Krylov value), fname
int exa_options_macro_tangent(const char* toml_path, int* out2, double* rel_tol, char* fname, int fnamelen, char* err, int errlen) {
   try {
      ExaOptions o; o.parse_options(toml_path);
      out2[0] = o.macro_tangent ? 1 : 0; out2[1] = o.macro_tangent_max_iter; *rel_tol = o.macro_tangent_rel_tol;
      if (fname && fnamelen > 0) { if ((int)o.macro_tangent_fname.size() >= fnamelen) throw std::runtime_error("Visualizations.macro_tangent_fname longer than the buffer"); std::strcpy(fname, o.macro_tangent_fname.c_str()); }
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

// out8 = { periodic (0 / 1), local groups of 2 / 4 / 8 images, canonical ids exchanged with other ranks (summed over the neighbours), neighbours, 0, 0 };
// vel_grad9 = the macroscopic velocity gradient in force (zeros when not periodic)
int exa_driver_periodic_info(exa_driver* d, int64_t* out8, double* vel_grad9) {
   try {
      const SystemDriver& sd = *d->sd; const Partition& p = sd.part;
      for (int k = 0; k < 8; k++) out8[k] = 0;
      for (int k = 0; k < 9; k++) vel_grad9[k] = 0.0;
      if (!p.periodic) return 0;
      out8[0] = 1; out8[1] = p.grp_count[0]; out8[2] = p.grp_count[1]; out8[3] = p.grp_count[2];
      for (const Neighbor& nb : p.nbrs) out8[4] += (int64_t)nb.dofs.size() / 3;
      out8[5] = (int64_t)p.nbrs.size();
      for (int k = 0; k < 9; k++) vel_grad9[k] = sd.vgrad_in_force()[k];
      return 0;
   } catch (const std::exception& e) { std::fprintf(stderr, "exa_driver_periodic_info: %s\n", e.what()); return -1; }
}

// which: 0 velocity, 1 current coordinates (after a completed step: its end), 2 reference coordinates; out [local nodes][3] or NULL; returns the local node count
int exa_driver_get_nodal(exa_driver* d, int which, double* out, char* err, int errlen) {
   try {
      SystemDriver& sd = *d->sd; NonlinearMechOperator& op = sd.oper();
      if (which < 0 || which > 2) throw std::runtime_error("exa_driver_get_nodal: field must be 0 (velocity), 1 (coords) or 2 (coords_ref)");
      const int nn = sd.part.NN;
      if (out) {
         const std::vector<double> h = (which == 0 ? sd.v_sol : (which == 1 ? op.x_cur : op.x_ref)).to_host(op.stream());
         for (int g = 0; g < nn; g++) for (int c = 0; c < 3; c++) out[3 * (size_t)g + c] = h[g + (size_t)nn * c];
      }
      return nn;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

// out2 = { residual norm the last Newton solve ended with, its bound max(rel |r0|, abs) }
int exa_driver_newton_info(exa_driver* d, double* out2) { out2[0] = d->sd->last_newton_norm; out2[1] = d->sd->last_newton_bound; return 0; }

// multigrid on a periodic cell is opt-in (Solvers.Krylov.mg_periodic): on != 0 lets exa_driver_set_preconditioner(2) and exa_driver_set_periodic meet
int exa_driver_set_mg_periodic(exa_driver* d, int on) { d->sd->AllowPeriodicMultigrid(on != 0); return 0; }

// multigrid at p_refinement = 2 is opt-in too (Solvers.Krylov.mg_p2): on != 0 before exa_driver_set_preconditioner(2)
int exa_driver_set_mg_p2(exa_driver* d, int on) { d->sd->AllowP2Multigrid(on != 0); return 0; }
// ... and so is multigrid under integ_model = "BBAR" (Solvers.Krylov.mg_bbar)
int exa_driver_set_mg_bbar(exa_driver* d, int on) { d->sd->AllowBbarMultigrid(on != 0); return 0; }
// p = 2 hierarchy, from the next set-up on: 1 level 1 and the fine diagonal from the point records where they can serve, 0 always probed
int exa_driver_set_mg_p2_build(exa_driver* d, int from_records) { d->sd->oper().mg_p2_build = from_records != 0 ? 1 : 0; return 0; }

int exa_driver_set_preconditioner(exa_driver* d, int kind, int levels, int degree, char* err, int errlen) {
   try { d->sd->SetPreconditioner(kind, levels, degree); return 0; } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

}  // extern "C"
namespace {
Multigrid& mg_of(exa_driver* d) {
   NonlinearMechOperator& op = d->sd->oper();
   if (op.precond != Precond::MULTIGRID || !op.mg) throw std::runtime_error("the driver has no multigrid preconditioner (exa_driver_set_preconditioner)");
   return *op.mg;
}
void check_level(Multigrid& mg, int l, bool transfer) {
   if (l < 0 || l > mg.levels() - (transfer ? 1 : 0)) throw std::runtime_error("multigrid: level " + std::to_string(l) + " does not exist");
}
}
extern "C" {

// out (>= 6 + 4 (levels + 1) doubles): { coarse levels L, ms of the last hierarchy set-up, ms of the last V-cycle, smoother degree,
// then per level l = 0 ... L: local elements per direction (3), lmax estimate of D^-1 A_l (0 before the first set-up),
// then: 1 on a periodic cell, free control entries in the control block of mixed loading (0 before the first set-up) }
int exa_driver_mg_info(exa_driver* d, double* out) {
   try {
      Multigrid& mg = mg_of(d);
      out[0] = mg.levels(); out[1] = mg.setup_ms; out[2] = mg.vcycle_ms(); out[3] = mg.degree();
      for (int l = 0; l <= mg.levels(); l++) {
         for (int k = 0; k < 3; k++) out[4 + 4 * l + k] = (mg.grid(l).n[k] - 1) / mg.order(l);   // (element boxes: levels 0 and 1 of a p = 2 hierarchy carry the same one)
         out[4 + 4 * l + 3] = mg.lmax(l);
      }
      out[4 + 4 * (mg.levels() + 1)] = mg.periodic() ? 1.0 : 0.0; out[5 + 4 * (mg.levels() + 1)] = mg.control_dofs();
      return 0;
   } catch (const std::exception& e) { std::fprintf(stderr, "exa_driver_mg_info: %s\n", e.what()); return -1; }
}

// out (>= 2 + L + 1 ints): { coarse levels L, level-1 build of the last set-up (0 probe, 1 records, -1 none yet / p = 1), order of every level }
int exa_driver_mg_info_order(exa_driver* d, int* out) {
   try {
      Multigrid& mg = mg_of(d);
      out[0] = mg.levels(); out[1] = mg.level1_build();
      for (int l = 0; l <= mg.levels(); l++) out[2 + l] = mg.order(l);
      return 0;
   } catch (const std::exception& e) { std::fprintf(stderr, "exa_driver_mg_info_order: %s\n", e.what()); return -1; }
}

// 1 where the hierarchy stands on the B-bar operator (Solvers.Krylov.mg_bbar), 0 otherwise, -1 without a multigrid preconditioner
int exa_driver_mg_bbar(exa_driver* d) {
   try { return mg_of(d).bbar() ? 1 : 0; } catch (const std::exception&) { return -1; }
}

// gradient set-up of the current state (what the next Newton iteration would do first) and the hierarchy build that follows it
int exa_driver_mg_setup(exa_driver* d, char* err, int errlen) {
   try { (void)mg_of(d); d->sd->oper().GetGradient(); return 0; } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

int64_t exa_driver_mg_level_dofs(exa_driver* d, int level) {
   try { Multigrid& mg = mg_of(d); check_level(mg, level, false); return mg.level_dofs(level); }
   catch (const std::exception& e) { std::fprintf(stderr, "exa_driver_mg_level_dofs: %s\n", e.what()); return -1; }
}

int exa_driver_mg_apply(exa_driver* d, int level, const double* x, double* y) {
   try {
      Multigrid& mg = mg_of(d); check_level(mg, level, false);
      const size_t n = mg.level_dofs(level); hipStream_t s = d->sd->oper().stream();
      DevBuf<double> dx(n), dy(n); dx.upload(x, n, s);
      mg.LevelApply(level, dx.p, dy.p); dy.download(y, n, s);
      return 0;
   } catch (const std::exception& e) { std::fprintf(stderr, "exa_driver_mg_apply: %s\n", e.what()); return -1; }
}

int exa_driver_mg_diag(exa_driver* d, int level, double* out) {
   try {
      Multigrid& mg = mg_of(d); check_level(mg, level, false);
      const size_t n = mg.level_dofs(level); hipStream_t s = d->sd->oper().stream();
      DevBuf<double> dy(n); mg.LevelDiag(level, dy.p); dy.download(out, n, s);
      return 0;
   } catch (const std::exception& e) { std::fprintf(stderr, "exa_driver_mg_diag: %s\n", e.what()); return -1; }
}

// dir 0: out (level l) = P in (level l + 1); dir 1: out (level l + 1) = restriction of in (level l)
int exa_driver_mg_transfer(exa_driver* d, int level, int dir, const double* in, double* out) {
   try {
      Multigrid& mg = mg_of(d); check_level(mg, level, true);
      if (dir != 0 && dir != 1) throw std::runtime_error("dir must be 0 (prolongation) or 1 (restriction)");
      const size_t nf = mg.level_dofs(level), nc = mg.level_dofs(level + 1); hipStream_t s = d->sd->oper().stream();
      DevBuf<double> di(dir == 0 ? nc : nf), dout(dir == 0 ? nf : nc);
      di.upload(in, di.n, s);
      if (dir == 0) mg.Prolong(level, di.p, dout.p); else mg.Restrict(level, di.p, dout.p);
      dout.download(out, dout.n, s);
      return 0;
   } catch (const std::exception& e) { std::fprintf(stderr, "exa_driver_mg_transfer: %s\n", e.what()); return -1; }
}

// the coarse operator of level l >= 1 as stored: 243 doubles per node, [(o * 9 + 3 r + c) * NN + node] (mg_kernels.hip)
int exa_driver_mg_stencil(exa_driver* d, int level, double* out) {
   try {
      Multigrid& mg = mg_of(d); check_level(mg, level, false);
      if (level < 1) throw std::runtime_error("level 0 has no stored stencil");
      const size_t n = (size_t)MG_STENCIL * (mg.level_dofs(level) / 3);
      EXA_HC(hipMemcpyAsync(out, mg.stencil(level), sizeof(double) * n, hipMemcpyDeviceToHost, d->sd->oper().stream()));
      EXA_HC(hipStreamSynchronize(d->sd->oper().stream()));
      return 0;
   } catch (const std::exception& e) { std::fprintf(stderr, "exa_driver_mg_stencil: %s\n", e.what()); return -1; }
}

int exa_driver_precond_apply(exa_driver* d, const double* r, double* z) {
   try {
      Multigrid& mg = mg_of(d);
      const size_t n = mg.level_dofs(0); hipStream_t s = d->sd->oper().stream();
      DevBuf<double> dr(n), dz(n); dr.upload(r, n, s);
      mg.Apply(dr.p, dz.p); dz.download(z, n, s);
      return 0;
   } catch (const std::exception& e) { std::fprintf(stderr, "exa_driver_precond_apply: %s\n", e.what()); return -1; }
}

int exa_driver_num_steps(exa_driver* d) { return d->sd->options().nsteps; }
int64_t exa_driver_local_qpts(exa_driver* d) { return (int64_t)d->sd->part.E * d->sd->part.qpts(); }
// out8 = { geometry (EXA_GEOM_*), order, nodes per element, points per element, local elements, local nodes, action route
//          (NonlinearMechOperator::action_route), 0 }
int exa_driver_mesh_info(exa_driver* d, int64_t* out8) {
   try {
      const Partition& p = d->sd->part;
      out8[0] = p.geom; out8[1] = p.p; out8[2] = p.n; out8[3] = p.qpts(); out8[4] = p.E; out8[5] = p.NN; out8[6] = d->sd->oper().action_route(); out8[7] = 0;
      return 0;
   } catch (const std::exception& e) { std::fprintf(stderr, "exa_driver_mesh_info: %s\n", e.what()); return -1; }
}
int64_t exa_driver_local_dofs(exa_driver* d) { return (int64_t)d->sd->part.NN * 3; }

int exa_driver_step(exa_driver* d, int ti, char* err, int errlen) {
   try { return d->sd->Step(ti) ? 1 : 0; } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

// the step's Newton/PCG solve without the end-of-step update (bench: the timed constitutive passes that follow repeat the step's converged launch)
int exa_driver_step_nocommit(exa_driver* d, int ti, char* err, int errlen) {
   try { return d->sd->Step(ti, false) ? 1 : 0; } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

// ... and its end-of-step update afterwards (bench: the solve goes on from the step whose converged launch was timed)
int exa_driver_commit_step(exa_driver* d, char* err, int errlen) {
   try { d->sd->CommitStep(); return 0; } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

int exa_driver_run(exa_driver* d, char* err, int errlen) {
   try { return d->sd->RunAll(); } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1000000; }
}

// which: 0 stress (6), 1 def_grad (9), 2 pl_work (1), 3 dp_tensor (6); returns rows copied
int exa_driver_get_avgs(exa_driver* d, int which, double* out, int maxrows) {
   const std::vector<double>* v = which == 0 ? &d->sd->avg_stress : (which == 1 ? &d->sd->avg_def_grad : (which == 2 ? &d->sd->avg_pl_work : &d->sd->avg_dp_tensor));
   const int w = which == 0 ? 6 : (which == 1 ? 9 : (which == 2 ? 1 : 6));
   int rows = (int)(v->size() / w); if (rows > maxrows) rows = maxrows;
   std::memcpy(out, v->data(), sizeof(double) * rows * w);
   return rows;
}

int exa_driver_get_stats(exa_driver* d, int* newton, int* krylov, int* model_calls, int maxrows) {
   int rows = (int)d->sd->stats.size(); if (rows > maxrows) rows = maxrows;
   for (int i = 0; i < rows; i++) { newton[i] = d->sd->stats[i].newton_iters; krylov[i] = d->sd->stats[i].krylov_iters; model_calls[i] = d->sd->stats[i].model_calls; }
   return rows;
}

// out[0] ms in the fused constitutive kernel, out[1] ms in PCG, out[2] ms in Solve (+SolveInit), out[3] qpt updates, out[4] PCG iterations
void exa_driver_get_timers(exa_driver* d, double* out) {
   d->sd->oper().FlushModelTimers();
   const Timers& t = d->sd->oper().timers; const KrylovSolver& k = d->sd->krylov();
   out[0] = t.t_model_ms; out[1] = k.krylov_ms; out[2] = t.t_solve_ms; out[3] = (double)t.qpt_updates; out[4] = (double)k.krylov_iters;
}
void exa_driver_reset_timers(exa_driver* d) { d->sd->oper().FlushModelTimers(); d->sd->oper().timers = Timers(); d->sd->krylov().ResetTotals(); }   // pending event pairs belong to the old totals
// out[0] quadrature points whose local solve failed (sum over all constitutive launches, this rank), out[1] linear solves that
// did not converge, out[2] PCG iterations that saw (Ad, d) < 0, out[3] flag of the last PCG solve (1 converged, 2 max_iter, -1 den == 0)
void exa_driver_get_diagnostics(exa_driver* d, int64_t* out) {
   d->sd->oper().ReadModelStatus();
   const KrylovSolver::Diagnostics& k = d->sd->krylov().diag;
   out[0] = d->sd->oper().model_fail_total; out[1] = k.not_converged; out[2] = k.indefinite_iters; out[3] = k.last_flag;
}
// launches of exa_slip_rates_from_state so far (lean end-of-step state: NonlinearMechOperator::EnsureSlipRates)
int64_t exa_driver_get_rate_launches(exa_driver* d) { return d->sd->oper().rate_launches; }
void exa_driver_get_record_launches(exa_driver* d, int64_t* out2) {
   long long n[2] = { 0, 0 };
   (void)exa_model_record_launches(d->sd->oper().GetModel()->ctx(), n);
   out2[0] = n[0]; out2[1] = n[1];
}
// launches of exa_element_fields so far (StepAnalyses::rows launches only when the rows it holds are not those of the state at hand)
int64_t exa_driver_get_field_launches(exa_driver* d) { return d->sd->analyses().field_launches; }

// out[0] = sqrt((r, M^-1 r) / (r0, M^-1 r0)) reached by the last PCG solve, out[1] = the worst value among the solves that stopped at max_iter
void exa_driver_get_pcg_reduction(exa_driver* d, double* out2) { out2[0] = d->sd->krylov().diag.last_reduction; out2[1] = d->sd->krylov().diag.worst_capped_reduction; }

// which: 1 = end-of-step state of the last constitutive launch, 0 = begin-of-step state (after a completed step: that step's converged launch)
int exa_driver_nfev_hist_of(exa_driver* d, int which, int* hist64, char* err, int errlen) {
   try {
      NonlinearMechOperator& op = d->sd->oper();
      const double* st = which == 0 ? op.matVars0.p : op.matVars1.p;
      if (exa_model_nfev_hist(op.GetModel()->ctx(), st, hist64, op.stream()) != EXA_OK) throw std::runtime_error(exa_last_error(op.GetModel()->ctx()));
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}
int exa_driver_nfev_hist(exa_driver* d, int* hist64, char* err, int errlen) { return exa_driver_nfev_hist_of(d, 1, hist64, err, errlen); }

int exa_driver_get_qf_component(exa_driver* d, int which, int comp, double* out, char* err, int errlen) {
   try {
      NonlinearMechOperator& op = d->sd->oper();
      const DevBuf<double>* b = which == 0 ? &op.matVars0 : (which == 1 ? &op.matVars1 : (which == 2 ? &op.stress0 : &op.stress1));
      const int W = which < 2 ? 28 : 6;
      if (comp < 0 || comp >= W) throw std::runtime_error("exa_driver_get_qf_component: component out of range");
      if (which < 2 && comp >= 14 && comp < 26) op.EnsureSlipRates(*b);   // slip rates of a lean state: written now
      EXA_HC(hipStreamSynchronize(op.stream()));
      const std::vector<double> h = b->to_host();
      const exa_ctx* ctx = op.GetModel()->ctx();
      const int Q = exa_qpts_per_elem(ctx); const int64_t E = d->sd->part.E;
      const bool blk = exa_get_quadrature_layout(ctx) == EXA_QLAYOUT_EB64;
      for (int64_t e = 0; e < E; e++)
         for (int q = 0; q < Q; q++)
            out[e * Q + q] = blk ? h[((((e >> 6) * Q + q) * (int64_t)W + comp) << 6) + (e & 63)] : h[(int64_t)W * (q + (int64_t)Q * e) + comp];
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

// ---- benchmark hooks --------------------------------------------------------------------------------------------------
// Kinematically drive the RVE into the plastic regime: nodal velocity v = L0 x (+ seeded perturbation), `nsteps` constitutive
// passes with state/coordinate updates and no equilibrium solve (SURVEY 8(d) kernel micro-benchmark).
int exa_driver_bench_prepare(exa_driver* d, int nsteps, const double* dts, double perturb, char* err, int errlen) {
   try {
      SystemDriver& sd = *d->sd; NonlinearMechOperator& op = sd.oper();
      const Partition& part = sd.part; const int nn = part.NN;
      d->v_kin.assign((size_t)3 * nn, 0.0);
      const double L0[3][3] = { { -0.45e-3, 0.3e-4, -0.2e-4 }, { -0.3e-4, -0.45e-3, 0.1e-4 }, { 0.2e-4, -0.1e-4, 1.0e-3 } };
      for (int g = 0; g < nn; g++) {
         const double x[3] = { part.X[g], part.X[g + nn], part.X[g + 2 * (size_t)nn] };
         // deterministic perturbation from the GLOBAL node coordinates so that duplicated interface nodes agree across ranks
         for (int c = 0; c < 3; c++) {
            const double ph = std::sin(12.9898 * x[0] * part.N[0] + 78.233 * x[1] * part.N[1] + 37.719 * x[2] * part.N[2] + 4.0 * c) * 43758.5453;
            const double u = 2.0 * (ph - std::floor(ph)) - 1.0;
            d->v_kin[g + (size_t)nn * c] = L0[c][0] * x[0] + L0[c][1] * x[1] + L0[c][2] * x[2] + perturb * 1.0e-4 / part.N[0] * u;
         }
      }
      sd.v_sol.upload(d->v_kin);
      for (int i = 0; i < nsteps; i++) {
         op.SetDt(dts[i]);
         op.Setup<true>(sd.v_sol.p);
         op.UpdateModel(); op.SwapCoords();
      }
      sd.analyses().Invalidate();   // (the state was swapped without a commit)
      op.SetDt(dts[nsteps > 0 ? nsteps - 1 : 0]);   // nsteps == 0: keep the virgin state, passes are then the elastic first step with dt = dts[0]
      EXA_HC(hipStreamSynchronize(op.stream()));
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

// `steps` constitutive passes (restriction + geometric factors + fused model kernel) from the fixed begin-of-step state, as the
// residual evaluations of one Newton solve do.  out[0] = wall ms of the whole loop (HIP events), out[1] = ms inside the fused
// constitutive kernel only, out[2] = non-converged points of the last pass.
int exa_driver_bench_model(exa_driver* d, int steps, double* out, char* err, int errlen) {
   try {
      SystemDriver& sd = *d->sd; NonlinearMechOperator& op = sd.oper();
      hipStream_t s = op.stream();
      hipEvent_t e0, e1; EXA_HC(hipEventCreate(&e0)); EXA_HC(hipEventCreate(&e1));
      op.FlushModelTimers();
      const double t0 = op.timers.t_model_ms;
      const std::string rname = "timed_region_model[passes=" + std::to_string(steps) + "]";   // the bench's warm-up / elastic / plastic loops differ in length
      ProfRegion prof(rname.c_str());
      EXA_HC(hipEventRecord(e0, s));
      for (int i = 0; i < steps; i++) op.Setup<true>(sd.v_sol.p);
      EXA_HC(hipEventRecord(e1, s)); EXA_HC(hipEventSynchronize(e1));
      float ms = 0; EXA_HC(hipEventElapsedTime(&ms, e0, e1)); (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
      op.FlushModelTimers(); op.ReadModelStatus();
      out[0] = ms; out[1] = op.timers.t_model_ms - t0; out[2] = (double)op.model_fail;
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

// Fixed-length PCG: residual + Jacobian set-up at the prepared state, then exactly `iters` PCG iterations (tolerances disabled).
// out[0] = ms of the PCG loop, out[1] = iterations executed, out[2] = ms of `iters` back-to-back gradient-action launches alone.
int exa_driver_bench_pcg(exa_driver* d, int iters, double* out, char* err, int errlen) {
   try {
      SystemDriver& sd = *d->sd; NonlinearMechOperator& op = sd.oper();
      hipStream_t s = op.stream(); const int nd = op.Height();
      DevBuf<double> r(nd), c(nd);
      op.Mult(sd.v_sol.p, r.p);
      op.GetGradient();
      // a solver of the hook's own (the run's chunk length and graph limit): its captured chunk, which refers to the local solution buffer c, goes
      // with it, and the run's diagnostics and totals do not see the capped solve
      PCGSolver::Settings ks = sd.krylov().set;
      ks.rel_tol = 0.0; ks.abs_tol = 0.0; ks.max_iter = iters;
      PCGSolver k(op, ks);
      const std::string rname = "timed_region_pcg[iters=" + std::to_string(iters) + "]";
      ProfRegion prof(rname.c_str());
      const int it = k.Solve(r.p, c.p);
      out[0] = k.krylov_ms; out[1] = it;
      hipEvent_t e0, e1; EXA_HC(hipEventCreate(&e0)); EXA_HC(hipEventCreate(&e1));
      EXA_HC(hipEventRecord(e0, s));
      for (int i = 0; i < iters; i++) exa_grad_apply_lvec(op.GetModel()->ctx(), r.p, c.p, op.ess_mask.p, s);
      EXA_HC(hipEventRecord(e1, s)); EXA_HC(hipEventSynchronize(e1));
      float ms = 0; EXA_HC(hipEventElapsedTime(&ms, e0, e1)); (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
      out[2] = ms;
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

// The drop-in route at the driver's current state: exactly the calls the MFEM adapters of include/exaconstit_mfem_adapters.hpp make
// (HipExaModel::ModelSetup -> exa_model_setup on the reference's (vdim, Q, E) quadrature functions with a Jacobian field and a velocity
// E-vector; HipExaNLFIntegrator::AssembleGradPA -> exa_grad_setup; AddMultGradPA -> exa_grad_apply on E-vectors between the element
// restriction and its transpose, which MFEM's nonlinear form performs around it: spec reference src/mechanics_operator_ext.cpp:149-157),
// on a second context in the AOS layout that is given this driver's begin-of-step state, coordinates and velocity.  `steps` timed
// constitutive launches, `iters` timed gradient actions; results compared with what the driver's own route produced from the same state.
//   out[0]  ms per exa_model_setup launch                     out[1]  ms per pass = velocity L->E + exa_model_setup
//   out[2]  ms of coordinates L->E + exa_jacobians            out[3]  ms per exa_grad_setup
//   out[4]  ms per exa_grad_apply (E-vector kernel alone)     out[5]  ms per action = L->E + exa_grad_apply + E->L
//   out[6]  max |stress1 - driver's| / max |stress1|          out[7]  max |state1 - driver's| / max |state1|
//   out[8]  max |K x - driver's K x| / max |K x|              out[9]  non-converged points
//   out[10] ms per launch of the driver's own route at this state (same loop)      out[11] ms of the driver's own gradient action
//   out[12] AOS staging through LDS in effect (1 / 0)         out[13] points whose evaluation count (state slot 3, left out of out[7]) differs
// and the L-vector pair (HipExaModelLVec / HipExaNLFIntegratorLVec) on the same context and quadrature functions:
//   out[14] ms per exa_model_setup_lvec launch (gathers + Jacobians + update, AOS rows staged)      out[15] ms per exa_grad_apply_lvec (gather + action + scatter)
//   out[16] max |stress1 - driver's| / max |stress1|          out[17] ms per exa_grad_setup with the compact tangent form
//   out[18] max |K x - driver's K x| / max |K x|              out[19] ms per exa_residual_lvec
//   out[20] ms per exa_model_setup_lvec_records on the reference layout (records instead of the tangent field: no exa_grad_setup)
//   out[21] its max |stress1 - driver's| / max |stress1|      out[22] max |K x - driver's K x| / max |K x| of the action on its records      out[23] 0
int exa_driver_bench_adapter_route(exa_driver* d, int steps, int iters, double* out, char* err, int errlen) {
   try {
      SystemDriver& sd = *d->sd; NonlinearMechOperator& op = sd.oper();
      if (sd.part.p != 1 || sd.comm.nranks != 1) throw std::runtime_error("exa_driver_bench_adapter_route: one rank, p = 1");
      hipStream_t s = op.stream(); const int nd = op.Height(); const int nn = nd / 3;
      const int64_t E = sd.part.E; const int Q = 8; const int64_t P = E * Q;
      for (int i = 0; i < 24; i++) out[i] = 0.0;
      // the driver's own residual evaluation + gradient data at this state: the outputs the adapter route is compared with
      DevBuf<double> r(nd), yC(nd), yA(nd);
      op.Mult(sd.v_sol.p, r.p);
      op.GetGradient();
      exa_ctx* ctxC = op.GetModel()->ctx();
      const bool blocked = exa_get_quadrature_layout(ctxC) == EXA_QLAYOUT_EB64;
      auto timed = [&](int n, auto&& body) {
         hipEvent_t e0, e1; EXA_HC(hipEventCreate(&e0)); EXA_HC(hipEventCreate(&e1));
         EXA_HC(hipEventRecord(e0, s));
         for (int i = 0; i < n; i++) body();
         EXA_HC(hipEventRecord(e1, s)); EXA_HC(hipEventSynchronize(e1));
         float ms = 0; EXA_HC(hipEventElapsedTime(&ms, e0, e1)); (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
         return (double)ms / (n > 0 ? n : 1);
      };
      {  ProfRegion prof("adapter_route_reference_launches");
         op.Setup<true>(sd.v_sol.p);
         out[10] = timed(steps, [&] { op.Setup<true>(sd.v_sol.p); });
         op.FlushModelTimers();
         EXA_HC(hipMemsetAsync(yC.p, 0, sizeof(double) * nd, s));
         out[11] = timed(iters, [&] { if (exa_grad_apply_lvec(ctxC, r.p, yC.p, nullptr, s) != EXA_OK) throw std::runtime_error(exa_last_error(ctxC)); });
         EXA_HC(hipMemsetAsync(yC.p, 0, sizeof(double) * nd, s));
         if (exa_grad_apply_lvec(ctxC, r.p, yC.p, nullptr, s) != EXA_OK) throw std::runtime_error(exa_last_error(ctxC));
      }
      // second context: the reference's quadrature-function layout, E-vector entry points
      exa_config cfg = op.cfg_used; cfg.props = op.props.data(); cfg.nprops = (int)op.props.size(); cfg.assembly = EXA_ASSEMBLY_PA; cfg.integ = EXA_INTEG_FULL;
      int ec = 0; exa_ctx* ctxA = exa_create(&cfg, &ec);
      if (!ctxA) throw std::runtime_error("exa_driver_bench_adapter_route: exa_create failed");
      struct Guard { exa_ctx* c; ~Guard() { exa_destroy(c); } } guard{ ctxA };
      auto chk = [&](int rc, const char* what) { if (rc < 0) throw std::runtime_error(std::string(what) + ": " + exa_last_error(ctxA)); };
      chk(exa_set_connectivity(ctxA, op.conn.p, nn), "exa_set_connectivity");
      chk(exa_set_newton_cap_auto(ctxA, 1, 0.0), "exa_set_newton_cap_auto");   // as the adapters' constructors do
      DevBuf<double> sv0((size_t)28 * P), s0((size_t)6 * P), sv1((size_t)28 * P), s1((size_t)6 * P), cm((size_t)36 * P), J((size_t)9 * P), tmp((size_t)28 * P);
      DevBuf<double> elx((size_t)24 * E), elv((size_t)24 * E), ely((size_t)24 * E), sc(3);
      auto to_aos = [&](int W, const DevBuf<double>& src, DevBuf<double>& dst) {
         if (blocked) vk_qf_eb64_to_aos(W, Q, E, src.p, dst.p, s);
         else EXA_HC(hipMemcpyAsync(dst.p, src.p, sizeof(double) * W * P, hipMemcpyDeviceToDevice, s));
      };
      op.EnsureSlipRates(op.matVars0); op.EnsureSlipRates(op.matVars1);   // (the reference launches are compared on all 28 slots)
      to_aos(28, op.matVars0, sv0); to_aos(6, op.stress0, s0);
      const double dt = op.dt();
      // geometric factors of the end-of-step configuration (MFEM: GetGeometricFactors + the re-layout of exa_jacobians_from_geom)
      out[2] = timed(2, [&] { chk(exa_restrict(ctxA, op.x_cur.p, elx.p, s), "exa_restrict"); chk(exa_jacobians(ctxA, elx.p, J.p, s), "exa_jacobians"); });
      chk(exa_restrict(ctxA, sd.v_sol.p, elv.p, s), "exa_restrict");
      auto model = [&] { chk(exa_model_setup(ctxA, dt, J.p, elv.p, s0.p, sv0.p, s1.p, sv1.p, cm.p, s), "exa_model_setup"); };
      model(); model();
      {  ProfRegion prof(("adapter_route_model[passes=" + std::to_string(steps) + "]").c_str());
         out[0] = timed(steps, model); }
      out[1] = timed(steps, [&] { chk(exa_restrict(ctxA, sd.v_sol.p, elv.p, s), "exa_restrict"); model(); });
      out[9] = (double)exa_model_status(ctxA, s);
      out[12] = (double)exa_get_aos_staging(ctxA);
      unsigned long long differing = 0;
      auto rel_diff = [&](int64_t n, const double* a, const double* b, int W = 0, int skip = -1) {
         vk_max_abs_diff(n, a, b, sc.p, s, W, skip);
         double h[3]; EXA_HC(hipMemcpyAsync(h, sc.p, sizeof(h), hipMemcpyDeviceToHost, s)); EXA_HC(hipStreamSynchronize(s));
         std::memcpy(&differing, &h[2], sizeof(differing));
         return h[1] > 0.0 ? h[0] / h[1] : h[0];
      };
      to_aos(6, op.stress1, tmp); out[6] = rel_diff(6 * P, s1.p, tmp.p);
      to_aos(28, op.matVars1, tmp); out[7] = rel_diff(28 * P, sv1.p, tmp.p, 28, 3); out[13] = (double)differing;   // slot 3 = the local solver's evaluation count
      // AssembleGradPA (HipExaNLFIntegrator: the compact tangent + adj(J) records after its defect check)
      {  double defect = 1.0; chk(exa_set_tangent_form(ctxA, EXA_TANGENT_DEV5_BULK_GEO), "exa_set_tangent_form");
         chk(exa_grad_tangent_defect(ctxA, cm.p, &defect, s), "exa_grad_tangent_defect");
         if (!(defect < 1e-11)) throw std::runtime_error("exa_driver_bench_adapter_route: tangent not of the compact form"); }
      chk(exa_grad_setup(ctxA, dt, J.p, cm.p, s), "exa_grad_setup");
      {  ProfRegion prof("adapter_route_grad_setup");
         out[3] = timed(3, [&] { chk(exa_grad_setup(ctxA, dt, J.p, cm.p, s), "exa_grad_setup"); }); }
      // AddMultGradPA between the element restriction and its transpose
      chk(exa_restrict(ctxA, r.p, elx.p, s), "exa_restrict");
      ely.zero(s);
      chk(exa_grad_apply(ctxA, elx.p, ely.p, s), "exa_grad_apply");
      {  ProfRegion prof(("adapter_route_grad_apply[iters=" + std::to_string(iters) + "]").c_str());
         out[4] = timed(iters, [&] { chk(exa_grad_apply(ctxA, elx.p, ely.p, s), "exa_grad_apply"); }); }
      auto action = [&] {
         chk(exa_restrict(ctxA, r.p, elx.p, s), "exa_restrict");
         ely.zero(s);
         chk(exa_grad_apply(ctxA, elx.p, ely.p, s), "exa_grad_apply");
         chk(exa_restrict_transpose_add(ctxA, ely.p, yA.p, s), "exa_restrict_transpose_add");
      };
      {  ProfRegion prof(("adapter_route_action[iters=" + std::to_string(iters) + "]").c_str());
         out[5] = timed(iters, action); }
      EXA_HC(hipMemsetAsync(yA.p, 0, sizeof(double) * nd, s));
      action();
      out[8] = rel_diff(nd, yA.p, yC.p);
      // ---- the L-vector pair on the same quadrature functions
      auto model_lv = [&] { chk(exa_model_setup_lvec(ctxA, dt, op.x_cur.p, sd.v_sol.p, s0.p, sv0.p, s1.p, sv1.p, cm.p, J.p, s), "exa_model_setup_lvec"); };
      model_lv(); model_lv();
      {  ProfRegion prof(("adapter_route_lvec_model[passes=" + std::to_string(steps) + "]").c_str());
         out[14] = timed(steps, model_lv); }
      if (exa_model_status(ctxA, s) != 0) throw std::runtime_error("exa_driver_bench_adapter_route: the L-vector launch left unconverged points");
      to_aos(6, op.stress1, tmp); out[16] = rel_diff(6 * P, s1.p, tmp.p);
      chk(exa_set_tangent_form(ctxA, EXA_TANGENT_DEV5_BULK), "exa_set_tangent_form");
      chk(exa_grad_setup(ctxA, dt, J.p, cm.p, s), "exa_grad_setup");
      out[17] = timed(3, [&] { chk(exa_grad_setup(ctxA, dt, J.p, cm.p, s), "exa_grad_setup"); });
      chk(exa_grad_set_coords(ctxA, op.x_cur.p), "exa_grad_set_coords");
      EXA_HC(hipMemsetAsync(yA.p, 0, sizeof(double) * nd, s));
      chk(exa_grad_apply_lvec(ctxA, r.p, yA.p, nullptr, s), "exa_grad_apply_lvec");
      out[18] = rel_diff(nd, yA.p, yC.p);
      {  ProfRegion prof(("adapter_route_lvec_apply[iters=" + std::to_string(iters) + "]").c_str());
         out[15] = timed(iters, [&] { chk(exa_grad_apply_lvec(ctxA, r.p, yA.p, nullptr, s), "exa_grad_apply_lvec"); }); }
      out[19] = timed(iters, [&] { chk(exa_residual_lvec(ctxA, J.p, s1.p, yA.p, s), "exa_residual_lvec"); });
      // ... and with AssembleGradPA fused into ModelSetup (HipExaModelLVec(.., fused_records = true)): the compact records instead of the tangent field, no exa_grad_setup
      auto model_rec = [&] { chk(exa_model_setup_lvec_records(ctxA, dt, op.x_cur.p, sd.v_sol.p, s0.p, sv0.p, s1.p, sv1.p, J.p, s), "exa_model_setup_lvec_records"); };
      model_rec(); model_rec();
      {  ProfRegion prof(("adapter_route_lvec_records[passes=" + std::to_string(steps) + "]").c_str());
         out[20] = timed(steps, model_rec); }
      if (exa_model_status(ctxA, s) != 0) throw std::runtime_error("exa_driver_bench_adapter_route: the record launch left unconverged points");
      to_aos(6, op.stress1, tmp); out[21] = rel_diff(6 * P, s1.p, tmp.p);
      EXA_HC(hipMemsetAsync(yA.p, 0, sizeof(double) * nd, s));
      chk(exa_grad_apply_lvec(ctxA, r.p, yA.p, nullptr, s), "exa_grad_apply_lvec");
      out[22] = rel_diff(nd, yA.p, yC.p);
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

int exa_choose_newton_cap(const int* hist64, double tail_cost) { return choose_newton_cap(hist64, tail_cost); }
int exa_choose_newton_caps(const int* hist64, double tail_cost, int* k1, int* k2) { if (!hist64 || !k1 || !k2) return -1; choose_newton_caps_resume(hist64, tail_cost, *k1, *k2); return 0; }

int exa_driver_element_fields(exa_driver* d, double* out, int64_t* elem_gid, int32_t* attribute, char* err, int errlen) {
   try {
      SystemDriver& sd = *d->sd;
      if (out) { std::vector<double> f; sd.analyses().ElementFields(sd.state(), f); std::memcpy(out, f.data(), sizeof(double) * f.size()); }
      if (elem_gid) std::memcpy(elem_gid, sd.part.elem_gid.data(), sizeof(int64_t) * sd.part.E);
      if (attribute) std::memcpy(attribute, sd.elem_attr.data(), sizeof(int32_t) * sd.part.E);
      return sd.part.E;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

int exa_driver_write_fields(exa_driver* d, const char* dir, int cycle, double t, char* err, int errlen) {
   try {
      if (!dir || !*dir) throw std::runtime_error("exa_driver_write_fields: no directory");
      d->sd->analyses().SaveFields(d->sd->state(), dir, cycle, t);
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

// out3 = { preconditioner: 0 key absent, 1 "jacobi", 2 "multigrid"; mg_levels (0: as many as the mesh allows); mg_smoother_degree }
int exa_options_query_solver(const char* toml_path, int* out3, char* err, int errlen) {
   try {
      ExaOptions o; o.parse_options(toml_path);
      out3[0] = o.precond; out3[1] = o.mg_levels; out3[2] = o.mg_degree;
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

int exa_mg_level_count(const int* N, int nranks, int cap) { return (nranks < 1 || N[0] < 1 || N[1] < 1 || N[2] < 1) ? -1 : mg_level_count(N, nranks, cap); }
int exa_mg_level_count_order(const int* N, int nranks, int cap, int order) {
   return (nranks < 1 || N[0] < 1 || N[1] < 1 || N[2] < 1 || order < 1 || order > 2) ? -1 : mg_level_count_order(N, nranks, cap, order);
}
int exa_options_query_mg_bbar(const char* toml_path, int* out1, char* err, int errlen) {
   try { ExaOptions o; o.parse_options(toml_path); out1[0] = o.mg_bbar ? 1 : 0; return 0; } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}
int exa_options_query_mg_p2(const char* toml_path, int* out1, char* err, int errlen) {
   try { ExaOptions o; o.parse_options(toml_path); out1[0] = o.mg_p2 ? 1 : 0; return 0; } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

int exa_options_query_vis(const char* toml_path, int* paraview, int* steps, int* light_up, char* floc, int floclen, char* err, int errlen) {
   try {
      ExaOptions o; o.parse_options(toml_path);
      if (paraview) *paraview = o.paraview ? 1 : 0;
      if (steps) *steps = o.vis_steps;
      if (light_up) *light_up = o.light_up ? 1 : 0;
      if (floc && floclen > 0) { if ((int)o.vis_floc.size() >= floclen) throw std::runtime_error("Visualizations.floc longer than the buffer"); std::strcpy(floc, o.vis_floc.c_str()); }
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

int exa_driver_lattice_strains(exa_driver* d, int nhkl, const int* hkl3, const double* s_dir3, double tol_deg, double* strain_out, double* volfrac_out,
                               char* err, int errlen) {
   try {
      if (nhkl < 1 || nhkl > EXA_LATTICE_MAX_HKL || !hkl3 || !s_dir3 || !strain_out || !volfrac_out) throw std::runtime_error("exa_driver_lattice_strains: 1 to 16 families, a direction and two outputs are required");
      const std::vector<int> hkl(hkl3, hkl3 + 3 * nhkl);
      d->sd->analyses().LatticeStrains(d->sd->state(), hkl, s_dir3, tol_deg, strain_out, volfrac_out);
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

int exa_driver_grain_averages(exa_driver* d, int32_t* grain_ids, double* vals, int64_t cap, char* err, int errlen) {
   try {
      std::vector<int32_t> ids; std::vector<double> v;
      d->sd->analyses().GrainAverages(d->sd->state(), ids, v);
      const int64_t n = (int64_t)ids.size();
      if (n <= cap) {
         if (grain_ids) std::memcpy(grain_ids, ids.data(), sizeof(int32_t) * n);
         if (vals) std::memcpy(vals, v.data(), sizeof(double) * v.size());
      }
      return (int)n;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

int exa_driver_lattice_curvature(exa_driver* d, double burgers, double* out, int64_t* elem_gid, int32_t* attribute, double* summary7, char* err, int errlen) {
   try {
      SystemDriver& sd = *d->sd;
      if (out || summary7) {
         std::vector<double> rows; double m[7];
         sd.analyses().LatticeCurvature(sd.state(), burgers, rows, m);
         if (out) std::memcpy(out, rows.data(), sizeof(double) * rows.size());
         if (summary7) std::memcpy(summary7, m, sizeof(m));
      }
      if (elem_gid) std::memcpy(elem_gid, sd.part.elem_gid.data(), sizeof(int64_t) * sd.part.E);
      if (attribute) std::memcpy(attribute, sd.elem_attr.data(), sizeof(int32_t) * sd.part.E);
      return sd.part.E;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

int exa_options_query_lattice_curvature(const char* toml_path, int* enabled, double* burgers, char* fname, int fnamelen, char* err, int errlen) {
   try {
      ExaOptions o; o.parse_options(toml_path);
      if (enabled) *enabled = o.lattice_curvature ? 1 : 0;
      if (burgers) *burgers = o.lattice_curvature_burgers;
      if (fname && fnamelen > 0) {
         if ((int)o.lattice_curvature_fname.size() >= fnamelen) throw std::runtime_error("Visualizations.lattice_curvature_fname longer than the buffer");
         std::strcpy(fname, o.lattice_curvature_fname.c_str());
      }
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

int exa_driver_enable_slip_activity(exa_driver* d, char* err, int errlen) {
   try { d->sd->analyses().EnableSlipActivity(); return 0; } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}
int exa_driver_reset_fatigue_window(exa_driver* d, char* err, int errlen) {
   try { d->sd->analyses().ResetFatigueWindow(d->sd->state()); return 0; } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}
int exa_driver_slip_activity(exa_driver* d, double k_fs, double sigma_y, double* acc_out, double* fip_out, int64_t* elem_gid, int32_t* attribute, double* summary8,
                             int32_t* grain_ids, double* grain_vals3, int64_t grain_cap, int64_t* n_grains, char* err, int errlen) {
   try {
      SystemDriver& sd = *d->sd;
      if (acc_out || fip_out || summary8 || n_grains) {
         StepAnalyses::SlipActivityResult r;
         sd.analyses().SlipActivity(sd.state(), k_fs, sigma_y, r, acc_out != nullptr);
         if (acc_out) std::memcpy(acc_out, r.acc.data(), sizeof(double) * r.acc.size());
         if (fip_out) std::memcpy(fip_out, r.fip.data(), sizeof(double) * r.fip.size());
         if (summary8) std::memcpy(summary8, r.summary, sizeof(r.summary));
         const int64_t n = (int64_t)r.grain_ids.size();
         if (n_grains) *n_grains = n;
         if (n <= grain_cap) {
            if (grain_ids) std::memcpy(grain_ids, r.grain_ids.data(), sizeof(int32_t) * n);
            if (grain_vals3) std::memcpy(grain_vals3, r.grain_vals.data(), sizeof(double) * r.grain_vals.size());
         }
      }
      if (elem_gid) std::memcpy(elem_gid, sd.part.elem_gid.data(), sizeof(int64_t) * sd.part.E);
      if (attribute) std::memcpy(attribute, sd.elem_attr.data(), sizeof(int32_t) * sd.part.E);
      return sd.part.E;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

int exa_options_query_fatigue(const char* toml_path, int* out2, double* out2d, char* fname, int fnamelen, char* err, int errlen) {
   try {
      ExaOptions o; o.parse_options(toml_path);
      if (out2) { out2[0] = o.fatigue ? 1 : 0; out2[1] = o.fatigue_cycle_steps; }
      if (out2d) { out2d[0] = o.fatigue_k; out2d[1] = o.fatigue_sigma_y; }
      if (fname && fnamelen > 0) {
         if ((int)o.fatigue_fname.size() >= fnamelen) throw std::runtime_error("Visualizations.fatigue_fname longer than the buffer");
         std::strcpy(fname, o.fatigue_fname.c_str());
      }
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

int exa_fatigue_write(const char* path, int nrows, const double* rows9, int append, char* err, int errlen) {
   try {
      if (!path || nrows < 0 || (nrows > 0 && !rows9)) throw std::runtime_error("exa_fatigue_write: a path and nrows rows are required");
      write_fatigue_rows(path, std::vector<double>(rows9, rows9 + (size_t)FATIGUE_ROW * nrows), append != 0);
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}
int exa_fatigue_grains_write(const char* path, int n, const int32_t* grain_ids, const double* vals3, char* err, int errlen) {
   try {
      if (!path || n < 0 || (n > 0 && (!grain_ids || !vals3))) throw std::runtime_error("exa_fatigue_grains_write: a path, ids and values are required");
      write_fatigue_grains(path, n, grain_ids, vals3);
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

int exa_driver_set_grains(exa_driver* d, const int32_t* grain_of_global_element, const double* grain_quats, int G, int64_t n_global, char* err, int errlen) {
   try {
      d->sd->SetGrains(grain_of_global_element, n_global, grain_quats, G);
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

int exa_driver_pole_figures(exa_driver* d, int nhkl, const int* hkl3, int ndir, const double* dirs3, double res_deg, double* mrd_out, char* err, int errlen) {
   try {
      if (nhkl < 0 || nhkl > EXA_TEXTURE_MAX_HKL || ndir < 0 || ndir > EXA_TEXTURE_MAX_DIRS || nhkl + ndir < 1 || (nhkl > 0 && !hkl3) || (ndir > 0 && !dirs3) || !mrd_out)
         throw std::runtime_error("exa_driver_pole_figures: 0 to 16 families, 0 to 3 directions (at least one set) and an output are required");
      const std::vector<int> hkl(hkl3, hkl3 + 3 * nhkl);
      std::vector<double> mrd;
      d->sd->analyses().PoleFigures(d->sd->state(), hkl, std::vector<double>(dirs3, dirs3 + 3 * ndir), res_deg, mrd);
      std::memcpy(mrd_out, mrd.data(), sizeof(double) * mrd.size());
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

int exa_options_query_texture(const char* toml_path, int* enabled, int* nhkl, int* hkl48, int* ndir, double* dirs9, double* res_deg, char* fname, int fnamelen,
                              char* err, int errlen) {
   try {
      ExaOptions o; o.parse_options(toml_path);
      if (enabled) *enabled = o.texture ? 1 : 0;
      if (nhkl) *nhkl = (int)o.texture_hkl.size() / 3;
      if (hkl48) for (size_t i = 0; i < o.texture_hkl.size(); i++) hkl48[i] = o.texture_hkl[i];
      if (ndir) *ndir = (int)o.texture_dirs.size() / 3;
      if (dirs9) for (size_t i = 0; i < o.texture_dirs.size(); i++) dirs9[i] = o.texture_dirs[i];
      if (res_deg) *res_deg = o.texture_res_deg;
      if (fname && fnamelen > 0) {
         if ((int)o.texture_fname.size() >= fnamelen) throw std::runtime_error("Visualizations.texture_fname longer than the buffer");
         std::strcpy(fname, o.texture_fname.c_str());
      }
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

int exa_options_query_grains(const char* toml_path, int* enabled, char* fname, int fnamelen, char* err, int errlen) {
   try {
      ExaOptions o; o.parse_options(toml_path);
      if (enabled) *enabled = o.grain_avgs ? 1 : 0;
      if (fname && fnamelen > 0) {
         if ((int)o.grain_avgs_fname.size() >= fnamelen) throw std::runtime_error("Visualizations.grain_avgs_fname longer than the buffer");
         std::strcpy(fname, o.grain_avgs_fname.c_str());
      }
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

int exa_grain_avgs_write(const char* path, int n, const int32_t* grain_ids, const double* vals, char* err, int errlen) {
   try {
      if (!path || n < 0 || (n > 0 && (!grain_ids || !vals))) throw std::runtime_error("exa_grain_avgs_write: a path and n rows are required");
      write_grain_avgs(path, n, grain_ids, vals);
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

int exa_options_query_lightup(const char* toml_path, int* enabled, int* nhkl, int* hkl48, double* s_dir3, double* tol_deg, char* strain_fname,
                              char* volume_fname, int fnamelen, char* err, int errlen) {
   try {
      ExaOptions o; o.parse_options(toml_path);
      if (enabled) *enabled = o.lightup() ? 1 : 0;
      if (nhkl) *nhkl = (int)o.lightup_hkl.size() / 3;
      if (hkl48) for (size_t i = 0; i < o.lightup_hkl.size(); i++) hkl48[i] = o.lightup_hkl[i];
      if (s_dir3) for (int i = 0; i < 3; i++) s_dir3[i] = o.lightup_s_dir[i];
      if (tol_deg) *tol_deg = o.lightup_tol_deg;
      auto put = [&](char* dst, const std::string& v, const char* what) {
         if (!dst || fnamelen <= 0) return;
         if ((int)v.size() >= fnamelen) throw std::runtime_error(std::string(what) + " longer than the buffer");
         std::strcpy(dst, v.c_str());
      };
      put(strain_fname, o.lightup_strain_fname, "Visualizations.light_up_strain_fname");
      put(volume_fname, o.lightup_volume_fname, "Visualizations.light_up_volume_fname");
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

// two unit hexahedra side by side (12 nodes byNODES, node g = i + 3 (j + 2 k) at (i, j, k)) saved as cycles 0 (t = 0) and 1 (t = 0.5) with the
// given field rows: x_cur = x_ref + 0.01 m, velocity 0.5 m for the value index m = g + 12 c; attribute = {1, 2}, GlobalElementId = {10, 11}
int exa_vtu_selftest(const char* dir, const double* fields, int light_up, char* err, int errlen) {
   try {
      const int NN = 12;
      std::vector<double> xr(3 * NN), xc(3 * NN), v(3 * NN);
      for (int g = 0; g < NN; g++) {
         const double ijk[3] = { (double)(g % 3), (double)((g / 3) % 2), (double)(g / 6) };
         for (int c = 0; c < 3; c++) { const int m = g + NN * c; xr[m] = ijk[c]; xc[m] = ijk[c] + 0.01 * m; v[m] = 0.5 * m; }
      }
      std::vector<int32_t> conn(16);
      for (int e = 0; e < 2; e++) {
         static const int V[8][3] = { { 0, 0, 0 }, { 1, 0, 0 }, { 1, 1, 0 }, { 0, 1, 0 }, { 0, 0, 1 }, { 1, 0, 1 }, { 1, 1, 1 }, { 0, 1, 1 } };
         for (int a = 0; a < 8; a++) conn[a + 8 * e] = (e + V[a][0]) + 3 * (V[a][1] + 2 * V[a][2]);
      }
      const int32_t attr[2] = { 1, 2 }; const int64_t gid[2] = { 10, 11 };
      vtu::Piece p;
      p.E = 2; p.NN = NN; p.n = 8; p.conn = conn.data(); p.x_cur = xc.data(); p.x_ref = xr.data(); p.vel = v.data(); p.fields = fields; p.attr = attr; p.gid = gid;
      std::vector<std::pair<int, double>> cycles;
      vtu::save_cycle(dir, 0, 1, 0, 0.0, light_up != 0, p, cycles);
      vtu::save_cycle(dir, 0, 1, 1, 0.5, light_up != 0, p, cycles);
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

int exa_options_query(const char* toml_path, double* out, char* err, int errlen) {
   try {
      ExaOptions o; o.parse_options(toml_path);
      const double v[20] = { o.temp_k, (double)o.nprops, (double)o.num_grains, o.xtal == XtalType::BCC ? 1.0 : 0.0, (double)(int)o.slip, o.dt_cust ? 1.0 : 0.0,
                             o.dt_auto ? 1.0 : 0.0, (double)o.nsteps, o.assembly == Assembly::PA ? 0.0 : 1.0, o.nl_solver == NLSolver::NRLS ? 1.0 : 0.0,
                             (double)o.newton_iter, o.newton_rel, o.newton_abs, (double)o.krylov_iter, o.krylov_rel, o.krylov_abs, (double)o.ref_ser,
                             (double)o.ncuts[0], o.additional_avgs ? 1.0 : 0.0, (double)o.bcs.size() };
      std::memcpy(out, v, sizeof(v));
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

// [BCs] table: out2 = { periodic, boundary-condition entries (update steps) }; vel_grad = 9 values per entry, at most max_entries of them (may be NULL)
int exa_options_query_bcs(const char* toml_path, int* out2, double* vel_grad, int max_entries, char* err, int errlen) {
   try {
      ExaOptions o; o.parse_options(toml_path);
      out2[0] = o.periodic ? 1 : 0; out2[1] = (int)o.bcs.size();
      if (vel_grad) for (int b = 0; b < (int)o.bcs.size() && b < max_entries; b++) std::memcpy(vel_grad + 9 * b, o.bcs[b].vgrad, sizeof(double) * 9);
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

// [BCs] periodic_free: out10 = { mixed loading on (0 / 1), the mask row by row }
int exa_options_query_periodic_free(const char* toml_path, int* out10, char* err, int errlen) {
   try {
      ExaOptions o; o.parse_options(toml_path);
      out10[0] = o.periodic_mixed ? 1 : 0;
      for (int k = 0; k < 9; k++) out10[1 + k] = o.periodic_free[k];
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

// the tables of mixed loading (Partition::make_periodic(true)) of a rank's block: info8 = { local nodes, top-face nodes of direction 0, 1, 2,
// image entries, neighbours, neighbour dofs in all, local groups }; arrays (may be NULL): weight (local nodes), face_nodes (the three lists back to
// back), ctrl4 (local ids of c_0 .. c_3, -1 where not held), img_nodes / img_code (image entries), canon (local nodes), nbr_dofs (concatenated)
int exa_partition_query_periodic_mixed(const int* N, int rank, int nranks, int order, int64_t* info8, double* weight, int32_t* face_nodes, int32_t* ctrl4,
                                       int32_t* img_nodes, uint8_t* img_code, int64_t* canon, int32_t* nbr_dofs) {
   Partition p; const double L[3] = { 1.0, 1.0, 1.0 };
   p.build(N, L, rank, nranks, (order >= 1 && order <= 6) ? order : 1);
   p.make_periodic(true);
   int64_t shared = 0; for (auto& nb : p.nbrs) shared += (int64_t)nb.dofs.size();
   info8[0] = p.NN; for (int d = 0; d < 3; d++) info8[1 + d] = (int64_t)p.face_nodes[d].size();
   info8[4] = (int64_t)p.img_nodes.size(); info8[5] = (int64_t)p.nbrs.size(); info8[6] = shared; info8[7] = (int64_t)p.grp_off.size() - 1;
   if (weight) std::memcpy(weight, p.weight.data(), sizeof(double) * p.weight.size());
   if (face_nodes) { size_t off = 0; for (int d = 0; d < 3; d++) { std::memcpy(face_nodes + off, p.face_nodes[d].data(), sizeof(int32_t) * p.face_nodes[d].size()); off += p.face_nodes[d].size(); } }
   if (ctrl4) for (int k = 0; k < 4; k++) ctrl4[k] = p.ctrl_node[k];
   if (img_nodes) std::memcpy(img_nodes, p.img_nodes.data(), sizeof(int32_t) * p.img_nodes.size());
   if (img_code) std::memcpy(img_code, p.img_code.data(), p.img_code.size());
   if (canon) std::memcpy(canon, p.canon.data(), sizeof(int64_t) * p.canon.size());
   if (nbr_dofs) { size_t off = 0; for (auto& nb : p.nbrs) { std::memcpy(nbr_dofs + off, nb.dofs.data(), sizeof(int32_t) * nb.dofs.size()); off += nb.dofs.size(); } }
   return 0;
}

// the periodic view of a rank's block (Partition::make_periodic): info8 = { local nodes, neighbours, neighbour dofs in all, local groups, their members in
// all, groups of 2, of 4, of 8 }; every array pointer may be NULL: canon / weight (local nodes), nbr_rank / nbr_count (neighbours), nbr_dofs (concatenated),
// grp_off (local groups + 1), grp_nodes (members in all)
int exa_partition_query_periodic(const int* N, int rank, int nranks, int order, int64_t* info8, int64_t* canon, double* weight, int32_t* nbr_rank, int32_t* nbr_count,
                                 int32_t* nbr_dofs, int32_t* grp_off, int32_t* grp_nodes) {
   Partition p; const double L[3] = { 1.0, 1.0, 1.0 };
   p.build(N, L, rank, nranks, (order >= 1 && order <= 6) ? order : 1);
   p.make_periodic();
   int64_t shared = 0; for (auto& nb : p.nbrs) shared += (int64_t)nb.dofs.size();
   info8[0] = p.NN; info8[1] = (int64_t)p.nbrs.size(); info8[2] = shared; info8[3] = (int64_t)p.grp_off.size() - 1; info8[4] = (int64_t)p.grp_nodes.size();
   for (int k = 0; k < 3; k++) info8[5 + k] = p.grp_count[k];
   if (canon) std::memcpy(canon, p.canon.data(), sizeof(int64_t) * p.canon.size());
   if (weight) std::memcpy(weight, p.weight.data(), sizeof(double) * p.weight.size());
   size_t off = 0;
   for (size_t i = 0; i < p.nbrs.size(); i++) {
      if (nbr_rank) nbr_rank[i] = p.nbrs[i].rank;
      if (nbr_count) nbr_count[i] = (int32_t)p.nbrs[i].dofs.size();
      if (nbr_dofs) std::memcpy(nbr_dofs + off, p.nbrs[i].dofs.data(), sizeof(int32_t) * p.nbrs[i].dofs.size());
      off += p.nbrs[i].dofs.size();
   }
   if (grp_off) std::memcpy(grp_off, p.grp_off.data(), sizeof(int32_t) * p.grp_off.size());
   if (grp_nodes) std::memcpy(grp_nodes, p.grp_nodes.data(), sizeof(int32_t) * p.grp_nodes.size());
   return 0;
}

static void export_partition(const Partition& p, int64_t* info, int32_t* conn, double* X, int64_t* elem_gid, double* weight,
                             int32_t* nbr_rank, int32_t* nbr_count, int32_t* nbr_dofs) {
   int64_t shared = 0; for (auto& nb : p.nbrs) shared += (int64_t)nb.dofs.size();
   info[0] = p.E; info[1] = p.NN; info[2] = (int64_t)p.nbrs.size(); info[3] = p.pg[0]; info[4] = p.pg[1]; info[5] = p.pg[2]; info[6] = shared; info[7] = p.n;
   if (conn) std::memcpy(conn, p.conn.data(), sizeof(int32_t) * p.conn.size());
   if (X) std::memcpy(X, p.X.data(), sizeof(double) * p.X.size());
   if (elem_gid) std::memcpy(elem_gid, p.elem_gid.data(), sizeof(int64_t) * p.elem_gid.size());
   if (weight) std::memcpy(weight, p.weight.data(), sizeof(double) * p.weight.size());
   size_t off = 0;
   for (size_t i = 0; i < p.nbrs.size(); i++) {
      if (nbr_rank) nbr_rank[i] = p.nbrs[i].rank;
      if (nbr_count) nbr_count[i] = (int32_t)p.nbrs[i].dofs.size();
      if (nbr_dofs) std::memcpy(nbr_dofs + off, p.nbrs[i].dofs.data(), sizeof(int32_t) * p.nbrs[i].dofs.size());
      off += p.nbrs[i].dofs.size();
   }
}

int exa_partition_query(const int* N, int rank, int nranks, int64_t* info, int32_t* conn, double* X, int64_t* elem_gid, double* weight,
                        int32_t* nbr_rank, int32_t* nbr_count, int32_t* nbr_dofs) {
   Partition p; const double L[3] = { 1.0, 1.0, 1.0 };
   const int order = (info[7] >= 2 && info[7] <= 6) ? (int)info[7] : 1;   // info[7] is in/out: H1 order on input (0/1 -> 1), nodes per element on output
   p.build(N, L, rank, nranks, order);
   export_partition(p, info, conn, X, elem_gid, weight, nbr_rank, nbr_count, nbr_dofs);
   return 0;
}

// the element order the driver runs with on several ranks (Partition::order_boundary_first): out2 = { E, E_bdr }; conn (n, E) and gid (E) may be null
int exa_partition_query_boundary_first(const int* N, int rank, int nranks, int order, int64_t* out2, int32_t* conn, int64_t* elem_gid) {
   Partition p; const double L[3] = { 1.0, 1.0, 1.0 };
   p.build(N, L, rank, nranks, order == 2 ? 2 : 1);
   p.order_boundary_first();
   out2[0] = p.E; out2[1] = p.E_bdr;
   if (conn) std::memcpy(conn, p.conn.data(), sizeof(int32_t) * p.conn.size());
   if (elem_gid) std::memcpy(elem_gid, p.elem_gid.data(), sizeof(int64_t) * p.elem_gid.size());
   return 0;
}

int exa_mesh_partition_query(const char* mesh_path, int rank, int nranks, int64_t* info, int32_t* conn, double* X, int64_t* elem_gid, double* weight,
                             int32_t* nbr_rank, int32_t* nbr_count, int32_t* nbr_dofs, char* err, int errlen) {
   try {
      Partition p; p.build_from_mfem_mesh(mesh_path, rank, nranks);
      export_partition(p, info, conn, X, elem_gid, weight, nbr_rank, nbr_count, nbr_dofs);
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

// the same at p_refinement = order (1 or 2: edge / face / element nodes added to the trilinear file mesh)
int exa_mesh_partition_query_order(const char* mesh_path, int rank, int nranks, int order, int64_t* info, int32_t* conn, double* X, int64_t* elem_gid, double* weight,
                                   int32_t* nbr_rank, int32_t* nbr_count, int32_t* nbr_dofs, char* err, int errlen) {
   try {
      Partition p; p.build_from_mfem_mesh(mesh_path, rank, nranks, order);
      export_partition(p, info, conn, X, elem_gid, weight, nbr_rank, nbr_count, nbr_dofs);
      return 0;
   } catch (const std::exception& e) { set_err(err, errlen, e.what()); return -1; }
}

}  // extern "C"
