// SystemDriver::SaveCheckpoint / LoadCheckpoint: one self-describing file per checkpoint, independent of the decomposition, the
// quadrature layout and the rank count.  Field sections are addressed by global element / node number, so every rank writes (pwrite) and
// reads (pread) the byte ranges of its own elements and of the nodes it owns (lowest rank holding a node); the section checksums are sums of
// 64-bit words and therefore add over ranks.  The quadrature functions pass through exa_qf_pack / exa_qf_unpack (csrc/checkpoint_kernels.hip),
// which also compute their checksums on the device.
#include "driver.hpp"
#include "checkpoint.hpp"
#include <dirent.h>
#include <fcntl.h>
#include <unistd.h>
#include <algorithm>
#include <cmath>
#include <fstream>
#include <iomanip>
#include <unordered_map>

namespace exa_host {

namespace {

using namespace exa_ckpt;

void ck(exa_ctx* ctx, int rc, const char* what) { if (rc < 0) throw std::runtime_error(std::string(what) + ": " + exa_last_error(ctx)); }

// exact sums of 64-bit integers over the ranks through the double all-reduce: four 16-bit digits per value (every partial sum stays below 2^53)
void allreduce_u64(Comm& comm, std::vector<uint64_t>& v, hipStream_t s) {
   if (comm.nranks == 1 || v.empty()) return;
   std::vector<double> h(4 * v.size());
   for (size_t i = 0; i < v.size(); i++) for (int k = 0; k < 4; k++) h[4 * i + k] = (double)((v[i] >> (16 * k)) & 0xffffull);
   DevBuf<double> t(h.size()); t.upload(h.data(), h.size(), s);
   comm.allreduce_sum(t.p, (int)h.size(), s);
   t.download(h.data(), h.size(), s);
   for (size_t i = 0; i < v.size(); i++) { uint64_t r = 0; for (int k = 0; k < 4; k++) r += (uint64_t)h[4 * i + k] << (16 * k); v[i] = r; }
}
// 0 on every rank, or a collective failure: every rank throws the same kind of error instead of leaving its peers in a barrier
void all_ok(Comm& comm, bool ok, const std::string& what) {
   if (comm.max_over_ranks(ok ? 0.0 : 1.0) != 0.0) throw std::runtime_error(what + (ok ? " (on another rank)" : ""));
}

void pwrite_all(int fd, const void* p, size_t n, uint64_t off) {
   const char* c = (const char*)p;
   while (n > 0) { const ssize_t w = ::pwrite(fd, c, n, (off_t)off); if (w <= 0) throw std::runtime_error("checkpoint: write failed"); c += w; n -= (size_t)w; off += (uint64_t)w; }
}
void pread_all(int fd, void* p, size_t n, uint64_t off) {
   char* c = (char*)p;
   while (n > 0) { const ssize_t r = ::pread(fd, c, n, (off_t)off); if (r <= 0) throw std::runtime_error("checkpoint: read failed (truncated file)"); c += r; n -= (size_t)r; off += (uint64_t)r; }
}
// rows of `row` bytes held locally in order i = 0 ... n-1 <-> file rows gid[i]; consecutive global numbers move in one call.  skip[i] != 0: row left out
template <bool WRITE>
void move_rows(int fd, uint64_t off, size_t row, const std::vector<int64_t>& gid, const uint8_t* skip, char* local) {
   const size_t n = gid.size();
   for (size_t i = 0; i < n;) {
      if (skip && skip[i]) { i++; continue; }
      size_t j = i + 1;
      while (j < n && gid[j] == gid[j - 1] + 1 && !(skip && skip[j])) j++;
      if (WRITE) pwrite_all(fd, local + row * i, row * (j - i), off + row * (uint64_t)gid[i]);
      else pread_all(fd, local + row * i, row * (j - i), off + row * (uint64_t)gid[i]);
      i = j;
   }
}

struct HostSec { std::string name; std::vector<unsigned char> bytes; };
HostSec host_sec(const std::string& name, const void* p, size_t nbytes) {
   HostSec h; h.name = name; h.bytes.assign((nbytes + 7) / 8 * 8, 0);
   if (nbytes) std::memcpy(h.bytes.data(), p, nbytes);
   return h;
}
HostSec host_sec(const std::string& name, const std::vector<double>& v) { return host_sec(name, v.data(), sizeof(double) * v.size()); }

void rewrite_rows(const std::string& path, const std::vector<double>& rows, int width) {
   { std::ofstream f(path, std::ios_base::trunc); }
   for (size_t r = 0; r + width <= rows.size(); r += width) append_row(path, rows.data() + r, width);
}

}  // namespace

std::string SystemDriver::checkpoint_path(int step) const {
   char tag[32]; std::snprintf(tag, sizeof(tag), "_%06d.ckpt", step);
   return out_dir + "/" + opt_.ckpt_floc + tag;
}

// rank 0: of the files <floc>_<step>.ckpt up to this step, the newest Checkpoint.keep stay
void SystemDriver::PruneCheckpoints(int step) {
   if (comm.rank != 0) return;
   std::vector<int> steps;
   const std::string pre = opt_.ckpt_floc + "_";
   if (DIR* d = ::opendir(out_dir.c_str())) {
      while (struct dirent* e = ::readdir(d)) {
         const std::string nm = e->d_name;
         if (nm.size() < pre.size() + 11 || nm.size() > pre.size() + 15 || nm.compare(0, pre.size(), pre) != 0 || nm.compare(nm.size() - 5, 5, ".ckpt") != 0) continue;
         const std::string num = nm.substr(pre.size(), nm.size() - pre.size() - 5);   // %06d: six digits, more beyond step 999999
         if (num.find_first_not_of("0123456789") != std::string::npos) continue;
         const int st = std::atoi(num.c_str());
         if (st <= step) steps.push_back(st);
      }
      ::closedir(d);
   }
   std::sort(steps.begin(), steps.end());
   for (int i = 0; i + opt_.ckpt_keep < (int)steps.size(); i++) (void)::unlink(checkpoint_path(steps[i]).c_str());
}

namespace {
// lowest rank holding a node owns it: skip[g] = 1 for the nodes a lower rank shares
std::vector<uint8_t> nodes_of_lower_ranks(const Partition& part, int rank) {
   if (part.periodic) return part.held_by_lower;   // (the periodic neighbour lists name images too: other nodes, which a lower rank does not write)
   std::vector<uint8_t> skip((size_t)part.NN, 0);
   for (const Neighbor& nb : part.nbrs) if (nb.rank < rank) for (int32_t d : nb.dofs) skip[(size_t)(d % part.NN)] = 1;
   return skip;
}
// mesh and grain-map hashes: sums of per-element hashes over all ranks (independent of element order and decomposition)
void mesh_hashes(const Partition& part, const std::vector<int32_t>& attr, Comm& comm, hipStream_t s, uint64_t& grain, uint64_t& conn) {
   std::vector<uint64_t> h(2, 0);
   for (int e = 0; e < part.E; e++) {
      const uint64_t g = mix64((uint64_t)part.elem_gid[e]);
      h[0] += mix64(g ^ (uint64_t)(uint32_t)attr[e]);
      uint64_t c = g;
      for (int a = 0; a < part.n; a++) c = mix64(c ^ (uint64_t)part.node_gid[(size_t)part.conn[a + (size_t)part.n * e]]);
      h[1] += c;
   }
   allreduce_u64(comm, h, s);
   grain = h[0]; conn = h[1];
}
}  // namespace

void SystemDriver::SaveCheckpoint(const std::string& path) {
   NonlinearMechOperator& op = *oper_;
   hipStream_t s = op.stream();
   exa_ctx* ctx = op.GetModel()->ctx();
   StepAnalyses& an = *analyses_; const StepAnalyses::Checkpointed& ac = an.ckpt;
   EXA_HC(hipStreamSynchronize(s));
   const int Q = exa_qpts_per_elem(ctx), nsv = exa_num_state_vars(ctx);
   Header h;
   h.E_global = part.E_glob; h.NN_global = part.NN_glob; h.Q = Q; h.geom = part.geom; h.order = part.p; h.model = op.cfg_used.model;
   h.nprops = (int)op.props.size(); h.nstatev = nsv; h.props_hash = fnv1a(op.props.data(), sizeof(double) * op.props.size());
   mesh_hashes(part, elem_attr, comm, s, h.grain_hash, h.conn_hash);
   h.steps_done = steps_done; h.time = time; h.dt_class = dt_class; h.last_dt = last_dt_; h.bc_index = bc_index_; h.nranks = comm.nranks;
   h.flags = (ac.cycle0_saved ? 1u : 0u) | (ac.texture0_written ? 2u : 0u);
   h.model_calls = op.model_calls; op.GetCapState(h.newton_cap, h.newton_cap2);
   // ---- host sections (the same on every rank; rank 0 writes them)
   std::vector<HostSec> hs;
   hs.push_back(host_sec("avg_stress", avg_stress));
   if (opt_.additional_avgs) { hs.push_back(host_sec("avg_def_grad", avg_def_grad)); hs.push_back(host_sec("avg_pl_work", avg_pl_work)); hs.push_back(host_sec("avg_dp_tensor", avg_dp_tensor)); }
   { std::vector<int32_t> st; for (const SolverStats& x : stats) { st.push_back(x.newton_iters); st.push_back(x.krylov_iters); st.push_back(x.model_calls); st.push_back(x.converged ? 1 : 0); }
     hs.push_back(host_sec("solver_stats", st.data(), sizeof(int32_t) * st.size())); }
   { std::vector<double> cyc; auto it = ac.pvd_cycles.find(an.vis_dir(state())); if (it != ac.pvd_cycles.end()) for (auto& c : it->second) { cyc.push_back((double)c.first); cyc.push_back(c.second); }
     hs.push_back(host_sec("pvd_cycles", cyc)); }
   hs.push_back(host_sec("lattice_strains", ac.lattice_rows)); hs.push_back(host_sec("lattice_volumes", ac.volume_rows)); hs.push_back(host_sec("auto_dt", auto_dt_rows_));
   if (opt_.macro_tangent) hs.push_back(host_sec("macro_tangent", macro_tangent_rows));   // (only with the option on: every other checkpoint stays byte for byte what it was)
   // slip activity (only with the feature on, like the tangent's rows): window start step and pending reset, the rows of the fatigue file
   const bool slip = an.slip_activity_on();
   const DevBuf<double>* slip_acc = slip ? &an.SlipAccumulators(state()) : nullptr;   // (started here if the run has not begun)
   if (slip) {
      const int64_t w[2] = { ac.fatigue_window_start, ac.fatigue_pending ? 1 : 0 };
      hs.push_back(host_sec("fatigue_window", w, sizeof(w))); hs.push_back(host_sec("fatigue_rows", ac.fatigue_rows));
   }
   // ---- layout
   std::vector<Section> sec;
   for (const HostSec& x : hs) { Section t; t.name = x.name; t.nbytes = x.bytes.size(); t.checksum = sum64(x.bytes.data(), x.bytes.size()); sec.push_back(t); }
   // ... and its accumulators (60, global element), ahead of the field sections every file has
   const size_t slip_sec = sec.size();
   if (slip) { Section t; t.name = "slip_activity"; t.nbytes = 8ull * EXA_NSLIPACC * (uint64_t)part.E_glob; sec.push_back(t); }
   const size_t first_field = sec.size();
   { Section t; t.name = "x_beg"; t.nbytes = 24 * (uint64_t)part.NN_glob; sec.push_back(t); t.name = "v_sol"; sec.push_back(t);
     t.name = "stress0"; t.nbytes = 8ull * 6 * Q * (uint64_t)part.E_glob; sec.push_back(t); t.name = "matVars0"; t.nbytes = 8ull * nsv * Q * (uint64_t)part.E_glob; sec.push_back(t);
     // copies of shared nodes that differ from their owner's value (sizes known once the ranks have compared; the last two sections of the file)
     t.nbytes = 0; t.name = "x_beg_copies"; sec.push_back(t); t.name = "v_sol_copies"; sec.push_back(t); }
   h.nsections = (int)sec.size();
   uint64_t off = HEADER_BYTES + ENTRY_BYTES * sec.size();
   for (Section& t : sec) { off = (off + 63) / 64 * 64; t.offset = off; off += t.nbytes; }
   const uint64_t total = off;
   // ---- the file: rank 0 creates <path>.tmp at its final size, then every rank opens it
   const std::string tmp = path + ".tmp";
   int fd = -1;
   if (comm.rank == 0) { fd = ::open(tmp.c_str(), O_CREAT | O_TRUNC | O_RDWR, 0644); if (fd >= 0 && ::ftruncate(fd, (off_t)total) != 0) { ::close(fd); fd = -1; } }
   // whatever way this function is left: no descriptor stays open, and a .tmp that did not become the checkpoint is removed
   struct Cleanup { int& fd; const std::string& tmp; bool rank0; bool renamed = false;
                    ~Cleanup() { if (fd >= 0) ::close(fd); if (rank0 && !renamed) (void)::unlink(tmp.c_str()); } } cleanup{ fd, tmp, comm.rank == 0 };
   all_ok(comm, comm.rank != 0 || fd >= 0, "checkpoint: cannot create " + tmp);
   if (comm.rank != 0) fd = ::open(tmp.c_str(), O_RDWR);
   all_ok(comm, fd >= 0, "checkpoint: cannot open " + tmp);
   std::vector<uint64_t> sums(7, 0);
   bool ok = true; std::string why;
   const std::vector<uint8_t> skip = nodes_of_lower_ranks(part, comm.rank);
   std::vector<double> rows[2];
   try {
      // nodes: byNODES (NN, 3) on the device -> rows (x, y, z) of the owned nodes by global node number
      const DevBuf<double>* nb[2] = { &op.x_beg, &v_sol };
      for (int f = 0; f < 2; f++) {
         std::vector<double> hv((size_t)3 * part.NN); rows[f].resize((size_t)3 * part.NN);
         nb[f]->download(hv.data(), hv.size(), s);
         for (int g = 0; g < part.NN; g++) for (int c = 0; c < 3; c++) rows[f][3 * (size_t)g + c] = hv[g + (size_t)part.NN * c];
         for (int g = 0; g < part.NN; g++) if (!skip[g]) sums[f] += sum64(&rows[f][3 * (size_t)g], 24);
         move_rows<true>(fd, sec[first_field + f].offset, 24, part.node_gid, skip.data(), (char*)rows[f].data());
      }
   } catch (const std::exception& e) { ok = false; why = e.what(); }
   all_ok(comm, ok, why.empty() ? "checkpoint: write failed" : why);   // (the barrier after which every owner's rows are in the file)
   // A rank's copy of a shared node may differ from its owner's in the last bits (the ordered halo sums of three or more sharers add in a different
   // order on every rank).  Same rank count, same bits after a restart: every rank reads its owners' rows back from the file and records the copies
   // that differ as { rank + 2^32 rank count, global node, x, y, z }.  A state loaded from another rank count has none of its own.
   std::vector<unsigned char> copies[2];
   std::vector<uint64_t> cnt((size_t)2 * comm.nranks, 0);
   try {
      if (comm.nranks > 1) {
         std::vector<uint8_t> owned((size_t)part.NN); for (int g = 0; g < part.NN; g++) owned[g] = skip[g] ? 0 : 1;
         for (int f = 0; f < 2; f++) {
            std::vector<double> theirs((size_t)3 * part.NN, 0.0);
            move_rows<false>(fd, sec[first_field + f].offset, 24, part.node_gid, owned.data(), (char*)theirs.data());
            for (int g = 0; g < part.NN; g++) if (skip[g] && std::memcmp(&theirs[3 * (size_t)g], &rows[f][3 * (size_t)g], 24) != 0) {
               unsigned char e[40]; const int64_t r = (int64_t)comm.rank + ((int64_t)comm.nranks << 32), gid = part.node_gid[g];
               std::memcpy(e, &r, 8); std::memcpy(e + 8, &gid, 8); std::memcpy(e + 16, &rows[f][3 * (size_t)g], 24);
               copies[f].insert(copies[f].end(), e, e + 40);
            }
         }
      }
      // entries of another decomposition that came with the file this state was loaded from, as long as the state is still that one
      if (comm.rank == 0 && ckpt_foreign_calls_ == (long)op.model_calls)
         for (int f = 0; f < 2; f++) copies[f].insert(copies[f].end(), ckpt_foreign_copies_[f].begin(), ckpt_foreign_copies_[f].end());
      for (int f = 0; f < 2; f++) cnt[(size_t)2 * comm.rank + f] = copies[f].size() / 40;
   } catch (const std::exception& e) { ok = false; why = e.what(); }
   all_ok(comm, ok, why.empty() ? "checkpoint: write failed" : why);
   allreduce_u64(comm, cnt, s);
   {  uint64_t o = sec[first_field + 3].offset + sec[first_field + 3].nbytes;
      for (int f = 0; f < 2; f++) {
         Section& t = sec[first_field + 4 + f];
         uint64_t n = 0, before = 0; for (int r = 0; r < comm.nranks; r++) { if (r < comm.rank) before += cnt[(size_t)2 * r + f]; n += cnt[(size_t)2 * r + f]; }
         o = (o + 63) / 64 * 64; t.offset = o; t.nbytes = 40 * n; o += t.nbytes;
         cnt[(size_t)2 * comm.rank + f] = before;   // (own slot reused: entries of the lower ranks)
      } }
   try {
      for (int f = 0; f < 2; f++) if (!copies[f].empty()) {
         pwrite_all(fd, copies[f].data(), copies[f].size(), sec[first_field + 4 + f].offset + 40 * cnt[(size_t)2 * comm.rank + f]);
         sums[4 + f] = sum64(copies[f].data(), copies[f].size());
      }
      // quadrature functions: one pack launch each (layout -> canonical rows in local element order + checksum), one copy to the host
      DevBuf<uint64_t> cks(1);
      op.EnsureSlipRates(op.matVars0);   // the file holds the full state, slip rates included
      const DevBuf<double>* qb[2] = { &op.stress0, &op.matVars0 }; const int W[2] = { 6, nsv };
      for (int f = 0; f < 2; f++) {
         const size_t n = (size_t)W[f] * Q * part.E;
         DevBuf<double> can(n);
         ck(ctx, exa_qf_pack(ctx, W[f], qb[f]->p, can.p, cks.p, s), "exa_qf_pack");
         std::vector<double> hv(n); can.download(hv.data(), n, s); cks.download(&sums[2 + f], 1, s);
         move_rows<true>(fd, sec[first_field + 2 + f].offset, sizeof(double) * W[f] * Q, part.elem_gid, nullptr, (char*)hv.data());
      }
      if (slip && part.E > 0) {   // planar [60][E_pad] on the device -> rows of 60 by global element (480 B per element: transposed on the host)
         const std::vector<double> pl = slip_acc->to_host(s);
         const size_t Ep = pl.size() / EXA_NSLIPACC, El = (size_t)part.E;
         std::vector<double> hv(EXA_NSLIPACC * El);
         for (int k = 0; k < EXA_NSLIPACC; k++) for (size_t e = 0; e < El; e++) hv[EXA_NSLIPACC * e + k] = pl[k * Ep + e];
         sums[6] = sum64(hv.data(), sizeof(double) * hv.size());
         move_rows<true>(fd, sec[slip_sec].offset, sizeof(double) * EXA_NSLIPACC, part.elem_gid, nullptr, (char*)hv.data());
      }
      if (comm.rank != 0) { const bool synced = ::fsync(fd) == 0; const bool closed = ::close(fd) == 0; fd = -1; if (!synced || !closed) throw std::runtime_error("checkpoint: cannot flush " + tmp); }
   } catch (const std::exception& e) { ok = false; why = e.what(); }
   all_ok(comm, ok, why.empty() ? "checkpoint: write failed" : why);
   allreduce_u64(comm, sums, s);   // (also the barrier after which every rank's rows are in the file)
   for (int f = 0; f < 6; f++) sec[first_field + f].checksum = sums[f];
   if (slip) sec[slip_sec].checksum = sums[6];
   ok = true; why.clear();
   if (comm.rank == 0) {
      try {
         // the file reaches the end of its last section even where that section is empty (their sizes were not known when the file was created)
         uint64_t end = total; for (const Section& t : sec) end = std::max(end, t.offset + t.nbytes);
         if (::ftruncate(fd, (off_t)end) != 0) throw std::runtime_error("checkpoint: cannot size " + tmp);
         for (size_t i = 0; i < hs.size(); i++) if (!hs[i].bytes.empty()) pwrite_all(fd, hs[i].bytes.data(), hs[i].bytes.size(), sec[i].offset);
         std::vector<unsigned char> t(ENTRY_BYTES * sec.size(), 0);
         for (size_t i = 0; i < sec.size(); i++) {
            unsigned char* e = t.data() + ENTRY_BYTES * i;
            std::memcpy(e, sec[i].name.c_str(), std::min(sec[i].name.size(), NAME_BYTES - 1)); put(e, 24, sec[i].offset); put(e, 32, sec[i].nbytes); put(e, 40, sec[i].checksum);
         }
         pwrite_all(fd, t.data(), t.size(), HEADER_BYTES);
         unsigned char hb[HEADER_BYTES]; encode_header(h, hb);
         pwrite_all(fd, hb, HEADER_BYTES, 0);
         const bool synced = ::fsync(fd) == 0; const bool closed = ::close(fd) == 0; fd = -1;
         if (!synced || !closed) throw std::runtime_error("checkpoint: cannot flush " + tmp);
         if (::rename(tmp.c_str(), path.c_str()) != 0) throw std::runtime_error("checkpoint: cannot rename " + tmp + " to " + path);
         cleanup.renamed = true;
      } catch (const std::exception& e) { ok = false; why = e.what(); }
   }
   all_ok(comm, ok, why.empty() ? "checkpoint: write failed" : why);
}

void SystemDriver::LoadCheckpoint(const std::string& path) {
   NonlinearMechOperator& op = *oper_;
   hipStream_t s = op.stream();
   exa_ctx* ctx = op.GetModel()->ctx();
   if (steps_done != 0 || !stats.empty() || op.model_calls != 0 || restarted_)
      throw std::runtime_error("checkpoint: a checkpoint can only be loaded into a freshly created driver before its first step (this driver has " +
                               std::string(restarted_ ? "already loaded one" : "taken " + std::to_string(std::max<size_t>(stats.size(), 1)) + " step(s)") + ")");
   // Every rank reads header and table and opens the file before the first collective call: a rank that cannot see the file fails all of them
   // together.  What follows up to the field sections depends on the file and on global quantities only, so every rank takes the same decision.
   Header h; std::vector<Section> sec;
   int fd = -1;
   struct Closer { int& fd; ~Closer() { if (fd >= 0) ::close(fd); } } closer{ fd };
   {  bool ok0 = true; std::string why0;
      try { read_info(path, h, sec); fd = ::open(path.c_str(), O_RDONLY); if (fd < 0) throw std::runtime_error("checkpoint: cannot open " + path); }
      catch (const std::exception& e) { ok0 = false; why0 = e.what(); }
      all_ok(comm, ok0, why0.empty() ? "checkpoint: cannot read " + path : why0); }
   const int Q = exa_qpts_per_elem(ctx), nsv = exa_num_state_vars(ctx);
   auto mismatch = [&](const std::string& what, const std::string& file, const std::string& mine) {
      throw std::runtime_error("checkpoint: " + what + " mismatch: the file has " + file + ", this run has " + mine + " (" + path + ")");
   };
   auto hex = [](uint64_t v) { char b[24]; std::snprintf(b, sizeof(b), "%016llx", (unsigned long long)v); return std::string(b); };
   if (h.geom != part.geom) mismatch("geometry", h.geom == 1 ? "tetrahedra" : "hexahedra", part.geom == 1 ? "tetrahedra" : "hexahedra");
   if (h.order != part.p) mismatch("order", "p = " + std::to_string(h.order), "p = " + std::to_string(part.p));
   if (h.E_global != part.E_glob) mismatch("global element count", std::to_string(h.E_global), std::to_string(part.E_glob));
   if (h.NN_global != part.NN_glob) mismatch("global node count", std::to_string(h.NN_global), std::to_string(part.NN_glob));
   if (h.Q != Q) mismatch("points per element", std::to_string(h.Q), std::to_string(Q));
   if (h.model != op.cfg_used.model) mismatch("model id", std::to_string(h.model), std::to_string(op.cfg_used.model));
   if (h.nprops != (int)op.props.size() || h.nstatev != nsv) mismatch("number of properties / state variables", std::to_string(h.nprops) + " / " + std::to_string(h.nstatev), std::to_string(op.props.size()) + " / " + std::to_string(nsv));
   const uint64_t ph = fnv1a(op.props.data(), sizeof(double) * op.props.size());
   if (h.props_hash != ph) mismatch("property hash", hex(h.props_hash), hex(ph));
   uint64_t gh, chh; mesh_hashes(part, elem_attr, comm, s, gh, chh);
   if (h.grain_hash != gh) mismatch("grain-map hash", hex(h.grain_hash), hex(gh));
   if (h.conn_hash != chh) mismatch("connectivity hash", hex(h.conn_hash), hex(chh));
   if (h.bc_index >= (int)opt_.bcs.size()) mismatch("essential-boundary entry", "entry " + std::to_string(h.bc_index) + " in force", std::to_string(opt_.bcs.size()) + " entries");
   auto need = [&](const std::string& name, uint64_t nbytes, bool exact) -> const Section& {
      const Section* t = find(sec, name);
      if (!t) throw std::runtime_error("checkpoint: section '" + name + "' is missing (" + path + ")");
      if (exact && t->nbytes != nbytes) throw std::runtime_error("checkpoint: section '" + name + "' holds " + std::to_string(t->nbytes) + " bytes, expected " + std::to_string(nbytes));
      return *t;
   };
   // ---- host sections (every rank reads them; identical decisions on every rank)
   auto host_doubles = [&](const std::string& name, int width, std::vector<double>& out) {
      const Section& t = need(name, 0, false);
      std::vector<double> v(t.nbytes / 8);
      if (t.nbytes) pread_all(fd, v.data(), t.nbytes, t.offset);
      if (sum64(v.data(), t.nbytes) != t.checksum) throw std::runtime_error("checkpoint: checksum mismatch in section '" + name + "' (" + path + ")");
      if (v.size() % width != 0) throw std::runtime_error("checkpoint: section '" + name + "' does not hold whole rows of " + std::to_string(width));
      out.swap(v);
   };
   std::vector<double> r_stress, r_F, r_pw, r_dp, r_cyc, r_ls, r_lv, r_dt;
   host_doubles("avg_stress", 6, r_stress);
   if (opt_.additional_avgs) { host_doubles("avg_def_grad", 9, r_F); host_doubles("avg_pl_work", 1, r_pw); host_doubles("avg_dp_tensor", 6, r_dp); }
   host_doubles("pvd_cycles", 2, r_cyc); host_doubles("auto_dt", 1, r_dt);
   const int H = std::max(1, (int)opt_.lightup_hkl.size() / 3);
   host_doubles("lattice_strains", H, r_ls); host_doubles("lattice_volumes", H, r_lv);
   std::vector<double> r_mt;   // rows of the macroscopic tangent: only files written with Visualizations.macro_tangent on carry them
   if (opt_.macro_tangent && find(sec, "macro_tangent")) host_doubles("macro_tangent", MACRO_TANGENT_ROW, r_mt);
   // slip activity: a run with the feature on continues the accumulators of the file; with it off the sections are ignored
   std::vector<double> r_fat; int64_t fat_window[2] = { 0, 0 }; const Section* fat_sec = nullptr;
   if (analyses_->slip_activity_on()) {
      if (!find(sec, "slip_activity")) throw std::runtime_error("checkpoint: section 'slip_activity' is missing: the file was written without Visualizations.fatigue / enable_slip_activity and cannot continue the accumulators of this run (" + path + ")");
      fat_sec = &need("slip_activity", 8ull * EXA_NSLIPACC * (uint64_t)part.E_glob, true);
      const Section& w = need("fatigue_window", 16, true);
      pread_all(fd, fat_window, 16, w.offset);
      if (sum64(fat_window, 16) != w.checksum) throw std::runtime_error("checkpoint: checksum mismatch in section 'fatigue_window' (" + path + ")");
      host_doubles("fatigue_rows", FATIGUE_ROW, r_fat);
   }
   std::vector<int32_t> r_stats;
   { const Section& t = need("solver_stats", 0, false);
     std::vector<unsigned char> b(t.nbytes); if (t.nbytes) pread_all(fd, b.data(), t.nbytes, t.offset);
     if (sum64(b.data(), b.size()) != t.checksum) throw std::runtime_error("checkpoint: checksum mismatch in section 'solver_stats' (" + path + ")");
     if (t.nbytes < 16ull * (uint64_t)h.steps_done) throw std::runtime_error("checkpoint: section 'solver_stats' holds fewer rows than steps_done");
     r_stats.resize((size_t)4 * h.steps_done); if (!r_stats.empty()) std::memcpy(r_stats.data(), b.data(), sizeof(int32_t) * r_stats.size()); }
   if ((int64_t)r_stress.size() != 6 * h.steps_done) throw std::runtime_error("checkpoint: section 'avg_stress' does not hold one row per completed step");
   // ---- field sections
   const Section* fs[4] = { &need("x_beg", 24 * (uint64_t)part.NN_glob, true), &need("v_sol", 24 * (uint64_t)part.NN_glob, true),
                            &need("stress0", 8ull * 6 * Q * (uint64_t)part.E_glob, true), &need("matVars0", 8ull * nsv * Q * (uint64_t)part.E_glob, true) };
   // copies of shared nodes that differed from their owner's value when the file was written: they belong to the writer's decomposition and
   // are put back when this run has the same rank count (and holds the node); any other reader starts from the owners' values alone
   std::vector<unsigned char> copies[2];
   for (int f = 0; f < 2; f++) if (const Section* t = find(sec, f == 0 ? "x_beg_copies" : "v_sol_copies")) {
      if (t->nbytes % 40 != 0) throw std::runtime_error("checkpoint: section '" + t->name + "' does not hold whole entries of 40 bytes");
      copies[f].resize(t->nbytes); if (t->nbytes) pread_all(fd, copies[f].data(), t->nbytes, t->offset);
      if (sum64(copies[f].data(), copies[f].size()) != t->checksum) throw std::runtime_error("checkpoint: checksum mismatch in section '" + t->name + "' (" + path + ")");
      // entries of another rank count are not for this run: kept aside (SaveCheckpoint)
      std::vector<unsigned char> mine; ckpt_foreign_copies_[f].clear();
      for (size_t i = 0; i + 40 <= copies[f].size(); i += 40) {
         int64_t r; std::memcpy(&r, &copies[f][i], 8);
         std::vector<unsigned char>& to = (r >> 32) == comm.nranks ? mine : ckpt_foreign_copies_[f];
         to.insert(to.end(), copies[f].begin() + i, copies[f].begin() + i + 40);
      }
      copies[f].swap(mine);
   }
   // Nothing of the driver is touched before every checksum has been verified: the node fields wait on the host, the quadrature functions are
   // unpacked into copies of the driver's buffers (copies, so that the padding lanes of the last element block keep what they held), which
   // replace the originals afterwards.  A load that fails leaves the driver as it was created.
   std::vector<uint64_t> sums(5, 0);
   bool ok = true; std::string why;
   std::vector<double> nodes[2];
   DevBuf<double> scratch[2];
   std::vector<double> fat_planar;
   try {
      const std::vector<uint8_t> skip = nodes_of_lower_ranks(part, comm.rank);
      std::unordered_map<int64_t, int> local_of;
      if (!copies[0].empty() || !copies[1].empty()) for (int g = 0; g < part.NN; g++) local_of.emplace(part.node_gid[g], g);
      for (int f = 0; f < 2; f++) {
         std::vector<double> rows((size_t)3 * part.NN); nodes[f].resize((size_t)3 * part.NN);
         move_rows<false>(fd, fs[f]->offset, 24, part.node_gid, nullptr, (char*)rows.data());
         for (int g = 0; g < part.NN; g++) if (!skip[g]) sums[f] += sum64(&rows[3 * (size_t)g], 24);
         for (size_t i = 0; i + 40 <= copies[f].size(); i += 40) {
            int64_t r, gid; std::memcpy(&r, &copies[f][i], 8); std::memcpy(&gid, &copies[f][i + 8], 8);
            if ((r & 0xffffffff) != comm.rank) continue;
            auto it = local_of.find(gid);
            if (it != local_of.end() && skip[it->second]) std::memcpy(&rows[3 * (size_t)it->second], &copies[f][i + 16], 24);
         }
         for (int g = 0; g < part.NN; g++) for (int c = 0; c < 3; c++) nodes[f][g + (size_t)part.NN * c] = rows[3 * (size_t)g + c];
      }
      DevBuf<uint64_t> cks(1);
      const DevBuf<double>* qb[2] = { &op.stress0, &op.matVars0 }; const int W[2] = { 6, nsv };
      for (int f = 0; f < 2; f++) {
         const size_t n = (size_t)W[f] * Q * part.E;
         std::vector<double> hv(n);
         move_rows<false>(fd, fs[2 + f]->offset, sizeof(double) * W[f] * Q, part.elem_gid, nullptr, (char*)hv.data());
         DevBuf<double> can(n); can.upload(hv.data(), n, s);
         scratch[f].alloc(qb[f]->n); scratch[f].copy_from(*qb[f], s);
         ck(ctx, exa_qf_unpack(ctx, W[f], can.p, scratch[f].p, cks.p, s), "exa_qf_unpack");
         cks.download(&sums[2 + f], 1, s);
      }
      if (fat_sec) {
         int64_t n = 0; exa_slip_activity_sizes(part.E, &n);
         const size_t El = (size_t)part.E, Ep = (size_t)n / EXA_NSLIPACC;
         std::vector<double> hv(EXA_NSLIPACC * El);
         move_rows<false>(fd, fat_sec->offset, sizeof(double) * EXA_NSLIPACC, part.elem_gid, nullptr, (char*)hv.data());
         sums[4] = sum64(hv.data(), sizeof(double) * hv.size());
         fat_planar.assign((size_t)std::max<int64_t>(n, 1), 0.0);
         for (int k = 0; k < EXA_NSLIPACC; k++) for (size_t e = 0; e < El; e++) fat_planar[k * Ep + e] = hv[EXA_NSLIPACC * e + k];
      }
   } catch (const std::exception& e) { ok = false; why = e.what(); }
   all_ok(comm, ok, why.empty() ? "checkpoint: read failed" : why);
   allreduce_u64(comm, sums, s);
   if (fat_sec && sums[4] != fat_sec->checksum) throw std::runtime_error("checkpoint: checksum mismatch in section 'slip_activity' (" + path + ")");
   for (int f = 0; f < 4; f++) if (sums[f] != fs[f]->checksum) throw std::runtime_error("checkpoint: checksum mismatch in section '" + fs[f]->name + "' (" + path + ")");
   // ---- verified: from here on the driver takes the state over
   op.x_beg.upload(nodes[0].data(), nodes[0].size(), s); op.x_cur.upload(nodes[0].data(), nodes[0].size(), s); v_sol.upload(nodes[1].data(), nodes[1].size(), s);
   op.stress0.swap(scratch[0]); op.matVars0.swap(scratch[1]); op.ForgetPendingRates();   // (a full state from the file; the old arrays are freed)
   // a state written by another code is brought into the form the constitutive kernels expect (slot 0 = sum of |slip rates|); this library's own
   // files satisfy it as stored and come back bit for bit
   if (h.writer != WRITER_THIS_LIBRARY) ck(ctx, exa_state_normalize(ctx, op.matVars0.p, s), "exa_state_normalize");
   EXA_HC(hipStreamSynchronize(s));
   // ---- host state
   time = h.time; dt_class = h.dt_class; last_dt_ = h.last_dt; steps_done = (int)h.steps_done;
   StepAnalyses::Checkpointed& ac = analyses_->ckpt;
   ac.cycle0_saved = (h.flags & 1u) != 0; ac.texture0_written = (h.flags & 2u) != 0;
   stats.resize((size_t)h.steps_done);
   for (size_t i = 0; i < stats.size(); i++) { stats[i].newton_iters = r_stats[4 * i]; stats[i].krylov_iters = r_stats[4 * i + 1]; stats[i].model_calls = r_stats[4 * i + 2]; stats[i].converged = r_stats[4 * i + 3] != 0; }
   avg_stress.swap(r_stress); avg_def_grad.swap(r_F); avg_pl_work.swap(r_pw); avg_dp_tensor.swap(r_dp);
   ac.lattice_rows.swap(r_ls); ac.volume_rows.swap(r_lv); auto_dt_rows_.swap(r_dt);
   macro_tangent_rows.swap(r_mt);
   if (fat_sec) { ac.fatigue_window_start = fat_window[0]; ac.fatigue_pending = fat_window[1] != 0; ac.fatigue_rows.swap(r_fat); }
   { const std::string vd = analyses_->vis_dir(state());
     auto& cyc = ac.pvd_cycles[vd]; cyc.clear(); for (size_t i = 0; i + 1 < r_cyc.size(); i += 2) cyc.emplace_back((int)r_cyc[i], r_cyc[i + 1]); if (cyc.empty()) ac.pvd_cycles.erase(vd); }
   analyses_->Restored(fat_sec ? &fat_planar : nullptr);   // (the element rows it holds are those of the state this one replaced)
   op.model_calls = (int)h.model_calls; op.SetCapState(h.newton_cap, h.newton_cap2);
   // the essential-boundary set in force, without the SolveInit that belongs to the step where it changed
   bc_index_ = h.bc_index;
   if (bc_index_ >= 0) UpdateEssBdr(opt_.bcs[(size_t)bc_index_]);
   op.SetDt(dt_class);
   // the append-mode files restart from the stored rows: a checkpoint older than the interruption would otherwise leave duplicate rows
   if (write_files && comm.rank == 0) {
      rewrite_rows(out_dir + "/" + opt_.avg_stress_fname, avg_stress, 6);
      if (opt_.additional_avgs) {
         rewrite_rows(out_dir + "/" + opt_.avg_pl_work_fname, avg_pl_work, 1); rewrite_rows(out_dir + "/" + opt_.avg_def_grad_fname, avg_def_grad, 9);
         rewrite_rows(out_dir + "/" + opt_.avg_dp_tensor_fname, avg_dp_tensor, 6);
      }
      if (opt_.lightup()) { rewrite_rows(out_dir + "/" + opt_.lightup_strain_fname, ac.lattice_rows, H); rewrite_rows(out_dir + "/" + opt_.lightup_volume_fname, ac.volume_rows, H); }
      if (opt_.macro_tangent) write_macro_tangent_rows(out_dir + "/" + opt_.macro_tangent_fname, macro_tangent_rows, false);
      if (opt_.fatigue) write_fatigue_rows(out_dir + "/" + opt_.fatigue_fname, ac.fatigue_rows, false);
      if (opt_.dt_auto) { std::ofstream f(out_dir + "/" + opt_.auto_dt_fname, std::ios_base::trunc); for (double v : auto_dt_rows_) f << std::setprecision(12) << v << std::endl; }
   }
   restarted_ = true; ckpt_foreign_calls_ = (long)op.model_calls;
}

}  // namespace exa_host
