// Slip-system activity and the Fatemi-Socie fatigue indicator parameter in the driver: the accumulators of csrc/fatigue_kernels.hip as
// persistent state of a run.  SystemDriver::CommitStep -> AccumulateSlip adds every committed step; SlipActivity evaluates (read-only), combines
// the summary over the ranks and forms the per-grain mean and maximum of FIP on the host from the downloaded rows.
#include "driver.hpp"
#include <algorithm>
#include <cmath>
#include <fstream>
#include <iomanip>
#include <limits>

namespace exa_host {

namespace {
void ck(exa_ctx* ctx, int rc, const char* what) { if (rc < 0) throw std::runtime_error(std::string(what) + ": " + exa_last_error(ctx)); }
}

void SystemDriver::EnableSlipActivity() {
   if (fatigue_on_) return;
   if (steps_done > 0 || !stats.empty() || restarted_) throw std::runtime_error("enable_slip_activity: the accumulators can only be switched on before the first step");
   if (exa_slip_plane_normals(oper_->cfg_used.model, fat_normals_) != 0) throw std::runtime_error("slip activity: no slip-plane normals for this model");
   fatigue_on_ = true;
}

// the accumulators of a fresh run: zero, and the window of the initial state (Gamma = 0, the normal stresses of its rows)
void SystemDriver::EnsureFatigueInit() {
   if (fatigue_init_) return;
   if (steps_done > 0) throw std::runtime_error("slip activity: the accumulators of this run were never started");
   hipStream_t s = oper_->stream();
   exa_ctx* ctx = oper_->GetModel()->ctx();
   int64_t n = 0; exa_slip_activity_sizes(part.E, &n);
   fat_acc_.alloc((size_t)std::max<int64_t>(n, 1)); fat_acc_.zero(s);
   fat_gid_.upload(part.elem_gid, s);
   ComputeElementFields();
   ck(ctx, exa_slip_accumulate(ctx, fields_dev_.p, fat_normals_, 0.0, 1, fat_acc_.p, s), "exa_slip_accumulate");
   fatigue_window_start_ = 0; fatigue_init_ = true;
}

// the committed step from the rows of the committed state, which stay in fields_dev_ for the step's other analyses.  Its size is step_dt_, what the
// step was solved with: under Time.Auto dt_class holds the next step's proposal by the time a step is committed
void SystemDriver::AccumulateSlip() {
   hipStream_t s = oper_->stream();
   exa_ctx* ctx = oper_->GetModel()->ctx();
   if (!fatigue_init_) {   // (a step solved with commit = false on a fresh driver whose Step did not start them: cannot happen; Step starts them)
      throw std::runtime_error("slip activity: the accumulators were not started before the first step");
   }
   ComputeElementFields();
   ck(ctx, exa_slip_accumulate(ctx, fields_dev_.p, fat_normals_, step_dt_, fatigue_pending_ ? 1 : 0, fat_acc_.p, s), "exa_slip_accumulate");
   if (fatigue_pending_) { fatigue_window_start_ = steps_done; fatigue_pending_ = false; }
}

void SystemDriver::ResetFatigueWindow() {
   if (!fatigue_on_) throw std::runtime_error("reset_fatigue_window: slip activity is not on (Visualizations.fatigue or enable_slip_activity)");
   if (steps_done == 0 && !restarted_) { EnsureFatigueInit(); return; }   // before step 1 the window is the initial state: nothing is pending
   fatigue_pending_ = true;
}

void SystemDriver::SlipActivity(double k_fs, double sigma_y, SlipActivityResult& res, bool fields_current, bool want_acc) {
   if (!fatigue_on_) throw std::runtime_error("slip activity is not on (Visualizations.fatigue or enable_slip_activity before the first step)");
   if (!(k_fs >= 0.0) || !std::isfinite(k_fs)) throw std::runtime_error("slip activity: k must be a finite number >= 0");
   if (!(sigma_y > 0.0) || !std::isfinite(sigma_y)) throw std::runtime_error("slip activity: sigma_y must be a finite number > 0");
   hipStream_t s = oper_->stream();
   exa_ctx* ctx = oper_->GetModel()->ctx();
   const bool fresh = !fatigue_init_;
   EnsureFatigueInit();
   if (!fields_current && !fresh) ComputeElementFields();
   const size_t E = (size_t)part.E;
   if (fat_rows_.n != std::max<size_t>(EXA_NFIP * E, 1)) fat_rows_.alloc(std::max<size_t>(EXA_NFIP * E, 1));
   if (fat_sum_.n < 8) fat_sum_.alloc(8);
   ck(ctx, exa_fip_rows(ctx, fat_acc_.p, k_fs, sigma_y, fat_rows_.p, s), "exa_fip_rows");
   ck(ctx, exa_fip_summary(ctx, fields_dev_.p, fat_rows_.p, fat_gid_.p, fat_sum_.p, s), "exa_fip_summary");
   // elements are not shared across ranks: three sums, three maxima; the element of the largest FIP is the smallest id among the ranks that attain it
   comm.allreduce_sum(fat_sum_.p, 3, s);
   double loc[7]; fat_sum_.download(loc, 7, s);
   comm.allreduce_max(fat_sum_.p + 3, 3, s);
   double t[7]; fat_sum_.download(t, 7, s);
   if (comm.nranks > 1) {
      const double cand = (part.E > 0 && loc[3] == t[3]) ? -loc[6] : -std::numeric_limits<double>::infinity();
      EXA_HC(hipMemcpyAsync(fat_sum_.p + 7, &cand, sizeof(double), hipMemcpyHostToDevice, s));
      comm.allreduce_max(fat_sum_.p + 7, 1, s);
      double m; EXA_HC(hipMemcpyAsync(&m, fat_sum_.p + 7, sizeof(double), hipMemcpyDeviceToHost, s)); EXA_HC(hipStreamSynchronize(s));
      t[6] = -m;
   }
   const double iv = 1.0 / t[0];
   res.summary[0] = t[0]; res.summary[1] = t[1] * iv; res.summary[2] = t[3]; res.summary[3] = t[6];
   res.summary[4] = t[2] * iv; res.summary[5] = t[5]; res.summary[6] = t[4]; res.summary[7] = (double)fatigue_window_start_;
   res.fip.resize(EXA_NFIP * E);
   if (E) fat_rows_.download(res.fip.data(), res.fip.size(), s);
   res.acc.clear();
   if (want_acc && E) {   // planar [EXA_NSLIPACC][E_pad] -> rows
      const size_t Ep = fat_acc_.n / EXA_NSLIPACC;
      const std::vector<double> pl = fat_acc_.to_host(s);
      res.acc.resize(EXA_NSLIPACC * E);
      for (int k = 0; k < EXA_NSLIPACC; k++) for (size_t e = 0; e < E; e++) res.acc[EXA_NSLIPACC * e + k] = pl[k * Ep + e];
   }
   // per grain: volume, sum V FIP and max FIP over the grain's elements, in ascending global element id on every rank
   int gmax = 0;
   for (int32_t a : elem_attr) gmax = std::max(gmax, (int)a);
   const int G = (int)comm.max_over_ranks((double)gmax);
   res.grain_ids.clear(); res.grain_vals.clear();
   if (G < 1) return;
   std::vector<double> V(E);
   if (E) {
      EXA_HC(hipMemcpy2DAsync(V.data(), sizeof(double), fields_dev_.p + EXA_F_VOLUME, sizeof(double) * EXA_NFIELDS, sizeof(double), E, hipMemcpyDeviceToHost, s));
      EXA_HC(hipStreamSynchronize(s));
   }
   std::vector<size_t> order(E);
   for (size_t e = 0; e < E; e++) order[e] = e;
   std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return part.elem_gid[a] < part.elem_gid[b]; });
   std::vector<double> g((size_t)3 * G, 0.0);
   std::fill(g.begin() + 2 * (size_t)G, g.end(), -std::numeric_limits<double>::infinity());
   for (size_t e : order) {
      const int a = elem_attr[e];
      if (a < 1) continue;
      const double f = res.fip[EXA_NFIP * e + EXA_FIP_FIP];
      g[a - 1] += V[e]; g[(size_t)G + a - 1] += V[e] * f; g[2 * (size_t)G + a - 1] = std::max(g[2 * (size_t)G + a - 1], f);
   }
   if (comm.nranks > 1) {
      if (fat_grain_.n < g.size()) fat_grain_.alloc(g.size());
      fat_grain_.upload(g.data(), g.size(), s);
      comm.allreduce_sum(fat_grain_.p, 2 * G, s);
      comm.allreduce_max(fat_grain_.p + 2 * (size_t)G, G, s);
      fat_grain_.download(g.data(), g.size(), s);
   }
   for (int a = 0; a < G; a++) {
      if (!(g[a] > 0.0)) continue;
      res.grain_ids.push_back(a + 1);
      res.grain_vals.push_back(g[a]); res.grain_vals.push_back(g[(size_t)G + a] / g[a]); res.grain_vals.push_back(g[2 * (size_t)G + a]);
   }
}

void SystemDriver::WriteFatigue(int step, const SlipActivityResult& r) {
   const double* m = r.summary;
   const double row[FATIGUE_ROW] = { (double)step, time, m[7], m[1], m[2], m[3], m[4], m[5], m[6] };
   fatigue_rows.insert(fatigue_rows.end(), row, row + FATIGUE_ROW);
   if (comm.rank != 0) return;
   const std::string path = out_dir + "/" + opt_.fatigue_fname;
   bool fresh = true;
   { std::ifstream g(path); fresh = !g || g.peek() == std::ifstream::traits_type::eof(); }
   if (fresh) write_fatigue_rows(path, std::vector<double>(), false);   // (the header)
   write_fatigue_rows(path, std::vector<double>(row, row + FATIGUE_ROW), true);
   if (!r.grain_ids.empty()) {
      char tag[32]; std::snprintf(tag, sizeof(tag), "fatigue_grains_%06d.txt", step);
      write_fatigue_grains(out_dir + "/" + tag, (int)r.grain_ids.size(), r.grain_ids.data(), r.grain_vals.data());
   }
}

// append = false: the file anew, header first (also rewrites the file of a restarted run: host/checkpoint.hip)
void write_fatigue_rows(const std::string& path, const std::vector<double>& rows, bool append) {
   std::ofstream f(path, append ? std::ios_base::app : std::ios_base::trunc);
   if (!f) throw std::runtime_error("fatigue: cannot write " + path);
   if (!append) f << "# step time window_start_step fip_mean fip_max fip_max_element accumulated_slip_mean accumulated_slip_max shear_range_max\n";
   f << std::setprecision(17);
   for (size_t i = 0; i + FATIGUE_ROW <= rows.size(); i += FATIGUE_ROW) {
      f << (long)rows[i] << ' ' << rows[i + 1] << ' ' << (long)rows[i + 2] << ' ' << rows[i + 3] << ' ' << rows[i + 4] << ' ' << (long long)rows[i + 5];
      for (int k = 6; k < FATIGUE_ROW; k++) f << ' ' << rows[i + k];
      f << '\n';
   }
   if (!f) throw std::runtime_error("fatigue: writing " + path + " failed");
}

void write_fatigue_grains(const std::string& path, int n, const int32_t* ids, const double* v) {
   std::ofstream f(path);
   if (!f) throw std::runtime_error("fatigue: cannot write " + path);
   f << "# grain_id volume fip_mean fip_max\n" << std::setprecision(17);
   for (int i = 0; i < n; i++) f << ids[i] << ' ' << v[3 * i] << ' ' << v[3 * i + 1] << ' ' << v[3 * i + 2] << '\n';
   if (!f) throw std::runtime_error("fatigue: writing " + path + " failed");
}

}  // namespace exa_host
