// StepAnalyses (host/analyses.hpp): the analyses of the element rows, their output schedule, and the writers of their text files.  No device code
// of its own: every launch goes through the C ABI.
#include "driver.hpp"
#include "vtu.hpp"
#include <algorithm>
#include <cmath>
#include <fstream>
#include <iomanip>
#include <limits>

namespace exa_host {

static void ck(exa_ctx* ctx, int rc, const char* what) { if (rc < 0) throw std::runtime_error(std::string(what) + ": " + exa_last_error(ctx)); }

StepAnalyses::StepAnalyses(NonlinearMechOperator& op, Comm& comm, const Partition& part, const ExaOptions& opt, const std::vector<int32_t>& elem_attr, std::vector<double> grain_qref)
   : op_(op), comm_(comm), part_(part), opt_(opt), elem_attr_(elem_attr), grain_qref_(std::move(grain_qref)) {
   if (opt_.fatigue) EnableSlipActivity();
}

long StepAnalyses::model_calls() const { return (long)op_.model_calls; }

// ---- the schedule ----------------------------------------------------------------------------------------------------------------------------------
void StepAnalyses::BeforeFirstStep(const StepState& at, bool commit) {
   started_ = true;
   // ParaView cycle 0: the initial state at t = 0, saved before the first step (reference src/mechanics_driver.cpp:640-700), outside the timed region
   // texture file of step 0 (the initial texture) at the same point; the two share the element rows
   const bool first = at.write_files && commit && at.step == 0;
   if (fatigue_on_) EnsureFatigueInit(at);
   if (first && opt_.paraview && !ckpt.cycle0_saved) { SaveFields(at, vis_dir(at), 0, 0.0); ckpt.cycle0_saved = true; }
   if (first && opt_.texture && !ckpt.texture0_written) { WriteTexture(at, 0); ckpt.texture0_written = true; }
}

// the committed step from the rows of the committed state, which the step's other analyses share.  Its size is at.dt, what the step was solved
// with: under Time.Auto the driver's dt_class holds the next step's proposal by the time a step is committed
void StepAnalyses::Committed(const StepState& at) {
   if (!fatigue_on_) return;
   hipStream_t s = op_.stream(); exa_ctx* ctx = op_.GetModel()->ctx();
   if (!fatigue_init_) throw std::runtime_error("slip activity: the accumulators were not started before the first step");   // (Step starts them)
   ComputeElementFields(at);
   ck(ctx, exa_slip_accumulate(ctx, fields_dev_.p, fat_normals_, at.dt, ckpt.fatigue_pending ? 1 : 0, fat_acc_.p, s), "exa_slip_accumulate");
   if (ckpt.fatigue_pending) { ckpt.fatigue_window_start = at.step; ckpt.fatigue_pending = false; }
}

bool StepAnalyses::AfterCommit(const StepState& at, int ti) {
   // ParaView cycle ti of the converged, swapped state every Visualizations.steps steps and at the last step (reference src/mechanics_driver.cpp:911-955)
   // per-grain averages and texture on the same cadence, whether or not ParaView output is on
   bool due = false, last_step = false;
   if ((opt_.paraview || opt_.grain_avgs || opt_.texture || opt_.macro_tangent || opt_.lattice_curvature || opt_.fatigue) && at.write_files) {
      bool last = ti >= opt_.nsteps;
      if (!opt_.dt_cust) { const double dtl = opt_.dt_auto ? at.dt : opt_.dt; last = last || std::fabs(at.time - opt_.t_final) <= std::fabs(1e-3 * dtl); }
      due = last || ti % opt_.vis_steps == 0; last_step = last;
   }
   const bool save = opt_.paraview && due, grains = opt_.grain_avgs && due, texture = opt_.texture && due;
   // light-up analysis: one row of lattice strains and one of fibre volume fractions per converged step, from the same element rows
   const bool lattice = opt_.lightup() && at.write_files;
   const bool curvature = opt_.lattice_curvature && due;
   // slip activity: a file row every fatigue_cycle_steps steps, followed by the request to restart the window, and at the last step (0: on the cadence above)
   const bool cycle_end = opt_.fatigue && at.write_files && opt_.fatigue_cycle_steps > 0 && ti % opt_.fatigue_cycle_steps == 0;
   const bool fatigue = opt_.fatigue && at.write_files && (opt_.fatigue_cycle_steps > 0 ? (cycle_end || last_step) : due);
   SlipActivityResult fat;
   if (fatigue || (save && opt_.fatigue)) SlipActivity(at, opt_.fatigue_k, opt_.fatigue_sigma_y, fat, save);
   if (fatigue) WriteFatigue(at, ti, fat);
   if (cycle_end && !last_step) ResetFatigueWindow(at);
   std::vector<double> curv_rows;
   if (curvature) { double m[7]; LatticeCurvature(at, opt_.lattice_curvature_burgers, curv_rows, m, save); WriteLatticeCurvature(at, ti, m); }
   if (save) SaveCycle(at, vis_dir(at), ti, at.time, curv_rows, fat);
   if (texture) WriteTexture(at, ti);
   if (grains) {
      std::vector<int32_t> ids; std::vector<double> vals;
      GrainAverages(at, ids, vals);
      if (comm_.rank == 0) {
         char tag[16]; std::snprintf(tag, sizeof(tag), "_%06d.txt", ti);
         write_grain_avgs(at.out_dir + "/" + opt_.grain_avgs_fname + tag, (int)ids.size(), ids.data(), vals.data());
      }
   }
   if (lattice) {
      const int H = (int)opt_.lightup_hkl.size() / 3;
      std::vector<double> strain(H), vf(H);
      LatticeStrains(at, opt_.lightup_hkl, opt_.lightup_s_dir, opt_.lightup_tol_deg, strain.data(), vf.data());
      ckpt.lattice_rows.insert(ckpt.lattice_rows.end(), strain.begin(), strain.end()); ckpt.volume_rows.insert(ckpt.volume_rows.end(), vf.begin(), vf.end());
      if (comm_.rank == 0) { append_row(at.out_dir + "/" + opt_.lightup_strain_fname, strain.data(), H); append_row(at.out_dir + "/" + opt_.lightup_volume_fname, vf.data(), H); }
   }
   return due;
}

void StepAnalyses::GrainsChanged(std::vector<double> grain_qref) {
   grain_qref_ = std::move(grain_qref); grain_plan_.clear(); grain_G_ = 0;
   Invalidate();
}

void StepAnalyses::Restored(const std::vector<double>* slip_planar) {
   restored_ = true; Invalidate();
   if (slip_planar) { fat_acc_.upload(*slip_planar, op_.stream()); fat_gid_.upload(part_.elem_gid, op_.stream()); fatigue_init_ = true; }
}

// ---- the analyses ----------------------------------------------------------------------------------------------------------------------------------
void StepAnalyses::ComputeElementFields(const StepState& at) {
   NonlinearMechOperator& op = op_;
   hipStream_t s = op.stream();
   exa_ctx* ctx = op.GetModel()->ctx();
   DevBuf<double> xe((size_t)3 * part_.n * part_.E), jac;
   if (fields_dev_.n != (size_t)EXA_NFIELDS * part_.E) fields_dev_.alloc((size_t)EXA_NFIELDS * part_.E);
   ck(ctx, exa_restrict(ctx, op.x_cur.p, xe.p, s), "exa_restrict");
   if (part_.p != 1 || part_.geom == 1) {   // p = 1 hexahedra: det J comes from the node coordinates inside the launch
      jac.alloc((size_t)exa_qf_size(ctx, 9));
      ck(ctx, exa_jacobians(ctx, xe.p, jac.p, s), "exa_jacobians");
   }
   op.EnsureSlipRates(op.matVars0);   // (the rows average slots 14..25)
   ck(ctx, exa_element_fields(ctx, jac.p, op.stress0.p, op.matVars0.p, xe.p, fields_dev_.p, s), "exa_element_fields");
   fields_step_ = at.step; fields_calls_ = model_calls(); field_launches++;
   EXA_HC(hipStreamSynchronize(s));   // xe and jac leave scope
}

void StepAnalyses::ElementFields(const StepState& at, std::vector<double>& out) {
   ComputeElementFields(at);
   out = fields_dev_.to_host(op_.stream());
}

void StepAnalyses::LatticeStrains(const StepState& at, const std::vector<int>& hkl, const double s_dir[3], double tol_deg, double* strain, double* volfrac) {
   NonlinearMechOperator& op = op_;
   hipStream_t s = op.stream();
   exa_ctx* ctx = op.GetModel()->ctx();
   double sd[3] = { s_dir[0], s_dir[1], s_dir[2] };
   ExaOptions::check_lightup(hkl, sd, tol_deg);
   const int H = (int)hkl.size() / 3;
   if (H < 1) throw std::runtime_error("lattice strains: no {hkl} family given");
   std::vector<double> axes; std::vector<int> off(1, 0);
   for (int j = 0; j < H; j++) {
      double a[3 * 24];
      const int na = exa_cubic_fiber_axes(hkl[3 * j], hkl[3 * j + 1], hkl[3 * j + 2], a, 24);
      if (na < 1 || na > 24) throw std::runtime_error("lattice strains: no fibre axes for a family");
      axes.insert(axes.end(), a, a + 3 * na); off.push_back(off.back() + na);
   }
   const double* fields = rows(at);
   if (lattice_sums_.n < (size_t)(2 * H + 1)) lattice_sums_.alloc(2 * EXA_LATTICE_MAX_HKL + 1);
   const double cos_tol = std::cos(tol_deg * (M_PI / 180.0));
   ck(ctx, exa_lattice_strains(ctx, fields, H, axes.data(), off.data(), sd, cos_tol, lattice_sums_.p, s), "exa_lattice_strains");
   comm_.allreduce_sum(lattice_sums_.p, 2 * H + 1, s);   // elements are not shared across ranks
   std::vector<double> h(2 * H + 1); lattice_sums_.download(h.data(), 2 * H + 1, s);
   for (int j = 0; j < H; j++) {
      const double v = h[2 * j + 1];
      strain[j] = v > 0.0 ? h[2 * j] / v : std::numeric_limits<double>::quiet_NaN();   // empty fibre: no lattice strain (written as nan)
      volfrac[j] = v / h[2 * H];
   }
}

// angle (degrees) of the rotation between unit quaternions a and b: d = conj(a) (x) b, 2 atan2(|d_vec|, |d_0|) (accurate near 0, unlike 2 acos |a . b|)
static double misorientation_deg(const double* a, const double* b) {
   const double d0 = a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
   const double d1 = a[0] * b[1] - b[0] * a[1] - (a[2] * b[3] - a[3] * b[2]);
   const double d2 = a[0] * b[2] - b[0] * a[2] - (a[3] * b[1] - a[1] * b[3]);
   const double d3 = a[0] * b[3] - b[0] * a[3] - (a[1] * b[2] - a[2] * b[1]);
   return 2.0 * std::atan2(std::sqrt(d1 * d1 + d2 * d2 + d3 * d3), std::fabs(d0)) * (180.0 / M_PI);
}

void StepAnalyses::EnsureGrainPlan() {
   if (!grain_plan_.empty()) return;
   int gmax = 0;
   for (int32_t a : elem_attr_) gmax = std::max(gmax, (int)a);
   const int G = (int)comm_.max_over_ranks((double)gmax);
   if (G < 1) throw std::runtime_error("grain averages: the mesh has no elements");
   if ((int64_t)4 * G > (int64_t)grain_qref_.size()) throw std::runtime_error("grain averages: grain " + std::to_string(G) + " has no reference orientation");
   if ((int64_t)G * EXA_GRAIN_NSUMS > (int64_t)INT32_MAX) throw std::runtime_error("grain averages: too many grains");
   int64_t len = 0, work = 0;
   if (exa_grain_plan(part_.E, elem_attr_.data(), nullptr, 0, &len, &work) != 0) throw std::runtime_error("grain averages: grain ids must be at least 1");
   std::vector<int32_t> plan((size_t)len);
   if (exa_grain_plan(part_.E, elem_attr_.data(), plan.data(), len, &len, &work) != 0) throw std::runtime_error("exa_grain_plan failed");
   hipStream_t s = op_.stream();
   grain_plan_dev_.alloc((size_t)len); grain_plan_dev_.upload(plan.data(), (size_t)len, s);
   grain_work_.alloc((size_t)std::max<int64_t>(work, 1));
   grain_sums_.alloc((size_t)G * EXA_GRAIN_NSUMS);
   grain_quat_dev_.alloc((size_t)4 * G);
   grain_attr_dev_.upload(elem_attr_, s);   // the map itself, for the analyses that take it element by element (LatticeCurvature)
   grain_G_ = G;
   grain_plan_ = std::move(plan);
}

void StepAnalyses::GrainMeans(const double* rows, std::vector<double>& h, std::vector<double>& qbar, double& vtot) {
   NonlinearMechOperator& op = op_;
   hipStream_t s = op.stream();
   exa_ctx* ctx = op.GetModel()->ctx();
   const int G = grain_G_; constexpr int K = EXA_GRAIN_NSUMS;
   // pass 1: the 39 sums of every grain; elements are not shared across ranks, grains are
   grain_quat_dev_.upload(grain_qref_.data(), (size_t)4 * G, s);
   grain_sums_.zero(s);
   ck(ctx, exa_grain_sums(ctx, 1, rows, grain_plan_.data(), grain_plan_dev_.p, G, grain_quat_dev_.p, grain_work_.p, grain_sums_.p, s), "exa_grain_sums");
   comm_.allreduce_sum(grain_sums_.p, G * K, s);
   h.resize((size_t)G * K); grain_sums_.download(h.data(), h.size(), s);
   // the grain means, identical on every rank
   qbar.assign(grain_qref_.begin(), grain_qref_.begin() + 4 * (size_t)G);
   vtot = 0.0;
   for (int g = 0; g < G; g++) {
      const double* r = &h[(size_t)g * K];
      if (!(r[1] > 0.0)) continue;
      vtot += r[0];
      const double n = std::sqrt(r[35] * r[35] + r[36] * r[36] + r[37] * r[37] + r[38] * r[38]);
      if (n > 0.0) for (int k = 0; k < 4; k++) qbar[4 * (size_t)g + k] = r[35 + k] / n;
   }
}

void StepAnalyses::GrainAverages(const StepState& at, std::vector<int32_t>& ids, std::vector<double>& vals) {
   NonlinearMechOperator& op = op_;
   hipStream_t s = op.stream();
   exa_ctx* ctx = op.GetModel()->ctx();
   EnsureGrainPlan();
   const int G = grain_G_; constexpr int K = EXA_GRAIN_NSUMS;
   const double* fields = rows(at);
   std::vector<double> h, qbar; double vtot = 0.0;
   GrainMeans(fields, h, qbar, vtot);
   // pass 2: sum V theta and max theta about the means
   grain_quat_dev_.upload(qbar.data(), (size_t)4 * G, s);
   EXA_HC(hipMemsetAsync(grain_sums_.p, 0, sizeof(double) * 2 * G, s));
   ck(ctx, exa_grain_sums(ctx, 2, fields, grain_plan_.data(), grain_plan_dev_.p, G, grain_quat_dev_.p, grain_work_.p, grain_sums_.p, s), "exa_grain_sums");
   comm_.allreduce_sum(grain_sums_.p, G, s);
   comm_.allreduce_max(grain_sums_.p + G, G, s);
   std::vector<double> h2((size_t)2 * G); grain_sums_.download(h2.data(), h2.size(), s);
   ids.clear(); vals.clear();
   for (int g = 0; g < G; g++) {
      const double* r = &h[(size_t)g * K];
      if (!(r[1] > 0.0)) continue;
      const double V = r[0], iv = 1.0 / V;
      double o[GRAIN_NVALS];
      o[0] = r[1]; o[1] = V; o[2] = V / vtot;
      for (int k = 0; k < 6; k++) o[3 + k] = r[2 + k] * iv;
      const double* t = o + 3;
      const double d01 = t[0] - t[1], d12 = t[1] - t[2], d20 = t[2] - t[0];   // EXA_F_VONMISES, EXA_F_HYDROSTATIC of the mean stress
      o[9] = std::sqrt(0.5 * (d01 * d01 + d12 * d12 + d20 * d20 + 6.0 * (t[3] * t[3] + t[4] * t[4] + t[5] * t[5])));
      o[10] = (t[0] + t[1] + t[2]) * (1.0 / 3.0);
      for (int k = 0; k < 12; k++) o[11 + k] = r[8 + k] * iv;    // elastic strain in the sample and the crystal frame
      for (int k = 0; k < 15; k++) o[23 + k] = r[20 + k] * iv;   // EffPlasticStrain, DpEff, Hardness, ShearRate (12)
      for (int k = 0; k < 4; k++) o[38 + k] = qbar[4 * (size_t)g + k];
      o[42] = h2[g] * iv; o[43] = h2[(size_t)G + g];
      o[44] = misorientation_deg(&qbar[4 * (size_t)g], &grain_qref_[4 * (size_t)g]);
      ids.push_back(g + 1);
      vals.insert(vals.end(), o, o + GRAIN_NVALS);
   }
}

// element rows -> grain means (pass 1 of the grain sums) -> per-element rotation vectors and their nodal sums -> the sum over the
// copies of a node, on the path every assembled L-vector takes (periodic images, then ranks; segment by segment in deterministic mode) ->
// curvature rows -> summary
void StepAnalyses::LatticeCurvature(const StepState& at, double burgers, std::vector<double>& rows, double* summary7, bool want_rows) {
   if (!(burgers > 0.0) || !std::isfinite(burgers)) throw std::runtime_error("lattice curvature: the Burgers vector length must be a finite number > 0");
   NonlinearMechOperator& op = op_;
   hipStream_t s = op.stream();
   exa_ctx* ctx = op.GetModel()->ctx();
   EnsureGrainPlan();
   const int G = grain_G_;
   const double* fields = this->rows(at);
   std::vector<double> h, qbar; double vtot = 0.0;
   GrainMeans(fields, h, qbar, vtot);
   grain_quat_dev_.upload(qbar.data(), (size_t)4 * G, s);
   int64_t work = 0; int planes = 0;
   exa_curvature_sizes(part_.E, &work, &planes);
   const size_t nn = (size_t)part_.NN;
   if (curv_work_.n != (size_t)std::max<int64_t>(work, 1)) curv_work_.alloc((size_t)std::max<int64_t>(work, 1));
   if (curv_nodal_.n != (size_t)planes * nn) curv_nodal_.alloc((size_t)planes * nn);
   if (curv_rows_.n != (size_t)EXA_NCURV * part_.E) curv_rows_.alloc((size_t)EXA_NCURV * part_.E);
   if (curv_sum_.n < 7) curv_sum_.alloc(7);
   if (curv_xe_.n != (size_t)3 * part_.n * part_.E) curv_xe_.alloc((size_t)3 * part_.n * part_.E);
   DevBuf<double>& xe = curv_xe_;
   ck(ctx, exa_restrict(ctx, op.x_cur.p, xe.p, s), "exa_restrict");
   ck(ctx, exa_curvature_nodal(ctx, fields, grain_attr_dev_.p, G, grain_quat_dev_.p, curv_work_.p, curv_nodal_.p, s), "exa_curvature_nodal");
   for (int t = 0; t < planes / 3; t++) op.SumLVector(curv_nodal_.p + (size_t)3 * nn * t, nullptr, false);
   ck(ctx, exa_curvature_elements(ctx, fields, grain_attr_dev_.p, G, grain_quat_dev_.p, curv_work_.p, curv_nodal_.p, xe.p, burgers, curv_rows_.p, s),
             "exa_curvature_elements");
   ck(ctx, exa_curvature_summary(ctx, fields, curv_rows_.p, curv_sum_.p, s), "exa_curvature_summary");
   comm_.allreduce_sum(curv_sum_.p, 4, s);   // elements are not shared across ranks
   comm_.allreduce_max(curv_sum_.p + 4, 3, s);
   double t7[7]; curv_sum_.download(t7, 7, s);
   rows.resize(want_rows ? (size_t)EXA_NCURV * part_.E : 0);
   if (!rows.empty()) curv_rows_.download(rows.data(), rows.size(), s);
   const double iv = 1.0 / t7[0];
   for (int k = 0; k < 3; k++) { summary7[2 * k] = t7[1 + k] * iv; summary7[2 * k + 1] = t7[4 + k]; }
   summary7[6] = t7[0];
}

void StepAnalyses::WriteLatticeCurvature(const StepState& at, int step, const double* m) {
   if (comm_.rank != 0) return;
   const std::string path = at.out_dir + "/" + opt_.lattice_curvature_fname;
   bool fresh = true;
   { std::ifstream g(path); fresh = !g || g.peek() == std::ifstream::traits_type::eof(); }
   std::ofstream f(path, std::ios_base::app);   // a restarted run goes on in the file it finds
   if (!f) throw std::runtime_error("lattice curvature: cannot write " + path);
   if (fresh) f << "# step time grod_mean_deg grod_max_deg kam_mean_deg kam_max_deg gnd_density_mean gnd_density_max\n";
   f << std::setprecision(17) << step << ' ' << at.time;
   for (int k = 0; k < 6; k++) f << ' ' << m[k];
   f << '\n';
}

void StepAnalyses::PoleFigures(const StepState& at, const std::vector<int>& hkl, std::vector<double> dirs, double res_deg, std::vector<double>& mrd) {
   NonlinearMechOperator& op = op_;
   hipStream_t s = op.stream();
   exa_ctx* ctx = op.GetModel()->ctx();
   ExaOptions::check_texture(hkl, dirs, res_deg, false);
   const int H = (int)hkl.size() / 3, D = (int)dirs.size() / 3, nset = H + D;
   int na = 0, nb = 0;
   exa_texture_grid(res_deg, &na, &nb);
   std::vector<double> axes; std::vector<int> off(1, 0);
   for (int j = 0; j < H; j++) {
      double a[3 * 24];
      const int n = exa_cubic_fiber_axes(hkl[3 * j], hkl[3 * j + 1], hkl[3 * j + 2], a, 24);
      if (n < 1 || n > 24) throw std::runtime_error("texture: no pole axes for a family");
      axes.insert(axes.end(), a, a + 3 * n); off.push_back(off.back() + n);
   }
   const double* fields = rows(at);
   // the quantum 2^q of the integer weights, the same on every rank and for any rank count: from the largest element volume and the element
   // count over all ranks (a max and a sum of integers are exact)
   if (texture_vmax_.n < 2) texture_vmax_.alloc(2);
   ck(ctx, exa_texture_volume_max(ctx, fields, texture_vmax_.p, s), "exa_texture_volume_max");
   const double ne = (double)part_.E;
   EXA_HC(hipMemcpyAsync(texture_vmax_.p + 1, &ne, sizeof(double), hipMemcpyHostToDevice, s));
   comm_.allreduce_max(texture_vmax_.p, 1, s);
   comm_.allreduce_sum(texture_vmax_.p + 1, 1, s);
   double vn[2] = { 0.0, 0.0 }; texture_vmax_.download(vn, 2, s);
   const int qlog2 = exa_texture_quantum_log2(vn[0], (int64_t)vn[1]);
   const size_t nbins = (size_t)nset * na * nb;
   if (texture_counts_.n < nbins) texture_counts_.alloc(nbins);
   ck(ctx, exa_texture_weights(ctx, fields, H, axes.data(), off.data(), D, dirs.data(), res_deg, qlog2, texture_counts_.p, s), "exa_texture_weights");
   std::vector<int64_t> c(nbins); texture_counts_.download(c.data(), nbins, s);
   if (comm_.nranks > 1) {   // exact sums over the ranks: the counts (< 2^62) travel as two 32-bit halves in doubles, whose sums stay below 2^53
      std::vector<double> h2(2 * nbins);
      for (size_t b = 0; b < nbins; b++) { h2[b] = (double)(uint64_t)(c[b] >> 32); h2[nbins + b] = (double)(uint64_t)(c[b] & 0xffffffffll); }
      DevBuf<double> d; d.upload(h2, s);
      comm_.allreduce_sum(d.p, (int)(2 * nbins), s);
      d.download(h2.data(), 2 * nbins, s);
      for (size_t b = 0; b < nbins; b++) c[b] = (int64_t)(((uint64_t)h2[b] << 32) + (uint64_t)h2[nbins + b]);
   }
   // MRD_ik = (W_ik / W_tot) 2 pi / dOmega_i with dOmega_i = res (cos i res - cos (i + 1) res)
   const double r = res_deg * (M_PI / 180.0);
   std::vector<double> f(na);
   for (int i = 0; i < na; i++) f[i] = 2.0 * M_PI / (r * (std::cos(i * r) - std::cos((i + 1) * r)));
   mrd.assign(nbins, 0.0);
   for (int j = 0; j < nset; j++) {
      const int64_t* w = c.data() + (size_t)j * na * nb;
      int64_t tot = 0;
      for (int b = 0; b < na * nb; b++) tot += w[b];
      const double inv = 1.0 / (double)tot;   // an empty set (no volume): NaN
      for (int i = 0; i < na; i++)
         for (int k = 0; k < nb; k++) mrd[(size_t)j * na * nb + (size_t)i * nb + k] = (double)w[i * nb + k] * inv * f[i];
   }
}

void StepAnalyses::WriteTexture(const StepState& at, int step) {
   std::vector<double> dirs = opt_.texture_dirs, mrd;
   PoleFigures(at, opt_.texture_hkl, dirs, opt_.texture_res_deg, mrd);
   if (comm_.rank != 0) return;
   char tag[16]; std::snprintf(tag, sizeof(tag), "_%06d.txt", step);
   write_texture(at.out_dir + "/" + opt_.texture_fname + tag, step, at.time, opt_.texture_res_deg, opt_.texture_hkl, dirs, mrd);
}

void write_texture(const std::string& path, int step, double t, double res_deg, const std::vector<int>& hkl, const std::vector<double>& dirs,
                   const std::vector<double>& mrd) {
   int na = 0, nb = 0;
   if (exa_texture_grid(res_deg, &na, &nb) != 0) throw std::runtime_error("texture: bad res_deg");
   const int H = (int)hkl.size() / 3, D = (int)dirs.size() / 3;
   if (mrd.size() != (size_t)(H + D) * na * nb) throw std::runtime_error("texture: " + path + ": MRD of the wrong size");
   std::ofstream f(path);
   if (!f) throw std::runtime_error("texture: cannot write " + path);
   f << std::setprecision(17);
   f << "# texture step " << step << " time " << t << " res_deg " << res_deg << " n_alpha " << na << " n_beta " << nb << "\n";
   for (int j = 0; j < H + D; j++) {
      if (j < H) f << "# pole figure {" << hkl[3 * j] << ' ' << hkl[3 * j + 1] << ' ' << hkl[3 * j + 2] << "}\n";
      else f << "# inverse pole figure [" << dirs[3 * (j - H)] << ' ' << dirs[3 * (j - H) + 1] << ' ' << dirs[3 * (j - H) + 2] << "]\n";
      const double* m = mrd.data() + (size_t)j * na * nb;
      for (int i = 0; i < na; i++) {
         for (int k = 0; k < nb; k++) f << (k ? " " : "") << m[i * nb + k];
         f << '\n';
      }
   }
   if (!f) throw std::runtime_error("texture: writing " + path + " failed");
}

void write_grain_avgs(const std::string& path, int n, const int32_t* ids, const double* vals) {
   std::ofstream f(path);
   if (!f) throw std::runtime_error("grain averages: cannot write " + path);
   f << "# grain_id n_elements volume volume_fraction stress_11 stress_22 stress_33 stress_23 stress_13 stress_12 von_mises hydrostatic"
        " elastic_strain_sample_11 elastic_strain_sample_22 elastic_strain_sample_33 elastic_strain_sample_23 elastic_strain_sample_13 elastic_strain_sample_12"
        " elastic_strain_xtal_11 elastic_strain_xtal_22 elastic_strain_xtal_33 elastic_strain_xtal_23 elastic_strain_xtal_13 elastic_strain_xtal_12"
        " eff_plastic_strain dp_eff hardness";
   for (int k = 1; k <= 12; k++) f << " shear_rate_" << k;
   f << " quat_0 quat_1 quat_2 quat_3 misori_mean_deg misori_max_deg rotation_deg\n";
   f << std::setprecision(17);
   for (int i = 0; i < n; i++) {
      const double* v = vals + (size_t)i * GRAIN_NVALS;
      f << ids[i] << ' ' << (int64_t)v[0];
      for (int k = 1; k < GRAIN_NVALS; k++) f << ' ' << v[k];
      f << '\n';
   }
   if (!f) throw std::runtime_error("grain averages: writing " + path + " failed");
}

void StepAnalyses::SaveFields(const StepState& at, const std::string& dir, int cycle, double t) {
   std::vector<double> curv; SlipActivityResult fat;
   if (opt_.lattice_curvature) { double m[7]; LatticeCurvature(at, opt_.lattice_curvature_burgers, curv, m); }
   if (opt_.fatigue) SlipActivity(at, opt_.fatigue_k, opt_.fatigue_sigma_y, fat);
   SaveCycle(at, dir, cycle, t, curv, fat);
}

// curv, fat: the curvature rows and the slip-activity evaluation of this state (read with Visualizations.lattice_curvature / fatigue on only)
void StepAnalyses::SaveCycle(const StepState& at, const std::string& dir, int cycle, double t, const std::vector<double>& curv, const SlipActivityResult& fat) {
   NonlinearMechOperator& op = op_;
   hipStream_t s = op.stream();
   rows(at); const std::vector<double> fields = fields_dev_.to_host(s);
   const std::vector<double> xc = op.x_cur.to_host(s), xr = op.x_ref.to_host(s), v = at.vel.to_host(s);
   vtu::Piece p;
   p.E = part_.E; p.NN = part_.NN; p.n = part_.n; p.tet = part_.geom == 1; p.conn = part_.conn.data();
   p.x_cur = xc.data(); p.x_ref = xr.data(); p.vel = v.data(); p.fields = fields.data(); p.attr = elem_attr_.data(); p.gid = part_.elem_gid.data();
   if (opt_.lattice_curvature) { p.has_curv = true; p.curv = curv.data(); }
   if (opt_.fatigue) { p.has_fatigue = true; p.fip = fat.fip.data(); p.slip_acc = fat.acc.data(); }
   vtu::save_cycle(dir, comm_.rank, comm_.nranks, cycle, t, opt_.light_up, p, ckpt.pvd_cycles[dir]);
}

void append_row(const std::string& path, const double* v, int n) {   // (also rewrites the files of a restarted run: host/checkpoint.hip)
   std::ofstream f(path, std::ios_base::app);
   for (int i = 0; i < n; i++) { f << v[i]; f << (i + 1 == n ? '\n' : ' '); }   // mfem::Vector::Print(out, width = n)
}

void StepAnalyses::EnableSlipActivity() {
   if (fatigue_on_) return;
   if (started_ || restored_) throw std::runtime_error("enable_slip_activity: the accumulators can only be switched on before the first step");
   if (exa_slip_plane_normals(op_.cfg_used.model, fat_normals_) != 0) throw std::runtime_error("slip activity: no slip-plane normals for this model");
   fatigue_on_ = true;
}

// the accumulators of a fresh run: zero, and the window of the initial state (Gamma = 0, the normal stresses of its rows)
void StepAnalyses::EnsureFatigueInit(const StepState& at) {
   if (fatigue_init_) return;
   if (at.step > 0) throw std::runtime_error("slip activity: the accumulators of this run were never started");
   hipStream_t s = op_.stream();
   exa_ctx* ctx = op_.GetModel()->ctx();
   int64_t n = 0; exa_slip_activity_sizes(part_.E, &n);
   fat_acc_.alloc((size_t)std::max<int64_t>(n, 1)); fat_acc_.zero(s);
   fat_gid_.upload(part_.elem_gid, s);
   ComputeElementFields(at);
   ck(ctx, exa_slip_accumulate(ctx, fields_dev_.p, fat_normals_, 0.0, 1, fat_acc_.p, s), "exa_slip_accumulate");
   ckpt.fatigue_window_start = 0; fatigue_init_ = true;
}

void StepAnalyses::ResetFatigueWindow(const StepState& at) {
   if (!fatigue_on_) throw std::runtime_error("reset_fatigue_window: slip activity is not on (Visualizations.fatigue or enable_slip_activity)");
   if (at.step == 0 && !restored_) { EnsureFatigueInit(at); return; }   // before step 1 the window is the initial state: nothing is pending
   ckpt.fatigue_pending = true;
}

void StepAnalyses::SlipActivity(const StepState& at, double k_fs, double sigma_y, SlipActivityResult& res, bool want_acc) {
   if (!fatigue_on_) throw std::runtime_error("slip activity is not on (Visualizations.fatigue or enable_slip_activity before the first step)");
   if (!(k_fs >= 0.0) || !std::isfinite(k_fs)) throw std::runtime_error("slip activity: k must be a finite number >= 0");
   if (!(sigma_y > 0.0) || !std::isfinite(sigma_y)) throw std::runtime_error("slip activity: sigma_y must be a finite number > 0");
   hipStream_t s = op_.stream();
   exa_ctx* ctx = op_.GetModel()->ctx();
   EnsureFatigueInit(at);
   const double* fields = rows(at);
   const size_t E = (size_t)part_.E;
   if (fat_rows_.n != std::max<size_t>(EXA_NFIP * E, 1)) fat_rows_.alloc(std::max<size_t>(EXA_NFIP * E, 1));
   if (fat_sum_.n < 8) fat_sum_.alloc(8);
   ck(ctx, exa_fip_rows(ctx, fat_acc_.p, k_fs, sigma_y, fat_rows_.p, s), "exa_fip_rows");
   ck(ctx, exa_fip_summary(ctx, fields, fat_rows_.p, fat_gid_.p, fat_sum_.p, s), "exa_fip_summary");
   // elements are not shared across ranks: three sums, three maxima; the element of the largest FIP is the smallest id among the ranks that attain it
   comm_.allreduce_sum(fat_sum_.p, 3, s);
   double loc[7]; fat_sum_.download(loc, 7, s);
   comm_.allreduce_max(fat_sum_.p + 3, 3, s);
   double t[7]; fat_sum_.download(t, 7, s);
   if (comm_.nranks > 1) {
      const double cand = (part_.E > 0 && loc[3] == t[3]) ? -loc[6] : -std::numeric_limits<double>::infinity();
      EXA_HC(hipMemcpyAsync(fat_sum_.p + 7, &cand, sizeof(double), hipMemcpyHostToDevice, s));
      comm_.allreduce_max(fat_sum_.p + 7, 1, s);
      double m; EXA_HC(hipMemcpyAsync(&m, fat_sum_.p + 7, sizeof(double), hipMemcpyDeviceToHost, s)); EXA_HC(hipStreamSynchronize(s));
      t[6] = -m;
   }
   const double iv = 1.0 / t[0];
   res.summary[0] = t[0]; res.summary[1] = t[1] * iv; res.summary[2] = t[3]; res.summary[3] = t[6];
   res.summary[4] = t[2] * iv; res.summary[5] = t[5]; res.summary[6] = t[4]; res.summary[7] = (double)ckpt.fatigue_window_start;
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
   for (int32_t a : elem_attr_) gmax = std::max(gmax, (int)a);
   const int G = (int)comm_.max_over_ranks((double)gmax);
   res.grain_ids.clear(); res.grain_vals.clear();
   if (G < 1) return;
   std::vector<double> V(E);
   if (E) {
      EXA_HC(hipMemcpy2DAsync(V.data(), sizeof(double), fields + EXA_F_VOLUME, sizeof(double) * EXA_NFIELDS, sizeof(double), E, hipMemcpyDeviceToHost, s));
      EXA_HC(hipStreamSynchronize(s));
   }
   std::vector<size_t> order(E);
   for (size_t e = 0; e < E; e++) order[e] = e;
   std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return part_.elem_gid[a] < part_.elem_gid[b]; });
   std::vector<double> g((size_t)3 * G, 0.0);
   std::fill(g.begin() + 2 * (size_t)G, g.end(), -std::numeric_limits<double>::infinity());
   for (size_t e : order) {
      const int a = elem_attr_[e];
      if (a < 1) continue;
      const double f = res.fip[EXA_NFIP * e + EXA_FIP_FIP];
      g[a - 1] += V[e]; g[(size_t)G + a - 1] += V[e] * f; g[2 * (size_t)G + a - 1] = std::max(g[2 * (size_t)G + a - 1], f);
   }
   if (comm_.nranks > 1) {
      if (fat_grain_.n < g.size()) fat_grain_.alloc(g.size());
      fat_grain_.upload(g.data(), g.size(), s);
      comm_.allreduce_sum(fat_grain_.p, 2 * G, s);
      comm_.allreduce_max(fat_grain_.p + 2 * (size_t)G, G, s);
      fat_grain_.download(g.data(), g.size(), s);
   }
   for (int a = 0; a < G; a++) {
      if (!(g[a] > 0.0)) continue;
      res.grain_ids.push_back(a + 1);
      res.grain_vals.push_back(g[a]); res.grain_vals.push_back(g[(size_t)G + a] / g[a]); res.grain_vals.push_back(g[2 * (size_t)G + a]);
   }
}

void StepAnalyses::WriteFatigue(const StepState& at, int step, const SlipActivityResult& r) {
   const double* m = r.summary;
   const double row[FATIGUE_ROW] = { (double)step, at.time, m[7], m[1], m[2], m[3], m[4], m[5], m[6] };
   ckpt.fatigue_rows.insert(ckpt.fatigue_rows.end(), row, row + FATIGUE_ROW);
   if (comm_.rank != 0) return;
   const std::string path = at.out_dir + "/" + opt_.fatigue_fname;
   bool fresh = true;
   { std::ifstream g(path); fresh = !g || g.peek() == std::ifstream::traits_type::eof(); }
   if (fresh) write_fatigue_rows(path, std::vector<double>(), false);   // (the header)
   write_fatigue_rows(path, std::vector<double>(row, row + FATIGUE_ROW), true);
   if (!r.grain_ids.empty()) {
      char tag[32]; std::snprintf(tag, sizeof(tag), "fatigue_grains_%06d.txt", step);
      write_fatigue_grains(at.out_dir + "/" + tag, (int)r.grain_ids.size(), r.grain_ids.data(), r.grain_vals.data());
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
