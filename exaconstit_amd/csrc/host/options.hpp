// options.toml reader for the stand-alone driver: the reference's option SCHEMA (reference src/options.toml,
// src/option_parser.cpp:26-932, src/option_types.hpp) for the subset of its hot path — auto-generated hex mesh,
// ExaCMech models, PA/EA assembly, NR/NRLS + PCG — parsed with a small TOML-subset reader (the reference vendors toml11;
// out of scope here).  Unknown keys are ignored like the reference's `toml::find_or` defaults; unsupported values abort
// with the reference's wording where one exists.
#pragma once
#include <cctype>
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../../include/exaconstit_hip.h"

namespace exa_host {

struct TomlValue {
   enum Kind { NONE, NUM, STR, BOOL, ARR } kind = NONE;
   double num = 0; std::string str; bool b = false; std::vector<TomlValue> arr;
};

class TomlDoc {
 public:
   std::map<std::string, TomlValue> kv;   // "Table.Sub.key" -> value
   static TomlDoc parse_file(const std::string& path) {
      std::ifstream f(path);
      if (!f) throw std::runtime_error("Cannot open options file: " + path);
      std::stringstream ss; ss << f.rdbuf();
      return parse(ss.str());
   }
   static TomlDoc parse(const std::string& text) {
      TomlDoc d; size_t pos = 0; std::string table;
      const size_t n = text.size();
      auto skip_ws = [&](bool newlines) { while (pos < n) { char c = text[pos]; if (c == '#') { while (pos < n && text[pos] != '\n') pos++; } else if (c == ' ' || c == '\t' || c == '\r' || (newlines && c == '\n')) pos++; else break; } };
      while (true) {
         skip_ws(true);
         if (pos >= n) break;
         if (text[pos] == '[') {
            size_t e = text.find(']', pos); if (e == std::string::npos) throw std::runtime_error("toml: unterminated table header");
            table = trim(text.substr(pos + 1, e - pos - 1)); pos = e + 1; continue;
         }
         size_t eq = text.find('=', pos); if (eq == std::string::npos) throw std::runtime_error("toml: expected key = value");
         std::string key = trim(text.substr(pos, eq - pos)); pos = eq + 1;
         skip_ws(false);
         TomlValue v = parse_value(text, pos);
         d.kv[table.empty() ? key : table + "." + key] = v;
      }
      return d;
   }
   bool has(const std::string& k) const { return kv.count(k) > 0; }
   bool has_table(const std::string& t) const { for (auto& p : kv) if (p.first.compare(0, t.size() + 1, t + ".") == 0) return true; return false; }
   double num(const std::string& k, double def) const { auto it = kv.find(k); return (it != kv.end() && it->second.kind == TomlValue::NUM) ? it->second.num : def; }
   std::string str(const std::string& k, const std::string& def) const { auto it = kv.find(k); return (it != kv.end() && it->second.kind == TomlValue::STR) ? it->second.str : def; }
   bool boolean(const std::string& k, bool def) const { auto it = kv.find(k); return (it != kv.end() && it->second.kind == TomlValue::BOOL) ? it->second.b : def; }
   const TomlValue* get(const std::string& k) const { auto it = kv.find(k); return it == kv.end() ? nullptr : &it->second; }

 private:
   static std::string trim(const std::string& s) { size_t a = 0, b = s.size(); while (a < b && std::isspace((unsigned char)s[a])) a++; while (b > a && std::isspace((unsigned char)s[b - 1])) b--; return s.substr(a, b - a); }
   static TomlValue parse_value(const std::string& t, size_t& pos) {
      TomlValue v; const size_t n = t.size();
      auto skip = [&]() { while (pos < n) { char c = t[pos]; if (c == '#') { while (pos < n && t[pos] != '\n') pos++; } else if (std::isspace((unsigned char)c)) pos++; else break; } };
      if (t[pos] == '"' || t[pos] == '\'') {
         const char q = t[pos]; size_t e = t.find(q, pos + 1); if (e == std::string::npos) throw std::runtime_error("toml: unterminated string");
         v.kind = TomlValue::STR; v.str = t.substr(pos + 1, e - pos - 1); pos = e + 1;
      } else if (t[pos] == '[') {
         v.kind = TomlValue::ARR; pos++;
         while (true) { skip(); if (pos >= n) throw std::runtime_error("toml: unterminated array"); if (t[pos] == ']') { pos++; break; } if (t[pos] == ',') { pos++; continue; } v.arr.push_back(parse_value(t, pos)); }
      } else if (t.compare(pos, 4, "true") == 0) { v.kind = TomlValue::BOOL; v.b = true; pos += 4; }
      else if (t.compare(pos, 5, "false") == 0) { v.kind = TomlValue::BOOL; v.b = false; pos += 5; }
      else {
         size_t e = pos; while (e < n && (std::isalnum((unsigned char)t[e]) || t[e] == '+' || t[e] == '-' || t[e] == '.' || t[e] == '_')) e++;
         std::string tok = t.substr(pos, e - pos); std::string clean; for (char c : tok) if (c != '_') clean += c;
         char* endp = nullptr; v.num = std::strtod(clean.c_str(), &endp);
         if (endp == clean.c_str()) throw std::runtime_error("toml: cannot parse value near '" + tok + "'");
         v.kind = TomlValue::NUM; pos = e;
      }
      return v;
   }
};

enum class Assembly { PA, EA };            // reference src/option_types.hpp (FULL is mapped to EA: same operator, no sparse matrix/AMG)
enum class NLSolver { NR, NRLS };
enum class XtalType { FCC, BCC };
enum class SlipType { POWERVOCE, POWERVOCENL, MTSDD };

// comps < 0: velocity-gradient condition on components |comp| (reference src/option_parser.cpp:178-195)
struct BCEntry { int step; std::vector<int> ids, comps; std::vector<double> vals; double vgrad[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 }; };

struct ExaOptions {
   std::string basedir;
   double temp_k = 298.0;
   std::string props_file; int nprops = 0;
   std::string ori_file, grain_file; int num_grains = 0; std::string ori_type = "quat";
   std::vector<BCEntry> bcs; bool vgrad_origin_flag = false; double vgrad_origin[3] = { 0, 0, 0 };
   // [BCs] periodic = true (not a key of the reference): periodic in all three directions under the macroscopic velocity gradient
   // essential_vel_grad (one 3 x 3 per update step with changing_ess_bcs); the entries of bcs then carry no ids, only vgrad
   bool periodic = false;
   // [BCs] periodic_free = 3 x 3 of 0 / 1: entry (i, d) free = the mean traction component i on face pair d is zero and the entry of
   // the velocity gradient an unknown; the others stay prescribed at essential_vel_grad.  All zero (or no key): every entry prescribed, as in 4.11.
   bool periodic_mixed = false; uint8_t periodic_free[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
   // the refusals of a mask, shared with SystemDriver::SetPeriodic: the message, or nullptr for a mask that can be run
   static const char* periodic_free_refusal(const uint8_t* f) {
      int n = 0; for (int k = 0; k < 9; k++) n += f[k] ? 1 : 0;
      if (n == 9) return "BCs.periodic_free: all nine entries are free - at least one entry of the velocity gradient must stay prescribed";
      for (int i = 0; i < 3; i++) for (int j = i + 1; j < 3; j++) if (f[3 * i + j] && f[3 * j + i])
         return "BCs.periodic_free: both entries of an off-diagonal pair (i, j), (j, i) are free - the rigid rotation would be free";
      return nullptr;
   }
   // multigrid and the polynomial order (options reader, SystemDriver::SetPreconditioner / SetPeriodic)
   static const char* mg_order_refusal() { return "Solvers.Krylov.preconditioner = \"multigrid\" is built for p_refinement = 1 only"; }   // (p_refinement = 2: opt-in, Solvers.Krylov.mg_p2 = true)
   static const char* mg_p2_no_higher_order() { return "Solvers.Krylov.preconditioner = \"multigrid\": mg_p2 = true serves p_refinement = 2; p_refinement >= 3 has no hierarchy (its nodes are not a uniform grid)"; }
   static const char* gmres_kdim_range() { return "Solvers.Krylov.gmres_kdim must be a whole number in 1 ... 100 (the Krylov dimension of GMRES; MFEM's default is 50)"; }
   static const char* mg_p2_no_periodic() { return "Solvers.Krylov.preconditioner = \"multigrid\" at p_refinement = 2 is not built for BCs.periodic = true (the fine diagonal probe and the fused periodic kernels need p_refinement = 1), with or without mg_periodic"; }
   // B-bar under multigrid is opt-in (Solvers.Krylov.mg_bbar; DESIGN 4.6, "B-bar"): the refusal without the key, and what stays refused with it
   static const char* mg_no_bbar() { return "Solvers.Krylov.preconditioner = \"multigrid\" is not built for integ_model = \"BBAR\""; }
   static const char* mg_bbar_no_periodic() { return "Solvers.Krylov.preconditioner = \"multigrid\" with mg_bbar = true is not built for BCs.periodic = true (the fused periodic kernels and the control block of mixed loading were never run on the B-bar operator), with or without mg_periodic"; }
   static const char* periodic_no_multigrid() { return "BCs.periodic = true runs under Solvers.Krylov.preconditioner = \"multigrid\" only where it is asked for: Solvers.Krylov.mg_periodic = true (Driver.set_preconditioner(\"multigrid\", periodic=True)); without it the combination is refused as before"; }
   static const char* periodic_needs_generated_mesh() { return "BCs.periodic = true needs a generated hexahedral mesh (Mesh.type = \"auto\"): file and tetrahedral meshes need node matching"; }
   XtalType xtal = XtalType::FCC; SlipType slip = SlipType::POWERVOCE;
   bool dt_cust = false, dt_auto = false; std::vector<double> cust_dt; double dt = 1.0, t_final = 1.0;
   double dt_min = 1.0, dt_scale = 0.25; int nsteps = 1; std::string auto_dt_fname = "auto_dt_out.txt";
   std::string avg_stress_fname = "avg_stress.txt", avg_def_grad_fname = "avg_def_grad.txt", avg_pl_work_fname = "avg_pl_work.txt", avg_dp_tensor_fname = "avg_dp_tensor.txt";
   bool additional_avgs = false;
   // [Checkpoint], every key optional: write = true writes <floc>_<step %06d>.ckpt into the output directory every `steps` steps and
   // after the last one, keeping the newest `keep` files; restart_from names a checkpoint to resume from (relative to the options file)
   bool ckpt_write = false; int ckpt_steps = 1, ckpt_keep = 2; std::string ckpt_floc = "checkpoint", ckpt_restart_from;
   // ParaView output of the per-element fields (reference src/option_parser.cpp:540-570): Visualizations.paraview / steps / floc / light_up.
   // visit, conduit and adios2 are read by the reference too; nothing is written for them here.
   bool paraview = false, light_up = false; int vis_steps = 1; std::string vis_floc = "results/exaconstit";
   // in-situ lattice strains of {hkl} fibres (the reference's light-up post-processing, scripts/postprocessing/calc_lattice_strain.py):
   // on when light_up = true and Visualizations.light_up_hkl is given.  lightup_hkl holds 3 integers per family; lightup_s_dir is unit.
   std::vector<int> lightup_hkl; double lightup_s_dir[3] = { 0, 0, 1 }; double lightup_tol_deg = 5.0;
   std::string lightup_strain_fname = "lattice_strains.txt", lightup_volume_fname = "lattice_volumes.txt";
   bool lightup() const { return light_up && !lightup_hkl.empty(); }
   // the checks of the light-up keys, shared with exa_driver_lattice_strains (hkl may be empty here); normalises s in place
   static void check_lightup(const std::vector<int>& hkl, double s[3], double tol_deg) {
      if (hkl.size() % 3 != 0) throw std::runtime_error("Visualizations.light_up_hkl must hold [h, k, l] triples");
      if (hkl.size() > 3 * 16) throw std::runtime_error("Visualizations.light_up_hkl holds at most 16 triples");
      for (size_t j = 0; j < hkl.size(); j += 3)
         if (hkl[j] == 0 && hkl[j + 1] == 0 && hkl[j + 2] == 0) throw std::runtime_error("Visualizations.light_up_hkl: [0, 0, 0] is not a plane family");
      const double n = std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
      if (!(n > 0.0) || !std::isfinite(n)) throw std::runtime_error("Visualizations.light_up_s_dir must be a non-zero vector");
      for (int i = 0; i < 3; i++) s[i] /= n;
      if (!(tol_deg > 0.0 && tol_deg <= 90.0)) throw std::runtime_error("Visualizations.light_up_dist_tol_deg must lie in (0, 90]");
   }
   // per-grain averages written every Visualizations.steps steps (host/analyses.hip, StepAnalyses::GrainAverages): <out_dir>/<grain_avgs_fname>_<step %06d>.txt
   bool grain_avgs = false; std::string grain_avgs_fname = "grain_avgs";
   // texture (host/analyses.hip, StepAnalyses::PoleFigures): pole figures of the texture_hkl families and inverse pole figures of the
   // texture_ipf_dirs (unit) in multiples of random distribution, written at step 0, every Visualizations.steps steps and at the last step
   // to <out_dir>/<texture_fname>_<step %06d>.txt
   bool texture = false; std::vector<int> texture_hkl = { 1, 1, 1, 2, 0, 0, 2, 2, 0 }; std::vector<double> texture_dirs = { 0, 0, 1 };
   double texture_res_deg = 5.0; std::string texture_fname = "texture";
   // macroscopic tangent (host/tangent.hip, SystemDriver::MacroTangent): d sigma_bar / d L_bar of the converged step of a periodic cell,
   // one row (step, time, dt, V, 81 values with 17 significant digits) appended to <out_dir>/<macro_tangent_fname> every Visualizations.steps steps
   // and at the last step.  rel_tol / max_iter of its nine solves: 0 = the Solvers.Krylov values
   bool macro_tangent = false; std::string macro_tangent_fname = "macro_tangent.txt"; double macro_tangent_rel_tol = 0.0; int macro_tangent_max_iter = 0;
   // intragranular misorientation and lattice curvature (host/analyses.hip, StepAnalyses::LatticeCurvature): one row (step, time, mean and
   // max of GROD, KAM and the GND density, 17 significant digits) appended to <out_dir>/<lattice_curvature_fname> every Visualizations.steps steps and
   // at the last step, and four more cell arrays in the ParaView pieces; lattice_curvature_burgers: Burgers vector length in the mesh's length unit
   bool lattice_curvature = false; double lattice_curvature_burgers = 1.0; std::string lattice_curvature_fname = "lattice_curvature.txt";
   // slip-system activity and the Fatemi-Socie fatigue indicator parameter (host/analyses.hip, StepAnalyses::SlipActivity): accumulated in every
   // committed step; evaluated every fatigue_cycle_steps steps (0: every Visualizations.steps steps) and at the last step - one row appended to
   // <out_dir>/<fatigue_fname>, the per-grain file fatigue_grains_<step %06d>.txt - and, with fatigue_cycle_steps > 0, the window reset after it; four
   // more cell arrays in the ParaView pieces.  fatigue_sigma_y (the yield stress that scales the normal stress) has no default
   bool fatigue = false; double fatigue_k = 0.5, fatigue_sigma_y = 0.0; int fatigue_cycle_steps = 0; std::string fatigue_fname = "fatigue.txt";
   static const char* macro_tangent_needs_periodic() { return "Visualizations.macro_tangent = true needs BCs.periodic = true: the homogenised tangent is that of a periodic cell"; }
   // the checks of the texture keys, shared with exa_driver_pole_figures (hkl: 3 integers per family, dirs: 3 components per direction,
   // normalised in place; the driver takes 0 families as long as there is a direction)
   static void check_texture(const std::vector<int>& hkl, std::vector<double>& dirs, double res_deg, bool need_hkl = true) {
      if (hkl.size() % 3 != 0) throw std::runtime_error("Visualizations.texture_hkl must hold [h, k, l] triples");
      if ((need_hkl && hkl.empty()) || hkl.size() > 3 * 16) throw std::runtime_error("Visualizations.texture_hkl holds 1 to 16 triples");
      for (size_t j = 0; j < hkl.size(); j += 3)
         if (hkl[j] == 0 && hkl[j + 1] == 0 && hkl[j + 2] == 0) throw std::runtime_error("Visualizations.texture_hkl: [0, 0, 0] is not a plane family");
      if (dirs.size() % 3 != 0 || dirs.size() > 9) throw std::runtime_error("Visualizations.texture_ipf_dirs holds 0 to 3 directions of 3 components");
      if (hkl.empty() && dirs.empty()) throw std::runtime_error("texture: no pole figure family and no inverse pole figure direction given");
      for (size_t m = 0; m < dirs.size(); m += 3) {
         const double n = std::sqrt(dirs[m] * dirs[m] + dirs[m + 1] * dirs[m + 1] + dirs[m + 2] * dirs[m + 2]);
         if (!(n > 0.0) || !std::isfinite(n)) throw std::runtime_error("Visualizations.texture_ipf_dirs: every direction must be a non-zero vector");
         for (int i = 0; i < 3; i++) dirs[m + i] /= n;
      }
      if (exa_texture_grid(res_deg, nullptr, nullptr) != 0)
         throw std::runtime_error("Visualizations.texture_res_deg must divide 90 and lie in [2, 30] degrees");
   }
   Assembly assembly = Assembly::EA; NLSolver nl_solver = NLSolver::NR; std::string integ_model = "FULL";
   int newton_iter = 25; double newton_rel = 1e-5, newton_abs = 1e-10;
   int krylov_iter = 200; double krylov_rel = 1e-10, krylov_abs = 1e-30; std::string krylov_solver = "PCG"; int gmres_kdim = 0;   // gmres_kdim: Krylov dimension, the opt-in of solver = "GMRES"
   // Solvers.Krylov.preconditioner (not a key of the reference, whose TOML reader ignores it): 0 absent (the jacobi flag of exa_driver_create
   // decides), 1 "jacobi", 2 "multigrid" (host/multigrid.hpp) with mg_levels coarse levels at most (0: as many as the mesh allows) and a
   // Chebyshev smoother of degree mg_smoother_degree (1 ... 8)
   int precond = 0, mg_levels = 0, mg_degree = 2;
   bool mg_bbar = false;       // Solvers.Krylov.mg_bbar: multigrid under integ_model = "BBAR" ("B-bar"); refused without it, as before; nothing on a FULL run
   bool mg_p2 = false;         // Solvers.Krylov.mg_p2: multigrid at p_refinement = 2 ("p = 2"); refused without it, as before the hierarchy served p = 2
   bool mg_periodic = false;   // Solvers.Krylov.mg_periodic: multigrid on a periodic cell ("periodic cells"); refused without it, as before the hierarchy served periodic cells
   int ref_ser = 0, order = 1; int ncuts[3] = { 1, 1, 1 }; double length[3] = { 1, 1, 1 }; std::string mesh_type = "auto", mesh_file;

   static std::vector<double> load_numbers(const std::string& path) {
      std::ifstream f(path); if (!f) throw std::runtime_error("Cannot open data file: " + path);
      std::vector<double> v; double x; while (f >> x) v.push_back(x); return v;
   }
   std::string resolve(const std::string& f) const { return (f.empty() || f[0] == '/') ? f : basedir + "/" + f; }

   static std::string lower(std::string s) { for (auto& c : s) c = (char)std::tolower((unsigned char)c); return s; }

   void parse_options(const std::string& path) {
      const size_t sl = path.find_last_of('/'); basedir = sl == std::string::npos ? "." : path.substr(0, sl);
      TomlDoc d = TomlDoc::parse_file(path);
      temp_k = d.num("Properties.temperature", 298.0);
      props_file = d.str("Properties.Matl_Props.floc", "props.txt"); nprops = (int)d.num("Properties.Matl_Props.num_props", 1);
      ori_file = d.str("Properties.Grain.ori_floc", "ori.txt"); grain_file = d.str("Properties.Grain.grain_floc", "grain_map.txt");
      num_grains = (int)d.num("Properties.Grain.num_grains", 0); ori_type = lower(d.str("Properties.Grain.ori_type", "euler"));
      if (ori_type != "quat" && ori_type != "quaternion") throw std::runtime_error("Only quaternion orientations (ori_type = \"quat\") are supported by this driver");
      // BCs (reference src/option_parser.cpp get_bcs): either flat arrays or arrays-of-arrays keyed by update_steps
      const bool changing = d.boolean("BCs.changing_ess_bcs", false);
      const TomlValue* ids = d.get("BCs.essential_ids"); const TomlValue* comps = d.get("BCs.essential_comps"); const TomlValue* vals = d.get("BCs.essential_vals");
      const TomlValue* vgr = d.get("BCs.essential_vel_grad");
      if (const TomlValue* pv = d.get("BCs.periodic")) {
         if (pv->kind != TomlValue::BOOL) throw std::runtime_error("BCs.periodic must be true or false");
         periodic = pv->b;
      }
      if (const TomlValue* pf = d.get("BCs.periodic_free")) {
         if (!periodic) throw std::runtime_error("BCs.periodic_free needs BCs.periodic = true");
         const char* bad = "BCs.periodic_free must be a 3 x 3 array of 0 / 1 (or true / false)";
         if (pf->kind != TomlValue::ARR || pf->arr.size() != 3) throw std::runtime_error(bad);
         for (int i = 0; i < 3; i++) {
            const TomlValue& row = pf->arr[i];
            if (row.kind != TomlValue::ARR || row.arr.size() != 3) throw std::runtime_error(bad);
            for (int j = 0; j < 3; j++) {
               const TomlValue& x = row.arr[j];
               if (x.kind == TomlValue::BOOL) periodic_free[3 * i + j] = x.b ? 1 : 0;
               else if (x.kind == TomlValue::NUM && (x.num == 0.0 || x.num == 1.0)) periodic_free[3 * i + j] = x.num == 1.0 ? 1 : 0;
               else throw std::runtime_error(bad);
            }
         }
         if (const char* why = periodic_free_refusal(periodic_free)) throw std::runtime_error(why);
         for (int k = 0; k < 9; k++) periodic_mixed = periodic_mixed || periodic_free[k];
      }
      if (periodic) {   // no faces are prescribed: the essential set is the eight corners (SystemDriver::UpdateEssBdr)
         auto given = [](const TomlValue* v) { return v && !(v->kind == TomlValue::ARR && v->arr.empty()); };
         if (given(ids) || given(comps) || given(vals))
            throw std::runtime_error("BCs.periodic = true: the faces cannot be both periodic and prescribed (leave essential_ids, essential_comps and essential_vals out)");
         if (!vgr) throw std::runtime_error("BCs.periodic = true needs the macroscopic velocity gradient BCs.essential_vel_grad (3 x 3)");
      } else if (!ids || !comps) throw std::runtime_error("BCs.essential_ids / essential_comps are required");
      if (const TomlValue* vo = d.get("BCs.vgrad_origin")) {
         if (!vo->arr.empty()) { if (vo->arr.size() != 3) throw std::runtime_error("BCs.vgrad_origin when provided must contain 3 components."); vgrad_origin_flag = true; for (int k = 0; k < 3; k++) vgrad_origin[k] = vo->arr[k].num; }
      }
      auto flat = [](const TomlValue& a) { std::vector<double> o; for (auto& e : a.arr) o.push_back(e.num); return o; };
      auto fill_vgrad = [](const TomlValue* m, BCEntry& e) {   // [[a,b,c],[d,e,f],[g,h,i]] flattened row by row
         if (!m) return; int k = 0;
         for (auto& row : m->arr) for (auto& x : row.arr) { if (k < 9) e.vgrad[k] = x.num; k++; }
         if (k != 0 && k != 9) throw std::runtime_error("BCs.essential_vel_grad must be a 3 x 3 array");
      };
      auto full_vgrad = [](const TomlValue& m) {   // periodic: exactly 3 rows of 3 numbers
         if (m.kind != TomlValue::ARR || m.arr.size() != 3) return false;
         for (auto& row : m.arr) { if (row.kind != TomlValue::ARR || row.arr.size() != 3) return false; for (auto& x : row.arr) if (x.kind != TomlValue::NUM) return false; }
         return true;
      };
      if (changing) {
         const TomlValue* us = d.get("BCs.update_steps"); if (!us) throw std::runtime_error("BCs.update_steps was not provided any values.");
         bool has1 = false; for (auto& u : us->arr) has1 = has1 || (int)u.num == 1;
         if (!has1) throw std::runtime_error("BCs.update_steps must contain 1 in the array");
         if (periodic && (vgr->kind != TomlValue::ARR || vgr->arr.size() != us->arr.size())) throw std::runtime_error("BCs.periodic = true: essential_vel_grad must hold one 3 x 3 array per update step");
         if (!periodic && ids->arr.size() != us->arr.size()) throw std::runtime_error("BCs.essential_ids did not contain the same number of arrays as number of update steps");
         if (!periodic && comps->arr.size() != us->arr.size()) throw std::runtime_error("BCs.essential_comps did not contain the same number of arrays as number of update steps");
         for (size_t b = 0; b < us->arr.size(); b++) {
            BCEntry e; e.step = (int)us->arr[b].num;
            if (periodic) {
               if (!full_vgrad(vgr->arr[b])) throw std::runtime_error("BCs.periodic = true: essential_vel_grad must hold one 3 x 3 array per update step");
               fill_vgrad(&vgr->arr[b], e); bcs.push_back(e);
               continue;
            }
            for (double v : flat(ids->arr[b])) e.ids.push_back((int)v);
            for (double v : flat(comps->arr[b])) e.comps.push_back((int)v);
            if (vals && b < vals->arr.size()) e.vals = flat(vals->arr[b]);
            if (vgr && b < vgr->arr.size()) fill_vgrad(&vgr->arr[b], e);
            bcs.push_back(e);
         }
      } else if (periodic) {
         if (!full_vgrad(*vgr)) throw std::runtime_error("BCs.periodic = true: essential_vel_grad must be a 3 x 3 array");
         BCEntry e; e.step = 1; fill_vgrad(vgr, e); bcs.push_back(e);
      } else {
         BCEntry e; e.step = 1;
         for (double v : flat(*ids)) e.ids.push_back((int)v);
         for (double v : flat(*comps)) e.comps.push_back((int)v);
         if (vals) e.vals = flat(*vals);
         fill_vgrad(vgr, e); bcs.push_back(e);
      }
      for (auto& e : bcs) {
         if (e.comps.size() != e.ids.size()) throw std::runtime_error("BCs: essential_comps must hold one entry per essential id");
         bool need_vel = false, need_vg = false; for (int c : e.comps) { if (c > 0) need_vel = true; if (c < 0) need_vg = true; }
         if (e.vals.empty() && need_vel) throw std::runtime_error("BCs.essential_vals was not provided any values  but a boundary requires this.");
         if (!vgr && need_vg) throw std::runtime_error("BCs.essential_vel_grad was not provided any values but a boundary requires this.");
         if (e.vals.empty()) e.vals.assign(3 * e.ids.size(), 0.0);
         if (e.vals.size() != 3 * e.ids.size()) throw std::runtime_error("BCs: essential_vals must hold 3 values per essential id");
      }
      if (lower(d.str("Model.mech_type", "")) != "exacmech") throw std::runtime_error("Only mech_type = \"exacmech\" is supported (UMAT is CPU-only in the reference)");
      const std::string xt = lower(d.str("Model.ExaCMech.xtal_type", "")), st = lower(d.str("Model.ExaCMech.slip_type", ""));
      if (xt == "fcc") xtal = XtalType::FCC; else if (xt == "bcc") xtal = XtalType::BCC; else throw std::runtime_error("Unknown xtal_type: " + xt);
      if (st == "powervoce") slip = SlipType::POWERVOCE; else if (st == "powervocenl") slip = SlipType::POWERVOCENL; else if (st == "mtsdd") slip = SlipType::MTSDD; else throw std::runtime_error("Unknown slip_type: " + st);
      // time: Custom > Auto > Fixed (reference src/mechanics_driver.cpp:842-851)
      if (d.has_table("Time.Custom")) {
         dt_cust = true; nsteps = (int)d.num("Time.Custom.nsteps", 1);
         cust_dt = load_numbers(resolve(d.str("Time.Custom.floc", "custom_dt.txt")));
         if ((int)cust_dt.size() < nsteps) throw std::runtime_error("Custom dt file has fewer entries than nsteps");
      } else if (d.has_table("Time.Auto")) {
         dt_auto = true; dt = d.num("Time.Auto.dt_start", 1.0); dt_min = d.num("Time.Auto.dt_min", 1.0); dt_scale = d.num("Time.Auto.dt_scale", 0.25); t_final = d.num("Time.Auto.t_final", 1.0);
         auto_dt_fname = d.str("Time.Auto.auto_dt_file", "auto_dt_out.txt");
         if (changing) throw std::runtime_error("Automatic time stepping is currently not compatible with changing boundary conditions");   // src/option_parser.cpp:509-511
         if (dt_scale < 0.0 || dt_scale > 1.0) throw std::runtime_error("dt_scale for auto time stepping needs to be between 0 and 1.");
         nsteps = (int)std::ceil(t_final / dt_min);   // reference src/mechanics_driver.cpp:212
      } else { dt = d.num("Time.Fixed.dt", 1.0); t_final = d.num("Time.Fixed.t_final", 1.0); nsteps = (int)std::ceil(t_final / dt - 1e-9); }
      avg_stress_fname = d.str("Visualizations.avg_stress_fname", "avg_stress.txt");
      additional_avgs = d.boolean("Visualizations.additional_avgs", false);
      paraview = d.boolean("Visualizations.paraview", false); light_up = d.boolean("Visualizations.light_up", false);
      vis_steps = (int)d.num("Visualizations.steps", 1); vis_floc = d.str("Visualizations.floc", "results/exaconstit");
      if (vis_steps < 1) throw std::runtime_error("Visualizations.steps must be at least 1");
      if (const TomlValue* h = d.get("Visualizations.light_up_hkl")) {
         if (h->kind != TomlValue::ARR || h->arr.empty()) throw std::runtime_error("Visualizations.light_up_hkl must be an array of [h, k, l] triples");
         if (h->arr.size() > 16) throw std::runtime_error("Visualizations.light_up_hkl holds at most 16 triples");
         for (auto& t : h->arr) {
            if (t.kind != TomlValue::ARR || t.arr.size() != 3) throw std::runtime_error("Visualizations.light_up_hkl: every entry must be an [h, k, l] triple of 3 integers");
            for (auto& x : t.arr) {
               if (x.kind != TomlValue::NUM || x.num != std::floor(x.num) || std::fabs(x.num) > 1000.0) throw std::runtime_error("Visualizations.light_up_hkl: Miller indices must be integers");
               lightup_hkl.push_back((int)x.num);
            }
         }
      }
      if (const TomlValue* sd = d.get("Visualizations.light_up_s_dir")) {
         if (sd->kind != TomlValue::ARR || sd->arr.size() != 3) throw std::runtime_error("Visualizations.light_up_s_dir must contain 3 components");
         for (int i = 0; i < 3; i++) lightup_s_dir[i] = sd->arr[i].num;
      }
      lightup_tol_deg = d.num("Visualizations.light_up_dist_tol_deg", 5.0);
      lightup_strain_fname = d.str("Visualizations.light_up_strain_fname", "lattice_strains.txt");
      lightup_volume_fname = d.str("Visualizations.light_up_volume_fname", "lattice_volumes.txt");
      check_lightup(lightup_hkl, lightup_s_dir, lightup_tol_deg);
      if (const TomlValue* g = d.get("Visualizations.grain_avgs")) {
         if (g->kind != TomlValue::BOOL) throw std::runtime_error("Visualizations.grain_avgs must be true or false");
         grain_avgs = g->b;
      }
      if (const TomlValue* g = d.get("Visualizations.grain_avgs_fname")) {
         if (g->kind != TomlValue::STR || g->str.empty() || g->str.find('/') != std::string::npos)
            throw std::runtime_error("Visualizations.grain_avgs_fname must be a non-empty file name without '/'");
         grain_avgs_fname = g->str;
      }
      if (const TomlValue* t = d.get("Visualizations.texture")) {
         if (t->kind != TomlValue::BOOL) throw std::runtime_error("Visualizations.texture must be true or false");
         texture = t->b;
      }
      if (const TomlValue* h = d.get("Visualizations.texture_hkl")) {
         if (h->kind != TomlValue::ARR || h->arr.empty() || h->arr.size() > 16) throw std::runtime_error("Visualizations.texture_hkl must be an array of 1 to 16 [h, k, l] triples");
         texture_hkl.clear();
         for (auto& t : h->arr) {
            if (t.kind != TomlValue::ARR || t.arr.size() != 3) throw std::runtime_error("Visualizations.texture_hkl: every entry must be an [h, k, l] triple of 3 integers");
            for (auto& x : t.arr) {
               if (x.kind != TomlValue::NUM || x.num != std::floor(x.num) || std::fabs(x.num) > 1000.0) throw std::runtime_error("Visualizations.texture_hkl: Miller indices must be integers");
               texture_hkl.push_back((int)x.num);
            }
         }
      }
      if (const TomlValue* v = d.get("Visualizations.texture_ipf_dirs")) {
         if (v->kind != TomlValue::ARR || v->arr.size() > 3) throw std::runtime_error("Visualizations.texture_ipf_dirs must be an array of 0 to 3 directions [x, y, z]");
         texture_dirs.clear();
         for (auto& t : v->arr) {
            if (t.kind != TomlValue::ARR || t.arr.size() != 3) throw std::runtime_error("Visualizations.texture_ipf_dirs: every entry must be a direction of 3 numbers");
            for (auto& x : t.arr) {
               if (x.kind != TomlValue::NUM) throw std::runtime_error("Visualizations.texture_ipf_dirs: every entry must be a direction of 3 numbers");
               texture_dirs.push_back(x.num);
            }
         }
      }
      if (const TomlValue* r = d.get("Visualizations.texture_res_deg")) {
         if (r->kind != TomlValue::NUM) throw std::runtime_error("Visualizations.texture_res_deg must be a number of degrees");
         texture_res_deg = r->num;
      }
      if (const TomlValue* f = d.get("Visualizations.texture_fname")) {
         if (f->kind != TomlValue::STR || f->str.empty() || f->str.find('/') != std::string::npos)
            throw std::runtime_error("Visualizations.texture_fname must be a non-empty file name without '/'");
         texture_fname = f->str;
      }
      check_texture(texture_hkl, texture_dirs, texture_res_deg);
      if (const TomlValue* t = d.get("Visualizations.macro_tangent")) {
         if (t->kind != TomlValue::BOOL) throw std::runtime_error("Visualizations.macro_tangent must be true or false");
         macro_tangent = t->b;
      }
      if (const TomlValue* f = d.get("Visualizations.macro_tangent_fname")) {
         if (f->kind != TomlValue::STR || f->str.empty() || f->str.find('/') != std::string::npos)
            throw std::runtime_error("Visualizations.macro_tangent_fname must be a non-empty file name without '/'");
         macro_tangent_fname = f->str;
      }
      if (const TomlValue* t = d.get("Visualizations.lattice_curvature")) {
         if (t->kind != TomlValue::BOOL) throw std::runtime_error("Visualizations.lattice_curvature must be true or false");
         lattice_curvature = t->b;
      }
      if (const TomlValue* b = d.get("Visualizations.lattice_curvature_burgers")) {
         if (b->kind != TomlValue::NUM || !(b->num > 0.0) || !std::isfinite(b->num)) throw std::runtime_error("Visualizations.lattice_curvature_burgers must be a number > 0");
         lattice_curvature_burgers = b->num;
      }
      if (const TomlValue* f = d.get("Visualizations.lattice_curvature_fname")) {
         if (f->kind != TomlValue::STR || f->str.empty() || f->str.find('/') != std::string::npos)
            throw std::runtime_error("Visualizations.lattice_curvature_fname must be a non-empty file name without '/'");
         lattice_curvature_fname = f->str;
      }
      if (const TomlValue* t = d.get("Visualizations.fatigue")) {
         if (t->kind != TomlValue::BOOL) throw std::runtime_error("Visualizations.fatigue must be true or false");
         fatigue = t->b;
      }
      if (const TomlValue* k = d.get("Visualizations.fatigue_k")) {
         if (k->kind != TomlValue::NUM || !(k->num >= 0.0) || !std::isfinite(k->num)) throw std::runtime_error("Visualizations.fatigue_k must be a number >= 0");
         fatigue_k = k->num;
      }
      if (const TomlValue* y = d.get("Visualizations.fatigue_sigma_y")) {
         if (y->kind != TomlValue::NUM || !(y->num > 0.0) || !std::isfinite(y->num)) throw std::runtime_error("Visualizations.fatigue_sigma_y must be a number > 0");
         fatigue_sigma_y = y->num;
      } else if (fatigue) throw std::runtime_error("Visualizations.fatigue = true needs Visualizations.fatigue_sigma_y (the yield stress in the stress unit of the run; no default is offered)");
      if (const TomlValue* v = d.get("Visualizations.fatigue_cycle_steps")) {
         if (v->kind != TomlValue::NUM || v->num != std::floor(v->num) || v->num < 0 || v->num > 1e9) throw std::runtime_error("Visualizations.fatigue_cycle_steps must be a whole number >= 0");
         fatigue_cycle_steps = (int)v->num;
      }
      if (const TomlValue* f = d.get("Visualizations.fatigue_fname")) {
         if (f->kind != TomlValue::STR || f->str.empty() || f->str.find('/') != std::string::npos)
            throw std::runtime_error("Visualizations.fatigue_fname must be a non-empty file name without '/'");
         fatigue_fname = f->str;
      }
      if (const TomlValue* r = d.get("Visualizations.macro_tangent_rel_tol")) {
         if (r->kind != TomlValue::NUM || !(r->num > 0.0) || !(r->num < 1.0)) throw std::runtime_error("Visualizations.macro_tangent_rel_tol must be a number in (0, 1)");
         macro_tangent_rel_tol = r->num;
      }
      if (const TomlValue* v = d.get("Visualizations.macro_tangent_max_iter")) {
         if (v->kind != TomlValue::NUM || v->num != std::floor(v->num) || v->num < 1 || v->num > 1e9) throw std::runtime_error("Visualizations.macro_tangent_max_iter must be a whole number of at least 1");
         macro_tangent_max_iter = (int)v->num;
      }
      if (const TomlValue* w = d.get("Checkpoint.write")) {
         if (w->kind != TomlValue::BOOL) throw std::runtime_error("Checkpoint.write must be true or false");
         ckpt_write = w->b;
      }
      if (const TomlValue* v = d.get("Checkpoint.steps")) {
         if (v->kind != TomlValue::NUM || v->num != std::floor(v->num) || v->num < 1 || v->num > 1e9) throw std::runtime_error("Checkpoint.steps must be a whole number of at least 1");
         ckpt_steps = (int)v->num;
      }
      if (const TomlValue* v = d.get("Checkpoint.keep")) {
         if (v->kind != TomlValue::NUM || v->num != std::floor(v->num) || v->num < 1 || v->num > 1e6) throw std::runtime_error("Checkpoint.keep must be a whole number of at least 1");
         ckpt_keep = (int)v->num;
      }
      if (const TomlValue* v = d.get("Checkpoint.floc")) {
         if (v->kind != TomlValue::STR || v->str.empty() || v->str.find('/') != std::string::npos) throw std::runtime_error("Checkpoint.floc must be a non-empty file name without '/'");
         ckpt_floc = v->str;
      }
      if (const TomlValue* v = d.get("Checkpoint.restart_from")) {
         if (v->kind != TomlValue::STR || v->str.empty()) throw std::runtime_error("Checkpoint.restart_from must be a non-empty path");
         ckpt_restart_from = v->str;
      }
      avg_def_grad_fname = d.str("Visualizations.avg_def_grad_fname", "avg_def_grad.txt");
      avg_pl_work_fname = d.str("Visualizations.avg_pl_work_fname", "avg_pl_work.txt");
      avg_dp_tensor_fname = d.str("Visualizations.avg_dp_tensor_fname", "avg_dp_tensor.txt");
      const std::string as = lower(d.str("Solvers.assembly", "FULL"));
      if (as == "pa") assembly = Assembly::PA; else if (as == "ea" || as == "full") assembly = Assembly::EA; else throw std::runtime_error("Unknown assembly: " + as);
      integ_model = d.str("Solvers.integ_model", "FULL");
      if (lower(integ_model) != "full" && lower(integ_model) != "bbar") throw std::runtime_error("Solvers.integ_model was not provided a valid type.");
      if (lower(integ_model) == "bbar" && assembly == Assembly::PA) throw std::runtime_error("integ_model = \"BBAR\" has no partial-assembly gradient (use EA or FULL), as in the reference");
      newton_iter = (int)d.num("Solvers.NR.iter", 25); newton_rel = d.num("Solvers.NR.rel_tol", 1e-5); newton_abs = d.num("Solvers.NR.abs_tol", 1e-10);
      { const std::string nl = lower(d.str("Solvers.NR.nl_solver", "NR"));   // reference src/option_parser.cpp:616-627 aborts on anything else
        if (nl == "nr") nl_solver = NLSolver::NR; else if (nl == "nrls") nl_solver = NLSolver::NRLS;
        else throw std::runtime_error("Solvers.NR.nl_solver was not provided a valid type."); }
      krylov_iter = (int)d.num("Solvers.Krylov.iter", 200); krylov_rel = d.num("Solvers.Krylov.rel_tol", 1e-10); krylov_abs = d.num("Solvers.Krylov.abs_tol", 1e-30);
      // reference src/option_parser.cpp:647-662: GMRES (its default), PCG or MINRES, anything else aborts.  PCG and GMRES are built here, and GMRES
      // is what the operator calls for: the plastic tangent is not symmetric (DESIGN 4.6 measures |A - A^T| / |A| = 1.9e-4).  GMRES is opt-in
      // through Solvers.Krylov.gmres_kdim (the Krylov dimension, MFEM's default is 50): a file that asks for - or defaults to - GMRES without it,
      // or for MINRES, is refused instead of silently running CG.
      krylov_solver = lower(d.str("Solvers.Krylov.solver", "GMRES"));
      const TomlValue* kd = d.get("Solvers.Krylov.gmres_kdim");
      if (kd) {
         if (kd->kind != TomlValue::NUM || kd->num != std::floor(kd->num) || kd->num < 1 || kd->num > 100) throw std::runtime_error(gmres_kdim_range());
         if (krylov_solver == "pcg") throw std::runtime_error("Solvers.Krylov.gmres_kdim stands next to solver = \"GMRES\" (or no solver key: the reference's default), not next to solver = \"PCG\"");
         gmres_kdim = (int)kd->num;
      }
      if (krylov_solver == "minres" || (krylov_solver == "gmres" && !kd))
         throw std::runtime_error("Solvers.Krylov.solver = \"" + krylov_solver + "\" (the reference's default is GMRES) is not built in this driver: set Solvers.Krylov.solver = \"PCG\""
                                  + (krylov_solver == "gmres" ? ", or add Solvers.Krylov.gmres_kdim = <1 ... 100> (MFEM's default is 50) to run GMRES" : ""));
      if (krylov_solver != "pcg" && krylov_solver != "gmres") throw std::runtime_error("Solvers.Krylov.solver was not provided a valid type.");
      ref_ser = (int)d.num("Mesh.ref_ser", 0); order = (int)d.num("Mesh.p_refinement", 1);   // tests write "prefinement": ignored like the reference (src/option_parser.cpp:677)
      mesh_type = lower(d.str("Mesh.type", "other"));
      mesh_file = d.str("Mesh.floc", "");
      if (mesh_type == "other" || mesh_type == "cubit") {   // file mesh (reference src/mechanics_driver.cpp:239-241); MFEM mesh v1.0 hexahedra only
         if (mesh_file.empty()) throw std::runtime_error("Mesh.floc is required for Mesh.type = \"other\"");
         if (ref_ser != 0) throw std::runtime_error("Mesh.ref_ser > 0 is only built for auto-generated meshes");
         if (order < 1 || order > 6) throw std::runtime_error("File meshes run at p_refinement = 1 ... 6");
      } else if (mesh_type == "auto") {
         const TomlValue* nc = d.get("Mesh.Auto.ncuts"); const TomlValue* ln = d.get("Mesh.Auto.length");
         if (!nc || !ln || nc->arr.size() != 3 || ln->arr.size() != 3) throw std::runtime_error("Must input mesh geometry/discretization for hex_mesh_gen");
         for (int i = 0; i < 3; i++) { ncuts[i] = (int)nc->arr[i].num; length[i] = ln->arr[i].num; }
      } else throw std::runtime_error("Mesh.type must be \"auto\", \"other\" or \"cubit\"");
      if (order < 1 || order > 6) throw std::runtime_error("p_refinement must be between 1 and 6");
      if (periodic && mesh_type != "auto") throw std::runtime_error(periodic_needs_generated_mesh());
      if (macro_tangent && !periodic) throw std::runtime_error(macro_tangent_needs_periodic());
      if (const TomlValue* pc = d.get("Solvers.Krylov.preconditioner")) {
         const std::string k = pc->kind == TomlValue::STR ? lower(pc->str) : std::string("?");
         if (k == "jacobi") precond = 1;
         else if (k == "multigrid") {
            precond = 2;
            const double lv = d.num("Solvers.Krylov.mg_levels", 0.0), dg = d.num("Solvers.Krylov.mg_smoother_degree", 2.0);
            if (lv < 0 || lv != std::floor(lv) || lv > 30) throw std::runtime_error("Solvers.Krylov.mg_levels must be a whole number >= 0 (0: as many levels as the mesh allows)");
            if (dg < 1 || dg > 8 || dg != std::floor(dg)) throw std::runtime_error("Solvers.Krylov.mg_smoother_degree must be a whole number in 1 ... 8");
            mg_levels = (int)lv; mg_degree = (int)dg;
            if (const TomlValue* m2 = d.get("Solvers.Krylov.mg_p2")) {
               if (m2->kind != TomlValue::BOOL) throw std::runtime_error("Solvers.Krylov.mg_p2 must be true or false");
               mg_p2 = m2->b;
            }
            if (const TomlValue* mb = d.get("Solvers.Krylov.mg_bbar")) {
               if (mb->kind != TomlValue::BOOL) throw std::runtime_error("Solvers.Krylov.mg_bbar must be true or false");
               mg_bbar = mb->b;
            }
            if (order != 1 && !mg_p2) throw std::runtime_error(mg_order_refusal());
            if (order > 2) throw std::runtime_error(mg_p2_no_higher_order());
            if (order == 2 && periodic) throw std::runtime_error(mg_p2_no_periodic());
            if (lower(integ_model) == "bbar" && !mg_bbar) throw std::runtime_error(mg_no_bbar());
            if (lower(integ_model) == "bbar" && periodic) throw std::runtime_error(mg_bbar_no_periodic());
            if (mesh_type != "auto") throw std::runtime_error("Solvers.Krylov.preconditioner = \"multigrid\" needs a generated mesh (Mesh.type = \"auto\"): file meshes need algebraic coarsening");
            if (const TomlValue* mp = d.get("Solvers.Krylov.mg_periodic")) {
               if (mp->kind != TomlValue::BOOL) throw std::runtime_error("Solvers.Krylov.mg_periodic must be true or false");
               mg_periodic = mp->b;
            }
            if (periodic && !mg_periodic) throw std::runtime_error(periodic_no_multigrid());
         } else throw std::runtime_error("Solvers.Krylov.preconditioner must be \"jacobi\" or \"multigrid\"");
      }
   }
};

}  // namespace exa_host
