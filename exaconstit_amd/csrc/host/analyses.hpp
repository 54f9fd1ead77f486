// In-situ analyses of a run: everything that is computed from the per-element rows of exa_element_fields - the ParaView save, light-up
// lattice strains (4.5), per-grain averages (4.7), texture (4.8), lattice curvature (4.14), slip activity / FIP (4.15) - with their device buffers,
// their output schedule and what a checkpoint carries of them.  SystemDriver owns one StepAnalyses (SystemDriver::analyses(), as it owns the PCG)
// and calls it at three points of a step; the object reads the operator's state and never writes it.
#pragma once
#include <map>
#include <string>
#include <vector>
#include "../../../include/exaconstit_hip.h"
#include "device_utils.hpp"
#include "mesh.hpp"
#include "options.hpp"

namespace exa_host {

class NonlinearMechOperator;
class Comm;

void append_row(const std::string& path, const double* v, int n);   // one row of an avg_* / light-up file, as mfem::Vector::Print(out, width = n)
// per-grain averages: value columns per grain (after the grain id) of StepAnalyses::GrainAverages and the grain_avgs files
constexpr int GRAIN_NVALS = 45;
// one grain_avgs file: a '#' header naming the 46 columns, then one row per grain (id, element count, 43 values with 17 significant digits)
void write_grain_avgs(const std::string& path, int n, const int32_t* ids, const double* vals);
// one texture file: a '# texture step .. time .. res_deg .. n_alpha .. n_beta ..' header, then per set a '# pole figure {h k l}' or
// '# inverse pole figure [d0 d1 d2]' line and n_alpha rows of n_beta MRD values (17 significant digits); mrd [nhkl + ndir][n_alpha][n_beta]
void write_texture(const std::string& path, int step, double t, double res_deg, const std::vector<int>& hkl, const std::vector<double>& dirs,
                   const std::vector<double>& mrd);
constexpr int FATIGUE_NSUMMARY = 8, FATIGUE_ROW = 9;   // SlipActivityResult::summary; row of the fatigue file: step, time, window start, mean FIP, max FIP, element, mean and max AccumulatedSlip, max ShearRange
void write_fatigue_rows(const std::string& path, const std::vector<double>& rows, bool append);   // append = false: the file anew, header first
void write_fatigue_grains(const std::string& path, int n, const int32_t* ids, const double* vals3);

// where the run stands when an analysis is asked for (SystemDriver::state()): committed steps, time, the size the last step was solved with (under
// Time.Auto after any cut-back), where files go and whether any are written, the velocity (ParaView save)
struct StepState { int step; double time, dt; const std::string& out_dir; bool write_files; const DevBuf<double>& vel; };

class StepAnalyses {
 public:
   // elem_attr: grain id of every local element (the driver's; SetGrains rewrites it and calls GrainsChanged); grain_qref: unit reference orientation
   // of every grain, [grain id - 1][4]
   StepAnalyses(NonlinearMechOperator& op, Comm& comm, const Partition& part, const ExaOptions& opt, const std::vector<int32_t>& elem_attr, std::vector<double> grain_qref);
   StepAnalyses(const StepAnalyses&) = delete; StepAnalyses& operator=(const StepAnalyses&) = delete;

   // The one answer to "are the rows current?" (DESIGN 4.4).  rows(): the device rows [E][EXA_NFIELDS] of the begin-of-step state - after a committed
   // step the converged one - and the current coordinates; exa_element_fields is launched only when the stamp of the last launch (committed steps,
   // constitutive launches, size) is not that of the state at hand.  Whoever replaces or rewrites stress0, matVars0 or x_cur outside a constitutive
   // launch or a commit calls Invalidate (SetGrains, LoadCheckpoint, the benchmark's state preparation).
   const double* rows(const StepState& at) { if (!(fields_step_ == at.step && fields_calls_ == model_calls() && fields_dev_.n == (size_t)EXA_NFIELDS * part_.E)) ComputeElementFields(at); return fields_dev_.p; }
   void Invalidate() { fields_step_ = -1; }
   int64_t field_launches = 0;                 // launches of exa_element_fields so far (Driver.diagnostics)
   // per-element output fields (reference SystemDriver::Project*, src/system_driver.cpp:560-870): the rows on the host, in local element order.  Always launches.
   void ElementFields(const StepState& at, std::vector<double>& out);
   // ParaView save of the rows as cycle `cycle` at time t under dir (host/vtu.hpp); every rank calls it.  With Visualizations.lattice_curvature /
   // fatigue on, the curvature rows and the slip-activity evaluation of this state are computed here
   void SaveFields(const StepState& at, const std::string& dir, int cycle, double t);
   // lattice strains of the {hkl} families (3 integers each; options.hpp check_lightup) of the same state, summed over all ranks (every rank calls
   // it): strain[j] = volume-weighted mean of s^T eps s over the elements of fibre j (NaN when the fibre is empty), volfrac[j] = its volume fraction
   void LatticeStrains(const StepState& at, const std::vector<int>& hkl, const double s_dir[3], double tol_deg, double* strain, double* volfrac);
   // per-grain averages of the same state over all ranks (every rank calls it): ids = the ascending 1-based ids of the grains with
   // elements, vals = GRAIN_NVALS values per grain (the value columns of the grain_avgs files, write_grain_avgs)
   void GrainAverages(const StepState& at, std::vector<int32_t>& ids, std::vector<double>& vals);
   // intragranular misorientation and lattice curvature of the same state (every rank calls it): rows = [E][EXA_NCURV] of the local
   // elements (exa_curvature_elements; burgers: Burgers vector length in the mesh's length unit), summary7 = over all ranks the volume-weighted
   // means of GROD, KAM and the GND density, their maxima and the total volume: { mean GROD, max GROD, mean KAM, max KAM, mean GND, max GND, V }
   // want_rows = false: the summary alone (rows is left empty and the [E][EXA_NCURV] copy to the host is skipped)
   void LatticeCurvature(const StepState& at, double burgers, std::vector<double>& rows, double* summary7, bool want_rows = true);
   // texture of the same state over all ranks (every rank calls it): pole figures of the {hkl} families (3 integers each) and
   // inverse pole figures of the sample directions dirs (3 components each, normalised here; options.hpp check_texture) on the grid of
   // res_deg; mrd = [nhkl + ndir][n_alpha][n_beta] multiples of random distribution, the same bits on every rank and for any rank count
   void PoleFigures(const StepState& at, const std::vector<int>& hkl, std::vector<double> dirs, double res_deg, std::vector<double>& mrd);
   // Slip-system activity and the Fatemi-Socie fatigue indicator parameter.  With the feature on (Visualizations.fatigue, or
   // EnableSlipActivity before the first step) Committed adds the committed step to the 60 accumulators of every element, from the rows of one
   // launch that the step's other analyses share.  A window reset is a request: it is carried out, fused into the accumulate launch, at the end
   // of the next committed step, whose values start the new window (before step 1 the window is the initial state already).
   struct SlipActivityResult {
      std::vector<double> acc, fip;            // [E][EXA_NSLIPACC] (Gamma | A | Gamma_min | Gamma_max | N_max, 12 each) and [E][EXA_NFIP] of the local elements
      double summary[FATIGUE_NSUMMARY];        // over all ranks: volume, mean FIP, max FIP, global element of the max, mean and max AccumulatedSlip, max ShearRange, window start step
      std::vector<int32_t> grain_ids; std::vector<double> grain_vals;   // over all ranks, ascending ids of the grains with elements: volume, mean FIP, max FIP
   };
   void EnableSlipActivity();
   bool slip_activity_on() const { return fatigue_on_; }
   // evaluation of the committed state, read-only on the accumulators (every rank calls it); want_acc = false: res.acc is left empty
   void SlipActivity(const StepState& at, double k_fs, double sigma_y, SlipActivityResult& res, bool want_acc = true);
   void ResetFatigueWindow(const StepState& at);
   // the grain map (elem_attr) and the reference orientations have changed, and with them the state
   void GrainsChanged(std::vector<double> grain_qref);
   std::string vis_dir(const StepState& at) const { return (opt_.vis_floc.empty() || opt_.vis_floc[0] == '/') ? opt_.vis_floc : at.out_dir + "/" + opt_.vis_floc; }

   // ---- the three calls of a step (SystemDriver::Step, CommitStep)
   // top of every Step: starts the accumulators; with commit, ParaView cycle 0 and the texture file of step 0 - the initial state, written once
   void BeforeFirstStep(const StepState& at, bool commit);
   void Committed(const StepState& at);        // CommitStep: the accumulate hook
   // after the commit of step ti: the output schedule (Visualizations.steps, the last step, fatigue_cycle_steps; one light-up row per step).  Returns
   // whether the step is on the Visualizations.steps cadence: the macroscopic tangent, which is the driver's, is written on it
   bool AfterCommit(const StepState& at, int ti);

   // ---- what a checkpoint carries (host/checkpoint.hip reads and writes this, the accumulators below, and nothing else)
   struct Checkpointed {
      bool cycle0_saved = false, texture0_written = false;
      std::vector<double> lattice_rows, volume_rows;   // light-up rows, which exist only in append-mode files otherwise
      std::vector<double> fatigue_rows;                // FATIGUE_ROW values per written evaluation
      int64_t fatigue_window_start = 0; bool fatigue_pending = false;   // first step of the window; reset requested
      std::map<std::string, std::vector<std::pair<int, double>>> pvd_cycles;   // saved cycles of each output directory (rank 0 writes the .pvd)
   } ckpt;
   const DevBuf<double>& SlipAccumulators(const StepState& at) { EnsureFatigueInit(at); return fat_acc_; }   // planar [EXA_NSLIPACC][E_pad], started if need be
   // a checkpoint has replaced the state (and ckpt); slip_planar (nullable): the accumulators that came with it
   void Restored(const std::vector<double>* slip_planar);
 private:
   long model_calls() const;
   void ComputeElementFields(const StepState& at);
   void EnsureGrainPlan();
   // pass 1 of exa_grain_sums on the rows, all-reduced: h = [G][EXA_GRAIN_NSUMS], qbar = the unit grain means (the reference orientation of a grain
   // without elements), vtot = the volume of all grains
   void GrainMeans(const double* rows, std::vector<double>& h, std::vector<double>& qbar, double& vtot);
   void EnsureFatigueInit(const StepState& at);
   void SaveCycle(const StepState& at, const std::string& dir, int cycle, double t, const std::vector<double>& curv, const SlipActivityResult& fat);
   void WriteLatticeCurvature(const StepState& at, int step, const double* summary7);
   void WriteTexture(const StepState& at, int step);
   // one row of Visualizations.fatigue_fname and the per-grain file of this step, from an evaluation with the options' k and sigma_y
   void WriteFatigue(const StepState& at, int step, const SlipActivityResult& res);

   NonlinearMechOperator& op_; Comm& comm_; const Partition& part_; const ExaOptions& opt_; const std::vector<int32_t>& elem_attr_;
   bool started_ = false, restored_ = false;    // a Step has begun; a checkpoint was loaded
   int fields_step_ = -1; long fields_calls_ = -1;   // the stamp: committed steps and constitutive launches at which fields_dev_ was last filled
   DevBuf<double> fields_dev_, lattice_sums_;   // [E][EXA_NFIELDS] element rows; 2 H + 1 lattice-strain sums
   std::vector<double> grain_qref_;
   // plan of exa_grain_sums for elem_attr (built on first use, dropped by GrainsChanged), its device copy and workspace; G = largest grain id over all ranks
   std::vector<int32_t> grain_plan_; DevBuf<int32_t> grain_plan_dev_, grain_attr_dev_; DevBuf<double> grain_work_, grain_sums_, grain_quat_dev_; int grain_G_ = 0;
   DevBuf<double> curv_work_, curv_nodal_, curv_rows_, curv_sum_, curv_xe_;   // LatticeCurvature: records, nodal planes, rows, 7 sums, current coordinates as an E-vector
   DevBuf<double> texture_vmax_; DevBuf<int64_t> texture_counts_;   // largest element volume; [set][n_alpha][n_beta] counts of exa_texture_weights
   // slip activity: on / accumulators initialised; planar accumulators, FIP rows, 7 sums (+ per-grain sums), global element ids on the device; unit plane normals of the model
   bool fatigue_on_ = false, fatigue_init_ = false;
   DevBuf<double> fat_acc_, fat_rows_, fat_sum_, fat_grain_; DevBuf<int64_t> fat_gid_; double fat_normals_[36];
};

}  // namespace exa_host
