// ParaView output of the per-element fields (reference: mfem::ParaViewDataCollection behind Visualizations.paraview, src/mechanics_driver.cpp:640-700,
// 911-955), written without a VTK library:
//   <floc>/Cycle%06d/proc%06d.vtu     one VTK XML UnstructuredGrid piece per rank (inline base64 "binary" arrays, UInt32 headers)
//   <floc>/Cycle%06d/data.pvtu        the parallel file naming every rank's piece (rank 0)
//   <floc>/<basename(floc)>.pvd       the collection, one DataSet per saved cycle with its time (rank 0, rewritten on every save)
// Cells: one VTK_HEXAHEDRON per element over its 8 vertex nodes at every order (the reference refines an order-p element into p^3 sub-cells;
// the cell values are element averages either way).  Pieces are in the driver's local element order; GlobalElementId maps them back.
// Arrays are streamed to the file value by value through a small base64 encoder: no piece is ever assembled in memory as text.
#pragma once
#include <sys/stat.h>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "../../../include/exaconstit_hip.h"

namespace exa_host {
namespace vtu {

// base64 of a byte stream, 3 bytes -> 4 characters, flushed with padding at the end of each encoded block
class B64 {
 public:
   explicit B64(std::ostream& o) : o_(o) {}
   void put(const void* p, size_t n) {
      const unsigned char* b = static_cast<const unsigned char*>(p);
      for (size_t i = 0; i < n; i++) { c_[k_++] = b[i]; if (k_ == 3) emit(3); }
   }
   void finish() { if (k_) emit(k_); o_.write(buf_.data(), (std::streamsize)buf_.size()); buf_.clear(); }
 private:
   void emit(int k) {
      static const char* T = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
      if (k < 3) std::memset(c_ + k, 0, 3 - k);
      char s[4] = { T[c_[0] >> 2], T[((c_[0] & 3) << 4) | (c_[1] >> 4)], k > 1 ? T[((c_[1] & 15) << 2) | (c_[2] >> 6)] : '=', k > 2 ? T[c_[2] & 63] : '=' };
      buf_.append(s, 4); k_ = 0;
      if (buf_.size() >= 1 << 16) { o_.write(buf_.data(), (std::streamsize)buf_.size()); buf_.clear(); }
   }
   std::ostream& o_; unsigned char c_[3]; int k_ = 0; std::string buf_;
};

inline bool is_little() { const uint16_t one = 1; unsigned char b; std::memcpy(&b, &one, 1); return b == 1; }

enum class T { F64, I32, I64, U8 };
inline const char* type_name(T t) { return t == T::F64 ? "Float64" : (t == T::I32 ? "Int32" : (t == T::I64 ? "Int64" : "UInt8")); }
inline size_t type_size(T t) { return t == T::F64 ? 8 : (t == T::I32 ? 4 : (t == T::I64 ? 8 : 1)); }

// an array read in place: tuple i, component c at base + i * tstride + c * cstride (bytes), values of type `type`
struct Array {
   std::string name; T type; int ncomp; const void* base; int64_t tstride, cstride;
};

inline void write_array(std::ostream& o, const Array& a, int64_t ntuples) {
   o << "        <DataArray type=\"" << type_name(a.type) << "\" Name=\"" << a.name << "\"";
   if (a.ncomp > 1) o << " NumberOfComponents=\"" << a.ncomp << "\"";
   o << " format=\"binary\">\n";
   const size_t vs = type_size(a.type);
   const uint32_t bytes = (uint32_t)(vs * a.ncomp * ntuples);
   if ((uint64_t)vs * a.ncomp * ntuples > 0xffffffffull) throw std::runtime_error("vtu: array " + a.name + " exceeds the 4 GB of a UInt32 header");
   { B64 h(o); h.put(&bytes, 4); h.finish(); }   // header and data are encoded as two blocks, like MFEM's and VTK's own writers
   B64 d(o);
   const char* b = static_cast<const char*>(a.base);
   for (int64_t i = 0; i < ntuples; i++)
      for (int c = 0; c < a.ncomp; c++) d.put(b + i * a.tstride + c * a.cstride, vs);
   d.finish();
   o << "\n        </DataArray>\n";
}

// host view of one rank's fields (everything host memory)
struct Piece {
   int64_t E = 0, NN = 0; int n = 8;
   bool tet = false;                                              // tetrahedra: VTK_TETRA over the first 4 nodes (the vertices, MFEM's order = VTK's)
   const int32_t* conn = nullptr;                                 // (n, E), native node order: the first 8 are the vertices in VTK_HEXAHEDRON order
   const double* x_cur = nullptr; const double* x_ref = nullptr;  // byNODES (NN, 3)
   const double* vel = nullptr;                                   // byNODES (NN, 3)
   const double* fields = nullptr;                                // [E][EXA_NFIELDS] (exa_element_fields)
   const int32_t* attr = nullptr; const int64_t* gid = nullptr;   // grain id (element attribute), global element index
   bool has_curv = false; const double* curv = nullptr;           // Visualizations.lattice_curvature: [E][EXA_NCURV] (exa_curvature_elements)
   bool has_fatigue = false; const double* fip = nullptr; const double* slip_acc = nullptr;   // Visualizations.fatigue: [E][EXA_NFIP] (exa_fip_rows), [E][EXA_NSLIPACC]
};

// the cell arrays of a save, in the order of the reference's RegisterField calls (ElemCentroid and XtalElasticStrain only with light_up)
inline std::vector<Array> cell_arrays(const Piece& p, bool light_up) {
   const int64_t rs = 8 * EXA_NFIELDS;
   auto col = [&](const char* nm, int c0, int nc) { return Array{ nm, T::F64, nc, p.fields + c0, rs, 8 }; };
   std::vector<Array> a = { col("ElementVolume", EXA_F_VOLUME, 1) };
   if (light_up) { a.push_back(col("ElemCentroid", EXA_F_CENTROID, 3)); a.push_back(col("XtalElasticStrain", EXA_F_XTALELASTICSTRAIN, 6)); }
   a.push_back(col("LatticeOrientation", EXA_F_ORIENTATION, 4));
   a.push_back(col("Stress", EXA_F_STRESS, 6));
   a.push_back(col("VonMisesStress", EXA_F_VONMISES, 1));
   a.push_back(col("HydrostaticStress", EXA_F_HYDROSTATIC, 1));
   a.push_back(col("DpEff", EXA_F_DPEFF, 1));
   a.push_back(col("EffPlasticStrain", EXA_F_EFFPLASTICSTRAIN, 1));
   a.push_back(col("ShearRate", EXA_F_SHEARRATE, 12));
   a.push_back(col("Hardness", EXA_F_HARDNESS, 1));
   a.push_back(Array{ "attribute", T::I32, 1, p.attr, 4, 0 });
   a.push_back(Array{ "GlobalElementId", T::I64, 1, p.gid, 8, 0 });
   if (p.has_curv) {
      auto ccol = [&](const char* nm, int c0, int nc) { return Array{ nm, T::F64, nc, p.curv + c0, 8 * EXA_NCURV, 8 }; };
      a.push_back(ccol("GROD", EXA_C_GROD, 1)); a.push_back(ccol("KAM", EXA_C_KAM, 1)); a.push_back(ccol("GNDDensity", EXA_C_GND, 1));
      a.push_back(ccol("LatticeCurvature", EXA_C_CURVATURE, 9));
   }
   if (p.has_fatigue) {
      auto fcol = [&](const char* nm, int c0) { return Array{ nm, T::F64, 1, p.fip + c0, 8 * EXA_NFIP, 8 }; };
      a.push_back(fcol("FIP", EXA_FIP_FIP)); a.push_back(fcol("ShearRange", EXA_FIP_SHEARRANGE)); a.push_back(fcol("AccumulatedSlip", EXA_FIP_ACCUMULATEDSLIP));
      a.push_back(Array{ "SlipAccumulated", T::F64, 12, p.slip_acc + EXA_ACC_SLIP, 8 * EXA_NSLIPACC, 8 });
   }
   return a;
}

inline void mkdir_p(const std::string& dir) {
   for (size_t i = 1; i <= dir.size(); i++) {
      if (i == dir.size() || dir[i] == '/') {
         const std::string d = dir.substr(0, i);
         if (::mkdir(d.c_str(), 0755) != 0 && errno != EEXIST) throw std::runtime_error("cannot create directory " + d + ": " + std::strerror(errno));
      }
   }
}

inline std::string cycle_dir(int cycle) { char b[32]; std::snprintf(b, sizeof(b), "Cycle%06d", cycle); return b; }
inline std::string piece_name(int rank) { char b[32]; std::snprintf(b, sizeof(b), "proc%06d.vtu", rank); return b; }

inline void write_piece(const std::string& path, const Piece& p, bool light_up) {
   std::ofstream o(path, std::ios::binary);
   if (!o) throw std::runtime_error("cannot write " + path);
   o << "<?xml version=\"1.0\"?>\n<VTKFile type=\"UnstructuredGrid\" version=\"0.1\" byte_order=\"" << (is_little() ? "LittleEndian" : "BigEndian") << "\" header_type=\"UInt32\">\n"
     << "  <UnstructuredGrid>\n    <Piece NumberOfPoints=\"" << p.NN << "\" NumberOfCells=\"" << p.E << "\">\n";
   // displacement x_cur - x_ref (byNODES) is the one array computed here
   std::vector<double> disp((size_t)3 * p.NN);
   for (size_t i = 0; i < disp.size(); i++) disp[i] = p.x_cur[i] - p.x_ref[i];
   o << "      <Points>\n";
   write_array(o, Array{ "Points", T::F64, 3, p.x_cur, 8, 8 * p.NN }, p.NN);
   o << "      </Points>\n      <Cells>\n";
   const int nv = p.tet ? 4 : 8;
   std::vector<int32_t> offs((size_t)p.E); for (int64_t e = 0; e < p.E; e++) offs[e] = (int32_t)(nv * (e + 1));
   const std::vector<uint8_t> types((size_t)p.E, p.tet ? 10 : 12);   // VTK_TETRA / VTK_HEXAHEDRON
   if (nv * p.E > INT32_MAX) throw std::runtime_error("vtu: piece too large for Int32 offsets");
   write_array(o, Array{ "connectivity", T::I32, nv, p.conn, 4 * (int64_t)p.n, 4 }, p.E);
   write_array(o, Array{ "offsets", T::I32, 1, offs.data(), 4, 0 }, p.E);
   write_array(o, Array{ "types", T::U8, 1, types.data(), 1, 0 }, p.E);
   o << "      </Cells>\n      <PointData>\n";
   write_array(o, Array{ "Displacement", T::F64, 3, disp.data(), 8, 8 * p.NN }, p.NN);
   write_array(o, Array{ "Velocity", T::F64, 3, p.vel, 8, 8 * p.NN }, p.NN);
   o << "      </PointData>\n      <CellData>\n";
   for (const Array& a : cell_arrays(p, light_up)) write_array(o, a, p.E);
   o << "      </CellData>\n    </Piece>\n  </UnstructuredGrid>\n</VTKFile>\n";
   if (!o) throw std::runtime_error("write failed: " + path);
}

inline void write_pvtu(const std::string& path, int nranks, bool light_up, bool has_curv = false, bool has_fatigue = false) {
   std::ofstream o(path);
   if (!o) throw std::runtime_error("cannot write " + path);
   o << "<?xml version=\"1.0\"?>\n<VTKFile type=\"PUnstructuredGrid\" version=\"0.1\" byte_order=\"" << (is_little() ? "LittleEndian" : "BigEndian") << "\" header_type=\"UInt32\">\n"
     << "  <PUnstructuredGrid GhostLevel=\"0\">\n    <PPoints>\n      <PDataArray type=\"Float64\" Name=\"Points\" NumberOfComponents=\"3\"/>\n    </PPoints>\n"
     << "    <PPointData>\n      <PDataArray type=\"Float64\" Name=\"Displacement\" NumberOfComponents=\"3\"/>\n"
     << "      <PDataArray type=\"Float64\" Name=\"Velocity\" NumberOfComponents=\"3\"/>\n    </PPointData>\n    <PCellData>\n";
   Piece none; none.has_curv = has_curv; none.has_fatigue = has_fatigue;
   for (const Array& a : cell_arrays(none, light_up)) {
      o << "      <PDataArray type=\"" << type_name(a.type) << "\" Name=\"" << a.name << "\"";
      if (a.ncomp > 1) o << " NumberOfComponents=\"" << a.ncomp << "\"";
      o << "/>\n";
   }
   o << "    </PCellData>\n";
   for (int r = 0; r < nranks; r++) o << "    <Piece Source=\"" << piece_name(r) << "\"/>\n";
   o << "  </PUnstructuredGrid>\n</VTKFile>\n";
}

inline void write_pvd(const std::string& path, const std::vector<std::pair<int, double>>& cycles) {
   const std::string tmp = path + ".tmp";
   {
      std::ofstream o(tmp);
      if (!o) throw std::runtime_error("cannot write " + tmp);
      o.precision(17);
      o << "<?xml version=\"1.0\"?>\n<VTKFile type=\"Collection\" version=\"0.1\" byte_order=\"" << (is_little() ? "LittleEndian" : "BigEndian") << "\">\n  <Collection>\n";
      for (auto& c : cycles) o << "    <DataSet timestep=\"" << c.second << "\" group=\"\" part=\"0\" file=\"" << cycle_dir(c.first) << "/data.pvtu\"/>\n";
      o << "  </Collection>\n</VTKFile>\n";
   }
   if (std::rename(tmp.c_str(), path.c_str()) != 0) throw std::runtime_error("cannot replace " + path);
}

inline std::string basename_of(const std::string& floc) {
   std::string f = floc; while (f.size() > 1 && f.back() == '/') f.pop_back();
   const size_t s = f.find_last_of('/'); return s == std::string::npos ? f : f.substr(s + 1);
}

// one save of a rank: its piece, and on rank 0 the parallel file and the collection (cycles: the collection's saves so far, this one appended)
inline void save_cycle(const std::string& floc, int rank, int nranks, int cycle, double t, bool light_up, const Piece& p, std::vector<std::pair<int, double>>& cycles) {
   const std::string dir = floc + "/" + cycle_dir(cycle);
   mkdir_p(dir);
   write_piece(dir + "/" + piece_name(rank), p, light_up);
   if (rank != 0) return;
   write_pvtu(dir + "/data.pvtu", nranks, light_up, p.has_curv, p.has_fatigue);
   bool found = false;
   for (auto& c : cycles) if (c.first == cycle) { c.second = t; found = true; }
   if (!found) cycles.emplace_back(cycle, t);
   write_pvd(floc + "/" + basename_of(floc) + ".pvd", cycles);
}

}  // namespace vtu
}  // namespace exa_host
