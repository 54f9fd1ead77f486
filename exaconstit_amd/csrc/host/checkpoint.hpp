// Checkpoint file of the stand-alone driver: header, section table, hashes.  Host code only: exa_checkpoint_info reads a header
// without a GPU.  All integers and doubles little-endian (the byte order of every host this library runs on).
//
//   bytes 0 ... 255     header (fields below, the rest zero; bytes 248 ... 255 = sum of the 31 preceding 64-bit words modulo 2^64)
//   bytes 256 ...       section table: nsections entries of 48 bytes { char name[24] (zero padded), u64 offset, u64 nbytes, u64 checksum }
//   then                the sections at their offsets (multiples of 64), each a whole number of 64-bit words (host sections zero padded; the
//                       offset of an empty section is not looked at by a reader);
//                       checksum = sum of the section's 64-bit words modulo 2^64
#pragma once
#include <sys/stat.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace exa_ckpt {

constexpr unsigned char MAGIC[8] = { 'E', 'X', 'A', 'C', 'K', 'P', 'T', 0 };
constexpr uint32_t VERSION = 1;
constexpr uint32_t WRITER_THIS_LIBRARY = 0x48415845u;   // "EXAH": matVars0 satisfies the slot-0 invariant of exa_state_normalize as stored
constexpr size_t HEADER_BYTES = 256, ENTRY_BYTES = 48, NAME_BYTES = 24;

struct Header {                       // offset
   uint32_t version = VERSION;        //   8
   uint32_t header_bytes = HEADER_BYTES;   // 12
   int64_t E_global = 0;              //  16
   int64_t NN_global = 0;             //  24
   int32_t Q = 0;                     //  32  quadrature points per element
   int32_t geom = 0;                  //  36  0 hexahedra, 1 tetrahedra
   int32_t order = 1;                 //  40
   int32_t model = 0;                 //  44  EXA_FCC_VOCE ...
   int32_t nprops = 0;                //  48
   int32_t nstatev = 28;              //  52
   uint64_t props_hash = 0;           //  56
   uint64_t grain_hash = 0;           //  64
   uint64_t conn_hash = 0;            //  72
   int64_t steps_done = 0;            //  80
   double time = 0, dt_class = 0, last_dt = 0;   // 88, 96, 104
   int32_t bc_index = -1;             // 112  index of the BCs.update_steps entry in force (-1: none applied yet)
   int32_t nranks = 1;                // 116  ranks that wrote the file (informational)
   uint32_t flags = 0;                // 120  bit 0 cycle0_saved, bit 1 texture0_written
   int32_t nsections = 0;             // 124
   int64_t model_calls = 0;           // 128  constitutive launches so far (schedule of the automatic Newton cap)
   int32_t newton_cap = 0, newton_cap2 = 0;   // 136, 140  caps in force
   uint32_t writer = WRITER_THIS_LIBRARY;     // 144
};                                    // 148 ... 247 zero, 248 header checksum

struct Section { std::string name; uint64_t offset = 0, nbytes = 0, checksum = 0; };

inline uint64_t sum64(const void* p, size_t nbytes) {
   uint64_t s = 0; const unsigned char* c = (const unsigned char*)p;
   for (size_t i = 0; i + 8 <= nbytes; i += 8) { uint64_t w; std::memcpy(&w, c + i, 8); s += w; }
   return s;
}
// FNV-1a over bytes (property values: the same on every rank)
inline uint64_t fnv1a(const void* p, size_t n, uint64_t h = 1469598103934665603ull) {
   const unsigned char* c = (const unsigned char*)p;
   for (size_t i = 0; i < n; i++) { h ^= c[i]; h *= 1099511628211ull; }
   return h;
}
// 64-bit finaliser (splitmix64): per-element hashes are mixed and then ADDED, so that the total does not depend on element order or rank count
inline uint64_t mix64(uint64_t x) { x += 0x9e3779b97f4a7c15ull; x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull; x = (x ^ (x >> 27)) * 0x94d049bb133111ebull; return x ^ (x >> 31); }

template <typename T> inline void put(unsigned char* b, size_t off, T v) { std::memcpy(b + off, &v, sizeof(T)); }
template <typename T> inline T get(const unsigned char* b, size_t off) { T v; std::memcpy(&v, b + off, sizeof(T)); return v; }

inline void encode_header(const Header& h, unsigned char* b /*256*/) {
   std::memset(b, 0, HEADER_BYTES); std::memcpy(b, MAGIC, 8);
   put(b, 8, h.version); put(b, 12, h.header_bytes); put(b, 16, h.E_global); put(b, 24, h.NN_global); put(b, 32, h.Q); put(b, 36, h.geom); put(b, 40, h.order);
   put(b, 44, h.model); put(b, 48, h.nprops); put(b, 52, h.nstatev); put(b, 56, h.props_hash); put(b, 64, h.grain_hash); put(b, 72, h.conn_hash);
   put(b, 80, h.steps_done); put(b, 88, h.time); put(b, 96, h.dt_class); put(b, 104, h.last_dt); put(b, 112, h.bc_index); put(b, 116, h.nranks);
   put(b, 120, h.flags); put(b, 124, h.nsections); put(b, 128, h.model_calls); put(b, 136, h.newton_cap); put(b, 140, h.newton_cap2); put(b, 144, h.writer);
   put(b, 248, sum64(b, 248));
}

// header and section table of a file; refuses what is not a complete checkpoint of this format, naming the reason
inline void read_info(const std::string& path, Header& h, std::vector<Section>& sec) {
   FILE* f = std::fopen(path.c_str(), "rb");
   if (!f) throw std::runtime_error("checkpoint: cannot open " + path);
   struct Closer { FILE* f; ~Closer() { std::fclose(f); } } closer{ f };
   struct stat st; if (::fstat(fileno(f), &st) != 0) throw std::runtime_error("checkpoint: cannot stat " + path);
   const uint64_t fsize = (uint64_t)st.st_size;
   unsigned char b[HEADER_BYTES];
   const size_t got = std::fread(b, 1, HEADER_BYTES, f);
   if (got < 8 || std::memcmp(b, MAGIC, 8) != 0) throw std::runtime_error("checkpoint: wrong magic (" + path + " is not a checkpoint file of this library)");
   if (got < HEADER_BYTES) throw std::runtime_error("checkpoint: truncated file (the header needs 256 bytes, the file has " + std::to_string(fsize) + ")");
   h.version = get<uint32_t>(b, 8); h.header_bytes = get<uint32_t>(b, 12);
   if (h.version != VERSION || h.header_bytes != HEADER_BYTES)
      throw std::runtime_error("checkpoint: unsupported format version " + std::to_string(h.version) + " (this library reads version " + std::to_string(VERSION) + ")");
   if (get<uint64_t>(b, 248) != sum64(b, 248)) throw std::runtime_error("checkpoint: checksum mismatch in the header");
   h.E_global = get<int64_t>(b, 16); h.NN_global = get<int64_t>(b, 24); h.Q = get<int32_t>(b, 32); h.geom = get<int32_t>(b, 36); h.order = get<int32_t>(b, 40);
   h.model = get<int32_t>(b, 44); h.nprops = get<int32_t>(b, 48); h.nstatev = get<int32_t>(b, 52); h.props_hash = get<uint64_t>(b, 56); h.grain_hash = get<uint64_t>(b, 64);
   h.conn_hash = get<uint64_t>(b, 72); h.steps_done = get<int64_t>(b, 80); h.time = get<double>(b, 88); h.dt_class = get<double>(b, 96); h.last_dt = get<double>(b, 104);
   h.bc_index = get<int32_t>(b, 112); h.nranks = get<int32_t>(b, 116); h.flags = get<uint32_t>(b, 120); h.nsections = get<int32_t>(b, 124);
   h.model_calls = get<int64_t>(b, 128); h.newton_cap = get<int32_t>(b, 136); h.newton_cap2 = get<int32_t>(b, 140); h.writer = get<uint32_t>(b, 144);
   if (h.nsections < 0 || h.nsections > 4096) throw std::runtime_error("checkpoint: implausible section count " + std::to_string(h.nsections));
   const uint64_t table_end = HEADER_BYTES + ENTRY_BYTES * (uint64_t)h.nsections;
   if (fsize < table_end) throw std::runtime_error("checkpoint: truncated file (the section table ends at byte " + std::to_string(table_end) + ", the file has " + std::to_string(fsize) + ")");
   std::vector<unsigned char> t(ENTRY_BYTES * (size_t)h.nsections);
   if (!t.empty() && std::fread(t.data(), 1, t.size(), f) != t.size()) throw std::runtime_error("checkpoint: truncated file (section table)");
   sec.resize(h.nsections);
   for (int i = 0; i < h.nsections; i++) {
      const unsigned char* e = t.data() + ENTRY_BYTES * (size_t)i;
      char nm[NAME_BYTES + 1]; std::memcpy(nm, e, NAME_BYTES); nm[NAME_BYTES] = 0;
      sec[i].name = nm; sec[i].offset = get<uint64_t>(e, 24); sec[i].nbytes = get<uint64_t>(e, 32); sec[i].checksum = get<uint64_t>(e, 40);
      if (sec[i].nbytes % 8 != 0 || sec[i].offset < table_end) throw std::runtime_error("checkpoint: malformed table entry of section '" + sec[i].name + "'");
      if (sec[i].nbytes > 0 && sec[i].offset + sec[i].nbytes > fsize)      // (an empty section holds no bytes wherever its offset points)
         throw std::runtime_error("checkpoint: truncated file (section '" + sec[i].name + "' ends at byte " + std::to_string(sec[i].offset + sec[i].nbytes) + ", the file has " +
                                  std::to_string(fsize) + ")");
   }
}

inline const Section* find(const std::vector<Section>& sec, const std::string& name) { for (const Section& s : sec) if (s.name == name) return &s; return nullptr; }

}  // namespace exa_ckpt
