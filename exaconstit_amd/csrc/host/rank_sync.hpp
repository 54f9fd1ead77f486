// Host-only pieces of the host-synchronous transports of comm.hip (in-process loopback, shared device): the rank-ordered fold of a reduction and the
// barrier the threads of a loopback group meet at.  No HIP in here: tests/rank_sync_check.cpp runs them under the thread and address sanitizers.
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <mutex>

namespace exa_host {

enum class RankOp { SUM = 0, MIN = 1, MAX = 2 };

// out[i] = (row(0)[i] op row(1)[i]) op row(2)[i] ...: a left fold starting from rank 0.  Every rank folds the same rows in the same order, so all of
// them hold the same bits afterwards, whatever the order they arrived in.
template <class Row>
inline void rank_fold(RankOp op, int nranks, int n, Row row, double* out) {
   const double* r0 = row(0);
   for (int i = 0; i < n; i++) out[i] = r0[i];
   for (int k = 1; k < nranks; k++) {
      const double* x = row(k);
      for (int i = 0; i < n; i++) out[i] = op == RankOp::SUM ? out[i] + x[i] : (op == RankOp::MIN ? std::min(out[i], x[i]) : std::max(out[i], x[i]));
   }
}

// n threads meet; reusable (generation counter)
struct HostBarrier {
   explicit HostBarrier(int n_) : n(n_) {}
   void meet() {
      std::unique_lock<std::mutex> lk(m);
      const uint64_t g = gen;
      if (++waiting == n) { waiting = 0; gen++; cv.notify_all(); }
      else cv.wait(lk, [&] { return gen != g; });
   }
 private:
   int n; std::mutex m; std::condition_variable cv; int waiting = 0; uint64_t gen = 0;
};

}  // namespace exa_host
