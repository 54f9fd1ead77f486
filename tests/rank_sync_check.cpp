// Stand-alone check of the host-only synchronisation of the host-synchronous transports (exaconstit_amd/csrc/host/rank_sync.hpp): THREADS threads
// run ROUNDS rounds of the reduction frame of host/comm.hip without its device copies - write the own row, meet, fold all rows in rank order, meet -
// with alternating ops and row lengths, and compare every result with the value known in closed form.  No GPU, no Python.
// scripts/rank_sync_sanitize.sh builds it with -fsanitize=thread and with -fsanitize=address,undefined and runs both.
#include "../exaconstit_amd/csrc/host/rank_sync.hpp"
#include <cstdio>
#include <thread>
#include <vector>

using namespace exa_host;

int main() {
   constexpr int THREADS = 4, ROUNDS = 400;
   HostBarrier bar(THREADS);
   std::vector<std::vector<double>> red(THREADS);   // per-rank contribution of the current reduction (LoopbackGroup::red)
   std::vector<int> bad(THREADS, 0);
   auto value = [](int rank, int round, int i) { return (double)((7 * rank + 3 * i + round) % 11 - 5 + rank); };
   auto work = [&](int rank) {
      std::vector<double> out;
      for (int round = 0; round < ROUNDS; round++) {
         const int n = 1 + round % 70; const RankOp op = (RankOp)(round % 3);
         std::vector<double>& mine = red[rank];
         if (mine.size() < (size_t)n) mine.resize(n);
         for (int i = 0; i < n; i++) mine[i] = value(rank, round, i);
         bar.meet();
         out.assign(n, 0.0);
         rank_fold(op, THREADS, n, [&](int k) { return (const double*)red[k].data(); }, out.data());
         bar.meet();   // everybody has read before the next round overwrites
         for (int i = 0; i < n; i++) {
            double want = value(0, round, i);
            for (int k = 1; k < THREADS; k++) { const double x = value(k, round, i); want = op == RankOp::SUM ? want + x : (op == RankOp::MIN ? std::min(want, x) : std::max(want, x)); }
            if (out[i] != want) bad[rank]++;
         }
      }
   };
   std::vector<std::thread> th;
   for (int r = 0; r < THREADS; r++) th.emplace_back(work, r);
   for (std::thread& t : th) t.join();
   // the order of the fold: ((1e16 + 1) + -1e16) = 0, every other order of the three gives 1
   const double rows[3] = { 1e16, 1.0, -1e16 }; double s = -1.0;
   rank_fold(RankOp::SUM, 3, 1, [&](int k) { return rows + k; }, &s);
   int nbad = s == 0.0 ? 0 : 1;
   for (int b : bad) nbad += b;
   std::printf("rank_sync_check: %d threads, %d rounds, %d wrong values\n", THREADS, ROUNDS, nbad);
   return nbad == 0 ? 0 : 1;
}
