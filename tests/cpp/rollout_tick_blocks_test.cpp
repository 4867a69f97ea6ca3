// rollout_tick_blocks_test.cpp — the block-index helpers of the tick rollouts (swarm_layout.h: mrs_tick_block_start, mrs_tick_block_end)
// against their statement, on the host: for every rate 1..12 and every n_ticks up to 48 that the rate divides, the blocks that START over
// the ticks 0..n-1 are exactly 0..n/every-1, each once, block j at tick j * every; the blocks that END are exactly the same ones, block j
// at tick (j + 1) * every - 1; no other tick reports a block.
#include <cstdio>
#include <vector>

#include "swarm_layout.h"

static int report(const char* what, int every, int n, int t, long long got) {
  std::printf("rollout_tick_blocks_test: %s: every %d, n_ticks %d, tick %d: block %lld\n", what, every, n, t, got);
  return 1;
}

int main() {
  long checked = 0;
  for (int every = 1; every <= 12; every++)
    for (int n = every; n <= 48; n += every) {
      const long long   blocks = n / every;
      std::vector<int> started((size_t)blocks, 0), ended((size_t)blocks, 0);
      for (int t = 0; t < n; t++) {
        const long long b = mrs_tick_block_start(t, every, blocks), j = mrs_tick_block_end(t, every, blocks);
        if (b < -1 || b >= blocks) return report("a start outside the blocks", every, n, t, b);
        if (j < -1 || j >= blocks) return report("an end outside the blocks", every, n, t, j);
        if (b >= 0 && t != b * every) return report("a block starts at the wrong tick", every, n, t, b);
        if (j >= 0 && t != (j + 1) * every - 1) return report("a block ends with the wrong tick", every, n, t, j);
        if (b >= 0) started[(size_t)b]++;
        if (j >= 0) ended[(size_t)j]++;
      }
      for (long long k = 0; k < blocks; k++) {
        if (started[(size_t)k] != 1) return report("a block does not start exactly once", every, n, started[(size_t)k], k);
        if (ended[(size_t)k] != 1) return report("a block does not end exactly once", every, n, ended[(size_t)k], k);
      }
      // a tick behind the call's last one names no block
      if (mrs_tick_block_start(n, every, blocks) != -1) return report("a start behind the last block", every, n, n, mrs_tick_block_start(n, every, blocks));
      if (mrs_tick_block_end(n + every - 1, every, blocks) != -1) return report("an end behind the last block", every, n, n + every - 1, blocks);
      checked++;
    }
  std::printf("rollout_tick_blocks_test: %ld schedules ok\n", checked);
  return 0;
}
