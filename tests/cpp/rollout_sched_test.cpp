// The per-launch schedule of the control-rate rollouts (swarm_layout.h: mrs_ro_launch_sched, mrs_ro_due, mrs_ro_due_count) against brute
// force, on the host: for every rate 1..70, every launch start 0, 64, ..., 448 and every launch length 1..64, the sub-steps the
// kernels' own test calls due are those of the rollout steps where a block starts (commands, forces) or ends (observations, evaluations),
// their ordinal plus the launch's first block is the call's block, the count is mrs_ro_due_count's, and a launch without a due step gets
// the word the kernels read as "nothing here".  No GPU, no library: the header alone.
#include <cstdio>

#include "swarm_layout.h"

// rollout step t starts a block of a start schedule, or ends one of an end schedule
static bool due_step(bool start, int t, int every) { return start ? t % every == 0 : (t + 1) % every == 0; }

static int report(const char* what, int every, int t0, int sub, bool start, const mrs_ro_launch& l) {
  std::printf("%s: every %d, t0 %d, sub %d, %s schedule: word %08x, first block %lld\n", what, every, t0, sub, start ? "start" : "end", (unsigned)l.word,
              l.blk0);
  return 1;
}

int main() {
  // a command word (width 4, FP32 rows), an observation / evaluation word whose groups have bit 5 set, the force word
  const uint32_t cmd_word = (4u | 32u) << 24, cmd_word64 = 4u << 24, groups_word = 0x3Fu << 24, force_word = 3u << 24;
  const struct {
    uint32_t call;
    bool     start;
    uint32_t idle;  // the launch's word when no step of it is due
  } kinds[] = {{cmd_word, true, 32u << 24}, {cmd_word64, true, 0u}, {force_word, true, 0u}, {groups_word, false, 0u}};
  long checked = 0;  // launches with a due step
  for (const auto& k : kinds)
    for (int every = 1; every <= 70; every++)
      for (int t0 = 0; t0 <= 448; t0 += 64)
        for (int sub = 1; sub <= 64; sub++) {
          const mrs_ro_launch l = mrs_ro_launch_sched(k.call, t0, sub, every, k.start);
          int                 want_n = 0;
          for (int s = 0; s < sub; s++) want_n += due_step(k.start, t0 + s, every) ? 1 : 0;
          if (want_n == 0) {  // the hooks read such a word as "no row in this launch" (no width, no groups) before they ask for a due step
            if (l.word != k.idle) return report("a launch without a due step", every, t0, sub, k.start, l);
            continue;
          }
          if ((l.word & 0xFF000000u) != (k.call & 0xFF000000u)) return report("the call's top byte", every, t0, sub, k.start, l);
          int n = 0;
          for (int s = 0; s < sub; s++) {
            const bool want = due_step(k.start, t0 + s, every);
            const int  j    = mrs_ro_due(l.word, s);
            if ((j >= 0) != want) return report("which sub-steps are due", every, t0, sub, k.start, l);
            if (!want) continue;
            if (j != n || l.blk0 + j != (t0 + s) / every) return report("the ordinal and block of a due sub-step", every, t0, sub, k.start, l);
            n++;
          }
          if (mrs_ro_due_count(l.word, sub) != n) return report("mrs_ro_due_count", every, t0, sub, k.start, l);
          checked++;
        }
  std::printf("rollout_sched_test: %ld launches with due steps ok\n", checked);
  return 0;
}
