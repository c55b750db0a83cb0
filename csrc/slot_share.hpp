// Which share of the compute units a slot's next task-queue launch gets, from the progress of the optimiser runs of one problem on
// one device (host only; next to lbfgs_trial_accepted the second pure decision of a fit: no clocks, no device state, the same
// answer for the same counts -- hbegp_debug_slot_shares hands it to the tests as it is).
//
// The runs of a fit do not finish together: the one with the most accepted line-search trials has the longest serial chain of
// evaluations and ends last, alone on the chip, where a single evaluation is bound by its chain of diagonal blocks and cannot use
// the freed compute units.  A run that is behind gets a larger launch while the others are still there to give way.
#pragma once
#include <algorithm>

enum SlotShare { SLOT_SHARE_EVEN = 0, SLOT_SHARE_LEAD = 1, SLOT_SHARE_LAG = 2 };

// A slot is behind when every other running slot has completed more than this many evaluations more (HBEGP_RUN_BALANCE_HYST
// overrides it).  Measured at 2 / 4 / 8 (profiles/run_balance_sweep.txt): the smallest won at every launch size -- the sooner the
// shares follow the drift, the less of it is left when the first run ends.
constexpr int SLOT_SHARE_HYSTERESIS = 2;
// A lead launch gives up this many workgroups of the even launch size and the lag launch takes what the leads gave up: with three
// slots on 256 compute units (even: 96) lead = 80 and lag = 128, the best of (88,104) (88,112) (80,128) (72,144) on config M.  A
// multiple of 8 (the dispatcher deals workgroups round-robin to the 8 XCCs); the launches of all slots together stay at what the
// even launches come to (288).
constexpr int SLOT_SHARE_STEP_WG = 16;
constexpr int SLOT_SHARE_MAX_SLOTS = 8;   // problems with more slots than this keep even shares
// Without HBEGP_RUN_BALANCE in the environment the policy is on from this many 128-blocks on (config M, 32
// blocks, gains 2.2 %; fits of 8 and 16 blocks were 0.6 % and 0.9 % slower with it, and keep the even shares)
constexpr int SLOT_SHARE_MIN_BLOCKS = 32;

inline int slot_share_lead_wg(int even_wg, int /*n_slots*/, int cus) { return std::max(8, std::min(cus, even_wg - SLOT_SHARE_STEP_WG)); }
inline int slot_share_lag_wg(int even_wg, int n_slots, int cus) {
  return std::max(8, std::min(cus, even_wg + SLOT_SHARE_STEP_WG * std::max(1, n_slots - 1)));
}

// running[i] != 0: slot i is inside an optimiser run; done[i]: evaluations that run has completed; maxeval[i]: its cap (a run at
// its cap counts as finished).  share[i] receives a SlotShare.  Rule: the running slot that has completed the fewest evaluations is
// LAG when every other running slot is ahead of it by more than `hysteresis`; the other running slots are then LEAD.  In every
// other case -- fewer than two running slots, a tie for the last place, a gap of at most `hysteresis` -- every slot is EVEN, as are
// slots that are not running.
inline void slot_shares(int n_slots, const int* running, const int* done, const int* maxeval, int hysteresis, int* share) {
  int last = -1, n_running = 0;
  for (int i = 0; i < n_slots; ++i) {
    share[i] = SLOT_SHARE_EVEN;
    if (!running[i] || done[i] >= maxeval[i]) continue;
    ++n_running;
    if (last < 0 || done[i] < done[last]) last = i;
  }
  if (n_running < 2) return;
  for (int i = 0; i < n_slots; ++i) {
    if (i == last || !running[i] || done[i] >= maxeval[i]) continue;
    if ((long long)done[i] - done[last] <= hysteresis) return;  // (share[] is all EVEN up to here)
  }
  for (int i = 0; i < n_slots; ++i)
    if (running[i] && done[i] < maxeval[i]) share[i] = i == last ? SLOT_SHARE_LAG : SLOT_SHARE_LEAD;
}
