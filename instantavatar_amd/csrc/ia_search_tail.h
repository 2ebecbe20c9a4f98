// ia_search_tail.h -- where the solves of a SPARSE wave of k_search sit (pure functions of 64-bit lane masks: no HIP types,
// so tests/test_cpu_search_tail_map.py compiles them into a host program).
//
// The deal of fetch_J_quad (ia_search_dev.h) is: round R, lane k of a quad serves pair 4R + k = (target (4R + k) / 3, row
// (4R + k) % 3).  Target 0 of a quad is served in round 0 alone, target 3 in round 2 alone, targets 1 and 2 in two rounds
// each, and fetch_round3<R> is skipped when no lane of the WAVE needs round R.  A wave whose live solves all sit in slot 0
// (lane & 3 == 0) therefore makes one load round trip per step and one whose solves sit in slots 0 and 3 makes two, where
// survivors in random slots make three.  Which lane runs a solve is free: results are written through `item`.
//   * refill: a pull that returns fewer items than the wave has idle lanes hands them out in slot priority 0, 3, 1, 2
//     (`ia_tail_refill_rank`); a full pull keeps the lane order (neighbouring lanes start from neighbouring points).
//   * tail: once at most 32 solves are live (the queue is empty by then: a wave with an idle lane always pulls) and one of
//     them sits outside the slots of its class -- {0, 3} for 17..32 survivors, {0} for at most 16 -- the survivors move, in
//     lane order, to the lanes of those slots (`ia_tail_dest`; `ia_tail_src` is its inverse, what a lane pulls from).  Lanes
//     only retire afterwards, so a wave moves at most twice: on crossing 32 and on crossing 16.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IA_TAIL_HD __host__ __device__ inline
#else
#define IA_TAIL_HD inline
#endif

#define IA_TAIL_SLOT0 0x1111111111111111ull   // the lanes with lane & 3 == 0

IA_TAIL_HD int ia_tail_popc(uint64_t m) { return __builtin_popcountll(m); }
IA_TAIL_HD uint64_t ia_tail_below(int lane) { return (1ull << lane) - 1ull; }
// how many bits of m lie below `lane`.  In device code `lane` must be the calling lane: the count is then v_mbcnt on the mask
// in its scalar registers, and no per-lane 64-bit mask is kept alive across the solver loop (registers bound k_search).
IA_TAIL_HD int ia_tail_count_below(uint64_t m, int lane) {
#if defined(__HIP_DEVICE_COMPILE__)
  (void)lane;
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
#else
  return ia_tail_popc(m & ia_tail_below(lane));
#endif
}

// the lanes a wave with n live solves wants them in: every lane above 32, slots {0, 3} for 17..32, slot 0 up to 16
IA_TAIL_HD uint64_t ia_tail_slots(int n) {
  return n > 32 ? ~0ull : (n > 16 ? (IA_TAIL_SLOT0 | (IA_TAIL_SLOT0 << 3)) : IA_TAIL_SLOT0);
}
// does the wave move its solves?  (no: more than 32 of them, none, or all of them already in their class's slots)
IA_TAIL_HD bool ia_tail_moves(uint64_t active) { return (active & ~ia_tail_slots(ia_tail_popc(active))) != 0; }
// the r-th lane of the class of n survivors
IA_TAIL_HD int ia_tail_slot_lane(int n, int r) { return n > 16 ? 4 * (r >> 1) + 3 * (r & 1) : 4 * r; }

// destination lane of the solve on `lane` (identity for a lane without one and for a wave that does not move)
IA_TAIL_HD int ia_tail_dest(uint64_t active, int lane) {
  if (!ia_tail_moves(active) || !((active >> lane) & 1)) return lane;
  return ia_tail_slot_lane(ia_tail_popc(active), ia_tail_count_below(active, lane));
}

// position of the r-th set bit of m (r < popcount(m)): a binary search on population counts, no loop over the bits
IA_TAIL_HD int ia_tail_nth_set(uint64_t m, int r) {
  int pos = 0;
  for (int w = 32; w > 0; w >>= 1) {
    const int c = ia_tail_popc(m & ((1ull << w) - 1ull));
    if (r >= c) { r -= c; pos += w; m >>= w; }
  }
  return pos;
}
// the lane whose solve lands on `lane` (inverse of ia_tail_dest on a wave that moves), -1 if none does
IA_TAIL_HD int ia_tail_src(uint64_t active, int lane) {
  const int n = ia_tail_popc(active);
  if (!((ia_tail_slots(n) >> lane) & 1)) return -1;
  const int r = n > 16 ? 2 * (lane >> 2) + ((lane & 3) != 0) : lane >> 2;
  return r < n ? ia_tail_nth_set(active, r) : -1;
}

// short pull: position among the idle lanes `need` in slot priority 0, 3, 1, 2, lane order inside a slot
IA_TAIL_HD int ia_tail_refill_rank(uint64_t need, int lane) {
  const uint64_t c0 = need & IA_TAIL_SLOT0, c1 = need & (IA_TAIL_SLOT0 << 1), c2 = need & (IA_TAIL_SLOT0 << 2), c3 = need & (IA_TAIL_SLOT0 << 3);
  const int n0 = ia_tail_popc(c0), n03 = n0 + ia_tail_popc(c3), n031 = n03 + ia_tail_popc(c1);
  const int s = lane & 3;
  return s == 0 ? ia_tail_count_below(c0, lane)
                : (s == 3 ? n0 + ia_tail_count_below(c3, lane)
                          : (s == 1 ? n03 + ia_tail_count_below(c1, lane) : n031 + ia_tail_count_below(c2, lane)));
}
