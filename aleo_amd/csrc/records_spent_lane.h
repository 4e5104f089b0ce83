// records_spent_lane.h — the set of spent serial numbers that records_unspent_strings[_many] asks (records_unspent.hip): what ONE lane does to put a row in
// and to ask for a serial number.
//
// The set S is n_spent rows of 32 bytes, in any order, duplicates allowed.  The table is `cap` slots of uint32, zero = empty, else a row's number + 1:
//   cap          the smallest power of two >= 2 n_spent, at least 64: the table is never more than half full, so every chain ends at an empty slot
//   first slot   of a row or of a serial number: its first little-endian 32-bit word, masked to cap - 1 (canonical serial numbers are uniform there)
//   next slot    (slot + 1) & (cap - 1): linear probing, wrapping at the table's end
//   insert       the first empty slot from the row's first slot on takes row + 1, through one compare-and-swap per slot tried; a duplicate row takes a slot of
//                its own
//   probe        from the serial number's first slot on, until an empty slot: a hit is a slot whose row equals the serial number in all eight words
// A crafted S — rows that share their first word — only lengthens chains: a hit compares the whole row, so no answer changes.  A row that is no canonical
// field element is stored like any other and equals no serial number.
// Plain C++: the compare-and-swap and the rows come through callables, so tests/cpp/records_spent_lane_emul.cpp runs it on the host.
#pragma once
#include <cstdint>

namespace aleo_mi355x {

static constexpr uint64_t SPENT_MAX_ROWS = (uint64_t)1 << 30;
static constexpr uint32_t SPENT_MIN_SLOTS = 64;

__host__ __device__ __forceinline__ uint32_t spent_capacity(uint64_t n_spent) {      // n_spent <= SPENT_MAX_ROWS: at most 2^31 slots
  uint32_t cap = SPENT_MIN_SLOTS;
  while ((uint64_t)cap < 2 * n_spent) cap <<= 1;
  return cap;
}

__host__ __device__ __forceinline__ uint32_t spent_first_slot(uint32_t word0, uint32_t cap) { return word0 & (cap - 1u); }

// cas(slot, expected, desired) -> the value the slot held (atomicCAS on the device).  Returns the slot taken, or cap where the table is full (it never is: it
// has twice the rows' slots).
template <class Cas>
__host__ __device__ __forceinline__ uint32_t spent_insert(uint32_t cap, uint32_t row, uint32_t word0, Cas&& cas) {
  uint32_t slot = spent_first_slot(word0, cap);
  for (uint32_t tried = 0; tried < cap; ++tried, slot = (slot + 1u) & (cap - 1u))
    if (cas(slot, 0u, row + 1u) == 0u) return slot;
  return cap;
}

// slot_at(slot) -> the slot's value; word_of(row, k) -> word k of row `row` of S.  sn: the serial number's little-endian words.
template <class SlotAt, class WordOf>
__host__ __device__ __forceinline__ bool spent_probe(uint32_t cap, const uint32_t (&sn)[8], SlotAt&& slot_at, WordOf&& word_of) {
  uint32_t slot = spent_first_slot(sn[0], cap);
  for (uint32_t tried = 0; tried < cap; ++tried, slot = (slot + 1u) & (cap - 1u)) {
    const uint32_t v = slot_at(slot);
    if (v == 0u) return false;
    uint32_t diff = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) diff |= word_of(v - 1u, k) ^ sn[k];
    if (diff == 0u) return true;
  }
  return false;
}

}  // namespace aleo_mi355x
