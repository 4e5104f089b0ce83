// The spent set's lane code (aleo_amd/csrc/records_spent_lane.h) run on the HOST: tables built with spent_insert and asked with spent_probe, every answer
// checked against std::set.  Plain C++ for the host compiler, built with the address and undefined-behaviour sanitizers and run as a program of its own
// (tests/test_records_unspent.py):
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -I aleo_amd/csrc tests/cpp/records_spent_lane_emul.cpp
// Cases: capacity 64 with 32 rows (a table half full); a chain that wraps the table's end, of rows whose first word is = capacity - 3 modulo the capacity;
// duplicates; a probe for a row that is absent from a chain as long as the table allows; rows that differ from a stored row in the last word only; and
// seeded random sets of several sizes.
#define __host__
#define __device__
#define __forceinline__ inline
#include "records_spent_lane.h"
#include <array>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <vector>

using namespace aleo_mi355x;
using Row = std::array<uint32_t, 8>;

static unsigned long wrong = 0, asked = 0, wrapped = 0;

struct Table {
  std::vector<Row> rows; std::vector<uint32_t> slots; uint32_t cap;
  explicit Table(const std::vector<Row>& r) : rows(r), cap(spent_capacity(r.size())) {
    slots.assign(cap, 0);
    for (uint32_t i = 0; i < rows.size(); ++i) {
      const uint32_t first = spent_first_slot(rows[i][0], cap);
      const uint32_t got = spent_insert(cap, i, rows[i][0], [&](uint32_t slot, uint32_t expected, uint32_t desired) { const uint32_t old = slots.at(slot); if (old == expected) slots.at(slot) = desired; return old; });
      if (got >= cap) { std::fprintf(stderr, "row %u found no slot\n", i); ++wrong; }
      else if (got < first) ++wrapped;
    }
  }
  bool has(const Row& sn) const {
    uint32_t w[8]; std::memcpy(w, sn.data(), 32);
    return spent_probe(cap, w, [&](uint32_t slot) { return slots.at(slot); }, [&](uint32_t row, uint32_t k) { return rows.at(row)[k]; });
  }
};

static void ask(const Table& t, const std::set<Row>& truth, const Row& sn, const char* what) {
  ++asked;
  if (t.has(sn) != (truth.count(sn) != 0)) { if (wrong++ < 8) std::fprintf(stderr, "%s: the table says %d, the set %d\n", what, (int)t.has(sn), (int)truth.count(sn)); }
}

static void check(const std::vector<Row>& rows, std::mt19937& rng, const char* what) {
  const Table t(rows); const std::set<Row> truth(rows.begin(), rows.end());
  if (t.cap < 64 || (t.cap & (t.cap - 1)) || (uint64_t)t.cap < 2 * rows.size() || (t.cap > 64 && (uint64_t)t.cap / 2 >= 2 * rows.size())) { std::fprintf(stderr, "%s: capacity %u for %zu rows\n", what, t.cap, rows.size()); ++wrong; }
  size_t used = 0; for (uint32_t v : t.slots) used += v != 0;
  if (used != rows.size()) { std::fprintf(stderr, "%s: %zu slots for %zu rows\n", what, used, rows.size()); ++wrong; }      // a duplicate takes a slot of its own
  for (const Row& r : rows) {
    ask(t, truth, r, what);
    Row last = r; last[7] ^= 1u; ask(t, truth, last, what);                 // differs in the last word only
    Row first = r; first[0] ^= 0x80000000u; ask(t, truth, first, what);     // the same first slot, another first word
    Row other; for (auto& w : other) w = rng(); other[0] = r[0]; ask(t, truth, other, what);      // absent, walks r's chain to its end
  }
  for (int i = 0; i < 64; ++i) { Row r; for (auto& w : r) w = rng(); ask(t, truth, r, what); }
}

int main() {
  std::mt19937 rng(20260);
  auto random_row = [&] { Row r; for (auto& w : r) w = rng(); return r; };
  check({}, rng, "no rows");
  { std::vector<Row> rows; for (int i = 0; i < 32; ++i) rows.push_back(random_row()); check(rows, rng, "capacity 64 with 32 rows"); if (Table(rows).cap != 64) { std::fprintf(stderr, "32 rows: capacity %u\n", Table(rows).cap); ++wrong; } }
  { std::vector<Row> rows; for (int i = 0; i < 33; ++i) rows.push_back(random_row()); if (Table(rows).cap != 128) { std::fprintf(stderr, "33 rows: capacity %u\n", Table(rows).cap); ++wrong; } }
  for (uint32_t n : {20u, 32u, 100u}) {                                      // a chain from slot capacity - 3 on: it wraps the table's end
    const uint32_t cap = spent_capacity(n); std::vector<Row> rows;
    for (uint32_t i = 0; i < n; ++i) { Row r = random_row(); r[0] = (r[0] & ~(cap - 1)) | (cap - 3); rows.push_back(r); }
    const unsigned long before = wrapped;
    check(rows, rng, "a wrapping chain");
    if (wrapped == before) { std::fprintf(stderr, "the chain of %u rows did not wrap\n", n); ++wrong; }
    Row absent = random_row(); absent[0] = cap - 3;                          // absent from a full chain: n slots walked, then the empty one
    ask(Table(rows), std::set<Row>(rows.begin(), rows.end()), absent, "absent from a full chain");
  }
  { std::vector<Row> rows; for (int i = 0; i < 10; ++i) rows.push_back(random_row()); for (int i = 0; i < 10; ++i) rows.push_back(rows[i % 3]); check(rows, rng, "duplicates"); }
  { std::vector<Row> rows(40, random_row()); check(rows, rng, "one row 40 times"); }
  for (uint32_t n : {1u, 63u, 64u, 65u, 1000u, 5000u}) { std::vector<Row> rows; for (uint32_t i = 0; i < n; ++i) rows.push_back(random_row()); check(rows, rng, "random rows"); }
  std::printf("records_spent_lane_emul: %lu probes, %lu inserts wrapped, %lu wrong answers\n", asked, wrapped, wrong);
  return wrong ? 1 : 0;
}
