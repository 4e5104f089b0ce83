// commit_host.hpp — the host side of the commitment lane (records_commit_lane.h): its table, built once per process from serial_host.hpp's BHP1024, and what is
// the same for every record of a call.  Plain C++ (no HIP, touches no device); the table is a function-local static (thread-safe).
#pragma once
#include "serial_host.hpp"
#include "records_commit_lane.h"

namespace aleo_mi355x { namespace serial {

struct CommitTables {
  EdH fixed;                                                 // chunks 0 .. 61 (the domain) and 74 .. 83 (the zero bits 34 .. 63 of the length) of iteration 0
  uint32_t head;                                             // the domain's last two bits, which open chunk 62
  std::vector<uint32_t> words;                               // records_lane.h RK_* and records_commit_lane.h CK_*
};

static const CommitTables& commit_tables() {
  static const CommitTables T = [] {
    CommitTables t;
    const RecordsConsts& C = records_consts();
    const Bhp& B = bhp1024();
    const uint8_t zeros[3 * (CM_PREFIX_CHUNKS - CM_DOMAIN_CHUNKS - CM_LENGTH_CHUNKS)] = {0};
    t.fixed = edh_identity();
    B.add_chunks(t.fixed, B.domain.data(), 3 * CM_DOMAIN_CHUNKS);
    B.add_chunks(t.fixed, zeros, sizeof zeros, CM_DOMAIN_CHUNKS + CM_LENGTH_CHUNKS);
    t.head = B.domain[3 * CM_DOMAIN_CHUNKS] | B.domain[3 * CM_DOMAIN_CHUNKS + 1] << 1;
    WordTable wt(CK_WORDS, C);
    wt.put(CK_TWO, HFr::from_u64(2));
    for (uint32_t e = 0; e < 4 * CM_CHUNKS; ++e) wt.put_cached(CK_TABLE + 3 * e, B.lookup[e]);
    t.words = std::move(wt.words);
    return t;
  }();
  return T;
}

// The bits of (program name | network | record name) of an accepted program id and record name, as the message opens with them
static std::vector<uint8_t> commit_name_bits(const char* program_id, size_t dot, const char* record_name) {
  std::vector<uint8_t> bits;
  auto bytes = [&](const char* p, size_t n) { for (size_t i = 0; i < n; ++i) for (int b = 0; b < 8; ++b) bits.push_back(((uint8_t)p[i] >> b) & 1); };
  bytes(program_id, dot); bytes(program_id + dot + 1, std::strlen(program_id + dot + 1)); bytes(record_name, std::strlen(record_name));
  return bits;
}

// The call's arguments of the lane: the table's fixed chunks and the whole chunks of the names, summed
static CommitArgs commit_args(const std::vector<uint8_t>& name_bits) {
  const CommitTables& T = commit_tables();
  CommitArgs A; std::memset(&A, 0, sizeof A);
  const size_t whole = name_bits.size() / 3;
  EdH p = T.fixed;
  bhp1024().add_chunks(p, name_bits.data(), 3 * whole, CM_PREFIX_CHUNKS);
  p = edh_normalised(p);
  put29(A.start, p.X); put29(A.start + 9, p.Y); put29(A.start + 18, p.T);
  A.first_chunk = CM_PREFIX_CHUNKS + (uint32_t)whole; A.name_bits = (uint32_t)name_bits.size(); A.head = T.head;
  A.lead_n = (uint32_t)(name_bits.size() - 3 * whole);
  for (uint32_t i = 0; i < A.lead_n; ++i) A.lead |= (uint32_t)name_bits[3 * whole + i] << i;
  return A;
}

}}  // namespace aleo_mi355x::serial
