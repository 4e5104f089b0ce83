// signatures.h — what signatures.hip and signatures_sign.hip share: the block of their kernels, the message bytes of one launch, and the cut of a call's messages
// into launches.
#pragma once
#include "entry.h"
#include <vector>

namespace aleo_mi355x {

static constexpr uint32_t SIG_BLOCK = 64;                    // one wave: a lane holds its whole signature in registers, and small batches spread over the CUs
static constexpr size_t SIG_CHUNK_BYTES = (size_t)1 << 30;   // message bytes per launch

// The launch that starts at row lo of n: rows lo .. hi, at most `cap` of them, ended by the row that brings the messages to SIG_CHUNK_BYTES.  text: the messages of
// the rows for which travels(i) holds, one after another; off: the hi - lo + 1 offsets into it (a message that does not travel is empty).  Returns hi.
template <class T> size_t cut_messages(std::vector<uint8_t>& text, std::vector<uint32_t>& off, const uint8_t* messages, const uint64_t* offsets, size_t lo, size_t n, size_t cap, T&& travels) {
  off.assign(1, 0); text.clear();
  size_t hi = lo;
  for (; hi < n && hi - lo < cap && text.size() < SIG_CHUNK_BYTES; ++hi) {
    if (travels(hi)) text.insert(text.end(), messages + offsets[hi], messages + offsets[hi + 1]);
    off.push_back((uint32_t)text.size());
  }
  return hi;
}

}  // namespace aleo_mi355x
