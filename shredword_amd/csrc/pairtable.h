// Host builder of the pair table (table.h): everything sw_encoder_create derives from the caller's
// merges before it touches the device.  Plain C++, no GPU needed: tests/test_pairtable.py runs it
// on the CPU through tests/native/pairtable_check.cpp.
#pragma once
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "table.h"

namespace sw {

// start values of the builders' xorshift generators (a parameter so that a test can sweep draws)
constexpr uint64_t kQ16Seed = 0x452821E638D01377ULL;
constexpr uint64_t kCuckooSeed = 0x243F6A8885A308D3ULL;

struct PairTableHost {
  DevTable table{};               // shift, m1, m2, wide, q16; buckets points into `buckets` below
  std::vector<uint32_t> buckets;  // the bucket image, four words per bucket
  std::vector<uint32_t> inv;      // split_ok: merge value -> pair, two words per value (kInf: none)
  bool ids16 = false;             // every pair member and value <= 0xFFFD, and not wide
  bool split_ok = false;          // values >= 256, unique, larger than both pair members
  int draws = 0;                  // draws of the hash constants up to the accepted image
  // dict: (a << 32 | b) -> value, the last value of a duplicated pair; order: first insertion
  std::unordered_map<uint64_t, int32_t> dict;
  std::vector<uint64_t> order;
  std::string error;              // the message of a status other than SW_OK
};

// SW_OK, or SW_ERR_ARG (a negative id or value) / SW_ERR_ALLOC (no table found) with out->error set;
// the seeds start the quotient and the cuckoo builder's draws
int32_t build_pair_table(const int32_t* pairs, const int32_t* vals, int64_t n, PairTableHost* out,
                         uint64_t q16_seed = kQ16Seed, uint64_t cuckoo_seed = kCuckooSeed);

}  // namespace sw
