// CPU check of the pair-table builder (csrc/pairtable.cpp) through the lookup the kernels call
// (csrc/table.h).  Stand-alone: tests/test_pairtable.py compiles it with pairtable.cpp and runs it
// as a subprocess; built by hand with -fsanitize=address,undefined it needs nothing else.
//
//   pairtable_check TABLE [--sweep N] [--image FILE]
// TABLE: int64 n, int32 pairs[2 n], int32 vals[n].  Builds the table with the default start
// values (and, with --sweep, with N - 1 further ones), checks every build and prints one JSON
// line; --image writes the default build's bucket image.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pairtable.h"

using namespace sw;

namespace {

struct Counts {
  long long keys = 0, bad_keys = 0, nonkeys = 0, bad_nonkeys = 0, bad_inv = 0;
};

uint32_t get(const PairTableHost& pt, uint32_t a, uint32_t b) {
  return pt.table.wide ? lookup<true>(pt.table, a, b) : lookup<false>(pt.table, a, b);
}

// every key resolves to its value, at least kMinNonKeys non-keys to kInf, the inverse maps back
void check(const PairTableHost& pt, Counts* c) {
  constexpr long long kMinNonKeys = 100000;
  auto non_key = [&](uint64_t a, uint64_t b) {
    if (a > 0x7FFFFFFFu || b > 0x7FFFFFFFu || pt.dict.count(a << 32 | b)) return;
    ++c->nonkeys;
    if (get(pt, (uint32_t)a, (uint32_t)b) != kInf) ++c->bad_nonkeys;
  };
  for (uint64_t k : pt.order) {
    const uint32_t a = (uint32_t)(k >> 32), b = (uint32_t)k, v = (uint32_t)pt.dict.at(k);
    ++c->keys;
    if (get(pt, a, b) != v) ++c->bad_keys;
    non_key(b, a);
    non_key(a, (uint64_t)b + 1);
    if (b > 0) non_key(a, (uint64_t)b - 1);
    if (!pt.table.wide) {  // (a narrow key drops the bits over 16: such a pair must still miss)
      non_key((uint64_t)a + 0x10000u, b);
      non_key(a, (uint64_t)b + 0x10000u);
      non_key((uint64_t)a + 0x30000u, (uint64_t)b + 0x50000u);
    }
    if (pt.split_ok && (pt.inv[2 * (size_t)v] != a || pt.inv[2 * (size_t)v + 1] != b)) ++c->bad_inv;
  }
  uint64_t s = 0x9E3779B97F4A7C15ULL;
  const uint32_t span = pt.table.wide ? 0x20000u : 0x10000u;
  for (const long long want = c->nonkeys + kMinNonKeys; c->nonkeys < want;) {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    non_key((uint32_t)(s >> 40) % span, (uint32_t)s % span);
  }
  if (pt.split_ok) {  // (values that no pair merges to stay empty)
    std::vector<uint8_t> used(pt.inv.size() / 2, 0);
    for (uint64_t k : pt.order) used[(size_t)pt.dict.at(k)] = 1;
    for (size_t v = 0; v < used.size(); ++v)
      if (!used[v] && (pt.inv[2 * v] != kInf || pt.inv[2 * v + 1] != kInf)) ++c->bad_inv;
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  int sweep = 1;
  const char* image = nullptr;
  for (int i = 2; i + 1 < argc; i += 2) {
    if (!std::strcmp(argv[i], "--sweep")) sweep = std::atoi(argv[i + 1]);
    else if (!std::strcmp(argv[i], "--image")) image = argv[i + 1];
    else return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t n = 0;
  if (std::fread(&n, sizeof(n), 1, f) != 1 || n < 0) return 2;
  std::vector<int32_t> pairs(2 * (size_t)n), vals((size_t)n);
  if (n > 0 && (std::fread(pairs.data(), 4, pairs.size(), f) != pairs.size() ||
                std::fread(vals.data(), 4, vals.size(), f) != vals.size()))
    return 2;
  std::fclose(f);

  PairTableHost pt;
  const int32_t status = build_pair_table(pairs.data(), vals.data(), n, &pt);
  Counts c;
  if (status == 0) {
    check(pt, &c);
    if (image) {
      std::FILE* o = std::fopen(image, "wb");
      if (!o || std::fwrite(pt.buckets.data(), 4, pt.buckets.size(), o) != pt.buckets.size()) return 2;
      std::fclose(o);
    }
  }
  // further start values: every build checked the same way; flags must not depend on the draw
  Counts sc;
  int sweep_builds = 0, sweep_failed = 0, sweep_flag_changes = 0;
  for (int i = 1; i < sweep && status == 0; ++i) {
    const uint64_t d = 0x9E3779B97F4A7C15ULL * (uint64_t)i;
    PairTableHost p2;
    ++sweep_builds;
    if (build_pair_table(pairs.data(), vals.data(), n, &p2, kQ16Seed ^ d, kCuckooSeed ^ d) != 0) { ++sweep_failed; continue; }
    if (p2.table.wide != pt.table.wide || p2.table.q16 != pt.table.q16 || p2.ids16 != pt.ids16 || p2.split_ok != pt.split_ok)
      ++sweep_flag_changes;
    check(p2, &sc);
  }
  std::printf("{\"status\": %d, \"error\": \"%s\", \"merges\": %zu, \"wide\": %u, \"ids16\": %d, \"q16\": %u, \"split_ok\": %d, "
              "\"draws\": %d, \"shift\": %u, \"m1\": %u, \"m2\": %u, \"buckets\": %zu, "
              "\"keys\": %lld, \"bad_keys\": %lld, \"nonkeys\": %lld, \"bad_nonkeys\": %lld, \"bad_inv\": %lld, "
              "\"sweep_builds\": %d, \"sweep_failed\": %d, \"sweep_flag_changes\": %d, \"sweep_keys\": %lld, "
              "\"sweep_bad_keys\": %lld, \"sweep_nonkeys\": %lld, \"sweep_bad_nonkeys\": %lld, \"sweep_bad_inv\": %lld}\n",
              status, pt.error.c_str(), pt.order.size(), pt.table.wide, (int)pt.ids16, pt.table.q16, (int)pt.split_ok,
              pt.draws, pt.table.shift, pt.table.m1, pt.table.m2, pt.buckets.size() / 4, c.keys, c.bad_keys, c.nonkeys,
              c.bad_nonkeys, c.bad_inv, sweep_builds, sweep_failed, sweep_flag_changes, sc.keys, sc.bad_keys, sc.nonkeys,
              sc.bad_nonkeys, sc.bad_inv);
  return 0;
}
