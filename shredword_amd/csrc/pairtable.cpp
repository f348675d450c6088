// Host builder of the pair table (pairtable.h, table.h).
#include "pairtable.h"

#include <algorithm>
#include <unordered_set>

#include "shredword_hip.h"

namespace sw {

namespace {
struct XorShift {
  uint64_t s;
  uint64_t operator()() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
};

// the quotient table (table.h) for 16-bit ids: buckets = the smallest power of two >= 2^16 with at
// most SW_Q16_FILL keys per bucket on average; constants redrawn (eight tries per size, then the
// buckets double) until no bucket holds more than four keys and no key has an empty entry's tag
bool build_q16(const std::unordered_map<uint64_t, int32_t>& dict, const std::vector<uint64_t>& order, DevTable* t,
               std::vector<uint32_t>* out, int* draws, uint64_t seed) {
  uint32_t log2b = 16;
  while ((double)(1ull << log2b) * 0.25 < (double)order.size()) ++log2b;
  XorShift next{seed};
  for (int attempt = 0; attempt < 64 && log2b <= 24; ++attempt) {
    if (attempt && attempt % 8 == 0) ++log2b;
    const size_t nb = (size_t)1 << log2b;
    t->shift = 32 - log2b;
    t->m1 = (uint32_t)next() | 1u;
    t->m2 = (uint32_t)next() | 1u;
    std::vector<uint32_t> w(nb * 4, 0xFFFFFFFFu);
    std::vector<uint8_t> fill(nb, 0);
    bool ok = true;
    for (uint64_t k : order) {
      const uint32_t a = (uint32_t)(k >> 32), c = (uint32_t)k, v = (uint32_t)dict.at(k);
      const uint32_t x = q16_mix((a << 16) | c, t->m1, t->m2);
      const uint32_t bk = x >> t->shift;
      if (fill[bk] == 4 || (x & 0xFFFFu) == 0xFFFFu) { ok = false; break; }  // (0xFFFF: an empty entry's tag)
      w[4 * (size_t)bk + fill[bk]++] = (x & 0xFFFFu) | (v << 16);
    }
    if (!ok) continue;
    out->swap(w);
    t->q16 = 1;
    *draws = attempt + 1;
    return true;
  }
  return false;
}

// Two-choice cuckoo table (see table.h).  Narrow buckets hold 2 slots, wide buckets 1; the
// bucket count starts at the load factor below and doubles (with fresh hash multipliers) until
// every pair is placed.
bool build_cuckoo(const std::unordered_map<uint64_t, int32_t>& dict, const std::vector<uint64_t>& order, bool wide,
                  DevTable* t, std::vector<uint32_t>* out, int* draws, uint64_t seed) {
  const int slots = wide ? 1 : 2;
  const double max_load = wide ? 0.40 : 0.80;
  uint32_t log2b = 4;
  while ((double)(1ull << log2b) * slots * max_load < (double)order.size()) ++log2b;
  XorShift next{seed};
  for (int attempt = 0; attempt < 64; ++attempt) {
    if (attempt && attempt % 4 == 0 && log2b < 30) ++log2b;
    const size_t nb = (size_t)1 << log2b;
    t->shift = 32 - log2b;
    t->m1 = (uint32_t)next() | 1u;
    t->m2 = (uint32_t)next() | 1u;
    std::vector<uint32_t> b(nb * 4, 0u);  // (every bucket empty: {kEmptyKey, 0, kEmptyKey, 0})
    for (size_t i = 0; i < nb; ++i) b[4 * i] = b[4 * i + 2] = kEmptyKey;
    bool ok = true;
    for (uint64_t k : order) {
      uint32_t a = (uint32_t)(k >> 32), c = (uint32_t)k, v = (uint32_t)dict.at(k);
      for (int kick = 0;; ++kick) {
        if (kick > 500) { ok = false; break; }
        const uint32_t f = mix_key(a, c);
        const uint32_t c1 = bucket1(f, *t), c2 = bucket2(f, *t);
        const uint32_t key = (a << 16) | c;  // (the narrow layout's)
        bool placed = false;
        for (uint32_t bk : {c1, c2}) {
          uint32_t* q = &b[4 * (size_t)bk];
          if (wide) {
            if (q[0] == kEmptyKey) { q[0] = a; q[1] = c; q[2] = v; q[3] = 0; placed = true; break; }
          } else {
            if (q[0] == kEmptyKey) { q[0] = key; q[1] = v; placed = true; break; }
            if (q[2] == kEmptyKey) { q[2] = key; q[3] = v; placed = true; break; }
          }
        }
        if (placed) break;
        // evict a random resident of a random candidate bucket and re-insert it
        uint32_t* q = &b[4 * (size_t)((next() & 1) ? c1 : c2)];
        if (wide) {
          std::swap(q[0], a); std::swap(q[1], c); std::swap(q[2], v);
          q[3] = 0;
        } else {
          const int s = (next() & 1) ? 0 : 2;
          const uint32_t old_key = q[s], old_v = q[s + 1];
          q[s] = key; q[s + 1] = v;
          a = old_key >> 16; c = old_key & 0xFFFF; v = old_v;
        }
      }
      if (!ok) break;
    }
    if (ok) { out->swap(b); *draws = attempt + 1; return true; }
  }
  return false;
}
}  // namespace

int32_t build_pair_table(const int32_t* pairs, const int32_t* vals, int64_t n, PairTableHost* out, uint64_t q16_seed,
                         uint64_t cuckoo_seed) {
  auto fail = [&](int32_t code, const char* msg) { out->error = msg; return code; };
  // dict semantics: the last value of a duplicated pair wins (base.py:145-148)
  auto& dict = out->dict;
  auto& order = out->order;
  dict.reserve((size_t)n * 2);
  order.reserve((size_t)n);
  bool wide = false, ids16 = true;
  for (int64_t i = 0; i < n; ++i) {
    int32_t a = pairs[2 * i], b = pairs[2 * i + 1], v = vals[i];
    if (a < 0 || b < 0) return fail(SW_ERR_ARG, "sw_encoder_create: negative token id in a pair");
    if (v < 0) return fail(SW_ERR_ARG, "sw_encoder_create: negative merge value");
    uint64_t k = ((uint64_t)(uint32_t)a << 32) | (uint32_t)b;
    auto it = dict.find(k);
    if (it == dict.end()) { dict.emplace(k, v); order.push_back(k); }
    else it->second = v;
    if (a > 0xFFFF || b > 0xFFFF || (a == 0xFFFF && b == 0xFFFF)) wide = true;
    if (a > 0xFFFD || b > 0xFFFD || v > 0xFFFD) ids16 = false;
  }
  // well-formed (the split path's precondition, kernels.h): every value >= 256, unique, and
  // larger than both members of its pair
  bool split_ok = true;
  uint32_t max_v = 0;
  {
    std::unordered_set<int32_t> seen;
    seen.reserve(order.size() * 2);
    for (uint64_t k : order) {
      const int32_t v = dict.at(k), a = (int32_t)(k >> 32), b = (int32_t)(uint32_t)k;
      if (v < 256 || v <= a || v <= b || !seen.insert(v).second) split_ok = false;
      max_v = std::max<uint32_t>(max_v, (uint32_t)v);
    }
    if (max_v >= (1u << 26)) split_ok = false;  // (inverse table bounded to 512 MiB)
  }
  out->split_ok = split_ok && !order.empty();
  out->ids16 = ids16 && !wide;
  out->table.wide = wide ? 1u : 0u;
  out->table.q16 = 0;
  if (!(out->ids16 && build_q16(dict, order, &out->table, &out->buckets, &out->draws, q16_seed)) &&
      !build_cuckoo(dict, order, wide, &out->table, &out->buckets, &out->draws, cuckoo_seed))
    return fail(SW_ERR_ALLOC, "sw_encoder_create: could not build the pair table");
  out->table.buckets = out->buckets.data();
  if (out->split_ok) {
    out->inv.assign(2 * ((size_t)max_v + 1), kInf);
    for (uint64_t k : order) {
      const size_t v = (size_t)dict.at(k);
      out->inv[2 * v] = (uint32_t)(k >> 32);
      out->inv[2 * v + 1] = (uint32_t)k;
    }
  }
  return SW_OK;
}

}  // namespace sw
