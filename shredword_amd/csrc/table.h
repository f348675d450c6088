// Pair -> rank table shared by the host builder and the device lookups.
//
// Replaces the `merges` dict (shredword/base.py:101, filled at :145-148): key (a, b), value
// merges[(a, b)], which is both the pair's rank and the id of the merged token.
//
// Layout: two-choice cuckoo hash with 16-byte buckets, so a lookup is exactly two independent
// 16-byte loads (one per candidate bucket) issued back to back -- one memory round trip, no
// probe loop, no lane of a wave waiting on a longer probe chain than its neighbours.
//   narrow (every pair member <= 0xFFFF): bucket = 2 slots {key = a << 16 | b, value}
//   wide   (any member > 0xFFFF):         bucket = 1 slot  {a, b, value, 0}
// Empty slots hold key / a = 0xFFFFFFFF (never a valid key: ids are non-negative int32 and the
// narrow key (0xFFFF, 0xFFFF) forces the wide layout).
//
// Round 6, tables whose every id is <= 0xFFFD (SW_INFO_IDS16: the 32k / 50k vocabularies): a
// QUOTIENT table, one 16-byte bucket per lookup instead of two.  The 32-bit key a << 16 | b goes
// through a bijective mix x (two odd multiplies and xor-shifts, constants drawn per build); the
// bucket is x's top bits (at least 16 of them) and each of its four 4-byte entries holds x's low
// 16 bits as the tag and the value: bucket and tag together are x, hence the key -- the lookup is
// exact with no key stored, PROVIDED no key's tag is 0xFFFF.  Empty entries are 0xFFFFFFFF (tag
// 0xFFFF, value 0xFFFF: no pair, as values are <= 0xFFFD), and the last matching entry wins, so
// in a bucket with fewer than four keys an empty entry would answer for such a key.  The builder
// (pairtable.cpp) redraws the constants (and doubles the buckets) until no bucket holds more than
// four keys and no key has that tag, so every lookup is one load and no lane ever needs a second
// probe.  At 32k merges: 2^17 buckets, 2 MB (L2-resident), half the L2 requests of the two-bucket
// lookup.
//
// Also compiles as plain C++ (pairtable.cpp and its CPU test), with four-word stand-ins for the
// HIP vector types: lookup() below is the one function that both the kernels and that test call.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SW_HD __host__ __device__
#define SW_HD_FORCE __host__ __device__ __forceinline__
namespace sw {
using Word4 = uint4;
using Word2 = uint2;
}  // namespace sw
#else
#define SW_HD
#define SW_HD_FORCE inline
namespace sw {
struct Word4 { uint32_t x, y, z, w; };
struct Word2 { uint32_t x, y; };
}  // namespace sw
#endif

namespace sw {

constexpr uint32_t kInf = 0xFFFFFFFFu;     // "pair not in merges" (rank +inf)
constexpr uint32_t kEmptyKey = 0xFFFFFFFFu;

struct DevTable {
  const void* buckets;  // Word4[n_buckets]
  uint32_t shift;       // 32 - log2(n_buckets)
  uint32_t m1, m2;      // odd multipliers of the two hash functions
  uint32_t wide;
  uint32_t q16;         // the quotient layout (16-bit ids; m1, m2: the mix constants)
};

// the quotient table's bijective 32-bit mix (m1, m2 odd): invertible, so bucket + tag identify the key
SW_HD inline uint32_t q16_mix(uint32_t k, uint32_t m1, uint32_t m2) {
  uint32_t x = k * m1;
  x ^= x >> 16;
  x *= m2;
  x ^= x >> 15;
  return x;
}

SW_HD inline uint32_t mix_key(uint32_t a, uint32_t b) {
  // 32-bit fingerprint of the pair used by both bucket choices
  uint32_t x = a * 0x9E3779B1u ^ (b + 0x7F4A7C15u) * 0x85EBCA77u;
  x ^= x >> 15;
  return x;
}
SW_HD inline uint32_t bucket1(uint32_t f, const DevTable& t) { return (f * t.m1) >> t.shift; }
SW_HD inline uint32_t bucket2(uint32_t f, const DevTable& t) { return ((f ^ 0xA5A5A5A5u) * t.m2) >> t.shift; }

// merges.get((a, b)): the value, or kInf.  Two independent 16-byte loads (both cuckoo
// candidate buckets), no loop: one memory round trip for every lane.
template <bool kWide>
SW_HD_FORCE uint32_t lookup(const DevTable& t, uint32_t a, uint32_t b) {
  if (!kWide && t.q16) {  // the quotient table (above): one 16-byte bucket, four tagged entries
    const uint32_t x = q16_mix((a << 16) | b, t.m1, t.m2), tag = x & 0xFFFFu;
    const Word4 q = ((const Word4*)t.buckets)[x >> t.shift];
    uint32_t v = 0xFFFFu;
    v = ((q.x & 0xFFFFu) == tag) ? (q.x >> 16) : v;
    v = ((q.y & 0xFFFFu) == tag) ? (q.y >> 16) : v;
    v = ((q.z & 0xFFFFu) == tag) ? (q.z >> 16) : v;
    v = ((q.w & 0xFFFFu) == tag) ? (q.w >> 16) : v;
    return (v == 0xFFFFu || (a | b) > 0xFFFFu) ? kInf : v;
  }
  const uint32_t f = mix_key(a, b);
  const Word4* B = (const Word4*)t.buckets;
  const Word4 q1 = B[bucket1(f, t)];
  const Word4 q2 = B[bucket2(f, t)];
  if (!kWide) {
    const uint32_t key = (a << 16) | b;
    uint32_t v = kInf;
    v = (q1.x == key) ? q1.y : v;
    v = (q1.z == key) ? q1.w : v;
    v = (q2.x == key) ? q2.y : v;
    v = (q2.z == key) ? q2.w : v;
    return ((a | b) > 0xFFFFu) ? kInf : v;
  } else {
    uint32_t v = kInf;
    v = (q1.x == a && q1.y == b) ? q1.z : v;
    v = (q2.x == a && q2.y == b) ? q2.z : v;
    return v;
  }
}

}  // namespace sw
