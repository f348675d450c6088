// Test harness (CPU): the bit gathers and the bit-plane transpose of presplit_bits.h on their own
// (their host fallbacks; the device instructions are covered by the GPU tests), beside the whole
// pre-split over a batch (psb_emul).  Built by tests/test_psb_utf8_masks.py.
#include "psb_emul.cpp"

// out[0]: bits4 of x (bit 7 of byte k -> bit k); out[1]: bits8 of (x, y); out[2]: the same for bit 3
extern "C" void psb_gather_words(uint32_t x, uint32_t y, uint32_t* out) {
  out[0] = sw::psb::bits8_raw<7>(x, 0u) >> 7;
  out[1] = sw::psb::bits8_raw<7>(x, y) >> 7;
  out[2] = sw::psb::bits8_raw<3>(x, y) >> 3;
}

// bit 7 of the 32 bytes of w[0..7] by the single-plane gather (bits32)
extern "C" uint32_t psb_gather32(const uint32_t* w) {
  return sw::psb::bits32<7>([&](int i) -> uint32_t { return w[i]; });
}

// planes[b]: bit k = bit b of byte k of the 32 bytes w[0..7] (bit_planes32)
extern "C" void psb_planes32(const uint32_t* w, uint32_t* planes) {
  uint32_t t[8];
  for (int i = 0; i < 8; ++i) t[i] = w[i];
  sw::psb::bit_planes32(t);
  for (int i = 0; i < 8; ++i) planes[i] = t[i];
}
