// The host batch path of the encoder: sw_encode_batch(_ex), its pipeline for large batches and the
// copy kernels that move a run over PCIe.  The device launch sequence it drives (encode_device,
// find_specials_device) is encode.hip's; the handle is encoder.h's.
#include <hip/hip_runtime.h>
#include <immintrin.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <utility>
#include <vector>

#include "copy_seg.h"
#include "encoder.h"

using namespace sw;

// ids to 16 bits for the device -> host copy (every id of an ids16 table fits)
__global__ void k_pack16(const int32_t* in, const int64_t* total, uint16_t* out) {
  const int64_t n = *total;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (uint16_t)in[i];
}

// Pipeline copies as kernels over PCIe: a few hundred waves of 16-byte loads keep enough requests
// in flight to run a copy at the link rate (about 57 GB/s each way measured, tools/h2d_probe.hip)
// while the encode kernels run beside them (copy_seg: copy_seg.h, its access ranges checked on the
// CPU by tests/native/copy_seg_emul.cpp).
constexpr int kCopySegs = 6;
struct CopySegs {
  const uint8_t* src[kCopySegs];
  uint8_t* dst[kCopySegs];
  int64_t n[kCopySegs];
};

__global__ void __launch_bounds__(256) k_copy_segs(CopySegs c) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  for (int k = 0; k < kCopySegs; ++k)
    if (c.n[k] > 0) copy_seg(c.src[k], c.dst[k], c.n[k], t, nt);
}

// one run's results straight into the caller's pinned arrays (sw_encoder_pin_host): its ids as
// int32 at the batch's running count done[0] and its string offsets rebased by it; done[1] set
// (nothing written) if the ids would pass out_cap.  k_push_advance then adds the run's count.
__global__ void __launch_bounds__(256) k_push_direct(const int32_t* __restrict__ ids, const int64_t* ntok,
                                                     const int64_t* d_oo, int64_t n_oo, int32_t* out, int64_t* out_off,
                                                     int64_t out_cap, const int64_t* done) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  const int64_t n = *ntok, base = done[0];
  if (done[1] || base + n > out_cap) return;
  copy_seg((const uint8_t*)ids, (uint8_t*)(out + base), n * 4, t, nt);
  for (int64_t j = t; j < n_oo; j += nt) out_off[j] = d_oo[j] + base;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // (system scope: the host-memory writes leave the caches here)
}
__global__ void k_push_advance(const int64_t* ntok, int64_t out_cap, int64_t* done) {
  if (threadIdx.x != 0) return;
  const int64_t n = *ntok;
  if (done[1] || done[0] + n > out_cap) done[1] = 1;
  else done[0] += n;
}

// one run's results to pinned host memory: ids (16-bit when every id fits, 8 per 16-byte store;
// else 32-bit) and the run's string offsets
__global__ void __launch_bounds__(256) k_push_run(const int32_t* __restrict__ ids, const int64_t* ntok, int wide,
                                                  void* h_ids, const int64_t* d_oo, int64_t n_oo, int64_t* h_oo) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  const int64_t n = *ntok;
  if (wide) {
    copy_seg((const uint8_t*)ids, (uint8_t*)h_ids, n * 4, t, nt);
  } else {
    const int64_t n8 = n >> 3;
    const v4u32* s = (const v4u32*)ids;
    v4u32* d = (v4u32*)h_ids;
    for (int64_t i = t; i < n8; i += nt) {
      const v4u32 a = __builtin_nontemporal_load(s + 2 * i), b = __builtin_nontemporal_load(s + 2 * i + 1);
      v4u32 o;
      o.x = (a.x & 0xFFFFu) | (a.y << 16);
      o.y = (a.z & 0xFFFFu) | (a.w << 16);
      o.z = (b.x & 0xFFFFu) | (b.y << 16);
      o.w = (b.z & 0xFFFFu) | (b.w << 16);
      d[i] = o;
    }
    uint16_t* d16 = (uint16_t*)h_ids;
    for (int64_t i = (n8 << 3) + t; i < n; i += nt) d16[i] = (uint16_t)ids[i];
  }
  copy_seg((const uint8_t*)d_oo, (uint8_t*)h_oo, n_oo * 8, t, nt);
}

namespace {

// special-token occurrences of a host batch (positions relative to its first byte, ascending)
struct HostSpecials {
  const int64_t* pos = nullptr;
  const int32_t* len = nullptr;
  const int32_t* id = nullptr;
  int64_t n = 0;
  bool narrow = true;  // every id fits the 16-bit download (<= 0xFFFD)
  bool dev = false;    // found on the device, launch by launch (the handle's specials table): pos /
                       // len / id unused, n = 1
};

// the occurrences inside bytes [a, b) of the batch: [*j0, *j1)
void sp_range(const HostSpecials& sp, int64_t a, int64_t b, int64_t* j0, int64_t* j1) {
  *j0 = std::lower_bound(sp.pos, sp.pos + sp.n, a) - sp.pos;
  *j1 = std::lower_bound(sp.pos, sp.pos + sp.n, b) - sp.pos;
}

// 16-bit ids -> the caller's int32 array, 8 at a time with non-temporal stores (the array is written
// once and not read back here: no read-for-ownership of its lines, about a third less host
// memory traffic than plain stores)
void widen16_stream(const uint16_t* src, int32_t* dst, int64_t n) {
  int64_t i = 0;
  for (; i < n && ((uintptr_t)(dst + i) & 15); ++i) dst[i] = (int32_t)src[i];
  const __m128i z = _mm_setzero_si128();
  for (; i + 8 <= n; i += 8) {
    const __m128i x = _mm_loadu_si128((const __m128i*)(src + i));
    _mm_stream_si128((__m128i*)(dst + i), _mm_unpacklo_epi16(x, z));
    _mm_stream_si128((__m128i*)(dst + i + 4), _mm_unpackhi_epi16(x, z));
  }
  for (; i < n; ++i) dst[i] = (int32_t)src[i];
  _mm_sfence();
}

// a batch call times its own launches: the handle's timing state while it runs, put back after
struct TimingScope {
  sw_encoder* h;
  const bool was_timing;
  const size_t was_used, was_cls;
  explicit TimingScope(sw_encoder* h_) : h(h_), was_timing(h_->timing), was_used(h_->ev_pool.used), was_cls(h_->ev_cls.used) {
    h->timing = true;
    h->ev_pool.used = 0;
    h->ev_cls.used = 0;
  }
  void restore() {
    h->timing = was_timing;
    h->ev_pool.used = was_timing ? was_used : 0;
    h->ev_cls.used = was_timing ? was_cls : 0;
  }
};

// sw_encode_batch for a large host batch: runs of whole strings (<= pipe_run bytes, or one longer
// string) through two slots of pinned and device buffers.  Host thread: stage run k (pool copies
// into pinned memory), enqueue its upload and encode, then drain run k - 1 (its 16/32-bit ids and
// offsets to pinned memory, pool copies out to the caller) while run k encodes.
int32_t encode_batch_pipelined(sw_encoder* h, const uint8_t* bytes, const int64_t* str_off, int64_t n_str,
                               int32_t pattern, const uint64_t* chunk_bits, const HostSpecials& sp, int32_t* out_ids,
                               int64_t out_cap, int64_t* out_off, sw_stats* stats,
                               std::chrono::steady_clock::time_point T0) {
  const bool narrow = h->ids16 && sp.narrow;  // (ids downloaded as 16 bits)
  const int64_t b0 = str_off[0];
  std::vector<std::pair<int64_t, int64_t>> runs;
  int64_t max_b = 1, max_s = 1, max_sp = 1;
  const int64_t run_cap = std::min(h->pipe_run, h->max_launch);  // (a run is one launch)
  for (int64_t s_lo = 0; s_lo < n_str;) {
    int64_t s_hi = s_lo + 1;
    while (s_hi < n_str && str_off[s_hi + 1] - str_off[s_lo] <= run_cap) ++s_hi;
    const int64_t nb = str_off[s_hi] - str_off[s_lo];
    if (nb > h->max_launch)  // (only a run of one string can be over run_cap)
      return fail(SW_ERR_ARG, "sw_encode_batch: a single string exceeds the launch limit");
    runs.emplace_back(s_lo, s_hi);
    max_b = std::max(max_b, nb);
    max_s = std::max(max_s, s_hi - s_lo);
    if (sp.dev) {
      max_sp = std::max(max_sp, nb / h->spt_min_len + 1);  // (the finder's capacity for the run)
    } else if (sp.n > 0) {
      int64_t j0, j1;
      sp_range(sp, str_off[s_lo] - str_off[0], str_off[s_hi] - str_off[0], &j0, &j1);
      max_sp = std::max(max_sp, j1 - j0);
    }
    s_lo = s_hi;
  }
  DeviceGuard g(h->device);
  HIP_TRY(h->s_h2d.ensure());
  HIP_TRY(h->s_d2h.ensure());
  if (!h->pool)
    h->pool = std::make_unique<sw::HostPool>((int)std::max(1u, std::min(16u, std::thread::hardware_concurrency())) - 1);
  for (int slot = 0; slot < h->pipe_depth; ++slot) {
    auto& p = h->pipe[slot];
    if (sp.n > 0 && (p.cap_sp < max_sp || (!sp.dev && !p.h_sp))) {
      p.h_sp.reset(); p.d_sp.reset();
      p.cap_sp = 0;
      // (pinned staging only for occurrences found on the host: the device finder writes d_sp itself)
      if (!sp.dev) HIP_TRY(p.h_sp.reset(3 * max_sp));
      HIP_TRY(p.d_sp.reset(3 * max_sp));
      p.cap_sp = max_sp;
    }
    if (p.cap_bytes >= max_b && p.cap_str >= max_s) continue;
    const int64_t cb = std::max(max_b, p.cap_bytes), cs = std::max(max_s, p.cap_str), cw = (cb + 63) / 64 + 1;
    static_cast<PipeBufs&>(p) = PipeBufs{};  // (every buffer freed before the first is allocated anew)
    HIP_TRY(p.h_in.reset(cb + 16));
    HIP_TRY(p.h_off.reset(cs + 1));
    HIP_TRY(p.h_bits.reset(cw));
    HIP_TRY(p.h_out.reset(cb));
    HIP_TRY(p.h_oo.reset(cs + 1));
    HIP_TRY(p.h_ntok.reset(1));
    HIP_TRY(p.d_in.reset(cb + 16));
    HIP_TRY(p.d_off.reset(cs + 1));
    HIP_TRY(p.d_bits.reset(cw));
    HIP_TRY(p.d_out.reset(cb));
    HIP_TRY(p.d_oo.reset(cs + 1));
    HIP_TRY(p.d_out16.reset(cb));
    HIP_TRY(p.d_ntok.reset(1));
    HIP_TRY(p.e_in.ensure());
    HIP_TRY(p.e_comp.ensure());
    HIP_TRY(p.e_out.ensure());
    p.cap_bytes = cb;
    p.cap_str = cs;
  }
  int32_t rc = ensure_workspace(h, max_b);
  if (rc) return rc;
  // caller ranges pinned by sw_encoder_pin_host: the input read over PCIe by the copy kernel (no
  // staging memcpy), the ids and offsets written by the device into the caller's arrays (no copy
  // or widening on the host)
  const uint8_t* in_dev =
      h->pipe_kcopy ? (const uint8_t*)h->pinned_dev(bytes + b0, std::max<int64_t>(str_off[n_str] - b0, 1)) : nullptr;
  int32_t* out_dev = h->pipe_kcopy ? (int32_t*)h->pinned_dev(out_ids, (int64_t)sizeof(int32_t) * out_cap) : nullptr;
  int64_t* oo_dev = h->pipe_kcopy ? (int64_t*)h->pinned_dev(out_off, (int64_t)sizeof(int64_t) * (n_str + 1)) : nullptr;
  const bool direct_out = out_dev && oo_dev;
  if (direct_out) {
    if (!h->d_done) HIP_TRY(h->d_done.reset(2));
    HIP_TRY(hipMemsetAsync(h->d_done, 0, 2 * sizeof(int64_t), h->s_d2h));
  }
  const bool count = stats && !chunk_bits;
  if (count) HIP_TRY(hipMemsetAsync(h->ws.d_pcount, 0, sizeof(unsigned long long), h->stream));
  TimingScope timing(h);
  sw::HostPool& pool = *h->pool;
  double ms_stage = 0, ms_drain = 0;
  int64_t done = 0;
  int64_t p_nsp[4] = {0, 0, 0, 0};  // special-token occurrences staged per slot
  static const bool trace = std::getenv("SW_PIPE_TRACE") != nullptr;  // (diagnostic timeline)
  auto stamp = [&](const char* what, size_t k) {
    if (trace)
      std::fprintf(stderr, "pipe %8.3f %-10s %zu\n",
                   std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - T0).count(), what, k);
  };
  auto stage = [&](size_t k) -> int32_t {
    auto& p = h->pipe[k % h->pipe_depth];
    const int64_t s_lo = runs[k].first, s_hi = runs[k].second, a0 = str_off[s_lo], nb = str_off[s_hi] - a0;
    auto t = std::chrono::steady_clock::now();
    const uint8_t* src = bytes + a0;
    if (!in_dev)
      pool.parallel_for(nb, [&](int64_t lo, int64_t hi) { std::memcpy(p.h_in + lo, src + lo, (size_t)(hi - lo)); });
    for (int64_t j = 0; j <= s_hi - s_lo; ++j) p.h_off[j] = str_off[s_lo + j] - a0;
    if (sp.dev) {
      p_nsp[k % h->pipe_depth] = nb / h->spt_min_len + 1;  // (found on the device after the upload)
    } else if (sp.n > 0) {  // the run's special-token occurrences, rebased: positions, then lengths and ids (int32)
      int64_t j0, j1;
      sp_range(sp, a0 - b0, a0 - b0 + nb, &j0, &j1);
      const int64_t m = j1 - j0;
      int32_t* l32 = (int32_t*)(p.h_sp + m);
      for (int64_t j = 0; j < m; ++j) {
        p.h_sp[j] = sp.pos[j0 + j] - (a0 - b0);
        l32[j] = sp.len[j0 + j];
        l32[m + j] = sp.id[j0 + j];
      }
      p_nsp[k % h->pipe_depth] = m;
    }
    if (chunk_bits) {  // the run's bits, realigned to its first byte
      const int64_t g0 = a0 - b0, nw = (nb + 63) / 64, last_q = (str_off[n_str] - b0 - 1) / 64;
      pool.parallel_for(nw, [&](int64_t lo, int64_t hi) {
        for (int64_t w = lo; w < hi; ++w) {
          const int64_t bit = g0 + 64 * w, q = bit >> 6, r = bit & 63;
          uint64_t x = chunk_bits[q] >> r;
          if (r && q + 1 <= last_q) x |= chunk_bits[q + 1] << (64 - r);
          p.h_bits[w] = x;
        }
      });
    }
    ms_stage += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
    stamp("staged", k);
    return SW_OK;
  };
  auto issue = [&](size_t k) -> int32_t {
    auto& p = h->pipe[k % h->pipe_depth];
    const int64_t s_lo = runs[k].first, s_hi = runs[k].second, nb = str_off[s_hi] - str_off[s_lo], ns = s_hi - s_lo;
    const int64_t n_bits = chunk_bits ? (int64_t)sizeof(uint64_t) * ((nb + 63) / 64) : 0;
    const int64_t m_sp = sp.n > 0 ? p_nsp[k % h->pipe_depth] : 0, n_sp_bytes = sp.dev ? 0 : 16 * m_sp;  // (8 + 4 + 4 B each)
    if (h->pipe_kcopy) {
      const uint8_t* in_src = in_dev ? in_dev + (str_off[s_lo] - b0) : p.h_in.get();
      const CopySegs c{{in_src, (const uint8_t*)p.h_off.get(), (const uint8_t*)p.h_bits.get(), (const uint8_t*)p.h_sp.get(), nullptr, nullptr},
                       {p.d_in, (uint8_t*)p.d_off.get(), (uint8_t*)p.d_bits.get(), (uint8_t*)p.d_sp.get(), nullptr, nullptr},
                       {nb, (int64_t)sizeof(int64_t) * (ns + 1), n_bits, n_sp_bytes, 0, 0}};
      hipLaunchKernelGGL(k_copy_segs, dim3(128), dim3(256), 0, h->s_h2d, c);
      HIP_TRY(hipGetLastError());
    } else {
      HIP_TRY(hipMemcpyAsync(p.d_in, p.h_in, (size_t)nb, hipMemcpyHostToDevice, h->s_h2d));
      HIP_TRY(hipMemcpyAsync(p.d_off, p.h_off, sizeof(int64_t) * (ns + 1), hipMemcpyHostToDevice, h->s_h2d));
      if (chunk_bits) HIP_TRY(hipMemcpyAsync(p.d_bits, p.h_bits, (size_t)n_bits, hipMemcpyHostToDevice, h->s_h2d));
      if (n_sp_bytes > 0) HIP_TRY(hipMemcpyAsync(p.d_sp, p.h_sp, (size_t)n_sp_bytes, hipMemcpyHostToDevice, h->s_h2d));
    }
    HIP_TRY(hipEventRecord(p.e_in, h->s_h2d));
    HIP_TRY(hipStreamWaitEvent(h->stream, p.e_in, 0));
    DevSpecials dsp;
    if (m_sp > 0) {
      dsp.pos = p.d_sp; dsp.len = (const int32_t*)(p.d_sp + m_sp); dsp.id = dsp.len + m_sp; dsp.n = m_sp;
    }
    if (sp.dev) {  // the occurrences found on the device, the count left there (p.d_sp's tail)
      int64_t* d_cnt = p.d_sp + 2 * m_sp;
      const int32_t r = find_specials_device(h, p.d_in, nb, p.d_off, ns, p.d_sp, (int32_t*)dsp.len, (int32_t*)dsp.id,
                                             m_sp, d_cnt, h->stream);
      if (r) return r;
      dsp.n_dev = d_cnt;
    }
    const int32_t r = encode_device(h, p.d_in, nb, p.d_off, ns, chunk_bits ? p.d_bits.get() : nullptr, dsp, p.d_out, false,
                                    p.d_oo, h->stream, nullptr, pattern);
    if (r) return r;
    if (count && nb > 0) launch_popcount(h->stream, h->ws.d_pbits, (nb + 63) / 64, h->ws.d_pcount);
    if (h->pipe_kcopy) {
      // the download kernel runs on s_d2h beside the next run's encode, which rewrites d_total
      HIP_TRY(hipMemcpyAsync(p.d_ntok, h->ws.d_total, sizeof(int64_t), hipMemcpyDeviceToDevice, h->stream));
    } else if (narrow) {
      hipLaunchKernelGGL(k_pack16, dim3(2048), dim3(256), 0, h->stream, p.d_out.get(), h->ws.d_total.get(), p.d_out16.get());
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(p.h_ntok, h->ws.d_total, sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipEventRecord(p.e_comp, h->stream));
    if (h->pipe_kcopy) {
      HIP_TRY(hipStreamWaitEvent(h->s_d2h, p.e_comp, 0));
      if (direct_out) {
        hipLaunchKernelGGL(k_push_direct, dim3(128), dim3(256), 0, h->s_d2h, p.d_out.get(), p.d_ntok.get(), p.d_oo.get(),
                           ns + 1, out_dev, oo_dev + s_lo, out_cap, h->d_done.get());
        hipLaunchKernelGGL(k_push_advance, dim3(1), dim3(64), 0, h->s_d2h, p.d_ntok.get(), out_cap, h->d_done.get());
      } else {
        hipLaunchKernelGGL(k_push_run, dim3(128), dim3(256), 0, h->s_d2h, p.d_out.get(), p.d_ntok.get(), narrow ? 0 : 1,
                           (void*)p.h_out.get(), p.d_oo.get(), ns + 1, p.h_oo.get());
      }
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(p.e_out, h->s_d2h));
    }
    return SW_OK;
  };
  auto drain = [&](size_t k) -> int32_t {
    auto& p = h->pipe[k % h->pipe_depth];
    const int64_t s_lo = runs[k].first, s_hi = runs[k].second, ns = s_hi - s_lo;
    HIP_TRY(hipEventSynchronize(p.e_comp));
    stamp("encoded", k);
    const int64_t nt = p.h_ntok[0];
    if (done + nt > out_cap) return fail(SW_ERR_CAP, "sw_encode_batch: out_cap too small");
    auto t = std::chrono::steady_clock::now();
    if (!h->pipe_kcopy) {
      HIP_TRY(hipStreamWaitEvent(h->s_d2h, p.e_comp, 0));
      if (nt > 0)
        HIP_TRY(hipMemcpyAsync(p.h_out, narrow ? (void*)p.d_out16.get() : (void*)p.d_out.get(),
                               (size_t)nt * (narrow ? 2 : 4), hipMemcpyDeviceToHost, h->s_d2h));
      HIP_TRY(hipMemcpyAsync(p.h_oo, p.d_oo, sizeof(int64_t) * (ns + 1), hipMemcpyDeviceToHost, h->s_d2h));
      HIP_TRY(hipEventRecord(p.e_out, h->s_d2h));
    }
    HIP_TRY(hipEventSynchronize(p.e_out));
    stamp("pushed", k);
    if (direct_out) {  // (the device wrote them into the caller's arrays)
      done += nt;
      ms_drain += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
      return SW_OK;
    }
    int32_t* dst = out_ids + done;
    if (narrow) {
      const uint16_t* s16 = (const uint16_t*)p.h_out.get();
      pool.parallel_for(nt, [&](int64_t lo, int64_t hi) { widen16_stream(s16 + lo, dst + lo, hi - lo); });
    } else {
      const int32_t* s32 = p.h_out;
      pool.parallel_for(nt, [&](int64_t lo, int64_t hi) { std::memcpy(dst + lo, s32 + lo, sizeof(int32_t) * (hi - lo)); });
    }
    for (int64_t j = 0; j <= ns; ++j) out_off[s_lo + j] = p.h_oo[j] + done;
    done += nt;
    stamp("drained", k);
    ms_drain += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
    return SW_OK;
  };
  // host order: stage k, issue k, then drain the oldest run when every slot is taken (pipe_depth
  // runs in flight: run k's upload overlaps the encodes and downloads of the runs before it)
  auto bail = [&](int32_t r) {  // leave nothing in flight on the slots' buffers
    (void)hipStreamSynchronize(h->s_h2d);
    (void)hipStreamSynchronize(h->stream);
    (void)hipStreamSynchronize(h->s_d2h);
    timing.restore();
    return r;
  };
  const size_t depth = (size_t)h->pipe_depth;
  size_t next_drain = 0;
  for (size_t k = 0; k < runs.size(); ++k) {
    rc = stage(k);
    if (!rc) rc = issue(k);
    if (!rc && next_drain + depth <= k + 1) rc = drain(next_drain++);  // frees run k + 1's slot
    if (rc) return bail(rc);
  }
  while (next_drain < runs.size())
    if ((rc = drain(next_drain++))) return bail(rc);
  if (n_str == 0) out_off[0] = 0;
  const double k_ms = sw_encoder_last_kernel_ms(h) * (double)runs.size();
  int64_t n_chunks = -1;
  if (count) {
    unsigned long long c = 0;
    HIP_TRY(hipMemcpy(&c, h->ws.d_pcount, sizeof(c), hipMemcpyDeviceToHost));
    n_chunks = (int64_t)c;
  }
  timing.restore();
  if (stats) {
    stats->n_bytes = str_off[n_str] - b0;
    stats->n_chunks = n_chunks;
    stats->n_tokens = done;
    stats->ms_presplit = 0;
    stats->ms_h2d = ms_stage;   // (host staging into pinned memory; the uploads overlap)
    stats->ms_kernels = k_ms;
    stats->ms_d2h = ms_drain;   // (downloads + copies out, overlapped with the next run's encode)
    stats->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - T0).count();
  }
  return SW_OK;
}

// sw_encode_batch(_ex) with the batch's special-token occurrences found (sp, relative to str_off[0])
int32_t encode_batch_impl(sw_encoder* h, const uint8_t* bytes, const int64_t* str_off, int64_t n_str, int32_t pattern,
                          const uint64_t* chunk_bits, const HostSpecials& sp, int32_t* out_ids, int64_t out_cap,
                          int64_t* out_off, sw_stats* stats) {
  auto T0 = std::chrono::steady_clock::now();
  if (!h || !str_off || !out_off || n_str < 0) return fail(SW_ERR_ARG, "sw_encode_batch: bad arguments");
  const int64_t b0 = n_str > 0 ? str_off[0] : 0;
  const int64_t n_bytes = n_str > 0 ? str_off[n_str] - b0 : 0;
  if (n_bytes < 0 || (n_bytes > 0 && !bytes)) return fail(SW_ERR_ARG, "sw_encode_batch: bad string offsets");
  for (int64_t s = 0; s < n_str; ++s)
    if (str_off[s + 1] < str_off[s]) return fail(SW_ERR_ARG, "sw_encode_batch: string offsets not monotone");
  if (n_bytes > 0 && !out_ids) return fail(SW_ERR_ARG, "sw_encode_batch: null out_ids");
  if (!chunk_bits && pattern != SW_PAT_CL100K && pattern != SW_PAT_GPT2 && pattern != SW_PAT_NONE)
    return fail(SW_ERR_ARG, "sw_encode_batch: bad pattern");
  if (h->pipe_run > 0 && n_bytes > 2 * h->pipe_run && !(h->host_presplit && !chunk_bits))
    return encode_batch_pipelined(h, bytes, str_off, n_str, pattern, chunk_bits, sp, out_ids, out_cap, out_off, stats,
                                  T0);
  if (n_bytes > h->max_launch) {
    // one device launch addresses < 2^30 bytes: encode runs of whole strings separately
    int64_t done = 0, s_lo = 0;
    if (stats) *stats = sw_stats{};
    while (s_lo < n_str) {
      int64_t s_hi = s_lo + 1;
      while (s_hi < n_str && str_off[s_hi + 1] - str_off[s_lo] <= h->max_launch) ++s_hi;
      if (str_off[s_hi] - str_off[s_lo] > h->max_launch)
        return fail(SW_ERR_ARG, "sw_encode_batch: a single string exceeds the launch limit (2^30 - 64 bytes)");
      std::vector<uint64_t> sub;
      if (chunk_bits) {  // the run's bits, realigned to its first byte
        const int64_t g0 = str_off[s_lo] - b0, nb = str_off[s_hi] - str_off[s_lo];
        sub.assign((size_t)((nb + 63) / 64 + 1), 0ULL);
        for (int64_t w = 0; w < (nb + 63) / 64; ++w) {
          const int64_t bit = g0 + 64 * w, q = bit >> 6, r = bit & 63;
          uint64_t x = chunk_bits[q] >> r;
          if (r && q + 1 <= (str_off[n_str] - b0 - 1) / 64) x |= chunk_bits[q + 1] << (64 - r);
          sub[(size_t)w] = x;
        }
      }
      sw_stats st{};
      HostSpecials ssp = sp;  // (the run's occurrences, rebased to its first byte)
      int64_t j0 = 0, j1 = 0;
      std::vector<int64_t> spos;
      if (sp.n > 0 && !sp.dev) {
        const int64_t g0 = str_off[s_lo] - b0;
        sp_range(sp, g0, str_off[s_hi] - b0, &j0, &j1);
        spos.resize((size_t)(j1 - j0));
        for (int64_t j = j0; j < j1; ++j) spos[(size_t)(j - j0)] = sp.pos[j] - g0;
        ssp.pos = spos.data(); ssp.len = sp.len + j0; ssp.id = sp.id + j0; ssp.n = j1 - j0;
      }
      int32_t rc = encode_batch_impl(h, bytes, str_off + s_lo, s_hi - s_lo, pattern, chunk_bits ? sub.data() : nullptr,
                                     ssp, out_ids + done, out_cap - done, out_off + s_lo, &st);
      if (rc) return rc;
      for (int64_t s = s_lo; s <= s_hi; ++s) out_off[s] += done;
      done = out_off[s_hi];
      if (stats) {
        // (a run without a chunk count -- caller bits -- makes the total unknown: -1)
        stats->n_chunks = (stats->n_chunks < 0 || st.n_chunks < 0) ? -1 : stats->n_chunks + st.n_chunks;
        stats->n_bytes += st.n_bytes; stats->n_tokens += st.n_tokens;
        stats->ms_presplit += st.ms_presplit; stats->ms_h2d += st.ms_h2d; stats->ms_kernels += st.ms_kernels;
        stats->ms_d2h += st.ms_d2h;
      }
      s_lo = s_hi;
    }
    if (stats)
      stats->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - T0).count();
    return SW_OK;
  }
  const int64_t n_words = (n_bytes + 63) / 64;
  std::vector<uint64_t> own_bits;
  double ms_pre = 0;
  int64_t n_chunks = -1;
  const bool device_presplit = !chunk_bits && !h->host_presplit;
  if (!chunk_bits && !device_presplit) {
    own_bits.resize((size_t)std::max<int64_t>(n_words, 1));
    auto a = std::chrono::steady_clock::now();
    n_chunks = sp.n > 0 ? sw_presplit_host_specials(bytes, str_off, n_str, pattern, sp.pos, sp.len, sp.n, own_bits.data(), 0)
                        : sw_presplit_host(bytes, str_off, n_str, pattern, own_bits.data(), 0);
    if (n_chunks < 0) return fail((int32_t)n_chunks, "sw_encode_batch: bad pattern or offsets");
    ms_pre = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
    chunk_bits = own_bits.data();
  }
  DeviceGuard g(h->device);
  IoStaging& io = h->io;
  // device staging (grown on demand)
  if (n_bytes > io.io_bytes || n_str > io.io_str) {
    io = IoStaging{};
    const int64_t nb = std::max<int64_t>(n_bytes, 1), ns = std::max<int64_t>(n_str, 1);
    HIP_TRY(io.d_bytes.reset(nb));
    HIP_TRY(io.d_str_off.reset(ns + 1));
    HIP_TRY(io.d_bits.reset((nb + 63) / 64));
    HIP_TRY(io.d_out.reset(nb));
    HIP_TRY(io.d_out_off.reset(ns + 1));
    io.io_bytes = nb; io.io_str = ns;
  }
  const int64_t sp_need = sp.dev ? n_bytes / h->spt_min_len + 1 : sp.n;  // (the device finder's capacity)
  if (sp_need > io.sp_cap) {
    io.d_sp_pos.reset(); io.d_sp_len.reset(); io.d_sp_id.reset();
    io.sp_cap = 0;
    HIP_TRY(io.d_sp_pos.reset(sp_need));
    HIP_TRY(io.d_sp_len.reset(sp_need));
    HIP_TRY(io.d_sp_id.reset(sp_need));
    io.sp_cap = sp_need;
  }
  if (sp.dev && !h->d_nsp) HIP_TRY(h->d_nsp.reset(1));
  std::vector<int64_t> rel((size_t)n_str + 1);
  for (int64_t s = 0; s <= n_str; ++s) rel[s] = n_str > 0 ? str_off[s] - b0 : 0;
  auto a = std::chrono::steady_clock::now();
  hipStream_t st = h->stream;
  if (n_bytes > 0) {
    HIP_TRY(hipMemcpyAsync(io.d_bytes, bytes + b0, n_bytes, hipMemcpyHostToDevice, st));
    if (!device_presplit)
      HIP_TRY(hipMemcpyAsync(io.d_bits, chunk_bits, sizeof(uint64_t) * n_words, hipMemcpyHostToDevice, st));
  }
  HIP_TRY(hipMemcpyAsync(io.d_str_off, rel.data(), sizeof(int64_t) * (n_str + 1), hipMemcpyHostToDevice, st));
  DevSpecials dsp;
  if (sp.dev) {
    const int32_t r = find_specials_device(h, io.d_bytes, n_bytes, io.d_str_off, n_str, io.d_sp_pos, io.d_sp_len,
                                           io.d_sp_id, io.sp_cap, h->d_nsp, st);
    if (r) return r;
    dsp.pos = io.d_sp_pos; dsp.len = io.d_sp_len; dsp.id = io.d_sp_id; dsp.n = io.sp_cap; dsp.n_dev = h->d_nsp;
  } else if (sp.n > 0) {
    HIP_TRY(hipMemcpyAsync(io.d_sp_pos, sp.pos, sizeof(int64_t) * sp.n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(io.d_sp_len, sp.len, sizeof(int32_t) * sp.n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(io.d_sp_id, sp.id, sizeof(int32_t) * sp.n, hipMemcpyHostToDevice, st));
    dsp.pos = io.d_sp_pos; dsp.len = io.d_sp_len; dsp.id = io.d_sp_id; dsp.n = sp.n;
  }
  HIP_TRY(hipStreamSynchronize(st));
  double ms_h2d = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
  int64_t n_tok = 0;
  TimingScope timing(h);
  int32_t rc = encode_device(h, io.d_bytes, n_bytes, io.d_str_off, n_str, device_presplit ? nullptr : io.d_bits.get(), dsp,
                             io.d_out, false, io.d_out_off, st, &n_tok, pattern);
  if (rc == SW_OK && device_presplit && stats && n_bytes > 0) {  // chunk count for the stats
    HIP_TRY(hipMemsetAsync(h->ws.d_pcount, 0, sizeof(unsigned long long), st));
    launch_popcount(st, h->ws.d_pbits, n_words, h->ws.d_pcount);
    unsigned long long c = 0;
    HIP_TRY(hipMemcpyAsync(&c, h->ws.d_pcount, sizeof(c), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    n_chunks = (int64_t)c;
  }
  const double k_ms = sw_encoder_last_kernel_ms(h);
  timing.restore();
  if (rc) return rc;
  if (n_tok > out_cap) return fail(SW_ERR_CAP, "sw_encode_batch: out_cap too small");
  a = std::chrono::steady_clock::now();
  if (n_tok > 0) HIP_TRY(hipMemcpyAsync(out_ids, io.d_out, sizeof(int32_t) * n_tok, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(out_off, io.d_out_off, sizeof(int64_t) * (n_str + 1), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  double ms_d2h = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
  if (stats) {
    stats->n_bytes = n_bytes;
    stats->n_chunks = n_chunks;
    stats->n_tokens = n_tok;
    stats->ms_presplit = ms_pre;
    stats->ms_h2d = ms_h2d;
    stats->ms_kernels = k_ms;
    stats->ms_d2h = ms_d2h;
    stats->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - T0).count();
  }
  return SW_OK;
}

}  // namespace

extern "C" int32_t sw_encode_batch(sw_encoder* h, const uint8_t* bytes, const int64_t* str_off, int64_t n_str,
                                   int32_t pattern, const uint64_t* chunk_bits, int32_t* out_ids, int64_t out_cap,
                                   int64_t* out_off, sw_stats* stats) {
  return encode_batch_impl(h, bytes, str_off, n_str, pattern, chunk_bits, HostSpecials{}, out_ids, out_cap, out_off,
                           stats);
}

// device memory the device special-token finder may take for sw_encode_batch_ex (its worst-case
// occurrence arrays of every pipeline slot and its per-tile lists); beyond it the host threads find them
constexpr int64_t kSpDeviceBudget = 1LL << 30;

extern "C" int32_t sw_encode_batch_ex(sw_encoder* h, const uint8_t* bytes, const int64_t* str_off, int64_t n_str,
                                      int32_t pattern, const uint64_t* chunk_bits, const sw_specials* specials,
                                      int32_t* out_ids, int64_t out_cap, int64_t* out_off, sw_stats* stats) {
  if (!specials || specials->n == 0)
    return encode_batch_impl(h, bytes, str_off, n_str, pattern, chunk_bits, HostSpecials{}, out_ids, out_cap, out_off,
                             stats);
  if (!h || !str_off || n_str < 0) return fail(SW_ERR_ARG, "sw_encode_batch_ex: bad arguments");
  for (int64_t k = 0; k < specials->n; ++k)
    if (specials->ids && (specials->ids[k] < 0 || specials->ids[k] == INT32_MAX))
      return fail(SW_ERR_ARG, "sw_encode_batch_ex: special token ids must be in [0, 2^31 - 2]");
  // the device finder: every special <= 64 bytes, the device pre-split (the host pre-split needs the
  // occurrences on the host), and room for its worst case (n / shortest special occurrences)
  if (h->device_specials && !chunk_bits && !h->host_presplit) {
    int32_t rc = set_specials(h, specials);
    if (rc) return rc;
    const int64_t nb = n_str > 0 ? str_off[n_str] - str_off[0] : 0;
    const int64_t run = h->pipe_run > 0 && nb > 2 * h->pipe_run ? std::min(h->pipe_run, h->max_launch)
                                                                   : std::min(nb, h->max_launch);
    // (the finder sizes its arrays for the worst case -- every run packed with the shortest special:
    // 24 B per possible occurrence and slot, and each tile's list -- so short specials on large runs
    // fall back to the host threads rather than take gigabytes of device memory)
    const int64_t slots = h->pipe_run > 0 && nb > 2 * h->pipe_run ? h->pipe_depth : 1;
    const int64_t worst = 24 * (run / h->spt_min_len + 1) * slots +
                          4 * ((run + kTile - 1) / kTile) * (kTile / h->spt_min_len + 1);
    if (h->spt_dev && worst <= kSpDeviceBudget && 16 * (run / h->spt_min_len + 1) <= (int64_t)1 << 31) {
      HostSpecials sp;
      sp.dev = true;
      sp.n = 1;
      for (int64_t k = 0; k < specials->n; ++k)
        if (specials->ids[k] > 0xFFFD) sp.narrow = false;
      return encode_batch_impl(h, bytes, str_off, n_str, pattern, chunk_bits, sp, out_ids, out_cap, out_off, stats);
    }
  }
  const int64_t cnt = sw_find_specials_host(bytes, str_off, n_str, specials, nullptr, nullptr, nullptr, 0, 0);
  if (cnt < 0) return fail((int32_t)cnt, "sw_encode_batch_ex: bad special tokens or string offsets");
  std::vector<int64_t> pos((size_t)std::max<int64_t>(cnt, 1));
  std::vector<int32_t> len(pos.size()), id(pos.size());
  if (cnt > 0) {
    const int64_t got = sw_find_specials_host(bytes, str_off, n_str, specials, pos.data(), len.data(), id.data(), cnt, 0);
    if (got != cnt) return fail(SW_ERR_ARG, "sw_encode_batch_ex: special-token scan");
  }
  HostSpecials sp;
  sp.pos = pos.data(); sp.len = len.data(); sp.id = id.data(); sp.n = cnt;
  for (int64_t k = 0; k < cnt; ++k)
    if (id[(size_t)k] > 0xFFFD) sp.narrow = false;
  return encode_batch_impl(h, bytes, str_off, n_str, pattern, chunk_bits, sp, out_ids, out_cap, out_off, stats);
}
