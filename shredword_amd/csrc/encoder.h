// The encoder handle and what its two units share (encode.hip: the C-ABI, the options and the
// device launch sequence; encode_batch.hip: the host batch path).  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "args.h"
#include "capi.h"
#include "chunktable.h"
#include "hostpool.h"
#include "shredword_hip.h"
#include "table.h"

namespace sw {

inline int32_t fail(int32_t code, const std::string& msg) { return set_error(code, msg); }
#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) return sw::fail(SW_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(e_)); \
  } while (0)

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// Move-only owner of one HIP object, released by Free in the destructor (with the device current
// that it was made on: sw_encoder_destroy).  Converts to the raw handle.
template <class H, hipError_t (*Free)(H)>
class Owned {
 public:
  Owned() = default;
  Owned(Owned&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); }
    return *this;
  }
  ~Owned() { reset(); }
  void reset() { if (p_) (void)Free(std::exchange(p_, nullptr)); }
  H get() const { return p_; }
  operator H() const { return p_; }

 protected:
  H p_ = nullptr;
};
template <class T> inline hipError_t free_device(T* p) { return hipFree((void*)p); }
template <class T> inline hipError_t free_pinned(T* p) { return hipHostFree((void*)p); }

// device memory: reset(n) frees, then allocates n elements
template <class T>
struct DevBuf : Owned<T*, free_device<T>> {
  using Owned<T*, free_device<T>>::reset;
  hipError_t reset(size_t n) {
    reset();
    return hipMalloc((void**)&this->p_, n * sizeof(T));
  }
};
// pinned (or, by its flags, mapped) host memory
template <class T>
struct PinnedBuf : Owned<T*, free_pinned<T>> {
  using Owned<T*, free_pinned<T>>::reset;
  hipError_t reset(size_t n, unsigned flags = hipHostMallocDefault) {
    reset();
    return hipHostMalloc((void**)&this->p_, n * sizeof(T), flags);
  }
};
// streams and events: made on first use
struct Stream : Owned<hipStream_t, hipStreamDestroy> {
  hipError_t ensure() { return p_ ? hipSuccess : hipStreamCreateWithFlags(&p_, hipStreamNonBlocking); }
};
struct Event : Owned<hipEvent_t, hipEventDestroy> {
  hipError_t ensure(unsigned flags = hipEventDisableTiming) { return p_ ? hipSuccess : hipEventCreateWithFlags(&p_, flags); }
};

// timing: one event pair per measured span since sw_encoder_set_timing(h, 1)
struct EventPairs {
  std::vector<Event> ev;
  size_t used = 0;  // pairs recorded
  // the events of the next pair; the caller records both and then counts the pair (++used)
  hipError_t next(hipEvent_t* begin, hipEvent_t* end) {
    while (ev.size() < 2 * (used + 1)) {
      ev.emplace_back();
      const hipError_t e = ev.back().ensure(hipEventDefault);
      if (e != hipSuccess) { ev.pop_back(); return e; }
    }
    *begin = ev[2 * used];
    *end = ev[2 * used + 1];
    return hipSuccess;
  }
  // the recorded pairs' mean time (synchronises on the last one); -1 if none or on an error
  double mean_ms() const {
    if (used == 0 || hipEventSynchronize(ev[2 * used - 1]) != hipSuccess) return -1.0;
    double sum = 0;
    for (size_t i = 0; i < used; ++i) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]) != hipSuccess) return -1.0;
      sum += ms;
    }
    return sum / (double)used;
  }
};

// The launch workspace, sized for cap_bytes input bytes and reused by every call (a call on
// another stream waits for the last one: sw_encoder::ws_done).
struct Workspace {
  int64_t cap_bytes = -1;
  DevBuf<int32_t> d_scratch;
  DevBuf<uint32_t> d_res;             // [2 * n_bytes] merge results, double-spaced position space
  DevBuf<int64_t> d_part;
  DevBuf<int64_t> d_tile_slo;
  DevBuf<int64_t> d_tile_sp;          // first special-token occurrence at or after each tile
  DevBuf<uint32_t> d_tile_slots;
  DevBuf<uint32_t> d_tile_nref;
  DevBuf<uint32_t> d_rlist;
  DevBuf<uint64_t> d_queue;           // dense merge queue (bucket-major)
  DevBuf<uint32_t> d_bcnt;            // [kNumBuckets * n_tiles] queued chunks per (bucket, tile)
  DevBuf<int64_t> d_boff;             // its exclusive scan
  DevBuf<int64_t> d_qtotal;
  DevBuf<unsigned long long> d_stamps;  // SW_STAMPS builds
  DevBuf<uint64_t> d_dtab;            // chunk dedupe table (sw_encoder::dd_slots entries)
  DevBuf<unsigned long long> d_ddfull;  // per launch: dedupable chunks that found every candidate taken
  DevBuf<uint4> d_dres;               // dense result heads, one per table entry
  DevBuf<uint8_t> d_dcnt;             // their id counts (<= 32), one byte per table entry
  DevBuf<uint32_t> d_big;             // chunks over kLongLds bytes: count, then their long-list indices
  // long chunks by split + verify (long_split.h): per long chunk, per piece, piece ids, counters
  DevBuf<char> d_lp;                  // one allocation, carved into LongArgs
  LongArgs lp{};
  DevBuf<int64_t> d_lpart;            // scan partials for the piece / chunk scans
  DevBuf<uint64_t> d_pbits;           // [n_bytes / 64] device pre-split bitmap
  DevBuf<uint32_t> d_edge;            // [kEdgeWords][n_tiles + 1] k_edges: the tile boundaries' masks and words
  DevBuf<unsigned int> d_redo;        // k_split_classify's tiles for k_split_redo: count, then the list (int64)
  DevBuf<unsigned long long> d_pcount;
  DevBuf<uint64_t> d_llist;           // k_classify's long chunks (EncArgs::llist) and their count
  DevBuf<unsigned long long> d_lcount;
  DevBuf<uint32_t> d_tile_cnt;
  DevBuf<int64_t> d_tile_base;
  DevBuf<int64_t> d_total;
};

// sw_encode_batch's device staging for one launch, grown on demand
struct IoStaging {
  int64_t io_bytes = -1, io_str = -1;
  DevBuf<uint8_t> d_bytes;
  DevBuf<int64_t> d_str_off;
  DevBuf<uint64_t> d_bits;
  DevBuf<int32_t> d_out;
  DevBuf<int64_t> d_out_off;
  int64_t sp_cap = 0;                 // special-token occurrences staged for sw_encode_batch_ex
  DevBuf<int64_t> d_sp_pos;
  DevBuf<int32_t> d_sp_len;
  DevBuf<int32_t> d_sp_id;
};

// one slot of sw_encode_batch's pipeline: a run's buffers, sized for cap_bytes / cap_str ...
struct PipeBufs {
  int64_t cap_bytes = 0, cap_str = 0;
  PinnedBuf<uint8_t> h_in; PinnedBuf<int64_t> h_off; PinnedBuf<uint64_t> h_bits;
  PinnedBuf<int32_t> h_out; PinnedBuf<int64_t> h_oo; PinnedBuf<int64_t> h_ntok;
  DevBuf<uint8_t> d_in; DevBuf<int64_t> d_off; DevBuf<uint64_t> d_bits;
  DevBuf<int32_t> d_out; DevBuf<int64_t> d_oo; DevBuf<uint16_t> d_out16;
  DevBuf<int64_t> d_ntok;  // this run's token count, kept apart from the shared workspace
};
// ... its special-token occurrences and its events
struct PipeSlot : PipeBufs {
  PinnedBuf<int64_t> h_sp; DevBuf<int64_t> d_sp;  // pos | len, id (3 x cap_sp x 8 B)
  int64_t cap_sp = 0;
  Event e_in, e_comp, e_out;
};

// special-token occurrences of one launch, on the device (sw_encode_ex)
struct DevSpecials {
  const int64_t* pos = nullptr;
  const int32_t* len = nullptr;
  const int32_t* id = nullptr;
  int64_t n = 0;                    // the count, or (n_dev given) the arrays' capacity
  const int64_t* n_dev = nullptr;   // the count in device memory (sw_find_specials_device)
};

}  // namespace sw

// Members are destroyed last to first, with the encoder's device current (sw_encoder_destroy):
// the streams come first so that every buffer and event is released before them.
struct sw_encoder {
  int device = 0;
  sw::Stream stream, s_h2d, s_d2h;
  // the merge kernels of different length buckets are independent: forked onto these streams
  // they overlap (each alone leaves most of the chip idle), joined before k_tile_count
  sw::Stream s_fork[2];
  bool merge_fork = true;             // SW_OPT_MERGE_STREAMS
  sw::Event ev_fork, ev_join[2];
  sw::Event ev_fork_long;             // (the long chunks' fork, right after k_classify)
  sw::DevTable table{};
  sw::DevBuf<char> d_table;
  int64_t n_merges = 0;
  bool ids16 = false;  // every pair member and value <= 0xFFFD: 16-bit ids in the kernels
  sw::DevChunkTable chunks{};
  sw::DevBuf<char> d_chunks;
  int64_t n_chunk_entries = 0;
  int64_t chunk_table_bytes = 0;
  // split + verify for long chunks (long_split.h): well-formed tables only
  bool split_ok = false;              // values >= 256, unique, larger than both pair members
  bool long_split = true;             // SW_OPT_LONG_SPLIT (0: the wave loop per long chunk)
  sw::DevBuf<uint2> d_inv;            // merge value -> pair
  uint32_t n_inv = 0;
  int64_t max_launch = sw::kMaxLaunchBytes;  // SW_OPT_MAX_LAUNCH_BYTES (sw_encode_batch splits above it)
  int n_cu = 256;                     // compute units (persistent grids)
  // the workspace is reused by every call: a call on another stream waits for the last one
  sw::Workspace ws;
  sw::Event ws_done;
  hipStream_t ws_stream = nullptr;
  bool ws_pending = false;
  int64_t last_tiles = 0;             // tiles of the last sw_encode_device launch (sw_encoder_last_counts)
  // sw_encode_batch's pipeline for large host batches (SW_OPT_PIPE_RUN_BYTES): runs of whole
  // strings go host -> pinned -> device -> encode -> (16-bit ids when they fit) -> pinned -> host,
  // run k's copies overlapping run k-1's encode; two slots of buffers
  struct Pinned {                     // sw_encoder_pin_host: a caller's range and its device address
    char* h = nullptr;
    int64_t n = 0;
    char* d = nullptr;
  };
  std::vector<Pinned> pins;
  sw::DevBuf<int64_t> d_done;         // the direct push (pinned caller arrays): ids written so far, overflow flag
  // (device address of [p, p + n) when it lies in a pinned range, else nullptr)
  void* pinned_dev(const void* p, int64_t n) const {
    for (const Pinned& r : pins)
      if ((const char*)p >= r.h && (const char*)p + n <= r.h + r.n) return r.d + ((const char*)p - r.h);
    return nullptr;
  }
  sw::PipeSlot pipe[4];
  int pipe_depth = 3;                 // SW_OPT_PIPE_DEPTH: runs in flight (slots)
  int64_t pipe_run = 128LL << 20;     // run size; batches over 2 runs take the pipeline (0: never; 128 MiB: e2e
                                      // 28.2 -> 30.1 GB/s pageable, 29.9 -> 31.8 pinned input against 64 MiB, r4z)
  bool pipe_kcopy = true;             // SW_OPT_PIPE_COPY_KERNELS
  std::unique_ptr<sw::HostPool> pool;
  sw::IoStaging io;                   // host-path staging
  uint32_t dmask = 0;
  int64_t dd_slots = 0;               // entries of ws.d_dtab (grown by grow_dedupe, kept across workspace reallocations)
  sw::PinnedBuf<unsigned long long> h_ddfull;  // ws.d_ddfull, its id count and merge loops, published by k_string_offsets (host-mapped, coherent)
  unsigned long long* hd_ddfull = nullptr;     // (its device address)
  bool dedupe = true;
  bool dedupe_exact = true;           // SW_OPT_DEDUPE_EXACT
  int64_t dedupe_slots = 0;           // SW_OPT_DEDUPE_SLOTS (0: automatic)
  bool dd_grow_stop = false;          // a growth allocation failed: keep the table that works
  int32_t test_fail_grow = 0;         // SW_OPT_TEST_FAIL_GROWTH: the next growth's allocations fail (tests)
  int32_t pattern = SW_PAT_CL100K;    // SW_OPT_PATTERN: device pre-split of sw_encode_device(bits = NULL)
  bool host_presplit = false;         // SW_OPT_HOST_PRESPLIT: sw_encode_batch pre-splits on the host
  bool fused_presplit = true;         // SW_OPT_FUSED_PRESPLIT: the device pre-split inside k_split_classify
  bool device_specials = true;        // SW_OPT_DEVICE_SPECIALS: sw_encode_batch_ex finds specials on the device
  int compact_kernel = 0;             // SW_OPT_COMPACT_KERNEL (0: from the last launch's ids per tile)
  int staged_heads = 0;               // SW_OPT_STAGED_HEADS: 0 automatic (a grown dedupe table), 1 always, 2 never
  int64_t cp_prev_tiles = 0;          // tiles of the previous launch (its id count: h_ddfull[1])
  uint32_t dedupe_fp_mask = (1u << 26) - 1;
  // the device special-token finder (specials_find.h): the specials' table, keyed by content, and
  // its per-tile work arrays
  sw::DevBuf<char> d_spt;
  sw::SpTab spt{};
  std::string spt_key;                // the specials the table holds (bytes, offsets, ids)
  bool spt_dev = false;               // every special fits the device finder (<= kSpMaxLen bytes)
  int32_t spt_min_len = 1;            // the shortest non-empty special
  int64_t spf_tiles = 0;              // capacity of the finder's arrays, in tiles
  int64_t spf_tcap = 0;               // ... and occurrences per tile
  sw::DevBuf<uint32_t> d_spf;         // candidate bits, occurrence bits, per-tile counts, flag
  sw::DevBuf<uint32_t> d_spf_list;    // per tile, its occurrences (k_sp_find)
  sw::DevBuf<int64_t> d_spf_off;      // per-tile occurrence offsets, twice (+ scan partials, totals)
  sw::DevBuf<int64_t> d_nsp;          // sw_encode_batch_ex: the finder's count
  // dominant-kernel timing since sw_encoder_set_timing(h, 1): the whole pipeline of each launch,
  // and its classification kernel alone
  bool timing = false;
  sw::EventPairs ev_pool, ev_cls;
};

namespace sw {

// encode.hip, for the host batch path
int32_t ensure_workspace(sw_encoder* h, int64_t n_bytes);
int32_t set_specials(sw_encoder* h, const sw_specials* sp);
int32_t find_specials_device(sw_encoder* h, const uint8_t* d_bytes, int64_t n_bytes, const int64_t* d_str_off,
                             int64_t n_str, int64_t* d_pos, int32_t* d_len, int32_t* d_id, int64_t cap, int64_t* d_count,
                             hipStream_t st);
// the device pipeline; d_out_ids is int32_t*, or uint16_t* when out16 (the table is ids16)
int32_t encode_device(sw_encoder* h, const uint8_t* d_bytes, int64_t n_bytes, const int64_t* d_str_off, int64_t n_str,
                      const uint64_t* d_chunk_bits, const DevSpecials& sp, void* d_out_ids, bool out16,
                      int64_t* d_out_off, void* stream, int64_t* n_tokens_host, int32_t pattern_call = -1);
// chunk starts of a pre-split bitmap, added to *d_count (k_popcount)
void launch_popcount(hipStream_t st, const uint64_t* d_bits, int64_t n_words, unsigned long long* d_count);

}  // namespace sw
