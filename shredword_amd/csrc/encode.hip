// MI355X (gfx950) batched BPE encode: kernels + host orchestration + the C-ABI.
//
// Semantics (exact, for ANY merge table): per pre-split chunk, ids = chunk bytes; while at
// least two ids remain, find the adjacent pair with the lowest merges-value (first occurrence
// wins ties), stop if no pair is in merges, else replace every non-overlapping occurrence of
// that pair, left to right, by the value.  This is the loop the reference's primitives
// compose: get_stats (shredword/base.py:10-20), min over merges.get (base.py:107-108 leaves
// encode abstract), merge (base.py:22-36).
//
// Device pipeline (all on one stream; inputs resident in HBM; kernels in kernels.h):
//   k_tile_strings   first string of each tile
//   k_classify       per 2 KiB tile: single bytes + whole-chunk-table hits settled, one slot
//                    per chunk, repeats of a multi-token chunk deduped, the rest queued by
//                    length bucket
//   k_scan_*/k_scatter  dense bucket-major merge queue
//   k_merge_bucket   exact merge loop of the distinct queued chunks, one chunk per lane, in
//                    registers (N = 4/8/16/32)
//   k_merge_long     wave-cooperative merge loop for chunks > 32 bytes
//   k_tile_count     ids per tile, then k_scan_* for the tile bases
//   k_compact        slots -> contiguous ids; string chunk index -> id offset
//   k_string_offsets final per-string offsets
//
// The handle and what this unit shares with the host batch path (encode_batch.hip): encoder.h.
// The pair table is built on the host by pairtable.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "encoder.h"
#include "kernels.h"
#include "long_split.h"
#include "pairtable.h"
#include "presplit_kernel.h"
#include "split_classify.h"
#include "specials_find.h"
#include "test_options.h"

using namespace sw;

// ------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------
static thread_local std::string g_err;
int32_t sw::set_error(int32_t code, const std::string& msg) {
  g_err = msg;
  return code;
}

extern "C" const char* sw_last_error(void) { return g_err.c_str(); }
extern "C" const char* sw_version(void) { return "shredword_hip 0.1 gfx950"; }
extern "C" int32_t sw_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

constexpr unsigned long long kStagedMinMerges = 6000000;  // (see make_args: k_tile_count_staged)

int32_t sw::ensure_workspace(sw_encoder* h, int64_t n_bytes) {
  if (n_bytes <= h->ws.cap_bytes) return SW_OK;
  h->ws = Workspace{};
  const int64_t nb = std::max<int64_t>(n_bytes, 1);
  const int64_t n_tiles = (nb + kTile - 1) / kTile;
  HIP_TRY(h->ws.d_scratch.reset(n_tiles * kTile));  // whole tiles: see k_compact
  // (+ slack for k_compact's head reads; k_classify's tile-local queue, aliased here, takes whole tiles)
  HIP_TRY(h->ws.d_res.reset(std::max<int64_t>(2 * nb + 16, n_tiles * kTile)));
  HIP_TRY(h->ws.d_tile_slo.reset(n_tiles));
  HIP_TRY(h->ws.d_tile_sp.reset(2 * (n_tiles + 1)));  // (tile_sp, then tile_spw)
  HIP_TRY(h->ws.d_tile_slots.reset(n_tiles));
  HIP_TRY(h->ws.d_tile_nref.reset(n_tiles));
  HIP_TRY(h->ws.d_rlist.reset(n_tiles * kTile));
  // queued chunks have >= 2 bytes: at most nb / 2 of them
  HIP_TRY(h->ws.d_queue.reset(nb / 2 + 64));
  HIP_TRY(h->ws.d_bcnt.reset(kNumBuckets * n_tiles));
  HIP_TRY(h->ws.d_boff.reset(kNumBuckets * n_tiles));
  HIP_TRY(h->ws.d_qtotal.reset(1));
  HIP_TRY(h->ws.d_part.reset((kNumBuckets * n_tiles + kScanBlock - 1) / kScanBlock + 1));
  {  // dedupe table: ~1 entry per 64 input bytes, 2^6 .. 2^22 entries (64 MiB) to start with, more
     // when a launch overflows it (grow_dedupe), and a 16-byte result head + a count byte per entry
    int64_t slots = 64;
    while (slots < nb / 64 && slots < kDdSlotsDefault) slots <<= 1;
    slots = std::max(slots, h->dd_slots);
    h->dd_slots = slots;
    HIP_TRY(h->ws.d_dtab.reset(kDdWords * slots));
    HIP_TRY(h->ws.d_dres.reset(slots));
    HIP_TRY(h->ws.d_dcnt.reset(slots));
    h->dmask = (uint32_t)(slots - 1);
  }
  HIP_TRY(h->ws.d_big.reset(nb / (kLongLds + 1) + 2));  // (count + list)
  {  // long_split.h: a long chunk has > kShort bytes and ceil(len / kPieceW) pieces
    const int64_t lcap = nb / (kShort + 1) + 64, pcap = nb / kPieceW + lcap;  // (ceil(len / W) pieces a chunk)
    const size_t bytes = 8 * (size_t)kLcAlloc + 4 * (size_t)lcap * 7 + 8 * (size_t)lcap  // chunks
                         + 4 * (size_t)pcap * 11                                         // pieces, lists
                         + 4 * (size_t)(nb + 64) + 4 * (size_t)pcap + 1024;             // ids, window list (+ alignment)
    HIP_TRY(h->ws.d_lp.reset(bytes));
    char* q = h->ws.d_lp;
    auto take = [&](size_t n) { char* r = q; q += (n + 15) & ~(size_t)15; return (void*)r; };
    LongArgs& L = h->ws.lp;
    L.ctl = (int64_t*)take(8 * (size_t)kLcAlloc);
    L.lpo = (int64_t*)take(8 * (size_t)lcap);
    L.lstart = (uint32_t*)take(4 * (size_t)lcap); L.llen = (uint32_t*)take(4 * (size_t)lcap);
    L.lnp = (uint32_t*)take(4 * (size_t)lcap); L.lfall = (uint32_t*)take(4 * (size_t)lcap);
    L.flist = (uint32_t*)take(4 * (size_t)lcap);
    L.wstart = (uint32_t*)take(4 * (size_t)lcap); L.wlen = (uint32_t*)take(4 * (size_t)lcap);
    L.pbeg = (uint32_t*)take(4 * (size_t)pcap); L.pcnt = (uint32_t*)take(4 * (size_t)pcap);
    L.pchunk = (uint32_t*)take(4 * (size_t)pcap); L.pflag = (uint32_t*)take(4 * (size_t)pcap);
    L.pprev = (uint32_t*)take(4 * (size_t)pcap); L.pnext = (uint32_t*)take(4 * (size_t)pcap);
    L.jlist[0] = (uint32_t*)take(4 * (size_t)pcap); L.jlist[1] = (uint32_t*)take(4 * (size_t)pcap);
    L.clist = (uint32_t*)take(4 * (size_t)pcap); L.hlist = (uint32_t*)take(4 * (size_t)pcap);
    L.pseen = (uint32_t*)take(4 * (size_t)pcap);
    L.pid = (uint32_t*)take(4 * (size_t)(nb + 64));
    L.wlist = (uint32_t*)take(4 * (size_t)pcap);
    L.lcap = lcap;
    L.pcap = pcap;
    HIP_TRY(h->ws.d_lpart.reset(kDscanGrid));
  }
  HIP_TRY(h->ws.d_tile_base.reset(n_tiles));
  HIP_TRY(h->ws.d_tile_cnt.reset(n_tiles));
  HIP_TRY(h->ws.d_total.reset(1));
  HIP_TRY(h->ws.d_pbits.reset((nb + 63) / 64));
  HIP_TRY(h->ws.d_edge.reset(kEdgeWords * (n_tiles + 1)));
  HIP_TRY(h->ws.d_redo.reset(2 * (n_tiles + 1)));
  HIP_TRY(h->ws.d_pcount.reset(1));
  HIP_TRY(h->ws.d_ddfull.reset(1));
  HIP_TRY(h->ws.d_llist.reset(nb / (kShort + 1) + 64));
  HIP_TRY(h->ws.d_lcount.reset(1));
  HIP_TRY(hipMemset(h->ws.d_ddfull, 0, sizeof(unsigned long long)));
#ifdef SW_STAMPS
  HIP_TRY(h->ws.d_stamps.reset(32 * 64));  // 64 copies per counter
  HIP_TRY(hipMemset(h->ws.d_stamps, 0, sizeof(unsigned long long) * 32 * 64));
#endif
  h->ws.cap_bytes = nb;
  return SW_OK;
}

// device pre-split of [d_bytes, d_bytes + n_bytes) into d_bits (every dword of the bitmap is
// stored: no clearing)
static hipError_t launch_presplit(hipStream_t st, const uint8_t* d_bytes, int64_t n_bytes, const int64_t* d_str_off,
                           int64_t n_str, int32_t pattern, uint64_t* d_bits, const int64_t* d_tile_slo) {
  if (n_bytes <= 0) return hipSuccess;
  PbArgs g{d_bytes, n_bytes, d_str_off, n_str, d_tile_slo};
  hipLaunchKernelGGL(k_presplit_bits, dim3((unsigned)((n_bytes + kPbBlock - 1) / kPbBlock)), dim3(kPbThreads), 0, st, g,
                     (int)pattern, (uint32_t*)d_bits);
  return hipGetLastError();
}

// exclusive scan of cnt[0..n) into base, total into *total (two small kernels: the blocks' sums,
// then each block's scan behind the sum of the sums before it)
hipError_t sw::launch_scan(hipStream_t st, const uint32_t* cnt, int64_t n, int64_t* part, int64_t* base,
                           int64_t* total, const int64_t* n_dev) {
  const int64_t n_parts = (n + kScanBlock - 1) / kScanBlock;
  if (n_parts == 0) {
    (void)hipMemsetAsync(total, 0, sizeof(int64_t), st);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_scan_reduce, dim3((unsigned)n_parts), dim3(kThreads), 0, st, cnt, n, n_dev, part);
  hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)n_parts), dim3(kThreads), 0, st, cnt, n, n_dev, part, base, total);
  return hipGetLastError();
}
int64_t sw::scan_block() { return kScanBlock; }

extern "C" int32_t sw_encoder_create(const int32_t* pairs, const int32_t* vals, int64_t n, int32_t device,
                                     sw_encoder** out) {
  if (!out || n < 0 || (n > 0 && (!pairs || !vals))) return fail(SW_ERR_ARG, "sw_encoder_create: bad arguments");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(SW_ERR_NODEV, "sw_encoder_create: no HIP device visible");
  if (device < 0 || device >= ndev) return fail(SW_ERR_ARG, "sw_encoder_create: bad device ordinal");
  // on the host: the pair table (pairtable.cpp), then the whole-chunk table from its dict
  PairTableHost pt;
  const int32_t rc = build_pair_table(pairs, vals, n, &pt);
  if (rc) return fail(rc, pt.error);
  ChunkTableHost ct;
  if (!build_chunk_table(pt.dict, pt.order, &ct))
    return fail(SW_ERR_ALLOC, "sw_encoder_create: could not build the chunk table");
  // the upload
  sw_encoder* h = new sw_encoder();
  h->device = device;
  h->n_merges = (int64_t)pt.order.size();
  h->split_ok = pt.split_ok;
  h->ids16 = pt.ids16;
  h->table = pt.table;
  h->n_chunk_entries = (int64_t)(ct.n_short + ct.n_long);
  DeviceGuard g(device);
  {
    int cu = 0;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cu > 0) h->n_cu = cu;
  }
  const size_t table_bytes = pt.buckets.size() * sizeof(uint32_t), inv_bytes = pt.inv.size() * sizeof(uint32_t);
  const size_t sb = ct.sb.size() * sizeof(uint4), lb = ct.lb.size() * sizeof(uint4);
  hipError_t e = h->stream.ensure();
  if (e == hipSuccess) e = h->d_table.reset(table_bytes);
  if (e == hipSuccess) e = hipMemcpy(h->d_table, pt.buckets.data(), table_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = h->d_chunks.reset(sb + lb);
  if (e == hipSuccess) e = hipMemcpy(h->d_chunks, ct.sb.data(), sb, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(h->d_chunks + sb, ct.lb.data(), lb, hipMemcpyHostToDevice);
  if (e == hipSuccess && h->split_ok) {
    e = h->d_inv.reset(pt.inv.size() / 2);
    if (e == hipSuccess) e = hipMemcpy(h->d_inv, pt.inv.data(), inv_bytes, hipMemcpyHostToDevice);
    h->n_inv = (uint32_t)(pt.inv.size() / 2);
  }
  if (e == hipSuccess) e = h->ws_done.ensure();
  if (e == hipSuccess)  // (the dedupe overflow count of the last launch, written by the device)
    e = h->h_ddfull.reset(3, hipHostMallocMapped | hipHostMallocCoherent);
  if (e == hipSuccess) {
    h->h_ddfull[0] = 0;  // (and [1]: the last launch's id count)
    h->h_ddfull[1] = 0;
    h->h_ddfull[2] = 0;  // (and [2]: its merge loops)
    e = hipHostGetDevicePointer((void**)&h->hd_ddfull, h->h_ddfull, 0);
  }
  if (e != hipSuccess) {
    sw_encoder_destroy(h);
    return fail(SW_ERR_HIP, std::string("sw_encoder_create: ") + hipGetErrorString(e));
  }
  h->table.buckets = h->d_table;
  h->chunk_table_bytes = (int64_t)(sb + lb);
  h->chunks.sb = (const uint4*)h->d_chunks.get();
  h->chunks.lb = (const uint4*)(h->d_chunks + sb);
  h->chunks.s_shift = ct.s_shift; h->chunks.s_m1 = ct.s_m1; h->chunks.s_m2 = ct.s_m2;
  h->chunks.l_shift = ct.l_shift; h->chunks.l_m1 = ct.l_m1; h->chunks.l_m2 = ct.l_m2;
  h->chunks.enabled = 1;
  *out = h;
  return SW_OK;
}

// Every stream this encoder has work on, idle: its own (launch, copy-in, copy-out, merge forks) and
// the caller's stream of its last device-entry launch (its ws_done event, recorded after that
// launch's last kernel and after the finder's).  Before anything is freed or unpinned: round 4's
// destroy freed first and synchronised only the launch stream.  Other encoders and
// the caller's unrelated work are not waited for.
static hipError_t drain_own(sw_encoder* h) {
  hipError_t e = hipSuccess;
  auto take = [&](hipError_t x) { if (e == hipSuccess) e = x; };
  if (h->ws_done) take(hipEventSynchronize(h->ws_done));
  for (hipStream_t s : {h->stream.get(), h->s_h2d.get(), h->s_d2h.get(), h->s_fork[0].get(), h->s_fork[1].get()})
    if (s) take(hipStreamSynchronize(s));
  return e;
}

extern "C" void sw_encoder_destroy(sw_encoder* h) {
  if (!h) return;
  DeviceGuard g(h->device);
  (void)drain_own(h);  // (every stream of this encoder idle before anything is freed or unpinned)
  for (const auto& r : h->pins) (void)hipHostUnregister((void*)((uintptr_t)r.h & ~(uintptr_t)4095));
  // with the encoder's device still current: the members free their memory, then their events,
  // the streams last (sw_encoder's member order)
  delete h;
}

extern "C" int32_t sw_encoder_pin_host(sw_encoder* h, void* ptr, int64_t bytes) {
  if (!h || !ptr || bytes <= 0) return fail(SW_ERR_ARG, "sw_encoder_pin_host: bad arguments");
  DeviceGuard g(h->device);
  for (const auto& r : h->pins)  // (whole pages: two ranges may not share one)
    if (((uintptr_t)ptr >> 12) <= (((uintptr_t)r.h + r.n - 1) >> 12) && (((uintptr_t)ptr + bytes - 1) >> 12) >= ((uintptr_t)r.h >> 12))
      return fail(SW_ERR_ARG, "sw_encoder_pin_host: shares a page with a pinned range");
  // (whole pages registered: a large numpy / malloc block starts 16 bytes into its first page)
  const uintptr_t pg = 4096, a0 = (uintptr_t)ptr & ~(pg - 1), a1 = ((uintptr_t)ptr + (uintptr_t)bytes + pg - 1) & ~(pg - 1);
  HIP_TRY(hipHostRegister((void*)a0, (size_t)(a1 - a0), hipHostRegisterMapped));
  void* d = nullptr;
  const hipError_t e = hipHostGetDevicePointer(&d, (void*)a0, 0);
  if (e != hipSuccess) {
    (void)hipHostUnregister((void*)a0);
    return fail(SW_ERR_HIP, std::string("sw_encoder_pin_host: ") + hipGetErrorString(e));
  }
  h->pins.push_back(sw_encoder::Pinned{(char*)ptr, bytes, (char*)d + ((uintptr_t)ptr - a0)});
  return SW_OK;
}

extern "C" int32_t sw_encoder_unpin_host(sw_encoder* h, void* ptr) {
  if (!h || !ptr) return fail(SW_ERR_ARG, "sw_encoder_unpin_host: bad arguments");
  DeviceGuard g(h->device);
  for (size_t i = 0; i < h->pins.size(); ++i) {
    if (h->pins[i].h != (char*)ptr) continue;
    // (nothing of this encoder may still read or write it -- a write into the range still in flight
    // when its mapping goes faults the device -- and only this encoder's streams touch its pins)
    HIP_TRY(drain_own(h));
    HIP_TRY(hipHostUnregister((void*)((uintptr_t)ptr & ~(uintptr_t)4095)));
    h->pins.erase(h->pins.begin() + (long)i);
    return SW_OK;
  }
  return fail(SW_ERR_ARG, "sw_encoder_unpin_host: not a pinned range");
}

extern "C" int32_t sw_encoder_reserve(sw_encoder* h, int64_t max_bytes, int64_t max_strings) {
  if (!h || max_bytes < 0 || max_strings < 0) return fail(SW_ERR_ARG, "sw_encoder_reserve: bad arguments");
  DeviceGuard g(h->device);
  return ensure_workspace(h, max_bytes);
}

extern "C" int32_t sw_encoder_set_option(sw_encoder* h, int32_t option, int64_t value) {
  if (!h) return fail(SW_ERR_ARG, "sw_encoder_set_option: null handle");
  switch (option) {
    case SW_OPT_CHUNK_TABLE: h->chunks.enabled = value ? 1u : 0u; return SW_OK;
    case SW_OPT_DEDUPE: h->dedupe = value != 0; return SW_OK;
    case SW_OPT_PATTERN:
      if (value != SW_PAT_CL100K && value != SW_PAT_GPT2 && value != SW_PAT_NONE) return fail(SW_ERR_ARG, "bad pattern");
      h->pattern = (int32_t)value;
      return SW_OK;
    case SW_OPT_HOST_PRESPLIT: h->host_presplit = value != 0; return SW_OK;
    case SW_OPT_DEDUPE_SLOTS:
      if (value != 0 && (value < 8 || (value & (value - 1)))) return fail(SW_ERR_ARG, "dedupe slots: 0 or a power of two >= 8");
      h->dedupe_slots = value;
      return SW_OK;
    case SW_OPT_DEDUPE_FP_BITS:
      if (value < 0 || value > 26) return fail(SW_ERR_ARG, "dedupe fingerprint bits: 0..26");
      h->dedupe_fp_mask = (uint32_t)((1ULL << value) - 1);
      return SW_OK;
    case SW_OPT_DEDUPE_EXACT: h->dedupe_exact = value != 0; return SW_OK;
    case SW_OPT_LONG_SPLIT: h->long_split = value != 0; return SW_OK;
    case SW_OPT_PIPE_COPY_KERNELS: h->pipe_kcopy = value != 0; return SW_OK;
    case SW_OPT_MERGE_STREAMS: h->merge_fork = value != 0; return SW_OK;
    case SW_OPT_FUSED_PRESPLIT: h->fused_presplit = value != 0; return SW_OK;
    case SW_OPT_TEST_FAIL_GROWTH: h->test_fail_grow = value ? 1 : 0; h->dd_grow_stop = false; return SW_OK;
    case SW_OPT_DEVICE_SPECIALS: h->device_specials = value != 0; return SW_OK;
    case SW_OPT_STAGED_HEADS:
      if (value < 0 || value > 2) return fail(SW_ERR_ARG, "staged heads: 0 (automatic), 1 (always) or 2 (never)");
      h->staged_heads = (int)value;
      return SW_OK;
    case SW_OPT_COMPACT_KERNEL:
      if (value < 0 || value > 3) return fail(SW_ERR_ARG, "SW_OPT_COMPACT_KERNEL: 0 .. 3");
      h->compact_kernel = (int)value;
      return SW_OK;
    case SW_OPT_PIPE_DEPTH:
      if (value < 2 || value > 4) return fail(SW_ERR_ARG, "pipeline depth: 2 .. 4");
      h->pipe_depth = (int)value;
      return SW_OK;
    case SW_OPT_PIPE_RUN_BYTES:
      if (value != 0 && value < 64) return fail(SW_ERR_ARG, "pipeline run bytes: 0 (off) or >= 64");
      h->pipe_run = std::min<int64_t>(value, kMaxLaunchBytes);
      return SW_OK;
    case SW_OPT_MAX_LAUNCH_BYTES:
      if (value != 0 && (value < 64 || value > kMaxLaunchBytes))
        return fail(SW_ERR_ARG, "max launch bytes: 0 (default) or 64 .. 2^30 - 64");
      h->max_launch = value ? value : kMaxLaunchBytes;
      return SW_OK;
    default: return fail(SW_ERR_ARG, "sw_encoder_set_option: unknown option");
  }
}

extern "C" int64_t sw_encoder_get_info(const sw_encoder* h, int32_t what) {
  if (!h) return SW_ERR_ARG;
  switch (what) {
    case SW_INFO_MERGES: return h->n_merges;
    case SW_INFO_CHUNK_ENTRIES: return h->n_chunk_entries;
    case SW_INFO_WIDE_TABLE: return h->table.wide;
    case SW_INFO_IDS16: return h->ids16 ? 1 : 0;
    case SW_INFO_SPLIT: return h->split_ok ? 1 : 0;
    case SW_INFO_DEDUPE_SLOTS: return h->dd_slots;
    case SW_INFO_CHUNK_TABLE_BYTES: return h->chunk_table_bytes;
    default: return SW_ERR_ARG;
  }
}

extern "C" int32_t sw_encoder_set_timing(sw_encoder* h, int32_t on) {
  if (!h) return fail(SW_ERR_ARG, "sw_encoder_set_timing: null handle");
  h->timing = on != 0;
  h->ev_pool.used = 0;
  h->ev_cls.used = 0;
  return SW_OK;
}

// Average device time of the classification kernel alone (k_split_classify, or k_classify with a
// caller's bitmap) over the launches recorded since the last sw_encoder_set_timing(h, 1): the
// pipeline's dominant kernel, for the per-kernel roofline (HIP events on the launch stream).
extern "C" double sw_encoder_last_classify_ms(const sw_encoder* h) {
  if (!h) return -1.0;
  DeviceGuard g(h->device);
  return h->ev_cls.mean_ms();
}

// Average device time of the whole sw_encode_device pipeline (k_tile_strings .. k_string_offsets) over the
// launches recorded since the last sw_encoder_set_timing(h, 1); synchronises on the last recorded event.
extern "C" double sw_encoder_last_kernel_ms(const sw_encoder* h) {
  if (!h) return -1.0;
  DeviceGuard g(h->device);
  return h->ev_pool.mean_ms();
}

// Diagnostic builds only (-DSW_STAMPS): cycles per pipeline phase summed over workgroups
// since the workspace was allocated (or the last reset).
extern "C" int32_t sw_encoder_phase_cycles(sw_encoder* h, double* out32, int32_t reset) {
#ifdef SW_STAMPS
  if (!h || !out32 || !h->ws.d_stamps) return fail(SW_ERR_ARG, "sw_encoder_phase_cycles: no workspace");
  DeviceGuard g(h->device);
  std::vector<unsigned long long> v(32 * 64);
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(v.data(), h->ws.d_stamps, sizeof(unsigned long long) * v.size(), hipMemcpyDeviceToHost));
  for (int i = 0; i < 32; ++i) {
    double sum = 0;
    for (int c = 0; c < 64; ++c) sum += (double)v[i * 64 + c];
    out32[i] = sum;
  }
  if (reset) HIP_TRY(hipMemset(h->ws.d_stamps, 0, sizeof(unsigned long long) * v.size()));
  return SW_OK;
#else
  (void)h; (void)out32; (void)reset;
  return fail(SW_ERR_ARG, "sw_encoder_phase_cycles: not a diagnostic (SW_STAMPS) build");
#endif
}

namespace {
// the long-chunk split + verify passes (long_split.h) on stream s: well-formed tables only
template <bool kWide, bool k16>
hipError_t launch_long_split(sw_encoder* h, hipStream_t s, const EncArgs& a, int part) {
  LongArgs& L = h->ws.lp;
  const dim3 g(kLpGrid), b(kThreads);
  if (part == 2) {  // (the passes that write res, where k_classify's tile-local queue lives until k_scatter)
    hipLaunchKernelGGL((k_lp_fallback<kWide, k16>), g, dim3(64), 0, s, a, L);
    hipLaunchKernelGGL(k_lp_gather, g, b, 0, s, a, L);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_dscan_reduce, dim3(kDscanGrid), b, 0, s, L.lnp, L.lcap, &L.ctl[kLcLong], h->ws.d_lpart);
  hipLaunchKernelGGL(k_dscan_parts, dim3(1), dim3(kDscanGrid), 0, s, h->ws.d_lpart, &L.ctl[kLcPieces]);
  hipLaunchKernelGGL(k_dscan_apply, dim3(kDscanGrid), b, 0, s, L.lnp, L.lcap, &L.ctl[kLcLong], h->ws.d_lpart, L.lpo);
  hipLaunchKernelGGL(k_lp_fill, g, b, 0, s, L);
  hipLaunchKernelGGL((k_lp_encode<kWide, k16>), g, b, 0, s, a, L);  // (and round 0's junctions)
  for (int r = 0; r < kLpRounds; ++r) {
    hipLaunchKernelGGL(k_lp_heads, g, b, 0, s, L, r);
    hipLaunchKernelGGL((k_lp_windows<kWide, k16>), g, b, 0, s, a, L, r);
    hipLaunchKernelGGL((k_lp_bigwin<kWide, k16>), g, dim3(64), 0, s, a, L, r);
    hipLaunchKernelGGL((k_lp_junctions<kWide>), g, b, 0, s, a, L, r + 1);  // (r + 1 == kLpRounds: the final check)
  }
  return hipGetLastError();
}

// every long chunk (> kShort bytes) on stream s, listed from the queue (k_lp_prep): split +
// verify over the whole GPU (long_split.h; well-formed tables), or the wave loop per chunk.
// (Started from the bitmap right after the pre-split, beside k_classify, they only slowed it
// down by as much: both fill the chip.  They run beside the merge kernels, which leave it
// mostly idle.)
// part 1 right after k_classify (its long list and the complete bitmap); part 2, the passes that
// write res, after k_scatter has consumed the tile-local queue aliased there (a.qtmp)
template <bool kWide, bool k16>
hipError_t launch_long(sw_encoder* h, hipStream_t s, const EncArgs& a, bool split, int part) {
  constexpr unsigned kLongGrid = 32768;  // k_merge_long_lds: a workgroup per long chunk (grid-stride past that)
  LongArgs& L = h->ws.lp;
  if (part == 2) {
    if (split) return launch_long_split<kWide, k16>(h, s, a, 2);
    hipLaunchKernelGGL((k_merge_long_lds<kWide, k16>), dim3(kLongGrid), dim3(64), 0, s, a);
    hipLaunchKernelGGL((k_merge_long<kWide>), dim3(512), dim3(kThreads), 0, s, a);  // (over kLongLds bytes)
    return hipGetLastError();
  }
  hipError_t e = hipMemsetAsync(L.ctl, 0, sizeof(int64_t) * kLcAlloc, s);
  if (e == hipSuccess) e = hipMemsetAsync(h->ws.d_big, 0, sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_lp_prep, dim3(kLpPrepGrid), dim3(kThreads), 0, s, a, L, split ? (int64_t)kShort : INT64_MAX);
  if (!split) return hipGetLastError();
  e = launch_long_split<kWide, k16>(h, s, a, 1);
#ifdef SW_LP_DEBUG
  if (e == hipSuccess && getenv("SW_LP_DEBUG")) {
    int64_t c[kLcAlloc];
    (void)hipStreamSynchronize(s);
    (void)hipMemcpy(c, L.ctl, sizeof(c), hipMemcpyDeviceToHost);
    fprintf(stderr, "lp: long %lld pieces %lld fall %lld\n", (long long)c[kLcLong], (long long)c[kLcPieces],
            (long long)c[kLcFall]);
    for (int r = 0; r <= kLpRounds; ++r)
      fprintf(stderr, "lp r%d: jun %lld conf %lld heads %lld big %lld big_bytes %lld big_max %lld\n", r,
              (long long)c[kLcJun + r], (long long)c[kLcConf + r], (long long)c[kLcHead + r], (long long)c[kLcBig + r],
              r < kLpRounds ? (long long)c[kLcDbg + r] : 0LL, r < kLpRounds ? (long long)c[kLcDbg + kLpRounds + r] : 0LL);
  }
#endif
  return e;
}

// The entries of the dedupe table a launch of n bytes uses: a prefix sized for its bytes -- 2^16 at
// least, one per 8 input bytes, at most what is allocated -- so that a small launch after a large
// one, or after the table has grown for a low-repetition corpus, clears kilobytes instead of the
// whole table (the 1 GiB launches use all of it: 2^22 entries by default, 2^24 grown)
int64_t launch_dd_slots(const sw_encoder* h, int64_t n_bytes) {
  int64_t want = 1LL << 16;
  while (want < n_bytes / 8 && want < h->dd_slots) want <<= 1;
  return std::min<int64_t>(want, h->dd_slots);
}

// A launch whose dedupe table overflowed (chunks that found all 8 candidates of their line taken,
// counted by the device and published to host memory by k_string_offsets) grows the table for
// the launches after it: to the power of two >= 2 x (entries + overflow), at most kDdSlotsMax.
// The count is read without waiting: a launch still running is seen by a later call.
// The new table is allocated beside the old one and swapped in only when all three buffers exist:
// growth is an optimisation, so an allocation failure keeps the table that works (and stops
// further attempts on this handle) instead of leaving the handle half-built.
int32_t grow_dedupe(sw_encoder* h, int64_t n_bytes) {
  if (launch_dd_slots(h, n_bytes) < h->dd_slots) return SW_OK;  // (a prefix launch: more entries would not serve it)
  const unsigned long long over = h->h_ddfull ? __atomic_load_n(h->h_ddfull.get(), __ATOMIC_ACQUIRE) : 0ULL;
  constexpr int64_t kGrowDiv = 32;  // (grow when more than slots / this many chunks found no entry)
  if (!h->ws.d_dtab || h->dedupe_slots || h->dd_grow_stop || over <= (unsigned long long)(h->dd_slots / kGrowDiv) ||
      h->dd_slots >= kDdSlotsMax)
    return SW_OK;  // (SW_OPT_DEDUPE_SLOTS caps the table on purpose: no growth)
  int64_t slots = h->dd_slots;
  while (slots < 2 * (h->dd_slots + (int64_t)over) && slots < kDdSlotsMax) slots <<= 1;
  DevBuf<uint64_t> dtab;
  DevBuf<uint4> dres;
  DevBuf<uint8_t> dcnt;
  const bool ok = !h->test_fail_grow && dtab.reset(kDdWords * slots) == hipSuccess &&
                  dres.reset(slots) == hipSuccess && dcnt.reset(slots) == hipSuccess;
  __atomic_store_n(h->h_ddfull.get(), 0ULL, __ATOMIC_RELEASE);
  if (!ok) {  // (what was allocated is freed on return)
    (void)hipGetLastError();  // (the failed allocation's status: not this launch's error)
    h->dd_grow_stop = true;
    return SW_OK;
  }
  // the old table may still be in use by the previous launch
  if (h->ws_pending) HIP_TRY(hipEventSynchronize(h->ws_done));
  h->ws.d_dtab = std::move(dtab);
  h->ws.d_dres = std::move(dres);
  h->ws.d_dcnt = std::move(dcnt);
  h->dd_slots = slots;
  h->dmask = (uint32_t)(slots - 1);
  return SW_OK;
}

}  // namespace

void sw::launch_popcount(hipStream_t st, const uint64_t* d_bits, int64_t n_words, unsigned long long* d_count) {
  hipLaunchKernelGGL(k_popcount, dim3(1024), dim3(256), 0, st, d_bits, n_words, d_count);
}

// the specials' table on the device (rebuilt only when the specials change)
int32_t sw::set_specials(sw_encoder* h, const sw_specials* sp) {
  if (sp && sp->n > 0 && (!sp->bytes || !sp->off || !sp->ids)) return fail(SW_ERR_ARG, "specials: null arrays");
  const int64_t n = sp ? sp->n : 0;
  std::string key;
  if (n > 0) {
    if (sp->off[0] < 0) return fail(SW_ERR_ARG, "specials: bad offsets");
    for (int64_t k = 0; k < n; ++k)
      if (sp->off[k + 1] < sp->off[k]) return fail(SW_ERR_ARG, "specials: bad offsets");
    const int64_t nb = sp->off[n];
    if (nb > INT32_MAX / 2 || n > INT32_MAX / 8) return fail(SW_ERR_ARG, "specials: too large");
    key.assign((const char*)&n, sizeof(n));
    key.append((const char*)sp->off, sizeof(int64_t) * (size_t)(n + 1));
    key.append((const char*)sp->ids, sizeof(int32_t) * (size_t)n);
    key.append((const char*)sp->bytes, (size_t)nb);
  }
  if (h->d_spt && key == h->spt_key) return SW_OK;
  DeviceGuard g(h->device);
  if (h->ws_pending) HIP_TRY(hipEventSynchronize(h->ws_done));  // (a finder still reading the old table)
  h->d_spt.reset();
  h->spt = SpTab{};
  h->spt_key.clear();
  h->spt_dev = false;
  if (n == 0) return SW_OK;
  const int64_t b0 = sp->off[0], nb = sp->off[n] - b0;
  std::vector<int32_t> off((size_t)n + 1), ids((size_t)n), list, first(257, 0);
  for (int64_t k = 0; k <= n; ++k) off[(size_t)k] = (int32_t)(sp->off[k] - b0);
  for (int64_t k = 0; k < n; ++k) ids[(size_t)k] = sp->ids[k];
  std::vector<std::vector<int32_t>> by_first(256);
  int32_t max_len = 0, min_len = INT32_MAX;
  const bool few = n <= 255;  // (the one-pass finder records a special's index in a byte)
  for (int64_t k = 0; k < n; ++k) {
    const int32_t L = off[(size_t)k + 1] - off[(size_t)k];
    if (L == 0) continue;  // (an empty special never matches)
    by_first[sp->bytes[sp->off[k]]].push_back((int32_t)k);
    max_len = std::max(max_len, L);
    min_len = std::min(min_len, L);
  }
  SpTab t{};
  uint32_t fb = 0;
  for (int b = 0; b < 256; ++b) {
    first[(size_t)b] = (int32_t)list.size();
    if (by_first[(size_t)b].empty()) continue;
    t.filt[b >> 5] |= 1u << (b & 31);
    if (t.n_first < kSpMaxFirstSwar) fb |= (uint32_t)b << (8 * t.n_first);
    ++t.n_first;
    list.insert(list.end(), by_first[(size_t)b].begin(), by_first[(size_t)b].end());
  }
  first[256] = (int32_t)list.size();
  if (list.empty()) list.push_back(0);
  t.fb = fb;
  t.max_len = max_len;
  t.n = (int32_t)n;
  // the LDS image of k_sp_find (specials_find.h, above sft_len), when the finder takes the table
  std::vector<uint32_t> img;
  if (few && max_len <= kSpMaxLen) {
    const int32_t n_list = first[256];
    t.o_first = (int32_t)n;
    t.o_rec = (t.o_first + 129 + 3) & ~3;  // (16-byte aligned records)
    t.o_tag = t.o_rec + kSfRecWords * n_list;
    t.o_words = t.o_tag + n_list;
    img.assign((size_t)t.o_words, 0u);
    for (int b = 0; b <= 256; ++b) img[(size_t)t.o_first + b / 2] |= (uint32_t)first[(size_t)b] << (16 * (b & 1));
    std::vector<uint32_t> wo_of((size_t)n, 0u);
    for (int64_t k = 0; k < n; ++k) {
      const int32_t L = off[(size_t)k + 1] - off[(size_t)k];
      const size_t wo = img.size() - (size_t)t.o_words;
      wo_of[(size_t)k] = (uint32_t)wo;
      img[(size_t)k] = (uint32_t)wo | (uint32_t)L << 16;
      img.resize(img.size() + (size_t)(L + 3) / 4, 0u);
      std::memcpy(img.data() + t.o_words + wo, sp->bytes + sp->off[k], (size_t)L);
    }
    for (int32_t g = 0; g < n_list; ++g) {
      const int32_t k = list[(size_t)g], L = off[(size_t)k + 1] - off[(size_t)k];
      uint32_t* rec = img.data() + t.o_rec + kSfRecWords * g;
      for (int32_t j = 0; j < std::min<int32_t>(L, 16); ++j) {
        rec[j / 4] |= (uint32_t)sp->bytes[sp->off[k] + j] << (8 * (j % 4));
        rec[4 + j / 4] |= 0xFFu << (8 * (j % 4));
      }
      img[(size_t)t.o_tag + g] = (uint32_t)k | (uint32_t)L << 8 | wo_of[(size_t)k] << 16;
    }
    img.push_back(0u);  // (k_sp_find reads a special's second word even for one of <= 4 bytes)
    t.img_words = (int32_t)img.size();
  }
  // one buffer: bytes | off | ids | list | first | LDS image
  const size_t o_off = ((size_t)nb + 15) & ~(size_t)15, o_ids = o_off + 4 * off.size(), o_list = o_ids + 4 * ids.size(),
               o_first = o_list + 4 * list.size(), o_img = o_first + 4 * first.size(), total = o_img + 4 * img.size();
  std::vector<char> host(total, 0);
  std::memcpy(host.data(), sp->bytes + b0, (size_t)nb);
  std::memcpy(host.data() + o_off, off.data(), 4 * off.size());
  std::memcpy(host.data() + o_ids, ids.data(), 4 * ids.size());
  std::memcpy(host.data() + o_list, list.data(), 4 * list.size());
  std::memcpy(host.data() + o_first, first.data(), 4 * first.size());
  if (!img.empty()) std::memcpy(host.data() + o_img, img.data(), 4 * img.size());
  HIP_TRY(h->d_spt.reset(total));
  HIP_TRY(hipMemcpy(h->d_spt, host.data(), total, hipMemcpyHostToDevice));
  char* d = h->d_spt;
  t.bytes = (const uint8_t*)d;
  t.off = (const int32_t*)(d + o_off);
  t.ids = (const int32_t*)(d + o_ids);
  t.list = (const int32_t*)(d + o_list);
  t.first = (const int32_t*)(d + o_first);
  t.img = img.empty() ? nullptr : (const uint32_t*)(d + o_img);
  h->spt = t;
  h->spt_key = key;
  h->spt_dev = t.n_first > 0 && max_len <= kSpMaxLen && few;
  h->spt_min_len = t.n_first > 0 ? min_len : 1;
  return SW_OK;
}

// the occurrences of the handle's specials in d_bytes (sw_find_specials_device), on stream st
int32_t sw::find_specials_device(sw_encoder* h, const uint8_t* d_bytes, int64_t n_bytes, const int64_t* d_str_off,
                             int64_t n_str, int64_t* d_pos, int32_t* d_len, int32_t* d_id, int64_t cap, int64_t* d_count,
                             hipStream_t st) {
  if (!h || n_bytes < 0 || n_str < 0 || !d_str_off || !d_count || (n_bytes > 0 && !d_bytes))
    return fail(SW_ERR_ARG, "sw_find_specials_device: bad arguments");
  if (n_bytes > kMaxLaunchBytes) return fail(SW_ERR_ARG, "sw_find_specials_device: n_bytes > 2^30 - 64");
  if (h->d_spt && h->spt.n_first > 0 && !h->spt_dev)
    return fail(SW_ERR_ARG, "sw_find_specials_device: a special over 64 bytes, or over 255 specials (use the host finder)");
  if (h->spt.n_first > 0 && n_bytes > 0 && (cap < n_bytes / h->spt_min_len || !d_pos || !d_len || !d_id))
    return fail(SW_ERR_CAP, "sw_find_specials_device: cap < n_bytes / (shortest special's length)");
  if (h->ws_pending && h->ws_stream != st) HIP_TRY(hipStreamWaitEvent(st, h->ws_done, 0));
  const int64_t n_tiles = (n_bytes + kTile - 1) / kTile;
  if (h->spt.n_first == 0 || n_tiles == 0) {
    HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(int64_t), st));
  } else {
    int32_t rc = ensure_workspace(h, n_bytes);
    if (rc) return rc;
    const int64_t tcap = kTile / h->spt_min_len + 1;  // (a tile's occurrences: at most this many)
    const int64_t n_parts = (n_tiles + kScanBlock - 1) / kScanBlock + 1;
    if (n_tiles > h->spf_tiles || tcap > h->spf_tcap) {
      h->d_spf.reset(); h->d_spf_list.reset(); h->d_spf_off.reset();
      h->spf_tiles = 0; h->spf_tcap = 0;
      HIP_TRY(h->d_spf.reset((size_t)n_tiles * (2 * 64 + 2) + 1));
      HIP_TRY(h->d_spf_list.reset((size_t)n_tiles * (size_t)tcap));
      HIP_TRY(h->d_spf_off.reset((size_t)(2 * (n_tiles + n_parts) + 1)));
      h->spf_tiles = n_tiles;
      h->spf_tcap = tcap;
    }
    SpFind f;
    f.bytes = d_bytes; f.n_bytes = n_bytes; f.str_off = d_str_off; f.n_str = n_str;
    f.tile_slo = h->ws.d_tile_slo; f.n_tiles = n_tiles;
    f.cbits = h->d_spf; f.chosen = h->d_spf + 64 * n_tiles;
    f.tcand = h->d_spf + 128 * n_tiles; f.tcnt = f.tcand + n_tiles;
    f.flag = (unsigned int*)(f.tcnt + n_tiles);
    f.list = h->d_spf_list; f.tcap = tcap;
    int64_t* toff = h->d_spf_off;                     // [n_tiles] + partials
    int64_t* toff2 = h->d_spf_off + n_tiles + n_parts;  // the global path's
    int64_t* total2 = toff2 + n_tiles + n_parts;
    const dim3 gw((unsigned)((n_tiles + kWaves - 1) / kWaves)), bw(kThreads);
    HIP_TRY(hipMemsetAsync(f.flag, 0, sizeof(unsigned int), st));
    hipLaunchKernelGGL(k_tile_strings, dim3((unsigned)((n_tiles + 255) / 256)), dim3(256), 0, st, d_str_off, n_str,
                       n_tiles, h->ws.d_tile_slo, nullptr);
    const bool swar = h->spt.n_first <= kSpMaxFirstSwar;
    // the one-pass path
    const size_t lds_tab = sizeof(uint32_t) * (size_t)h->spt.img_words;
    if (swar) hipLaunchKernelGGL(k_sp_find<true>, gw, bw, lds_tab, st, h->spt, f);
    else hipLaunchKernelGGL(k_sp_find<false>, gw, bw, lds_tab, st, h->spt, f);
    HIP_TRY(launch_scan(st, f.tcnt, n_tiles, toff + n_tiles, toff, d_count));
    const dim3 ge((unsigned)((n_tiles + kWaves * kSfEmitTiles - 1) / (kWaves * kSfEmitTiles)));
    hipLaunchKernelGGL(k_sp_emit, ge, bw, 0, st, h->spt, f, (const int64_t*)toff, d_pos, d_len, d_id);
    // the global-memory path: its kernels return at once unless k_sp_find raised the flag (small
    // grids that loop over the tiles)
    const dim3 gg(std::min<unsigned>(gw.x, kSfGlobalBlocks));
    if (swar) hipLaunchKernelGGL(k_sp_detect<true>, gg, bw, 0, st, h->spt, f);
    else hipLaunchKernelGGL(k_sp_detect<false>, gg, bw, 0, st, h->spt, f);
    hipLaunchKernelGGL(k_sp_resolve, gg, bw, lds_tab, st, h->spt, f);
    hipLaunchKernelGGL(k_sp_count, gg, bw, 0, st, f);
    HIP_TRY(launch_scan(st, f.tcnt, n_tiles, toff2 + n_tiles, toff2, total2));
    hipLaunchKernelGGL(k_sp_write, gg, bw, 0, st, h->spt, f, (const int64_t*)toff2, d_pos, d_len, d_id);
    hipLaunchKernelGGL(k_sp_fix_count, dim3(1), dim3(64), 0, st, (const unsigned int*)f.flag, (const int64_t*)total2,
                       d_count);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(h->ws_done, st));
  h->ws_stream = st;
  h->ws_pending = true;
  return SW_OK;
}

// ------------------------------------------------------------------------------------------
// the device pipeline (encode_device), stage by stage
// ------------------------------------------------------------------------------------------
namespace {

// the kernels' arguments for one launch (spa: its special-token occurrences per tile)
EncArgs make_args(sw_encoder* h, const uint8_t* d_bytes, int64_t n_bytes, const int64_t* d_str_off, int64_t n_str,
                  const uint64_t* d_chunk_bits, const SpArgs& spa, int64_t* d_out_off, int64_t n_tiles) {
  Workspace& w = h->ws;
  EncArgs a;
  a.bytes = d_bytes; a.n_bytes = n_bytes; a.bits = d_chunk_bits; a.n_words = (n_bytes + 63) / 64;
  a.str_off = d_str_off; a.n_str = n_str; a.table = h->table; a.chunks = h->chunks;
  a.scratch = w.d_scratch; a.res = w.d_res;
  a.tile_slots = w.d_tile_slots; a.tile_nref = w.d_tile_nref; a.rlist = w.d_rlist; a.tile_cnt = w.d_tile_cnt;
  a.dtab = w.d_dtab; a.dedupe = h->dedupe ? 1u : 0u; a.dfp_mask = h->dedupe_fp_mask;
  {
    const uint32_t lmask = (uint32_t)(launch_dd_slots(h, n_bytes) - 1);
    a.dmask = h->dedupe_slots ? std::min<uint32_t>(lmask, (uint32_t)(h->dedupe_slots - 1)) : lmask;
  }
  a.dexact = h->dedupe_exact ? (uint32_t)kDdExactMax : 0u;
  a.dres = w.d_dres;
  a.dcnt = w.d_dcnt;
  a.dd_full = w.d_ddfull;
  a.llist = w.d_llist; a.l_count = w.d_lcount;
  a.big_count = w.d_big; a.big_list = w.d_big + 1;
  a.out_off = d_out_off; a.tile_slo = w.d_tile_slo;
  a.n_tiles = n_tiles; a.qtmp = w.d_res; a.bcnt = w.d_bcnt; a.boff = w.d_boff; a.q_total = w.d_qtotal;
  a.queue = w.d_queue; a.stamps = w.d_stamps;
  a.inv = h->d_inv; a.n_inv = h->n_inv; a.ids16 = h->ids16 ? 1u : 0u;
  a.lstart = w.lp.wstart; a.llen = w.lp.wlen; a.n_long = &w.lp.ctl[kLcWave]; a.lcap = w.lp.lcap;
  a.sp = spa;
  // the result heads staged by k_tile_count when the dedupe table has grown past the caches (its
  // heads, 16 B an entry, are random HBM reads that k_compact would otherwise make a second time)
  // (automatic: the previous launch ran more than kStagedMinMerges merge loops, i.e. its distinct
  // results' heads spread over more 64-byte lines than the 256 MB Infinity Cache holds -- ENTROPY's
  // 15.6 M per GiB; a GPT-2 pre-split with specials runs 3 M and keeps them cached, and C2 0.75 M.
  // Read without waiting, like the compaction kernel's choice: results are identical either way)
  const unsigned long long prev_merges = h->h_ddfull ? __atomic_load_n(&h->h_ddfull[2], __ATOMIC_RELAXED) : 0ULL;
  a.staged_heads = (h->staged_heads == 1 || (h->staged_heads == 0 && h->dedupe && prev_merges > kStagedMinMerges)) ? 1u : 0u;
  return a;
}

// the classification kernel and the pass over the tiles it leaves: fused with the device
// pre-split (pg given: k_split_classify, k_split_redo) or from the bitmap a.bits (k_classify;
// k_classify_big takes the tiles over its chunk-start capacity).  c0 / c1: the timing events
// around the first kernel alone.
template <bool kSp>
hipError_t launch_classify_pair(sw_encoder* h, hipStream_t st, const EncArgs& a, const PbArgs* pg, int pattern,
                                hipEvent_t c0, hipEvent_t c1) {
  const dim3 gc((unsigned)((a.n_tiles + kWaves - 1) / kWaves)), gr(kRedoGrid), b(kThreads);
  unsigned int* count = h->ws.d_redo;  // the tiles left: count, then the list (int64)
  int64_t* tiles = (int64_t*)(count + 2);
  hipError_t e = c0 ? hipEventRecord(c0, st) : hipSuccess;
  if (e != hipSuccess) return e;
  if (pg) {
    const RedoList redo{count, tiles};  // (its count zeroed by k_edges)
    const uint32_t* edge = h->ws.d_edge;
    uint32_t* pbits = (uint32_t*)h->ws.d_pbits.get();
    hipLaunchKernelGGL(k_split_classify<kSp>, gc, b, 0, st, ScArgs{a, *pg, pattern, edge, pbits, redo});
    if (c1 && (e = hipEventRecord(c1, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_split_redo<kSp>, gr, b, 0, st, a, *pg, pattern, edge, pbits, redo);
  } else {
    hipLaunchKernelGGL(k_classify<kSp>, gc, b, 0, st, a, count, tiles);
    if (c1 && (e = hipEventRecord(c1, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_classify_big<kSp>, gr, b, 0, st, a, (const unsigned int*)count, (const int64_t*)tiles);
  }
  return hipGetLastError();
}

// the dedupe table cleared, then the classification: fused (k_edges + k_split_classify: the device
// pre-split inside it) or from the bitmap a.bits
int32_t launch_classify(sw_encoder* h, hipStream_t st, const EncArgs& a, int32_t pattern, bool fused) {
  const int64_t n_tiles = a.n_tiles;
  // (cleared per launch rather than entry by entry by the merge kernels that empty the claims:
  // the memset leaves the table's lines in the caches, and the probes then hit -- clearing only
  // the claims made k_split_classify 2% slower on C2, r4n/r4o A/B)
  const size_t dtab_bytes = sizeof(uint64_t) * kDdWords * ((size_t)a.dmask + 1);
  // (k_edges' threads clear the table -- +4 us of k_edges for a 9 us memset on C2, r8b -- when its
  // grid covers the table in a few stores per thread; a small launch after the table has grown
  // for a large one keeps the memset, which is not limited to k_edges' few blocks)
  const int64_t edge_threads = (n_tiles + 1 + 255) / 256 * 256;
  const bool clr_in_edges = fused && dtab_bytes % 16 == 0 && (int64_t)(dtab_bytes / 16) <= 16 * edge_threads;
  if (h->dedupe && !clr_in_edges) HIP_TRY(hipMemsetAsync(h->ws.d_dtab, 0, dtab_bytes, st));
  hipEvent_t c0 = nullptr, c1 = nullptr;  // (timing: the classification kernel alone -- k_split_classify or k_classify)
  if (h->timing) HIP_TRY(h->ev_cls.next(&c0, &c1));
  const PbArgs pg{a.bytes, a.n_bytes, a.str_off, a.n_str, a.tile_slo, a.sp};
  if (fused)
    hipLaunchKernelGGL(k_edges, dim3((unsigned)((n_tiles + 1 + 255) / 256)), dim3(256), 0, st, pg, n_tiles, (int)pattern,
                       h->ws.d_edge.get(), h->ws.d_redo.get(), h->dedupe && clr_in_edges ? (uint4*)h->ws.d_dtab.get() : nullptr,
                       (int64_t)(dtab_bytes / 16));
  else
    HIP_TRY(hipMemsetAsync(h->ws.d_redo, 0, sizeof(unsigned int), st));
  HIP_TRY(a.sp.n > 0 ? launch_classify_pair<true>(h, st, a, fused ? &pg : nullptr, (int)pattern, c0, c1)
                     : launch_classify_pair<false>(h, st, a, fused ? &pg : nullptr, (int)pattern, c0, c1));
  if (c1) ++h->ev_cls.used;
  return SW_OK;
}

// the four bucket launches of one table variant: 17..32 B, 9..16 B, 5..8 B, 2..4 B on their streams
template <bool kWide, bool k16, bool kWF>
void launch_merge_buckets(const EncArgs& a, const hipStream_t (&ms)[4]) {
  const dim3 pg(2048), pb(kThreads);  // persistent grid for the queue kernels
  hipLaunchKernelGGL((k_merge_bucket<kWide, k16, 32, kWF>), pg, pb, 0, ms[0], a, 8, 9);
  hipLaunchKernelGGL((k_merge_bucket<kWide, k16, 16, kWF>), pg, pb, 0, ms[1], a, 5, 7);
  hipLaunchKernelGGL((k_merge_bucket<kWide, k16, 8, kWF>), pg, pb, 0, ms[2], a, 3, 4);
  hipLaunchKernelGGL((k_merge_bucket<kWide, k16, 4, kWF>), pg, pb, 0, ms[1], a, 0, 2);
}

// the merge loops of the queued chunks: the fork, the long chunks' first part, the dense queue
// (scan + scatter), the long chunks' second part, the buckets, the join
template <bool kWide, bool k16, bool kWF>
int32_t launch_merges_as(sw_encoder* h, hipStream_t st, const EncArgs& a) {
  const int64_t n_tiles = a.n_tiles;
  const bool split = h->split_ok && h->long_split;  // (split + verify needs a well-formed table)
  // streams of the merge kernels: [0] buckets 17..32 B, then 5..8 B, [1] 9..16 B, then 2..4 B
  // (balanced for the memo-off loads: 9.4 + 6.6 against 12.3 + 3.1 ms), [3] the long chunks,
  // forked right here: they start from k_classify's long list and the complete bitmap, beside
  // the scan and the scatter (C2: their ~20 small passes no longer outlast the merge kernels).
  // (Two forks only: streams beyond the process's hardware queues (4) share one and run in
  // launch order, which put the long chunks behind a bucket.)
  hipStream_t ms[4] = {st, st, st, st};
  if (h->merge_fork) {
    for (int k = 0; k < 2; ++k) {
      HIP_TRY(h->s_fork[k].ensure());
      HIP_TRY(h->ev_join[k].ensure());
    }
    HIP_TRY(h->ev_fork.ensure());
    HIP_TRY(h->ev_fork_long.ensure());
    HIP_TRY(hipEventRecord(h->ev_fork_long, st));
    HIP_TRY(hipStreamWaitEvent(h->s_fork[1], h->ev_fork_long, 0));
    ms[1] = h->s_fork[0];
    ms[3] = h->s_fork[1];
  }
  HIP_TRY((launch_long<kWide, k16>(h, ms[3], a, split, 1)));
  HIP_TRY(launch_scan(st, h->ws.d_bcnt, kNumBuckets * n_tiles, h->ws.d_part, h->ws.d_boff, h->ws.d_qtotal));
  hipLaunchKernelGGL(k_scatter, dim3((unsigned)((n_tiles + 15) / 16)), dim3(kThreads), 0, st, a);  // (4 tiles a wave)
  if (h->merge_fork) {
    HIP_TRY(hipEventRecord(h->ev_fork, st));
    for (int k = 0; k < 2; ++k) HIP_TRY(hipStreamWaitEvent(h->s_fork[k], h->ev_fork, 0));
  }
  HIP_TRY((launch_long<kWide, k16>(h, ms[3], a, split, 2)));
  launch_merge_buckets<kWide, k16, kWF>(a, ms);
  if (h->merge_fork) {
    for (int k = 0; k < 2; ++k) {
      HIP_TRY(hipEventRecord(h->ev_join[k], h->s_fork[k]));
      HIP_TRY(hipStreamWaitEvent(st, h->ev_join[k], 0));
    }
  }
  HIP_TRY(hipGetLastError());
  return SW_OK;
}

// ... with the table's variant resolved once: wide ids, 16-bit ids, and among those the
// well-formed tables (the rank-matching loop)
int32_t launch_merges(sw_encoder* h, hipStream_t st, const EncArgs& a) {
  if (h->table.wide) return launch_merges_as<true, false, false>(h, st, a);
  if (h->ids16 && h->split_ok) return launch_merges_as<false, true, true>(h, st, a);
  if (h->ids16) return launch_merges_as<false, true, false>(h, st, a);
  return launch_merges_as<false, false, false>(h, st, a);
}

// ids per tile, their scan, and the slots compacted into OutT ids
template <class OutT>
int32_t launch_compact_as(sw_encoder* h, hipStream_t st, const EncArgs& a, OutT* d_out_ids) {
  const int64_t n_tiles = a.n_tiles;
  if (a.staged_heads)
    hipLaunchKernelGGL(k_tile_count_staged, dim3((unsigned)((n_tiles + kWaves - 1) / kWaves)), dim3(kThreads), 0, st, a);
  else
    hipLaunchKernelGGL(k_tile_count, dim3((unsigned)((n_tiles + kWaves * kTcTiles - 1) / (kWaves * kTcTiles))),
                       dim3(kThreads), 0, st, a);
  HIP_TRY(launch_scan(st, h->ws.d_tile_cnt, n_tiles, h->ws.d_part, h->ws.d_tile_base, h->ws.d_total));
  // the compaction kernel from the last launch's ids per tile (read without waiting: a heuristic)
  int ck = h->compact_kernel;
  if (ck == 0) {
    ck = 1;
    const unsigned long long ids = h->h_ddfull ? __atomic_load_n(&h->h_ddfull[1], __ATOMIC_RELAXED) : 0ULL;
    const unsigned long long tl = (unsigned long long)h->cp_prev_tiles;
    if (tl > 0 && ids > 0) ck = ids <= tl * kCompactTypedMaxIdsPerTile ? 3 : ids <= tl * kCompact7MaxIdsPerTile ? 2 : 1;
  }
  h->cp_prev_tiles = n_tiles;
  const int64_t* tile_base = h->ws.d_tile_base;
  auto launch = [&](auto kernel) {  // one wave per tile
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n_tiles + 3) / 4)), dim3(kThreads), 0, st, a, tile_base, d_out_ids);
  };
  if (ck == 3) launch(k_compact7<OutT, true>);
  else if (ck == 2) launch(k_compact7<OutT, false>);
  else launch(k_compact<OutT>);
  HIP_TRY(hipGetLastError());
  return SW_OK;
}

int32_t launch_compact(sw_encoder* h, hipStream_t st, const EncArgs& a, void* d_out_ids, bool out16) {
  return out16 ? launch_compact_as(h, st, a, (uint16_t*)d_out_ids) : launch_compact_as(h, st, a, (int32_t*)d_out_ids);
}

}  // namespace

int32_t sw::encode_device(sw_encoder* h, const uint8_t* d_bytes, int64_t n_bytes, const int64_t* d_str_off, int64_t n_str,
                          const uint64_t* d_chunk_bits, const DevSpecials& sp, void* d_out_ids, bool out16,
                          int64_t* d_out_off, void* stream, int64_t* n_tokens_host, int32_t pattern_call) {
  if (pattern_call < -1 || pattern_call > SW_PAT_NONE) return fail(SW_ERR_ARG, "sw_encode_device: unknown pattern");
  if (!h || n_bytes < 0 || n_str < 0 || !d_str_off || !d_out_off || (n_bytes > 0 && (!d_bytes || !d_out_ids)))
    return fail(SW_ERR_ARG, "sw_encode_device: bad arguments");
  if (sp.n < 0 || (sp.n > 0 && (!sp.pos || !sp.len || !sp.id)))
    return fail(SW_ERR_ARG, "sw_encode_device: bad special-token occurrences");
  if (out16 && !h->ids16) return fail(SW_ERR_ARG, "sw_encode_device: 16-bit output needs a table whose ids fit 16 bits");
  if (out16 && sp.n > 0) return fail(SW_ERR_ARG, "sw_encode_device: 16-bit output with special tokens is not supported");
  if (n_bytes > kMaxLaunchBytes) return fail(SW_ERR_ARG, "sw_encode_device: n_bytes > 2^30 - 64 (split the batch)");
  DeviceGuard g(h->device);
  const int32_t pattern = pattern_call >= 0 ? pattern_call : h->pattern;  // (per call, or the handle's option)
  hipStream_t st = (hipStream_t)stream;  // (NULL: the null stream, as torch's default stream)
  // the workspace belongs to the handle: order this launch after the previous one on any stream
  if (h->ws_pending && h->ws_stream != st) HIP_TRY(hipStreamWaitEvent(st, h->ws_done, 0));
  int32_t rc = ensure_workspace(h, n_bytes);
  if (rc == SW_OK && h->dedupe) rc = grow_dedupe(h, n_bytes);
  if (rc) return rc;
  Workspace& w = h->ws;
  const int64_t n_tiles = (n_bytes + kTile - 1) / kTile;
  h->last_tiles = n_tiles;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (h->timing) {  // the whole device pipeline, k_tile_strings .. k_string_offsets
    HIP_TRY(h->ev_pool.next(&e0, &e1));
    HIP_TRY(hipEventRecord(e0, st));
  }
  if (n_tiles > 0) {
    // (the pre-split and k_classify start from each tile's first string)
    hipLaunchKernelGGL(k_tile_strings, dim3((unsigned)((n_tiles + 255) / 256)), dim3(256), 0, st, d_str_off, n_str,
                       n_tiles, w.d_tile_slo.get(), w.d_lcount.get());  // (and the long list emptied)
    const SpArgs spa{sp.pos, sp.len, sp.id, sp.n, w.d_tile_sp, w.d_tile_sp + (n_tiles + 1)};
    if (sp.n > 0)  // (... and their first special-token occurrence; the count last)
      hipLaunchKernelGGL(k_tile_specials, dim3((unsigned)((n_tiles + 1 + 255) / 256)), dim3(256), 0, st, sp.pos, sp.len,
                         sp.n, sp.n_dev, n_tiles, w.d_tile_sp.get(), w.d_tile_sp + (n_tiles + 1));
    // the full path (no caller bitmap): the device pre-split, fused into the classification
    // (k_edges + k_split_classify) or as its own kernel first (SW_OPT_FUSED_PRESPLIT 0; special
    // tokens always take the fused kernel)
    const bool fused = !d_chunk_bits && (h->fused_presplit || sp.n > 0);
    if (!d_chunk_bits) {
      if (!fused) HIP_TRY(launch_presplit(st, d_bytes, n_bytes, d_str_off, n_str, pattern, w.d_pbits, w.d_tile_slo));
      d_chunk_bits = w.d_pbits;
    }
    const EncArgs a = make_args(h, d_bytes, n_bytes, d_str_off, n_str, d_chunk_bits, spa, d_out_off, n_tiles);
    if ((rc = launch_classify(h, st, a, pattern, fused)) != SW_OK) return rc;
    if ((rc = launch_merges(h, st, a)) != SW_OK) return rc;
    if ((rc = launch_compact(h, st, a, d_out_ids, out16)) != SW_OK) return rc;
  } else {
    HIP_TRY(hipMemsetAsync(w.d_total, 0, sizeof(int64_t), st));
  }
  hipLaunchKernelGGL(k_string_offsets, dim3((unsigned)((n_str + 1 + 255) / 256)), dim3(256), 0, st, d_str_off, n_str,
                     n_bytes, w.d_total.get(), d_out_off, w.d_ddfull.get(), h->hd_ddfull,
                     n_tiles > 0 ? w.d_qtotal.get() : nullptr);
  HIP_TRY(hipGetLastError());
  if (h->timing) {
    HIP_TRY(hipEventRecord(e1, st));
    ++h->ev_pool.used;
  }
  HIP_TRY(hipEventRecord(h->ws_done, st));
  h->ws_stream = st;
  h->ws_pending = true;
  if (n_tokens_host) {
    HIP_TRY(hipMemcpyAsync(n_tokens_host, w.d_total, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  return SW_OK;
}

extern "C" int32_t sw_encode_device(sw_encoder* h, const uint8_t* d_bytes, int64_t n_bytes, const int64_t* d_str_off,
                                    int64_t n_str, const uint64_t* d_chunk_bits, int32_t* d_out_ids,
                                    int64_t* d_out_off, void* stream, int64_t* n_tokens_host) {
  return encode_device(h, d_bytes, n_bytes, d_str_off, n_str, d_chunk_bits, DevSpecials{}, d_out_ids, false, d_out_off,
                       stream, n_tokens_host);
}

extern "C" int32_t sw_encode_device_ex(sw_encoder* h, const uint8_t* d_bytes, int64_t n_bytes, const int64_t* d_str_off,
                                       int64_t n_str, const sw_encode_ex* ex, void* d_out_ids, int64_t* d_out_off,
                                       void* stream, int64_t* n_tokens_host) {
  if (!ex)
    return encode_device(h, d_bytes, n_bytes, d_str_off, n_str, nullptr, DevSpecials{}, d_out_ids, false, d_out_off,
                         stream, n_tokens_host);
  if (ex->struct_size != (int32_t)sizeof(sw_encode_ex))
    return fail(SW_ERR_ARG, "sw_encode_device_ex: struct_size is not sizeof(sw_encode_ex) of this library");
  if (ex->out_bits != 0 && ex->out_bits != 16 && ex->out_bits != 32)
    return fail(SW_ERR_ARG, "sw_encode_device_ex: out_bits 16 or 32");
  if ((ex->flags & SW_EX_PATTERN) && (ex->pattern < SW_PAT_CL100K || ex->pattern > SW_PAT_NONE))
    return fail(SW_ERR_ARG, "sw_encode_device_ex: unknown pattern");
  DevSpecials sp;
  sp.pos = ex->sp_pos; sp.len = ex->sp_len; sp.id = ex->sp_id; sp.n = ex->n_sp; sp.n_dev = ex->d_n_sp;
  if (sp.n_dev && sp.n <= 0) return fail(SW_ERR_ARG, "sw_encode_device_ex: d_n_sp needs n_sp = the arrays' capacity");
  return encode_device(h, d_bytes, n_bytes, d_str_off, n_str, ex->chunk_bits, sp, d_out_ids, ex->out_bits == 16,
                       d_out_off, stream, n_tokens_host, (ex->flags & SW_EX_PATTERN) ? ex->pattern : -1);
}

extern "C" int32_t sw_encoder_set_specials(sw_encoder* h, const sw_specials* sp) {
  if (!h) return fail(SW_ERR_ARG, "sw_encoder_set_specials: null handle");
  return set_specials(h, sp);
}

extern "C" int32_t sw_find_specials_device(sw_encoder* h, const uint8_t* d_bytes, int64_t n_bytes,
                                           const int64_t* d_str_off, int64_t n_str, int64_t* d_pos, int32_t* d_len,
                                           int32_t* d_id, int64_t cap, int64_t* d_count, void* stream, int64_t* n_host) {
  if (!h) return fail(SW_ERR_ARG, "sw_find_specials_device: null handle");
  DeviceGuard g(h->device);
  const hipStream_t st = (hipStream_t)stream;
  const int32_t rc = find_specials_device(h, d_bytes, n_bytes, d_str_off, n_str, d_pos, d_len, d_id, cap, d_count, st);
  if (rc) return rc;
  if (n_host) {
    HIP_TRY(hipMemcpyAsync(n_host, d_count, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  return SW_OK;
}


extern "C" int32_t sw_encoder_last_counts(sw_encoder* h, int64_t* out4) {
  if (!h || !out4) return fail(SW_ERR_ARG, "sw_encoder_last_counts: bad arguments");
  DeviceGuard g(h->device);
  for (int i = 0; i < 4; ++i) out4[i] = 0;
  out4[3] = h->last_tiles;
  if (!h->ws_pending || h->last_tiles == 0) return SW_OK;
  HIP_TRY(hipEventSynchronize(h->ws_done));
  std::vector<uint32_t> slots((size_t)h->last_tiles), nref((size_t)h->last_tiles);
  HIP_TRY(hipMemcpy(slots.data(), h->ws.d_tile_slots, sizeof(uint32_t) * slots.size(), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(nref.data(), h->ws.d_tile_nref, sizeof(uint32_t) * nref.size(), hipMemcpyDeviceToHost));
  int64_t q = 0;
  HIP_TRY(hipMemcpy(&q, h->ws.d_qtotal, sizeof(q), hipMemcpyDeviceToHost));
  for (size_t t = 0; t < slots.size(); ++t) { out4[0] += slots[t]; out4[1] += nref[t]; }
  out4[2] = q;
  return SW_OK;
}

extern "C" int32_t sw_presplit_device(sw_encoder* h, const uint8_t* d_bytes, int64_t n_bytes, const int64_t* d_str_off,
                                      int64_t n_str, int32_t pattern, uint64_t* d_chunk_bits, void* stream,
                                      int64_t* n_chunks_host) {
  if (!h || n_bytes < 0 || n_str < 0 || !d_str_off || (n_bytes > 0 && (!d_bytes || !d_chunk_bits)))
    return fail(SW_ERR_ARG, "sw_presplit_device: bad arguments");
  if (pattern != SW_PAT_CL100K && pattern != SW_PAT_GPT2 && pattern != SW_PAT_NONE)
    return fail(SW_ERR_ARG, "sw_presplit_device: bad pattern");
  DeviceGuard g(h->device);
  hipStream_t st = (hipStream_t)stream;  // (NULL: the null stream, as torch's default stream)
  int32_t rc = ensure_workspace(h, n_bytes);
  if (rc) return rc;
  if (n_bytes > 0)
    hipLaunchKernelGGL(k_tile_strings, dim3((unsigned)(((n_bytes + kTile - 1) / kTile + 255) / 256)), dim3(256), 0, st,
                       d_str_off, n_str, (n_bytes + kTile - 1) / kTile, h->ws.d_tile_slo, nullptr);
  HIP_TRY(launch_presplit(st, d_bytes, n_bytes, d_str_off, n_str, pattern, d_chunk_bits, h->ws.d_tile_slo));
  if (n_chunks_host) {
    *n_chunks_host = 0;
    if (n_bytes > 0) {
      HIP_TRY(hipMemsetAsync(h->ws.d_pcount, 0, sizeof(unsigned long long), st));
      launch_popcount(st, d_chunk_bits, (n_bytes + 63) / 64, h->ws.d_pcount);
      unsigned long long c = 0;
      HIP_TRY(hipMemcpyAsync(&c, h->ws.d_pcount, sizeof(c), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      *n_chunks_host = (int64_t)c;
    }
  }
  return SW_OK;
}
