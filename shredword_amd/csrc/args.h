// What the encoder handle (encoder.h) keeps of the kernels' world: the launch limits and the two
// argument structs it holds between launches.  No device code here, so that the host batch unit
// (encode_batch.hip) sees the handle without compiling the kernels a second time.
#pragma once
#include <cstdint>

namespace sw {

constexpr int kTileBits = 11;
constexpr int kTile = 1 << kTileBits;        // input bytes per classify workgroup
constexpr int64_t kRefSpace = 1LL << 30;              // position references below, dense ones above
constexpr int64_t kMaxLaunchBytes = kRefSpace - 64;   // slot references are int32

// long chunks by split + verify (long_split.h): one allocation of the workspace, carved up
struct LongArgs {
  // the long chunks of the per-chunk wave loop (EncArgs::lstart / llen, count ctl[kLcWave];
  // SW_OPT_LONG_SPLIT 0 or an ill-formed table)
  uint32_t* wstart;
  uint32_t* wlen;
  // per long chunk of these passes (index i: k_lp_prep's order), lcap of each
  uint32_t* lstart;  // first byte
  uint32_t* llen;    // bytes
  uint32_t* lnp;     // pieces
  int64_t* lpo;      // exclusive scan of lnp: the chunk's first piece
  uint32_t* lfall;   // 1: the chunk takes the exact wave loop (k_lp_fallback)
  uint32_t* flist;   // ... those chunks (count ctl[kLcFall])
  // per piece (index j: pieces of chunk i are lpo[i] .. lpo[i] + lnp[i] - 1), pcap of each
  uint32_t* pbeg;    // first byte
  uint32_t* pcnt;    // ids (0 once absorbed by a window)
  uint32_t* pchunk;  // its chunk
  uint32_t* pflag;   // kLpAlive | kLpConf
  uint32_t* pprev;   // previous / next live piece of the chunk (kLpNone at the ends)
  uint32_t* pnext;
  uint32_t* pid;     // [n_bytes] a live piece's ids from its first byte's position on, then holes
                     // (kLpHole) up to the next live piece
  uint32_t* wlist;   // big windows of the current round: (head, last) piece pairs
  uint32_t* jlist[2];  // junctions (their right piece) to check in an even / odd round (r > 0)
  uint32_t* clist;   // pieces whose left junction conflicts (this round)
  uint32_t* hlist;   // window heads (this round)
  uint32_t* pseen;   // the last round r > 0 that checked the piece's left junction (a piece can be
                     // listed twice: after one window and as the head of another)
  int64_t* ctl;      // kLcWords counters
  int64_t lcap, pcap;
};

// the tokenizer's specials on the device (sw_encoder_set_specials; specials_find.h)
struct SpTab {
  const uint8_t* bytes;  // every special's bytes, concatenated
  const int32_t* off;    // [n + 1]
  const int32_t* ids;    // [n]
  const int32_t* list;   // the non-empty specials grouped by first byte, dict order within a group
  const int32_t* first;  // [257]: first byte b's group is list[first[b] .. first[b + 1])
  uint32_t filt[8];      // the first-byte set
  uint32_t fb;           // the distinct first bytes, one per byte (n_first <= kSpMaxFirstSwar)
  int32_t n_first;
  int32_t max_len;
  int32_t n;
  const uint32_t* img;   // the table as k_sp_find stages it in LDS (layout above sft_len)
  int32_t img_words, o_first, o_rec, o_tag, o_words;
};

}  // namespace sw
