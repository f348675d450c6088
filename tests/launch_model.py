"""A CPU model of what one device launch does, computed from the oracle alone (launch_counts and
what it calls use no product code), and at the end of the file the helpers the GPU tests share to
run one launch through the C-ABI and read back what it reports.

sw_encoder_last_counts publishes four numbers per sw_encode_device launch.  Two of them are the work
the memoisation shortcuts leave over, and both shortcuts fail silently (a miss gives the same ids),
so the ids cannot show a regression; these counts can.  The convention, as the kernels count
(classify_chunks in csrc/kernels.h, build_chunk_table in csrc/chunktable.cpp):

  chunks    the pre-split chunks of every string.  A special-token occurrence (leftmost first, the
            first special in dict order at one position, empty specials never match -- as
            encode_with_specials finds them) is one chunk; the text between occurrences is pre-split
            on its own.
  to_merge  the chunks whose slot refers to a merge result: every chunk that is not a single byte,
            not a special occurrence and not "tabled".  Tabled: 2..16 bytes, the oracle's encoding
            of the chunk is exactly one id, and that id is < 2^24 (the whole-chunk table's token
            field).  Chunks over 32 bytes are always in to_merge.
  distinct  the distinct byte strings among the to_merge chunks of at most 32 bytes: what the
            in-launch dedupe leaves to the merge loops (chunks over 32 bytes take the long-chunk
            path and are not counted here).
  tiles     ceil(n_bytes / 2048).

On an ill-formed table (duplicate byte strings, members used before they exist) the whole-chunk
table may lack entries the rule above would give it, so there `to_merge` is a lower bound.

A chunk's encoding is OracleModel.encode_chunk of its bytes; the distinct chunks of a batch are
encoded in one call, OracleModel.encode_batch with PAT_NONE (each string one chunk, through the same
orc_encode_chunk -- tests/test_launch_model.py checks the two against each other).
"""
from collections import namedtuple

import numpy as np

import oracle

TILE = 2048          # bytes per tile
SHORT = 32           # longest chunk the dedupe and the merge buckets take; longer ones are "long"
TABLE_MIN, TABLE_MAX = 2, 16  # chunk lengths the whole-chunk table holds
TABLE_ID_LIMIT = 1 << 24      # ... and its token field

Counts = namedtuple("Counts", "chunks to_merge distinct tiles long_chunks multi specials")
Counts.__doc__ = """chunks / to_merge / distinct / tiles: as the module docstring defines them;
long_chunks: chunks over 32 bytes; multi: non-special chunks of 2 bytes or more (to_merge with the
whole-chunk table switched off); specials: special-token occurrences."""


def find_specials(data, specials):
    """The occurrences of `specials` (dict str -> id) in one string (bytes), as encode_with_specials
    scans: left to right, at one position the first special in dict order, the scan going on after
    the occurrence -> list of (pos, len, id)."""
    names = [(k.encode("utf-8"), v) for k, v in specials.items()]
    names = [(b, v) for b, v in names if b]
    out = []
    nxt = [data.find(b) for b, _ in names]
    p = 0
    while True:
        best = -1
        for k, q in enumerate(nxt):
            if 0 <= q < p:
                q = nxt[k] = data.find(names[k][0], p)
            if q >= 0 and (best < 0 or q < nxt[best]):  # (strict: ties go to the earlier special)
                best = k
        if best < 0:
            return out
        q, (b, v) = nxt[best], names[best]
        out.append((q, len(b), v))
        p = q + len(b)


def split_chunks(buf, off, pattern=oracle.PAT_CL100K, specials=None):
    """The chunks of the batch buf[off[s]:off[s+1]] -> (data bytes, starts int64[n], lens int64[n],
    sp_id int64[n]) with positions relative to off[0] and sp_id -1 for ordinary chunks, else the
    special's id.  In byte order."""
    off = np.asarray(off, dtype=np.int64)
    base = int(off[0]) if len(off) else 0
    end = int(off[-1]) if len(off) else 0
    data = np.ascontiguousarray(buf, dtype=np.uint8)[base:end].tobytes()
    starts, sp = [], {}
    bounds = (off - base).tolist()
    for s in range(len(bounds) - 1):
        a, e = bounds[s], bounds[s + 1]
        if e <= a:
            continue
        seg = a
        if specials:
            for q, ln, v in find_specials(data[a:e], specials):
                if a + q > seg:
                    starts += [seg + x for x in oracle.presplit(data[seg:a + q], pattern)]
                sp[a + q] = v
                starts.append(a + q)
                seg = a + q + ln
        if e > seg:
            starts += [seg + x for x in oracle.presplit(data[seg:e], pattern)]
    starts = np.array(starts, dtype=np.int64)
    lens = np.diff(np.append(starts, len(data))) if len(starts) else np.zeros(0, np.int64)
    # (a chunk ends where the next one starts: chunks tile every non-empty string, and an empty
    # string has none, so the next start is also the string's or the occurrence's end)
    sp_id = np.full(len(starts), -1, dtype=np.int64)
    if sp:
        where = np.searchsorted(starts, np.array(list(sp.keys()), dtype=np.int64))
        sp_id[where] = np.array(list(sp.values()), dtype=np.int64)
    return data, starts, lens, sp_id


def encode_keys(model, keys):
    """dict chunk bytes -> tuple of ids for the byte strings `keys` (one oracle call)."""
    keys = list(keys)
    if not keys:
        return {}
    koff = np.zeros(len(keys) + 1, dtype=np.int64)
    np.cumsum([len(k) for k in keys], out=koff[1:])
    ids, ioff = model.encode_batch(np.frombuffer(b"".join(keys), dtype=np.uint8), koff, oracle.PAT_NONE, n_threads=8)
    ids, ioff = ids.tolist(), ioff.tolist()
    return {k: tuple(ids[ioff[i]:ioff[i + 1]]) for i, k in enumerate(keys)}


def is_tabled(key, enc):
    return TABLE_MIN <= len(key) <= TABLE_MAX and len(enc) == 1 and 0 <= enc[0] < TABLE_ID_LIMIT


def launch_counts(merges, buf, off, pattern=oracle.PAT_CL100K, specials=None, model=None):
    """The expected Counts of one launch over the batch (see the module docstring).  model: an
    OracleModel of `merges` to reuse."""
    model = model or oracle.OracleModel(merges)
    data, starts, lens, sp_id = split_chunks(buf, off, pattern, specials)
    ordinary = sp_id < 0
    multi = ordinary & (lens >= 2)
    long_ = multi & (lens > SHORT)
    short_idx = np.flatnonzero(multi & ~long_)
    st, ln = starts[short_idx].tolist(), lens[short_idx].tolist()
    keys = [data[a:a + n] for a, n in zip(st, ln)]
    uniq = set(keys)
    enc = encode_keys(model, [k for k in uniq if len(k) <= TABLE_MAX])
    tabled = {k for k, e in enc.items() if is_tabled(k, e)}
    n_short_merge = sum(1 for k in keys if k not in tabled)
    n_long = int(long_.sum())
    return Counts(chunks=len(starts), to_merge=n_short_merge + n_long, distinct=len(uniq - tabled),
                  tiles=(len(data) + TILE - 1) // TILE, long_chunks=n_long, multi=int(multi.sum()),
                  specials=int((~ordinary).sum()))


def chunk_ids(merges, buf, off, pattern=oracle.PAT_CL100K, specials=None, model=None):
    """The batch's ids as the concatenation of its chunks' encodings (a special occurrence: its id)
    -> int32 array; equal to encode_batch / encode_batch_specials when the chunking above is the
    oracle's."""
    model = model or oracle.OracleModel(merges)
    data, starts, lens, sp_id = split_chunks(buf, off, pattern, specials)
    keys = [data[a:a + n] for a, n in zip(starts.tolist(), lens.tolist())]
    enc = encode_keys(model, {k for k, v in zip(keys, sp_id.tolist()) if v < 0})
    out = []
    for k, v in zip(keys, sp_id.tolist()):
        out.extend(enc[k] if v < 0 else (v,))
    return np.array(out, dtype=np.int32)


# ---------------------------------------------------------------------------------------------
# the device side: one launch through the C-ABI on torch buffers, and what it reports
# ---------------------------------------------------------------------------------------------
def last_counts(tok):
    """sw_encoder_last_counts of the tokenizer's handle -> [chunks, to_merge, merged, tiles]."""
    import ctypes

    from shredword_amd import _lib
    out4 = (ctypes.c_int64 * 4)()
    _lib.check(_lib.lib().sw_encoder_last_counts(tok._encoder(), out4))
    return list(out4)


def device_launch(tok, buf, off, pattern, entry="ex", bits=None, sp=None, out_bits=32, mis=0):
    """One sw_encode_device (entry "plain": the pattern set as the handle's SW_OPT_PATTERN) or
    sw_encode_device_ex (entry "ex": the pattern in the call) launch of buf[off[0]:off[-1]] on torch
    buffers.  bits: a caller's pre-split bitmap (uint64 words) or None (the device pre-splits);
    sp: special-token occurrences, (pos, len, id) numpy arrays or find_specials_device's tuple of
    device tensors; mis: the input's device pointer is this many bytes past a 16-byte boundary.
    -> (ids int64 numpy, offsets int64 numpy, last_counts)."""
    import ctypes

    import torch

    from shredword_amd import _lib
    L, h = _lib.lib(), tok._encoder()
    dev = torch.device("cuda", tok.device)
    off = np.ascontiguousarray(off, dtype=np.int64)
    base, n, n_str = int(off[0]), int(off[-1] - off[0]), len(off) - 1
    raw = torch.zeros(n + 16, dtype=torch.uint8, device=dev)
    assert raw.data_ptr() % 16 == 0
    d_buf = raw[mis:mis + n]
    if n:
        d_buf.copy_(torch.from_numpy(np.ascontiguousarray(buf[base:base + n], dtype=np.uint8)))
    d_off = torch.from_numpy(off - base).to(dev)
    d_out = torch.empty(n + 1, dtype=torch.int16 if out_bits == 16 else torch.int32, device=dev)
    d_oo = torch.empty(n_str + 1, dtype=torch.int64, device=dev)
    d_bits = None if bits is None else torch.from_numpy(np.ascontiguousarray(bits).view(np.int64)).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    n_tok = ctypes.c_int64(-1)
    if entry == "plain":
        assert sp is None and out_bits == 32
        _lib.check(L.sw_encoder_set_option(h, _lib.SW_OPT_PATTERN, pattern))
        _lib.check(L.sw_encode_device(h, d_buf.data_ptr(), n, d_off.data_ptr(), n_str,
                                      d_bits.data_ptr() if d_bits is not None else None, d_out.data_ptr(),
                                      d_oo.data_ptr(), st, ctypes.byref(n_tok)))
    else:
        ex = _lib.SwEncodeEx(d_bits.data_ptr() if d_bits is not None else None, out_bits, pattern=pattern)
        keep = None
        if sp is not None and len(sp[0]):
            keep = sp if torch.is_tensor(sp[0]) else tuple(
                torch.from_numpy(np.ascontiguousarray(x, dtype=t)).to(dev)
                for x, t in zip(sp, (np.int64, np.int32, np.int32)))
            ex.sp_pos, ex.sp_len, ex.sp_id, ex.n_sp = keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[0].numel()
            if len(keep) > 3:
                ex.d_n_sp = keep[3].data_ptr()
        _lib.check(L.sw_encode_device_ex(h, d_buf.data_ptr(), n, d_off.data_ptr(), n_str, ctypes.byref(ex),
                                         d_out.data_ptr(), d_oo.data_ptr(), st, ctypes.byref(n_tok)))
        del keep
    counts = last_counts(tok)
    ids = d_out[:n_tok.value].cpu().numpy()
    ids = ids.view(np.uint16).astype(np.int64) if out_bits == 16 else ids.astype(np.int64)
    return ids, d_oo.cpu().numpy(), counts
