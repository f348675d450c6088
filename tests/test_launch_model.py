"""The CPU model of the per-launch counts (tests/launch_model.py) against what pins it: its chunking
and per-chunk encodings concatenate to the oracle's batch encode (and so to the reference-generated
fixtures), its chunk count is the popcount of the host pre-split bitmap, and its counts keep their
invariants -- on the committed fixtures and one synthetic batch per corpus kind, with and without
special tokens.  No GPU."""
import numpy as np
import pytest

import oracle
from shredword_amd import corpus
from conftest import PATTERNS, golden_index, load_fixture, load_model_merges

import launch_model as lm

FIXTURES = golden_index()["fixtures"]
SPECIALS = {"<|endoftext|>": 100257, "<|fim_prefix|>": 100258, "<|fim|>": 100259, "<|": 100260}
KINDS = {"ascii": corpus.ASCII, "mixed": corpus.MIXED, "stress": corpus.STRESS, "entropy": corpus.ENTROPY}


def popcount(bits):
    return int(np.unpackbits(np.ascontiguousarray(bits).view(np.uint8)).sum())


def check_invariants(c, n_bytes):
    assert 0 <= c.distinct <= c.to_merge <= c.multi <= c.chunks <= n_bytes
    assert c.long_chunks <= c.to_merge and c.distinct <= c.to_merge - c.long_chunks
    assert c.tiles == (n_bytes + 2047) // 2048
    assert c.tiles * 2048 >= n_bytes > (c.tiles - 1) * 2048 or n_bytes == 0


@pytest.mark.parametrize("entry", FIXTURES, ids=[e["file"] for e in FIXTURES])
def test_model_on_fixtures(entry):
    """Chunk encodings concatenated == the reference-generated ids == the oracle's batch encode; the
    chunk count == the host pre-split bitmap's popcount; every distinct chunk's batched encoding ==
    OracleModel.encode_chunk."""
    fx = load_fixture(entry)
    merges = load_model_merges(entry["model"])
    om = oracle.OracleModel(merges)
    pat = PATTERNS[entry["pattern"]]
    buf, off = fx["bytes"], fx["off"]
    ids = lm.chunk_ids(merges, buf, off, pat, model=om)
    np.testing.assert_array_equal(ids, fx["ids"])
    np.testing.assert_array_equal(ids, om.encode_batch(buf, off, pat)[0])
    c = lm.launch_counts(merges, buf, off, pat, model=om)
    bits, cnt = corpus.presplit(buf, off, pat)
    assert c.chunks == cnt == popcount(bits)
    data, starts, lens, sp_id = lm.split_chunks(buf, off, pat)
    assert np.array_equal(np.flatnonzero(np.unpackbits(bits.view(np.uint8), bitorder="little")[:len(data)]), starts)
    check_invariants(c, len(data))
    keys = {data[a:a + n] for a, n in zip(starts.tolist(), lens.tolist())}
    enc = lm.encode_keys(om, keys)
    for k in keys:
        assert list(enc[k]) == om.encode_chunk(k), k
    if om.well_formed:
        # a tabled chunk is its token's byte string: distinct tabled chunks <= vocabulary entries
        assert len({k for k in keys if lm.is_tabled(k, enc[k])}) <= len(merges)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("pattern", ["cl100k", "gpt2", "none"])
def test_model_on_synthetic_batches(kind, pattern):
    """One corpus.synth batch per kind: the same checks against the oracle, without and with
    special tokens spliced in (each occurrence one chunk, the text between pre-split on its own)."""
    merges = load_model_merges("bl32k.model")
    om = oracle.OracleModel(merges)
    pat = PATTERNS[pattern]
    buf, off = corpus.synth(41, KINDS[kind], 300, 500)
    np.testing.assert_array_equal(lm.chunk_ids(merges, buf, off, pat, model=om), om.encode_batch(buf, off, pat)[0])
    c = lm.launch_counts(merges, buf, off, pat, model=om)
    bits, cnt = corpus.presplit(buf, off, pat)
    assert c.chunks == cnt == popcount(bits) and c.specials == 0
    check_invariants(c, len(buf))
    if pattern == "none":
        assert c.chunks == int((np.diff(off) > 0).sum())

    sbuf, soff = corpus.splice_specials(buf, off, SPECIALS, per_kib=4.0, end_special=0)
    np.testing.assert_array_equal(lm.chunk_ids(merges, sbuf, soff, pat, SPECIALS, model=om),
                                  om.encode_batch_specials(sbuf, soff, SPECIALS, pat)[0])
    cs = lm.launch_counts(merges, sbuf, soff, pat, SPECIALS, model=om)
    pos, ln, ids = corpus.find_specials(sbuf, soff, SPECIALS)
    sbits, scnt = corpus.presplit_specials(sbuf, soff, pos, ln, pat)
    assert cs.chunks == scnt == popcount(sbits)
    assert cs.specials == len(pos) >= len(off) - 1
    data, starts, lens, sp_id = lm.split_chunks(sbuf, soff, pat, SPECIALS)
    at = np.flatnonzero(sp_id >= 0)
    np.testing.assert_array_equal(starts[at], pos)
    np.testing.assert_array_equal(lens[at], ln)
    np.testing.assert_array_equal(sp_id[at], ids)
    check_invariants(cs, len(sbuf))


def test_find_specials_rule():
    """Leftmost first, dict order at one position, empty specials never match, the scan goes on
    after the occurrence -- the oracle's encode_with_specials on the same strings."""
    om = oracle.OracleModel({})
    for sp in ({"aa": 300, "aaa": 301}, {"aaa": 301, "aa": 300, "a": 299}, {"ab": 310, "ba": 311, "aba": 312},
               {"<|a|>": 320, "<|a": 321, "|>": 322, "": 323}):
        for text in ("", "a", "aaaaaaa", "abababa", "xx<|a|><|a|>|>", "<|a", "ba" * 9 + "a", "zzz"):
            found = lm.find_specials(text.encode(), sp)
            exp = om.encode_with_specials(text, sp, oracle.PAT_NONE)
            got, p = [], 0
            for q, n, v in found:
                got += list(text.encode()[p:q]) + [v]
                p = q + n
            assert got + list(text.encode()[p:]) == exp, (sp, text)


def test_counts_by_hand():
    """A table small enough to count by hand: merges a+b -> 256, 256+c -> 257.  Strings (pattern
    none): "a" single byte; "ab", "abc" tabled; "ac" two ids; "abcabc" two ids; 33 and 40 bytes long."""
    merges = {(97, 98): 256, (256, 99): 257}
    datas = [b"a", b"ab", b"abc", b"ac", b"ac", b"abcabc", b"", b"x" * 33, b"x" * 33, b"y" * 40, b"abc"]
    off = np.zeros(len(datas) + 1, np.int64)
    np.cumsum([len(d) for d in datas], out=off[1:])
    buf = np.frombuffer(b"".join(datas), np.uint8)
    c = lm.launch_counts(merges, buf, off, oracle.PAT_NONE)
    assert c == lm.Counts(chunks=10, to_merge=6, distinct=2, tiles=1, long_chunks=3, multi=9, specials=0)
    wide = {(97, 98): 1 << 24, ((1 << 24), 99): (1 << 24) + 1}  # ids the table's token field cannot hold
    c = lm.launch_counts(wide, buf, off, oracle.PAT_NONE)
    assert (c.to_merge, c.distinct) == (9, 4)
