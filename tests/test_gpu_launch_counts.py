"""What one launch did (sw_encoder_last_counts) against the CPU model of tests/launch_model.py.

The whole-chunk table and the in-launch dedupe fail silently by design: a table miss sends the
chunk to the merge loop and a dedupe miss merges the chunk on its own, both with the same ids.  So
after every launch here the ids and string offsets are compared with the oracle, and then the
counts with the model: out4[0] chunks, out4[1] chunks sent to the merge loop, out4[3] tiles exactly
(out4[1] as a lower bound on ill-formed tables), out4[2] -- the distinct chunks merged -- exactly
wherever no dedupe line can fill, and within the measured bound elsewhere.

Every test makes its own Tokenizer (a fresh handle: the dedupe table's size, and with it which
lines can fill, is part of what is measured)."""
import random

import numpy as np
import pytest

import oracle
import shredword_amd as sa
from shredword_amd import _lib, corpus
from conftest import load_model_merges

import launch_model as lm

pytestmark = pytest.mark.gpu

PAT_ID = {"cl100k": oracle.PAT_CL100K, "gpt2": oracle.PAT_GPT2, "none": oracle.PAT_NONE}
SPECIALS = {"<|endoftext|>": 100257, "<|fim_prefix|>": 100258, "<|fim|>": 100259, "<|": 100260}
TILE = lm.TILE


@pytest.fixture(scope="module", autouse=True)
def need_device():
    if _lib.lib().sw_device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu must run on the MI355X box")


def pack(datas):
    off = np.zeros(len(datas) + 1, dtype=np.int64)
    np.cumsum([len(d) for d in datas], out=off[1:])
    return np.frombuffer(b"".join(datas) or b"\0", dtype=np.uint8)[:int(off[-1])].copy(), off


def shifted(base, by):
    return {(a if a < 256 else a + by, b if b < 256 else b + by): v + by for (a, b), v in base.items()}


def illformed_table(seed=3):
    """test_random_illformed_tables' recipe: random pairs, duplicate values, values below their
    members, ids used before they exist."""
    r = random.Random(seed)
    ids = list(b"abcd ") + list(range(256, 256 + 40))
    merges = {}
    for _ in range(r.randint(5, 300)):
        merges[(r.choice(ids), r.choice(ids))] = r.randint(0, 300) if seed % 2 else r.randint(256, 295)
    return merges


def table(name):
    if name == "illformed":
        return illformed_table()
    if name.startswith("wide"):
        return shifted(load_model_merges("bl32k.model"), 70_000 if name == "wide" else 20_000_000)
    return load_model_merges(name + ".model")


def tokenizer(merges):
    t = sa.Tokenizer(device=0)
    t.merges = merges
    return t


def vocab_words(merges):
    """build_vocab's byte strings of the merge values, in dict order."""
    vocab = {i: bytes([i]) for i in range(256)}
    for (a, b), v in merges.items():
        vocab[v] = vocab[a] + vocab[b]
    return [w for i, w in vocab.items() if i >= 256]


def expect(om, buf, off, pattern, specials=None):
    if specials:
        return om.encode_batch_specials(buf, off, specials, pattern, n_threads=8)
    return om.encode_batch(buf, off, pattern, n_threads=8)


def check_launch(got, exp, model, exact_table=True, distinct=None, what=""):
    """ids and offsets == the oracle's, then the counts == the model's.  distinct: "exact", an int
    (the allowed excess of out4[2] over the model's distinct count), or None: only
    out4[2] >= distinct (which holds whatever the dedupe table's load)."""
    ids, off, c = got
    np.testing.assert_array_equal(off, exp[1], err_msg=what)
    np.testing.assert_array_equal(ids, exp[0], err_msg=what)
    print("%s: out4 %s model %s excess %d" % (what, c, tuple(model), c[2] - model.distinct))
    assert c[0] == model.chunks, (what, c, model)
    assert c[3] == model.tiles, (what, c, model)
    if exact_table:
        assert c[1] == model.to_merge, (what, c, model)
    else:
        assert model.to_merge <= c[1] <= model.multi, (what, c, model)
    if distinct == "exact":
        assert c[2] == model.distinct, (what, c, model)
    else:
        assert model.distinct <= c[2] <= c[1], (what, c, model)
        if distinct is not None:
            assert c[2] <= model.distinct + distinct, (what, c, model)


def set_opt(t, opt, value):
    _lib.check(_lib.lib().sw_encoder_set_option(t._encoder(), opt, value))


# ------------------------------------------------------------------------------- tables and paths
def prose_batch(name):
    """~0.5 MiB: prose of several scripts, the tile-boundary sweep of
    test_tile_boundaries_and_long_chunks, and strings of 1, 2, 16, 17, 32 and 33 bytes (one chunk
    each under the pattern "none": both sides of the table's and the dedupe's length limits)."""
    if name == "illformed":
        r = random.Random(8)
        datas = [bytes(r.choice(b"abcd ") for _ in range(r.randint(0, 120))) for _ in range(5200)]
        datas.append(bytes(r.choice(b"abcd") for _ in range(5000)))
    else:
        buf, off = corpus.synth(17, corpus.MIXED, 1100, 300)
        datas = [buf[off[i]:off[i + 1]].tobytes() for i in range(len(off) - 1)]
        datas += [b"x" * shift + b" hello world the of and" * 150 for shift in range(0, 40)]
    r = random.Random(9)
    for n in (1, 2, 16, 17, 32, 33):
        datas += [bytes(r.choice(b"abcd ") for _ in range(n)) for _ in range(3)] + [(b" the and of it was" * 2)[:n]] * 2
    return pack(datas)


@pytest.mark.parametrize("name", ["bl32k", "toy500", "wide", "wide20m", "illformed"])
def test_counts_per_table_pattern_and_path(name):
    """One batch per table, three patterns, three ways to the classification -- the fused device
    pre-split (k_split_classify), SW_OPT_FUSED_PRESPLIT 0 (the pre-split kernel, then k_classify)
    and a caller's bitmap (k_classify) -- each == the oracle and == the model, so identical to each
    other.  "wide": ids + 70,000 (the wide pair table; chunks still tabled, ids < 2^24);
    "wide20m": ids + 20,000,000, which the table's token field cannot hold: nothing is tabled and
    every chunk of 2 bytes or more goes to the merge loop."""
    merges = table(name)
    om = oracle.OracleModel(merges)
    t = tokenizer(merges)
    buf, off = prose_batch(name)
    assert 1 << 18 <= len(buf) <= 1 << 21
    entries = _lib.lib().sw_encoder_get_info(t._encoder(), _lib.SW_INFO_CHUNK_ENTRIES)
    assert (entries == 0) == (name == "wide20m")
    try:
        for pname, pat in PAT_ID.items():
            exp = expect(om, buf, off, pat)
            model = lm.launch_counts(merges, buf, off, pat, model=om)
            if name == "wide20m":
                assert model.to_merge == model.multi
            elif name != "illformed":
                assert model.to_merge < model.multi  # (the table answers something: the test means something)
            bits, cnt = corpus.presplit(buf, off, pat)
            assert cnt == model.chunks
            seen = []
            for path in ("fused", "unfused", "bitmap"):
                set_opt(t, _lib.SW_OPT_FUSED_PRESPLIT, 0 if path == "unfused" else 1)
                got = lm.device_launch(t, buf, off, pat, entry="plain" if path == "unfused" else "ex",
                                       bits=bits if path == "bitmap" else None)
                check_launch(got, exp, model, exact_table=name != "illformed", what="%s %s %s" % (name, pname, path))
                seen.append(got[2])
            assert [s[:2] + s[3:] for s in seen] == [seen[0][:2] + seen[0][3:]] * 3
    finally:
        t.close()


def test_encode_packed_is_one_launch_with_the_same_counts():
    """Tokenizer.encode_packed under the launch limit is one sw_encode_device launch: the counts
    after it are the model's too (device and host pre-split)."""
    merges = table("bl32k")
    om = oracle.OracleModel(merges)
    t = tokenizer(merges)
    buf, off = prose_batch("bl32k")
    model = lm.launch_counts(merges, buf, off, oracle.PAT_CL100K, model=om)
    exp = expect(om, buf, off, oracle.PAT_CL100K)
    try:
        for host in (0, 1):
            set_opt(t, _lib.SW_OPT_HOST_PRESPLIT, host)
            ids, o = t.encode_packed(buf, off)
            check_launch((ids, o, lm.last_counts(t)), exp, model, what="encode_packed host_presplit=%d" % host)
    finally:
        t.close()


# ---------------------------------------------------------------------------------------- options
# out4[2] - distinct, measured over five runs of each case on an MI355X, a fresh handle each run:
#   mixed             0 0 0 0 0    (1,081 distinct strings, a table of 16,384 entries)
#   lowrep           88 88 88 88 88 (5,333 distinct strings, a table of 16,384 entries = 2,048 lines)
#   lowrep, reserved  0            (the same after sw_encoder_reserve(16 MiB): 65,536 entries in use)
# and 0 for the mixed batch under every option set of test_memoisation_options.  The bound is twice
# the worst value seen.
EXCESS_BOUND = {"mixed": 0, "lowrep": 2 * 88, "lowrep_reserved": 0}


def repeated(buf, off, times):
    total = int(off[-1])
    return np.tile(buf, times), np.concatenate([[0]] + [off[1:] + k * total for k in range(times)]).astype(np.int64)


def mixed_batch():
    """MIXED prose (six scripts, Zipf words), the same 42 KB sixteen times over: a dedupe that works
    removes 15 of 16 merge loops."""
    return repeated(*corpus.synth(7, corpus.MIXED, 40, 1074), 16)


def lowrep_batch():
    """Low-repetition text (ENTROPY: a flat Zipf over 1 M words in six scripts), the same 64 KB
    twelve times over."""
    return repeated(*corpus.synth(31, corpus.ENTROPY, 120, 540), 12)


@pytest.mark.parametrize("case", ["mixed", "lowrep", "lowrep_reserved"])
def test_distinct_count_general(case):
    """out4[2], the merge loops run, against the distinct byte strings of the model.

    dedupe_claim (csrc/kernels.h) gives a chunk 8 candidate entries, all in one 64-byte line chosen
    by the hash of its bytes.  A candidate holding another key is skipped, a free one is claimed by a
    CAS whose loser sees the winner's key and shares it (equality is by bytes: exact keys up to 7
    bytes, a fingerprint then a byte comparison beyond), so the only way a repeated chunk merges again
    is a FULL LINE: 8 other keys already sit in its line, and then every occurrence of it merges on its
    own.  Which line a key goes to depends on its bytes and the table's size alone; timing only
    decides which 8 of a crowded line's keys get in.  A fresh handle sizes the table at one entry per
    64 input bytes (ensure_workspace), 16,384 entries for these batches: the mixed batch's 1,081
    strings fill no line (excess 0 in every run, so equality is asserted); the low-repetition batch's
    5,333 strings overfill a few of the 2,048 lines by 8 keys in all, each occurring 12 times: 88 more
    merge loops than distinct strings, in every run -- bounded here at twice that.  With the workspace
    reserved for 16 MiB first (65,536 entries in use) the same batch merges exactly its distinct
    strings.  Each batch has to_merge >= 10 x distinct (asserted), so a dedupe that stopped matching
    lands an order of magnitude outside these bounds."""
    merges = table("bl32k")
    om = oracle.OracleModel(merges)
    buf, off = mixed_batch() if case == "mixed" else lowrep_batch()
    assert 1 << 18 <= len(buf) <= 1 << 21
    model = lm.launch_counts(merges, buf, off, oracle.PAT_CL100K, model=om)
    assert model.to_merge - model.long_chunks >= 10 * model.distinct > 0, model
    exp = expect(om, buf, off, oracle.PAT_CL100K)
    t = tokenizer(merges)
    try:
        if case == "lowrep_reserved":
            _lib.check(_lib.lib().sw_encoder_reserve(t._encoder(), 16 << 20, 1 << 16))
        got = lm.device_launch(t, buf, off, oracle.PAT_CL100K)
        check_launch(got, exp, model, distinct=EXCESS_BOUND[case], what=case)
    finally:
        t.close()


def test_memoisation_options():
    """SW_OPT_CHUNK_TABLE 0: every chunk of 2 bytes or more goes to the merge loop.  SW_OPT_DEDUPE 0:
    every such chunk of at most 32 bytes runs its own loop.  SW_OPT_DEDUPE_EXACT 0 and
    SW_OPT_DEDUPE_FP_BITS 0 / 3: equality is by bytes, so the fingerprint's width and the exact keys
    change nothing in what is shared -- the same out4[2] as the default."""
    merges = table("bl32k")
    om = oracle.OracleModel(merges)
    buf, off = mixed_batch()
    pat = oracle.PAT_CL100K
    model = lm.launch_counts(merges, buf, off, pat, model=om)
    exp = expect(om, buf, off, pat)
    data, starts, lens, sp_id = lm.split_chunks(buf, off, pat)
    all_short = {data[a:a + n] for a, n in zip(starts.tolist(), lens.tolist()) if 2 <= n <= lm.SHORT}
    t = tokenizer(merges)
    try:
        set_opt(t, _lib.SW_OPT_CHUNK_TABLE, 0)
        no_table = model._replace(to_merge=model.multi, distinct=len(all_short))
        check_launch(lm.device_launch(t, buf, off, pat), exp, no_table, what="chunk table off")
        set_opt(t, _lib.SW_OPT_CHUNK_TABLE, 1)
        set_opt(t, _lib.SW_OPT_DEDUPE, 0)
        no_dedupe = model._replace(distinct=model.to_merge - model.long_chunks)
        check_launch(lm.device_launch(t, buf, off, pat), exp, no_dedupe, distinct="exact", what="dedupe off")
        set_opt(t, _lib.SW_OPT_DEDUPE, 1)
        for exact, fp_bits in ((0, 26), (1, 0), (1, 3), (0, 0), (1, 26)):
            set_opt(t, _lib.SW_OPT_DEDUPE_EXACT, exact)
            set_opt(t, _lib.SW_OPT_DEDUPE_FP_BITS, fp_bits)
            check_launch(lm.device_launch(t, buf, off, pat), exp, model, distinct=EXCESS_BOUND["mixed"],
                         what="exact=%d fp_bits=%d" % (exact, fp_bits))
    finally:
        t.close()


# ------------------------------------------------------------------------------ chunk-table edges
def test_chunk_table_tile_edges():
    """Single-token words of every length 2..16 from the vocabulary (8 | 9: the short and the long
    table), one chunk each (pattern "none": a string is a chunk), placed so that a tabled chunk
    starts at every offset 2030..2047 of a tile with every length -- from offset 2033 on the
    16-byte ones end in the next tile, at 2047 every one does -- with a tabled chunk as the batch's
    first and as its last bytes; and single-token words of 17 bytes or more, which the table does
    not hold: merge-loop chunks.  Every miss here would be a count off by one."""
    merges = table("bl32k")
    om = oracle.OracleModel(merges)
    words = sorted(set(vocab_words(merges)))
    enc = lm.encode_keys(om, words)
    single = {}
    for w in words:
        if len(enc[w]) == 1:
            single.setdefault(len(w), []).append(w)
    assert all(len(single[n]) >= 3 for n in range(2, 19))
    r = random.Random(21)
    datas, pos = [], 0

    def put(w):
        nonlocal pos
        datas.append(w)
        pos += len(w)

    crossing = 0
    put(r.choice(single[9]))  # (the batch's first bytes)
    for o in range(2030, 2048):
        for n in list(range(2, 17)) + [17, 18]:
            while True:  # fill with tabled words (and single bytes) up to offset o of the tile
                room = (o - pos) % TILE
                if room == 0:
                    break
                k = min(room, r.randint(1, 16))
                put(r.choice(single[k]) if k >= 2 else b"e")
            assert pos % TILE == o
            put(r.choice(single[n]))
            crossing += (o + n > TILE)
    put(r.choice(single[16]))  # (the batch's last bytes)
    buf, off = pack(datas)
    assert crossing >= 100 and 1 << 18 <= len(buf) <= 1 << 21
    pat = oracle.PAT_NONE
    model = lm.launch_counts(merges, buf, off, pat, model=om)
    n_over = sum(1 for d in datas if len(d) > 16)
    assert model.to_merge == n_over == 18 * 2 and model.chunks == len(datas)
    exp = expect(om, buf, off, pat)
    bits, _ = corpus.presplit(buf, off, pat)
    t = tokenizer(merges)
    try:
        for mis in (0, 1):
            for use_bits in (False, True):
                got = lm.device_launch(t, buf, off, pat, bits=bits if use_bits else None, mis=mis)
                check_launch(got, exp, model, distinct=0, what="table edges mis=%d bitmap=%d" % (mis, use_bits))
    finally:
        t.close()


# ---------------------------------------------------------------------------------- dedupe edges
def eight_keys():
    """Eight byte strings that are not tabled (checked by the caller through the model): lengths
    2, 5, 7 (exact keys), 8, 8, 13, 17, 32 (fingerprint + byte comparison); the 7-byte one is the
    prefix of both 8-byte ones, which differ in their last byte."""
    keys = [b"q7", b"zq7xj", b"zq7xjkv", b"zq7xjkvA", b"zq7xjkvB", b"0k1j2h3g4f5d6", b"9x8y7z6w5v4u3t2s1",
            b"QzXwVuTsRqPoNmLkJiHgFeDcBa9876_-"]
    assert [len(k) for k in keys] == [2, 5, 7, 8, 8, 13, 17, 32]
    return keys


@pytest.mark.parametrize("mis", [0, 1, 2, 3])
def test_dedupe_eight_keys_exact(mis):
    """At most 8 distinct byte strings go to the merge loop: a key has 8 candidate entries in its
    line, so no line can be full for it and out4[2] must be exactly 8 -- each string 6,000 times
    over 270 tiles, lengths on both sides of the exact keys' 7 bytes, two keys sharing a 7-byte
    prefix, the input pointer 0..3 bytes off a 4-byte boundary (the verification read's
    realignment), and the batch ending in the 13-, the 8- and the 32-byte key so that whichever
    occurrence claims the entry, the others' verification reads reach the input's last word."""
    merges = table("bl32k")
    om = oracle.OracleModel(merges)
    keys = eight_keys()
    r = random.Random(40 + mis)
    datas = [k for k in keys for _ in range(6000)]
    r.shuffle(datas)
    tail = [keys[5], keys[4], keys[7]] * 4
    datas += tail[:len(tail) - mis]  # (the last key differs with mis, and so does the length mod 4)
    buf, off = pack(datas)
    pat = oracle.PAT_NONE
    model = lm.launch_counts(merges, buf, off, pat, model=om)
    assert model.distinct == 8 and model.to_merge == len(datas) and model.tiles >= 256
    exp = expect(om, buf, off, pat)
    t = tokenizer(merges)
    try:
        got = lm.device_launch(t, buf, off, pat, mis=mis)
        check_launch(got, exp, model, distinct="exact", what="eight keys mis=%d" % mis)
        bits, _ = corpus.presplit(buf, off, pat)
        got = lm.device_launch(t, buf, off, pat, bits=bits, mis=mis)
        check_launch(got, exp, model, distinct="exact", what="eight keys, bitmap, mis=%d" % mis)
    finally:
        t.close()


def test_dedupe_first_occurrence_in_the_last_tile():
    """Keys whose every occurrence lies in the last tile, the last one ending at the input's last
    byte (the last_word guard of the verification read), behind 300 tiles of other text; cl100k
    chunks this time (a leading space and letters)."""
    merges = table("bl32k")
    om = oracle.OracleModel(merges)
    r = random.Random(50)
    common = [" zqxjkvw", " qq7", " xkcdzzq", " wvutsrqponmlkjih"]
    late = [" jqzxvkwy", " zzkqxjvwqpgh", " kkzzqqxxjjvvwwppggyyffbbmm"]
    text = "".join(r.choice(common) for _ in range(60000))
    text = text[:(len(text) // TILE) * TILE]  # (whole tiles, cut inside a word: one odd chunk at the cut)
    text += "".join(r.choice(late) for _ in range(60)) + late[1]
    buf, off = pack([text.encode()])
    pat = oracle.PAT_CL100K
    model = lm.launch_counts(merges, buf, off, pat, model=om)
    assert model.distinct <= 8 and model.tiles >= 256 and len(buf) - (model.tiles - 1) * TILE >= 600
    exp = expect(om, buf, off, pat)
    t = tokenizer(merges)
    try:
        for mis in (0, 3):
            got = lm.device_launch(t, buf, off, pat, mis=mis)
            check_launch(got, exp, model, distinct="exact", what="late keys mis=%d" % mis)
    finally:
        t.close()


# --------------------------------------------------------------------------------------- specials
def test_specials_at_tile_edges():
    """k_split_classify<true> / k_classify<true>: special-token occurrences starting at a tile's
    first byte, at its last byte, and ending at its last byte.  Each occurrence is a chunk (out4[0])
    and never a reference to a merge result (out4[1]), found on the host or on the device."""
    merges = table("bl32k")
    om = oracle.OracleModel(merges)
    sp = "<|endoftext|>"
    fill, _ = corpus.synth(23, corpus.ASCII, 700, 1000)
    fill = bytes(b if b != 0x3C else 0x20 for b in fill.tobytes())  # (no '<': no stray "<|")
    out, src = bytearray(), 0
    for tile, at in enumerate([0, TILE - 1, TILE - len(sp), 0, 5, TILE - 1] * 25):
        want = tile * TILE + at
        if want < len(out):
            continue
        out += fill[src:src + want - len(out)]
        src += 4096
        out += sp.encode()
    out += fill[src:src + 3000] + b"<|fim|>"
    cut = [0, 7, len(out) // 2, len(out)]  # (three strings, one empty-free cut inside the text)
    buf, off = np.frombuffer(bytes(out), dtype=np.uint8).copy(), np.array(cut, dtype=np.int64)
    pat = oracle.PAT_CL100K
    model = lm.launch_counts(merges, buf, off, pat, SPECIALS, model=om)
    pos, ln, ids = corpus.find_specials(buf, off, SPECIALS)
    assert model.specials == len(pos) >= 100 and 1 << 18 <= len(buf) <= 1 << 21
    for at in (0, TILE - 1, TILE - len(sp)):
        assert int(((pos % TILE == at) & (ln == len(sp))).sum()) >= 20
    exp = expect(om, buf, off, pat, SPECIALS)
    t = tokenizer(merges)
    t.special_tokens = dict(SPECIALS)
    try:
        import torch
        check_launch(lm.device_launch(t, buf, off, pat, sp=(pos, ln, ids)), exp, model,
                     what="specials, host-found, fused")
        bits, cnt = corpus.presplit_specials(buf, off, pos, ln, pat)
        assert cnt == model.chunks
        check_launch(lm.device_launch(t, buf, off, pat, sp=(pos, ln, ids), bits=bits), exp, model,
                     what="specials, host-found, bitmap")
        d_buf, d_off = torch.from_numpy(buf).to("cuda:0"), torch.from_numpy(off).to("cuda:0")
        found = t.find_specials_device(d_buf, d_off, n_bytes=len(buf))
        check_launch(lm.device_launch(t, buf, off, pat, sp=found), exp, model,
                     what="specials, device-found, fused")
        assert int(found[3].item()) == len(pos)
    finally:
        t.close()
