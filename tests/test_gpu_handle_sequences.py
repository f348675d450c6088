"""One encoder handle driven through a seeded, deliberately mixed sequence of launches.

A handle carries state from launch to launch: the workspace's capacity, the dedupe table's size
after growth and the prefix a smaller launch clears, the compaction kernel picked from the previous
launch's ids per tile, the staged result heads a grown table switches on, the specials finder's
arrays, the tile count of the last launch.  Every step of a sequence runs on the same handle and is
checked against the oracle (ids and string offsets) and, where the step is one launch, against the
count model of tests/launch_model.py (chunks, chunks sent to the merge loop and tiles exactly; the
merge loops run at least the distinct chunks, and exactly where at most 8 byte strings are merged).

A sequence is make_sequence(seed): 30-40 steps, the forced orderings below in a seeded order with
seeded random steps between them.  A failure names the seed, the step's index and its choices;
`make_sequence(seed)[index]` is that step again."""
import ctypes
import random

import numpy as np
import pytest

import oracle
import shredword_amd as sa
from shredword_amd import _lib, corpus
from conftest import load_model_merges

import launch_model as lm

pytestmark = pytest.mark.gpu

PATTERNS = {"cl100k": oracle.PAT_CL100K, "gpt2": oracle.PAT_GPT2, "none": oracle.PAT_NONE}
TOK_PATTERN = {"cl100k": "", "gpt2": sa.GPT2_PATTERN, "none": 2}
SPECIAL_SETS = {
    "a": {"<|endoftext|>": 100257, "<|fim_prefix|>": 100258, "<|fim|>": 100259, "<|": 100260},
    "b": {"\n\n": 100300, "<|endoftext|>": 100257, "the": 100301},
}
KINDS = {"ascii": corpus.ASCII, "mixed": corpus.MIXED, "stress": corpus.STRESS, "entropy": corpus.ENTROPY}
SIZES = (0, 1, 63, 2047, 2048, 2049, 70_000, 1_000_000, 4_000_000)
ENTRIES = ("packed", "plain", "ex", "ex_bits", "presplit", "find")


@pytest.fixture(scope="module", autouse=True)
def need_device():
    if _lib.lib().sw_device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu must run on the MI355X box")


# ------------------------------------------------------------------------------------------ batches
def pack(datas):
    off = np.zeros(len(datas) + 1, dtype=np.int64)
    np.cumsum([len(d) for d in datas], out=off[1:])
    return np.frombuffer(b"".join(datas) or b"\0", dtype=np.uint8)[:int(off[-1])].copy(), off


_BATCH = {}


def batch(name):
    """A named batch -> (buf, off), made once.  Names: "<kind>:<bytes>:<mean>" (a synthetic corpus
    cut to exactly that many bytes, at most 20,000 strings, the strings past the cut empty),
    "onebyte:<n>" (n one-byte strings), "empty:<n>" (n empty strings), and the forced orderings'."""
    if name in _BATCH:
        return _BATCH[name]
    kind, _, rest = name.partition(":")
    r = random.Random(name)
    if kind in KINDS:
        size, mean = (int(x) for x in rest.split(":"))
        n_str = max(1, min(20000, size // mean + 3))
        buf, off = corpus.synth(len(name) + size, KINDS[kind], n_str, mean)
        while len(buf) < size:  # (a corpus that came out short: the same strings again)
            buf, off = np.concatenate([buf, buf]), np.concatenate([off, off[1:] + off[-1]])
        buf, off = buf[:size].copy(), np.minimum(off, size)[:20001]
        off[-1] = size
    elif kind == "onebyte":
        buf, off = pack([bytes([r.choice(b"abcxyz \n")]) for _ in range(int(rest))])
    elif kind == "empty":
        buf, off = np.zeros(0, np.uint8), np.zeros(int(rest) + 1, np.int64)
    elif name == "overflow":  # test_dedupe_table_grows_and_clears_itself's recipe: low-repetition text
        buf, off = corpus.synth(31, corpus.ENTROPY, 3900, 1074)
    elif name == "eight":  # at most 8 distinct byte strings for the merge loop, one chunk a string
        keys = [b"q7", b"zq7xj", b"zq7xjkv", b"zq7xjkvA", b"zq7xjkvB", b"0k1j2h3g4f5d6", b"9x8y7z6w5v4u3t2s1",
                b"QzXwVuTsRqPoNmLkJiHgFeDcBa9876_-"]
        buf, off = pack([r.choice(keys) for _ in range(12000)])
    elif name == "dense":  # test_compaction_kernel_choice's: many short ids per tile
        g = np.random.default_rng(11)
        off = np.concatenate([[0], np.cumsum(g.integers(1, 600, size=3000))]).astype(np.int64)
        buf = g.integers(128, 256, size=int(off[-1]), dtype=np.uint8)
    elif name == "long4096":  # 4096-byte chunks (letters, a letter run, spaces) between STRESS strings
        sbuf, soff = corpus.synth(4, corpus.STRESS, 300, 600)
        datas = []
        for i in range(len(soff) - 1):
            datas.append(sbuf[soff[i]:soff[i + 1]].tobytes())
            if i % 10 == 0:
                datas.append((bytes(r.choice(b"abcdefghij") for _ in range(4096)), b"a" * 4096, b" " * 4096)[i // 10 % 3])
        buf, off = pack(datas)
    else:
        raise KeyError(name)
    _BATCH[name] = (buf, off)
    return _BATCH[name]


_SPLICED = {}


def spliced(name, sp_name):
    """The batch with the special set's tokens spliced in (made once)."""
    key = (name, sp_name)
    if key not in _SPLICED:
        buf, off = batch(name)
        if len(buf) == 0:
            _SPLICED[key] = (buf, off)
        else:
            _SPLICED[key] = corpus.splice_specials(buf, off, SPECIAL_SETS[sp_name], per_kib=3.0, end_special=0,
                                                   seed=len(name))
    return _SPLICED[key]


_EXPECT = {}


def expectation(table, merges, om, name, pattern, sp_name, want_model):
    """(buf, off, expected ids, expected offsets, model counts or None), computed once per table,
    batch, pattern and special set and shared by every sequence."""
    key = (table, name, pattern, sp_name)
    buf, off = spliced(name, sp_name) if sp_name else batch(name)
    if key not in _EXPECT:
        sp = SPECIAL_SETS[sp_name] if sp_name else None
        pat = PATTERNS[pattern]
        ids, o = (om.encode_batch_specials(buf, off, sp, pat, n_threads=8) if sp else
                  om.encode_batch(buf, off, pat, n_threads=8))
        _EXPECT[key] = [ids, o, None]
    if want_model and _EXPECT[key][2] is None:
        sp = SPECIAL_SETS[sp_name] if sp_name else None
        _EXPECT[key][2] = lm.launch_counts(merges, buf, off, PATTERNS[pattern], sp, model=om)
    return (buf, off) + tuple(_EXPECT[key])


# ----------------------------------------------------------------------------------------- sequences
def random_step(r, size):
    kind = r.choice(list(KINDS) + ["onebyte"])
    if size >= 1_000_000:  # (the large references are few: shared by all sequences)
        kind, pattern, sp = ("mixed" if size > 1_000_000 else r.choice(["ascii", "stress"])), "cl100k", None
        name = "%s:%d:1074" % (kind, size)
    else:
        if size == 0:
            name = "empty:%d" % r.choice([0, 1, 5])
        elif kind == "onebyte" and size <= 20000:
            name = "onebyte:%d" % size
        else:
            name = "%s:%d:%d" % ("mixed" if kind == "onebyte" else kind, size, r.choice([3, 40, 300, 1074]))
        pattern = r.choice(list(PATTERNS))
        sp = r.choice([None, None, "a", "b"])
    entry = r.choice(ENTRIES)
    step = {"batch": name, "pattern": pattern, "specials": sp, "entry": entry, "timing": r.random() < 0.5,
            "out_bits": 32, "finder": None, "mis": r.choice([0, 0, 1, 2, 3])}
    if entry == "find" and sp is None and size < 1_000_000:
        step["specials"] = r.choice(["a", "b", None])  # (None: set_specials back to no specials)
    if entry == "presplit":
        step["specials"] = None
    if entry == "plain":
        step["specials"] = None  # (sw_encode_device takes no occurrences)
    if step["specials"] and step["entry"] in ("ex", "ex_bits"):
        step["finder"] = "host" if step["entry"] == "ex_bits" else r.choice(["host", "device"])
    if step["specials"] is None and step["entry"] in ("ex", "ex_bits") and r.random() < 0.4:
        step["out_bits"] = 16
    return step


def forced(name, **kw):
    step = {"batch": name, "pattern": "cl100k", "specials": None, "entry": "ex", "timing": False, "out_bits": 32,
            "finder": None, "mis": 0}
    step.update(kw)
    return step


def make_sequence(seed):
    """The steps of sequence `seed` (dicts).  Forced orderings, each kept together, in a seeded order:
      big     the largest batch, then 1 byte, then the largest again (capacity, stale tiles);
      grow    a launch that overflows the dedupe table, the same again (it grows the table), a 2 KiB launch (the
              prefix clear of the grown table), then at most 8 distinct strings (exact merge count);
      compact many short ids per tile, then few, then many (the compaction kernel picked from the
              previous launch's ids per tile);
      long    4096-byte chunks, then a batch without long chunks (stale long lists and counters)."""
    r = random.Random(seed)
    blocks = {
        "big": [forced("mixed:4000000:1074", entry=r.choice(["ex", "packed"])),
                forced("ascii:1:1074", entry=r.choice(["ex", "plain", "packed"])),
                forced("mixed:4000000:1074", entry=r.choice(["ex", "plain"]))],
        "grow": [forced("overflow", entry="packed", check="before_grow"),
                 forced("overflow", entry=r.choice(["ex", "packed"]), check="grown"),
                 forced("ascii:2048:300", entry=r.choice(["ex", "plain"])),
                 forced("eight", pattern="none", entry=r.choice(["ex", "ex_bits"]), check="exact", mis=r.choice([0, 1, 2, 3]))],
        "compact": [forced("dense"), forced(r.choice(["stress:70000:300", "ascii:70000:1074"])), forced("dense")],
        "long": [forced("long4096", entry=r.choice(["ex", "ex_bits", "packed"])),
                 forced("onebyte:20000", entry=r.choice(["ex", "plain"])),
                 forced("mixed:70000:40")],
    }
    order = list(blocks)
    r.shuffle(order)
    steps = []
    n_random = r.randint(17, 27)  # (+ 13 forced: 30 .. 40 steps)
    sizes = [x for _ in range(3) for x in r.sample(SIZES, len(SIZES))]  # (every size in every sequence)
    nxt = iter(sizes)
    cuts = sorted(r.randint(0, n_random) for _ in range(len(order)))
    done = 0
    for name, cut in zip(order, cuts):
        steps += [random_step(r, next(nxt)) for _ in range(cut - done)]
        done = cut
        steps += blocks[name]
    steps += [random_step(r, next(nxt)) for _ in range(n_random - done)]
    assert 30 <= len(steps) <= 40
    return steps


# --------------------------------------------------------------------------------------------- steps
def bare_presplit(t, buf, off, pattern):
    """sw_presplit_device on the encoder's workspace -> (bitmap uint64 words, chunk count)."""
    import torch
    dev = torch.device("cuda", 0)
    n = len(buf)
    d_buf = torch.from_numpy(buf if n else np.zeros(1, np.uint8)).to(dev)
    d_off = torch.from_numpy(off).to(dev)
    d_bits = torch.full((max((n + 63) // 64, 1),), -1, dtype=torch.int64, device=dev)
    cnt = ctypes.c_int64(-1)
    _lib.check(_lib.lib().sw_presplit_device(t._encoder(), d_buf.data_ptr(), n, d_off.data_ptr(), len(off) - 1, pattern,
                                             d_bits.data_ptr(), torch.cuda.current_stream(dev).cuda_stream,
                                             ctypes.byref(cnt)))
    return d_bits.cpu().numpy().view(np.uint64)[:(n + 63) // 64], cnt.value


def run_step(t, table, merges, om, step, state):
    L, h = _lib.lib(), t._encoder()
    name, pattern, sp_name, entry = step["batch"], step["pattern"], step["specials"], step["entry"]
    pat = PATTERNS[pattern]
    sp = SPECIAL_SETS[sp_name] if sp_name else None
    one_launch = entry in ("packed", "plain", "ex", "ex_bits")
    buf, off, e_ids, e_off, model = expectation(table, merges, om, name, pattern, sp_name,
                                                want_model=(one_launch and name != "overflow") or entry == "presplit")
    _lib.check(L.sw_encoder_set_timing(h, 1 if step["timing"] else 0))
    if step.get("check") == "before_grow":
        state["slots"] = L.sw_encoder_get_info(h, _lib.SW_INFO_DEDUPE_SLOTS)
    got = counts = None
    if entry == "packed":
        t.pattern = TOK_PATTERN[pattern]
        ids, o = t.encode_packed(buf, off, specials=sp)
        got, counts = (ids, o), lm.last_counts(t)
    elif entry == "plain":
        ids, o, counts = lm.device_launch(t, buf, off, pat, entry="plain", mis=step["mis"])
        got = (ids, o)
    elif entry in ("ex", "ex_bits"):
        # (the handle's own pattern option set to another pattern: the call's must win)
        _lib.check(L.sw_encoder_set_option(h, _lib.SW_OPT_PATTERN, (pat + 1) % 3))
        occ = bits = None
        if sp:
            pos, ln, sid = corpus.find_specials(buf, off, sp)
            occ = (pos, ln, sid)
            if step["finder"] == "device":
                import torch
                t.special_tokens = dict(sp)
                d_buf = torch.from_numpy(buf if len(buf) else np.zeros(1, np.uint8)).to("cuda:0")
                occ = t.find_specials_device(d_buf, torch.from_numpy(off).to("cuda:0"), n_bytes=len(buf))
            if entry == "ex_bits":
                bits, _ = corpus.presplit_specials(buf, off, pos, ln, pat)
        elif entry == "ex_bits":
            bits, _ = corpus.presplit(buf, off, pat)
        ids, o, counts = lm.device_launch(t, buf, off, pat, bits=bits, sp=occ, out_bits=step["out_bits"], mis=step["mis"])
        got = (ids, o)
    elif entry == "presplit":  # a bare device pre-split between two encodes: the host's bitmap
        bits, cnt = bare_presplit(t, buf, off, pat)
        h_bits, h_cnt = corpus.presplit(buf, off, pat)
        assert cnt == h_cnt == model.chunks
        np.testing.assert_array_equal(bits, h_bits[:len(bits)])
    elif entry == "find":  # a bare device finder (set_specials with this step's set): the host finder's
        import torch
        t.special_tokens = dict(sp or {})
        d_buf = torch.from_numpy(buf if len(buf) else np.zeros(1, np.uint8)).to("cuda:0")
        pos, ln, sid, cnt, n = t.find_specials_device(d_buf, torch.from_numpy(off).to("cuda:0"), n_bytes=len(buf), sync=True)
        h_pos, h_len, h_id = corpus.find_specials(buf, off, sp or {})
        assert n == int(cnt.item()) == len(h_pos)
        np.testing.assert_array_equal(pos[:n].cpu().numpy(), h_pos)
        np.testing.assert_array_equal(ln[:n].cpu().numpy(), h_len)
        np.testing.assert_array_equal(sid[:n].cpu().numpy(), h_id)
    if got is not None:
        np.testing.assert_array_equal(got[1], e_off)
        np.testing.assert_array_equal(got[0], e_ids)
    if counts is not None and model is not None:
        assert counts[0] == model.chunks and counts[3] == model.tiles, (counts, model)
        assert counts[1] == model.to_merge, (counts, model)
        assert model.distinct <= counts[2] <= counts[1] - model.long_chunks, (counts, model)
        if step.get("check") == "exact":
            assert model.distinct <= 8 and counts[2] == model.distinct, (counts, model)
    if got is not None and len(buf):
        # (a host batch call times its own launches for its stats and puts the caller's window back)
        if entry == "packed":
            assert t.last_stats.ms_kernels > 0
        assert (L.sw_encoder_last_kernel_ms(h) > 0) == (step["timing"] and entry != "packed")
    if step.get("check") == "grown":
        assert L.sw_encoder_get_info(h, _lib.SW_INFO_DEDUPE_SLOTS) > state["slots"]


@pytest.mark.parametrize("table", ["bl32k", "toy500"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_mixed_sequence_on_one_handle(seed, table):
    merges = load_model_merges(table + ".model")
    om = oracle.OracleModel(merges)
    t = sa.Tokenizer(device=0)
    t.merges = merges
    steps = make_sequence(seed)
    state = {}
    try:
        for i, step in enumerate(steps):
            try:
                run_step(t, table, merges, om, step, state)
            except Exception as e:
                raise AssertionError("sequence seed=%d table=%s step %d of %d: %r\n%s: %s" % (
                    seed, table, i, len(steps), step, type(e).__name__, e)) from e
    finally:
        t.close()


def test_sequences_are_reproducible_and_cover_the_choices():
    """make_sequence is a function of the seed alone, and the three seeds together take every
    entry point, pattern, special set, finder, output width and size."""
    seqs = {s: make_sequence(s) for s in (1, 2, 3)}
    assert all(make_sequence(s) == seqs[s] for s in seqs)
    steps = [x for s in seqs.values() for x in s]
    assert {x["entry"] for x in steps} == set(ENTRIES)
    assert {x["pattern"] for x in steps} == set(PATTERNS)
    assert {x["specials"] for x in steps} == {None, "a", "b"}
    assert {x["finder"] for x in steps} == {None, "host", "device"}
    assert {x["out_bits"] for x in steps} == {16, 32} and {x["timing"] for x in steps} == {True, False}
    for seq in seqs.values():
        assert set(SIZES) <= {len(batch(x["batch"])[0]) for x in seq}
