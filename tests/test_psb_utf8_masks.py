"""The class masks of the bit-parallel pre-split (csrc/presplit_bits.h `classify`: the bit-plane
transpose, the dot-product gathers, the UTF-8 lead checks) on the CPU, chunk by chunk as the device
lanes run them (tests/native/psb_masks.cpp), against the host pre-split (sw_presplit_host) for
cl100k and GPT-2: every code point at the chunk offsets where its bytes straddle a chunk end, and
every kind of ill-formed sequence."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from shredword_amd import corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATS = (0, 1)  # cl100k, GPT-2


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="psb_masks_")
    so = os.path.join(d, "psb_masks.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "shredword_amd", "csrc"),
                    "-I", os.path.join(ROOT, "tests", "native"), "-o", so,
                    os.path.join(ROOT, "tests", "native", "psb_masks.cpp")], check=True)
    L = ctypes.CDLL(so)
    L.psb_emul.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    L.psb_emul.restype = ctypes.c_int64
    L.psb_gather_words.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    L.psb_gather32.argtypes = [ctypes.c_void_p]
    L.psb_gather32.restype = ctypes.c_uint32
    L.psb_planes32.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    return L


def check(lib, buf, off):
    """the header's chunk starts == the host pre-split's, both patterns"""
    n = int(off[-1])
    buf = np.ascontiguousarray(buf)
    off = np.ascontiguousarray(off, dtype=np.int64)
    for pat in PATS:
        exp, _ = corpus.presplit(buf, off, pat)
        got = np.zeros(max((n + 63) // 64, 1), dtype=np.uint64)
        assert lib.psb_emul(buf.ctypes.data, off.ctypes.data, len(off) - 1, pat, got.ctypes.data) >= 0
        bad = np.nonzero(got != exp[:len(got)])[0]
        if len(bad):
            w = int(bad[0])
            lo = max(0, w * 64 - 16)
            raise AssertionError("pattern %d: first differing word %d (bytes %r)\n got %s\n exp %s" % (
                pat, w, bytes(buf[lo:w * 64 + 80]), bin(int(got[w]))[::-1], bin(int(exp[w]))[::-1]))


def pack(datas):
    off = np.zeros(len(datas) + 1, dtype=np.int64)
    np.cumsum([len(d) for d in datas], out=off[1:])
    return np.frombuffer(b"".join(datas) or b"\0", dtype=np.uint8)[:int(off[-1])].copy(), off


# ---- generators (tests/test_gpu_split_masks.py draws from them too) -------------------------
FILL = np.frombuffer(b"a1 .\n", dtype=np.uint8)  # a letter, a digit, a space, punctuation, a newline
SLOTS = (28, 32, 61, 94, 127)  # first byte at chunk offsets 28, 0, 29, 30, 31 of a 128-byte record
REC = 128


def utf8_rows(cps):
    """the UTF-8 bytes of the code points (surrogates as their raw three bytes): [len(cps), 4] and lengths"""
    cps = np.asarray(cps, dtype=np.uint32)
    n = np.where(cps < 0x80, 1, np.where(cps < 0x800, 2, np.where(cps < 0x10000, 3, 4)))
    b = np.zeros((len(cps), 4), dtype=np.uint8)
    m = n == 1
    b[m, 0] = cps[m]
    m = n == 2
    b[m, 0] = 0xC0 | (cps[m] >> 6)
    b[m, 1] = 0x80 | (cps[m] & 0x3F)
    m = n == 3
    b[m, 0] = 0xE0 | (cps[m] >> 12)
    b[m, 1] = 0x80 | ((cps[m] >> 6) & 0x3F)
    b[m, 2] = 0x80 | (cps[m] & 0x3F)
    m = n == 4
    b[m, 0] = 0xF0 | (cps[m] >> 18)
    b[m, 1] = 0x80 | ((cps[m] >> 12) & 0x3F)
    b[m, 2] = 0x80 | ((cps[m] >> 6) & 0x3F)
    b[m, 3] = 0x80 | (cps[m] & 0x3F)
    return b, n


def straddle_batch(cps, records_per_string=64):
    """One 128-byte record per code point: the sequence five times, its first byte at offsets 28,
    0, 29, 30 and 31 of a 32-byte chunk (so that it ends at, or straddles, the chunk's end), in a
    filler of letters, digits, spaces, punctuation and newlines whose phase turns with the record,
    so that the neighbours on either side vary.  Strings of 64 records: every 16th record's last
    sequence lies across a multiple of 2048 bytes (a tile boundary of the device kernel)."""
    b, n = utf8_rows(cps)
    R = len(cps)
    total = R * REC + 4
    pos = np.arange(total)
    buf = FILL[(pos + pos // REC) % len(FILL)].copy()
    base = np.arange(R) * REC
    for s in SLOTS:
        for j in range(4):
            m = n > j
            buf[base[m] + s + j] = b[m, j]
    off = list(range(0, R * REC, records_per_string * REC)) + [total]
    return buf, np.asarray(off, dtype=np.int64)


def ill_formed_strings():
    """ill-formed UTF-8 of every kind, each sequence between filler bytes of varying length"""
    fills = [b"a", b" 1", b".\n ", b"x y'", b"12 ab", b"\n", b"'s "]
    seqs = []
    for b0 in range(0x80, 0x100):  # every pair
        for b1 in range(0x100):
            seqs.append(bytes([b0, b1]))
    tails = (0x7F, 0x80, 0xBF, 0xC0)
    for b0 in range(0xE0, 0xF0):  # every 3-byte lead with every second byte
        for b1 in range(0x100):
            for b2 in tails:
                seqs.append(bytes([b0, b1, b2]))
    for b0 in range(0xF0, 0xF8):  # every 4-byte lead with every second byte
        for b1 in range(0x100):
            for b2 in tails:
                for b3 in tails:
                    seqs.append(bytes([b0, b1, b2, b3]))
    datas, cur = [], []
    for i, s in enumerate(seqs):
        cur.append(fills[i % len(fills)] + s)
        if len(cur) == 97:  # (97 sequences a string: the strings' lengths, and so the offsets, vary)
            datas.append(b"".join(cur))
            cur = []
    datas.append(b"".join(cur))
    valid = ["é", "中", "\U0001f642", "ſ", "٣", "　"]
    for v in valid:  # truncated at a string end; a string start inside the sequence at every interior byte
        e = v.encode()
        for cut in range(1, len(e)):
            for pre in (b"", b"a", b"ab 1", b"x" * 29, b"x" * 30, b"x" * 31):
                datas += [pre + e[:cut], e[cut:] + b"b", pre + e[:cut], b"z"]
    datas += [bytes([0x80 + (i % 0x40) for i in range(40)]), b"a" + b"\xbf" * 40 + b"b", b"\x80" * 40]
    return datas


# ---- tests ----------------------------------------------------------------------------------
CP_STEP = 0x4000


@pytest.mark.parametrize("lo", range(0, 0x110000, CP_STEP))
def test_every_code_point_straddling_chunks(lib, lo):
    """Every code point lo .. lo + 0x3FFF (surrogates as raw bytes) at the chunk offsets 0, 28, 29,
    30 and 31, between letters, digits, spaces and punctuation: 2 MiB a case."""
    check(lib, *straddle_batch(np.arange(lo, lo + CP_STEP)))


def test_ill_formed(lib):
    datas = ill_formed_strings()
    for shift in (0, 29):  # (the whole batch at another phase of the chunk grid)
        check(lib, *pack([b"#" * shift] + datas))


def test_bit_gathers(lib):
    """bits8_raw / bits32 / bit_planes32 (their host fallbacks) against the definition: bit k of
    the result = bit B of byte k."""
    rng = np.random.default_rng(7)
    words = [0x80808080, 0x7F7F7F7F, 0, 0xFFFFFFFF, 0x80000000, 0x00000080, 0x08080808, 0xF7F7F7F7]
    words += [int(x) for x in rng.integers(0, 1 << 32, size=2000, dtype=np.uint64)]

    def bits(ws, b):  # the definition
        v = 0
        for i, w in enumerate(ws):
            for k in range(4):
                v |= ((w >> (8 * k + b)) & 1) << (4 * i + k)
        return v

    out = (ctypes.c_uint32 * 3)()
    for i, x in enumerate(words):
        y = words[(i * 7 + 3) % len(words)]
        lib.psb_gather_words(x, y, out)
        assert out[0] == bits([x], 7) and out[1] == bits([x, y], 7) and out[2] == bits([x, y], 3)
    for i in range(0, len(words) - 8, 5):
        ws = words[i:i + 8]
        arr = (ctypes.c_uint32 * 8)(*ws)
        assert lib.psb_gather32(arr) == bits(ws, 7)
        planes = (ctypes.c_uint32 * 8)()
        lib.psb_planes32(arr, planes)
        assert [planes[b] for b in range(8)] == [bits(ws, b) for b in range(8)]
