"""The class masks of the device pre-split on the GPU (presplit_bits.h `classify` with the device
instructions behind its helpers: v_perm_b32, v_bfi_b32, v_dot4_u32_u8), standalone
(sw_presplit_device) and fused into the classification (k_split_classify, whose arguments are read
through the kernel-argument segment), on small batches where the kernel can still go wrong: tile
edges, the aligned and the unaligned staging path, dense non-ASCII tiles, tiny batches, runs that
send a tile to k_split_redo, special tokens at tile boundaries.  Everything must equal the host
pre-split (sw_presplit_host), resp. the encode given the host bitmap and the oracle."""
import ctypes
import random

import numpy as np
import pytest

import oracle
import shredword_amd as sa
from shredword_amd import _lib, corpus
from conftest import load_model_merges
from test_psb_utf8_masks import ill_formed_strings, pack, straddle_batch

pytestmark = pytest.mark.gpu

PATS = [_lib.SW_PAT_CL100K, _lib.SW_PAT_GPT2]
TILE = 2048


@pytest.fixture(scope="module")
def tok():
    t = sa.Tokenizer(device=0)
    t.merges = load_model_merges("bl32k.model")
    yield t
    t.close()


def to_device(buf, off, shift):
    """the batch on the device, its first byte `shift` bytes past an aligned address"""
    import torch
    dev = torch.device("cuda", 0)
    n = int(off[-1])
    big = torch.zeros(n + 64, dtype=torch.uint8, device=dev)
    assert big.data_ptr() % 16 == 0
    d_buf = big[shift:shift + max(n, 1)]
    d_buf[:n] = torch.from_numpy(np.ascontiguousarray(buf[:n])).to(dev)
    return d_buf, torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).to(dev)


def device_bits(tok, d_buf, d_off, n, pattern):
    import torch
    d_bits = torch.full((max((n + 63) // 64, 1),), -1, dtype=torch.int64, device=d_buf.device)
    cnt = ctypes.c_int64()
    _lib.check(_lib.lib().sw_presplit_device(tok._encoder(), d_buf.data_ptr(), n, d_off.data_ptr(), d_off.numel() - 1,
                                             pattern, d_bits.data_ptr(),
                                             torch.cuda.current_stream(d_buf.device).cuda_stream, ctypes.byref(cnt)))
    torch.cuda.synchronize()
    return d_bits.cpu().numpy().view(np.uint64)


def check(tok, buf, off, shifts=(0,), pats=PATS):
    """standalone bitmap == host bitmap; fused ids == ids of the encode given the host bitmap"""
    import torch
    n = int(off[-1])
    for pat in pats:
        exp, _ = corpus.presplit(buf, off, pat)
        tok.pattern = "" if pat == _lib.SW_PAT_CL100K else sa.GPT2_PATTERN
        ref = None
        for shift in shifts:
            d_buf, d_off = to_device(buf, off, shift)
            got = device_bits(tok, d_buf, d_off, n, pat)
            np.testing.assert_array_equal(got, exp[:len(got)], err_msg="pattern %d shift %d" % (pat, shift))
            fused = tok.encode_device(d_buf, d_off, n_bytes=n)
            if ref is None:
                d_bits = torch.from_numpy(exp.view(np.int64)).to(d_buf.device)
                ref = [x.cpu().numpy() for x in tok.encode_device(d_buf, d_off, d_bits=d_bits, n_bytes=n)]
            np.testing.assert_array_equal(fused[1].cpu().numpy(), ref[1], err_msg="pattern %d shift %d" % (pat, shift))
            np.testing.assert_array_equal(fused[0].cpu().numpy(), ref[0], err_msg="pattern %d shift %d" % (pat, shift))
    tok.pattern = ""


def test_five_tiles_aligned_and_offset(tok):
    """10 KiB (5 tiles: 1..3 take the aligned staging path, 0 and 4 the slow one) of ~40 strings from
    the CPU tests' generators; then the same bytes one byte past an aligned address (every tile
    takes the slow path)."""
    rng = random.Random(3)
    sbuf, soff = straddle_batch(np.array([0xE9, 0x17F, 0x4E2D, 0xD7FF, 0xD800, 0x1F642, 0x10FFFF, 0x3000, 0x663, 0x85,
                                          0x41, 0x27, 0x2028, 0xFFFD, 0x20000, 0xA0] * 2), records_per_string=4)
    pieces = [bytes(sbuf[int(soff[i]):int(soff[i + 1])]) for i in range(len(soff) - 1)]
    bad = ill_formed_strings()
    pieces += [bad[i][:300] for i in rng.sample(range(800), 24)]       # (pairs, 3- and 4-byte sequences)
    pieces += [bad[i] for i in rng.sample(range(850, len(bad)), 12)]  # (truncated and cut sequences, lone tails)
    pieces += [b"it's we'll they'RE don't", " 12345 \r\n\r\n  x".encode(), b""]
    rng.shuffle(pieces)
    data = b"".join(pieces)[:5 * TILE]
    cut = sorted(rng.sample(range(1, len(data)), 39))
    off = np.array([0] + cut + [len(data)], dtype=np.int64)
    assert len(data) == 5 * TILE
    check(tok, np.frombuffer(data, dtype=np.uint8).copy(), off, shifts=(0, 1))


@pytest.mark.parametrize("kind", ["latin2", "cjk3", "emoji4", "invalid", "alternate"])
def test_dense_non_ascii_tile(tok, kind):
    """One tile of 2-byte letters / 3-byte CJK / 4-byte emoji / invalid bytes 0x80..0xFF / alternating
    ASCII letter and CJK (the worst lane imbalance), between two ASCII tiles."""
    rng = random.Random(11)
    if kind == "latin2":
        mid = "".join(chr(rng.randrange(0xC0, 0x250)) for _ in range(TILE // 2)).encode()
    elif kind == "cjk3":
        mid = "".join(chr(rng.randrange(0x4E00, 0x9FFF)) for _ in range(TILE // 3)).encode() + b"ab"
    elif kind == "emoji4":
        mid = "".join(chr(rng.randrange(0x1F600, 0x1F650)) for _ in range(TILE // 4)).encode()
    elif kind == "invalid":
        mid = bytes(rng.randrange(0x80, 0x100) for _ in range(TILE))
    else:
        mid = "".join("a" + chr(rng.randrange(0x4E00, 0x9FFF)) for _ in range(TILE // 4)).encode()
    assert len(mid) == TILE
    asc = ("Hello world, it's 2024.\n" * 100).encode()[:TILE]
    data = asc + mid + asc
    check(tok, np.frombuffer(data, dtype=np.uint8).copy(), np.array([0, 700, TILE + 5, 2 * TILE + 1, 3 * TILE], np.int64))


@pytest.mark.parametrize("n", [1, 31, 32, 33, 2047, 2048, 2049])
def test_tiny_batches(tok, n):
    """n bytes as one string, and as n strings of one byte"""
    data = ("a é中1 '\n😀." * 300).encode()[:n]
    buf = np.frombuffer(data, dtype=np.uint8).copy()
    check(tok, buf, np.array([0, n], dtype=np.int64))
    check(tok, buf, np.arange(n + 1, dtype=np.int64))


def test_runs_across_a_tile_take_the_redo_kernel(tok):
    """A digit run and a \\r\\n run crossing a tile boundary in a 6 KiB batch: the tiles go to
    k_split_redo, which still takes its arguments by value."""
    data = b"x" * 1500 + b"7" * 1200 + b" word." + b"\r\n" * 700 + b" z" + b"y" * 100
    data = (data + b" tail" * 1000)[:3 * TILE]
    check(tok, np.frombuffer(data, dtype=np.uint8).copy(), np.array([0, 3 * TILE], dtype=np.int64))


def test_specials_at_a_tile_boundary(tok):
    """k_split_classify<true>: an 8 KiB batch with one occurrence ending at a tile boundary and one
    spanning the next; against the oracle."""
    import torch
    sp = {"<|endoftext|>": 100257}
    s = "<|endoftext|>"
    text = "a" * (TILE - len(s)) + s + " b1" * ((TILE - 8) // 3)
    text += "c" * (2 * TILE - 6 - len(text)) + s + " é中 it's" * 400
    data = text.encode()[:4 * TILE]
    buf, off = np.frombuffer(data, dtype=np.uint8).copy(), np.array([0, 3000, 4 * TILE], dtype=np.int64)
    pos, ln, ids = corpus.find_specials(buf, off, sp)
    assert TILE in (pos + ln) and any(p < 2 * TILE < p + l for p, l in zip(pos, ln))
    exp = oracle.OracleModel(tok.merges).encode_batch_specials(buf, off, sp, oracle.PAT_CL100K, n_threads=2)
    dev = torch.device("cuda", 0)
    d_buf, d_off = to_device(buf, off, 0)
    d_sp = tuple(torch.from_numpy(x).to(dev) for x in (pos, ln, ids))
    g_ids, g_off = tok.encode_device(d_buf, d_off, d_specials=d_sp, n_bytes=len(data))
    np.testing.assert_array_equal(g_off.cpu().numpy(), exp[1])
    np.testing.assert_array_equal(g_ids.cpu().numpy(), exp[0])
