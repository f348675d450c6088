"""The pair-table builder (csrc/pairtable.cpp) on the CPU: tests/native/pairtable_check.cpp builds a
table and checks it through csrc/table.h's lookup -- the function the kernels call.  For every
table: the layout flags, every key resolves to its dict value, at least 100,000 non-keys ((b, a),
(a, b +- 1), members over 0xFFFF on the narrow layouts, random pairs) return "no pair", and the
inverse table maps each value back to its pair.

The quotient layout's precondition (table.h): no key's tag may be 0xFFFF, the tag of an empty
entry.  With the default start value the first draw gives the byte pairs (32, 151) and (246, 181)
that tag, so their tables must take a later draw; the golden models have no such key and keep
their images bit for bit (hashes below: taken from the builder before it rejected such draws)."""
import hashlib
import json
import os
import random
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import load_model_merges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shredword_amd", "csrc")

# model -> (sha256 of the bucket image, shift, m1, m2) of the builder without the tag rule
GOLDEN_IMAGES = {
    "toy500.model": ("bb6518aba069cbc984343c9f27e852307cfceaffda127b2032f617b9ebb3a160", 16, 3756625553, 3934247373),
    "bl32k.model": ("a88ccf6d9d235fa9226cd9de114acdd33098a35f584b9ccb291484db0d4bf245", 15, 1679556353, 3098683583),
    "bl50k.model": ("68f55a0a5b21c9a653ca7e9cce87f657726e9cf1e10f683b3446bb5c5dfd046a", 14, 1234883967, 1496932117),
}


@pytest.fixture(scope="module")
def checker():
    d = tempfile.mkdtemp(prefix="pairtable_check_")
    exe = os.path.join(d, "pairtable_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "native", "pairtable_check.cpp"), os.path.join(CSRC, "pairtable.cpp")],
                   check=True)

    def run(pairs, vals, sweep=1, image=False):
        """pairs / vals in the order given (duplicates allowed) -> the checker's report."""
        path = os.path.join(d, "table.bin")
        with open(path, "wb") as f:
            f.write(np.int64(len(vals)).tobytes())
            f.write(np.asarray(pairs, dtype=np.int32).tobytes())
            f.write(np.asarray(vals, dtype=np.int32).tobytes())
        cmd = [exe, path, "--sweep", str(sweep)]
        if image:
            cmd += ["--image", os.path.join(d, "image.bin")]
        rep = json.loads(subprocess.run(cmd, check=True, capture_output=True, text=True).stdout)
        if image:
            rep["sha256"] = hashlib.sha256(open(os.path.join(d, "image.bin"), "rb").read()).hexdigest()
        return rep

    return run


def run_merges(checker, merges, **kw):
    return checker([p for p in merges], list(merges.values()), **kw)


def wellformed(n, seed):
    """n pairs as a trainer emits them: each value new, >= 256 and larger than its pair's members."""
    r = random.Random(seed)
    ids, merges = list(range(256)), {}
    while len(merges) < n:
        p = (r.choice(ids), r.choice(ids))
        if p not in merges:
            merges[p] = 256 + len(merges)
            ids.append(merges[p])
    return merges


def assert_exact(rep, n, wide, ids16, q16, split_ok):
    assert rep["status"] == 0, rep["error"]
    assert (rep["wide"], rep["ids16"], rep["q16"], rep["split_ok"]) == (wide, ids16, q16, split_ok), rep
    assert rep["merges"] == rep["keys"] == n
    assert rep["bad_keys"] == 0 and rep["bad_nonkeys"] == 0 and rep["bad_inv"] == 0, rep
    assert rep["nonkeys"] >= 100000


TAG_FFFF = [{(32, 151): 256}, {(32, 151): 256, (246, 181): 257}]


@pytest.mark.parametrize("merges", TAG_FFFF, ids=["one", "two"])
def test_keys_with_the_empty_entrys_tag(checker, merges):
    """(32, 151) and (246, 181) have tag 0xFFFF under the first draw of the default start value: the
    builder must not accept that draw, and the keys resolve."""
    rep = run_merges(checker, merges)
    assert_exact(rep, len(merges), 0, 1, 1, 1)
    assert rep["draws"] > 1, rep


@pytest.mark.parametrize("model", sorted(GOLDEN_IMAGES))
def test_golden_models_exact_and_images_unchanged(checker, model):
    merges = load_model_merges(model)
    rep = run_merges(checker, merges, image=True)
    assert_exact(rep, len(merges), 0, 1, 1, 1)
    assert (rep["sha256"], rep["shift"], rep["m1"], rep["m2"]) == GOLDEN_IMAGES[model]


@pytest.mark.parametrize("n,sweep", [(300, 64), (16384, 1), (16385, 64), (50000, 1)])
def test_random_wellformed_tables(checker, n, sweep):
    """Both sides of the 2^16 -> 2^17 bucket step (16,384 pairs fill a quarter of 2^16 x 4 entries);
    the 300- and 16,385-pair tables again under 63 further start values."""
    rep = run_merges(checker, wellformed(n, n), sweep=sweep)
    assert_exact(rep, n, 0, 1, 1, 1)
    assert rep["buckets"] == (1 << 16 if n <= 16384 else 1 << 17 if n <= 32768 else 1 << 18)
    assert rep["sweep_builds"] == sweep - 1 and rep["sweep_failed"] == 0 and rep["sweep_flag_changes"] == 0
    assert rep["sweep_keys"] == n * (sweep - 1) and rep["sweep_nonkeys"] >= 100000 * (sweep - 1)
    assert rep["sweep_bad_keys"] == 0 and rep["sweep_bad_nonkeys"] == 0 and rep["sweep_bad_inv"] == 0, rep


def test_illformed_table(checker):
    """Duplicate values, values < 256 and below their members, a duplicated pair (its last value
    wins): exact lookups, no split path."""
    r = random.Random(7)
    ids = list(b"abcd ") + list(range(256, 296))
    pairs = [(r.choice(ids), r.choice(ids)) for _ in range(300)]
    vals = [r.randint(0, 300) for _ in pairs]
    pairs.append(pairs[0])
    vals.append(vals[0] + 1)
    rep = checker(pairs, vals)
    assert_exact(rep, len(set(pairs)), 0, 1, 1, 0)


def test_value_fffe_takes_the_narrow_cuckoo_table(checker):
    rep = run_merges(checker, {(97, 98): 256, (256, 99): 0xFFFE})
    assert_exact(rep, 2, 0, 0, 0, 1)


def test_id_70000_takes_the_wide_table(checker):
    rep = run_merges(checker, {(97, 98): 256, (256, 99): 70000, (70000, 97): 70001})
    assert_exact(rep, 3, 1, 0, 0, 1)


def test_negative_ids_are_refused_with_the_encoders_messages(checker):
    assert checker([(1, -2)], [256])["error"] == "sw_encoder_create: negative token id in a pair"
    assert checker([(1, 2)], [-256])["error"] == "sw_encoder_create: negative merge value"
