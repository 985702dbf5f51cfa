"""Inputs and checks shared by test_emu_bgzf.py (the kernel source under the CPU emulator) and test_gpu_bgzf.py (the library on the device).
The judge of a compressor's output is Python's gzip / zlib: gzip.decompress checks every member's CRC-32 and ISIZE."""
import gzip
import zlib

import numpy as np

import bam_reader

BLOCK = 0xff00
LENGTHS = (1, 2, 3, 4, 63, 64, 65, 257, 258, 259, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 3)
CONTENTS = ("byte", "counter", "random")
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)


def _rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def content(kind, n):
    if kind == "byte":
        return b"\x5a" * n
    if kind == "counter":
        return (np.arange(n, dtype=np.int64) % 251).astype(np.uint8).tobytes()
    return _rand(n, 1000 + n)


def check(raw, data):
    """raw: concatenated BGZF members of data cut every BLOCK bytes; returns [(member size, ISIZE)]"""
    blocks = bam_reader.bgzf_blocks(raw)
    assert len(blocks) == (len(data) + BLOCK - 1) // BLOCK
    assert all(b <= 0x10000 and i <= BLOCK for b, i in blocks), blocks
    assert [i for _, i in blocks] == [min(BLOCK, len(data) - o) for o in range(0, len(data), BLOCK)]
    assert gzip.decompress(raw) == data
    return blocks


def distance_boundary(period):
    """a whole block: a random pattern of `period` bytes and the start of its repetition"""
    p = _rand(period, 77 + period)
    return (p + p)[:BLOCK]


def every_code():
    """one block holding, for every match length 3 .. 258 and for one distance of each of the 30 distance codes, a repeat of that length at that distance,
    fresh random bytes between the repeats"""
    rng = np.random.default_rng(4242)
    buf = bytearray(rng.integers(0, 256, DIST_BASE[-1] + 8, dtype=np.uint8).tobytes())
    for k, length in enumerate(range(3, 259)):
        dist = DIST_BASE[(k * 7) % 30]   # 7 and 30 are coprime: every code, and lengths of all sizes at every one
        buf += rng.integers(0, 256, 4, dtype=np.uint8).tobytes()
        for _ in range(length):   # byte by byte: the repeat may overlap its source
            buf.append(buf[-dist])
    assert len(buf) <= BLOCK
    return bytes(buf)


def entropy_bound(data):
    """n (H + 1) / 8 + 400 bytes, H the order-0 entropy in bits: what a Huffman code over the bytes, a header without run-length codes and the framing stay under"""
    cnt = np.bincount(np.frombuffer(data, dtype=np.uint8), minlength=256)
    p = cnt[cnt > 0] / len(data)
    h = float(-(p * np.log2(p)).sum())
    return len(data) * (h + 1) / 8 + 400


def huffman_only_size(data):
    """zlib's size for the block with matching switched off (raw deflate) plus the 26 bytes of BGZF framing"""
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_HUFFMAN_ONLY)
    return len(c.compress(data) + c.flush()) + 26


def fib_counts():
    f = [0, 1, 1]
    while len(f) <= 22:
        f.append(f[-1] + f[-2])
    return f


def fib_block(shuffled):
    """byte value k occurs fib(k) times, k = 1 .. 22 (46,367 bytes): an unlimited Huffman code would be 21 levels deep"""
    f = fib_counts()
    a = np.concatenate([np.full(f[k], k, dtype=np.uint8) for k in range(1, 23)])
    assert a.size == 46367
    if shuffled:
        np.random.default_rng(99).shuffle(a)
    return a.tobytes()


def skewed_block():
    """BLOCK bytes iid from a fixed skewed distribution over 16 symbols"""
    w = np.array([2.0 ** -(k + 1) for k in range(15)] + [2.0 ** -15])
    return np.random.default_rng(31337).choice(np.arange(16, dtype=np.uint8) + 65, size=BLOCK, p=w / w.sum()).astype(np.uint8).tobytes()


def degenerate():
    two_long = np.random.default_rng(5).integers(0, 2, 3000, dtype=np.uint8) + 65
    return {
        "two_values_no_match": b"ABBAB",                    # no three bytes occur twice: literals only
        "two_values": two_long.tobytes(),
        "one_distance": (b"abcdefg" * 100)[:64 + 2 * 258],  # matches begin at 64 and 322, each at distance 7
        "one_value": b"\x00" * 700,
    }


def many_blocks(n_blocks, seed=8):
    """mixed content: per block a run, text-like bytes, a periodic stretch or noise"""
    rng = np.random.default_rng(seed)
    parts = []
    for k in range(n_blocks):
        kind = k % 4
        if kind == 0:
            parts.append(bytes([k & 0xff]) * BLOCK)
        elif kind == 1:
            parts.append((rng.integers(0, 64, BLOCK, dtype=np.uint8) + 48).tobytes())
        elif kind == 2:
            parts.append((rng.integers(0, 256, 97 + k % 31, dtype=np.uint8).tobytes() * (BLOCK // 97 + 1))[:BLOCK])
        else:
            parts.append(rng.integers(0, 256, BLOCK, dtype=np.uint8).tobytes())
    return b"".join(parts)[:n_blocks * BLOCK - 17]   # (the last block is short)


# ---- cases 1 - 7: each takes a compressor (anything with .compress(bytes) -> bytes) and asserts what holds for it
def case_lengths(z, kind):
    for n in LENGTHS:
        data = content(kind, n)
        blocks = check(z.compress(data), data)
        if kind == "random":   # nothing to find: stored, 5 bytes of block header and 26 of framing
            assert all(b <= i + 31 for b, i in blocks), (n, blocks)


def case_distance_boundary(z):
    d = distance_boundary(32768)   # the second half: matches at distance 32,768 exactly
    assert check(z.compress(d), d)[0][0] < 0.6 * len(d)
    d = distance_boundary(32769)   # the only repeat lies one byte beyond the window
    check(z.compress(d), d)


def case_every_code(z):
    d = every_code()
    check(z.compress(d), d)


def case_length_limit(z):
    d = fib_block(True)
    assert huffman_only_size(d) <= entropy_bound(d)   # the bound is attainable: zlib without matching meets it
    size = check(z.compress(d), d)[0][0]
    assert size <= entropy_bound(d), (size, entropy_bound(d))
    d = fib_block(False)   # in runs: matches thin the literals and change the code
    check(z.compress(d), d)


def case_degenerate(z):
    for name, d in degenerate().items():
        check(z.compress(d), d)


def case_literal_coding(z):
    d = skewed_block()
    assert huffman_only_size(d) <= entropy_bound(d)
    size = check(z.compress(d), d)[0][0]
    assert size <= entropy_bound(d), (size, entropy_bound(d))   # an encoder that codes every chance 3-byte match exceeds it


def case_matches(z):
    d = bytes(BLOCK)
    assert check(z.compress(d), d)[0][0] < 2048   # 254 matches; Huffman alone needs 8 KiB


CASES = {"lengths_byte": lambda z: case_lengths(z, "byte"), "lengths_counter": lambda z: case_lengths(z, "counter"), "lengths_random": lambda z: case_lengths(z, "random"),
         "distance_boundary": case_distance_boundary, "every_code": case_every_code, "length_limit": case_length_limit, "degenerate": case_degenerate,
         "literal_coding": case_literal_coding, "matches": case_matches}


def case_chunking(lib, device=0):
    """case 8: the same 40 blocks through compressors of 1, 7 and the default number of blocks per launch, and twice through one"""
    data = many_blocks(40)
    outs = []
    for mb in (1, 7, 0):
        z = lib.bgzf(device=device, max_blocks=mb)
        outs.append(z.compress(data))
        if mb == 7:
            outs.append(z.compress(data))
        z.close()
    check(outs[0], data)
    assert all(o == outs[0] for o in outs[1:])
