"""numpy restatement of the 2-bit-packed read layout of include/kmap_hip.h, for the tests that hand packed arrays to the raw entry
points (tests/test_gpu_alignment.py, tests/test_gpu_footprint.py).  tests/test_footprint_host.py holds it to known words."""
import numpy as np


def packed_groups(n):
    """the data groups, two all-invalid halo groups, an even total"""
    return (((n + 15) // 16 + 2) + 1) & ~1


def ref_pack(seq, rng=None):
    """The header's contract: codes[g] holds base i of group g in bits [31 - 2 i, 30 - 2 i] (first base most significant), bit
    15 - i of inval[g] marks position 16 g + i as not A/C/G/T or at / past n.  -> codes, inval, valid (code bits that count).
    The code bits of an invalid position are not part of the contract: `rng` fills them with noise (for inputs), else 0."""
    n = len(seq)
    ng = packed_groups(n)
    s = np.full(ng * 16, 255, np.uint8)
    s[:n] = seq
    bad = (s > 3).reshape(ng, 16)
    two = np.where(s > 3, 0 if rng is None else rng.integers(0, 4, size=ng * 16), s).astype(np.uint32).reshape(ng, 16)
    sh = (30 - 2 * np.arange(16)).astype(np.uint32)
    codes = np.bitwise_or.reduce(two << sh, axis=1).astype(np.uint32)
    valid = np.bitwise_or.reduce(np.where(bad, 0, 3).astype(np.uint32) << sh, axis=1).astype(np.uint32)
    inval = np.bitwise_or.reduce(bad.astype(np.uint32) << (15 - np.arange(16)).astype(np.uint32), axis=1).astype(np.uint16)
    return codes, inval, valid


def ref_planes(codes):
    """planes[2w] / planes[2w + 1] = the high / the low bits of the 32 base codes of groups 2w, 2w + 1, first position most
    significant"""
    c = codes.reshape(-1, 2).astype(np.uint64)
    word = (c[:, 0] << np.uint64(32)) | c[:, 1]                        # 32 codes, first one in bits 63:62
    hi = np.zeros(len(word), np.uint64)
    lo = np.zeros(len(word), np.uint64)
    for j in range(32):
        code = (word >> np.uint64(62 - 2 * j)) & np.uint64(3)
        hi |= (code >> np.uint64(1)) << np.uint64(31 - j)
        lo |= (code & np.uint64(1)) << np.uint64(31 - j)
    return np.stack([hi, lo], axis=1).astype(np.uint32).reshape(-1)
