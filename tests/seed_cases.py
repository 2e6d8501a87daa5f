"""The noise contract of the seeded-noise path (include/vsd.h) in a few lines of numpy -- written from the contract's sentences, not by
calling the library: Philox4x32-10 in uint64 arithmetic, the uniform map, Box-Muller in fp64.  tests/test_seed_host.py holds it to the
Random123 known answers; tests/test_seed_gpu.py holds the kernels to it (the integers bit for bit, the normals to the fp32 bound)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
Z_MAX = float(np.sqrt(48.0 * np.log(2.0)))  # |z| <= sqrt(-2 ln(2^-24)) = 5.77: the smallest u is 0.5 * 2^-23

# (counter, key, output) of Philox4x32-10 as published with Random123 (kat_vectors)
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((MASK, MASK, MASK, MASK), (MASK, MASK), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]

SEEDS = [0, 42, 2 ** 32 + 5, 2 ** 64 - 1]


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """counters: uint64 arrays (or ints) holding 32-bit values; key: two ints -> four uint64 arrays of 32-bit values"""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & MASK, int(k1) & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]  # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK)]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def key_of(seed: int):
    seed = int(seed) % (1 << 64)
    return seed & MASK, seed >> 32


def raw_draw(seed: int, kind: int, draw: int, hw: int) -> np.ndarray:
    """the integers X of one draw: uint32 [hw][4]"""
    k0, k1 = key_of(seed)
    x = philox4x32_10(np.arange(hw, dtype=np.uint64), draw, kind, 0, k0, k1)
    return np.stack(x, axis=1).astype(np.uint32)


def uniform(x) -> np.ndarray:
    """u(x) = ((x >> 9) + 0.5) * 2^-23 (fp64 here; every value is an fp32 number)"""
    return ((np.asarray(x, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def normal_draw(seed: int, kind: int, draw: int, hw: int) -> np.ndarray:
    """one draw as fp64 [4][hw] (the layout of Engine.noise): Box-Muller of (X0, X1) -> channels 0, 1 and of (X2, X3) -> channels 2, 3"""
    x = raw_draw(seed, kind, draw, hw)
    out = np.empty((4, hw), dtype=np.float64)
    for h in range(2):
        r = np.sqrt(-2.0 * np.log(uniform(x[:, 2 * h])))
        t = 2.0 * np.pi * uniform(x[:, 2 * h + 1])
        out[2 * h] = r * np.cos(t)
        out[2 * h + 1] = r * np.sin(t)
    return out
