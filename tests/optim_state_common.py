"""Host model of the bf16 optimizer state (include/egopack_optim.h): how one f32 moment is rounded to the
bf16 value a launch stores, and which 16 random bits every element of every buffer draws.

Independent of the package (nothing is imported from ``egopack_amd``): numpy integer arithmetic over tests/philox_ref.py, so every
comparison with a kernel's state is bit for bit -- there is no tolerance.

  rounding   x with f32 bits b.  Exponent all ones (inf / NaN), or state_round == 0: round to nearest even, the bits of the
             library's f2bf (= torch's ``.to(torch.bfloat16)``).  state_round == 1: (b + r) >> 16 with 16 random bits r -- the
             magnitude grows with probability (b & 0xFFFF) / 65536 for either sign, a representable value is returned unchanged,
             the expectation is x, a carry out of the largest finite value gives inf.
  bits       element e = elem0 + i of a launch at counted step t:
                 w = philox4x32_10(ctr = ((t & 0xFFFFFF) << 40) | (e >> 2), key = state_seed)[e & 3]
                 r(state0) = w >> 16, r(state1) = w & 0xFFFF
"""
import numpy as np

from tests import philox_ref as P

KEY_SALT = int.from_bytes(b"OPT_STAT", "big")  # egopack_amd.ops.OPTIM_STATE_KEY_SALT (the CPU test compares the two)


def key(seed):
    """The Philox key of a run with ``seed``: never the seed itself (the dropout key), never the LTA sampler's key."""
    return (int(seed) ^ KEY_SALT) & P.MASK64


def f32_bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def nearest_bits(b):
    """uint32 f32 bits -> uint16 bf16 bits, round to nearest even; a NaN stays a NaN (quiet bit set), inf stays inf."""
    b = np.asarray(b, dtype=np.uint32).astype(np.uint64)
    nan = ((b & np.uint64(0x7F800000)) == np.uint64(0x7F800000)) & ((b & np.uint64(0x007FFFFF)) != 0)
    rne = (b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    out = np.where(nan, (b >> np.uint64(16)) | np.uint64(0x0040), rne)
    return (out & np.uint64(0xFFFF)).astype(np.uint16)


def stochastic_bits(b, r):
    """uint32 f32 bits, 16 random bits each -> uint16 bf16 bits: (b + r) >> 16; inf / NaN as ``nearest_bits``."""
    b = np.asarray(b, dtype=np.uint32).astype(np.uint64)
    r = np.asarray(r).astype(np.uint64) & np.uint64(0xFFFF)
    special = (b & np.uint64(0x7F800000)) == np.uint64(0x7F800000)
    out = ((b + r) >> np.uint64(16)) & np.uint64(0xFFFF)
    return np.where(special, nearest_bits(b.astype(np.uint32)).astype(np.uint64), out).astype(np.uint16)


def random_bits(seed_key, t, elem0, n):
    """(r of state0, r of state1), uint32 arrays [n] holding 16 bits each: what elements elem0 .. elem0 + n - 1 draw at step t."""
    e = np.uint64(int(elem0)) + np.arange(n, dtype=np.uint64)
    ctr = np.uint64((int(t) & 0xFFFFFF) << 40) | (e >> np.uint64(2))
    words = P.philox_u64(ctr, seed_key)  # [n, 4]
    w = words[np.arange(n), (e & np.uint64(3)).astype(np.int64)]
    return w >> np.uint32(16), w & np.uint32(0xFFFF)


def round_state(x, mode, seed_key=0, t=0, elem0=0, buffer=0):
    """f32 array [n] -> uint16 bf16 bits [n] as a launch stores them.  mode 0: nearest; 1: stochastic with the bits of ``buffer``."""
    b = f32_bits(x).reshape(-1)
    if mode == 0:
        return nearest_bits(b)
    return stochastic_bits(b, random_bits(seed_key, t, elem0, b.size)[buffer])


def widen(bits16):
    """uint16 bf16 bits -> the f32 values they stand for (exact)."""
    return (np.asarray(bits16, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)
