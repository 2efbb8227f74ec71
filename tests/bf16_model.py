"""A numpy model of the two row conversions of csrc/sot_bf16.hip and the values that can break them (tests/test_bf16_host.py holds the
model to torch on the CPU; tests/test_bf16_gpu.py feeds the same values to the kernels).

bfloat16 is the upper half of a float32: widening appends 16 zero bits (exact), narrowing rounds the lower half away to nearest, ties to
even -- in integer arithmetic `bits + 0x7FFF + (bit 16 of bits)`, whose carry turns the largest finite values into infinity, as IEEE
rounding does.  A NaN must be caught first: its payload may live in the lower half only (0x7F800001 would round to infinity) or carry
into the sign (0x7FFFFFFF + 0x8000).  It becomes the quiet NaN 0x7FC0, which is what torch writes."""
import numpy as np


def widen(bits):
    """uint16 bfloat16 bit patterns -> float32"""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def narrow(values):
    """float32 -> uint16 bfloat16 bit patterns, round to nearest even"""
    u = np.ascontiguousarray(values, np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return np.where(nan, 0x7FC0, r).astype(np.uint16)


def is_nan_bits(bits):
    b = np.asarray(bits, np.uint16)
    return (b & 0x7FFF) > 0x7F80


def adversarial_bits():
    """float32 bit patterns (uint32) around every decision of the narrowing: both signs of each"""
    pos = [
        0x00000000,                                       # zero
        0x3F800000, 0x3F810000,                           # exactly representable, even / odd last kept bit
        0x3F808000, 0x3F818000,                           # ties: to even (down), to even (up)
        0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,   # one ulp on either side of a tie
        0x3F80FFFF, 0x3FFFFFFF, 0x3FFF8000,               # carries into the exponent
        0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF,               # the largest finite float32 -> inf; its tie -> inf; just below -> largest finite bfloat16
        0x00000001, 0x00007FFF, 0x00008000, 0x00008001,   # subnormals: below half a bfloat16 ulp, the tie at the bottom (to zero), just above
        0x00018000, 0x007F8000, 0x007FFFFF,               # subnormal ties upward; the largest subnormal becomes the smallest normal
        0x00800000, 0x00808000,                           # the smallest normal and a tie next to it
        0x7F800000,                                       # infinity is kept
        0x7FC00000, 0x7F800001, 0x7F80FFFF, 0x7FFFFFFF, 0x7FA00000,   # NaNs: quiet, payload in the lower half only, all ones, signalling
    ]
    return np.array(pos + [b | 0x80000000 for b in pos], np.uint32)


def adversarial_values():
    return adversarial_bits().view(np.float32)


def random_values(count, seed):
    """float32 values of every magnitude (random bit patterns, NaN and infinity patterns included) mixed with ordinary ones"""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 1 << 32, size=count, dtype=np.uint64).astype(np.uint32).view(np.float32)
    plain = (rng.standard_normal(count) * np.exp(rng.uniform(-20, 20, count))).astype(np.float32)
    return np.where(rng.random(count) < 0.5, raw, plain).astype(np.float32)
