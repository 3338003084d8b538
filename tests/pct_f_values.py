"""The float32 values the "%f" round trip and the .pss formatter are held to,
once per binade: for every exponent field 0..254 (denormals to the largest
finite binade) and both signs the smallest mantissa, the largest mantissa and
six seeded random ones; and every odd multiple of 1/128 up to 2, the exact
ties of the sixth decimal (k / 128 = k * 7812.5e-6), of both parities and
both signs.  Python's '%f' is the exact round-half-even expansion these are
compared with."""
import numpy as np


def binade_sweep(seed=20240):
    rng = np.random.default_rng(seed)
    bits = []
    for ex in range(255):
        mant = [0, 0x7FFFFF] + [int(x) for x in rng.integers(1, 0x7FFFFF, 6)]
        for sign in (0, 1):
            bits += [(sign << 31) | (ex << 23) | m for m in mant]
    vals = np.array(bits, dtype=np.uint32).view(np.float32)
    ties = np.array([k / 128.0 for k in range(1, 256, 2)], dtype=np.float32)
    assert '%f' % (1 / 128) == '0.007812' and '%f' % (3 / 128) == '0.023438'
    return np.concatenate([vals, ties, -ties])


def expected_cost(x):
    """float(-1 * atof(printf("%f", x))) bit for bit."""
    return np.float32(-float('%f' % float(x)))
