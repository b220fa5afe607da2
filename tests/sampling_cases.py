"""What the sampling tests (tests/test_sampling.py, tests/test_gpu_sampling.py) share: the weight sets, a pure-Python
restatement of csrc/mlp/sample.h's draw, the exact probabilities an alias table implies and the error bound that the
header derives."""
import numpy as np

from cme213_sp18_amd.sampling import Balanced, Weighted

M64 = (1 << 64) - 1
U = 1 << 32
GOLDEN = 0x9e3779b97f4a7c15
SAMPLE_STREAM = 0x3c6ef372fe94f82b
AUGMENT_STREAM = 0xa5a5c3c35a5a3c3c


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def sample_key(seed, it):
    return mix64(((seed << 32) ^ it) ^ SAMPLE_STREAM)


def draw(d, n, key, table):
    """sample_draw of csrc/mlp/sample.h with Python integers."""
    h = mix64((key + (d + 1) * GOLDEN) & M64)
    j = ((h & 0xffffffff) * n) >> 32
    return j if (h >> 32) < int(table[j, 0]) else int(table[j, 1])


def zipf_labels(n, classes=62, seed=0):
    """Labels of min(classes, n) classes with Zipf-like counts (class c about 1 / (c + 1) of class 0), shuffled."""
    c = min(classes, n)
    share = 1.0 / np.arange(1, c + 1)
    counts = 1 + np.floor(share / share.sum() * (n - c)).astype(np.int64)  # one row each, the rest by share
    counts[0] += n - counts.sum()
    assert counts.min() >= 1 and counts.sum() == n
    labels = np.repeat(np.arange(c, dtype=np.int32), counts)
    np.random.default_rng(seed).shuffle(labels)
    return labels


SETS = ("uniform", "one_nonzero", "seventh_zero", "zipf62_balanced", "lognormal")


def policy_of(name, n, seed=0):
    """(policy, labels) of weight set ``name`` at size n, or None where the set does not exist (N == 1 with every 7th
    weight zero has no positive weight)."""
    rng = np.random.default_rng(100 + n)
    labels = zipf_labels(n)
    if name == "uniform":
        return Weighted(np.ones(n), seed), labels
    if name == "one_nonzero":
        w = np.zeros(n)
        w[n // 3] = 2.5
        return Weighted(w, seed), labels
    if name == "seventh_zero":
        w = rng.random(n) ** 8
        w[::7] = 0.0
        return (Weighted(w, seed), labels) if w.any() else None
    if name == "zipf62_balanced":
        return Balanced(seed), labels
    if name == "lognormal":
        return Weighted(np.exp(rng.normal(0.0, 2.0, n)), seed), labels
    raise KeyError(name)


def implied(table):
    """p[i] of every row as Python integers, in units of 2^-32 / N, and the number of columns that alias to each row."""
    n = table.shape[0]
    p, a = [0] * n, [0] * n
    for j in range(n):
        t, al = int(table[j, 0]), int(table[j, 1])
        if al == j:
            p[j] += U
        else:
            p[j] += t
            p[al] += U - t
            a[al] += 1
    return p, a


def exact_weights(w):
    """The weights as integers over one common power-of-two denominator: (W, sum(W))."""
    pairs = [float(v).as_integer_ratio() for v in w]
    k = max(d.bit_length() - 1 for _, d in pairs)
    W = [m << (k - (d.bit_length() - 1)) for m, d in pairs]
    return W, sum(W)


def bound(w, table, a):
    """csrc/mlp/sample.h's bound on |p[i] - 2^32 N w[i] / sum(w)| per row, in units.  The floating-point terms are
    formed in fp64 here and widened by 1e-6 of themselves, which covers this function's own rounding."""
    n = table.shape[0]
    u, e0 = 2.0 ** -53, 6 * 2.0 ** -53
    w = np.asarray(w, np.float64)
    q = w / float(np.sum(w, dtype=np.longdouble)) * n
    a = np.asarray(a, np.float64)
    E = 2.0 * a * u * (q * (1 + e0) + 1.0)
    D = n * e0 + float(E.sum())
    own = table[:, 1] == np.arange(n)
    clamped = ((table[:, 0] == 0xffffffff) & ~own).astype(np.int64)  # thresholds stored as 2^32 - 1
    c = clamped.copy()
    np.add.at(c, table[~own, 1].astype(np.int64), clamped[~own])
    return (a + 1 + c) / 2.0 + (1 + 1e-6) * U * (q * e0 + E + own * D)
