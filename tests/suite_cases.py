"""Inputs, fp64 references and derived error bounds for the homework-suite kernels (csrc/suite/*.hip).  No GPU here:
tests/test_suite_cases.py proves on the CPU that the bounds hold for a plain fp32 evaluation and are exceeded by
subtly wrong ones; tests/test_gpu_suite_edges.py holds the HIP kernels to them.

u = 2^-24 is the unit roundoff of fp32 (round to nearest), gamma_n = n u / (1 - n u) <= (n + 1) u for the n below.

Stencil
-------
One output is ``fma(ycfl, sy, fma(xcfl, sx, c))`` with ``sx = sum_k c_k u(x + k)`` and ``sy`` alike, each a chain of
2B + 1 fused multiply-adds from 0 (csrc/suite/stencil.hip: apply_stencil).  A product ``c_k u`` of sx passes through at
most 2B + 1 roundings inside the chain and 2 more in the two outer FMAs: 2B + 3; a product of sy through 2B + 2; the
centre through 2.  An evaluation without FMAs (the native host oracle: products and sums rounded apart, csrc/cpu/
suite_cpu.cpp) rounds a product of sx at most 1 + 2B + 1 + 2 = 2B + 4 times.  So for either form, computed from an
fp32 grid v,

    |computed(v) - S(v)| <= gamma_{2B+4} * A(|v|),      A = the step with |c_k|, |xcfl|, |ycfl|, |scale|,

and with v = u64 + e, |e| <= E:  |computed - S(u64)| <= A(E) + gamma_{2B+4} A(|u64| + E).  The running bound carried
here is the issue's ``E' = A(E) + g A(|u64|)`` with g = (2B + 6) u: gamma_{2B+4} < (2B + 5) u, and the remaining u A(|u64|)
absorbs the second-order term g A(E) (E is about 1e-6 |u64|).  A border cell is one product ``v * scale``: one rounding,
far inside ``|scale| E + g |scale| |u64|``.  The fp64 evaluation's own error (2^-53) is nothing next to u.  The noise
inputs hold no value near the fp32 subnormals, so underflow adds nothing.

PageRank
--------
``out[i] = 0.5f / n + 0.5f * sum_j in[e_j] * inv[e_j]``: every term is non-negative.  Each product is rounded once;
summing deg terms in ANY order or tree (one lane, 2/4/8 lanes and a shuffle reduction, an unrolled loop adding exact
zeros) rounds each term at most deg - 1 times; the multiplication by 0.5 is exact; the last addition rounds once; the
base 0.5f / (float)n is a rounded quotient (n < 2^24 is exact as a float) that the last addition rounds again.  At most
deg + 1 roundings on anything: gamma_{deg+1} <= (deg + 4) u for every deg <= 7000 (the longest row here has 5000
edges).  With the inputs within E of the reference,

    E'[i] = 0.5 sum_j E[e_j] inv[e_j] + (deg_i + 4) u ref'[i].

The pre-multiplied form gathers w[e] = fl(out[e] * inv[e]) formed by the previous propagation: the SAME single rounding
of the same product, moved -- so its ``out`` obeys the same bound.  The additional rounding the issue asks to include
shows where the form stores it: |w[i] - ref[i] inv[i]| <= inv[i] (E[i] + u (ref[i] + E[i])) (``pagerank_w_bound``).
"""
from __future__ import annotations

import functools

import numpy as np

U = 2.0 ** -24
F32 = np.float32

# ------------------------------------------------------------------------------------------------------- stencil
COEF = {2: (1.0, -2.0, 1.0),
        4: (-1.0, 16.0, -30.0, 16.0, -1.0),
        8: (-9.0, 128.0, -1008.0, 8064.0, -14350.0, 8064.0, -1008.0, 128.0, -9.0)}
# (xcfl, ycfl): deliberately unequal (a swap must show), near the stability limit 0.5 / sum|c| of each order, and NOT
# SimParams' (which are equal on a square domain)
STENCIL_CFL = {2: (0.031, 0.017), 4: (0.0077, 0.0043), 8: (3.0e-5, 1.7e-5)}
STENCIL_SCALE = 0.9873
STENCIL_STEPS = 3
# (nx, ny) of the noise tests: one cell; thinner than a float4; one row block of very wide rows; the suite's odd
# shape; three 248-column strips of the two-step walk with a partial last block
NOISE_SHAPES = [(1, 1), (3, 2), (5, 1023), (257, 131), (500, 390)]
# bitwise tests of the LDS walk's instantiations: two row blocks at 128 rows per wave (512 per workgroup), a partial
# last block, a partial last strip (256- and 248-column strips alike)
BITWISE_SHAPE = (500, 800)
# every (rows, ahead, nt) of stencil_lds_tune's switch (nt bit 0: non-temporal loads, bit 1: alternating walk,
# bit 2: plain stores)
LDS_TUNE_CASES = [(32, 4, 6), (32, 6, 6), (64, 4, 6), (32, 6, 2), (16, 4, 2), (32, 4, 2), (32, 8, 2), (64, 8, 2),
                  (16, 8, 2), (32, 4, 0), (32, 4, 1), (32, 8, 0), (32, 8, 1), (64, 4, 0), (64, 8, 0), (64, 8, 1),
                  (128, 8, 0), (128, 8, 1)]
# every (rows, ahead) of stencil_step2_bc's switch, and (0, 0): the automatic pick
LDS2_CASES = [(64, 4), (64, 2), (32, 4), (96, 4), (128, 4), (128, 2), (32, 2), (64, 3), (64, 1), (96, 2), (0, 0)]
# (nx, ny) just past the 1024 x 256 boundary-cell cap of the fused launches: 2 (gx + gy - 2B) B > 262,144
BC_CAP_WIDE = {2: (131_100, 1), 4: (65_600, 1), 8: (32_800, 1)}
# past stencil_bc's own 4096 x 256 cap: 2 (gx + gy - 2B) B > 1,048,576 at order 8
BC_CAP_TALL_BC = (1, 131_100)


def stencil_params(order: int) -> tuple[float, float, float]:
    """(xcfl, ycfl, scale) as the fp32 values the kernel receives, widened to Python floats."""
    x, y = STENCIL_CFL[order]
    return float(F32(x)), float(F32(y)), float(F32(STENCIL_SCALE))


def stencil_gamma(order: int) -> float:
    return (order + 6) * U  # (2B + 6) u


def noise_grid(nx: int, ny: int, order: int, seed: int | None = None) -> np.ndarray:
    """Uniform noise in [-1, 1] on the whole [gy][gx] grid, border included: neighbours are unrelated, so a tap read
    one cell off changes the result by the size of the tap itself."""
    b = order // 2
    seed = nx * 1_000_003 + ny * 101 + order if seed is None else seed
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (ny + 2 * b, nx + 2 * b)).astype(F32)


def stencil_step64(u: np.ndarray, order: int, xcfl: float, ycfl: float, scale: float, *, coef=None, halo=None,
                   scale_interior: bool = False) -> np.ndarray:
    """One step in fp64: the stencil on the interior, ``u * scale`` on the border.  The keyword arguments build WRONG
    steps for tests/test_suite_cases.py: ``coef`` another coefficient table; ``halo=("row", r)`` the y-taps read grid
    row r one cell to the right, ``("col", c)`` the x-taps read grid column c one cell down; ``scale_interior`` the
    boundary factor applied to the interior too."""
    b = order // 2
    co = COEF[order] if coef is None else coef
    gy, gx = u.shape
    ux = uy = u
    if halo is not None:
        kind, idx = halo
        if kind == "row":
            uy = u.copy()
            uy[idx] = np.roll(u[idx], -1)
        else:
            ux = u.copy()
            ux[:, idx] = np.roll(u[:, idx], -1)
    out = u * scale
    sx = np.zeros((gy - 2 * b, gx - 2 * b))
    sy = np.zeros_like(sx)
    for k in range(-b, b + 1):
        sx += co[k + b] * ux[b:gy - b, b + k:gx - b + k]
        sy += co[k + b] * uy[b + k:gy - b + k, b:gx - b]
    inner = u[b:gy - b, b:gx - b] + xcfl * sx + ycfl * sy
    out[b:gy - b, b:gx - b] = inner * scale if scale_interior else inner
    return out


def stencil_reference(g0: np.ndarray, order: int, steps: int = STENCIL_STEPS, params=None, **wrong):
    """(u64, E) after ``steps`` steps from the fp32 grid ``g0``: the fp64 restatement and the running per-element
    bound of the module docstring.  ``wrong`` (see stencil_step64, and ``swap=True``: xcfl and ycfl exchanged) gives
    a perturbed u64 instead; its E is meaningless."""
    xcfl, ycfl, scale = params or stencil_params(order)
    if wrong.pop("swap", False):
        xcfl, ycfl = ycfl, xcfl
    g = stencil_gamma(order)
    absco = tuple(abs(c) for c in COEF[order])
    u = np.asarray(g0, F32).astype(np.float64)
    E = np.zeros_like(u)
    for _ in range(steps):
        E = (stencil_step64(E, order, abs(xcfl), abs(ycfl), abs(scale), coef=absco)
             + g * stencil_step64(np.abs(u), order, abs(xcfl), abs(ycfl), abs(scale), coef=absco))
        u = stencil_step64(u, order, xcfl, ycfl, scale, **wrong)
    return u, E


@functools.lru_cache(maxsize=None)
def noise_case(nx: int, ny: int, order: int, steps: int = STENCIL_STEPS):
    """(g0, u64, E) of a noise test, computed once and shared (read-only) by the tests that need it."""
    g0 = noise_grid(nx, ny, order)
    u, E = stencil_reference(g0, order, steps)
    for a in (g0, u, E):
        a.setflags(write=False)
    return g0, u, E


def worst_ratio(got: np.ndarray, ref: np.ndarray, bound: np.ndarray) -> float:
    """max |got - ref| / bound; an error where the bound is 0 counts as infinite, 0 / 0 as 0."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


def border_mask(gy: int, gx: int, b: int) -> np.ndarray:
    m = np.ones((gy, gx), bool)
    m[b:gy - b, b:gx - b] = False
    return m


# ------------------------------------------------------------------------------------------------------ PageRank
class CsrGraph:
    """indptr / edges (uint32), inv_deg / values (fp32) -- what hw2.Graph holds, without importing the package."""

    def __init__(self, indptr, edges, inv_deg, values):
        self.indptr = np.ascontiguousarray(indptr, np.uint32)
        self.edges = np.ascontiguousarray(edges, np.uint32)
        self.inv_deg = np.ascontiguousarray(inv_deg, F32)
        self.values = np.ascontiguousarray(values, F32)

    @property
    def n(self) -> int:
        return len(self.values)

    @property
    def deg(self) -> np.ndarray:
        return np.diff(self.indptr.astype(np.int64))


ADV_NODES = 3001          # not a multiple of 256
ADV_ROW65, ADV_ROW5000 = 100, 200
PAGERANK_ITERS = 3


def _finish_graph(deg: np.ndarray, rng) -> CsrGraph:
    n = len(deg)
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(deg, out=indptr[1:])
    edges = rng.integers(0, n, int(indptr[-1]), dtype=np.int64)
    inv = np.exp2(rng.uniform(-6.0, 1.0, n)).astype(F32)        # positive, arbitrary: nothing to do with 1 / deg
    vals = rng.uniform(0.0, 1.0, n).astype(F32)
    vals[vals == 0] = F32(0.5)                                   # (0, 1) open
    return CsrGraph(indptr, edges, inv, vals), indptr


@functools.lru_cache(maxsize=None)
def adversarial_graph() -> CsrGraph:
    """3001 nodes: rows of every length 0..40, one of 65 edges (8 x 8 + 1: one past a trip of the 8-lane kernel's
    unrolled loop) and one of 5000, empty first and last rows, self-loops, duplicate edges, inv_deg unrelated to the
    degrees, values uniform in (0, 1)."""
    rng = np.random.default_rng(20260213)
    n = ADV_NODES
    deg = (np.arange(n, dtype=np.int64) * 7) % 41                # every length 0..40, neighbours unlike
    deg[0] = deg[n - 1] = 0
    deg[ADV_ROW65], deg[ADV_ROW5000] = 65, 5000
    g, indptr = _finish_graph(deg, rng)
    edges = g.edges.astype(np.int64)
    rows = np.arange(n)
    loops = rows[(deg >= 1) & (rows % 5 == 0)]
    edges[indptr[loops]] = loops                                 # self-loops (first edge of every fifth row)
    dups = rows[(deg >= 2) & (rows % 3 == 0)]
    edges[indptr[dups] + 1] = edges[indptr[dups]]                # duplicate edges
    edges[indptr[ADV_ROW5000]:indptr[ADV_ROW5000] + 8] = ADV_ROW5000 - 1
    g = CsrGraph(indptr, edges, g.inv_deg, g.values)
    d = g.deg
    assert set(range(41)) <= set(d.tolist()) and d[0] == 0 and d[-1] == 0 and n % 256
    return g


LARGE_NODES = 4_194_304 + 257   # the smallest n past pagerank_w_kernel<1>'s 16384 x 256 lanes; past every other cap


@functools.lru_cache(maxsize=None)
def large_graph() -> CsrGraph:
    """4,194,561 nodes whose degrees cycle through 0..3 (6.3 M edges)."""
    rng = np.random.default_rng(4194561)
    deg = np.arange(LARGE_NODES, dtype=np.int64) % 4
    return _finish_graph(deg, rng)[0]


def pagerank_reference(g: CsrGraph, iters: int = PAGERANK_ITERS, history: bool = False):
    """(ref, E) in fp64 after ``iters`` propagations, with the bound of the module docstring; ``history=True``
    returns the list of (ref, E) after 0, 1, .. iters propagations instead."""
    n = g.n
    deg = g.deg
    row = np.repeat(np.arange(n), deg)
    e = g.edges.astype(np.int64)
    inv = g.inv_deg.astype(np.float64)
    ref = g.values.astype(np.float64)
    E = np.zeros(n)
    hist = [(ref, E)]
    for _ in range(iters):
        s = np.bincount(row, weights=ref[e] * inv[e], minlength=n)
        se = np.bincount(row, weights=E[e] * inv[e], minlength=n)
        ref = 0.5 / n + 0.5 * s
        E = 0.5 * se + (deg + 4) * U * ref
        hist.append((ref, E))
    return hist if history else hist[-1]


def pagerank_w_bound(g: CsrGraph, ref: np.ndarray, E: np.ndarray):
    """(w_ref, bound) of the pre-multiplied operand w = out * inv_deg stored beside ``out``: one more rounding."""
    inv = g.inv_deg.astype(np.float64)
    return ref * inv, inv * (E + U * (ref + E))


def premul_exact(values: np.ndarray, inv: np.ndarray) -> np.ndarray:
    """fl(values * inv) exactly: the fp64 product of two fp32 numbers is exact, so narrowing it rounds once."""
    return (values.astype(np.float64) * inv.astype(np.float64)).astype(F32)


# ------------------------------------------------------------------------------------------------- integer kernels
def sum_even_odd_exact(v: np.ndarray) -> tuple[int, int]:
    """(even sum, odd sum) in Python ints."""
    v = np.asarray(v, np.uint32)
    odd = (v & 1).astype(bool)
    # exact: uint64 holds 2^32 values of 2^32; folded to Python ints
    return int(v[~odd].astype(np.uint64).sum(dtype=np.uint64)), int(v[odd].astype(np.uint64).sum(dtype=np.uint64))


def sum_inputs(n: int, kind: str) -> np.ndarray:
    rng = np.random.default_rng(n * 7 + len(kind))
    v = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    if kind == "ones":
        v[:] = 0xFFFFFFFF
    elif kind == "even":
        v &= np.uint32(0xFFFFFFFE)
    elif kind == "odd":
        v |= np.uint32(1)
    else:
        assert kind == "full"
    return v


def stable_partition(keys: np.ndarray, start_bit: int) -> np.ndarray:
    """One stable 8-bit radix pass: keys ordered by digit, equal digits in input order."""
    keys = np.asarray(keys, np.uint32)
    return keys[np.argsort((keys >> np.uint32(start_bit)) & np.uint32(255), kind="stable")]


def shifted_matches_exact(t: np.ndarray, lo: int, hi: int) -> list[int]:
    """counts[s - lo] = #{i : i + s < n, t[i] == t[i + s]}; shifts >= n count 0."""
    n = len(t)
    return [int(np.count_nonzero(t[:n - s] == t[s:])) if s < n else 0 for s in range(lo, hi)]


def residue_hist_exact(t: np.ndarray, period: int) -> np.ndarray:
    return np.stack([np.bincount(t[r::period], minlength=256) for r in range(period)])


# the bytes next to the letter ranges, the ends of the ranges, and the upper half of the byte range
SANITIZE_EDGE_BYTES = np.array([ord(c) for c in "@AZ[`az{"] + list(range(128, 256)), np.uint8)
SANITIZE_SIZES = [0, 1, 15, 16, 17, 4095, 4096, 4097, 4096 * 1024 + 1]


def sanitize_input(n: int, kind: str) -> np.ndarray:
    rng = np.random.default_rng(n + 17 * len(kind))
    if kind == "full":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "letters":
        return np.where(rng.random(n) < 0.5, rng.integers(65, 91, n), rng.integers(97, 123, n)).astype(np.uint8)
    if kind == "none":
        pool = np.array([b for b in range(256) if not (65 <= b <= 90 or 97 <= b <= 122)], np.uint8)
        return pool[rng.integers(0, len(pool), n)]
    assert kind == "edges"
    return SANITIZE_EDGE_BYTES[rng.integers(0, len(SANITIZE_EDGE_BYTES), n)]
