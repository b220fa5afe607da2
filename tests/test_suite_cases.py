"""The references and bounds of tests/suite_cases.py, checked on the CPU before the GPU kernels are held to them
(tests/test_gpu_suite_edges.py): the native fp32 host oracles -- plain loops, no FMA chain, one summation order --
stay inside the bounds on the very inputs the GPU tests use, and every subtly wrong fp64 restatement leaves them.
A wrong KERNEL would compute the wrong restatement in fp32, within its own bound of it; so the perturbed references are
asked to leave the bound twice over (2 E), which puts their fp32 evaluation outside E as well."""
import numpy as np
import pytest

from cme213_sp18_amd.suite import hw1, hw2, hw4
from cme213_sp18_amd.suite._dev import host

from . import suite_cases as sc

ORDERS = [2, 4, 8]
# the perturbations are shown on the two largest noise shapes and on the thinnest one that has a neighbour to confuse
PERTURB_SHAPES = [(3, 2), (257, 131), (500, 390)]


# --------------------------------------------------------------------------------------------------------- stencil
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", sc.NOISE_SHAPES)
def test_stencil_host_oracle_is_inside_the_bound(shape, order):
    g0, u, E = sc.noise_case(shape[0], shape[1], order)
    xcfl, ycfl, scale = sc.stencil_params(order)
    got = host().stencil(np.array(g0), order, xcfl, ycfl, scale, sc.STENCIL_STEPS)
    r = sc.worst_ratio(got, u, E)
    assert r <= 1.0, r
    assert np.isfinite(E).all() and (E > 0).all()
    # the bound is tight enough to mean something -- steps * g * |A|^steps of a unit field, |A| = 1 + (xcfl + ycfl)
    # sum|c| < 2.6: some 1e-5, not a tolerance one could drive a wrong tap through
    norm_a = 1 + (xcfl + ycfl) * sum(abs(c) for c in sc.COEF[order])
    assert norm_a < 2.6 and E.max() <= sc.STENCIL_STEPS * sc.stencil_gamma(order) * norm_a ** sc.STENCIL_STEPS


def _leaves_bound(shape, order, **wrong):
    g0, u, E = sc.noise_case(shape[0], shape[1], order)
    bad, _ = sc.stencil_reference(g0, order, **wrong)
    return int(np.count_nonzero(np.abs(bad - u) > 2 * E))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", PERTURB_SHAPES)
def test_stencil_bound_catches_swapped_cfl(shape, order):
    assert _leaves_bound(shape, order, swap=True) > 0


@pytest.mark.parametrize("order,k", [(2, 0), (2, 1), (4, 0), (4, 1), (4, 2), (8, 0), (8, 1), (8, 3), (8, 4), (8, 8)])
@pytest.mark.parametrize("shape", PERTURB_SHAPES)
def test_stencil_bound_catches_one_coefficient_off_by_one(shape, order, k):
    """ONE entry of the table moved by one unit (8064 -> 8063, -9 -> -8, ...): at order 8 that is 3e-5 of a tap."""
    co = list(sc.COEF[order])
    co[k] += 1.0 if co[k] < 0 else -1.0
    assert _leaves_bound(shape, order, coef=tuple(co)) > 0


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", PERTURB_SHAPES)
@pytest.mark.parametrize("which", ["top row", "bottom row", "left column", "right column"])
def test_stencil_bound_catches_a_halo_line_read_one_cell_off(shape, order, which):
    gy, gx = shape[1] + order, shape[0] + order
    halo = {"top row": ("row", 0), "bottom row": ("row", gy - 1), "left column": ("col", 0),
            "right column": ("col", gx - 1)}[which]
    assert _leaves_bound(shape, order, halo=halo) > 0


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", PERTURB_SHAPES)
def test_stencil_bound_catches_scale_on_the_interior(shape, order):
    assert _leaves_bound(shape, order, scale_interior=True) > 0


def test_stencil_instantiation_lists_match_the_switches():
    """The enumerations the bitwise GPU tests walk are the ``case`` labels of csrc/suite/stencil.hip, read from the
    source: a case added to a switch and not to the list fails here, without a GPU."""
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "suite",
                            "stencil.hip")).read()
    tune = sorted(int(k) for k in re.findall(r"case (\d+): launch_lds_tune<", src))
    want = sorted(r * 100 + a * 10 + (nt & 1) + (100000 if nt & 2 else 0) + (1000000 if nt & 4 else 0)
                  for r, a, nt in sc.LDS_TUNE_CASES)
    assert tune == want and len(set(want)) == len(want)
    two = sorted(int(k) for k in re.findall(r"case (\d+): launch_lds2<", src))
    assert two == sorted(r * 10 + a for r, a in sc.LDS2_CASES if r)
    assert (0, 0) in sc.LDS2_CASES


def test_boundary_cap_shapes_cross_their_caps():
    for order, (nx, ny) in sc.BC_CAP_WIDE.items():
        b = order // 2
        cells = 2 * ((nx + 2 * b) * b + ny * b)
        assert 1024 * 256 < cells < 1024 * 256 + 1024  # just past the fused launches' cap
    nx, ny = sc.BC_CAP_TALL_BC
    assert 2 * ((nx + 8) * 4 + ny * 4) > 4096 * 256


# -------------------------------------------------------------------------------------------------------- PageRank
def test_adversarial_graph_is_what_it_says():
    g = sc.adversarial_graph()
    d = g.deg
    assert g.n % 256 and d[0] == 0 and d[-1] == 0
    assert set(range(41)) <= set(d.tolist()) and d[sc.ADV_ROW65] == 65 and d.max() == d[sc.ADV_ROW5000] == 5000
    e, p = g.edges.astype(np.int64), g.indptr.astype(np.int64)
    rows = np.repeat(np.arange(g.n), d)
    assert np.count_nonzero(e == rows) > 100                                   # self-loops
    assert sum(len(set(e[p[i]:p[i + 1]].tolist())) < d[i] for i in range(g.n)) > 100   # duplicate edges
    assert (g.inv_deg > 0).all() and np.count_nonzero(np.abs(g.inv_deg * d - 1) < 1e-3) < g.n // 100  # not 1 / deg
    assert (g.values > 0).all() and (g.values < 1).all()


@pytest.mark.parametrize("which", ["adversarial", "large"])
def test_pagerank_host_oracle_is_inside_the_bound(which):
    g = sc.adversarial_graph() if which == "adversarial" else sc.large_graph()
    iters = sc.PAGERANK_ITERS if which == "adversarial" else 1
    ref, E = sc.pagerank_reference(g, iters)
    got = hw2.pagerank_host(hw2.Graph(g.indptr, g.edges, g.inv_deg, g.values), iters)
    assert sc.worst_ratio(got, ref, E) <= 1.0
    empty = g.deg == 0
    assert (got[empty] == np.float32(0.5) / np.float32(g.n)).all()
    # relative bounds add up along a path: at most (longest row + 4) u per propagation, 1e-6 where no long row feeds in
    assert (E <= iters * (g.deg.max() + 4) * sc.U * ref).all()
    assert np.median(E / ref) < 1e-5


def _pagerank_leaves_bound(g, bad):
    ref, E = sc.pagerank_reference(g)
    got, _ = sc.pagerank_reference(bad)
    return int(np.count_nonzero(np.abs(got - ref) > 2 * E))


def _drop_edge(g, row, j):
    p = g.indptr.astype(np.int64)
    at = p[row] + j
    p2 = p.copy()
    p2[row + 1:] -= 1
    return sc.CsrGraph(p2, np.delete(g.edges, at), g.inv_deg, g.values)


def test_pagerank_bound_catches_an_edge_dropped_from_the_longest_row():
    """At 5000 edges the bound is 3e-4 of the row's value while an average edge carries 2e-4 of it: no bound valid for
    every summation order can see an average edge go.  The edge dropped is the row's heaviest in the last propagation,
    about ten times the average (inv_deg spans 2^-6..2)."""
    g = sc.adversarial_graph()
    p = g.indptr.astype(np.int64)
    lo, hi = p[sc.ADV_ROW5000], p[sc.ADV_ROW5000 + 1]
    last_in = sc.pagerank_reference(g, history=True)[-2][0]
    src = g.edges[lo:hi].astype(np.int64)
    j = int(np.argmax(last_in[src] * g.inv_deg[src]))
    assert _pagerank_leaves_bound(g, _drop_edge(g, sc.ADV_ROW5000, j)) > 0


def test_pagerank_bound_catches_the_last_edge_dropped_from_the_65_edge_row():
    """The edge an 8-lane, 2-deep unrolled loop reaches only on its fifth trip (65 = 4 x 16 + 1)."""
    g = sc.adversarial_graph()
    assert _pagerank_leaves_bound(g, _drop_edge(g, sc.ADV_ROW65, 64)) > 0


@pytest.mark.parametrize("row", ["first", "last"])
def test_pagerank_bound_catches_an_empty_row_given_an_edge(row):
    g = sc.adversarial_graph()
    r = 0 if row == "first" else g.n - 1
    p = g.indptr.astype(np.int64).copy()
    p[r + 1:] += 1
    bad = sc.CsrGraph(p, np.insert(g.edges, p[r], 7), g.inv_deg, g.values)
    assert _pagerank_leaves_bound(g, bad) > 0


def test_pagerank_bound_catches_inv_deg_off_by_1024_ulp():
    """inv_deg of ONE node moved by 2^10 units in its last place (1.2e-4 relative).  The node is the single source of a
    one-edge row and has a short row itself, so that its own value is known to 1e-5 and the change is not hidden."""
    g = sc.adversarial_graph()
    d, p = g.deg, g.indptr.astype(np.int64)
    ones = np.flatnonzero(d == 1)
    k = next(int(g.edges[p[i]]) for i in ones if 0 < d[g.edges[p[i]]] <= 40)
    inv = g.inv_deg.copy()
    inv[k] = (inv[k:k + 1].view(np.int32) + 1024).view(np.float32)[0]
    assert _pagerank_leaves_bound(g, sc.CsrGraph(g.indptr, g.edges, inv, g.values)) > 0


def test_premul_is_the_correctly_rounded_product():
    g = sc.adversarial_graph()
    assert np.array_equal(sc.premul_exact(g.values, g.inv_deg), g.values * g.inv_deg)


# ------------------------------------------------------------------------------------------------- integer kernels
@pytest.mark.parametrize("kind", ["full", "ones", "even", "odd"])
def test_sum_inputs_overflow_32_bits_and_match_the_host(kind):
    v = sc.sum_inputs(100_003, kind)
    even, odd = sc.sum_even_odd_exact(v)
    assert (even, odd) == (sum(int(x) for x in v if x % 2 == 0), sum(int(x) for x in v if x % 2))
    assert even + odd >= 2 ** 32 * 1000
    assert hw1.sum_even_odd_serial(v) == (even, odd) == hw1.sum_even_odd_parallel(v)
    if kind in ("ones", "odd"):
        assert even == 0
    if kind == "even":
        assert odd == 0


@pytest.mark.parametrize("start_bit", [0, 8, 16, 24])
def test_stable_partition_is_observable_on_keys_alone(start_bit):
    keys = np.random.default_rng(start_bit).integers(0, 2 ** 32, 40_000, dtype=np.uint64).astype(np.uint32)
    out = sc.stable_partition(keys, start_bit)
    dig = (out >> np.uint32(start_bit)) & np.uint32(255)
    assert (np.diff(dig.astype(np.int64)) >= 0).all() and np.array_equal(np.sort(out), np.sort(keys))
    # an UNSTABLE partition (equal digits in reverse input order) differs: equal digits carry distinct other bits
    rev = keys[::-1][np.argsort(((keys[::-1] >> np.uint32(start_bit)) & np.uint32(255)), kind="stable")]
    assert not np.array_equal(rev, out)
    # four passes are the sort
    k = keys
    for b in (0, 8, 16, 24):
        k = sc.stable_partition(k, b)
    assert np.array_equal(k, np.sort(keys))


def test_shifted_matches_exact_counts_zero_past_the_end():
    t = np.random.default_rng(5).integers(97, 100, 50, dtype=np.uint8)
    c = sc.shifted_matches_exact(t, 1, 300)
    assert c[:49] == [sum(int(t[i] == t[i + s]) for i in range(50 - s)) for s in range(1, 50)]
    assert c[49:] == [0] * 250 and sum(c[:20]) > 100


@pytest.mark.parametrize("kind", ["full", "letters", "none", "edges"])
def test_sanitize_inputs_are_what_they_say(kind):
    t = sc.sanitize_input(5000, kind)
    clean = hw4.sanitize_host(t)
    if kind == "letters":
        assert clean.size == t.size and (t < 97).any() and (t >= 97).any()
    elif kind == "none":
        assert clean.size == 0 and (t >= 128).any() and {64, 91, 96, 123} <= set(t.tolist())
    elif kind == "edges":
        assert set(t.tolist()) == set(sc.SANITIZE_EDGE_BYTES.tolist())
        assert set(clean.tolist()) == {97, 122}
    else:
        assert 0 < clean.size < t.size and (t >= 128).any()
    assert ((clean >= 97) & (clean <= 122)).all()


def test_vigenere_host_handles_every_byte_and_shift():
    """The host reference over the full byte range with shifts of 0, negatives, +-26, +-1000, against Python ints."""
    t = np.arange(256, dtype=np.uint8)
    shifts = [0, -1, 26, -26, 1000, -1000, 25]
    for sign in (1, -1):
        w = hw4.vigenere_host(t, shifts, sign, True)
        r = hw4.vigenere_host(t, shifts, sign, False)
        for i in range(256):
            s = sign * shifts[i % 7]
            assert w[i] == 97 + (i - 97 + s) % 26 and r[i] == (i + s) % 256
