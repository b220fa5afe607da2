"""The homework-suite kernels (csrc/suite/*.hip) past their grid caps, at every instantiation, and on inputs that can
fail: each HIP kernel against an fp64 restatement with a derived per-element bound, or an exact integer reference
(tests/suite_cases.py; the bounds are shown to hold and to bite on the CPU in tests/test_suite_cases.py).

Grid-stride loops and the test that makes each take a second trip:
  pagerank_kernel<1>, pagerank_premul_kernel (8192 x 256)        test_pagerank_large_graph_wraps_every_cap
  pagerank_w_kernel<1|2|4|8> (16384 x 256, n lpn > 4,194,304)    test_pagerank_large_graph_wraps_every_cap
  stencil_fused / stencil_lds2_fused boundary workgroups (1024)  test_stencil_boundary_workgroups_past_their_cap,
                                                                 test_stencil_two_step_boundary_past_its_cap
  stencil_bc_kernel (4096 x 256)                                 test_stencil_bc_alone_past_its_cap
  vigenere_kernel (4096 x 256)                                   test_vigenere_full_range
  byte_hist_kernel (1024 x 256 x 4 B)                            test_byte_histogram_past_its_cap
  residue_hist_kernel (512 x 256)                                test_residue_histogram_past_its_cap
  shift_*_kernel (grid_cap)                                      test_shift_small_grid_cap
  radix_scan_kernel rounds of 1024 tiles (run += rtot)           test_radix_sort_second_scan_round, test_radix_pass_*
  scan_exclusive_kernel with per > 1 (more than 1024 tiles)      test_sanitize (n = 4096 * 1024 + 1)
Instantiations that had never been compared: every (rows, ahead) of stencil_step2_bc -- <64,2> and <96,2>, the forms
behind the published 12288^2 and 8192^2 figures, among them -- in test_stencil_two_step_instantiation_is_bitwise; every
(rows, ahead, nt) of stencil_lds_tune in test_stencil_lds_tune_instantiation_is_bitwise; pagerank_propagate_w at every
lpn, forced, on rows shorter than lpn and n lpn off a multiple of 256 in test_pagerank_adversarial_graph.

Worst measured |err| / bound per kernel on the MI355X (profiles/numerics_suite.jsonl), all below 1:
  stencil, 3 steps of noise (global, block, shared, vec: the same bits)   order 2: 0.118   4: 0.091   8: 0.060
  stencil shared2 (two-step walk), 3 steps of noise                       order 8: 0.060
  stencil, 1 step on the cap shapes (every variant the same bits)         order 2: 0.228   4: 0.201   8: 0.179
  stencil shared2, 2 steps on the cap shapes                              0.038;  shared on (500, 800): 0.201
  pagerank_kernel<1> / <8>                      adversarial 0.206 / 0.206     4,194,561 nodes 0.391 / 0.394
  pagerank_w_kernel lpn 1, 2, 4, 8: out         adversarial 0.206             4,194,561 nodes 0.391 .. 0.394
  pagerank_w_kernel lpn 1, 2, 4, 8: w_out       adversarial 0.283             4,194,561 nodes 0.445
The integer kernels, the border cells, pagerank_premul and every instantiation test are exact comparisons.
"""
import json

import numpy as np
import pytest
import torch

from cme213_sp18_amd.suite import hw1, hw2, hw4
from cme213_sp18_amd.suite._dev import kernels, stream_handle

from . import suite_cases as sc

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL = 0x7FC0DEAD  # a quiet NaN no kernel produces
GUARD = 4096           # floats of guard band on either side (a multiple of 4: the grid stays 16-byte aligned)


def _log(**kw):
    print("NUMERICS " + json.dumps(kw))


def _cuda(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


# ===================================================================================================== stencil
VARIANT = {"global": 0, "block": 1, "shared": 2, "vec": 3}


def _run_stencil(g0, order, variant, fused, steps):
    """``steps`` steps through the bindings with suite_cases' parameters (not SimParams').  ``shared2``: pairs of
    steps by the two-step walk, an odd last one by the one-step LDS walk in the asked form."""
    k, s = kernels(), stream_handle()
    xcfl, ycfl, scale = sc.stencil_params(order)
    gy, gx = g0.shape
    cur = torch.from_numpy(np.array(g0)).cuda()
    nxt = cur.clone()

    def one(v):
        if fused:
            k.stencil_step_bc(nxt.data_ptr(), cur.data_ptr(), gx, gy, order, xcfl, ycfl, v, scale, s)
        else:
            k.stencil_bc(nxt.data_ptr(), cur.data_ptr(), gx, gy, order // 2, scale, s)
            k.stencil_step(nxt.data_ptr(), cur.data_ptr(), gx, gy, order, xcfl, ycfl, v, s)

    done = 0
    while done < steps:
        if variant == "shared2" and steps - done >= 2:
            k.stencil_step2_bc(nxt.data_ptr(), cur.data_ptr(), gx, gy, order, xcfl, ycfl, scale, s)
            done += 2
        else:
            one(VARIANT["shared" if variant == "shared2" else variant])
            done += 1
        cur, nxt = nxt, cur
    return cur.cpu().numpy()


NOISE_CASES = [(v, o, f) for v in ["global", "block", "shared", "vec", "shared2"] for o in [2, 4, 8]
               for f in ["fused", "two-launch"] if v != "shared2" or o == 8]  # (the two-step walk: order 8 only)


@pytest.mark.parametrize("variant,order,form", NOISE_CASES)
def test_stencil_noise_within_fp64_bound(variant, order, form):
    """Uniform noise in [-1, 1], 3 steps, |gpu - u64| <= E on every element, border included, at (1, 1), (3, 2),
    (5, 1023), (257, 131) and (500, 390)."""
    fused = form == "fused"
    worst = {}
    for nx, ny in sc.NOISE_SHAPES:
        g0, u, E = sc.noise_case(nx, ny, order)
        got = _run_stencil(g0, order, variant, fused, sc.STENCIL_STEPS)
        worst[(nx, ny)] = r = sc.worst_ratio(got, u, E)
        _log(kernel="stencil", variant=variant, order=order, fused=fused, shape=[nx, ny], steps=sc.STENCIL_STEPS,
             ratio=r)
    assert max(worst.values()) <= 1.0, worst


@pytest.fixture(scope="module")
def bitwise_grid():
    """Order-8 noise on (500, 800); the production walk's interior step and two fused one-step launches."""
    nx, ny = sc.BITWISE_SHAPE
    g0 = sc.noise_grid(nx, ny, 8)
    k, s = kernels(), stream_handle()
    xcfl, ycfl, scale = sc.stencil_params(8)
    gy, gx = g0.shape
    a = torch.from_numpy(g0).cuda()
    one = a.clone()
    k.stencil_step(one.data_ptr(), a.data_ptr(), gx, gy, 8, xcfl, ycfl, 2, s)
    b, c = a.clone(), a.clone()
    k.stencil_step_bc(b.data_ptr(), a.data_ptr(), gx, gy, 8, xcfl, ycfl, 2, scale, s)
    k.stencil_step_bc(c.data_ptr(), b.data_ptr(), gx, gy, 8, xcfl, ycfl, 2, scale, s)
    u1, E1 = sc.stencil_reference(g0, 8, 1)
    u2, E2 = sc.stencil_reference(g0, 8, 2)
    r1 = sc.worst_ratio(one.cpu().numpy()[4:-4, 4:-4], u1[4:-4, 4:-4], E1[4:-4, 4:-4])
    r2 = sc.worst_ratio(c.cpu().numpy(), u2, E2)
    _log(kernel="stencil", variant="shared", order=8, shape=[nx, ny], steps=1, ratio=r1)
    _log(kernel="stencil", variant="shared", order=8, shape=[nx, ny], steps=2, ratio=r2)
    assert r1 <= 1.0 and r2 <= 1.0  # what the others are bitwise equal to is itself right
    return dict(a=a, one=one, two=c, gx=gx, gy=gy, p=(xcfl, ycfl, scale))


@pytest.mark.parametrize("rows,ahead,nt", sc.LDS_TUNE_CASES)
def test_stencil_lds_tune_instantiation_is_bitwise(bitwise_grid, rows, ahead, nt):
    """stencil_lds_tune's (rows 16/32/64/128, ahead 4/6/8, non-temporal loads, one-direction or alternating walk,
    plain stores) against stencil_step(variant 2) on the interior: two row blocks at rows = 128, a partial last block,
    a partial last strip."""
    w = bitwise_grid
    out = w["a"].clone()
    kernels().stencil_lds_tune(out.data_ptr(), w["a"].data_ptr(), w["gx"], w["gy"], w["p"][0], w["p"][1], rows, ahead,
                               nt, stream_handle())
    assert torch.equal(out.view(torch.int32), w["one"].view(torch.int32))


@pytest.mark.parametrize("rows,ahead", sc.LDS2_CASES)
def test_stencil_two_step_instantiation_is_bitwise(bitwise_grid, rows, ahead):
    """stencil_step2_bc's launch_lds2<rows, ahead> -- (0, 0) the automatic pick -- against two
    stencil_step_bc(variant 2) launches on the whole grid."""
    w = bitwise_grid
    out = torch.full_like(w["a"], float("nan"))
    kernels().stencil_step2_bc(out.data_ptr(), w["a"].data_ptr(), w["gx"], w["gy"], 8, *w["p"], stream_handle(),
                               rows, ahead)
    assert torch.equal(out.view(torch.int32), w["two"].view(torch.int32))


class _GuardedPair:
    """curr and next, each between two guard bands of NaN sentinels; next starts as sentinels throughout."""

    def __init__(self, g0):
        self.gy, self.gx = g0.shape
        self.n = g0.size
        self.raw = [torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(2)]
        self.raw[0].view(torch.float32)[GUARD:GUARD + self.n] = torch.from_numpy(g0.ravel()).cuda()
        self.cur_bits = _bits(g0)
        self.curr, self.next = (r[GUARD:].data_ptr() for r in self.raw)
        assert self.curr % 16 == 0 and self.next % 16 == 0

    def result(self):
        """next's grid as fp32 [gy][gx], after checking that no guard cell and no cell of curr was written."""
        raw = [r.cpu().numpy() for r in self.raw]
        for row in raw:
            assert (row[:GUARD] == SENTINEL).all() and (row[GUARD + self.n:] == SENTINEL).all(), "guard band written"
        assert np.array_equal(raw[0][GUARD:GUARD + self.n].reshape(self.gy, self.gx), self.cur_bits), "curr written"
        return raw[1][GUARD:GUARD + self.n].view(F32).reshape(self.gy, self.gx)


def _cap_shape(order, side):
    nx, ny = sc.BC_CAP_WIDE[order]
    return (nx, ny) if side == "wide" else (ny, nx)


@pytest.mark.parametrize("side", ["wide", "tall"])
@pytest.mark.parametrize("order", [2, 4, 8])
@pytest.mark.parametrize("variant", ["global", "block", "shared", "vec"])
def test_stencil_boundary_workgroups_past_their_cap(variant, order, side):
    """stencil_fused's boundary workgroups are capped at 1024 x 256 threads; these grids have just over 262,144 border
    cells, in the top and bottom strips (wide: ny = 1) or in the side strips (tall: nx = 1), so the stride loop takes
    a second trip.  One step on noise: border bitwise float32(curr * scale), interior within the bound, nothing
    written outside the grid."""
    nx, ny = _cap_shape(order, side)
    b = order // 2
    g0 = sc.noise_grid(nx, ny, order)
    xcfl, ycfl, scale = sc.stencil_params(order)
    pair = _GuardedPair(g0)
    kernels().stencil_step_bc(pair.next, pair.curr, pair.gx, pair.gy, order, xcfl, ycfl, VARIANT[variant], scale,
                              stream_handle())
    got = pair.result()
    m = sc.border_mask(pair.gy, pair.gx, b)
    assert np.array_equal(_bits(got)[m], _bits(g0 * F32(scale))[m])
    u, E = sc.stencil_reference(g0, order, 1)
    r = sc.worst_ratio(got[~m], u[~m], E[~m])
    _log(kernel="stencil", test="bc cap", variant=variant, order=order, shape=[nx, ny], steps=1, ratio=r)
    assert r <= 1.0


@pytest.mark.parametrize("side", ["wide", "tall"])
def test_stencil_two_step_boundary_past_its_cap(side):
    """stencil_lds2_fused's boundary workgroups (bc2_cells, the same 1024 x 256 cap) at (32800, 1) and (1, 32800):
    border bitwise float32(float32(curr * scale) * scale), interior within the two-step bound, guards untouched."""
    nx, ny = _cap_shape(8, side)
    g0 = sc.noise_grid(nx, ny, 8)
    xcfl, ycfl, scale = sc.stencil_params(8)
    pair = _GuardedPair(g0)
    kernels().stencil_step2_bc(pair.next, pair.curr, pair.gx, pair.gy, 8, xcfl, ycfl, scale, stream_handle())
    got = pair.result()
    m = sc.border_mask(pair.gy, pair.gx, 4)
    assert np.array_equal(_bits(got)[m], _bits((g0 * F32(scale)) * F32(scale))[m])
    u, E = sc.stencil_reference(g0, 8, 2)
    r = sc.worst_ratio(got[~m], u[~m], E[~m])
    _log(kernel="stencil", test="bc cap", variant="shared2", order=8, shape=[nx, ny], steps=2, ratio=r)
    assert r <= 1.0


@pytest.mark.parametrize("order,shape", [(2, sc.BC_CAP_WIDE[2]), (8, sc.BC_CAP_WIDE[8]), (8, sc.BC_CAP_WIDE[8][::-1]),
                                         (8, sc.BC_CAP_TALL_BC), (8, sc.BC_CAP_TALL_BC[::-1])],
                         ids=["order2-wide", "order8-wide", "order8-tall", "order8-tall-1M", "order8-wide-1M"])
def test_stencil_bc_alone_past_its_cap(order, shape):
    """stencil_bc_kernel alone (the two-launch form's first launch): 4096 x 256 threads; the 1M shapes have more than
    1,048,576 border cells.  Border bitwise float32(curr * scale); the interior and the guards keep their sentinels."""
    nx, ny = shape
    b = order // 2
    g0 = sc.noise_grid(nx, ny, order)
    scale = sc.stencil_params(order)[2]
    pair = _GuardedPair(g0)
    kernels().stencil_bc(pair.next, pair.curr, pair.gx, pair.gy, b, scale, stream_handle())
    got = pair.result()
    m = sc.border_mask(pair.gy, pair.gx, b)
    assert np.array_equal(_bits(got)[m], _bits(g0 * F32(scale))[m])
    assert (_bits(got)[~m] == SENTINEL).all()


# ==================================================================================================== PageRank
PR_FORMS = ["thread", "lanes8", "w-lpn1", "w-lpn2", "w-lpn4", "w-lpn8"]


class _DevGraph:
    def __init__(self, g):
        self.g, self.n = g, g.n
        self.indptr, self.edges, self.inv, self.vals = _cuda(g.indptr), _cuda(g.edges), _cuda(g.inv_deg), _cuda(g.values)

    def run(self, form, iters):
        """(out, w_out or None) after ``iters`` propagations of one form, lpn forced through the binding."""
        k, s = kernels(), stream_handle()
        src, dst = self.vals.clone(), torch.empty_like(self.vals)
        if not form.startswith("w-"):
            for _ in range(iters):
                k.pagerank_propagate(self.indptr.data_ptr(), self.edges.data_ptr(), src.data_ptr(), dst.data_ptr(),
                                     self.inv.data_ptr(), self.n, 0 if form == "thread" else 1, s)
                src, dst = dst, src
            return src.cpu().numpy(), None
        lpn = int(form[5:])
        wsrc, wdst = torch.empty_like(src), torch.empty_like(src)
        k.pagerank_premul(src.data_ptr(), self.inv.data_ptr(), wsrc.data_ptr(), self.n, s)
        for _ in range(iters):
            k.pagerank_propagate_w(self.indptr.data_ptr(), self.edges.data_ptr(), wsrc.data_ptr(), dst.data_ptr(),
                                   wdst.data_ptr(), self.inv.data_ptr(), self.n, lpn, s)
            src, dst, wsrc, wdst = dst, src, wdst, wsrc
        return src.cpu().numpy(), wsrc.cpu().numpy()


def _check_pagerank(dg, form, iters, ref, E, tag):
    g = dg.g
    out, w = dg.run(form, iters)
    r = sc.worst_ratio(out, ref, E)
    rw = None
    if w is not None:
        wref, wE = sc.pagerank_w_bound(g, ref, E)
        rw = sc.worst_ratio(w, wref, wE)
    _log(kernel="pagerank", graph=tag, form=form, iters=iters, ratio=r, ratio_w=rw)
    assert r <= 1.0 and (rw is None or rw <= 1.0)
    assert (out[g.deg == 0] == F32(0.5) / F32(g.n)).all()  # an empty row is the base, bitwise


@pytest.fixture(scope="module")
def adversarial():
    g = sc.adversarial_graph()
    return _DevGraph(g), sc.pagerank_reference(g, sc.PAGERANK_ITERS)


@pytest.mark.parametrize("form", PR_FORMS)
def test_pagerank_adversarial_graph(adversarial, form):
    """3001 nodes (n lpn off a multiple of 256), rows of 0..40, 65 and 5000 edges (shorter than lpn; past one trip of
    the unrolled loops), empty first and last rows, self-loops, duplicates, arbitrary inv_deg: 3 iterations of
    pagerank_kernel<1>, <8> and pagerank_w_kernel at lpn 1, 2, 4, 8 within the fp64 bound."""
    dg, (ref, E) = adversarial
    _check_pagerank(dg, form, sc.PAGERANK_ITERS, ref, E, "adversarial")


@pytest.fixture(scope="module")
def large():
    g = sc.large_graph()
    return _DevGraph(g), sc.pagerank_reference(g, 1)


@pytest.mark.parametrize("form", PR_FORMS + ["premul"])
def test_pagerank_large_graph_wraps_every_cap(large, form):
    """n = 4,194,304 + 257: pagerank_kernel<1> and pagerank_premul_kernel (8192 x 256 threads) and pagerank_w_kernel at
    every lpn -- 1, 2 and 4 for the first time -- (16384 x 256) take a second trip of their node loops."""
    dg, (ref, E) = large
    if form == "premul":
        w = torch.empty_like(dg.vals)
        kernels().pagerank_premul(dg.vals.data_ptr(), dg.inv.data_ptr(), w.data_ptr(), dg.n, stream_handle())
        assert np.array_equal(_bits(w.cpu().numpy()), _bits(sc.premul_exact(dg.g.values, dg.g.inv_deg)))
        return
    _check_pagerank(dg, form, 1, ref, E, "large")


# ========================================================================================================= hw1
@pytest.mark.parametrize("kind", ["full", "ones", "even", "odd"])
def test_sum_even_odd_64_bit(kind):
    """Full-range values: both sums are far past 2^32, so a 32-bit accumulator anywhere shows.  n = 4 * 2^20 + 0..3
    (the scalar tail after the 16-byte loads) and 7."""
    for n in [4 * 2 ** 20 + r for r in range(4)] + [7]:
        v = sc.sum_inputs(n, kind)
        got = hw1.sum_even_odd_gpu(_cuda(v)).cpu().tolist()
        want = sc.sum_even_odd_exact(v)
        assert tuple(x & (2 ** 64 - 1) for x in got) == want, (kind, n)
        assert n == 7 or sum(want) > 2 ** 32 * 1_000_000


def _sort(keys):
    return hw1.radix_sort_gpu(_cuda(keys)).cpu().numpy().view(np.uint32)


def _keys(n, seed=0):
    return np.random.default_rng(seed + n).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)


def test_radix_sort_second_scan_round():
    """4096 * 1024 + 1 keys: 1025 tiles, so radix_scan_kernel's loop runs a second round (run += rtot) whose only tile
    holds one key."""
    keys = _keys(4096 * 1024 + 1)
    assert np.array_equal(_sort(keys), np.sort(keys))


@pytest.mark.parametrize("kind", ["sorted", "reversed", "equal", "ones", "low-digits-constant", "empty"])
def test_radix_sort_patterns(kind):
    n = 100_003
    keys = _keys(n, 1)
    if kind == "sorted":
        keys = np.sort(keys)
    elif kind == "reversed":
        keys = np.sort(keys)[::-1].copy()
    elif kind == "equal":
        keys[:] = 0x12345678
    elif kind == "ones":
        keys[:] = 0xFFFFFFFF
    elif kind == "low-digits-constant":
        keys = (keys & np.uint32(0xFF000000)) | np.uint32(0x00A5C33C)
    else:
        keys = keys[:0]
    out = _sort(keys)
    assert out.shape == keys.shape and np.array_equal(out, np.sort(keys))


@pytest.mark.parametrize("n", [40_001, 4096 * 1024 + 1])
@pytest.mark.parametrize("start_bit", [8, 16, 24])
def test_radix_pass_is_the_stable_partition(start_bit, n):
    """radix_pass_u32 on the upper digits against a stable argsort of the digit: equal digits carry distinct other
    bits, so an unstable or misplaced scatter shows on the keys alone."""
    keys = _keys(n, start_bit)
    d = _cuda(keys)
    dst = torch.empty_like(d)
    hw1.GpuRadixSorter(n).pass_(d, dst, start_bit)
    assert np.array_equal(dst.cpu().numpy().view(np.uint32), sc.stable_partition(keys, start_bit))


def test_sum_even_odd_refuses_a_wrong_out():
    """Nothing is launched: the wrapper refuses an ``out`` the kernel would overrun."""
    v = torch.zeros(8, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        hw1.sum_even_odd_gpu(v, torch.empty(1, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        hw1.sum_even_odd_gpu(v, torch.empty(3, dtype=torch.int64, device="cuda"))
    with pytest.raises(TypeError):
        hw1.sum_even_odd_gpu(v, torch.empty(2, dtype=torch.int32, device="cuda"))
    with pytest.raises(TypeError):
        hw1.sum_even_odd_gpu(v, torch.empty(2, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        hw1.sum_even_odd_gpu(v, torch.empty(2, dtype=torch.int64))
    with pytest.raises(ValueError):
        hw1.sum_even_odd_gpu(v, torch.empty(4, dtype=torch.int64, device="cuda")[::2])
    out = torch.empty(2, dtype=torch.int64, device="cuda")
    assert hw1.sum_even_odd_gpu(v, out) is out and out.tolist() == [0, 0]


# =================================================================================================== hw2 shift
@pytest.mark.parametrize("block", [64, 1024])
@pytest.mark.parametrize("grid_cap", [1, 3])
@pytest.mark.parametrize("width", hw2.SHIFT_WIDTHS)
def test_shift_small_grid_cap(width, grid_cap, block):
    """shift_u8_kernel and shift_wide_kernel<4|8|16> with the grid clamped to 1 or 3 workgroups: the stride loop runs
    many trips over n = 10,007 bytes and leaves a tail."""
    t = np.random.default_rng(width).integers(0, 256, 10_007, dtype=np.uint8)
    d = _cuda(t)
    for shift in (0, 1, 200, 255):
        out = hw2.shift_gpu(d, shift, width, block=block, grid_cap=grid_cap).cpu().numpy()
        assert np.array_equal(out, hw2.shift_host(t, shift)), shift


def test_shift_refuses_a_wrong_out():
    """Nothing is launched: the wrapper refuses an ``out`` the kernel would overrun or write misaligned."""
    inp = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        hw2.shift_gpu(inp, 1, 16, out=torch.empty(63, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        hw2.shift_gpu(inp, 1, 1, out=torch.empty(65, dtype=torch.uint8, device="cuda"))
    with pytest.raises(TypeError):
        hw2.shift_gpu(inp, 1, 4, out=torch.empty(64, dtype=torch.int8, device="cuda"))
    with pytest.raises(TypeError):
        hw2.shift_gpu(inp, 1, 4, out=torch.empty(16, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        hw2.shift_gpu(inp, 1, 4, out=torch.empty(64, dtype=torch.uint8))
    with pytest.raises(ValueError):
        hw2.shift_gpu(inp, 1, 1, out=torch.empty(128, dtype=torch.uint8, device="cuda")[::2])
    big = torch.empty(80, dtype=torch.uint8, device="cuda")
    for width in (4, 8, 16):
        with pytest.raises(ValueError):
            hw2.shift_gpu(inp, 1, width, out=big[1:65])
    out = big[1:65]
    assert hw2.shift_gpu(inp, 7, 1, out=out) is out and (out == 7).all()  # a byte-wide lane needs no alignment


# ========================================================================================================= hw4
@pytest.mark.parametrize("kind", ["full", "letters", "none", "edges"])
def test_sanitize(kind):
    """Random bytes over the full range, all letters, no letters, and only the bytes at the edges of the letter ranges
    (@ A Z [ ` a z {) with bytes >= 128, at sizes around one thread's 16 bytes and one tile's 4096, and at 1025 tiles
    (scan_exclusive_kernel with two counts per thread)."""
    for n in sc.SANITIZE_SIZES:
        t = sc.sanitize_input(n, kind)
        got = hw4.sanitize(t).cpu().numpy()
        assert np.array_equal(got, hw4.sanitize_host(t)), (kind, n)


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("period", ["1", "7", "longer-than-n"])
@pytest.mark.parametrize("wrap", [True, False])
def test_vigenere_full_range(wrap, period, sign):
    """n = 1,048,576 + 300 (vigenere_kernel's 4096 x 256 threads take a second trip) of full-range bytes; shifts of
    0, negatives, +-26, +-1000."""
    n = 1_048_576 + 300
    t = np.random.default_rng(11).integers(0, 256, n, dtype=np.uint8)
    if period == "1":
        shifts = np.array([-1000], np.int32)
    elif period == "7":
        shifts = np.array([0, -1, 26, -26, 1000, -1000, 25], np.int32)
    else:
        shifts = np.random.default_rng(12).integers(-1000, 1001, n + 5).astype(np.int32)
    got = hw4.apply_shift(_cuda(t), shifts, sign, wrap).cpu().numpy()
    assert np.array_equal(got, hw4.vigenere_host(t, shifts, sign, wrap))


@pytest.mark.parametrize("extra", [1, 2, 3, 5])
def test_byte_histogram_past_its_cap(extra):
    """n = 1,048,576 + 1, 2, 3, 5: byte_hist_kernel's 1024 x 256 threads x 4 bytes take a second trip that is a
    partial word (or a word and a partial one); and one input that is a single byte value."""
    n = 1_048_576 + extra
    t = np.random.default_rng(extra).integers(0, 256, n, dtype=np.uint8)
    assert np.array_equal(hw4.byte_histogram(_cuda(t)).cpu().numpy(), np.bincount(t, minlength=256))
    t[:] = 0xC3
    h = hw4.byte_histogram(_cuda(t)).cpu().numpy()
    assert h[0xC3] == n and h.sum() == n


@pytest.mark.parametrize("period", [1, 7, 63, 64])
def test_residue_histogram_past_its_cap(period):
    """n = 131,072 + 77: residue_hist_kernel's 512 x 256 threads take a second trip."""
    t = np.random.default_rng(period).integers(0, 256, 131_072 + 77, dtype=np.uint8)
    got = hw4.residue_histogram(_cuda(t), period).cpu().numpy()
    assert np.array_equal(got, sc.residue_hist_exact(t, period))


@pytest.mark.parametrize("lo,hi", [(1, 2), (7, 300), (4095, 4096), (1, 4096)])
def test_shifted_matches_ranges(lo, hi):
    """Shift ranges up to the kernel's 4096-shift window, texts around one 4096-byte chunk; shifts >= n count 0.
    Three symbols, so the counts are large."""
    for n in (1, 2, 4095, 4096, 4097, 10_000):
        t = np.random.default_rng(n).integers(97, 100, n, dtype=np.uint8)
        got = hw4.shifted_matches(_cuda(t), lo, hi).tolist()
        assert got == sc.shifted_matches_exact(t, lo, hi), (lo, hi, n)
