"""Operands that put the output layer and the sigmoid at saturated logits while keeping the fp64 reference
unambiguous (shared by tests/test_saturation.py, which checks the construction on the CPU, and
tests/test_gpu_saturation.py).  numpy only; no project code.

Every logit is z2[c][j] = top_j - gap[c][j] with gap from the ladder G, and every operand is chosen so that each
product and each partial sum of W2 a1 + b2 is exactly representable in fp32 (and bf16 planes): K-splits, MFMA chains,
the z2 all-gather and any summation order give the same logits bit for bit, so the reference is the exact softmax of
known numbers and the tolerances bound the nonlinear part alone.

A column (sample) j carries one of S = 16 patterns, p = (j + p0) % 16:
* rows 0..15 of a1 are the pattern's one-hot (a1 = 1 in row p, 0 in the others) and W2[c][p] = z2[c] - b2[c];
* the rows from 16 on come in pairs (ra, rb) with W2[:, ra] = -W2[:, rb] (multiples of 1/2 up to 64) and
  a1[ra][j] = a1[rb][j] in {0, 1/2, 1}: they cancel exactly in z2, put 1/2 into a1 and make the sums dense.
  |partial sum| < 2^17 in multiples of 1/4: 19 bits.
* the pattern's winner (gap 0) is class 7 p % C; the other classes walk the ladder's rungs 1.. (wrapping over the
  classes); patterns 3, 7, 11, 15 (C = 2: 15 only, so that no rung is lost) add a second class at gap 0: the last live
  class, the next class, a class 16 up (another class tile at C > 16; 4 up below: another lane group), the last class.
* top_p cycles over TOPS1 for the shifted softmax; for the unshifted form (shift = 0) over TOPS0 with the ladder cut
  to the rungs that keep the logit >= -80.  TOPS0 = {0, +-4, 2}: unshifted, __expf rounds its argument z . log2(e)
  relative to |z|, not to the gap, so the issue's (gap + 8) 2^-23 bound is derived only where |z_c| + |top| <= 2 gap
  + 16 -- true for |top| <= 4 at every rung, false for e.g. top = 40 next to a gap of 1/2.
* labels (labels_for) put the label's gap on every rung within any 32 consecutive columns, from "the label is the
  winner" to "the label underflowed" (a single column's label is its most underflowed class).

Whole steps reach the same a1 through the first layer: raw pixels {0, 1} at 16 pattern positions and 4 bit
positions, arbitrary bytes elsewhere; W1 in {0, +-8192} at those positions and 0 elsewhere, b1 = 0, so z1 is a
multiple of 8192 and a1 = sigmoid(z1) is exactly 0, 1/2 or 1 in f32, f64 and bf16 modes."""
import numpy as np

G = (0.0, 0.5, 1.0, 3.0, 8.0, 16.0, 32.0, 64.0, 80.0, 86.0, 87.0, 88.0, 90.0, 104.0, 150.0, 200.0)
TOPS1 = (0.0, 40.0, -75.0, 1000.0)
TOPS0 = (0.0, 4.0, -4.0, 2.0)
S = 16
SEL = tuple(5 + 47 * i for i in range(S))  # the pattern pixels of a 784-pixel sample
BIT = (20, 300, 555, 770)                  # the bit pixels
BIG = 8192.0

EPS32, EPS64, TINY32 = 2.0 ** -23, 2.0 ** -50, 2.0 ** -126


def pattern_logits(C, shift):
    """z2 [C][S], gap [C][S] of the S patterns."""
    tops = TOPS1 if shift else TOPS0
    Z, gap = np.zeros((C, S)), np.zeros((C, S))
    for p in range(S):
        top = tops[(p + p // 4) % 4]
        rungs = [g for g in G[1:] if shift or top - g >= -80.0]
        win = 7 * p % C
        for c in range(C):
            k = (c - win) % C
            gap[c, p] = 0.0 if k == 0 else rungs[(k - 1 + 2 * p) % len(rungs)]
        if (p % 4 == 3 and C > 2) or p == 15:
            last = C - 1 if win != C - 1 else 0
            partner = {3: last, 7: (win + 1) % C, 11: (win + (16 if C > 16 else 4)) % C, 15: last}[p]
            if partner == win:
                partner = (win + 1) % C
            gap[partner, p] = 0.0
        Z[:, p] = top - gap[:, p]
    return Z, gap


def patterns(n, p0=0):
    return (np.arange(n) + p0) % S


def labels_for(gap, pat):
    """One label per column.  Every other column (alternating with each pass over the 16 patterns) is labelled with
    its winner; the 16 others of every 32 columns walk the ladder: each takes, from its own turn's rung upward
    (cyclically), the first rung that none of them has taken yet and that a class of the column sits on.  (Half the
    columns are easy so that the deep rungs spread over the 16-column blocks: the loss partial is an fp32 sum of its
    block, and its bound does not budget for the rounding of a sum of sixteen terms near 100.)  A single column is
    labelled with its most underflowed class."""
    C = gap.shape[0]
    lab = np.zeros(len(pat), np.int32)
    seen, turn = set(), 0
    for j, p in enumerate(pat):
        if j % 32 == 0:
            seen, turn = set(), 0
        if len(pat) == 1:
            lab[j] = int(np.argmax(gap[:, p]))
        elif (j + j // 16) % 2:
            lab[j] = int(np.argmin(gap[:, p]))
        else:
            order = [G[1 + (7 * turn + i) % 15] for i in range(15)]
            have = [g for g in order if (gap[:, p] == g).any()]
            g = next((g for g in have if g not in seen), have[0] if have else 0.0)  # (C = 2's tie: both at gap 0)
            seen.add(g)
            turn += 1
            lab[j] = int(np.argmax(gap[:, p] == g))
    return lab


def head_operands(C, H, n, shift, p0=0, seed=0):
    """W2 [C][H], b2 [C], a1 [H][n], labels [n], and the exact z2 [C][n], gap [C][n] -- all fp64 arrays holding
    values exact in fp32."""
    assert H >= S
    rng = np.random.default_rng((C, H, n, seed))
    Z, gap = pattern_logits(C, shift)
    pat = patterns(n, p0)
    b2 = -0.5 * (np.arange(C) % 5)
    W2 = np.zeros((C, H))
    W2[:, :S] = Z - b2[:, None]
    a1 = np.zeros((H, n))
    a1[pat, np.arange(n)] = 1.0
    rows = S + rng.permutation(H - S)
    for ra, rb in zip(rows[0::2], rows[1::2]):  # (an odd row out keeps W2 = 0, a1 = 0)
        v = rng.integers(-128, 129, C) * 0.5
        W2[:, ra], W2[:, rb] = v, -v
        a1[ra] = a1[rb] = rng.integers(0, 3, n) * 0.5
    return W2, b2, a1, labels_for(gap, pat), Z[:, pat], gap[:, pat]


def step_operands(P, H, C, N, seed=0):
    """Whole-step operands (shifted softmax): pixels [N][P] uint8, labels [N], W1 [H][P], b1 [H], W2 [C][H], b2 [C],
    and the exact a1 [H][N], z2 [C][N], gap [C][N] they give."""
    assert P > max(SEL + BIT) and H >= S
    rng = np.random.default_rng((P, H, C, N, seed))
    Z, gap = pattern_logits(C, 1)
    pat = patterns(N)
    x = rng.integers(0, 256, (N, P)).astype(np.uint8)
    x[:, SEL] = 0
    x[np.arange(N), np.asarray(SEL)[pat]] = 1
    bits = rng.integers(0, 2, (N, len(BIT)))
    x[:, BIT] = bits
    W1 = np.zeros((H, P))
    W1[:S, SEL] = -BIG
    W1[np.arange(S), SEL] = BIG
    b2 = -0.5 * (np.arange(C) % 5)
    W2 = np.zeros((C, H))
    W2[:, :S] = Z - b2[:, None]
    a1 = np.zeros((H, N))
    a1[pat, np.arange(N)] = 1.0
    rows = S + rng.permutation(H - S)
    for ra, rb in zip(rows[0::2], rows[1::2]):
        v = rng.integers(-128, 129, C) * 0.5
        W2[:, ra], W2[:, rb] = v, -v
        s = rng.choice([-1.0, 0.0, 0.0, 1.0], len(BIT))
        W1[ra, BIT] = W1[rb, BIT] = s * BIG
        k = bits @ s
        a1[ra] = a1[rb] = np.where(k > 0, 1.0, np.where(k < 0, 0.0, 0.5))
    if (H - S) % 2:
        a1[rows[-1]] = 0.5  # (the odd row out: W1 = 0 -> z1 = 0; W2 = 0)
    return x, labels_for(gap, pat), W1, np.zeros(H), W2, b2, a1, Z[:, pat], gap[:, pat]


def softmax_reference(z2, lab):
    """fp64: yhat [C][n], the loss of every column (log sum - (z_label - m)), the first maximum of every column."""
    z2 = np.asarray(z2, np.float64)
    m = z2.max(0)
    e = np.exp(z2 - m)
    s = e.sum(0)
    cols = np.arange(z2.shape[1])
    return e / s, np.log(s) - (z2[lab, cols] - m), z2.argmax(0)


def head_reference(W2, b2, a1, lab, z2, scale):
    """fp64 yhat, D / scale, D, dZ1, per-column loss, first maximum."""
    yh, loss, pred = softmax_reference(z2, lab)
    onehot = np.zeros_like(yh)
    onehot[lab, np.arange(len(lab))] = 1.0
    D = (yh - onehot) * scale
    dZ1 = (W2.T @ D) * a1 * (1.0 - a1)
    return yh, yh - onehot, D, dZ1, loss, pred


def head_f32(W2, b2, a1, lab, scale, shift):
    """A plain fp32 numpy restatement of the stable formulas (independent of the project's code): yhat, D, dZ1, loss
    per column.  z2 is summed in fp32."""
    f = np.float32
    W2, b2, a1 = W2.astype(f), b2.astype(f), a1.astype(f)
    z2 = (W2 @ a1 + b2[:, None]).astype(f)
    m = z2.max(0) if shift else np.zeros(z2.shape[1], f)
    e = np.exp(z2 - m).astype(f)
    s = e.sum(0, dtype=f)
    yh = (e * (f(1) / s)).astype(f)
    cols = np.arange(z2.shape[1])
    onehot = np.zeros_like(yh)
    onehot[lab, cols] = 1
    D = ((yh - onehot) * f(scale)).astype(f)
    dZ1 = ((W2.T @ D) * a1 * (f(1) - a1)).astype(f)
    loss = (np.log(s).astype(f) - (z2[lab, cols] - m)).astype(f)
    return yh, D, dZ1, loss


def prob_bound(gap, ref, eps=EPS32, floor=TINY32):
    """|got - ref| <= (gap + 8) eps |ref| + floor, per element."""
    return (gap + 8.0) * eps * np.abs(ref) + floor


def grad_bound(gap, yh, onehot, eps=EPS32, floor=TINY32):
    """The bound of D / scale = yhat - onehot.  Off the label it is prob_bound of the element itself.  At the label
    the reference yhat - 1 can be far smaller than yhat's own last bit (yhat = 1 - 1e-7: no fp32 yhat is closer than
    3e-8), so there the bound is taken with |ref| = max(yhat, 1 - yhat): yhat's error at its own bound, plus the
    rounding of the subtraction and of the scaling, each half an ulp of |yhat - 1|."""
    ref = np.where(onehot > 0, np.maximum(yh, 1.0 - yh), yh)
    return (gap + 8.0) * eps * ref + floor


def loss_bound(loss_cols):
    """The bound of the fp32 loss partial of every 16-column block: sum over its columns of (l + 4) 2^-22."""
    b = (np.asarray(loss_cols) + 4.0) * 2.0 ** -22
    return np.array([b[k:k + 16].sum() for k in range(0, len(b), 16)])


def block_sums(v):
    return np.array([v[k:k + 16].sum() for k in range(0, len(v), 16)])


def block_sums32(v):
    """The same sums added left to right in fp32."""
    out = []
    for k in range(0, len(v), 16):
        s = np.float32(0)
        for t in v[k:k + 16]:
            s = np.float32(s + np.float32(t))
        out.append(s)
    return np.array(out, np.float64)


def worst_ratio(got, ref, bound):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):  # (a zero bound -- fp64 at an exact 0 -- admits only err = 0)
        return float(np.where(err == 0, 0.0, err / bound).max())


# the sigmoid ladder: pre-activations b1[h] (W1 = 0), both signs
SIG_LADDER = (0.0, 0.5, 1.0, 8.0, 17.0, 40.0, 87.0, 88.0, 89.0, 104.0, 128.0, 8192.0, 3e38)


def sigmoid_ladder(H):
    """b1 [H]: the ladder with both signs, repeated over the rows."""
    vals = [0.0] + [s * v for v in SIG_LADDER[1:] for s in (1.0, -1.0)]
    return np.array([vals[h % len(vals)] for h in range(H)])


def sigmoid_reference(x):
    """fp64 sigmoid without overflow: exactly 1 / 0 at the ends as the fp64 value rounds."""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))
