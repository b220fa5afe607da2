"""The XCD-local step pipeline's dW1 tiles reading their pixel operand from the forward's fragment-ordered copy
(csrc/mlp/xstep.hip PIX, csrc/mlp/mma_tile.h BLDS: 16-byte loads of the blocks the XCD's L2 already holds, a
wave-private LDS image, ds_read_b64_tr_b8 column reads) instead of the feature-major copy: the MFMA operands are the
same registers, so the parameters stay BITWISE those of the two-launch step, which keeps reading the feature-major
copy.  Shapes: the smallest fragment-ordered batch (17 sample tiles, most dW1 waves without a K range), an odd chunk
count (a half pair in the tail), the largest batch the pipeline takes, fewer row tiles than XCDs."""
import pytest
import torch

from cme213_sp18_amd.models.mlp import NeuralNetwork
from cme213_sp18_amd.parallel.engine import MlpEngine
from cme213_sp18_amd.utils.data import synthetic_mnist

pytestmark = pytest.mark.gpu

LR, REG = 0.05, 1e-4
SHAPES = [(100, 272), (100, 304), (128, 960), (64, 400)]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _pair(H, n, N, seed, pix, b1_zero=False):
    """[0] the two-launch step (xstep = 0), [1] the pipeline with the dW1 pixel operand's form `pix`."""
    x, y = synthetic_mnist(N, seed=seed)
    nn = NeuralNetwork([784, H, 10])
    params = list(nn.params)
    if b1_zero:
        params[1] = params[1] * 0
    out = []
    for xs in (0, -1):
        e = MlpEngine(nn.H, "f32", max_cols=n, device="cuda", path="split3")
        e.set_params(*params)
        e.load_dataset(x, y)
        e.set_store_a1(False)
        st = e._hip_step()
        st.xstep, st.head_dw2, st.xstep_pix = xs, 1, pix
        out.append(e)
    return out


def _plan(e, g0, count, n, N):
    e._hip_step().run_steps(g0, count, n, 0, n, N, 1.0 / n, REG, LR, 1, _stream())


def _both(engines, fn, pipeline=True):
    for e in engines:
        fn(e)
    torch.cuda.synchronize()
    assert torch.equal(engines[0].params, engines[1].params)
    if pipeline:
        st = engines[1]._hip_step()
        assert st.xstep_used == 1, st.xstep_reason
        assert st.dz_left_swz == 1  # (the fragment-ordered form, not the row-major one)
        assert engines[0]._hip_step().xstep_used == 0
    for e in engines:
        assert not e.kernel_error()


@pytest.mark.parametrize("H,n", SHAPES)
def test_pixels_from_the_forwards_copy_are_bitwise_the_two_launch_step(H, n):
    """Two epochs as one plan (with the wrap to sample 0), a plan from sample 48 (a sample tile that starts no
    64-sample pair), a two-launch step, a plan again: parameters bitwise equal throughout."""
    N = 5 * n + 48
    engines = _pair(H, n, N, seed=H + n, pix=1)
    _both(engines, lambda e: _plan(e, 0, 2 * (N // n), n, N))
    _both(engines, lambda e: _plan(e, 16 * 3, 3, n, N))
    _both(engines, lambda e: e.run(16, n, 1.0 / n, REG, LR, sgd=True), pipeline=False)
    _both(engines, lambda e: _plan(e, 2 * n, 4, n, N))
    assert torch.equal(engines[0].dz1()[:, :n], engines[1].dz1()[:, :n])


def test_both_pixel_forms_give_the_same_bits():
    """MlpStep.xstep_pix 0 (the feature-major copy) and 1 at (100, 272): the same bits, over launches that alternate
    the control banks."""
    H, n = 100, 272
    N = 5 * n + 48
    x, y = synthetic_mnist(N, seed=5)
    nn = NeuralNetwork([784, H, 10])
    engines = []
    for pix in (0, 1):
        e = MlpEngine(nn.H, "f32", max_cols=n, device="cuda", path="split3")
        e.set_params(*nn.params)
        e.load_dataset(x, y)
        e.set_store_a1(False)
        e._hip_step().xstep_pix = pix
        engines.append(e)
    for g0, k in ((0, 2 * (N // n)), (48, 3), (n, 5)):
        for e in engines:
            _plan(e, g0, k, n, N)
        torch.cuda.synchronize()
        assert all(e._hip_step().xstep_used == 1 for e in engines), [e._hip_step().xstep_reason for e in engines]
        assert torch.equal(engines[0].params, engines[1].params)
    for e in engines:
        assert not e.kernel_error()


@pytest.mark.parametrize("H,n", SHAPES)
def test_bias_row_after_one_step_from_zero(H, n):
    """db1 is the dW1 GEMM's all-ones column, which the fragment-ordered copy does not have (it is synthesized in
    registers): after one step from b1 = 0, b1 is bitwise the two-launch step's (and not zero)."""
    N = 5 * n + 48
    engines = _pair(H, n, N, seed=H + n + 1, pix=1, b1_zero=True)
    assert float(engines[1].b1.abs().max()) == 0.0
    _both(engines, lambda e: _plan(e, 0, 1, n, N))
    assert torch.equal(engines[0].b1, engines[1].b1)
    assert float(engines[1].b1.abs().max()) > 0.0
