"""What the shuffle and the augmentation tests on the GPU (tests/test_gpu_shuffle.py, tests/test_gpu_augment.py) share:
an engine loaded with a given set, and the comparison of every resident layout of two engines."""
import torch

from cme213_sp18_amd.parallel import MlpEngine

LAYOUTS = ("X", "XT", "Xs", "Xw", "XTw", "labels")


def engine(path, dtype, H, x, y, keep=False):
    e = MlpEngine((x.shape[1], H, 10), dtype=dtype, max_cols=64, path=path)
    e.load_dataset(x, y, keep_source=keep)
    return e


def same_layouts(e, f, what):
    for name in LAYOUTS:
        a, b = getattr(e, name), getattr(f, name)
        assert (a is None) == (b is None), (what, name)
        if a is not None:  # (padding included: Xs's zeros and XT's ones row are part of the tensors)
            assert a.shape == b.shape and torch.equal(a, b), (what, name)
