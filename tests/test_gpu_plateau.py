"""Reduce the learning rate on a validation plateau on the GPU (csrc/mlp/plateau.hip, the scale word of the apply launch
in csrc/mlp/optim.hip, MlpEngine.set_plateau / enqueue_plateau, DataParallelTrainer(plateau=...)): the decision launch
bitwise against the header over scripted sequences from both input forms, graph replay against eager, the apply launch
with the scale word bitwise against the host evaluation of the headers, and the trainer against the torch backend's
decisions, against its own epoch-by-epoch twin, across calls, through a snapshot and on two ranks sharing the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cme213_sp18_amd._native import cpu, hip
from cme213_sp18_amd.optim import Optimizer, Plateau
from tests.plateau_oracle import (CONFIGS, EPOCHS, NAN, REG, SCRIPTS, assert_matches_twin, make_trainer, rule_for,
                                  run_twin, same_record, start)
from tests.sched_workers import RULES, rule_code

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 8  # sentinel words on either side of the record
LR = 0.05


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _f64bits(x: float) -> int:
    return int(np.float64(x).view(np.int64))


def _slot(n, correct, loss_sum):
    return torch.tensor([int(n), int(correct), _f64bits(loss_sum), 99, 98], dtype=torch.int64, device="cuda")


def _same(x, y):
    """Bitwise equal device tensors (a NaN norm in the last-update record compares equal to itself)."""
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8),
                                                                     y.contiguous().view(torch.uint8))


def _dev(a, offset=0):
    """The array on the device, `offset` elements past a fresh allocation (1: 16-byte misaligned)."""
    pad = np.zeros(offset, a.dtype)
    return torch.from_numpy(np.concatenate([pad, a])).cuda()[offset:]


# ------------------------------------------------------------------------------------------------ the decision launch
class Record:
    """One device record between sentinel words, and its host twin."""

    def __init__(self, rule: Plateau):
        self.rule = rule
        self.buf = torch.full((GUARD + 8 + GUARD,), -7.0, dtype=torch.float64, device="cuda")
        self.rec = self.buf[GUARD:GUARD + 8]
        self.hrec = np.asarray(start(rule.monitor))
        self.rec.copy_(torch.from_numpy(self.hrec))

    def launch(self, slot=None, rows=None):
        hip().mlp_plateau(*self.rule.native(), self.rec.data_ptr(), slot.data_ptr() if slot is not None else 0,
                          rows.data_ptr() if rows is not None else 0, int(rows.shape[0]) if rows is not None else 1,
                          _stream())

    def decide(self, triples, slot=None, rows=None):
        self.launch(slot, rows)
        self.hrec, reduced = cpu().plateau_decide(self.hrec, self.rule.native(),
                                                  np.asarray(triples, np.float64).reshape(-1, 3))
        self.check()
        return bool(reduced)

    def check(self):
        torch.cuda.synchronize()
        buf = self.buf.cpu().numpy()
        assert same_record(buf[GUARD:GUARD + 8], self.hrec), (buf[GUARD:GUARD + 8].tolist(), self.hrec.tolist())
        assert bool((buf[:GUARD] == -7.0).all()) and bool((buf[GUARD + 8:] == -7.0).all())


def _split(triple, R, k):
    """One triple as R rows whose rank-order sum is the triple's metric: counts split exactly, the loss in parts that
    do not add associatively for R = 3 (the reference is the header over the same rows)."""
    n, c, l = triple
    if R == 1:
        return [list(triple)]
    rows = [[float(n // R), float(c // R), l / R] for _ in range(R)]
    rows[0][0] += n - (n // R) * R
    rows[0][1] += c - (c // R) * R
    if R == 3 and k % 2:
        rows[0][2], rows[1][2], rows[2][2] = 1e16, l, -1e16  # (1e16 + l) - 1e16 != l
    return rows


RULES_SCRIPTED = {
    "nan_first": Plateau(factor=0.5, patience=1, threshold=0.0, threshold_mode="abs"),
    "tie": Plateau(factor=0.5, patience=1, threshold=0.0, threshold_mode="abs"),
    "patience_edge": Plateau(factor=0.1, patience=2, threshold=0.0, threshold_mode="abs"),
    "cooldown": Plateau(factor=0.5, patience=0, threshold=0.0, threshold_mode="abs", cooldown=2),
    "clamp": Plateau(factor=0.5, patience=0, threshold=0.0, threshold_mode="abs", cooldown=1, min_factor=0.2),
    "nan_inside": Plateau(factor=0.5, patience=1, threshold=0.125, threshold_mode="rel", cooldown=1),
    "improving": Plateau(factor=0.1, patience=0, threshold=0.5, threshold_mode="rel"),
}


@pytest.mark.parametrize("form", ["slot", "rows1", "rows2", "rows3"])
@pytest.mark.parametrize("monitor", ["loss", "accuracy"])
def test_decision_launch_is_bitwise_the_header_over_the_scripted_sequences(monitor, form):
    import dataclasses

    reductions = 0
    for name, seq in SCRIPTS.items():
        rule = dataclasses.replace(RULES_SCRIPTED[name], monitor=monitor)
        r = Record(rule)
        for k, m in enumerate(seq):
            v = m if monitor == "loss" else 4.0 - m
            # n = 8 samples; loss_sum = 8 v and correct = 8 v' with v' = v / 4 in [0, 1]: the metric is v (loss) or
            # v / 4 (accuracy), exact for the scripts' dyadic values; NaN: an empty set (0 / 0)
            triple = (0, 0, 0.0) if m != m else (8, int(2 * v), 8.0 * v)
            if form == "slot":
                reductions += r.decide([triple], slot=_slot(*triple))
            else:
                rows = _split(triple, int(form[-1]), k)
                reductions += r.decide(rows, rows=torch.tensor(rows, dtype=torch.float64, device="cuda"))
        assert r.hrec[0] == len(seq)
        if name == "clamp":
            assert r.hrec[4] == 0.2 and r.hrec[5] == 3.0
        if name == "nan_first":
            assert r.hrec[5] >= 1 and np.isfinite(r.hrec[1])
    assert reductions >= 10


def test_launcher_refuses_what_it_cannot_run():
    r = Record(Plateau(factor=0.5, patience=0))
    s = _slot(8, 1, 1.0)
    rows = torch.zeros(2, 3, dtype=torch.float64, device="cuda")
    m = hip()
    args = lambda **kw: {**dict(monitor=0, factor=0.5, patience=0, threshold=0.0, threshold_mode=0,  # noqa: E731
                                cooldown=0, min_factor=0.0, eps=0.0, rec=r.rec.data_ptr(), slot=s.data_ptr(), rows=0,
                                R=1, stream=_stream()), **kw}
    for bad in (dict(rec=0), dict(rec=r.rec.data_ptr() + 4), dict(slot=0), dict(rows=rows.data_ptr()),
                dict(slot=0, rows=rows.data_ptr(), R=0), dict(R=2), dict(monitor=2), dict(factor=0.0), dict(factor=1.0),
                dict(patience=-1), dict(threshold=-1.0), dict(threshold_mode=2), dict(cooldown=-1),
                dict(min_factor=1.5), dict(min_factor=-0.5), dict(eps=-1.0), dict(factor=NAN),
                dict(slot=0, rows=rows.data_ptr() + 4, R=2)):
        with pytest.raises(ValueError):
            m.mlp_plateau(**args(**bad))
    r.check()  # nothing was launched: the record is at its start


def test_graph_replays_advance_the_record_like_eager_launches():
    rule = Plateau(factor=0.5, patience=1, threshold=0.0, threshold_mode="abs", cooldown=1, min_factor=0.1)
    a, b, warm = Record(rule), Record(rule), Record(rule)
    slot = _slot(8, 1, 16.0)
    warm.launch(slot=slot)  # (the kernel loaded before the capture, on a record of its own)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a.launch(slot=slot)
    torch.cuda.synchronize()
    a.check()  # a capture runs nothing
    seq = SCRIPTS["clamp"] + SCRIPTS["tie"] + SCRIPTS["improving"]
    for m in seq:  # the slot is refilled in place: the graph holds its address
        slot.copy_(_slot(8, 1, 8.0 * m))
        g.replay()
        b.decide([(8, 1, 8.0 * m)], slot=slot)
        a.hrec = b.hrec
        a.check()
    assert b.hrec[0] == len(seq) and b.hrec[5] >= 3 and b.hrec[4] == 0.1
    assert _same(a.buf, b.buf)


# ------------------------------------------------------------------------------------------------ the apply launch
WINDOW = (1, np.array([0.5, 2.0, 0.125]))  # t0 = 1: launch 0 clamps below the window
SCALES = (1.0, 0.25, 0.3)  # no change, a power of two, a non-dyadic one


class Arena:
    """Device buffers of one apply-launch problem and their host twins (numpy, same dtype); `offset` = 1 starts every
    arena-sized buffer one element past its allocation (16-byte misaligned: the scalar path)."""

    def __init__(self, tdt, opt, count, w1n, np_, clip, window, offset, scale, seed=0):
        self.rng = np.random.default_rng(seed + count)
        self.ndt = np.float32 if tdt == torch.float32 else np.float64
        self.tdt, self.opt, self.count, self.w1n, self.np_, self.clip = tdt, opt, count, w1n, np_, float(clip)
        self.hp = self.rng.standard_normal(count).astype(self.ndt)
        self.hs = [np.zeros(count, self.ndt) for _ in range(opt.num_state)]
        self.t, self.b1p, self.b2p = 0, 1.0, 1.0
        self.p = _dev(self.hp, offset)
        self.g = _dev(np.zeros(count, self.ndt), offset)
        self.s = [_dev(s, offset) for s in self.hs]
        assert (self.p.data_ptr() % 16 != 0) == bool(offset)
        self.rec = torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float64).repeat(hip().optim_grid(count), 1).cuda()
        self.planes = torch.full((max(np_, 1), max(w1n, 1)), 7.0, dtype=torch.bfloat16, device="cuda")
        self.status = torch.zeros(1, dtype=tdt, device="cuda")
        self.last = torch.full((4,), -3.0, dtype=torch.float64, device="cuda")
        self.part = torch.zeros(64, dtype=torch.float64, device="cuda")
        self.hlast = None
        self.segs = [(0, count)] if count < 8 else [(0, count // 3), (count // 3, count - count // 3 - 1)]
        self.window = window
        self.win = None
        if window is not None:
            host = np.concatenate([[float(window[0]), float(len(window[1]))], window[1]])
            self.win = torch.zeros(2 + 8, dtype=torch.float64, device="cuda")
            self.win[:host.size].copy_(torch.from_numpy(host))
        # a whole plateau record (start values, the scale word set): the launch reads word plateau_scale_word alone
        self.scale = scale
        self.prec = None
        if scale is not None:
            h = np.asarray(start())
            h[hip().plateau_scale_word] = scale
            self.prec = torch.from_numpy(h).cuda()

    def grads(self):
        g = self.rng.standard_normal(self.count).astype(self.ndt)
        if self.count > 8:
            g[5] = 0.0
            g[7] = np.float32(1e-42) if self.ndt == np.float32 else 5e-320  # denormal
        return g

    def launch(self, lr=LR, default_plateau=False):
        o = self.opt
        dt = 0 if self.tdt == torch.float32 else 1
        npart = 0
        if self.clip > 0:
            npart = int(hip().clip_grid(sum(s for _, s in self.segs)))
            hip().grad_sumsq(dt, self.g.data_ptr(), self.count, self.segs, self.part.data_ptr(), npart, _stream())
        word = 0 if self.prec is None else self.prec.data_ptr() + 8 * int(hip().plateau_scale_word)
        tail = () if default_plateau else (word,)  # (the trailing argument left out: the call as it was)
        hip().optim_apply(dt, rule_code(o), *o.hyper(lr), self.p.data_ptr(), self.g.data_ptr(),
                          self.s[0].data_ptr() if self.s else 0, self.s[1].data_ptr() if len(self.s) > 1 else 0,
                          self.count, self.planes.data_ptr() if self.np_ else 0, self.np_,
                          self.w1n if self.np_ else 0, self.status.data_ptr(), self.rec.data_ptr(),
                          int(self.rec.shape[0]), self.win.data_ptr() if self.win is not None else 0,
                          int(self.win.numel()) - 2 if self.win is not None else 0,
                          self.part.data_ptr() if npart else 0, npart, self.clip, self.last.data_ptr(), _stream(),
                          *tail)

    def host_step(self, g, lr=LR):
        o = self.opt
        g = g.copy()
        lr_t = lr if self.window is None else cpu().window_rate(lr, self.window[0], self.window[1], self.t)
        if self.scale is not None:
            lr_t = cpu().plateau_rate(lr_t, self.scale)
        norm, coef = float("nan"), 1.0
        if self.clip > 0:
            norm, coef = cpu().grad_clip(g, self.segs, self.clip)
        self.hlast = np.array([float(self.t), lr_t, norm, coef])
        self.t, self.b1p, self.b2p = cpu().optim_step(rule_code(o), o.hyper(lr_t), self.hp, g,
                                                      self.hs[0] if self.hs else None,
                                                      self.hs[1] if len(self.hs) > 1 else None, self.t, self.b1p,
                                                      self.b2p)
        return lr_t

    def tensors(self):
        return (self.p, *self.s, self.rec, self.planes, self.last)

    def check(self, tag):
        torch.cuda.synchronize()
        assert np.array_equal(_bits(self.p.cpu().numpy()), _bits(self.hp)), (tag, "params")
        for i, (d, h) in enumerate(zip(self.s, self.hs)):
            assert np.array_equal(_bits(d.cpu().numpy()), _bits(h)), (tag, "state", i)
        rec = self.rec.cpu()
        want = torch.tensor([float(self.t), self.b1p, self.b2p, 0.0], dtype=torch.float64)
        assert torch.equal(rec, want.expand_as(rec)), (tag, "records")
        assert np.array_equal(_bits(self.last.cpu().numpy()), _bits(self.hlast)), (tag, "last", self.last, self.hlast)
        if self.prec is not None:  # the launch only reads the record
            h = np.asarray(start())
            h[hip().plateau_scale_word] = self.scale
            assert same_record(self.prec.cpu().numpy(), h), (tag, "plateau record")
        if self.np_ and self.w1n:
            pl = self.planes[:, :self.w1n].float()
            if self.np_ == 3:
                assert torch.equal((pl[0] + pl[1]) + pl[2], self.p[:self.w1n].float()), (tag, "planes")
            else:
                assert torch.equal(self.planes[0, :self.w1n], self.p[:self.w1n].to(torch.bfloat16)), (tag, "shadow")


W1NS = {7: 5, 1031: 523}  # (523: not a multiple of 4 -- the planes' element-by-element stores)


@pytest.mark.parametrize("count", [1031, 7])
@pytest.mark.parametrize("kind", list(RULES))
@pytest.mark.parametrize("tdt,np_", [(torch.float32, 3), (torch.float32, 1), (torch.float64, 0)])
def test_apply_launch_with_the_scale_word_is_bitwise_the_host_evaluation(tdt, np_, kind, count):
    """kSgd, Nesterov momentum and Adam, f32 (three planes / one shadow plane) and f64, 1031 elements (a vector body
    plus a scalar tail; two workgroups) and 7, aligned and misaligned, with and without a window and clipping, the scale
    1.0, a power of two and a non-dyadic one: three launches each against _cpu.optim_step at
    plateau_rate(window_rate(...), scale)."""
    opt, w1n = RULES[kind], W1NS[count]
    root = float(np.sqrt(count))
    for policy in (False, True):
        for offset in (0, 1):
            runs = {s: Arena(tdt, opt, count, w1n, np_, root / 4 if policy else 0.0, WINDOW if policy else None,
                             offset, s) for s in (None,) + SCALES}
            for k in range(3):
                g = runs[None].grads()
                rates = {}
                for s, a in runs.items():
                    a.g.copy_(torch.from_numpy(g))
                    a.launch()
                    rates[s] = a.host_step(g)
                    a.check((policy, offset, s, k))
                f = (0.5, 0.5, 2.0)[k] if policy else 1.0
                assert rates[None] == LR * f and rates[0.25] == LR * f * 0.25 and rates[0.3] == (LR * f) * 0.3
                # the scale 1.0 is bitwise the launch without the pointer
                for x, y in zip(runs[None].tensors(), runs[1.0].tensors()):
                    assert _same(x, y), ("scale 1.0", policy, offset, k)
                assert not torch.equal(runs[None].p, runs[0.3].p)
            assert runs[0.3].t == 3


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_null_pointer_is_the_call_as_it_was_and_nonzero_status_changes_nothing(kind):
    opt = RULES[kind]
    a, b, c = (Arena(torch.float32, opt, 1031, 523, 3, 5.0, WINDOW, 0, s) for s in (None, None, 0.3))
    g = a.grads()
    for x in (a, b, c):
        x.g.copy_(torch.from_numpy(g))
    for k in range(2):
        a.launch()                       # plateau = 0, passed explicitly
        b.launch(default_plateau=True)   # the trailing argument left out: every existing call
        a.host_step(g)
        b.host_step(g)
        a.check(k)
        b.check(k)
        for x, y in zip(a.tensors(), b.tensors()):
            assert _same(x, y)
    c.launch()
    c.host_step(g)
    c.check("before")
    held = [t.clone() for t in c.tensors()] + [c.prec.clone()]
    for bad in (1.0, float("nan")):
        c.status.fill_(bad)
        c.launch()
        torch.cuda.synchronize()
        for t, h in zip(c.tensors() + (c.prec,), held):
            assert bool((t.view(torch.uint8) == h.view(torch.uint8)).all()), bad
    c.status.zero_()
    c.launch()
    c.host_step(g)
    c.check("after")
    assert c.t == 2
    with pytest.raises(ValueError):  # a misaligned scale word
        hip().optim_apply(0, 2, *Optimizer.sgd().hyper(0.1), a.p.data_ptr(), a.g.data_ptr(), 0, 0, 1031,
                          rec=a.rec.data_ptr(), nrec=int(a.rec.shape[0]), plateau=c.prec.data_ptr() + 4)


def test_graph_replays_read_the_scale_the_decision_launch_left():
    """One graph of {decision launch, apply launch}: every replay decides from the slot's current content and the
    update behind it uses the scale that decision left."""
    rule = Plateau(factor=0.5, patience=0, threshold=0.0, threshold_mode="abs")
    r, warm = Record(rule), Record(rule)
    a = Arena(torch.float32, RULES["nesterov"], 1031, 523, 3, 0.0, None, 0, 1.0)
    w = Arena(torch.float32, RULES["nesterov"], 1031, 523, 3, 0.0, None, 0, 1.0)
    a.prec = r.rec  # the apply launch reads the live record
    g = a.grads()
    a.g.copy_(torch.from_numpy(g))
    slot = _slot(8, 1, 16.0)
    warm.launch(slot=slot)
    w.launch()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r.launch(slot=slot)
        a.launch()
    torch.cuda.synchronize()
    scales = []
    for m in (2.0, 3.0, 1.0, 1.0, 4.0):  # improve, bad (0.5), improve, tie (0.25), bad (0.125)
        slot.copy_(_slot(8, 1, 8.0 * m))
        graph.replay()
        r.hrec, _ = cpu().plateau_decide(r.hrec, rule.native(), np.array([[8.0, 1.0, 8.0 * m]]))
        r.check()
        a.scale = float(r.hrec[4])
        scales.append(a.scale)
        a.host_step(g)
        prec, a.prec = a.prec, None  # (check()'s record comparison is for the start record; r.check() covered it)
        a.check(m)
        a.prec = prec
    assert scales == [1.0, 0.5, 0.5, 0.25, 0.125] and a.hlast[1] == LR * 0.125


# ------------------------------------------------------------------------------------------------ trainer
def _hip_trainer(name, dtype, H, executor="graph", rule=None, **over):
    kw, _, _ = CONFIGS[name]
    return make_trainer(rule, dtype=dtype, H=H, device="cuda", backend="hip", use_graphs=True, executor=executor,
                        **{**kw, **over})


def _sure(name):
    """Threshold 0.5 with patience 0: an evaluation that does not halve the best loss reduces the rate."""
    return rule_for(name, threshold=0.5)


SHAPES = {"f32": 100, "bf16": 100, "f64": 16}
_TWINS: dict = {}


def _twin(name, dtype, rule):
    key = (name, dtype, rule.threshold)
    if key not in _TWINS:  # computed once, shared, left unchanged
        _TWINS[key] = run_twin(name, rule, dtype=dtype, H=SHAPES[dtype], device="cuda", backend="hip",
                               use_graphs=True, executor="eager")
        print("TWIN", key, _TWINS[key]["scales"], [round(m, 5) for m in _TWINS[key]["metrics"]], _TWINS[key]["rec"])
    return _TWINS[key]


@pytest.mark.parametrize("executor", ["graph", "eager"])
@pytest.mark.parametrize("name,dtype", [("sgd", "f32"), ("momentum", "f32"), ("adam", "f32"), ("sgd", "bf16"),
                                        ("momentum", "bf16"), ("sgd", "f64"), ("adam", "f64")])
def test_hip_trainer_equals_its_epoch_by_epoch_twin(name, dtype, executor):
    """784-100-10 (f32, bf16) and 784-16-10 (f64), 512 / 256 samples, batch 128, 6 epochs evaluated after each, factor
    0.5, patience 0, threshold 0.5: against the twin on the same backend (no rule, one epoch at a time at lr * scale,
    torch's scheduler deciding on the host), bitwise in parameters and record."""
    rule = _sure(name)
    twin = _twin(name, dtype, rule)
    assert twin["rec"][5] >= 2 and twin["records"][0][1] == twin["metrics"][0]  # reduced; an evaluation improved
    _, lr, _ = CONFIGS[name]
    tr = _hip_trainer(name, dtype, SHAPES[dtype], executor, rule)
    st = tr.train(EPOCHS, lr, REG, eval_every=1)
    assert_matches_twin(tr, twin)
    assert st.plateau["reductions"] == int(twin["rec"][5]) and st.plateau["scale"] == twin["rec"][4]
    assert [e["loss"] for e in st.evals] == twin["metrics"]
    got, ref = tr.engine.optim_state(), twin["optim"]
    assert got["t"] == ref["t"] == 4 * EPOCHS
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got["state"], ref["state"]))
    sched = CONFIGS[name][0].get("schedule")
    f = sched.factor(4 * EPOCHS - 1, 4) if sched is not None else 1.0
    assert tr.engine.last_update()["lr"] == (lr * f) * twin["scales"][-1]
    assert tr.native_plan(tr.epoch_plan()) is None
    if name == "sgd":
        assert "plateau" in tr.native_reason and "plateau" in tr.engine._hip_step().xstep_reason


@pytest.mark.parametrize("name", list(CONFIGS))
def test_hip_f64_with_later_improvements_equals_its_twin_and_two_plus_two_equals_four(name):
    """The configurations' own thresholds (3 %, 10 %, 2 %: reductions AND later improvements on the fp64 trajectory)
    on the graph executor, as train(2) + train(2) + train(2)."""
    rule = rule_for(name)
    twin = _twin(name, "f64", rule)
    best = [r[1] for r in twin["records"]]
    assert twin["rec"][5] >= 2 and any(b < a for a, b in zip(best, best[1:])), twin["records"]
    _, lr, _ = CONFIGS[name]
    tr = _hip_trainer(name, "f64", 16, "graph", rule)
    for done in (2, 4, 6):
        st = tr.train(2, lr, REG, eval_every=1)
        assert st.plateau["evals"] == done
        assert_matches_twin(tr, twin, done)
    whole = _hip_trainer(name, "f64", 16, "graph", rule)
    whole.train(4, lr, REG, eval_every=1)
    assert_matches_twin(whole, twin, 4)


@pytest.mark.parametrize("name,dtype", [("sgd", "f32"), ("adam", "f32"), ("sgd", "bf16"), ("adam", "bf16"),
                                        ("sgd", "f64"), ("momentum", "f64"), ("adam", "f64")])
def test_hip_trainer_takes_the_torch_backends_decisions(name, dtype):
    """The same run on the torch backend (CPU, the same dtype): every decision equal -- evals, bad, cooldown_left, scale,
    reductions, last_reduced_index.  The two backends sum in different orders, so the metrics differ in their last
    places (bf16: by the rounding of the operands, 2^-9 relative each); the reference's own decisions must therefore be
    clear of their thresholds by 5 % of the metric, ten times that and more, which is asserted on the reference alone
    (momentum at 784-100-10 comes within 1 % of halving its loss and is left to the fp64 case)."""
    rule = _sure(name)
    kw, lr, _ = CONFIGS[name]
    ref = make_trainer(rule, dtype=dtype, H=SHAPES[dtype], **kw)
    sr = ref.train(EPOCHS, lr, REG, eval_every=1)
    best, clear = float("inf"), []
    for e in sr.evals:
        if best != float("inf"):
            clear.append(abs(e["loss"] - best * 0.5) / e["loss"])
        best = e["loss"] if e["loss"] < best * 0.5 else best
    print("REFERENCE", name, dtype, [round(e["loss"], 5) for e in sr.evals], [round(c, 3) for c in clear], sr.plateau)
    assert min(clear) >= 0.05 and sr.plateau["reductions"] >= 2
    tr = _hip_trainer(name, dtype, SHAPES[dtype], "graph", rule)
    st = tr.train(EPOCHS, lr, REG, eval_every=1)
    print("HIP", [round(e["loss"], 5) for e in st.evals], st.plateau)
    for k in ("evals", "bad", "cooldown_left", "scale", "reductions", "last_reduced_index"):
        assert st.plateau[k] == sr.plateau[k], (k, st.plateau, sr.plateau)
    assert abs(st.plateau["best"] - sr.plateau["best"]) <= 0.05 * sr.plateau["best"]


def test_hip_snapshot_restore_repeats_the_rates_and_nothing_is_allocated_without_a_rule():
    name, dtype = "momentum", "f32"
    rule = _sure(name)
    twin = _twin(name, dtype, rule)
    _, lr, _ = CONFIGS[name]
    tr = _hip_trainer(name, dtype, 100, "graph", rule)
    tr.train(3, lr, REG, eval_every=1)
    snap, it = tr._snapshot(), tr.iter
    rec, params = tr.engine.plateau_record(), tr.engine.params.clone()
    tr.train(3, lr, REG, eval_every=1)
    assert_matches_twin(tr, twin, 6)
    assert not same_record(tr.engine.plateau_record(), rec)
    tr._restore(snap)
    tr.iter = it
    torch.cuda.synchronize()
    assert same_record(tr.engine.plateau_record(), rec) and torch.equal(tr.engine.params, params)
    tr.train(3, lr, REG, eval_every=1)  # the recovered epochs repeat their rates
    assert_matches_twin(tr, twin, 6)
    # without the feature nothing is allocated and a snapshot is what it was
    plain = _hip_trainer(name, dtype, 100, "graph", None)
    st = plain.train(1, lr, REG, eval_every=1)
    assert plain.engine._plateau is None and st.plateau is None and len(plain._snapshot()) == 5
    bare = _hip_trainer("sgd", dtype, 100, "graph", None)
    assert bare.engine.opt_rec is None and bare.engine.opt_last is None and not bare.engine.uses_apply_launch


def test_hip_keep_best_and_ema_together_with_the_rule():
    from cme213_sp18_amd.optim import Ema

    name, dtype = "momentum", "f32"
    rule = _sure(name)
    twin = _twin(name, dtype, rule)
    _, lr, _ = CONFIGS[name]
    tr = _hip_trainer(name, dtype, 100, "graph", rule, ema=Ema(0.9))
    st = tr.train(EPOCHS, lr, REG, eval_every=1, keep_best="loss", eval_weights="current")
    assert_matches_twin(tr, twin)
    assert st.best["metric"] == min(twin["metrics"]) and tr.engine.ema_count() == 4 * EPOCHS
    assert st.plateau["last_metric"] == tr.engine.best_state()["last_metric"]


# ------------------------------------------------------------------------------------------------ two ranks, one GPU
@pytest.mark.parametrize("mode,keep_best", [("rccl", False), ("rccl", True), ("host", False)])
def test_two_ranks_sharing_the_gpu_decide_like_one_process(tmp_path, mode, keep_best):
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.plateau_workers import gpu_shared_plateau_main; " \
           f"gpu_shared_plateau_main({str(tmp_path)!r}, {mode!r}, {keep_best!r})"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    from tests.plateau_workers import EPOCHS as E2
    z = [dict(np.load(tmp_path / f"plateau_{mode}_{int(keep_best)}_{rank}.npz")) for rank in range(2)]
    assert [int(z[r]["shard"]) for r in range(2)] == [127, 128]
    rule = _sure("sgd")
    rec = np.asarray(start())
    for k in range(E2):  # the header over the gathered triples, in rank order
        rows = np.stack([z[0]["triples"][k], z[1]["triples"][k]])
        rec, _ = cpu().plateau_decide(rec, rule.native(), rows)
        for rank in range(2):
            assert same_record(z[rank]["recs"][k], rec), (mode, k, rank)
    print("RECORD", mode, keep_best, rec.tolist(), str(z[0]["impl"]))
    assert rec[5] >= 2
    for rank in range(2):
        assert float(z[rank]["agree"]) == 1.0
        assert same_record(z[rank]["rows"], np.stack([z[0]["triples"][-1], z[1]["triples"][-1]]))
        assert z[rank]["last"][1] == CONFIGS["sgd"][1] * float(z[rank]["recs"][E2 - 2][4])  # the last epoch's rate
    for k in ("params", "recs", "last"):
        assert np.array_equal(z[0][k].view(np.uint8), z[1][k].view(np.uint8)), (mode, k)
    # ... and one process takes the same decisions (the metrics differ in their last places: another summation order;
    # with threshold 0.5 every comparison is clear of its threshold by a third of the metric)
    one = _hip_trainer("sgd", "f32", 100, "graph", rule, nval=255)
    st = one.train(E2, CONFIGS["sgd"][1], REG, eval_every=1)
    for j, k in ((0, "evals"), (2, "bad"), (3, "cooldown_left"), (4, "scale"), (5, "reductions"),
                 (7, "last_reduced_index")):
        assert st.plateau[k] == rec[j], (k, st.plateau, rec.tolist())
    assert abs(st.plateau["best"] - rec[1]) <= 1e-3 * rec[1]
