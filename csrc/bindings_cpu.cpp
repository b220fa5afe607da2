// pybind11 bindings for the native CPU runtime (module cme213_sp18_amd._cpu).
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <omp.h>

#include <cstring>

#include "cpu/io.h"
#include "cpu/mlp_cpu.h"
#include "cpu/suite_cpu.h"
#include "mlp/affine.h"
#include "mlp/augment.h"
#include "mlp/best.h"
#include "mlp/plateau.h"
#include "mlp/clip.h"
#include "mlp/ema.h"
#include "mlp/sample.h"
#include "mlp/shuffle.h"
#include "mlp/warp.h"

namespace py = pybind11;
using f64arr = py::array_t<double, py::array::c_style | py::array::forcecast>;
using i32arr = py::array_t<int32_t, py::array::c_style | py::array::forcecast>;
using u32arr = py::array_t<uint32_t, py::array::c_style | py::array::forcecast>;

namespace {

double* mut(py::array_t<double>& a) {
  if (!(a.flags() & py::array::c_style)) throw std::invalid_argument("expected C-contiguous float64 array");
  return a.mutable_data();
}

cme::cpu::NetView view(py::array_t<double>& W1, py::array_t<double>& b1, py::array_t<double>& W2,
                       py::array_t<double>& b2) {
  if (W1.ndim() != 2 || W2.ndim() != 2) throw std::invalid_argument("W1, W2 must be 2-D");
  cme::cpu::NetView v{(int)W1.shape(1), (int)W1.shape(0), (int)W2.shape(0), mut(W1), mut(b1), mut(W2), mut(b2)};
  if (W2.shape(1) != v.H || b1.size() != v.H || b2.size() != v.C) throw std::invalid_argument("param shape mismatch");
  return v;
}

// (lr, mu, nesterov, beta1, beta2, eps) -> the update rules' hyper-parameters (mlp/optim.h)
cme::OptimHyper hyper_of(py::handle h) {
  const py::tuple t = h.cast<py::tuple>();
  if (t.size() != 6) throw std::invalid_argument("hyper = (lr, mu, nesterov, beta1, beta2, eps)");
  cme::OptimHyper o;
  o.lr = t[0].cast<double>(); o.mu = t[1].cast<double>(); o.nesterov = t[2].cast<bool>() ? 1 : 0;
  o.beta1 = t[3].cast<double>(); o.beta2 = t[4].cast<double>(); o.eps = t[5].cast<double>();
  return o;
}

// [(offset, size), ...] -> the segments of clip.h, each inside an array of `len` elements
cme::ClipSegs segs_of(const std::vector<std::pair<int64_t, int64_t>>& segments, int64_t len) {
  if (segments.empty() || segments.size() > cme::kClipMaxSegs)
    throw std::invalid_argument("1 .. 4 (offset, size) segments expected");
  cme::ClipSegs s;
  s.n = (int)segments.size();
  for (int i = 0; i < s.n; ++i) {
    s.off[i] = segments[i].first;
    s.size[i] = segments[i].second;
    if (s.off[i] < 0 || s.size[i] < 0 || s.off[i] > len || s.size[i] > len - s.off[i])
      throw std::invalid_argument("a segment lies outside the array");
  }
  return s;
}

// the sum of squares of a float32 / float64 array's segments in clip.h's order: (partials, sumsq)
std::pair<py::array_t<double>, double> sumsq_of(const py::array& g, const cme::ClipSegs& s) {
  if (!(g.flags() & py::array::c_style)) throw std::invalid_argument("a C-contiguous array expected");
  py::array_t<double> partials(cme::clip_grid(s.count()));
  double total;
  if (g.dtype().is(py::dtype::of<float>()))
    total = cme::clip_host_sumsq(static_cast<const float*>(g.data()), s, partials.mutable_data());
  else if (g.dtype().is(py::dtype::of<double>()))
    total = cme::clip_host_sumsq(static_cast<const double*>(g.data()), s, partials.mutable_data());
  else
    throw std::invalid_argument("float32 or float64 array expected");
  return {partials, total};
}

void check_x(const f64arr& X, int P) {
  if (X.ndim() != 2 || X.shape(1) != P) throw std::invalid_argument("X must be [n][P] float64");
}

}  // namespace

PYBIND11_MODULE(_cpu, m) {
  m.doc() = "cme213_sp18_amd native CPU runtime (fp64 oracle trainer, IDX/raw_ascii I/O, OpenMP suite)";

  m.def("omp_max_threads", []() { return omp_get_max_threads(); });

  m.def("init_params", [](py::array_t<double> W1, py::array_t<double> b1, py::array_t<double> W2,
                          py::array_t<double> b2) { cme::cpu::init_params(view(W1, b1, W2, b2)); });

  m.def(
      "feedforward",
      [](py::array_t<double> W1, py::array_t<double> b1, py::array_t<double> W2, py::array_t<double> b2, f64arr X,
         bool shift) {
        auto v = view(W1, b1, W2, b2);
        check_x(X, v.P);
        const int n = (int)X.shape(0);
        py::array_t<double> a1({n, v.H}), yc({n, v.C});
        {
          py::gil_scoped_release r;
          cme::cpu::feedforward(v, X.data(), n, a1.mutable_data(), yc.mutable_data(), shift);
        }
        return py::make_tuple(a1, yc);
      },
      py::arg("W1"), py::arg("b1"), py::arg("W2"), py::arg("b2"), py::arg("X"), py::arg("shift") = true);

  m.def(
      "backprop",
      [](py::array_t<double> W1, py::array_t<double> b1, py::array_t<double> W2, py::array_t<double> b2, f64arr X,
         i32arr labels, double reg, f64arr a1, f64arr yc, double scale) {
        auto v = view(W1, b1, W2, b2);
        check_x(X, v.P);
        const int n = (int)X.shape(0);
        py::array_t<double> dW1({v.H, v.P}), db1(v.H), dW2({v.C, v.H}), db2(v.C);
        {
          py::gil_scoped_release r;
          cme::cpu::backprop(v, X.data(), labels.data(), n, reg, a1.data(), yc.data(), scale, dW1.mutable_data(),
                             db1.mutable_data(), dW2.mutable_data(), db2.mutable_data());
        }
        return py::make_tuple(dW1, db1, dW2, db2);
      });

  m.def("loss", [](py::array_t<double> W1, py::array_t<double> b1, py::array_t<double> W2, py::array_t<double> b2,
                   f64arr yc, i32arr labels, double reg) {
    auto v = view(W1, b1, W2, b2);
    return cme::cpu::loss(v, yc.data(), labels.data(), (int)labels.size(), reg);
  });

  m.def(
      "predict",
      [](py::array_t<double> W1, py::array_t<double> b1, py::array_t<double> W2, py::array_t<double> b2, f64arr X,
         bool shift) {
        auto v = view(W1, b1, W2, b2);
        check_x(X, v.P);
        const int n = (int)X.shape(0);
        py::array_t<int32_t> out(n);
        {
          py::gil_scoped_release r;
          cme::cpu::predict(v, X.data(), n, out.mutable_data(), shift);
        }
        return out;
      },
      py::arg("W1"), py::arg("b1"), py::arg("W2"), py::arg("b2"), py::arg("X"), py::arg("shift") = true);

  m.def(
      "numgrad",
      [](py::array_t<double> W1, py::array_t<double> b1, py::array_t<double> W2, py::array_t<double> b2, f64arr X,
         i32arr labels, double reg, bool shift) {
        auto v = view(W1, b1, W2, b2);
        check_x(X, v.P);
        py::array_t<double> dW1({v.H, v.P}), db1(v.H), dW2({v.C, v.H}), db2(v.C);
        cme::cpu::numgrad(v, X.data(), labels.data(), (int)X.shape(0), reg, dW1.mutable_data(), db1.mutable_data(),
                          dW2.mutable_data(), db2.mutable_data(), shift);
        return py::make_tuple(dW1, db1, dW2, db2);
      },
      py::arg("W1"), py::arg("b1"), py::arg("W2"), py::arg("b2"), py::arg("X"), py::arg("labels"),
      py::arg("reg"), py::arg("shift") = true);

  m.def(
      "train",
      [](py::array_t<double> W1, py::array_t<double> b1, py::array_t<double> W2, py::array_t<double> b2, f64arr X,
         i32arr labels, double lr, double reg, int epochs, int batch, int print_every, bool debug,
         std::string outdir, bool shift, int ckpt_precision, int iter0, py::object optim, py::object rates,
         double clip_norm, py::object update_log, py::object ema) {
        auto v = view(W1, b1, W2, b2);
        check_x(X, v.P);
        cme::cpu::TrainOpts o;
        o.lr = lr; o.reg = reg; o.epochs = epochs; o.batch = batch; o.print_every = print_every;
        o.debug = debug; o.outdir = outdir; o.shift = shift; o.ckpt_precision = ckpt_precision; o.iter0 = iter0;
        // optim: None, or (kind, hyper, s1, s2 | None, counter): the state arrays (float64, H P + H + C H + C) and
        // the counter array {t, b1^t, b2^t} are updated in place; kind 2 (plain SGD under a schedule or clipping: the
        // kSgd rule) has no state, s1 = s2 = None
        // rates: None or the float64 rate of every update of the call; clip_norm: 0 = no clipping; update_log: None
        // or a list that gets one (t, rate, grad_norm, clip_coef) per update
        cme::OptimCounter ctr;
        py::array_t<double> counter;
        if (!optim.is_none()) {
          const py::tuple t = optim.cast<py::tuple>();
          if (t.size() != 5) throw std::invalid_argument("train: optim = (kind, hyper, s1, s2, counter)");
          o.optim_kind = t[0].cast<int>();
          o.hyper = hyper_of(t[1]);
          const int64_t total = (int64_t)v.H * v.P + v.H + (int64_t)v.C * v.H + v.C;
          auto state = [&](py::handle h) {
            if (!py::isinstance<py::array_t<double>>(h)) throw std::invalid_argument("train: float64 state expected");
            auto a = h.cast<py::array_t<double>>();
            if (a.size() != total) throw std::invalid_argument("train: optimizer state must hold every parameter");
            return mut(a);
          };
          if (o.optim_kind == cme::kSgd) o.optim_kind = -1;
          else o.s1 = state(t[2]);
          if (!t[3].is_none()) o.s2 = state(t[3]);
          if (!py::isinstance<py::array_t<double>>(t[4])) throw std::invalid_argument("train: float64 counter expected");
          counter = t[4].cast<py::array_t<double>>();
          if (counter.size() < 3) throw std::invalid_argument("train: the counter holds {t, b1^t, b2^t}");
          const double* c = mut(counter);
          ctr = {c[0], c[1], c[2]};
          o.counter = &ctr;
        }
        f64arr rate_table;
        if (!rates.is_none()) {
          rate_table = rates.cast<f64arr>();
          o.rates = rate_table.data();
          o.nrates = rate_table.size();
        }
        o.clip_norm = clip_norm;
        std::vector<double> ulog;
        if (!update_log.is_none()) o.update_log = &ulog;
        // ema: None, or (decay, warmup, average, count): the average (float64, H P + H + C H + C, [W1|b1|W2|b2]) and the
        // one-element float64 count of averaged updates are updated in place (csrc/mlp/ema.h)
        py::array_t<double> ema_avg, ema_cnt;
        if (!ema.is_none()) {
          const py::tuple t = ema.cast<py::tuple>();
          if (t.size() != 4) throw std::invalid_argument("train: ema = (decay, warmup, average, count)");
          o.ema_rule.decay = t[0].cast<double>();
          o.ema_rule.warmup = t[1].cast<bool>() ? 1 : 0;
          if (!py::isinstance<py::array_t<double>>(t[2]) || !py::isinstance<py::array_t<double>>(t[3]))
            throw std::invalid_argument("train: a float64 average and count expected");
          ema_avg = t[2].cast<py::array_t<double>>();
          ema_cnt = t[3].cast<py::array_t<double>>();
          const int64_t total = (int64_t)v.H * v.P + v.H + (int64_t)v.C * v.H + v.C;
          if (ema_avg.size() != total || ema_cnt.size() < 1)
            throw std::invalid_argument("train: the average must hold every parameter, the count one double");
          o.ema = mut(ema_avg);
          o.ema_t = mut(ema_cnt);
        }
        std::vector<double> losses;
        {
          py::gil_scoped_release r;
          losses = cme::cpu::train(v, X.data(), labels.data(), (int)X.shape(0), o);
        }
        if (!update_log.is_none()) {
          py::list out = update_log.cast<py::list>();
          for (size_t i = 0; i + 4 <= ulog.size(); i += 4)
            out.append(py::make_tuple((int64_t)ulog[i], ulog[i + 1], ulog[i + 2], ulog[i + 3]));
        }
        if (o.counter) {
          double* c = mut(counter);
          c[0] = ctr.t; c[1] = ctr.b1p; c[2] = ctr.b2p;
        }
        return losses;
      },
      py::arg("W1"), py::arg("b1"), py::arg("W2"), py::arg("b2"), py::arg("X"), py::arg("labels"), py::arg("lr"),
      py::arg("reg"), py::arg("epochs"), py::arg("batch"), py::arg("print_every") = 0, py::arg("debug") = false,
      py::arg("outdir") = "Outputs", py::arg("shift") = true, py::arg("ckpt_precision") = 12,
      py::arg("iter0") = 0, py::arg("optim") = py::none(), py::arg("rates") = py::none(), py::arg("clip_norm") = 0.0,
      py::arg("update_log") = py::none(), py::arg("ema") = py::none());

  // the exponential moving average of the parameters (csrc/mlp/ema.h, the header the kernel compiles) on float32 or
  // float64 arrays: ema_step folds params into ema in place as update t (0-based) and returns t + 1; ema_decay is the
  // decay d_t of that update.
  m.def(
      "ema_decay",
      [](double decay, bool warmup, int64_t t) {
        const cme::EmaRule r{decay, warmup ? 1 : 0};
        if (!cme::ema_rule_ok(r)) throw std::invalid_argument("ema_decay: decay must be in [0, 1)");
        if (t < 0) throw std::invalid_argument("ema_decay: t must be >= 0");
        return cme::ema_decay(r, (double)t);
      },
      py::arg("decay"), py::arg("warmup"), py::arg("t"));
  m.def(
      "ema_step",
      [](py::array ema, py::array params, double decay, bool warmup, int64_t t) {
        const cme::EmaRule r{decay, warmup ? 1 : 0};
        if (!cme::ema_rule_ok(r)) throw std::invalid_argument("ema_step: decay must be in [0, 1)");
        if (t < 0) throw std::invalid_argument("ema_step: t must be >= 0");
        const bool f32 = ema.dtype().is(py::dtype::of<float>());
        if (!f32 && !ema.dtype().is(py::dtype::of<double>()))
          throw std::invalid_argument("ema_step: float32 or float64 arrays expected");
        if (!params.dtype().is(ema.dtype()) || params.size() != ema.size() || !(ema.flags() & py::array::c_style) ||
            !(params.flags() & py::array::c_style) || !ema.writeable())
          throw std::invalid_argument("ema_step: arrays of one dtype and size, C-contiguous, a writable average expected");
        const double d = cme::ema_decay(r, (double)t);
        const py::ssize_t n = ema.size();
        auto run = [&](auto tag) {
          using T = decltype(tag);
          T* e = static_cast<T*>(ema.mutable_data());
          const T* p = static_cast<const T*>(params.data());
          const T omd = cme::ema_omd<T>(d);
          for (py::ssize_t i = 0; i < n; ++i) e[i] = cme::ema_update<T>(e[i], p[i], omd);
        };
        if (f32) run(float{});
        else run(double{});
        return t + 1;
      },
      py::arg("ema"), py::arg("params"), py::arg("decay"), py::arg("warmup"), py::arg("t"));

  // one update of the stateful rules (csrc/mlp/optim.h, the header the kernel compiles) on float32 or float64 arrays,
  // in place: kind 0 = momentum / Nesterov (s1 = v), 1 = adam (s1 = m, s2 = s), 2 = the stateless sgd rule (s1 = None:
  // what plain SGD runs under a schedule or clipping); hyper = (lr, mu, nesterov, beta1,
  // beta2, eps); t = the updates applied so far, b1p / b2p the running products b1^t, b2^t (None: formed by t
  // multiplications).  Returns the advanced (t, b1p, b2p).
  m.def(
      "optim_step",
      [](int kind, py::object hyper, py::array params, py::array grads, py::object s1, py::object s2, int64_t t,
         py::object b1p, py::object b2p) {
        const cme::OptimHyper h = hyper_of(hyper);
        if (kind != cme::kMomentum && kind != cme::kAdam && kind != cme::kSgd)
          throw std::invalid_argument("optim_step: kind 0, 1 or 2");
        cme::OptimCounter c;
        if (b1p.is_none() || b2p.is_none()) {
          for (int64_t i = 0; i < t; ++i) cme::optim_advance(c, h);
        } else {
          c = {(double)t, b1p.cast<double>(), b2p.cast<double>()};
        }
        cme::optim_advance(c, h);
        const bool f32 = params.dtype().is(py::dtype::of<float>());
        if (!f32 && !params.dtype().is(py::dtype::of<double>()))
          throw std::invalid_argument("optim_step: float32 or float64 arrays expected");
        std::vector<py::array> arrs = {params, grads};
        if (kind != cme::kSgd) {
          if (s1.is_none()) throw std::invalid_argument("optim_step: momentum and adam need s1");
          arrs.push_back(s1.cast<py::array>());
        }
        if (kind == cme::kAdam) {
          if (s2.is_none()) throw std::invalid_argument("optim_step: adam needs s2");
          arrs.push_back(s2.cast<py::array>());
        }
        const py::ssize_t n = params.size();
        for (size_t k = 0; k < arrs.size(); ++k) {
          const auto& a = arrs[k];
          if (!a.dtype().is(params.dtype()) || a.size() != n || !(a.flags() & py::array::c_style) ||
              (k != 1 && !a.writeable()))
            throw std::invalid_argument("optim_step: arrays of one dtype and size, C-contiguous and writable, expected");
        }
        auto run = [&](auto tag) {
          using T = decltype(tag);
          T* p = static_cast<T*>(arrs[0].mutable_data());
          const T* g = static_cast<const T*>(arrs[1].data());
          if (kind == cme::kSgd) {
            const auto k = cme::sgd_coef<T>(h);
            for (py::ssize_t i = 0; i < n; ++i) cme::sgd_update(p[i], g[i], k);
            return;
          }
          T* a = static_cast<T*>(arrs[2].mutable_data());
          if (kind == cme::kMomentum) {
            const auto k = cme::momentum_coef<T>(h);
            for (py::ssize_t i = 0; i < n; ++i) cme::momentum_update(p[i], a[i], g[i], k);
          } else {
            T* b = static_cast<T*>(arrs[3].mutable_data());
            const auto k = cme::adam_coef<T>(h, c);
            for (py::ssize_t i = 0; i < n; ++i) cme::adam_update(p[i], a[i], b[i], g[i], k);
          }
        };
        if (f32) run(float{});
        else run(double{});
        return py::make_tuple((int64_t)c.t, c.b1p, c.b2p);
      },
      py::arg("kind"), py::arg("hyper"), py::arg("params"), py::arg("grads"), py::arg("s1") = py::none(),
      py::arg("s2") = py::none(), py::arg("t") = 0, py::arg("b1p") = py::none(), py::arg("b2p") = py::none());

  // gradient-norm clipping on the host (csrc/mlp/clip.h, the header the kernels compile).  grad_sumsq: the partial
  // sums of squares of the segments [(offset, size), ...] of a float32 / float64 array, one per workgroup of the
  // kernel's grid, and the norm the apply launch forms from them.  grad_clip: scales the WHOLE array in place by
  // T(coef) when coef = clip_norm / (norm + 1e-6) < 1 (the apply launch scales every element it reads) and returns
  // (norm, coef).  window_rate: lr times the factor the apply launch reads for update t from the window (t0, factors).
  m.def("clip_grid", &cme::clip_grid, py::arg("count"));
  m.def(
      "grad_sumsq",
      [](py::array g, std::vector<std::pair<int64_t, int64_t>> segments) {
        auto r = sumsq_of(g, segs_of(segments, g.size()));
        return py::make_tuple(r.first, std::sqrt(r.second));
      },
      py::arg("g"), py::arg("segments"));
  m.def(
      "grad_clip",
      [](py::array g, std::vector<std::pair<int64_t, int64_t>> segments, double clip_norm) {
        if (!(clip_norm > 0.0)) throw std::invalid_argument("grad_clip: clip_norm must be > 0");
        if (!g.writeable()) throw std::invalid_argument("grad_clip: a writable array expected");
        const cme::ClipCoef c = cme::clip_coef(sumsq_of(g, segs_of(segments, g.size())).second, clip_norm);
        if (c.clipped) {
          const py::ssize_t n = g.size();
          if (g.dtype().is(py::dtype::of<float>())) {
            float* p = static_cast<float*>(g.mutable_data());
            for (py::ssize_t i = 0; i < n; ++i) p[i] = cme::clip_scale(p[i], (float)c.coef);
          } else {
            double* p = static_cast<double*>(g.mutable_data());
            for (py::ssize_t i = 0; i < n; ++i) p[i] = cme::clip_scale(p[i], c.coef);
          }
        }
        return py::make_tuple(c.norm, c.coef);
      },
      py::arg("g"), py::arg("segments"), py::arg("clip_norm"));
  m.def(
      "window_rate",
      [](double lr, double t0, f64arr factors, int64_t t) {
        if (factors.size() < 1) throw std::invalid_argument("window_rate: at least one factor");
        std::vector<double> w(cme::kWindowHeader + factors.size());
        w[0] = t0;
        w[1] = (double)factors.size();
        std::copy(factors.data(), factors.data() + factors.size(), w.begin() + cme::kWindowHeader);
        return cme::window_rate(lr, w.data(), (int)factors.size(), (double)t);
      },
      py::arg("lr"), py::arg("t0"), py::arg("factors"), py::arg("t"));

  // keeping the best validation weights (csrc/mlp/best.h, the header the kernel compiles): one decision.  record = the
  // 8 doubles {evals, best_index, best_metric, bad, stopped, stop_index, last_metric, spare}; monitor 0 = loss, 1 =
  // accuracy; patience < 0 never stops; triples = [R][3] doubles {n, correct, loss_sum}, summed in rank order.
  // Returns (the advanced record, improved).
  m.def(
      "best_decide",
      [](f64arr record, int monitor, double min_delta, int patience, f64arr triples) {
        if (record.size() != cme::kBestRecWords) throw std::invalid_argument("best_decide: a record of 8 doubles");
        if (monitor != cme::kBestLoss && monitor != cme::kBestAccuracy)
          throw std::invalid_argument("best_decide: monitor 0 (loss) or 1 (accuracy)");
        if (!(min_delta >= 0.0)) throw std::invalid_argument("best_decide: min_delta must be >= 0");
        if (triples.ndim() != 2 || triples.shape(0) < 1 || triples.shape(1) != 3)
          throw std::invalid_argument("best_decide: triples [R][3], R >= 1");
        cme::BestRecord rec = cme::best_load(record.data());
        const cme::BestRule rule{monitor, min_delta, patience};
        const double metric = cme::best_metric_of(triples.data(), (int)triples.shape(0), monitor);
        const bool improved = cme::best_decide(rec, rule, metric);
        py::array_t<double> out(cme::kBestRecWords);
        cme::best_store(out.mutable_data(), rec);
        return py::make_tuple(out, improved);
      },
      py::arg("record"), py::arg("monitor"), py::arg("min_delta"), py::arg("patience"), py::arg("triples"));
  m.def("best_start", [] {
    py::array_t<double> out(cme::kBestRecWords);
    cme::best_store(out.mutable_data(), cme::best_start());
    return out;
  });

  // reduce on plateau (csrc/mlp/plateau.h, the header the kernels compile): one decision.  record = the 8 doubles
  // {evals, best, bad, cooldown_left, scale, reductions, last_metric, last_reduced_index}; rule = (monitor, factor,
  // patience, threshold, threshold_mode, cooldown, min_factor, eps) with monitor 0 = loss (min), 1 = accuracy (max) and
  // threshold_mode 0 = rel, 1 = abs; triples = [R][3] doubles {n, correct, loss_sum}, summed in rank order.  Returns
  // (the advanced record, reduced).  plateau_decide_metric takes the metric itself.  plateau_rate: lr_t * scale.
  {
    auto rule_of = [](py::tuple r) {
      if (r.size() != 8) throw std::invalid_argument("plateau: rule = (monitor, factor, patience, threshold, threshold_mode, cooldown, min_factor, eps)");
      cme::PlateauRule q{r[0].cast<int>(), r[1].cast<double>(), r[2].cast<int>(), r[3].cast<double>(),
                         r[4].cast<int>(), r[5].cast<int>(), r[6].cast<double>(), r[7].cast<double>()};
      if (!cme::plateau_rule_ok(q)) throw std::invalid_argument("plateau: rule out of range");
      return q;
    };
    auto decide = [](f64arr record, const cme::PlateauRule& rule, double metric) {
      if (record.size() != cme::kPlateauRecWords) throw std::invalid_argument("plateau_decide: a record of 8 doubles");
      cme::PlateauRecord rec = cme::plateau_load(record.data());
      const bool reduced = cme::plateau_decide(rec, rule, metric);
      py::array_t<double> out(cme::kPlateauRecWords);
      cme::plateau_store(out.mutable_data(), rec);
      return py::make_tuple(out, reduced);
    };
    m.def(
        "plateau_decide",
        [rule_of, decide](f64arr record, py::tuple rule, f64arr triples) {
          if (triples.ndim() != 2 || triples.shape(0) < 1 || triples.shape(1) != 3)
            throw std::invalid_argument("plateau_decide: triples [R][3], R >= 1");
          const cme::PlateauRule q = rule_of(rule);
          return decide(record, q, cme::best_metric_of(triples.data(), (int)triples.shape(0), q.monitor));
        },
        py::arg("record"), py::arg("rule"), py::arg("triples"));
    m.def(
        "plateau_decide_metric",
        [rule_of, decide](f64arr record, py::tuple rule, double metric) { return decide(record, rule_of(rule), metric); },
        py::arg("record"), py::arg("rule"), py::arg("metric"));
    m.def("plateau_start", [](int monitor) {
      py::array_t<double> out(cme::kPlateauRecWords);
      cme::plateau_store(out.mutable_data(), cme::plateau_start(monitor));
      return out;
    }, py::arg("monitor") = 0);
    m.def("plateau_rate", &cme::plateau_rate, py::arg("lr_t"), py::arg("scale"));
    m.attr("plateau_scale_word") = cme::kPlateauScaleWord;
  }

  // the per-epoch shuffle's order (csrc/mlp/shuffle.h, the header the gather kernel compiles): sample i of the
  // shuffled set is source sample perm[i]; key = the iteration counter at the epoch start
  m.def(
      "epoch_permutation",
      [](int64_t n, uint32_t seed, uint32_t key) {
        if (n < 0 || n > INT32_MAX) throw std::invalid_argument("epoch_permutation: n must be in [0, 2^31)");
        py::array_t<int32_t> out(n);
        int32_t* o = out.mutable_data();
        const uint64_t k = cme::shuffle_key(seed, key);
        for (int64_t i = 0; i < n; ++i) o[i] = (int32_t)cme::shuffle_index((uint32_t)i, (uint32_t)n, k);
        return out;
      },
      py::arg("n"), py::arg("seed"), py::arg("key"));

  // sampling with replacement (csrc/mlp/sample.h, the header the gather kernels compile).  The alias table of per-sample
  // weights: uint32 [N][2] = {threshold, alias}, a pure function of the weights (fp64, no math library)
  m.def(
      "alias_table",
      [](const py::array& weights) {
        if (weights.ndim() != 1) throw std::invalid_argument("alias_table: the weights must be a vector [N]");
        const f64arr w = f64arr::ensure(weights);
        if (!w) throw std::invalid_argument("alias_table: the weights must be numbers");
        const int64_t n = w.shape(0);
        if (n < 1 || n >= (int64_t{1} << 31)) throw std::invalid_argument("alias_table: N must be in [1, 2^31)");
        u32arr out({n, (int64_t)2});
        cme::sample_alias_table(w.data(), n, out.mutable_data());
        return out;
      },
      py::arg("weights"));
  // ... and the draws of the epoch that starts at iteration counter `key`: sample i of the resident set is source
  // sample draws[i] (rows may repeat), with the kernel's bits
  m.def(
      "epoch_draws",
      [](int64_t n, uint32_t seed, uint32_t key, const u32arr& table) {
        if (n < 1 || n > INT32_MAX) throw std::invalid_argument("epoch_draws: n must be in [1, 2^31)");
        if (table.ndim() != 2 || table.shape(0) != n || table.shape(1) != 2)
          throw std::invalid_argument("epoch_draws: the table must be uint32 [n][2]");
        const uint32_t* t = table.data();
        if (reinterpret_cast<uintptr_t>(t) & 7) throw std::invalid_argument("epoch_draws: the table must be 8-byte aligned");
        for (int64_t i = 0; i < n; ++i)
          if (t[2 * i + 1] >= (uint64_t)n) throw std::invalid_argument("epoch_draws: an alias is outside [0, n)");
        py::array_t<int32_t> out(n);
        int32_t* o = out.mutable_data();
        const uint64_t k = cme::sample_key(seed, key);
        for (int64_t i = 0; i < n; ++i) o[i] = (int32_t)cme::sample_draw((uint32_t)i, (uint32_t)n, k, t);
        return out;
      },
      py::arg("n"), py::arg("seed"), py::arg("key"), py::arg("table"));

  // the augmentation's shifts (csrc/mlp/augment.h, the header the augmenting gather compiles): row i = (dx, dy) of
  // SOURCE sample i in the epoch that starts at iteration counter `key`
  m.def(
      "epoch_shifts",
      [](int64_t n, uint32_t seed, uint32_t key, int max_dx, int max_dy) {
        if (n < 0 || n > INT32_MAX) throw std::invalid_argument("epoch_shifts: n must be in [0, 2^31)");
        if (max_dx < 0 || max_dy < 0 || max_dx > (1 << 20) || max_dy > (1 << 20))
          throw std::invalid_argument("epoch_shifts: the shift bounds must be in [0, 2^20]");
        py::array_t<int32_t> out({n, (int64_t)2});
        int32_t* o = out.mutable_data();
        const uint64_t k = cme::augment_key(seed, key);
        for (int64_t i = 0; i < n; ++i) {
          const cme::AugmentShift s = cme::augment_shift((uint32_t)i, k, max_dx, max_dy);
          o[2 * i] = s.dx;
          o[2 * i + 1] = s.dy;
        }
        return out;
      },
      py::arg("n"), py::arg("seed"), py::arg("key"), py::arg("max_dx"), py::arg("max_dy"));
  // rows of h x w images, each moved by its own (dx, dy): out[i][f] = x[i][augment_src_feature(f, ...)] or all-zero
  // bits.  Any element of 1 / 2 / 4 / 8 bytes (uint8, float32, float64, ...): the rule moves bytes
  m.def(
      "augment_rows",
      [](const py::array& x, const i32arr& shifts, int h, int w) {
        if (x.ndim() != 2 || !(x.flags() & py::array::c_style))
          throw std::invalid_argument("augment_rows: x must be a C-contiguous [N][P] array");
        const int64_t n = x.shape(0), p = x.shape(1), es = x.itemsize();
        if (es != 1 && es != 2 && es != 4 && es != 8)
          throw std::invalid_argument("augment_rows: the element size must be 1, 2, 4 or 8 bytes");
        if (h < 1 || w < 1 || (int64_t)h * w != p) throw std::invalid_argument("augment_rows: h * w must equal P");
        if (p > INT32_MAX) throw std::invalid_argument("augment_rows: P must be below 2^31");
        if (shifts.ndim() != 2 || shifts.shape(0) != n || shifts.shape(1) != 2)
          throw std::invalid_argument("augment_rows: shifts must be int32 [N][2]");
        py::array out(x.dtype(), {n, p});
        const char* src = static_cast<const char*>(x.data());
        char* dst = static_cast<char*>(out.mutable_data());
        const int32_t* sh = shifts.data();
        for (int64_t i = 0; i < n; ++i) {
          const int dx = sh[2 * i], dy = sh[2 * i + 1];
          for (int64_t f = 0; f < p; ++f) {
            const int sf = cme::augment_src_feature((int)f, dx, dy, h, w);
            char* d = dst + (i * p + f) * es;
            if (sf >= 0) std::memcpy(d, src + (i * p + sf) * es, (size_t)es);
            else std::memset(d, 0, (size_t)es);
          }
        }
        return out;
      },
      py::arg("x"), py::arg("shifts"), py::arg("h"), py::arg("w"));

  // the affine augmentation (csrc/mlp/affine.h, the header the affine gather compiles).  The table: int32 [T][4], the
  // Q16 inverse maps {q00, q01, q10, q11}, a pure function of the arguments (fp64 through libm)
  m.def(
      "affine_table",
      [](uint32_t seed, int T, double rotate, double lo, double hi, double shear) {
        if (T < 1 || T > cme::kAffineMaxTable) throw std::invalid_argument("affine_table: 1 <= T <= 65536");
        if (!(rotate >= 0.0 && rotate <= 180.0)) throw std::invalid_argument("affine_table: 0 <= rotate <= 180");
        if (!(shear >= 0.0 && shear <= 60.0)) throw std::invalid_argument("affine_table: 0 <= shear <= 60");
        if (!(lo >= 1.0 / 16 && lo <= hi && hi <= 16.0))
          throw std::invalid_argument("affine_table: 1/16 <= lo <= hi <= 16");
        py::array_t<int32_t> out({(int64_t)T, (int64_t)4});
        int32_t* o = out.mutable_data();
        for (int k = 0; k < T; ++k) {
          const cme::AffineEntry e = cme::affine_table_entry(seed, (uint32_t)k, rotate, lo, hi, shear);
          o[4 * k] = e.q00, o[4 * k + 1] = e.q01, o[4 * k + 2] = e.q10, o[4 * k + 3] = e.q11;
        }
        return out;
      },
      py::arg("seed"), py::arg("T"), py::arg("rotate"), py::arg("lo"), py::arg("hi"), py::arg("shear"));
  // the table index of SOURCE sample i in the epoch that starts at iteration counter `key`
  m.def(
      "epoch_transforms",
      [](int64_t n, uint32_t seed, uint32_t key, int T) {
        if (n < 0 || n > INT32_MAX) throw std::invalid_argument("epoch_transforms: n must be in [0, 2^31)");
        if (T < 1 || T > cme::kAffineMaxTable) throw std::invalid_argument("epoch_transforms: 1 <= T <= 65536");
        py::array_t<int32_t> out(n);
        int32_t* o = out.mutable_data();
        const uint64_t k = cme::augment_key(seed, key);
        for (int64_t i = 0; i < n; ++i) o[i] = (int32_t)cme::affine_index((uint32_t)i, k, (uint32_t)T);
        return out;
      },
      py::arg("n"), py::arg("seed"), py::arg("key"), py::arg("T"));
  // rows of h x w images, row i resampled through entries[i] = {q00, q01, q10, q11} and moved by shifts[i] = (dx, dy).
  // kind: 0 uint8, 1 bf16 (as 2-byte integers), 2 float32, 3 float64; -1: by the dtype (a 2-byte element is bf16)
  m.def(
      "affine_rows",
      [](const py::array& x, const i32arr& shifts, const i32arr& entries, int h, int w, int kind) {
        if (x.ndim() != 2 || !(x.flags() & py::array::c_style))
          throw std::invalid_argument("affine_rows: x must be a C-contiguous [N][P] array");
        const int64_t n = x.shape(0), p = x.shape(1), es = x.itemsize();
        if (kind < 0) {
          const char dk = x.dtype().kind();
          kind = es == 1 ? cme::kAffineU8 : es == 2 ? cme::kAffineBf16 : (es == 4 && dk == 'f') ? cme::kAffineF32
                 : (es == 8 && dk == 'f') ? cme::kAffineF64 : -1;
        }
        if (cme::affine_kind_size(kind) != es || es == 0)
          throw std::invalid_argument("affine_rows: elements must be uint8, bf16 bits, float32 or float64");
        if (h < 1 || w < 1 || (int64_t)h * w != p) throw std::invalid_argument("affine_rows: h * w must equal P");
        if (h > cme::kAffineMaxSide || w > cme::kAffineMaxSide)
          throw std::invalid_argument("affine_rows: h and w must be <= 2^24");
        if (shifts.ndim() != 2 || shifts.shape(0) != n || shifts.shape(1) != 2)
          throw std::invalid_argument("affine_rows: shifts must be int32 [N][2]");
        if (entries.ndim() != 2 || entries.shape(0) != n || entries.shape(1) != 4)
          throw std::invalid_argument("affine_rows: entries must be int32 [N][4]");
        const int32_t* sh = shifts.data();
        const int32_t* en = entries.data();
        for (int64_t i = 0; i < n; ++i) {
          if (sh[2 * i] <= -w || sh[2 * i] >= w || sh[2 * i + 1] <= -h || sh[2 * i + 1] >= h)
            throw std::invalid_argument("affine_rows: a shift must be smaller than the image");
          for (int j = 0; j < 4; ++j)
            if (en[4 * i + j] <= -(1 << 23) || en[4 * i + j] >= (1 << 23))
              throw std::invalid_argument("affine_rows: an entry must be below 2^23 in magnitude");
        }
        py::array out(x.dtype(), {n, p});
        const auto run = [&](auto u) {
          using U = decltype(u);
          const U* src = static_cast<const U*>(x.data());
          U* dst = static_cast<U*>(out.mutable_data());
          for (int64_t i = 0; i < n; ++i) {
            const cme::AffineEntry q{en[4 * i], en[4 * i + 1], en[4 * i + 2], en[4 * i + 3]};
            for (int y = 0; y < h; ++y)
              for (int xx = 0; xx < w; ++xx)
                dst[i * p + (int64_t)y * w + xx] = cme::affine_pixel<U>(src + i * p, y, xx, sh[2 * i], sh[2 * i + 1], q, h, w);
          }
        };
        if (es == 1) run(uint8_t{});
        else if (es == 2) run(uint16_t{});
        else if (es == 4) run(uint32_t{});
        else run(uint64_t{});
        return out;
      },
      py::arg("x"), py::arg("shifts"), py::arg("entries"), py::arg("h"), py::arg("w"), py::arg("kind") = -1);

  // the elastic distortion (csrc/mlp/warp.h, the header the warping gather compiles).  The axis tables: int32
  // [h + w][5] = {i, w0, w1, w2, w3}, the y axis first, a pure function of the arguments
  m.def(
      "warp_axes",
      [](int h, int w, int gy, int gx) {
        if (h < 1 || w < 1 || h > cme::kAffineMaxSide || w > cme::kAffineMaxSide)
          throw std::invalid_argument("warp_axes: 1 <= h, w <= 2^24");
        if (gy < 1 || gy > cme::kWarpMaxGrid || gx < 1 || gx > cme::kWarpMaxGrid)
          throw std::invalid_argument("warp_axes: 1 <= gy, gx <= 5");
        py::array_t<int32_t> out({(int64_t)h + w, (int64_t)5});
        int32_t* o = out.mutable_data();
        for (int64_t k = 0; k < (int64_t)h + w; ++k) {
          const cme::WarpAxis e = k < h ? cme::warp_axis_entry((int)k, h, gy) : cme::warp_axis_entry((int)(k - h), w, gx);
          o[5 * k] = e.i;
          for (int j = 0; j < 4; ++j) o[5 * k + 1 + j] = e.w[j];
        }
        return out;
      },
      py::arg("h"), py::arg("w"), py::arg("gy"), py::arg("gx"));
  // int32 [n][L][2]: (ddx, ddy) in Q8 of node j of SOURCE sample i in the epoch that starts at iteration counter `key`
  m.def(
      "epoch_nodes",
      [](int64_t n, uint32_t seed, uint32_t key, int L, int A) {
        if (n < 0 || n > INT32_MAX) throw std::invalid_argument("epoch_nodes: n must be in [0, 2^31)");
        if (L < 1 || L > cme::kWarpMaxNodes) throw std::invalid_argument("epoch_nodes: 1 <= L <= 64");
        if (A < 0 || A > cme::kWarpMaxA) throw std::invalid_argument("epoch_nodes: 0 <= A <= 2048");
        py::array_t<int32_t> out({n, (int64_t)L, (int64_t)2});
        int32_t* o = out.mutable_data();
        const uint64_t k = cme::augment_key(seed, key);
        for (int64_t i = 0; i < n; ++i) {
          const uint64_t nk = cme::warp_node_key((uint32_t)i, k);
          for (int j = 0; j < L; ++j) {
            const cme::WarpNode nd = cme::warp_node(nk, (uint32_t)j, A);
            o[(i * L + j) * 2] = nd.ddx, o[(i * L + j) * 2 + 1] = nd.ddy;
          }
        }
        return out;
      },
      py::arg("n"), py::arg("seed"), py::arg("key"), py::arg("L"), py::arg("A"));
  {
    // what warp_field and warp_rows share: the axis tables and one sample's or every sample's nodes, range-checked so
    // that no node index leaves the lattice and no product leaves int32
    const auto check_axes = [](const char* who, const i32arr& axes, int h, int w, int gy, int gx) {
      const std::string p = std::string(who) + ": ";
      if (gy < 1 || gy > cme::kWarpMaxGrid || gx < 1 || gx > cme::kWarpMaxGrid)
        throw std::invalid_argument(p + "1 <= gy, gx <= 5");
      if (h < 1 || w < 1 || h > cme::kAffineMaxSide || w > cme::kAffineMaxSide)
        throw std::invalid_argument(p + "1 <= h, w <= 2^24");
      if (axes.ndim() != 2 || axes.shape(0) != (int64_t)h + w || axes.shape(1) != 5)
        throw std::invalid_argument(p + "axes must be int32 [h + w][5]");
      const int32_t* ax = axes.data();
      for (int64_t k = 0; k < (int64_t)h + w; ++k) {
        if (ax[5 * k] < 0 || ax[5 * k] >= (k < h ? gy : gx))
          throw std::invalid_argument(p + "an axis entry's cell must lie inside the grid");
        int sum = 0;
        for (int j = 1; j < 5; ++j) {
          if (ax[5 * k + j] < 0 || ax[5 * k + j] > cme::kWarpOne)
            throw std::invalid_argument(p + "an axis weight must be in [0, 4096]");
          sum += ax[5 * k + j];
        }
        if (sum != cme::kWarpOne) throw std::invalid_argument(p + "an axis entry's weights must sum to 4096");
      }
    };
    const auto check_nodes = [](const char* who, const int32_t* nd, int64_t count) {
      for (int64_t k = 0; k < count; ++k)
        if (nd[k] < -cme::kWarpMaxA || nd[k] > cme::kWarpMaxA)
          throw std::invalid_argument(std::string(who) + ": a node must be in [-2048, 2048]");
    };
    const auto axis_at = [](const int32_t* ax, int64_t k) {
      return cme::WarpAxis{ax[5 * k], {ax[5 * k + 1], ax[5 * k + 2], ax[5 * k + 3], ax[5 * k + 4]}};
    };
    // int32 [h][w][2]: (d17x, d17y), the displacement of every destination pixel in 2^-17 pixel, of one sample's
    // nodes int32 [L][2]
    m.def(
        "warp_field",
        [=](const i32arr& nodes, const i32arr& axes, int h, int w, int gy, int gx) {
          check_axes("warp_field", axes, h, w, gy, gx);
          const int L = (gy + 3) * (gx + 3);
          if (nodes.ndim() != 2 || nodes.shape(0) != L || nodes.shape(1) != 2)
            throw std::invalid_argument("warp_field: nodes must be int32 [(gy + 3)(gx + 3)][2]");
          const int32_t* nd = nodes.data();
          check_nodes("warp_field", nd, 2 * (int64_t)L);
          const int32_t* ax = axes.data();
          py::array_t<int32_t> out({(int64_t)h, (int64_t)w, (int64_t)2});
          int32_t* o = out.mutable_data();
          for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
              const cme::WarpDisp d = cme::warp_displace(axis_at(ax, y), axis_at(ax, (int64_t)h + x), gx, [&](int j) {
                return cme::WarpNode{nd[2 * j], nd[2 * j + 1]};
              });
              o[((int64_t)y * w + x) * 2] = d.x, o[((int64_t)y * w + x) * 2 + 1] = d.y;
            }
          return out;
        },
        py::arg("nodes"), py::arg("axes"), py::arg("h"), py::arg("w"), py::arg("gy"), py::arg("gx"));
    // affine_rows with row i's source positions moved by the field of nodes[i] (int32 [N][L][2]); kind as there
    m.def(
        "warp_rows",
        [=](const py::array& x, const i32arr& shifts, const i32arr& entries, const i32arr& nodes, const i32arr& axes,
            int h, int w, int gy, int gx, int kind) {
          if (x.ndim() != 2 || !(x.flags() & py::array::c_style))
            throw std::invalid_argument("warp_rows: x must be a C-contiguous [N][P] array");
          const int64_t n = x.shape(0), p = x.shape(1), es = x.itemsize();
          if (kind < 0) {
            const char dk = x.dtype().kind();
            kind = es == 1 ? cme::kAffineU8 : es == 2 ? cme::kAffineBf16 : (es == 4 && dk == 'f') ? cme::kAffineF32
                   : (es == 8 && dk == 'f') ? cme::kAffineF64 : -1;
          }
          if (cme::affine_kind_size(kind) != es || es == 0)
            throw std::invalid_argument("warp_rows: elements must be uint8, bf16 bits, float32 or float64");
          if (h < 1 || w < 1 || (int64_t)h * w != p) throw std::invalid_argument("warp_rows: h * w must equal P");
          check_axes("warp_rows", axes, h, w, gy, gx);
          const int L = (gy + 3) * (gx + 3);
          if (shifts.ndim() != 2 || shifts.shape(0) != n || shifts.shape(1) != 2)
            throw std::invalid_argument("warp_rows: shifts must be int32 [N][2]");
          if (entries.ndim() != 2 || entries.shape(0) != n || entries.shape(1) != 4)
            throw std::invalid_argument("warp_rows: entries must be int32 [N][4]");
          if (nodes.ndim() != 3 || nodes.shape(0) != n || nodes.shape(1) != L || nodes.shape(2) != 2)
            throw std::invalid_argument("warp_rows: nodes must be int32 [N][(gy + 3)(gx + 3)][2]");
          const int32_t* sh = shifts.data();
          const int32_t* en = entries.data();
          const int32_t* nd = nodes.data();
          const int32_t* ax = axes.data();
          check_nodes("warp_rows", nd, n * L * 2);
          for (int64_t i = 0; i < n; ++i) {
            if (sh[2 * i] <= -w || sh[2 * i] >= w || sh[2 * i + 1] <= -h || sh[2 * i + 1] >= h)
              throw std::invalid_argument("warp_rows: a shift must be smaller than the image");
            for (int j = 0; j < 4; ++j)
              if (en[4 * i + j] <= -(1 << 23) || en[4 * i + j] >= (1 << 23))
                throw std::invalid_argument("warp_rows: an entry must be below 2^23 in magnitude");
          }
          py::array out(x.dtype(), {n, p});
          const auto run = [&](auto u) {
            using U = decltype(u);
            const U* src = static_cast<const U*>(x.data());
            U* dst = static_cast<U*>(out.mutable_data());
            for (int64_t i = 0; i < n; ++i) {
              const cme::AffineEntry q{en[4 * i], en[4 * i + 1], en[4 * i + 2], en[4 * i + 3]};
              const int32_t* ni = nd + i * L * 2;
              for (int y = 0; y < h; ++y)
                for (int xx = 0; xx < w; ++xx) {
                  const cme::WarpDisp d = cme::warp_displace(axis_at(ax, y), axis_at(ax, (int64_t)h + xx), gx, [&](int j) {
                    return cme::WarpNode{ni[2 * j], ni[2 * j + 1]};
                  });
                  const cme::AffineTaps t = cme::warp_taps(y, xx, sh[2 * i], sh[2 * i + 1], q, h, w, d);
                  dst[i * p + (int64_t)y * w + xx] = cme::warp_blend<U>(src + i * p, t, h, w);
                }
            }
          };
          if (es == 1) run(uint8_t{});
          else if (es == 2) run(uint16_t{});
          else if (es == 4) run(uint32_t{});
          else run(uint64_t{});
          return out;
        },
        py::arg("x"), py::arg("shifts"), py::arg("entries"), py::arg("nodes"), py::arg("axes"), py::arg("h"),
        py::arg("w"), py::arg("gy"), py::arg("gx"), py::arg("kind") = -1);
  }

  // ---------------------------------------------------------------- I/O
  m.def(
      "read_idx_images",
      [](const std::string& path, int max_n) {
        int n, r, c;
        auto v = cme::io::read_idx_images(path, &n, &r, &c, max_n);
        py::array_t<uint8_t> a({n, r * c});
        std::memcpy(a.mutable_data(), v.data(), v.size());
        return py::make_tuple(a, r, c);
      },
      py::arg("path"), py::arg("max_n") = -1);
  m.def(
      "read_idx_labels",
      [](const std::string& path, int max_n) {
        int n;
        auto v = cme::io::read_idx_labels(path, &n, max_n);
        py::array_t<uint8_t> a(n);
        std::memcpy(a.mutable_data(), v.data(), v.size());
        return a;
      },
      py::arg("path"), py::arg("max_n") = -1);
  m.def("write_idx_images", [](const std::string& path, py::array_t<uint8_t, py::array::c_style> px, int rows,
                               int cols) {
    cme::io::write_idx_images(path, px.data(), (int)(px.size() / ((size_t)rows * cols)), rows, cols);
  });
  m.def("write_idx_labels", [](const std::string& path, py::array_t<uint8_t, py::array::c_style> lab) {
    cme::io::write_idx_labels(path, lab.data(), (int)lab.size());
  });
  m.def(
      "save_raw_ascii",
      [](const std::string& path, f64arr a, int precision) {
        const int64_t rows = a.ndim() >= 1 ? a.shape(0) : 1;
        const int64_t cols = a.ndim() == 2 ? a.shape(1) : 1;
        cme::io::save_raw_ascii(path, a.data(), rows, cols, precision);
      },
      py::arg("path"), py::arg("a"), py::arg("precision") = 12);
  m.def("load_raw_ascii", [](const std::string& path) {
    int64_t r, c;
    auto v = cme::io::load_raw_ascii(path, &r, &c);
    py::array_t<double> a({r, c});
    std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(double));
    return a;
  });
  m.def("save_label", [](const std::string& path, i32arr lab) { cme::io::save_label(path, lab.data(), lab.size()); });

  cme::cpu::bind_suite_cpu(m);
}
