// pybind11 bindings for the gfx950 kernels (module cme213_sp18_amd._hip).
//
// Tensors cross the boundary as raw device pointers (int) and the HIP stream
// as an int handle (torch.cuda.current_stream().cuda_stream), so any launch
// issued while torch is capturing a HIP graph is recorded into that graph.
// No torch headers: the extension only depends on the HIP runtime, which it
// shares with torch (same SONAME, torch is always imported first).
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <unordered_map>

#include "common/hip_common.h"
#include "mlp/mlp_kernels.h"
#include "mlp/mlp_split.h"
#include "mlp/mlp_step.h"
#include "mlp/best.h"
#include "mlp/plateau.h"
#include "mlp/clip.h"
#include "mlp/ema.h"
#include "mlp/optim.h"
#include "mlp/affine.h"
#include "mlp/augment.h"
#include "mlp/sample.h"
#include "mlp/shuffle.h"
#include "mlp/warp.h"
#include "suite/suite_kernels.h"

namespace py = pybind11;
using cme::DType;
using cme::MlpStep;

namespace {

template <typename T>
inline T* P(uintptr_t p) { return reinterpret_cast<T*>(p); }
inline hipStream_t S(uintptr_t s) { return reinterpret_cast<hipStream_t>(s); }
inline DType to_dt(int d) {
  if (d < 0 || d > 2) throw std::invalid_argument("dtype code must be 0 (f32), 1 (f64) or 2 (bf16)");
  return static_cast<DType>(d);
}

// Binds the engine's buffers and shapes in ONE call (MlpEngine._hip_step): every device pointer, count and
// layout flag the step reads, by name; an unknown name is an error.  The runtime switches stay plain fields
// (fh_allgather, store_a1, lazy_planes, ag_*, diagnostics).
using BindFn = void (*)(MlpStep&, py::handle);
template <auto M>
void bind_field(MlpStep& s, py::handle v) { s.*M = v.cast<std::decay_t<decltype(s.*M)>>(); }
#define CME_F(name) {#name, &bind_field<&MlpStep::name>}
const std::unordered_map<std::string, BindFn> kBindFields = {
    CME_F(dt), CME_F(P), CME_F(H), CME_F(C), CME_F(ld), CME_F(N), CME_F(X), CME_F(labels), CME_F(XT), CME_F(Xw),
    CME_F(XTw), CME_F(W1), CME_F(b1), CME_F(W2), CME_F(b2), CME_F(W1g), CME_F(gW1), CME_F(gb1), CME_F(gW2),
    CME_F(gb2), CME_F(gstatus), CME_F(a1), CME_F(D), CME_F(dZ1), CME_F(dZ1g), CME_F(loss), CME_F(act), CME_F(split),
    CME_F(npw), CME_F(npz), CME_F(xscale), CME_F(W1p), CME_F(dZ1p), CME_F(z2p), CME_F(bias_col), CME_F(fh_counters),
    CME_F(fh_tiles), CME_F(ag_counters), CME_F(ag_slabs), CME_F(ag_gran), CME_F(ag_gran_count), CME_F(kpart),
    CME_F(kpart_cap), CME_F(w1s), CME_F(xs), CME_F(dz1s)};
#undef CME_F
void bind(MlpStep& s, const py::dict& d) {
  for (const auto& kv : d) {
    const std::string k = py::str(kv.first);
    const auto it = kBindFields.find(k);
    if (it == kBindFields.end()) throw std::invalid_argument("MlpStep.bind: unknown name '" + k + "'");
    it->second(s, kv.second);
  }
}

// a step's form as plain ints and strings (MlpStep.plan / plan_steps: tests and diagnostics)
py::dict form_dict(const cme::StepForm& p) {
  using namespace py::literals;
  const bool fused = p.fwd != cme::StepForm::kNone && p.fwd != cme::StepForm::kSeparate;
  const char* names[] = {"none", "allgather", "last_arriver", p.w.dw2_cols == 128 ? "wide128" : "wide64", "separate"};
  return py::dict(
      "form"_a = names[p.fwd], "fwd"_a = int(fused || p.run_fwd), "head"_a = int(fused || p.run_head),
      "a_fp32"_a = p.w.a_fp32, "w1_swz"_a = p.w.w1_swz, "x_swz"_a = p.w.x_swz, "dz_swz"_a = p.w.dz_swz,
      "head_dz32"_a = int(p.h.dZ1 != nullptr), "head_planes"_a = int(p.h.dZ1_planes != nullptr),
      "a1_stored"_a = int(p.fwd == cme::StepForm::kWide ? p.store_a1 != 0 : p.f.a1 != nullptr),
      "dw2_cols"_a = p.w.dw2part ? p.w.dw2_cols : 0, "xcd_rows"_a = p.w.xcd_rows, "pf_wgs"_a = p.w.pf_wgs,
      "pf_wgs_xt"_a = p.w.pf_wgs_xt, "wide_eng"_a = p.w.wide_eng, "w1s_refresh"_a = int(p.refresh_swz),
      "w1s_stale"_a = int(p.mark_swz_stale), "planes_refresh"_a = int(p.refresh_planes),
      "planes_left_stale"_a = int(p.planes_left_stale));
}

// what mlp_shuffle and mlp_augment share (csrc/mlp/shuffle.h ShuffleArgs): the source, the six layouts and perm as
// device addresses, the shapes and the order
cme::ShuffleArgs gather_args(uintptr_t X0, uintptr_t labels0, uintptr_t X, uintptr_t labels, uintptr_t XT,
                             uintptr_t Xs, uintptr_t Xw, uintptr_t XTw, uintptr_t perm, int N, int Pd, int es,
                             uint64_t key, int identity, uintptr_t sample_table, uint32_t sample_seed,
                             uint32_t iter) {
  cme::ShuffleArgs a;
  // a sampler (csrc/mlp/sample.h): the alias table's device address (0: none) and the key of the epoch's draws
  a.sample_table = P<const uint32_t>(sample_table);
  a.sample_key = sample_table ? cme::sample_key(sample_seed, iter) : 0;
  a.X0 = P<const void>(X0); a.labels0 = P<const int>(labels0); a.X = P<void>(X); a.labels = P<int>(labels);
  a.XT = P<void>(XT); a.Xs = P<void>(Xs); a.Xw = P<void>(Xw); a.XTw = P<void>(XTw); a.perm = P<int>(perm);
  a.N = N; a.P = Pd; a.es = es; a.key = key; a.identity = identity;
  return a;
}

}  // namespace

void bind_suite(py::module_& m);  // suite_bindings.cpp
void bind_comm(py::module_& m);   // comm/comm_bindings.cpp

#ifndef CME_HIP_MODULE
#define CME_HIP_MODULE _hip  // (_hip_diag: the diagnostics library, cme213_sp18_amd/_build.py --diag)
#endif
PYBIND11_MODULE(CME_HIP_MODULE, m) {
  m.attr("diag_stamps") = CME_DIAG_STAMPS;
  m.doc() = "cme213_sp18_amd gfx950 HIP kernels (MFMA MLP engine + homework kernel suite)";

  m.def(
      "mlp_forward1",
      [](int dt, uintptr_t W1g, uintptr_t b1, uintptr_t X, int Pd, int H, int n, uintptr_t a1, int lda, int act,
         uintptr_t s) {
        cme::mlp_forward1(to_dt(dt), P<void>(W1g), P<void>(b1), P<void>(X), Pd, H, n, P<void>(a1), lda, act, S(s));
      },
      py::arg("dt"), py::arg("W1g"), py::arg("b1"), py::arg("X"), py::arg("P"), py::arg("H"), py::arg("n"),
      py::arg("a1"), py::arg("lda"), py::arg("act"), py::arg("stream"));

  m.def(
      "mlp_head",
      [](int dt, int mode, uintptr_t a1, int lda, uintptr_t W2, uintptr_t b2, uintptr_t labels, int H, int C,
         int n, double scale, uintptr_t Dp, int ldd, uintptr_t dZ1, int ldz, uintptr_t dZ1_bf16, uintptr_t loss,
         uintptr_t pred, uintptr_t probs, int ldp, int shift, uintptr_t s, uintptr_t dZ1_planes, int npz) {
        cme::HeadArgs h{};
        h.a1 = P<void>(a1); h.lda = lda; h.W2 = P<void>(W2); h.b2 = P<void>(b2);
        h.labels = P<int>(labels); h.H = H; h.C = C; h.n = n; h.scale = scale;
        h.D = P<void>(Dp); h.ldd = ldd; h.dZ1 = P<void>(dZ1); h.ldz = ldz; h.dZ1_bf16 = P<void>(dZ1_bf16);
        h.loss_partial = P<float>(loss); h.pred = P<int>(pred); h.probs = P<void>(probs); h.ldp = ldp;
        h.shift = shift; h.mode = mode;
        h.dZ1_planes = P<void>(dZ1_planes); h.npz = npz;
        cme::mlp_head(to_dt(dt), h, S(s));
      },
      py::arg("dt"), py::arg("mode"), py::arg("a1"), py::arg("lda"), py::arg("W2"), py::arg("b2"),
      py::arg("labels") = 0, py::arg("H"), py::arg("C"), py::arg("n"), py::arg("scale") = 1.0,
      py::arg("D") = 0, py::arg("ldd") = 0, py::arg("dZ1") = 0, py::arg("ldz") = 0, py::arg("dZ1_bf16") = 0,
      py::arg("loss") = 0, py::arg("pred") = 0, py::arg("probs") = 0, py::arg("ldp") = 0,
      py::arg("shift") = 1, py::arg("stream") = 0, py::arg("dZ1_planes") = 0, py::arg("npz") = 0);
  m.def(
      "mlp_eval_head",
      [](int dt, uintptr_t a1, int lda, uintptr_t W2, uintptr_t b2, uintptr_t labels, int H, int C, int n,
         uintptr_t stats, uintptr_t partials, int zero, uintptr_t s) {
        cme::EvalArgs e{};
        e.a1 = P<void>(a1); e.lda = lda; e.W2 = P<void>(W2); e.b2 = P<void>(b2); e.labels = P<int>(labels);
        e.H = H; e.C = C; e.n = n; e.stats = P<unsigned long long>(stats); e.partials = P<double>(partials);
        e.zero = zero;
        cme::mlp_eval_head(to_dt(dt), e, S(s));
      },
      py::arg("dt"), py::arg("a1"), py::arg("lda"), py::arg("W2"), py::arg("b2"), py::arg("labels"), py::arg("H"),
      py::arg("C"), py::arg("n"), py::arg("stats"), py::arg("partials"), py::arg("zero") = 1, py::arg("stream") = 0);
  m.def("mlp_eval_num_partials", &cme::mlp_eval_num_partials, py::arg("n"));
  m.def("mlp_eval_slot_words", &cme::mlp_eval_slot_words, py::arg("C"));
  m.def("mlp_head_num_blocks", &cme::mlp_head_num_blocks);
  m.def("head_big_scratch_floats", &cme::head_big_scratch_floats);

  m.def(
      "mlp_wgrad",
      [](int dt, uintptr_t dZ1g, int ldz, uintptr_t X, int Pd, uintptr_t dZ1, uintptr_t Dp, int ldd, uintptr_t a1,
         int lda, int H, int C, int n, double reg, double lr, int sgd, uintptr_t W1, uintptr_t b1, uintptr_t W2,
         uintptr_t b2, uintptr_t gW1, uintptr_t gb1, uintptr_t gW2, uintptr_t gb2, uintptr_t W1_bf16,
         uintptr_t XT, int ldxt, int roles, uintptr_t s) {
        cme::WgradArgs w{};
        w.XT = P<void>(XT); w.ldxt = ldxt; w.roles = roles;
        w.dZ1g = P<void>(dZ1g); w.ldz = ldz; w.X = P<void>(X); w.P = Pd; w.dZ1 = P<void>(dZ1);
        w.D = P<void>(Dp); w.ldd = ldd; w.a1 = P<void>(a1); w.lda = lda; w.H = H; w.C = C; w.n = n;
        w.reg = reg; w.lr = lr; w.sgd = sgd; w.W1 = P<void>(W1); w.b1 = P<void>(b1); w.W2 = P<void>(W2);
        w.b2 = P<void>(b2); w.gW1 = P<void>(gW1); w.gb1 = P<void>(gb1); w.gW2 = P<void>(gW2);
        w.gb2 = P<void>(gb2); w.W1_bf16 = P<void>(W1_bf16);
        cme::mlp_wgrad(to_dt(dt), w, S(s));
      },
      py::arg("dt"), py::arg("dZ1g"), py::arg("ldz"), py::arg("X"), py::arg("P"), py::arg("dZ1"), py::arg("D"),
      py::arg("ldd"), py::arg("a1"), py::arg("lda"), py::arg("H"), py::arg("C"), py::arg("n"), py::arg("reg"),
      py::arg("lr"), py::arg("sgd"), py::arg("W1"), py::arg("b1"), py::arg("W2"), py::arg("b2"),
      py::arg("gW1") = 0, py::arg("gb1") = 0, py::arg("gW2") = 0, py::arg("gb2") = 0, py::arg("W1_bf16") = 0,
      py::arg("XT") = 0, py::arg("ldxt") = 0, py::arg("roles") = 7, py::arg("stream") = 0);

  m.def(
      "sgd_flat",
      [](int dt, uintptr_t params, uintptr_t grads, int64_t count, double lr, uintptr_t shadow,
         int64_t shadow_count, uintptr_t s) {
        cme::sgd_flat(to_dt(dt), P<void>(params), P<void>(grads), count, lr, P<void>(shadow), shadow_count, S(s));
      },
      py::arg("dt"), py::arg("params"), py::arg("grads"), py::arg("count"), py::arg("lr"), py::arg("shadow") = 0,
      py::arg("shadow_count") = 0, py::arg("stream") = 0);

  m.def(
      "gemm",
      [](int dt, bool tA, bool tB, int M, int N, int K, double alpha, uintptr_t A, int lda, uintptr_t B, int ldb,
         double beta, uintptr_t Cp, int ldc, uintptr_t s) {
        cme::gemm(to_dt(dt), tA, tB, M, N, K, alpha, P<void>(A), lda, P<void>(B), ldb, beta, P<void>(Cp), ldc, S(s));
      },
      py::arg("dt"), py::arg("transA"), py::arg("transB"), py::arg("M"), py::arg("N"), py::arg("K"),
      py::arg("alpha"), py::arg("A"), py::arg("lda"), py::arg("B"), py::arg("ldb"), py::arg("beta"), py::arg("C"),
      py::arg("ldc"), py::arg("stream") = 0);

  m.def(
      "convert_f32_to_bf16",
      [](uintptr_t src, uintptr_t dst, int64_t n, uintptr_t s) {
        cme::convert_f32_to_bf16(P<const float>(src), P<void>(dst), n, S(s));
      },
      py::arg("src"), py::arg("dst"), py::arg("n"), py::arg("stream") = 0);

  py::class_<MlpStep>(m, "MlpStep")
      .def(py::init<>())
      .def("bind", &bind, py::arg("buffers"))
      .def_readonly("dt", &MlpStep::dt)
      .def_readonly("P", &MlpStep::P)
      .def_readonly("H", &MlpStep::H)
      .def_readonly("C", &MlpStep::C)
      .def_readonly("ld", &MlpStep::ld)
      .def_readonly("split", &MlpStep::split)
      .def_readwrite("shift", &MlpStep::shift)
      .def_readwrite("ag_err", &MlpStep::ag_err)
      .def_readwrite("head_dw2", &MlpStep::head_dw2)
      .def_readwrite("fh_allgather", &MlpStep::fh_allgather)
      .def_readwrite("ag_wait_us", &MlpStep::ag_wait_us)
      .def_readwrite("ag_test_skip", &MlpStep::ag_test_skip)
      .def_readwrite("store_a1", &MlpStep::store_a1)
      .def_readwrite("ag_tiles64", &MlpStep::ag_tiles64)
      .def_readwrite("xcd_rows", &MlpStep::xcd_rows)
      .def_readwrite("xcd_pack", &MlpStep::xcd_pack)
      .def_readwrite("w1_swz", &MlpStep::w1_swz)
      .def_readwrite("x_swz", &MlpStep::x_swz)
      .def_readwrite("a_fp32", &MlpStep::a_fp32)
      .def_readwrite("dz_swz", &MlpStep::dz_swz)
      .def_property_readonly("dz_left_swz", [](const MlpStep& st) { return st.left.dz_swz; })
      .def_readwrite("swz_stale", &MlpStep::swz_stale)
      .def_readwrite("prefetch", &MlpStep::prefetch)
      .def_readwrite("prefetch_xt", &MlpStep::prefetch_xt)
      .def_readwrite("wide_eng", &MlpStep::wide_eng)
      .def_readwrite("xp_dbg", &MlpStep::xp_dbg)
      .def_readwrite("g64_touch", &MlpStep::g64_touch)
      .def_readwrite("xstep", &MlpStep::xstep)
      .def_readwrite("xstep_pix", &MlpStep::xstep_pix)
      .def_readonly("xstep_used", &MlpStep::xstep_used)
      // (writable: a trainer that never enters run_steps -- a stateful optimizer -- records why here)
      .def_readwrite("xstep_reason", &MlpStep::xstep_reason)
      .def_readwrite("xs_stamps", &MlpStep::xs_stamps)
      .def_readwrite("xs_stamp_steps", &MlpStep::xs_stamp_steps)
      .def_readwrite("xs_w1stamps", &MlpStep::xs_w1stamps)
      .def_readwrite("lazy_planes", &MlpStep::lazy_planes)
      .def_readwrite("planes_stale", &MlpStep::planes_stale)
      .def_readwrite("dw2p", &MlpStep::dw2p)
      .def_readwrite("stamps", &MlpStep::stamps)
      .def_readwrite("hstamps", &MlpStep::hstamps)
      .def_readwrite("wstamps", &MlpStep::wstamps)
      .def("refresh_planes", &MlpStep::refresh_planes, py::arg("stream"))
      .def("w1_planes_read", &MlpStep::w1_planes_read)
      .def("lazy_planes_apply", &MlpStep::lazy_planes_apply)
      .def("plan",
           [](const MlpStep& st, int64_t off, int n, int sgd, int parts, int with_loss) {
             return form_dict(st.plan(off, n, 1.0, 0.0, 0.0, sgd, with_loss, parts));
           },
           py::arg("off"), py::arg("n"), py::arg("sgd"), py::arg("parts") = 3, py::arg("with_loss") = 0)
      .def("plan_steps",  // (does not look at stream capture: run_steps does)
           [](const MlpStep& st, int64_t gstart0, int64_t count, int64_t B, int64_t shard_off, int n, int64_t N_end) {
             cme::StepForm p;
             const char* why = st.plan_steps(gstart0, count, B, shard_off, n, N_end, 1.0, 0.0, 0.0, nullptr, p);
             py::dict d = why ? py::dict() : form_dict(p);
             d["xstep"] = int(!why);
             d["why_not"] = why ? why : "";
             if (!why) d["row_major"] = int(p.w.dz_swz == 0);
             return d;
           },
           py::arg("gstart0"), py::arg("count"), py::arg("B"), py::arg("shard_off"), py::arg("n"), py::arg("N_end"))
      .def("tp_forward", &MlpStep::tp_forward)
      .def("tp_head", &MlpStep::tp_head)
      .def("set_xgmi", &MlpStep::set_xgmi, py::arg("desc"), py::arg("slots"), py::arg("off_b1"), py::arg("off_W2"),
           py::arg("off_b2"), py::arg("push") = 0)
      .def_property_readonly("xgmi_push", [](const MlpStep& st) { return st.xf.push; })
      .def("run_steps", &MlpStep::run_steps, py::arg("gstart0"), py::arg("count"), py::arg("B"), py::arg("shard_off"),
           py::arg("n"), py::arg("N_end"), py::arg("scale"), py::arg("reg"), py::arg("lr"), py::arg("sgd"),
           py::arg("stream"),
           py::call_guard<py::gil_scoped_release>())
      .def("run_wgrad", &MlpStep::run_wgrad, py::arg("off"), py::arg("n"), py::arg("scale"), py::arg("reg"),
           py::arg("lr"), py::arg("sgd"), py::arg("parts"), py::arg("row0"), py::arg("rows"), py::arg("stream"))
      .def("predict", &MlpStep::predict, py::arg("x"), py::arg("n"), py::arg("a1buf"), py::arg("lda"),
           py::arg("pred"), py::arg("stream"))
      .def("evaluate", &MlpStep::evaluate, py::arg("x"), py::arg("labels"), py::arg("n"), py::arg("a1buf"),
           py::arg("lda"), py::arg("stats"), py::arg("partials"), py::arg("stream"), py::arg("zero") = 0)
      .def("run", &MlpStep::run, py::arg("off"), py::arg("n"), py::arg("scale"), py::arg("reg"), py::arg("lr"),
           py::arg("sgd"), py::arg("with_loss"), py::arg("stream"), py::arg("parts") = 3, py::arg("pf_next") = -1);

  m.def(
      "occupy_cus",
      [](int wgs, int lds_bytes, int64_t ns, uintptr_t s, uintptr_t running) {
        cme::occupy_cus(wgs, lds_bytes, ns, S(s), reinterpret_cast<int*>(running));
      },
      py::arg("wgs"), py::arg("lds_bytes"), py::arg("ns"), py::arg("stream"), py::arg("running") = 0);
  m.def(
      "mlp_split_w1s_floats", [](int H, int Pd) { return cme::mlp_split_w1s_floats(H, Pd); }, py::arg("H"),
      py::arg("P"));

  m.def(
      "split_planes",
      [](uintptr_t W, uintptr_t planes, int64_t n, int np, uintptr_t s) {
        cme::mlp_split_planes(P<const float>(W), P<void>(planes), n, np, S(s));
      },
      py::arg("W"), py::arg("planes"), py::arg("n"), py::arg("np"), py::arg("stream") = 0);
  m.def(
      "split_sgd",
      [](uintptr_t params, uintptr_t grads, int64_t count, double lr, uintptr_t W1p, int64_t w1n, int npw,
         uintptr_t s, uintptr_t status) {
        cme::mlp_split_sgd(P<float>(params), P<const float>(grads), count, lr, P<void>(W1p), w1n, npw, S(s),
                           P<const float>(status));
      },
      py::arg("params"), py::arg("grads"), py::arg("count"), py::arg("lr"), py::arg("W1p"), py::arg("w1n"),
      py::arg("npw"), py::arg("stream") = 0, py::arg("status") = 0);
  m.def(
      "mlp_shuffle",
      [](uintptr_t X0, uintptr_t labels0, uintptr_t X, uintptr_t labels, uintptr_t XT, uintptr_t Xs, uintptr_t Xw,
         uintptr_t XTw, uintptr_t perm, int N, int Pd, int es, uint32_t seed, uint32_t key, int identity, uintptr_t s,
         uintptr_t sample_table, uint32_t sample_seed) {
        cme::mlp_shuffle(gather_args(X0, labels0, X, labels, XT, Xs, Xw, XTw, perm, N, Pd, es,
                                     cme::shuffle_key(seed, key), identity, sample_table, sample_seed, key),
                         P<void>(s));
      },
      py::arg("X0"), py::arg("labels0"), py::arg("X"), py::arg("labels"), py::arg("XT"), py::arg("Xs"), py::arg("Xw"),
      py::arg("XTw"), py::arg("perm"), py::arg("N"), py::arg("P"), py::arg("es"), py::arg("seed"), py::arg("key"),
      py::arg("identity") = 0, py::arg("stream") = 0, py::arg("sample_table") = 0, py::arg("sample_seed") = 0);
  // the augmenting gather (csrc/mlp/augment.hip): mlp_shuffle's layouts, each image moved by its keyed (dx, dy);
  // shuffled != 0: the order of shuffle_key(shuffle_seed, key), else the loaded order.  sample_table != 0 (all four
  // gathers; csrc/mlp/sample.h): the draws of sample_key(sample_seed, key) through that alias table instead, and the
  // augmentations keyed by the destination
  m.def(
      "mlp_augment",
      [](uintptr_t X0, uintptr_t labels0, uintptr_t X, uintptr_t labels, uintptr_t XT, uintptr_t Xs, uintptr_t Xw,
         uintptr_t XTw, uintptr_t perm, uintptr_t shifts, int N, int Pd, int es, int h, int w, int max_dx, int max_dy,
         uint32_t aug_seed, uint32_t key, int shuffled, uint32_t shuffle_seed, uintptr_t s, uintptr_t sample_table,
         uint32_t sample_seed) {
        cme::AugmentArgs aa;
        aa.base = gather_args(X0, labels0, X, labels, XT, Xs, Xw, XTw, perm, N, Pd, es,
                              cme::shuffle_key(shuffle_seed, key), shuffled || sample_table ? 0 : 1, sample_table,
                              sample_seed, key);
        aa.h = h; aa.w = w; aa.max_dx = max_dx; aa.max_dy = max_dy; aa.akey = cme::augment_key(aug_seed, key);
        aa.shifts = P<int>(shifts);
        cme::mlp_augment(aa, P<void>(s));
      },
      py::arg("X0"), py::arg("labels0"), py::arg("X"), py::arg("labels"), py::arg("XT"), py::arg("Xs"), py::arg("Xw"),
      py::arg("XTw"), py::arg("perm"), py::arg("shifts"), py::arg("N"), py::arg("P"), py::arg("es"), py::arg("h"),
      py::arg("w"), py::arg("max_dx"), py::arg("max_dy"), py::arg("aug_seed"), py::arg("key"),
      py::arg("shuffled") = 0, py::arg("shuffle_seed") = 0, py::arg("stream") = 0, py::arg("sample_table") = 0,
      py::arg("sample_seed") = 0);
  // the affine gather (csrc/mlp/affine.hip): mlp_augment's arguments, each image resampled through its table entry
  // (table: int32 [T][4] on the device; kind: 0 uint8, 1 bf16, 2 f32, 3 f64; transforms: int32 [N] or 0)
  m.def(
      "mlp_affine",
      [](uintptr_t X0, uintptr_t labels0, uintptr_t X, uintptr_t labels, uintptr_t XT, uintptr_t Xs, uintptr_t Xw,
         uintptr_t XTw, uintptr_t perm, uintptr_t shifts, uintptr_t transforms, uintptr_t table, int T, int kind, int N,
         int Pd, int es, int h, int w, int max_dx, int max_dy, uint32_t aug_seed, uint32_t key, int shuffled,
         uint32_t shuffle_seed, uintptr_t s, uintptr_t sample_table,
         uint32_t sample_seed) {
        cme::AffineArgs fa;
        cme::AugmentArgs& aa = fa.aug;
        aa.base = gather_args(X0, labels0, X, labels, XT, Xs, Xw, XTw, perm, N, Pd, es,
                              cme::shuffle_key(shuffle_seed, key), shuffled || sample_table ? 0 : 1, sample_table,
                              sample_seed, key);
        aa.h = h; aa.w = w; aa.max_dx = max_dx; aa.max_dy = max_dy; aa.akey = cme::augment_key(aug_seed, key);
        aa.shifts = P<int>(shifts);
        fa.table = P<const int32_t>(table); fa.T = T; fa.kind = kind; fa.transforms = P<int>(transforms);
        cme::mlp_affine(fa, P<void>(s));
      },
      py::arg("X0"), py::arg("labels0"), py::arg("X"), py::arg("labels"), py::arg("XT"), py::arg("Xs"), py::arg("Xw"),
      py::arg("XTw"), py::arg("perm"), py::arg("shifts"), py::arg("transforms"), py::arg("table"), py::arg("T"),
      py::arg("kind"), py::arg("N"), py::arg("P"), py::arg("es"), py::arg("h"), py::arg("w"), py::arg("max_dx"),
      py::arg("max_dy"), py::arg("aug_seed"), py::arg("key"), py::arg("shuffled") = 0, py::arg("shuffle_seed") = 0,
      py::arg("stream") = 0, py::arg("sample_table") = 0,
      py::arg("sample_seed") = 0);
  // the warping gather (csrc/mlp/warp.hip): mlp_affine's arguments, every source position moved by the sample's own
  // displacement field (axes: int32 [h + w][5] on the device; gy, gx: cells per axis; A: the nodes' bound in Q8)
  m.def(
      "mlp_warp",
      [](uintptr_t X0, uintptr_t labels0, uintptr_t X, uintptr_t labels, uintptr_t XT, uintptr_t Xs, uintptr_t Xw,
         uintptr_t XTw, uintptr_t perm, uintptr_t shifts, uintptr_t transforms, uintptr_t table, int T, int kind,
         uintptr_t axes, int gy, int gx, int A, int N, int Pd, int es, int h, int w, int max_dx, int max_dy,
         uint32_t aug_seed, uint32_t key, int shuffled, uint32_t shuffle_seed, uintptr_t s, uintptr_t sample_table,
         uint32_t sample_seed) {
        cme::WarpArgs wa;
        cme::AffineArgs& fa = wa.aff;
        cme::AugmentArgs& aa = fa.aug;
        aa.base = gather_args(X0, labels0, X, labels, XT, Xs, Xw, XTw, perm, N, Pd, es,
                              cme::shuffle_key(shuffle_seed, key), shuffled || sample_table ? 0 : 1, sample_table,
                              sample_seed, key);
        aa.h = h; aa.w = w; aa.max_dx = max_dx; aa.max_dy = max_dy; aa.akey = cme::augment_key(aug_seed, key);
        aa.shifts = P<int>(shifts);
        fa.table = P<const int32_t>(table); fa.T = T; fa.kind = kind; fa.transforms = P<int>(transforms);
        wa.axes = P<const int32_t>(axes); wa.gy = gy; wa.gx = gx; wa.A = A;
        cme::mlp_warp(wa, P<void>(s));
      },
      py::arg("X0"), py::arg("labels0"), py::arg("X"), py::arg("labels"), py::arg("XT"), py::arg("Xs"), py::arg("Xw"),
      py::arg("XTw"), py::arg("perm"), py::arg("shifts"), py::arg("transforms"), py::arg("table"), py::arg("T"),
      py::arg("kind"), py::arg("axes"), py::arg("gy"), py::arg("gx"), py::arg("A"), py::arg("N"), py::arg("P"),
      py::arg("es"), py::arg("h"), py::arg("w"), py::arg("max_dx"), py::arg("max_dy"), py::arg("aug_seed"),
      py::arg("key"), py::arg("shuffled") = 0, py::arg("shuffle_seed") = 0, py::arg("stream") = 0,
      py::arg("sample_table") = 0, py::arg("sample_seed") = 0);
  m.def("mlp_split_fused_tiles", &cme::mlp_split_fused_tiles, py::arg("P"), py::arg("H"), py::arg("cap"));
  // the stateful optimizer step (csrc/mlp/optim.h): kind 0 = momentum / Nesterov, 1 = adam; rec = optim_grid(count)
  // records of 4 doubles {t, b1^t, b2^t, 0}
  m.def("optim_grid", &cme::optim_grid, py::arg("count"));
  m.def(
      "optim_step",
      [](int dt, int kind, double lr, double mu, int nesterov, double beta1, double beta2, double eps,
         uintptr_t params, uintptr_t grads, uintptr_t s1, uintptr_t s2, int64_t count, uintptr_t planes, int np,
         int64_t w1n, uintptr_t status, uintptr_t rec, int nrec, uintptr_t s) {
        cme::OptimArgs a;
        a.dtype = dt; a.kind = kind;
        a.h.lr = lr; a.h.mu = mu; a.h.nesterov = nesterov; a.h.beta1 = beta1; a.h.beta2 = beta2; a.h.eps = eps;
        a.params = P<void>(params); a.grads = P<const void>(grads); a.s1 = P<void>(s1); a.s2 = P<void>(s2);
        a.count = count; a.planes = P<void>(planes); a.np = np; a.w1n = w1n; a.status = P<const void>(status);
        a.rec = P<double>(rec); a.nrec = nrec;
        cme::mlp_optim_step(a, P<void>(s));
      },
      py::arg("dt"), py::arg("kind"), py::arg("lr"), py::arg("mu"), py::arg("nesterov"), py::arg("beta1"),
      py::arg("beta2"), py::arg("eps"), py::arg("params"), py::arg("grads"), py::arg("s1"), py::arg("s2"),
      py::arg("count"), py::arg("planes") = 0, py::arg("np") = 0, py::arg("w1n") = 0, py::arg("status") = 0,
      py::arg("rec") = 0, py::arg("nrec") = 0, py::arg("stream") = 0);
  // the extended apply launch: optim_step's arguments by the same names, plus kind 2 = the stateless sgd rule (s1 = 0),
  // window = the schedule window {t0, n, f[0 .. n)} with room for wcap factors (0: the rate is lr), partials / npart /
  // clip_norm = the sum-of-squares partials of grad_sumsq and the threshold (clip_norm 0: no clipping), last = the
  // 4-double last-update record {t, lr_t, grad_norm, clip_coef} (0: none), plateau = the scale word of a plateau record
  // (0: none; trailing, so every earlier call keeps its signature)
  m.def(
      "optim_apply",
      [](int dt, int kind, double lr, double mu, int nesterov, double beta1, double beta2, double eps,
         uintptr_t params, uintptr_t grads, uintptr_t s1, uintptr_t s2, int64_t count, uintptr_t planes, int np,
         int64_t w1n, uintptr_t status, uintptr_t rec, int nrec, uintptr_t window, int wcap, uintptr_t partials,
         int npart, double clip_norm, uintptr_t last, uintptr_t s, uintptr_t plateau) {
        cme::OptimArgs a;
        a.dtype = dt; a.kind = kind;
        a.h.lr = lr; a.h.mu = mu; a.h.nesterov = nesterov; a.h.beta1 = beta1; a.h.beta2 = beta2; a.h.eps = eps;
        a.params = P<void>(params); a.grads = P<const void>(grads); a.s1 = P<void>(s1); a.s2 = P<void>(s2);
        a.count = count; a.planes = P<void>(planes); a.np = np; a.w1n = w1n; a.status = P<const void>(status);
        a.rec = P<double>(rec); a.nrec = nrec;
        cme::OptimExt x;
        x.window = P<const double>(window); x.wcap = wcap; x.partials = P<const double>(partials); x.npart = npart;
        x.clip_norm = clip_norm; x.last = P<double>(last); x.plateau = P<const double>(plateau);
        cme::mlp_optim_apply(a, x, P<void>(s));
      },
      py::arg("dt"), py::arg("kind"), py::arg("lr"), py::arg("mu"), py::arg("nesterov"), py::arg("beta1"),
      py::arg("beta2"), py::arg("eps"), py::arg("params"), py::arg("grads"), py::arg("s1"), py::arg("s2"),
      py::arg("count"), py::arg("planes") = 0, py::arg("np") = 0, py::arg("w1n") = 0, py::arg("status") = 0,
      py::arg("rec") = 0, py::arg("nrec") = 0, py::arg("window") = 0, py::arg("wcap") = 0, py::arg("partials") = 0,
      py::arg("npart") = 0, py::arg("clip_norm") = 0.0, py::arg("last") = 0, py::arg("stream") = 0, py::arg("plateau") = 0);
  // gradient-norm clipping (csrc/mlp/clip.h): the sum of squares of the segments [(offset, size), ...] of the bucket
  // (`arena` elements) into clip_grid(sum of sizes) partials
  m.def("clip_grid", &cme::clip_grid, py::arg("count"));
  m.def(
      "grad_sumsq",
      [](int dt, uintptr_t grads, int64_t arena, std::vector<std::pair<int64_t, int64_t>> segments, uintptr_t partials,
         int npart, uintptr_t s) {
        if (segments.empty() || segments.size() > cme::kClipMaxSegs)
          throw std::invalid_argument("grad_sumsq: 1 .. 4 (offset, size) segments");
        cme::ClipSegs sg;
        sg.n = static_cast<int>(segments.size());
        for (int i = 0; i < sg.n; ++i) { sg.off[i] = segments[i].first; sg.size[i] = segments[i].second; }
        cme::mlp_grad_sumsq(dt, P<const void>(grads), arena, sg, P<double>(partials), npart, P<void>(s));
      },
      py::arg("dt"), py::arg("grads"), py::arg("arena"), py::arg("segments"), py::arg("partials"), py::arg("npart"),
      py::arg("stream") = 0);
  // keeping the best validation weights (csrc/mlp/best.h): one launch behind an evaluation; rec = best_grid(count)
  // records of 8 doubles; exactly one of slot (a stats slot of eval.h) and rows ([R][3] doubles) is non-zero
  m.def("best_grid", &cme::best_grid, py::arg("count"));
  m.def(
      "mlp_keep_best",
      [](int dt, int monitor, double min_delta, int patience, uintptr_t params, uintptr_t best, int64_t count,
         uintptr_t rec, int nrec, uintptr_t slot, uintptr_t rows, int R, uintptr_t s) {
        cme::BestArgs a;
        a.dtype = dt; a.rule.monitor = monitor; a.rule.min_delta = min_delta; a.rule.patience = patience;
        a.params = P<const void>(params); a.best = P<void>(best); a.count = count; a.rec = P<double>(rec);
        a.nrec = nrec; a.slot = P<const unsigned long long>(slot); a.rows = P<const double>(rows); a.R = R;
        cme::mlp_keep_best(a, P<void>(s));
      },
      py::arg("dt"), py::arg("monitor"), py::arg("min_delta"), py::arg("patience"), py::arg("params"), py::arg("best"),
      py::arg("count"), py::arg("rec"), py::arg("nrec"), py::arg("slot") = 0, py::arg("rows") = 0, py::arg("R") = 1,
      py::arg("stream") = 0);
  m.def(
      "mlp_best_pack",
      [](uintptr_t slot, uintptr_t rows, int R, int rank, uintptr_t s) {
        cme::mlp_best_pack(P<const unsigned long long>(slot), P<double>(rows), R, rank, P<void>(s));
      },
      py::arg("slot"), py::arg("rows"), py::arg("R"), py::arg("rank"), py::arg("stream") = 0);
  // reduce on plateau (csrc/mlp/plateau.h): one launch behind an evaluation advances the one record of 8 doubles;
  // exactly one of slot (a stats slot of eval.h) and rows ([R][3] doubles) is non-zero.  plateau_scale_word: the index
  // of the record's word the apply launch reads
  m.attr("plateau_scale_word") = cme::kPlateauScaleWord;
  m.def(
      "mlp_plateau",
      [](int monitor, double factor, int patience, double threshold, int threshold_mode, int cooldown,
         double min_factor, double eps, uintptr_t rec, uintptr_t slot, uintptr_t rows, int R, uintptr_t s) {
        cme::PlateauArgs a;
        a.rule = {monitor, factor, patience, threshold, threshold_mode, cooldown, min_factor, eps};
        a.rec = P<double>(rec); a.slot = P<const unsigned long long>(slot); a.rows = P<const double>(rows); a.R = R;
        cme::mlp_plateau(a, P<void>(s));
      },
      py::arg("monitor"), py::arg("factor"), py::arg("patience"), py::arg("threshold"), py::arg("threshold_mode"),
      py::arg("cooldown"), py::arg("min_factor"), py::arg("eps"), py::arg("rec"), py::arg("slot") = 0,
      py::arg("rows") = 0, py::arg("R") = 1, py::arg("stream") = 0);
  // the exponential moving average of the parameters (csrc/mlp/ema.h): one launch behind every applied update; rec =
  // ema_grid(count) records of 4 doubles; status (the parameter dtype) and err (int32) are the optional skip words
  m.def("ema_grid", &cme::ema_grid, py::arg("count"));
  m.def(
      "mlp_ema_step",
      [](int dt, double decay, int warmup, uintptr_t params, uintptr_t ema, int64_t count, uintptr_t rec, int nrec,
         uintptr_t status, uintptr_t err, uintptr_t s) {
        cme::EmaArgs a;
        a.dtype = dt; a.rule.decay = decay; a.rule.warmup = warmup;
        a.params = P<const void>(params); a.ema = P<void>(ema); a.count = count; a.rec = P<double>(rec);
        a.nrec = nrec; a.status = P<const void>(status); a.err = P<const int32_t>(err);
        cme::mlp_ema_step(a, P<void>(s));
      },
      py::arg("dt"), py::arg("decay"), py::arg("warmup"), py::arg("params"), py::arg("ema"), py::arg("count"),
      py::arg("rec"), py::arg("nrec"), py::arg("status") = 0, py::arg("err") = 0, py::arg("stream") = 0);

  bind_suite(m);
  bind_comm(m);
}
