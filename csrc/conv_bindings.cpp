// Torch bindings for the conv torso kernels (see kernels/conv_torso.hip).
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <c10/core/DeviceGuard.h>

#include <climits>

#include "kernels/conv_launchers.h"

namespace {

hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }

void check_act(const at::Tensor& t, const char* name, int64_t C) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous(), name, " must be a contiguous GPU tensor");
  TORCH_CHECK(t.dim() == 4 && t.size(3) == C, name, " must be NHWC with C=", C);
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, name, " must be bfloat16");
  // validated sizes (and the largest learner chunk: ops/conv_f32.py
  // MAX_FRAMES); an oversized call fails here instead of computing garbage
  TORCH_CHECK(t.numel() * 2 < (int64_t{1} << 32), name, " is ", t.numel() * 2,
              " bytes: bf16 conv tensors must stay under 4 GB (chunk the frames)");
}
void check_w(const at::Tensor& w, const at::Tensor& b, int64_t cin, int64_t cout) {
  TORCH_CHECK(w.is_cuda() && w.is_contiguous() && w.scalar_type() == at::kFloat,
              "weights must be contiguous fp32 GPU");
  TORCH_CHECK(w.dim() == 4 && w.size(0) == 3 && w.size(1) == 3 && w.size(2) == cin &&
              w.size(3) == cout, "weights must be [3,3,", cin, ",", cout, "]");
  TORCH_CHECK(b.numel() == cout && b.scalar_type() == at::kFloat && b.is_contiguous(),
              "bias must be fp32 [cout]");
}
void check_grad(const at::Tensor& dw, const at::Tensor& db, int64_t cin, int64_t cout) {
  TORCH_CHECK(dw.is_contiguous() && dw.scalar_type() == at::kFloat &&
              dw.numel() == 9 * cin * cout, "dw must be fp32 [3,3,cin,cout]");
  TORCH_CHECK(db.is_contiguous() && db.scalar_type() == at::kFloat && db.numel() == cout,
              "db must be fp32 [cout]");
}
bool supported(int64_t c) { return c == 16 || c == 32; }

// Deterministic mode: a stream-ordered slot workspace for the wgrad flush
// (empty when the mode is off).
at::Tensor wgrad_part(const at::Tensor& like, int64_t cin, int64_t cout, bool conv1) {
  const int64_t n = sa::conv::wgrad_part_floats((int)cin, (int)cout, conv1);
  return n ? at::empty({n}, like.options()) : at::Tensor();
}
float* ptr_or_null(const at::Tensor& t) { return t.defined() ? t.data_ptr<float>() : nullptr; }

std::vector<at::Tensor> conv1_pool_fwd(at::Tensor x, at::Tensor w, at::Tensor b,
                                       int64_t pb_h, int64_t pb_w) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.scalar_type() == at::kByte &&
              x.dim() == 4 && (x.size(3) == 3 || x.size(3) == 4),
              "frames must be uint8 NHWC with C = 3 or 4");
  const int64_t C = x.size(3);
  check_w(w, b, C, 16);
  const c10::DeviceGuard g(x.device());
  const int64_t N = x.size(0), H = x.size(1), W = x.size(2);
  const int64_t Hp = (H + 1) / 2, Wo = (W + 1) / 2;
  auto pooled = at::empty({N, Hp, Wo, 16}, x.options().dtype(at::kBFloat16));
  auto arg = at::empty({N, Hp, Wo, 16}, x.options());
  sa::conv::conv1_pool_fwd_launch(x.data_ptr<uint8_t>(), w.data_ptr<float>(),
                                  b.data_ptr<float>(), pooled.data_ptr(),
                                  arg.data_ptr<uint8_t>(), N, H, W, C, pb_h, pb_w,
                                  stream());
  return {pooled, arg};
}

std::vector<at::Tensor> conv_pool_fwd(at::Tensor x, at::Tensor w, at::Tensor b,
                                      int64_t pb_h, int64_t pb_w) {
  const int64_t CIN = x.size(3), COUT = w.size(3);
  TORCH_CHECK(supported(CIN) && supported(COUT), "channels must be 16/32");
  check_act(x, "x", CIN);
  check_w(w, b, CIN, COUT);
  TORCH_CHECK(!(CIN == 32 && COUT == 16), "32->16 not instantiated");
  const c10::DeviceGuard g(x.device());
  const int64_t N = x.size(0), H = x.size(1), W = x.size(2);
  const int64_t Hp = (H + 1) / 2, Wo = (W + 1) / 2;
  auto pooled = at::empty({N, Hp, Wo, COUT}, x.options());
  auto arg = at::empty({N, Hp, Wo, COUT}, x.options().dtype(at::kByte));
  sa::conv::conv_pool_fwd_launch(x.data_ptr(), w.data_ptr<float>(), b.data_ptr<float>(),
                                 pooled.data_ptr(), arg.data_ptr<uint8_t>(), N, H, W,
                                 CIN, COUT, pb_h, pb_w, stream());
  return {pooled, arg};
}

// y = conv(relu_in ? relu(x) : x) + b [+ resid] [then relu]
at::Tensor res_conv_fwd(at::Tensor x, at::Tensor w, at::Tensor b,
                        c10::optional<at::Tensor> resid, bool post_relu,
                        bool relu_in) {
  const int64_t C = x.size(3);
  TORCH_CHECK(supported(C), "channels must be 16/32");
  check_act(x, "x", C);
  check_w(w, b, C, C);
  const void* rp = nullptr;
  if (resid.has_value() && resid->defined()) {
    check_act(*resid, "resid", C);
    TORCH_CHECK(resid->sizes() == x.sizes(), "resid shape");
    rp = resid->data_ptr();
  }
  const c10::DeviceGuard g(x.device());
  auto y = at::empty_like(x);
  sa::conv::res_conv_fwd_launch(x.data_ptr(), w.data_ptr<float>(), b.data_ptr<float>(),
                                rp, y.data_ptr(), x.size(0), x.size(1), x.size(2), C,
                                post_relu, relu_in, stream());
  return y;
}

// -> {t, y}: t = relu(conv1(relu(x)) + b1), y = conv2(t) + b2 + x [+ relu]
std::vector<at::Tensor> res_block_fwd(at::Tensor x, at::Tensor w1, at::Tensor b1,
                                      at::Tensor w2, at::Tensor b2, bool post_relu) {
  const int64_t C = x.size(3);
  TORCH_CHECK(supported(C), "channels must be 16/32");
  check_act(x, "x", C);
  check_w(w1, b1, C, C);
  check_w(w2, b2, C, C);
  const c10::DeviceGuard g(x.device());
  auto t = at::empty_like(x);
  auto y = at::empty_like(x);
  sa::conv::res_block_fwd_launch(x.data_ptr(), w1.data_ptr<float>(), b1.data_ptr<float>(),
                                 w2.data_ptr<float>(), b2.data_ptr<float>(), t.data_ptr(),
                                 y.data_ptr(), x.size(0), x.size(1), x.size(2), C,
                                 post_relu, stream());
  return {t, y};
}

// ---- one-launch stages of the no-grad forward (stage_fwd_kernel) ----
int stage_form(const at::Tensor& x, int64_t cin, int64_t cout) {
  const int64_t N = x.size(0), H = x.size(1), W = x.size(2);
  if (N > INT_MAX || H > INT_MAX || W > INT_MAX) return 0;
  return sa::conv::stage_bf16_form(static_cast<int>(N), static_cast<int>(H),
                                   static_cast<int>(W), static_cast<int>(cin),
                                   static_cast<int>(cout));
}

at::Tensor stage_launch(const at::Tensor& x, const at::Tensor* w, const at::Tensor* b,
                        const at::Tensor* const blk[8], int64_t C, int64_t pb_h,
                        int64_t pb_w, bool last, const char* name) {
  const int64_t CIN = x.size(3);
  const float* wb[8];
  for (int i = 0; i < 8; i += 2) {
    check_w(*blk[i], *blk[i + 1], C, C);
    TORCH_CHECK(blk[i + 1]->is_cuda(), "bias must be on the GPU");
    wb[i] = blk[i]->data_ptr<float>();
    wb[i + 1] = blk[i + 1]->data_ptr<float>();
  }
  if (w) TORCH_CHECK(b->is_cuda(), "bias must be on the GPU");
  const int64_t N = x.size(0), H = x.size(1), W = x.size(2);
  // the pool's pad_before is 0 or 1 (TF SAME, 3x3/2); an odd width needs 1
  TORCH_CHECK(pb_h >= 0 && pb_h <= 1 && pb_w >= (w ? (W & 1) : 0) && pb_w <= 1,
              name, ": pb_h / pb_w must be the TF-SAME pad_before of the 3x3/2 pool");
  TORCH_CHECK(stage_form(x, CIN, C) == (w ? 1 : 2), name, ": no one-launch form for ", N,
              " maps of ", H, "x", W, "x", CIN, " -> ", C, " channels");
  const c10::DeviceGuard g(x.device());
  auto y = w ? at::empty({N, (H + 1) / 2, (W + 1) / 2, C}, x.options()) : at::empty_like(x);
  sa::conv::stage_bf16_fwd_launch(x.data_ptr(), w ? w->data_ptr<float>() : nullptr,
                                  w ? b->data_ptr<float>() : nullptr, wb, y.data_ptr(),
                                  static_cast<int>(N), static_cast<int>(H),
                                  static_cast<int>(W), static_cast<int>(CIN),
                                  static_cast<int>(C), static_cast<int>(pb_h),
                                  static_cast<int>(pb_w), last, stream());
  const hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, name, ": launch failed: ", hipGetErrorString(e));
  return y;
}

// y = the stage's output: conv(x, w) + b -> max-pool -> two residual blocks
// [+ final relu]; bitwise conv_pool_fwd + two res_block_fwd
at::Tensor stage_bf16_fwd(at::Tensor x, at::Tensor w, at::Tensor b, at::Tensor w1,
                          at::Tensor b1, at::Tensor w2, at::Tensor b2, at::Tensor w3,
                          at::Tensor b3, at::Tensor w4, at::Tensor b4, int64_t pb_h,
                          int64_t pb_w, bool last) {
  TORCH_CHECK(x.dim() == 4 && w.dim() == 4, "stage_bf16_fwd: x must be NHWC, w HWIO");
  const int64_t CIN = x.size(3), COUT = w.size(3);
  TORCH_CHECK(supported(CIN) && COUT == 32, "stage_bf16_fwd: channels must be 16/32 -> 32");
  check_act(x, "x", CIN);
  check_w(w, b, CIN, COUT);
  const at::Tensor* blk[8] = {&w1, &b1, &w2, &b2, &w3, &b3, &w4, &b4};
  return stage_launch(x, &w, &b, blk, COUT, pb_h, pb_w, last, "stage_bf16_fwd");
}

// y = two residual blocks [+ final relu] of a pooled 16-channel map
at::Tensor stage_tail_bf16_fwd(at::Tensor x, at::Tensor w1, at::Tensor b1, at::Tensor w2,
                               at::Tensor b2, at::Tensor w3, at::Tensor b3, at::Tensor w4,
                               at::Tensor b4, bool last) {
  TORCH_CHECK(x.dim() == 4 && x.size(3) == 16, "stage_tail_bf16_fwd: x must be NHWC, C = 16");
  check_act(x, "x", 16);
  const at::Tensor* blk[8] = {&w1, &b1, &w2, &b2, &w3, &b3, &w4, &b4};
  return stage_launch(x, nullptr, nullptr, blk, 16, 0, 0, last, "stage_tail_bf16_fwd");
}

// dx = [skip +] dgrad(dy) * (act > 0); dW += relu?(act)^T dy; db += sum dy
at::Tensor res_conv_bwd(at::Tensor dy, at::Tensor act, c10::optional<at::Tensor> skip,
                        at::Tensor w, at::Tensor dw, at::Tensor db, bool relu_act) {
  const int64_t C = act.size(3);
  TORCH_CHECK(supported(C), "channels must be 16/32");
  check_act(dy, "dy", C);
  check_act(act, "act", C);
  TORCH_CHECK(dy.sizes() == act.sizes(), "dy/act shape");
  TORCH_CHECK(w.is_contiguous() && w.scalar_type() == at::kFloat && w.numel() == 9 * C * C,
              "w");
  check_grad(dw, db, C, C);
  const void* sp = nullptr;
  if (skip.has_value() && skip->defined()) {
    check_act(*skip, "skip", C);
    sp = skip->data_ptr();
  }
  const c10::DeviceGuard g(dy.device());
  auto dx = at::empty_like(act);
  auto part = wgrad_part(dw, C, C, false);
  sa::conv::res_conv_bwd_launch(dy.data_ptr(), act.data_ptr(), sp, w.data_ptr<float>(),
                                dx.data_ptr(), dw.data_ptr<float>(), db.data_ptr<float>(),
                                act.size(0), act.size(1), act.size(2), C, relu_act,
                                stream(), ptr_or_null(part));
  return dx;
}

c10::optional<at::Tensor> pool_conv_bwd(at::Tensor dP, at::Tensor arg, at::Tensor x,
                                        at::Tensor w, at::Tensor dw, at::Tensor db,
                                        bool need_dx, int64_t pb_h, int64_t pb_w) {
  const int64_t CIN = x.size(3), COUT = dP.size(3);
  TORCH_CHECK(supported(CIN) && supported(COUT), "channels must be 16/32");
  TORCH_CHECK(!(CIN == 32 && COUT == 16), "32->16 not instantiated");
  check_act(x, "x", CIN);
  check_act(dP, "dP", COUT);
  TORCH_CHECK(arg.sizes() == dP.sizes() && arg.scalar_type() == at::kByte &&
              arg.is_contiguous(), "argmax");
  TORCH_CHECK(dP.size(1) == (x.size(1) + 1) / 2 && dP.size(2) == (x.size(2) + 1) / 2,
              "pooled shape");
  TORCH_CHECK(w.numel() == 9 * CIN * COUT && w.scalar_type() == at::kFloat, "w");
  check_grad(dw, db, CIN, COUT);
  const c10::DeviceGuard g(x.device());
  c10::optional<at::Tensor> dx;
  void* dxp = nullptr;
  if (need_dx) {
    dx = at::empty_like(x);
    dxp = dx->data_ptr();
  }
  auto part = wgrad_part(dw, CIN, COUT, false);
  sa::conv::pool_conv_bwd_launch(dP.data_ptr(), arg.data_ptr<uint8_t>(), x.data_ptr(),
                                 w.data_ptr<float>(), dxp, dw.data_ptr<float>(),
                                 db.data_ptr<float>(), x.size(0), x.size(1), x.size(2),
                                 CIN, COUT, pb_h, pb_w, stream(), ptr_or_null(part));
  return dx;
}

void conv1_pool_bwd(at::Tensor dP, at::Tensor arg, at::Tensor x, at::Tensor dw,
                    at::Tensor db, int64_t pb_h, int64_t pb_w) {
  TORCH_CHECK(x.scalar_type() == at::kByte && x.dim() == 4 &&
              (x.size(3) == 3 || x.size(3) == 4) && x.is_contiguous(), "frames");
  const int64_t C = x.size(3);
  check_act(dP, "dP", 16);
  TORCH_CHECK(arg.sizes() == dP.sizes() && arg.scalar_type() == at::kByte, "argmax");
  TORCH_CHECK(dP.size(1) == (x.size(1) + 1) / 2 && dP.size(2) == (x.size(2) + 1) / 2,
              "pooled shape");
  check_grad(dw, db, C, 16);
  const c10::DeviceGuard g(x.device());
  auto part = wgrad_part(dw, C, 16, true);
  sa::conv::conv1_pool_bwd_launch(dP.data_ptr(), arg.data_ptr<uint8_t>(),
                                  x.data_ptr<uint8_t>(), dw.data_ptr<float>(),
                                  db.data_ptr<float>(), x.size(0), x.size(1),
                                  x.size(2), C, pb_h, pb_w, stream(), ptr_or_null(part));
}

// ---- the shallow torso on bf16 MFMA (kernels/conv_shallow_bf16.hip) ----
constexpr int64_t kSbSteps[3] = {8, 16, 18};    // K = 32 steps per layer
constexpr int64_t kSbCout[3] = {32, 64, 128};

// fp32 HWIO w1 [8,8,C<=4,32], w2 [4,4,32,64], w3 [3,3,64,128] -> the kernel's
// bf16 B-operand layout [kstep][ntile][lane][8] (w1 zero-padded to 4 input
// channels; one RNE rounding).  Off the hot path: once per weight publish.
std::vector<at::Tensor> shallow_bf16_pack(at::Tensor w1, at::Tensor w2, at::Tensor w3) {
  const at::Tensor* ws[3] = {&w1, &w2, &w3};
  const int64_t dims[3][2] = {{8, -1}, {4, 32}, {3, 64}};
  std::vector<at::Tensor> out;
  for (int i = 0; i < 3; ++i) {
    const at::Tensor& w = *ws[i];
    TORCH_CHECK(w.dim() == 4 && w.scalar_type() == at::kFloat && w.size(0) == dims[i][0] &&
                    w.size(1) == dims[i][0] && w.size(3) == kSbCout[i] &&
                    (i == 0 ? (w.size(2) >= 1 && w.size(2) <= 4) : w.size(2) == dims[i][1]),
                "shallow_bf16_pack: layer ", i + 1, " weights must be fp32 HWIO [", dims[i][0],
                ",", dims[i][0], ",", (i == 0 ? "C<=4" : (i == 1 ? "32" : "64")), ",",
                kSbCout[i], "]");
    at::Tensor f = w.detach();
    if (i == 0 && f.size(2) != 4) f = at::constant_pad_nd(f, {0, 0, 0, 4 - f.size(2)}, 0);
    // [K, cout] -> (kstep, g, j, ntile, m) -> (kstep, ntile, g, m, j); lane = 16 g + m
    f = f.reshape({kSbSteps[i], 4, 8, kSbCout[i] / 16, 16}).permute({0, 3, 1, 4, 2});
    out.push_back(f.to(at::kBFloat16).contiguous().reshape({-1}));
  }
  return out;
}

at::Tensor shallow_bf16_fwd(at::Tensor x, at::Tensor w1p, at::Tensor b1, at::Tensor w2p,
                            at::Tensor b2, at::Tensor w3p, at::Tensor b3) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 4,
              "shallow_bf16_fwd: frames must be a contiguous NHWC GPU tensor");
  TORCH_CHECK(x.scalar_type() == at::kByte, "shallow_bf16_fwd: frames must be uint8 NHWC");
  const int64_t N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  const at::Tensor* ws[3] = {&w1p, &w2p, &w3p};
  const at::Tensor* bs[3] = {&b1, &b2, &b3};
  for (int i = 0; i < 3; ++i) {
    const int64_t want = kSbSteps[i] * 32 * kSbCout[i];
    TORCH_CHECK(ws[i]->is_cuda() && ws[i]->is_contiguous() &&
                    ws[i]->scalar_type() == at::kBFloat16 && ws[i]->numel() == want,
                "shallow_bf16_fwd: layer ", i + 1, " packed weights must be ", want,
                " contiguous bf16 on the GPU (shallow_bf16_pack)");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(ws[i]->data_ptr()) % 16 == 0,
                "shallow_bf16_fwd: packed weights must be 16-byte aligned");
    TORCH_CHECK(bs[i]->is_cuda() && bs[i]->scalar_type() == at::kFloat &&
                    bs[i]->is_contiguous() && bs[i]->numel() == kSbCout[i],
                "shallow_bf16_fwd: layer ", i + 1, " bias must be fp32 [", kSbCout[i], "]");
  }
  TORCH_CHECK(N <= INT_MAX && H <= INT_MAX && W <= INT_MAX && C <= INT_MAX &&
                  sa::conv::shallow_bf16_form(static_cast<int>(N), static_cast<int>(H),
                                              static_cast<int>(W), static_cast<int>(C)),
              "shallow_bf16_fwd: no kernel for ", N, " frames of ", H, "x", W, "x", C);
  const c10::DeviceGuard g(x.device());
  const int64_t H1 = (H + 3) / 4, W1 = (W + 3) / 4, H2 = (H1 + 1) / 2, W2 = (W1 + 1) / 2;
  auto y = at::empty({N, (H2 + 1) / 2, (W2 + 1) / 2, 128}, x.options().dtype(at::kBFloat16));
  TORCH_CHECK(sa::conv::shallow_bf16_fwd_launch(
                  x.data_ptr<uint8_t>(), w1p.data_ptr(), b1.data_ptr<float>(), w2p.data_ptr(),
                  b2.data_ptr<float>(), w3p.data_ptr(), b3.data_ptr<float>(), y.data_ptr(),
                  static_cast<int>(N), static_cast<int>(H), static_cast<int>(W),
                  static_cast<int>(C), stream()),
              "shallow_bf16_fwd: frames must be 4-byte aligned");
  const hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "shallow_bf16_fwd: launch failed: ", hipGetErrorString(e));
  return y;
}

}  // namespace

void register_conv_ops(pybind11::module& m) {
  m.def("conv1_pool_fwd", &conv1_pool_fwd);
  m.def("conv_pool_fwd", &conv_pool_fwd);
  m.def("res_block_fwd", &res_block_fwd);
  m.def("res_conv_fwd", &res_conv_fwd, pybind11::arg("x"), pybind11::arg("w"),
        pybind11::arg("b"), pybind11::arg("resid") = pybind11::none(),
        pybind11::arg("post_relu") = false, pybind11::arg("relu_in") = true);
  m.def("res_conv_bwd", &res_conv_bwd, pybind11::arg("dy"), pybind11::arg("act"),
        pybind11::arg("skip"), pybind11::arg("w"), pybind11::arg("dw"),
        pybind11::arg("db"), pybind11::arg("relu_act") = true);
  m.def("pool_conv_bwd", &pool_conv_bwd);
  m.def("conv1_pool_bwd", &conv1_pool_bwd);
  m.def("shallow_bf16_fwd", &shallow_bf16_fwd, pybind11::arg("frames"), pybind11::arg("w1p"),
        pybind11::arg("b1"), pybind11::arg("w2p"), pybind11::arg("b2"), pybind11::arg("w3p"),
        pybind11::arg("b3"));
  m.def("shallow_bf16_pack", &shallow_bf16_pack);
  // 1 where shallow_bf16_fwd takes N uint8 frames of [H, W, C], else 0
  m.def("shallow_bf16_form",
        [](int N, int H, int W, int C) { return sa::conv::shallow_bf16_form(N, H, W, C); });
  m.def("stage_bf16_fwd", &stage_bf16_fwd, pybind11::arg("x"), pybind11::arg("w"),
        pybind11::arg("b"), pybind11::arg("w1"), pybind11::arg("b1"), pybind11::arg("w2"),
        pybind11::arg("b2"), pybind11::arg("w3"), pybind11::arg("b3"), pybind11::arg("w4"),
        pybind11::arg("b4"), pybind11::arg("pb_h"), pybind11::arg("pb_w"),
        pybind11::arg("last"));
  m.def("stage_tail_bf16_fwd", &stage_tail_bf16_fwd, pybind11::arg("x"),
        pybind11::arg("w1"), pybind11::arg("b1"), pybind11::arg("w2"), pybind11::arg("b2"),
        pybind11::arg("w3"), pybind11::arg("b3"), pybind11::arg("w4"), pybind11::arg("b4"),
        pybind11::arg("last"));
  // 0, 1 (stage: [frames,H,W,CIN] input, CIN -> COUT = 32) or 2 (tail: a pooled
  // [frames,H,W,16] map, CIN == COUT == 16); host arithmetic only
  m.def("stage_bf16_form", [](int frames, int H, int W, int CIN, int COUT) {
          return sa::conv::stage_bf16_form(frames, H, W, CIN, COUT);
        }, pybind11::arg("frames"), pybind11::arg("H"), pybind11::arg("W"),
        pybind11::arg("CIN"), pybind11::arg("COUT"));
  // read-only record of a family's last launch ("" = the most recent one)
  m.def("conv_launch_info", [](const std::string& family) {
          const sa::conv::LaunchInfo i = sa::conv::launch_info(family.c_str());
          pybind11::dict d;
          d["family"] = std::string(i.family);
          d["grid"] = i.grid;
          d["grid_max"] = i.grid_max;
          d["ntiles"] = i.ntiles;
          d["rows"] = i.rows;
          d["specialized"] = i.specialized;
          return d;
        }, pybind11::arg("family") = "");
  m.def("conv_tune", [](const std::string& key, int64_t value) {
          return sa::conv::conv_tune_set(key.c_str(), static_cast<int>(value));
        }, pybind11::arg("key"), pybind11::arg("value") = -1);
}
