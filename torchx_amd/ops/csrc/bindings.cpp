// Torch extension bindings for the torchx_amd CDNA4 kernels.
// Compiled with hipcc for gfx950; no CUDA paths, no multi-backend dispatch.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include <hip/hip_runtime.h>

extern "C" {
void rope_launch(const void*, void*, const void*, const void*, long, int, int,
                 int, float, hipStream_t);
void swiglu_fwd_launch(const void*, const void*, void*, long, hipStream_t);
void swiglu_bwd_launch(const void*, const void*, const void*, void*, void*,
                       long, hipStream_t);
void rmsnorm_fwd_launch(const void*, const void*, void*, void*, long, int,
                        float, hipStream_t);
void rmsnorm_bwd_launch(const void*, const void*, const void*, const void*,
                        const void*, void*, void*, void*, long, int,
                        hipStream_t);
long rmsnorm_bwd_dw_chunks(long);
void adamw_launch(void*, void*, const void*, void*, void*, long, float, float,
                  float, float, float, float, float, hipStream_t);
void ce_fwd_launch(const void*, const void*, void*, void*, long, int,
                   hipStream_t);
void ce_bwd_launch(const void*, const void*, const void*, const void*, void*,
                   long, int, hipStream_t);
void attn_fwd_launch(const void*, const void*, const void*, void*, void*, int,
                     int, int, int, float, int, long, long, hipStream_t);
void attn_bwd_launch(const void*, const void*, const void*, const void*,
                     const void*, const void*, void*, void*, void*, void*,
                     void*, int, int, int, int, float, int, long, long, long,
                     long, hipStream_t);
long attn_bwd_ds_bytes(int, int, int, int);
int attn_bwd_dkv_impl_get();
void attn_bwd_dkv_impl_set(int);
int attn_fwd_map_get();
void attn_fwd_map_set(int);
void rope_qkv_launch(const void*, void*, const void*, const void*, long, int,
                     long, int, float, hipStream_t);
void swiglu_gu_fwd_launch(const void*, void*, long, long, hipStream_t);
void swiglu_gu_bwd_launch(const void*, const void*, void*, long, long,
                          hipStream_t);
void swiglu_gu_bwd_t_launch(const void*, const void*, void*, void*, long,
                            long, hipStream_t);
void mfma_probe_launch(const void*, const void*, void*, hipStream_t);
void mfma_probe_tr_launch(const void*, const void*, void*, void*,
                          hipStream_t);
void fp8_cast_transpose_launch(const void*, void*, void*, void*,
                               const void*, long, long, int, hipStream_t);
void transpose_bf16_launch(const void*, void*, long, long, hipStream_t);
void decode_attn_launch(const void*, const void*, const void*, void*,
                        const void*, int, int, int, int, int, int, float,
                        hipStream_t);
void gemv_bf16_launch(const void*, const void*, void*, int, int, int,
                      hipStream_t);
void decode_attn_split_launch(const void*, const void*, const void*, void*,
                              void*, void*, const void*, int, int, int, int,
                              int, int, int, float, hipStream_t);
void decode_rope_cache_launch(const void*, void*, void*, void*, const void*,
                              const void*, const void*, int, int, int, int,
                              int, int, hipStream_t);
void rmsnorm_res_launch(const void*, const void*, const void*, void*, void*,
                        void*, long, int, float, hipStream_t);
void gemv_swiglu_launch(const void*, const void*, void*, int, int, int,
                        hipStream_t);
void paged_decode_attn_launch(const void*, const void*, const void*, void*,
                              void*, void*, const void*, const void*, int,
                              int, int, int, int, int, int, float,
                              hipStream_t);
void paged_decode_rope_cache_launch(const void*, void*, void*, void*,
                                    const void*, const void*, const void*,
                                    const void*, int, int, int, int, int,
                                    int, int, hipStream_t);
void paged_prefill_attn_launch(const void*, const void*, const void*, void*,
                               const void*, const void*, int, int, int, int,
                               int, int, int, float, hipStream_t);
void paged_prefill_attn_ragged_launch(const void*, const void*, const void*,
                                      void*, const void*, const void*,
                                      const void*, int, int, int, int, int,
                                      int, int, int, float, hipStream_t);
void paged_prefill_rope_cache_launch(const void*, void*, void*, void*,
                                     const void*, const void*, const void*,
                                     const void*, long, int, int, long, int,
                                     hipStream_t);
}

namespace {

hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

void check_bf16(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

void check_f32(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == at::kFloat, name, " must be f32");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

}  // namespace

// ---- RMSNorm --------------------------------------------------------------
std::vector<at::Tensor> rmsnorm_fwd(at::Tensor x, at::Tensor w, double eps) {
  check_bf16(x, "x");
  check_bf16(w, "w");
  const long H = x.size(-1);
  TORCH_CHECK(H % 2048 == 0 && H <= 8192, "rmsnorm: H must be k*2048, <=8192");
  const long rows = x.numel() / H;
  auto y = at::empty_like(x);
  auto invrms = at::empty({rows}, x.options().dtype(at::kFloat));
  rmsnorm_fwd_launch(x.data_ptr(), w.data_ptr(), y.data_ptr(),
                     invrms.data_ptr(), rows, (int)H, (float)eps,
                     cur_stream());
  return {y, invrms};
}

// dres (optional): the gradient that reaches the norm's input along the
// residual stream; dx is then bf16(dx) + dres, the bits of the separate
// accumulate-add (add_rmsnorm backward).
std::vector<at::Tensor> rmsnorm_bwd(at::Tensor dy, at::Tensor x, at::Tensor w,
                                    at::Tensor invrms,
                                    c10::optional<at::Tensor> dres) {
  check_bf16(dy, "dy");
  check_bf16(x, "x");
  check_bf16(w, "w");
  check_f32(invrms, "invrms");
  const long H = x.size(-1);
  TORCH_CHECK(H % 2048 == 0 && H <= 8192, "rmsnorm: H must be k*2048, <=8192");
  const long rows = x.numel() / H;
  TORCH_CHECK(dy.sizes() == x.sizes(), "dy shape mismatch");
  TORCH_CHECK(w.numel() == H && invrms.numel() == rows,
              "w / invrms size mismatch");
  const void* rp = nullptr;
  if (dres.has_value()) {
    check_bf16(*dres, "dres");
    TORCH_CHECK(dres->sizes() == x.sizes(), "dres shape mismatch");
    rp = dres->data_ptr();
  }
  auto dx = at::empty_like(x);
  auto dw = at::empty({H}, x.options().dtype(at::kFloat));
  // per-row-chunk partial sums of dw, reduced in a fixed order
  auto dw_part = at::empty({rmsnorm_bwd_dw_chunks(rows), H}, dw.options());
  rmsnorm_bwd_launch(dy.data_ptr(), x.data_ptr(), w.data_ptr(),
                     invrms.data_ptr(), rp, dx.data_ptr(), dw.data_ptr(),
                     dw_part.data_ptr(), rows, (int)H, cur_stream());
  return {dx, dw};
}

// ---- RoPE -----------------------------------------------------------------
at::Tensor rope(at::Tensor x, at::Tensor cos_t, at::Tensor sin_t, long heads,
                double sign) {
  check_bf16(x, "x");
  check_f32(cos_t, "cos");
  check_f32(sin_t, "sin");
  const long D = x.size(-1);
  const long rows = x.numel() / D;
  const long S = cos_t.size(0);
  TORCH_CHECK(cos_t.size(1) == D / 2, "cos table must be [S, D/2]");
  auto y = at::empty_like(x);
  rope_launch(x.data_ptr(), y.data_ptr(), cos_t.data_ptr(), sin_t.data_ptr(),
              rows, (int)D, (int)heads, (int)S, (float)sign, cur_stream());
  return y;
}

// ---- SwiGLU ---------------------------------------------------------------
at::Tensor swiglu_fwd(at::Tensor g, at::Tensor u) {
  check_bf16(g, "g");
  check_bf16(u, "u");
  auto out = at::empty_like(g);
  swiglu_fwd_launch(g.data_ptr(), u.data_ptr(), out.data_ptr(), g.numel(),
                    cur_stream());
  return out;
}

std::vector<at::Tensor> swiglu_bwd(at::Tensor dout, at::Tensor g,
                                   at::Tensor u) {
  check_bf16(dout, "dout");
  auto dg = at::empty_like(g);
  auto du = at::empty_like(u);
  swiglu_bwd_launch(dout.data_ptr(), g.data_ptr(), u.data_ptr(), dg.data_ptr(),
                    du.data_ptr(), g.numel(), cur_stream());
  return {dg, du};
}

// ---- AdamW ----------------------------------------------------------------
void adamw_step(at::Tensor p32, at::Tensor p16, at::Tensor g, at::Tensor m,
                at::Tensor v, double lr, double beta1, double beta2,
                double eps, double wd, long step) {
  check_f32(p32, "p32");
  check_bf16(p16, "p16");
  check_bf16(g, "g");
  const long n = p32.numel();
  TORCH_CHECK(n % 4 == 0, "adamw: n must be a multiple of 4");
  const float bc1 = 1.0f - powf((float)beta1, (float)step);
  const float bc2 = 1.0f - powf((float)beta2, (float)step);
  adamw_launch(p32.data_ptr(), p16.data_ptr(), g.data_ptr(), m.data_ptr(),
               v.data_ptr(), n, (float)lr, (float)beta1, (float)beta2,
               (float)eps, (float)wd, bc1, bc2, cur_stream());
}

// ---- Cross entropy --------------------------------------------------------
std::vector<at::Tensor> ce_fwd(at::Tensor logits, at::Tensor targets) {
  check_bf16(logits, "logits");
  TORCH_CHECK(targets.scalar_type() == at::kLong, "targets must be int64");
  const long V = logits.size(-1);
  const long T = logits.numel() / V;
  auto loss = at::empty({T}, logits.options().dtype(at::kFloat));
  auto lse = at::empty({T}, logits.options().dtype(at::kFloat));
  ce_fwd_launch(logits.data_ptr(), targets.data_ptr(), loss.data_ptr(),
                lse.data_ptr(), T, (int)V, cur_stream());
  return {loss, lse};
}

at::Tensor ce_bwd(at::Tensor logits, at::Tensor targets, at::Tensor lse,
                  at::Tensor gscale) {
  check_bf16(logits, "logits");
  check_f32(lse, "lse");
  check_f32(gscale, "gscale");
  const long V = logits.size(-1);
  const long T = logits.numel() / V;
  auto dlogits = at::empty_like(logits);
  ce_bwd_launch(logits.data_ptr(), targets.data_ptr(), lse.data_ptr(),
                gscale.data_ptr(), dlogits.data_ptr(), T, (int)V,
                cur_stream());
  return dlogits;
}

// ---- Attention ------------------------------------------------------------
std::vector<at::Tensor> attn_fwd(at::Tensor q, at::Tensor k, at::Tensor v,
                                 double scale, bool causal) {
  check_bf16(q, "q");
  check_bf16(k, "k");
  check_bf16(v, "v");
  const int B = q.size(0), S = q.size(1), Hq = q.size(2), D = q.size(3);
  const int Hkv = k.size(2);
  TORCH_CHECK(D == 128, "attention: head_dim must be 128");
  TORCH_CHECK(Hq % Hkv == 0, "attention: Hq must be a multiple of Hkv");
  auto o = at::empty_like(q);
  auto lse = at::empty({B, Hq, S}, q.options().dtype(at::kFloat));
  attn_fwd_launch(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                  lse.data_ptr(), B, S, Hq, Hkv, (float)scale, causal ? 1 : 0,
                  (long)Hq * 128, (long)Hkv * 128, cur_stream());
  return {o, lse};
}

// dQ path of the attention backward.  "stream": the dkv kernel exports dS
// into a scratch buffer and dQ is one streamed GEMM over it; "recompute":
// the dQ kernel rebuilds S, dP and dS itself.  Initial value from
// TORCHX_AMD_DQ_MODE (default stream); set_attn_bwd_dq_mode switches it at
// run time so one process can run both.
int g_dq_stream = -1;

bool dq_stream_mode() {
  if (g_dq_stream < 0) {
    const char* e = getenv("TORCHX_AMD_DQ_MODE");
    g_dq_stream = (e && std::string(e) == "recompute") ? 0 : 1;
  }
  return g_dq_stream == 1;
}

void set_attn_bwd_dq_mode(const std::string& mode) {
  TORCH_CHECK(mode == "stream" || mode == "recompute",
              "attn bwd dq mode must be 'stream' or 'recompute', got '",
              mode, "'");
  g_dq_stream = (mode == "stream") ? 1 : 0;
}

std::string get_attn_bwd_dq_mode() {
  return dq_stream_mode() ? "stream" : "recompute";
}

// dK/dV kernel of the attention backward.  "merged": one wave accumulates
// both dK and dV for its kv rows (S, P and dP computed once); "split": the
// 8-wave kernel with separate dV and dK waves.  Both give the same bits.
// Initial value from TORCHX_AMD_DKV_IMPL (read once by the launcher).
void set_attn_bwd_dkv_impl(const std::string& impl) {
  TORCH_CHECK(impl == "merged" || impl == "split",
              "attn bwd dkv impl must be 'merged' or 'split', got '", impl,
              "'");
  attn_bwd_dkv_impl_set(impl == "merged" ? 1 : 0);
}

std::string get_attn_bwd_dkv_impl() {
  return attn_bwd_dkv_impl_get() == 1 ? "merged" : "split";
}

// Block map of the dense forward kernel.  "legacy": map_block_fwd (whole
// (b, kv head) groups per XCD, q tiles ascending); "balanced": the G heads
// of a (b, kv head, q tile) unit adjacent on one XCD, units heaviest first;
// "adjacent": the same unit layout with q tiles ascending (A/B only).  All
// give the same bits.  Initial value from TORCHX_AMD_FWD_MAP (read once by
// the launcher).
void set_attn_fwd_map(const std::string& name) {
  TORCH_CHECK(name == "legacy" || name == "balanced" || name == "adjacent",
              "attn fwd map must be 'balanced', 'legacy' or 'adjacent', "
              "got '", name, "'");
  attn_fwd_map_set(name == "legacy" ? 0 : name == "balanced" ? 1 : 2);
}

std::string get_attn_fwd_map() {
  const int m = attn_fwd_map_get();
  return m == 0 ? "legacy" : m == 1 ? "balanced" : "adjacent";
}

// The scratch is transient HBM on top of the saved activations and grows
// with S^2 (2.2 GB at B=4, Hq=32, S=4096 causal; 4.4 GB at B=2, S=8192).
// Above 8 GiB — under 3% of the 288 GB of an MI355X — the call takes the
// recompute kernel, whose memory does not grow with S^2.
constexpr long kDsScratchCapBytes = 8L << 30;

// dS scratch for one backward call, or an undefined tensor (null pointer)
// when the recompute path is to run.
at::Tensor alloc_ds_scratch(const at::Tensor& like, int B, int S, int Hq,
                            bool causal) {
  if (!dq_stream_mode()) return at::Tensor();
  const long bytes = attn_bwd_ds_bytes(B, S, Hq, causal ? 1 : 0);
  if (bytes > kDsScratchCapBytes) return at::Tensor();
  return at::empty({bytes}, like.options().dtype(at::kByte));
}

std::vector<at::Tensor> attn_bwd(at::Tensor q, at::Tensor k, at::Tensor v,
                                 at::Tensor o, at::Tensor dout, at::Tensor lse,
                                 double scale, bool causal) {
  check_bf16(dout, "dout");
  const int B = q.size(0), S = q.size(1), Hq = q.size(2);
  const int Hkv = k.size(2);
  auto dq = at::empty_like(q);
  auto dk = at::empty_like(k);
  auto dv = at::empty_like(v);
  auto delta = at::empty({B, Hq, S}, q.options().dtype(at::kFloat));
  auto ds = alloc_ds_scratch(q, B, S, Hq, causal);
  attn_bwd_launch(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                  dout.data_ptr(), lse.data_ptr(), delta.data_ptr(),
                  dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                  ds.defined() ? ds.data_ptr() : nullptr, B, S, Hq, Hkv,
                  (float)scale, causal ? 1 : 0, (long)Hq * 128,
                  (long)Hkv * 128, (long)Hq * 128, (long)Hkv * 128,
                  cur_stream());
  return {dq, dk, dv};
}

// ---- fused qkv attention (strided views over the packed qkv buffer) ------
// qkv: [B, S, (Hq+2*Hkv)*128] bf16 from the fused qkv GEMM.  q starts at 0,
// k at Hq*128, v at (Hq+Hkv)*128; row stride = (Hq+2*Hkv)*128.  Saves the
// split/contiguous copies forward and the torch.cat backward.
std::vector<at::Tensor> attn_fwd_qkv(at::Tensor qkv, long Hq, long Hkv,
                                     double scale, bool causal) {
  check_bf16(qkv, "qkv");
  const int B = qkv.size(0), S = qkv.size(1);
  const long rs = (Hq + 2 * Hkv) * 128;
  TORCH_CHECK(qkv.size(2) == rs, "qkv last dim mismatch");
  auto o = at::empty({B, S, Hq, 128}, qkv.options());
  auto lse = at::empty({B, Hq, S}, qkv.options().dtype(at::kFloat));
  const unsigned short* base = (const unsigned short*)qkv.data_ptr();
  attn_fwd_launch(base, base + Hq * 128, base + (Hq + Hkv) * 128,
                  o.data_ptr(), lse.data_ptr(), B, S, (int)Hq, (int)Hkv,
                  (float)scale, causal ? 1 : 0, rs, rs, cur_stream());
  return {o, lse};
}

at::Tensor attn_bwd_qkv(at::Tensor qkv, at::Tensor o, at::Tensor dout,
                        at::Tensor lse, long Hq, long Hkv, double scale,
                        bool causal) {
  check_bf16(dout, "dout");
  const int B = qkv.size(0), S = qkv.size(1);
  const long rs = (Hq + 2 * Hkv) * 128;
  auto dqkv = at::empty_like(qkv);
  auto delta = at::empty({B, Hq, S}, qkv.options().dtype(at::kFloat));
  auto ds = alloc_ds_scratch(qkv, B, S, (int)Hq, causal);
  const unsigned short* base = (const unsigned short*)qkv.data_ptr();
  unsigned short* dbase = (unsigned short*)dqkv.data_ptr();
  attn_bwd_launch(base, base + Hq * 128, base + (Hq + Hkv) * 128,
                  o.data_ptr(), dout.data_ptr(), lse.data_ptr(),
                  delta.data_ptr(), dbase, dbase + Hq * 128,
                  dbase + (Hq + Hkv) * 128,
                  ds.defined() ? ds.data_ptr() : nullptr, B, S, (int)Hq,
                  (int)Hkv, (float)scale, causal ? 1 : 0, rs, rs, rs, rs,
                  cur_stream());
  return dqkv;
}

// RoPE over the packed qkv buffer's q+k heads (y may alias x for in-place
// gradient rotation; the v region is copied when y != x).
at::Tensor rope_qkv(at::Tensor x, at::Tensor cos_t, at::Tensor sin_t,
                    long Hq, long Hkv, double sign, bool inplace) {
  check_bf16(x, "x");
  check_f32(cos_t, "cos");
  check_f32(sin_t, "sin");
  const int B = x.size(0), S = x.size(1);
  const long rs = (Hq + 2 * Hkv) * 128;
  TORCH_CHECK(x.size(2) == rs, "qkv last dim mismatch");
  at::Tensor y = inplace ? x : at::empty_like(x);
  rope_qkv_launch(x.data_ptr(), y.data_ptr(), cos_t.data_ptr(),
                  sin_t.data_ptr(), (long)B * S, (int)(Hq + Hkv), rs, S,
                  (float)sign, cur_stream());
  if (!inplace) {
    const long v0 = (Hq + Hkv) * 128;
    y.narrow(2, v0, Hkv * 128).copy_(x.narrow(2, v0, Hkv * 128));
  }
  return y;
}

// ---- packed swiglu --------------------------------------------------------
at::Tensor swiglu_gu_fwd(at::Tensor gu) {
  check_bf16(gu, "gu");
  const long twoI = gu.size(-1);
  TORCH_CHECK(twoI % 16 == 0, "gu last dim must be 2I, I % 8 == 0");
  const long I = twoI / 2;
  const long rows = gu.numel() / twoI;
  auto sizes = gu.sizes().vec();
  sizes.back() = I;
  auto out = at::empty(sizes, gu.options());
  swiglu_gu_fwd_launch(gu.data_ptr(), out.data_ptr(), rows, I, cur_stream());
  return out;
}

at::Tensor swiglu_gu_bwd(at::Tensor dout, at::Tensor gu) {
  check_bf16(dout, "dout");
  const long twoI = gu.size(-1);
  const long I = twoI / 2;
  const long rows = gu.numel() / twoI;
  auto dgu = at::empty_like(gu);
  swiglu_gu_bwd_launch(dout.data_ptr(), gu.data_ptr(), dgu.data_ptr(), rows,
                       I, cur_stream());
  return dgu;
}

// dgu as swiglu_gu_bwd plus dguT [2I, rows] = dgu^T from the same pass.
std::vector<at::Tensor> swiglu_gu_bwd_t(at::Tensor dout, at::Tensor gu) {
  check_bf16(dout, "dout");
  check_bf16(gu, "gu");
  const long twoI = gu.size(-1);
  const long I = twoI / 2;
  const long rows = gu.numel() / twoI;
  TORCH_CHECK(twoI % 2 == 0 && I % 64 == 0 && rows % 64 == 0 && rows > 0 &&
                  (rows / 64) * (I / 64) < (1L << 31),
              "swiglu_gu_bwd_t: rows and I must be multiples of 64");
  TORCH_CHECK(dout.numel() == rows * I && dout.size(-1) == I,
              "swiglu_gu_bwd_t: dout must be [rows, I]");
  auto dgu = at::empty_like(gu);
  auto dguT = at::empty({twoI, rows}, gu.options());
  swiglu_gu_bwd_t_launch(dout.data_ptr(), gu.data_ptr(), dgu.data_ptr(),
                         dguT.data_ptr(), rows, I, cur_stream());
  return {dgu, dguT};
}

// ---- fp8 fused cast+transpose ---------------------------------------------
// x bf16 [R, C] -> (fp8 [R, C], fp8 [C, R], amax_next scalar).
// scale divides the values (delayed scaling: pass the PREVIOUS amax-derived
// scale; amax_next feeds the next call).
std::vector<at::Tensor> fp8_cast_transpose(at::Tensor x, at::Tensor scale,
                                           bool e5m2) {
  check_bf16(x, "x");
  check_f32(scale, "scale");
  const long C = x.size(-1);
  const long R = x.numel() / C;
  TORCH_CHECK(R % 8 == 0 && C % 8 == 0, "fp8 cast: dims must be 8-aligned");
  auto dt = e5m2 ? at::kFloat8_e5m2 : at::kFloat8_e4m3fn;
  auto out = at::empty({R, C}, x.options().dtype(dt));
  auto out_t = at::empty({C, R}, x.options().dtype(dt));
  auto amax = at::zeros({1}, x.options().dtype(at::kFloat));
  fp8_cast_transpose_launch(x.data_ptr(), out.data_ptr(), out_t.data_ptr(),
                            amax.data_ptr(), scale.data_ptr(), R, C,
                            e5m2 ? 1 : 0, cur_stream());
  return {out, out_t, amax};
}

// ---- bf16 transpose -------------------------------------------------------
at::Tensor transpose_bf16(at::Tensor x) {
  check_bf16(x, "x");
  TORCH_CHECK(x.dim() == 2, "transpose_bf16: 2D only");
  const long R = x.size(0), C = x.size(1);
  TORCH_CHECK(R % 64 == 0 && C % 64 == 0,
              "transpose_bf16: dims must be multiples of 64");
  auto out = at::empty({C, R}, x.options());
  transpose_bf16_launch(x.data_ptr(), out.data_ptr(), R, C, cur_stream());
  return out;
}

// ---- decode attention -----------------------------------------------------
// Split count of the flash-decode variants for q [B, Hq, 128] (enough
// blocks to fill the chip, at most 16 slices) and the f32 scratch of the
// partials; split == 1 is the single-pass kernel and needs no scratch.
struct DecodeSplit {
  int split;
  at::Tensor ml, oacc;  // [B*Hq, split, 2], [B*Hq, split, 128]
  void* mlp = nullptr;
  void* oaccp = nullptr;
};

static DecodeSplit decode_split(const at::Tensor& q) {
  const long BHq = q.size(0) * q.size(1);
  DecodeSplit sp{(int)std::max(1L, std::min(16L, 512 / BHq))};
  if (sp.split > 1) {
    sp.ml = at::empty({BHq * sp.split * 2}, q.options().dtype(at::kFloat));
    sp.oacc = at::empty({BHq * sp.split * 128}, q.options().dtype(at::kFloat));
    sp.mlp = sp.ml.data_ptr();
    sp.oaccp = sp.oacc.data_ptr();
  }
  return sp;
}

// q [B, Hq, 128] bf16; k/v caches [B, T, Hkv, 128] bf16; first L rows
// valid. Returns o [B, Hq, 128].
at::Tensor decode_attn(at::Tensor q, at::Tensor kc, at::Tensor vc, long L,
                       double scale) {
  check_bf16(q, "q");
  check_bf16(kc, "kc");
  check_bf16(vc, "vc");
  const int B = q.size(0), Hq = q.size(1);
  const int T = kc.size(1), Hkv = kc.size(2);
  TORCH_CHECK(q.size(2) == 128 && kc.size(3) == 128, "head_dim must be 128");
  TORCH_CHECK(L >= 1 && L <= T, "invalid cache length");
  TORCH_CHECK(Hq % Hkv == 0, "GQA group mismatch");
  auto o = at::empty_like(q);
  const DecodeSplit sp = decode_split(q);
  if (sp.split > 1) {
    decode_attn_split_launch(q.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                             sp.mlp, sp.oaccp, o.data_ptr(), nullptr, B, Hq,
                             Hkv, T, (int)L, sp.split, 0,
                             (float)scale, cur_stream());
  } else {
    decode_attn_launch(q.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                       o.data_ptr(), nullptr, B, Hq, Hkv, T, (int)L, 0,
                       (float)scale, cur_stream());
  }
  return o;
}

// graph-capturable variant: cache length = pos + 1 read on DEVICE from an
// int32 scalar tensor, so a captured decode step stays valid as the cache
// grows between replays.
at::Tensor decode_attn_dev(at::Tensor q, at::Tensor kc, at::Tensor vc,
                           at::Tensor pos, double scale) {
  check_bf16(q, "q");
  const int B = q.size(0), Hq = q.size(1);
  TORCH_CHECK(pos.scalar_type() == at::kInt &&
                  (pos.numel() == 1 || pos.numel() == B),
              "pos must be an int32 scalar or [B] tensor on device");
  TORCH_CHECK(pos.is_contiguous(), "pos must be contiguous");
  const int per_row = pos.numel() == B && B > 1 ? 1 : 0;
  const int T = kc.size(1), Hkv = kc.size(2);
  auto o = at::empty_like(q);
  const DecodeSplit sp = decode_split(q);
  if (sp.split > 1) {
    decode_attn_split_launch(q.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                             sp.mlp, sp.oaccp, o.data_ptr(), pos.data_ptr(),
                             B, Hq, Hkv, T, 0, sp.split, per_row,
                             (float)scale, cur_stream());
  } else {
    decode_attn_launch(q.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                       o.data_ptr(), pos.data_ptr(), B, Hq, Hkv, T, 0,
                       per_row, (float)scale, cur_stream());
  }
  return o;
}

// ---- skinny-M GEMV (decode linears) ---------------------------------------
// x [M, K] bf16 (M <= 8), w [N, K] bf16 (nn.Linear layout) -> out [M, N].
at::Tensor gemv_bf16(at::Tensor x, at::Tensor w) {
  check_bf16(x, "x");
  check_bf16(w, "w");
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2, "gemv: 2D only");
  const long M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(M >= 1 && M <= 8, "gemv: M must be 1..8");
  TORCH_CHECK(w.size(1) == K, "gemv: K mismatch");
  TORCH_CHECK(K % 512 == 0, "gemv: K must be a multiple of 512");
  auto out = at::empty({M, N}, x.options());
  gemv_bf16_launch(x.data_ptr(), w.data_ptr(), out.data_ptr(), (int)M,
                   (int)N, (int)K, cur_stream());
  return out;
}

// ---- fused skinny-M GEMV + SwiGLU (decode MLP) ----------------------------
// x [M, K], w [2I, K] packed (gate | up) -> silu(x@gate.T) * (x@up.T),
// [M, I]: the wgu projection and the swiglu activation in one dispatch.
at::Tensor gemv_swiglu_bf16(at::Tensor x, at::Tensor w) {
  check_bf16(x, "x");
  check_bf16(w, "w");
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2, "gemv_swiglu: 2D only");
  const long M = x.size(0), K = x.size(1), I = w.size(0) / 2;
  TORCH_CHECK(M >= 1 && M <= 8, "gemv_swiglu: M must be 1..8");
  TORCH_CHECK(w.size(0) == 2 * I && w.size(1) == K, "gemv_swiglu: shape");
  TORCH_CHECK(K % 512 == 0, "gemv_swiglu: K must be a multiple of 512");
  auto out = at::empty({M, I}, x.options());
  gemv_swiglu_launch(x.data_ptr(), w.data_ptr(), out.data_ptr(), (int)M,
                     (int)I, (int)K, cur_stream());
  return out;
}

// ---- fused decode rope + cache append -------------------------------------
// qkv [B, (Hq+2*Hkv)*128] (one position); ropes q/k with cos/sin [S, 64]
// f32 tables at row `pos` (host int, or device int32 scalar when `pos_dev`
// is given), appends k/v to the caches at `pos`, returns q [B, Hq, 128].
at::Tensor decode_rope_cache(at::Tensor qkv, at::Tensor kc, at::Tensor vc,
                             at::Tensor cos_t, at::Tensor sin_t, long pos,
                             c10::optional<at::Tensor> pos_dev) {
  check_bf16(qkv, "qkv");
  check_bf16(kc, "kc");
  check_bf16(vc, "vc");
  check_f32(cos_t, "cos");
  check_f32(sin_t, "sin");
  const int B = qkv.size(0), T = kc.size(1), Hkv = kc.size(2);
  TORCH_CHECK(kc.size(3) == 128 && cos_t.size(1) == 64,
              "head_dim must be 128");
  const long nh = qkv.size(1) / 128;
  const int Hq = (int)nh - 2 * Hkv;
  TORCH_CHECK(Hq >= 1 && qkv.size(1) == nh * 128, "qkv width mismatch");
  const void* pd = nullptr;
  int per_row = 0;
  if (pos_dev.has_value()) {
    TORCH_CHECK(pos_dev->scalar_type() == at::kInt &&
                    (pos_dev->numel() == 1 || pos_dev->numel() == B),
                "pos_dev must be an int32 scalar or [B] tensor");
    TORCH_CHECK(pos_dev->is_contiguous(), "pos_dev must be contiguous");
    pd = pos_dev->data_ptr();
    per_row = pos_dev->numel() == B && B > 1 ? 1 : 0;
  } else {
    TORCH_CHECK(pos >= 0 && pos < T, "pos out of cache range");
    TORCH_CHECK(pos < cos_t.size(0), "pos beyond rope table");
  }
  auto q = at::empty({B, (long)Hq, 128}, qkv.options());
  decode_rope_cache_launch(qkv.data_ptr(), q.data_ptr(), kc.data_ptr(),
                           vc.data_ptr(), cos_t.data_ptr(), sin_t.data_ptr(),
                           pd, B, Hq, Hkv, T, (int)pos, per_row,
                           cur_stream());
  return q;
}

// ---- paged KV cache (block-table) decode -----------------------------------
// kpool/vpool [num_pages, P, Hkv, 128] bf16; block_table int32 [B, M]
// (logical page j of sequence b -> physical page); pos int32 [B]. The
// kernels clamp every table entry and position, so the checks here are
// about shapes and dtypes only. Returns log2(P).
int check_paged(const at::Tensor& kpool, const at::Tensor& vpool,
                const at::Tensor& bt, const at::Tensor& pos, long B) {
  check_bf16(kpool, "kpool");
  check_bf16(vpool, "vpool");
  TORCH_CHECK(kpool.dim() == 4 && kpool.sizes() == vpool.sizes(),
              "kpool/vpool must be 4-D [num_pages, P, Hkv, 128] with "
              "identical shapes");
  TORCH_CHECK(kpool.size(3) == 128, "head_dim must be 128");
  const long P = kpool.size(1);
  TORCH_CHECK(P >= 16 && P <= 256 && (P & (P - 1)) == 0,
              "page size must be a power of two in [16, 256]");
  TORCH_CHECK(kpool.size(0) >= 1 && kpool.size(0) * P < (1L << 31),
              "invalid num_pages");
  TORCH_CHECK(bt.is_cuda() && bt.scalar_type() == at::kInt &&
                  bt.dim() == 2 && bt.is_contiguous(),
              "block_table must be a contiguous int32 [B, M] device tensor");
  TORCH_CHECK(bt.size(0) == B, "block_table rows must equal the batch");
  TORCH_CHECK(bt.size(1) >= 1 && bt.size(1) * P < (1L << 31),
              "invalid block_table width");
  TORCH_CHECK(pos.is_cuda() && pos.scalar_type() == at::kInt &&
                  pos.is_contiguous() && pos.numel() == B,
              "pos must be a contiguous int32 [B] device tensor");
  int logP = 0;
  while ((1L << logP) < P) ++logP;
  return logP;
}

at::Tensor paged_decode_attn(at::Tensor q, at::Tensor kpool,
                             at::Tensor vpool, at::Tensor bt, at::Tensor pos,
                             double scale) {
  check_bf16(q, "q");
  TORCH_CHECK(q.dim() == 3 && q.size(2) == 128, "q must be [B, Hq, 128]");
  const int B = q.size(0), Hq = q.size(1);
  const int logP = check_paged(kpool, vpool, bt, pos, B);
  const int num_pages = kpool.size(0), Hkv = kpool.size(2);
  const int M = bt.size(1);
  TORCH_CHECK(Hq % Hkv == 0, "GQA group mismatch");
  auto o = at::empty_like(q);
  const DecodeSplit sp = decode_split(q);
  paged_decode_attn_launch(q.data_ptr(), kpool.data_ptr(), vpool.data_ptr(),
                           sp.mlp, sp.oaccp, o.data_ptr(), bt.data_ptr(),
                           pos.data_ptr(), B, Hq, Hkv, num_pages, logP, M,
                           sp.split, (float)scale, cur_stream());
  return o;
}

// qkv [B, (Hq+2*Hkv)*128] (one position): ropes q/k at pos[b], appends
// k/v to the pools at slot bt[b][pos/P]*P + pos%P, returns q [B, Hq, 128].
at::Tensor paged_decode_rope_cache(at::Tensor qkv, at::Tensor kpool,
                                   at::Tensor vpool, at::Tensor bt,
                                   at::Tensor cos_t, at::Tensor sin_t,
                                   at::Tensor pos) {
  check_bf16(qkv, "qkv");
  check_f32(cos_t, "cos");
  check_f32(sin_t, "sin");
  TORCH_CHECK(qkv.dim() == 2, "qkv must be [B, (Hq+2*Hkv)*128]");
  const int B = qkv.size(0);
  const int logP = check_paged(kpool, vpool, bt, pos, B);
  const int num_pages = kpool.size(0), Hkv = kpool.size(2);
  const int M = bt.size(1);
  TORCH_CHECK(cos_t.dim() == 2 && cos_t.size(1) == 64 &&
                  cos_t.size(0) >= 1 && sin_t.sizes() == cos_t.sizes(),
              "cos/sin must be [S, 64] (head_dim 128)");
  const long nh = qkv.size(1) / 128;
  const int Hq = (int)nh - 2 * Hkv;
  TORCH_CHECK(Hq >= 1 && qkv.size(1) == nh * 128, "qkv width mismatch");
  TORCH_CHECK(Hq % Hkv == 0, "GQA group mismatch");
  const int rope_rows = (int)std::min<long>(cos_t.size(0), 1L << 30);
  auto q = at::empty({B, (long)Hq, 128}, qkv.options());
  paged_decode_rope_cache_launch(qkv.data_ptr(), q.data_ptr(),
                                 kpool.data_ptr(), vpool.data_ptr(),
                                 bt.data_ptr(), cos_t.data_ptr(),
                                 sin_t.data_ptr(), pos.data_ptr(), B, Hq,
                                 Hkv, num_pages, logP, M, rope_rows,
                                 cur_stream());
  return q;
}

// q [B, S, Hq, 128]: a chunk of S query rows at logical positions
// ctx[b] .. ctx[b]+S-1, attending the ctx[b]+S rows the pools already hold
// for sequence b (causal). Returns o [B, S, Hq, 128].
at::Tensor paged_prefill_attn(at::Tensor q, at::Tensor kpool,
                              at::Tensor vpool, at::Tensor bt, at::Tensor ctx,
                              double scale) {
  check_bf16(q, "q");
  TORCH_CHECK(q.dim() == 4 && q.size(3) == 128,
              "q must be [B, S, Hq, 128]");
  const int B = q.size(0), Hq = q.size(2);
  TORCH_CHECK(q.size(1) >= 1 && q.size(1) < (1L << 30), "need 1 <= S < 2^30");
  const int S = q.size(1);
  const int logP = check_paged(kpool, vpool, bt, ctx, B);
  TORCH_CHECK(ctx.dim() == 1, "ctx must be int32 [B]");
  const int num_pages = kpool.size(0), Hkv = kpool.size(2);
  const int M = bt.size(1);
  TORCH_CHECK(Hq % Hkv == 0, "GQA group mismatch");
  const long nqt = (S + 127) / 128;
  TORCH_CHECK((long)B * Hq * nqt < (1L << 31), "grid too large");
  auto o = at::empty_like(q);
  paged_prefill_attn_launch(q.data_ptr(), kpool.data_ptr(), vpool.data_ptr(),
                            o.data_ptr(), bt.data_ptr(), ctx.data_ptr(), B, S,
                            Hq, Hkv, num_pages, logP, M, (float)scale,
                            cur_stream());
  return o;
}

// q [T, Hq, 128]: the chunks of B sequences packed back to back. tiles is
// the host-built int32 [ntiles, 4] list (sequence, q tile, first packed
// row, chunk length); the kernel clamps every field, so its content cannot
// address outside q, o or the table. Returns o [T, Hq, 128].
at::Tensor paged_prefill_attn_ragged(at::Tensor q, at::Tensor kpool,
                                     at::Tensor vpool, at::Tensor bt,
                                     at::Tensor ctx, at::Tensor tiles,
                                     double scale) {
  check_bf16(q, "q");
  TORCH_CHECK(q.dim() == 3 && q.size(2) == 128, "q must be [T, Hq, 128]");
  TORCH_CHECK(q.size(0) >= 1 && q.size(0) < (1L << 30), "need 1 <= T < 2^30");
  const int T = q.size(0), Hq = q.size(1);
  const int B = bt.dim() == 2 ? bt.size(0) : 0;
  const int logP = check_paged(kpool, vpool, bt, ctx, B);
  TORCH_CHECK(B >= 1 && ctx.dim() == 1, "ctx must be int32 [B], B >= 1");
  TORCH_CHECK(tiles.is_cuda() && tiles.scalar_type() == at::kInt &&
                  tiles.dim() == 2 && tiles.size(1) == 4 &&
                  tiles.size(0) >= 1 && tiles.is_contiguous(),
              "tiles must be a contiguous int32 [ntiles, 4] device tensor");
  const int num_pages = kpool.size(0), Hkv = kpool.size(2);
  const int M = bt.size(1);
  TORCH_CHECK(Hq % Hkv == 0, "GQA group mismatch");
  const long ntiles = tiles.size(0);
  TORCH_CHECK((ntiles * Hkv + 7) / 8 * 8 * (Hq / Hkv) < (1L << 31),
              "grid too large");
  auto o = at::empty_like(q);
  paged_prefill_attn_ragged_launch(
      q.data_ptr(), kpool.data_ptr(), vpool.data_ptr(), o.data_ptr(),
      bt.data_ptr(), ctx.data_ptr(), tiles.data_ptr(), (int)ntiles, B, T, Hq,
      Hkv, num_pages, logP, M, (float)scale, cur_stream());
  return o;
}

// qkv [T, (Hq+2*Hkv)*128], packed tokens: ropes q/k of token t at pos[t],
// writes k/v to pool row slot[t], returns q [T, Hq, 128].
at::Tensor paged_prefill_rope_cache(at::Tensor qkv, at::Tensor kpool,
                                    at::Tensor vpool, at::Tensor cos_t,
                                    at::Tensor sin_t, at::Tensor pos,
                                    at::Tensor slot) {
  check_bf16(qkv, "qkv");
  check_bf16(kpool, "kpool");
  check_bf16(vpool, "vpool");
  check_f32(cos_t, "cos");
  check_f32(sin_t, "sin");
  TORCH_CHECK(qkv.dim() == 2 && qkv.size(0) >= 1,
              "qkv must be [T, (Hq+2*Hkv)*128]");
  TORCH_CHECK(kpool.dim() == 4 && kpool.sizes() == vpool.sizes() &&
                  kpool.size(3) == 128 && kpool.size(0) >= 1 &&
                  kpool.size(1) >= 1 && kpool.size(2) >= 1,
              "kpool/vpool must be [num_pages, P, Hkv, 128], same shape");
  const long T = qkv.size(0);
  const int Hkv = kpool.size(2);
  const long pool_rows = kpool.size(0) * kpool.size(1);
  TORCH_CHECK(pool_rows < (1L << 31), "pool too large for int32 slots");
  for (const at::Tensor* t : {&pos, &slot}) {
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kInt &&
                    t->is_contiguous() && t->dim() == 1 && t->size(0) == T,
                "pos/slot must be contiguous int32 [T] device tensors");
  }
  TORCH_CHECK(cos_t.dim() == 2 && cos_t.size(1) == 64 &&
                  cos_t.size(0) >= 1 && sin_t.sizes() == cos_t.sizes(),
              "cos/sin must be [S, 64] (head_dim 128)");
  const long nh = qkv.size(1) / 128;
  const int Hq = (int)nh - 2 * Hkv;
  TORCH_CHECK(Hq >= 1 && qkv.size(1) == nh * 128, "qkv width mismatch");
  TORCH_CHECK(Hq % Hkv == 0, "GQA group mismatch");
  const int rope_rows = (int)std::min<long>(cos_t.size(0), 1L << 30);
  auto q = at::empty({T, (long)Hq, 128}, qkv.options());
  paged_prefill_rope_cache_launch(
      qkv.data_ptr(), q.data_ptr(), kpool.data_ptr(), vpool.data_ptr(),
      cos_t.data_ptr(), sin_t.data_ptr(), pos.data_ptr(), slot.data_ptr(), T,
      Hq, Hkv, pool_rows, rope_rows, cur_stream());
  return q;
}

// ---- fused residual add + rmsnorm (inference) ------------------------------
// s = x + res, y = rmsnorm(s) * w; returns (s, y). res omitted -> plain
// rmsnorm (s aliases x).
std::vector<at::Tensor> rmsnorm_res(at::Tensor x,
                                    c10::optional<at::Tensor> res,
                                    at::Tensor w, double eps) {
  check_bf16(x, "x");
  check_bf16(w, "w");
  const long H = x.size(-1);
  TORCH_CHECK(H % 2048 == 0 && H <= 8192, "rmsnorm: H must be k*2048, <=8192");
  const long R = x.numel() / H;
  auto y = at::empty_like(x);
  at::Tensor s = x;
  const void* rp = nullptr;
  void* sp = nullptr;
  if (res.has_value()) {
    check_bf16(*res, "res");
    TORCH_CHECK(res->sizes() == x.sizes(), "res shape mismatch");
    s = at::empty_like(x);
    rp = res->data_ptr();
    sp = s.data_ptr();
  }
  rmsnorm_res_launch(x.data_ptr(), rp, w.data_ptr(), sp, y.data_ptr(),
                     nullptr, R, (int)H, (float)eps, cur_stream());
  return {s, y};
}

// ---- fused residual add + rmsnorm (training) -------------------------------
// s = bf16(x + delta), y = rmsnorm(s) * w; returns (s, y, invrms) with
// invrms [rows] f32 saved for rmsnorm_bwd.
std::vector<at::Tensor> add_rmsnorm_fwd(at::Tensor x, at::Tensor delta,
                                        at::Tensor w, double eps) {
  check_bf16(x, "x");
  check_bf16(delta, "delta");
  check_bf16(w, "w");
  const long H = x.size(-1);
  TORCH_CHECK(H % 2048 == 0 && H <= 8192, "rmsnorm: H must be k*2048, <=8192");
  TORCH_CHECK(delta.sizes() == x.sizes(), "delta shape mismatch");
  TORCH_CHECK(w.numel() == H, "w size mismatch");
  const long R = x.numel() / H;
  auto s = at::empty_like(x);
  auto y = at::empty_like(x);
  auto invrms = at::empty({R}, x.options().dtype(at::kFloat));
  rmsnorm_res_launch(x.data_ptr(), delta.data_ptr(), w.data_ptr(),
                     s.data_ptr(), y.data_ptr(), invrms.data_ptr(), R, (int)H,
                     (float)eps, cur_stream());
  return {s, y, invrms};
}

// ---- probe ----------------------------------------------------------------
std::vector<at::Tensor> mfma_probe_tr(at::Tensor a, at::Tensor b) {
  check_bf16(a, "a");
  check_bf16(b, "b");
  TORCH_CHECK(a.size(0) == 32 && a.size(1) == 16, "a must be [32,16]");
  TORCH_CHECK(b.size(0) == 16 && b.size(1) == 32, "b must be [16,32]");
  auto c = at::empty({32, 32}, a.options().dtype(at::kFloat));
  auto raw = at::empty({64, 8}, a.options());
  mfma_probe_tr_launch(a.data_ptr(), b.data_ptr(), c.data_ptr(),
                       raw.data_ptr(), cur_stream());
  return {c, raw};
}

at::Tensor mfma_probe(at::Tensor a, at::Tensor b) {
  check_bf16(a, "a");
  check_bf16(b, "b");
  TORCH_CHECK(a.size(0) == 32 && a.size(1) == 16, "a must be [32,16]");
  TORCH_CHECK(b.size(0) == 16 && b.size(1) == 32, "b must be [16,32]");
  auto c = at::empty({32, 32}, a.options().dtype(at::kFloat));
  mfma_probe_launch(a.data_ptr(), b.data_ptr(), c.data_ptr(), cur_stream());
  return c;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rmsnorm_fwd", &rmsnorm_fwd);
  m.def("rmsnorm_bwd", &rmsnorm_bwd, py::arg("dy"), py::arg("x"),
        py::arg("w"), py::arg("invrms"), py::arg("dres") = c10::nullopt);
  m.def("add_rmsnorm_fwd", &add_rmsnorm_fwd);
  m.def("rope", &rope);
  m.def("swiglu_fwd", &swiglu_fwd);
  m.def("swiglu_bwd", &swiglu_bwd);
  m.def("adamw_step", &adamw_step);
  m.def("ce_fwd", &ce_fwd);
  m.def("ce_bwd", &ce_bwd);
  m.def("attn_fwd", &attn_fwd);
  m.def("attn_bwd", &attn_bwd);
  m.def("set_attn_bwd_dq_mode", &set_attn_bwd_dq_mode);
  m.def("get_attn_bwd_dq_mode", &get_attn_bwd_dq_mode);
  m.def("set_attn_bwd_dkv_impl", &set_attn_bwd_dkv_impl);
  m.def("get_attn_bwd_dkv_impl", &get_attn_bwd_dkv_impl);
  m.def("set_attn_fwd_map", &set_attn_fwd_map);
  m.def("get_attn_fwd_map", &get_attn_fwd_map);
  m.def("attn_fwd_qkv", &attn_fwd_qkv);
  m.def("attn_bwd_qkv", &attn_bwd_qkv);
  m.def("rope_qkv", &rope_qkv);
  m.def("swiglu_gu_fwd", &swiglu_gu_fwd);
  m.def("swiglu_gu_bwd", &swiglu_gu_bwd);
  m.def("swiglu_gu_bwd_t", &swiglu_gu_bwd_t);
  m.def("fp8_cast_transpose", &fp8_cast_transpose);
  m.def("mfma_probe", &mfma_probe);
  m.def("mfma_probe_tr", &mfma_probe_tr);
  m.def("transpose_bf16", &transpose_bf16);
  m.def("decode_attn", &decode_attn);
  m.def("decode_attn_dev", &decode_attn_dev);
  m.def("gemv_bf16", &gemv_bf16);
  m.def("gemv_swiglu_bf16", &gemv_swiglu_bf16);
  m.def("decode_rope_cache", &decode_rope_cache,
        py::arg("qkv"), py::arg("kc"), py::arg("vc"), py::arg("cos"),
        py::arg("sin"), py::arg("pos") = 0,
        py::arg("pos_dev") = c10::nullopt);
  m.def("paged_decode_attn", &paged_decode_attn);
  m.def("paged_decode_rope_cache", &paged_decode_rope_cache);
  m.def("paged_prefill_attn", &paged_prefill_attn);
  m.def("paged_prefill_attn_ragged", &paged_prefill_attn_ragged);
  m.def("paged_prefill_rope_cache", &paged_prefill_rope_cache);
  m.def("rmsnorm_res", &rmsnorm_res,
        py::arg("x"), py::arg("res"), py::arg("w"), py::arg("eps"));
}
