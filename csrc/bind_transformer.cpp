// Python bindings for the fused transformer kernels (csrc/kernels/transformer.hip).
#include "bind_common.h"
#include "kernels/transformer_api.h"

namespace dtf {
namespace {
int rows_of(const at::Tensor& t, int H) { return (int)(t.numel() / H); }
void need_p(double p, const char* op) {
  require(p >= 0.0 && p < 1.0, std::string(op) + ": dropout p must be in [0, 1)");
}
// the last dimension as the row width: at least 1, so that rows_of can divide by it
int width_of(const at::Tensor& t, const char* op) {
  require(t.dim() >= 1 && t.size(-1) > 0, std::string(op) + ": the last dimension is empty");
  return (int)t.size(-1);
}
}  // namespace

// y = LN(dropout(x + bias) + res) ; x, res, y, s bf16 [N, H]; bias/gamma/beta fp32 [H]
void bdrln_fwd(at::Tensor x, at::Tensor bias, c10::optional<at::Tensor> res, at::Tensor gamma, at::Tensor beta,
               at::Tensor y, c10::optional<at::Tensor> s, at::Tensor mean, at::Tensor rstd, double eps, double p,
               int64_t seed) {
  const int H = width_of(x, "bdrln_fwd");
  need(x, at::kBFloat16, "x"); need(y, at::kBFloat16, "y"); need(bias, at::kFloat, "bias");
  need(gamma, at::kFloat, "gamma"); need(beta, at::kFloat, "beta"); need(mean, at::kFloat, "mean");
  need(rstd, at::kFloat, "rstd");
  if (res.has_value()) need(*res, at::kBFloat16, "res");
  if (s.has_value()) need(*s, at::kBFloat16, "s");
  const int N = rows_of(x, H);
  if (mean.numel() < N || rstd.numel() < N || y.numel() != x.numel()) throw std::runtime_error("bdrln_fwd shapes");
  require(bias.numel() >= H && gamma.numel() >= H && beta.numel() >= H,
          "bdrln_fwd: bias / gamma / beta need H elements");
  require(!res.has_value() || res->numel() == x.numel(), "bdrln_fwd: res size");
  require(!s.has_value() || s->numel() == x.numel(), "bdrln_fwd: s size");
  need_p(p, "bdrln_fwd");
  hip_check(dtfk_bdrln_fwd(x.data_ptr(), bias.data_ptr<float>(), opt_ptr(res), gamma.data_ptr<float>(),
                           beta.data_ptr<float>(), y.data_ptr(), opt_ptr(s), mean.data_ptr<float>(),
                           rstd.data_ptr<float>(), N, H, (float)eps, (float)p, (unsigned long long)seed, cur_stream()),
            "bdrln_fwd");
}

void ln_fwd_f32in(at::Tensor x, at::Tensor gamma, at::Tensor beta, at::Tensor y, c10::optional<at::Tensor> s,
                  at::Tensor mean, at::Tensor rstd, double eps, double p, int64_t seed) {
  const int H = width_of(x, "ln_fwd_f32in");
  need(x, at::kFloat, "x"); need(y, at::kBFloat16, "y");
  need(gamma, at::kFloat, "gamma"); need(beta, at::kFloat, "beta"); need(mean, at::kFloat, "mean");
  need(rstd, at::kFloat, "rstd");
  if (s.has_value()) need(*s, at::kBFloat16, "s");
  const int N = rows_of(x, H);
  require(y.numel() == x.numel() && (!s.has_value() || s->numel() == x.numel()), "ln_fwd_f32in: y / s size");
  require(gamma.numel() >= H && beta.numel() >= H, "ln_fwd_f32in: gamma / beta need H elements");
  require(mean.numel() >= N && rstd.numel() >= N, "ln_fwd_f32in: mean / rstd need N elements");
  need_p(p, "ln_fwd_f32in");
  hip_check(dtfk_ln_fwd_f32in(x.data_ptr<float>(), gamma.data_ptr<float>(), beta.data_ptr<float>(), y.data_ptr(),
                              opt_ptr(s), mean.data_ptr<float>(), rstd.data_ptr<float>(), N, H, (float)eps, (float)p,
                              (unsigned long long)seed, cur_stream()),
            "ln_fwd_f32in");
}

// BERT embedding block: y = dropout(LN(word[ids] + typ[tt] + pos[t % S])), s = bf16 of the sum
void emb_ln_fwd(at::Tensor word, at::Tensor ids, at::Tensor typ, at::Tensor tt, at::Tensor pos, int64_t S,
                at::Tensor gamma, at::Tensor beta, at::Tensor y, at::Tensor s, at::Tensor mean, at::Tensor rstd,
                double eps, double p, int64_t seed) {
  const int H = (int)word.size(-1);
  need(word, at::kFloat, "word"); need(typ, at::kFloat, "typ"); need(pos, at::kFloat, "pos");
  need(gamma, at::kFloat, "gamma"); need(beta, at::kFloat, "beta");
  need(y, at::kBFloat16, "y"); need(s, at::kBFloat16, "s"); need(mean, at::kFloat, "mean");
  need(rstd, at::kFloat, "rstd");
  need(ids, at::kLong, "ids"); need(tt, at::kLong, "tt");
  const int64_t N = ids.numel();
  if (tt.numel() != N || y.numel() != N * H || s.numel() != N * H || mean.numel() < N || rstd.numel() < N ||
      typ.size(-1) != H || pos.size(-1) != H || pos.size(0) < S || S < 1 || N % S)
    throw std::runtime_error("emb_ln_fwd shapes");
  require(N >= 1 && H >= 1 && gamma.numel() >= H && beta.numel() >= H, "emb_ln_fwd: gamma / beta need H elements");
  need_p(p, "emb_ln_fwd");
  hip_check(dtfk_emb_ln_fwd(word.data_ptr<float>(), ids.data_ptr<int64_t>(), typ.data_ptr<float>(),
                            tt.data_ptr<int64_t>(), pos.data_ptr<float>(), (int)S, gamma.data_ptr<float>(),
                            beta.data_ptr<float>(), y.data_ptr(), s.data_ptr(), mean.data_ptr<float>(),
                            rstd.data_ptr<float>(), (int)N, H, (float)eps, (float)p, (unsigned long long)seed,
                            cur_stream()),
            "emb_ln_fwd");
}
// position / 2-row token-type gradients of the embedding block from ds [B*S, H] bf16:
// pos_grad rows [0, S) (+)= sum over b; typ_grad [2, H] (+)= per-type sums
void emb_bwd_aux(at::Tensor ds, at::Tensor tt, int64_t S, at::Tensor pos_grad, at::Tensor typ_grad, at::Tensor part,
                 bool accumulate) {
  const int H = (int)ds.size(-1);
  need(ds, at::kBFloat16, "ds"); need(tt, at::kLong, "tt"); need(pos_grad, at::kFloat, "pos_grad");
  need(typ_grad, at::kFloat, "typ_grad"); need(part, at::kFloat, "part");
  const int64_t N = tt.numel();
  if (S < 1 || N % S || ds.numel() != N * H || pos_grad.numel() < S * H || typ_grad.numel() < 2 * H ||
      part.numel() < 2 * S * H)
    throw std::runtime_error("emb_bwd_aux shapes");
  hip_check(dtfk_emb_bwd_aux(ds.data_ptr(), tt.data_ptr<int64_t>(), (int)(N / S), (int)S, H, pos_grad.data_ptr<float>(),
                             part.data_ptr<float>(), accumulate ? 1 : 0, cur_stream()),
            "emb_bwd_aux");
  const float* parts[2] = {part.data_ptr<float>(), part.data_ptr<float>() + S * H};
  float* outs[2] = {typ_grad.data_ptr<float>(), typ_grad.data_ptr<float>() + H};
  hip_check(dtfk_colsum_partials_multi(parts, outs, 2, (int)S, H, accumulate ? 1 : 0, cur_stream()),
            "emb_bwd_aux colsum");
}

// returns nothing; dgamma/dbeta/dbias (fp32 [H]) written if given
void ln_bwd(at::Tensor dy, at::Tensor s, at::Tensor mean, at::Tensor rstd, at::Tensor gamma, at::Tensor ds,
            c10::optional<at::Tensor> dxb, at::Tensor part, c10::optional<at::Tensor> dgamma,
            c10::optional<at::Tensor> dbeta, c10::optional<at::Tensor> dbias, double p, int64_t seed,
            bool accumulate) {
  const int H = width_of(dy, "ln_bwd");
  need(dy, at::kBFloat16, "dy"); need(s, at::kBFloat16, "s"); need(ds, at::kBFloat16, "ds");
  need(part, at::kFloat, "part"); need(mean, at::kFloat, "mean"); need(rstd, at::kFloat, "rstd");
  need(gamma, at::kFloat, "gamma");
  if (dxb.has_value()) need(*dxb, at::kBFloat16, "dxb");
  const int N = rows_of(dy, H);
  const int grid = (int)(part.numel() / (3LL * H));
  if (grid < 1) throw std::runtime_error("ln_bwd: partial buffer too small (needs 3*grid*H floats)");
  require(s.numel() == dy.numel() && ds.numel() == dy.numel() && (!dxb.has_value() || dxb->numel() == dy.numel()),
          "ln_bwd: s / ds / dxb size");
  require(mean.numel() >= N && rstd.numel() >= N, "ln_bwd: mean / rstd need N elements");
  require(gamma.numel() >= H, "ln_bwd: gamma needs H elements");
  need_p(p, "ln_bwd");
  for (const auto* t : {&dgamma, &dbeta, &dbias})
    if (t->has_value()) {
      need(**t, at::kFloat, "param grad");
      require((*t)->numel() >= H, "ln_bwd: gradient output too small");
    }
  float* pg = part.data_ptr<float>();
  float* pb = pg + (size_t)grid * H;
  float* px = pb + (size_t)grid * H;
  hip_check(dtfk_ln_bwd(dy.data_ptr(), s.data_ptr(), mean.data_ptr<float>(), rstd.data_ptr<float>(),
                        gamma.data_ptr<float>(), ds.data_ptr(), opt_ptr(dxb), dgamma.has_value() ? pg : nullptr,
                        dbeta.has_value() ? pb : nullptr, dbias.has_value() ? px : nullptr, grid, N, H, (float)p,
                        (unsigned long long)seed, cur_stream()),
            "ln_bwd");
  // dgamma / dbeta / dbias: one finishing launch (accumulate: += into sunk .grad)
  const float* parts[3];
  float* outs[3];
  int nb = 0;
  auto add = [&](const c10::optional<at::Tensor>& t, const float* pp) {
    if (!t.has_value()) return;
    need(*t, at::kFloat, "param grad");
    if (t->numel() < H) throw std::runtime_error("ln_bwd: gradient output too small");
    parts[nb] = pp;
    outs[nb++] = t->data_ptr<float>();
  };
  add(dgamma, pg);
  add(dbeta, pb);
  add(dbias, px);
  if (nb) hip_check(dtfk_colsum_partials_multi(parts, outs, nb, grid, H, accumulate ? 1 : 0, cur_stream()), "colsum");
}

// bias gradient of a bf16 [N, H] matrix: out (+)= column sums (part: P*H floats)
void colsum_bf16(at::Tensor x, at::Tensor part, at::Tensor out, bool accumulate) {
  need(x, at::kBFloat16, "x"); need(part, at::kFloat, "part"); need(out, at::kFloat, "out");
  const int H = width_of(x, "colsum_bf16");
  const int N = rows_of(x, H);
  const int P = (int)(part.numel() / H);
  if (P < 1 || out.numel() < H) throw std::runtime_error("colsum_bf16 shapes");
  hip_check(dtfk_colsum_bf16(x.data_ptr(), part.data_ptr<float>(), out.data_ptr<float>(), N, H, P, accumulate ? 1 : 0,
                             cur_stream()),
            "colsum_bf16");
}

// out (+)= sum over the leading dim of slabs [S, n] (fp32; 16-byte vector path when aligned)
void slab_sum(at::Tensor slabs, at::Tensor out, bool accumulate) {
  need(slabs, at::kFloat, "slabs"); need(out, at::kFloat, "out");
  const int64_t n = out.numel();
  if (n == 0 || slabs.numel() % n) throw std::runtime_error("slab_sum shapes");
  if (!slabs.is_contiguous() || !out.is_contiguous()) throw std::runtime_error("slab_sum: contiguous tensors only");
  const int S = (int)(slabs.numel() / n);
  hip_check(dtfk_slab_sum(slabs.data_ptr<float>(), out.data_ptr<float>(), S, n, accumulate ? 1 : 0, cur_stream()),
            "slab_sum");
}

void bias_gelu_fwd(at::Tensor x, at::Tensor bias, at::Tensor y) {
  need(x, at::kBFloat16, "x"); need(y, at::kBFloat16, "y"); need(bias, at::kFloat, "bias");
  const int H = width_of(x, "bias_gelu_fwd");
  if (H % 4) throw std::runtime_error("bias_gelu: H % 4 != 0");
  require(bias.numel() >= H && y.numel() == x.numel(), "bias_gelu_fwd: bias needs H elements, y the size of x");
  hip_check(dtfk_bias_gelu_fwd(x.data_ptr(), bias.data_ptr<float>(), y.data_ptr(), x.numel(), H, cur_stream()),
            "bias_gelu_fwd");
}

void bias_gelu_bwd(at::Tensor dy, at::Tensor x, at::Tensor bias, at::Tensor dx, at::Tensor part, at::Tensor dbias,
                   bool accumulate) {
  need(dy, at::kBFloat16, "dy"); need(x, at::kBFloat16, "x"); need(dx, at::kBFloat16, "dx");
  need(part, at::kFloat, "part"); need(dbias, at::kFloat, "dbias");
  const int H = width_of(x, "bias_gelu_bwd");
  const int N = rows_of(x, H);
  const int slices = (int)(part.numel() / H);
  if (slices < 1 || H % 4) throw std::runtime_error("bias_gelu_bwd shapes");
  require(bias.numel() >= H && dbias.numel() >= H && dy.numel() == x.numel() && dx.numel() == x.numel(),
          "bias_gelu_bwd: bias / dbias need H elements, dy / dx the size of x");
  hip_check(dtfk_bias_gelu_bwd(dy.data_ptr(), x.data_ptr(), bias.data_ptr<float>(), dx.data_ptr(),
                               part.data_ptr<float>(), N, H, slices, cur_stream()),
            "bias_gelu_bwd");
  const float* pp[1] = {part.data_ptr<float>()};
  float* po[1] = {dbias.data_ptr<float>()};
  hip_check(dtfk_colsum_partials_multi(pp, po, 1, slices, H, accumulate ? 1 : 0, cur_stream()), "colsum");
}

void softmax_fwd(at::Tensor S, c10::optional<at::Tensor> mask, at::Tensor P, c10::optional<at::Tensor> Pd,
                 int64_t rows_per_batch, double scale, double p, int64_t seed) {
  need(S, at::kBFloat16, "S"); need(P, at::kBFloat16, "P");
  if (Pd.has_value()) need(*Pd, at::kBFloat16, "Pd");
  if (mask.has_value()) need(*mask, at::kFloat, "mask");
  const int Sk = width_of(S, "softmax_fwd");
  const int rows = (int)(S.numel() / Sk);
  require(rows_per_batch >= 1, "softmax_fwd: rows_per_batch must be at least 1");
  require(P.numel() == S.numel() && (!Pd.has_value() || Pd->numel() == S.numel()), "softmax_fwd: P / Pd size");
  require(!mask.has_value() || mask->numel() >= ((int64_t)rows + rows_per_batch - 1) / rows_per_batch * Sk,
          "softmax_fwd: mask needs ceil(rows / rows_per_batch) * Sk elements");
  need_p(p, "softmax_fwd");
  hip_check(dtfk_softmax_fwd(S.data_ptr(), opt_ptr<float>(mask), P.data_ptr(), opt_ptr(Pd), rows, Sk,
                             (int)rows_per_batch, (float)scale, (float)p, (unsigned long long)seed, cur_stream()),
            "softmax_fwd");
}

void softmax_bwd(at::Tensor dPd, at::Tensor P, at::Tensor dS, double scale, double p, int64_t seed) {
  need(dPd, at::kBFloat16, "dPd"); need(P, at::kBFloat16, "P"); need(dS, at::kBFloat16, "dS");
  const int Sk = width_of(P, "softmax_bwd");
  const int rows = (int)(P.numel() / Sk);
  require(dPd.numel() == P.numel() && dS.numel() == P.numel(), "softmax_bwd: dPd / dS size");
  need_p(p, "softmax_bwd");
  hip_check(dtfk_softmax_bwd(dPd.data_ptr(), P.data_ptr(), dS.data_ptr(), rows, Sk, (float)scale, (float)p,
                             (unsigned long long)seed, cur_stream()),
            "softmax_bwd");
}

void dropout_bf16(at::Tensor x, at::Tensor y, double p, int64_t seed) {
  need(x, at::kBFloat16, "x"); need(y, at::kBFloat16, "y");
  if (x.numel() % 4) throw std::runtime_error("dropout_bf16: numel % 4 != 0");
  require(y.numel() == x.numel(), "dropout_bf16: y size");
  need_p(p, "dropout_bf16");
  hip_check(dtfk_dropout_bf16(x.data_ptr(), y.data_ptr(), x.numel(), (float)p, (unsigned long long)seed, cur_stream()),
            "dropout");
}

// qkv [B, S, 3*NH*64] bf16 (pre-bias projection), bias [3*NH*64] fp32 or None,
// mask [B, S] additive fp32 or None -> ctx [B, S, NH*64] bf16, lse [B, NH, S] fp32
void attn_check(const at::Tensor& qkv, const c10::optional<at::Tensor>& bias, const c10::optional<at::Tensor>& mask,
                int64_t NH) {
  need(qkv, at::kBFloat16, "qkv");
  if (qkv.dim() != 3 || qkv.size(2) != 3 * NH * 64) throw std::runtime_error("attn: qkv must be [B, S, 3*NH*64]");
  if (!dtfk_attn_supported((int)qkv.size(1), 64)) throw std::runtime_error("attn: unsupported sequence length");
  if (bias.has_value()) {
    need(*bias, at::kFloat, "bias");
    if (bias->numel() != qkv.size(2)) throw std::runtime_error("attn: bias size");
  }
  if (mask.has_value()) {
    need(*mask, at::kFloat, "mask");
    if (mask->numel() != qkv.size(0) * qkv.size(1)) throw std::runtime_error("attn: mask must be [B, S]");
  }
}

void attn_fwd(at::Tensor qkv, c10::optional<at::Tensor> bias, c10::optional<at::Tensor> mask, at::Tensor ctx,
              at::Tensor lse, int64_t NH, double scale, double p, int64_t seed) {
  attn_check(qkv, bias, mask, NH);
  const int64_t B = qkv.size(0), S = qkv.size(1);
  need(ctx, at::kBFloat16, "ctx"); need(lse, at::kFloat, "lse");
  if (ctx.numel() != B * S * NH * 64 || lse.numel() != B * NH * S) throw std::runtime_error("attn_fwd: output sizes");
  hip_check(dtfk_attn_fwd(qkv.data_ptr(), opt_ptr<float>(bias), opt_ptr<float>(mask), ctx.data_ptr(),
                          lse.data_ptr<float>(), (int)B, (int)S, (int)NH, (float)scale, (float)p,
                          (unsigned long long)seed, cur_stream()),
            "attn_fwd");
}

// dbias (optional, with bpart [B * S / 16, 3 * NH * 64] fp32 scratch): the qkv
// bias gradient = column sums of dqkv, from per-wave partial sums the backward
// kernels write (no pass over dqkv); accumulate: dbias +=.
void attn_bwd(at::Tensor qkv, c10::optional<at::Tensor> bias, c10::optional<at::Tensor> mask, at::Tensor ctx,
              at::Tensor dctx, at::Tensor lse, at::Tensor Dbuf, at::Tensor dqkv, int64_t NH, double scale, double p,
              int64_t seed, c10::optional<at::Tensor> bpart, c10::optional<at::Tensor> dbias, bool accumulate) {
  attn_check(qkv, bias, mask, NH);
  const int64_t B = qkv.size(0), S = qkv.size(1);
  need(ctx, at::kBFloat16, "ctx"); need(dctx, at::kBFloat16, "dctx"); need(dqkv, at::kBFloat16, "dqkv");
  need(lse, at::kFloat, "lse"); need(Dbuf, at::kFloat, "Dbuf");
  if (ctx.numel() != B * S * NH * 64 || dctx.numel() != ctx.numel() || dqkv.numel() != qkv.numel() ||
      lse.numel() != B * NH * S || Dbuf.numel() != lse.numel())
    throw std::runtime_error("attn_bwd: sizes");
  const int64_t H3 = 3 * NH * 64, P = B * S / 16;
  if (bpart.has_value() != dbias.has_value()) throw std::runtime_error("attn_bwd: bpart and dbias go together");
  if (bpart.has_value()) {
    need(*bpart, at::kFloat, "bpart"); need(*dbias, at::kFloat, "dbias");
    if (bpart->numel() < P * H3 || dbias->numel() != H3 || !dbias->is_contiguous())
      throw std::runtime_error("attn_bwd: bpart needs B*S/16 x 3*NH*64 floats, dbias 3*NH*64");
  }
  hip_check(dtfk_attn_bwd(qkv.data_ptr(), opt_ptr<float>(bias), opt_ptr<float>(mask), ctx.data_ptr(), dctx.data_ptr(),
                          lse.data_ptr<float>(), Dbuf.data_ptr<float>(), dqkv.data_ptr(), (int)B, (int)S, (int)NH,
                          (float)scale, (float)p, (unsigned long long)seed,
                          bpart.has_value() ? bpart->data_ptr<float>() : nullptr, cur_stream()),
            "attn_bwd");
  if (bpart.has_value()) {
    const float* pp[1] = {bpart->data_ptr<float>()};
    float* po[1] = {dbias->data_ptr<float>()};
    hip_check(dtfk_colsum_partials_multi(pp, po, 1, (int)P, (int)H3, accumulate ? 1 : 0, cur_stream()),
              "attn_bwd dbias");
  }
}

void init_transformer(pybind11::module& m) {
  m.def("attn_supported", [](int64_t S, int64_t d) { return dtfk_attn_supported((int)S, (int)d) != 0; });
  m.def("attn_fwd", &attn_fwd);
  m.def("attn_bwd", &attn_bwd, py::arg("qkv"), py::arg("bias"), py::arg("mask"), py::arg("ctx"), py::arg("dctx"),
        py::arg("lse"), py::arg("Dbuf"), py::arg("dqkv"), py::arg("NH"), py::arg("scale"), py::arg("p"),
        py::arg("seed"), py::arg("bpart") = py::none(), py::arg("dbias") = py::none(), py::arg("accumulate") = false);
  m.def("bdrln_fwd", &bdrln_fwd);
  m.def("ln_fwd_f32in", &ln_fwd_f32in);
  m.def("emb_ln_fwd", &emb_ln_fwd);
  m.def("emb_bwd_aux", &emb_bwd_aux);
  m.def("ln_bwd", &ln_bwd, py::arg("dy"), py::arg("s"), py::arg("mean"), py::arg("rstd"), py::arg("gamma"),
        py::arg("ds"), py::arg("dxb"), py::arg("part"), py::arg("dgamma"), py::arg("dbeta"), py::arg("dbias"),
        py::arg("p"), py::arg("seed"), py::arg("accumulate") = false);
  m.def("colsum_bf16", &colsum_bf16, py::arg("x"), py::arg("part"), py::arg("out"), py::arg("accumulate") = false);
  m.def("slab_sum", &slab_sum, py::arg("slabs"), py::arg("out"), py::arg("accumulate") = false);
  m.def("bias_gelu_fwd", &bias_gelu_fwd);
  m.def("bias_gelu_bwd", &bias_gelu_bwd, py::arg("dy"), py::arg("x"), py::arg("bias"), py::arg("dx"), py::arg("part"),
        py::arg("dbias"), py::arg("accumulate") = false);
  m.def("softmax_fwd", &softmax_fwd);
  m.def("softmax_bwd", &softmax_bwd);
  m.def("dropout_bf16", &dropout_bf16);
}

}  // namespace dtf
