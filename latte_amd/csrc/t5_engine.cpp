// Host side of the T5 v1.1 encoder (latte_t5_* in include/latte_amd.h): weight slots under the transformers key names, the
// workspace, the relative-position buckets, and the launch sequence of one encode.  Kernels: t5.hip.
#include <cmath>
#include <string>
#include <vector>

#include "weight_store.h"

using namespace latte;

namespace {
enum T5Pack : int { TP_F32 = 0, TP_SPLIT };   // WeightSlot::kind; TP_SPLIT fills the pair dst / dst_lo
struct T5Layer {
  half_t *qkv_hi, *qkv_lo, *o_hi, *o_lo, *wi_hi, *wi_lo, *wo_hi, *wo_lo;
  float *ln0, *ln1;
};
}  // namespace

struct latte_t5 {
  latte_t5_config_t cfg;
  int max_batch, max_len, inner;
  DeviceArena arena;
  WeightSlots weights;
  std::vector<T5Layer> layers;
  float *emb = nullptr, *rel = nullptr, *table = nullptr, *final_ln = nullptr;
  int* bucket = nullptr;
  bool table_built = false;
  // workspace
  float *x = nullptr, *slabs = nullptr;
  half_t *n_hi = nullptr, *n_lo = nullptr, *c_hi = nullptr, *c_lo = nullptr, *a_hi = nullptr, *a_lo = nullptr, *qkv = nullptr;
};

namespace {

// a slot with its expected shape; `group` 0: the tied embedding, filled by either of its two names
void t5_slot(latte_t5* t, const std::string& key, std::vector<int64_t> shape, int kind, void* dst, void* dst_lo = nullptr, int group = -1) {
  int64_t numel = 1;
  for (int64_t d : shape) numel *= d;
  WeightSlot& s = t->weights.add(key, numel, kind, dst);
  s.shape = std::move(shape);
  s.dst_lo = dst_lo;
  s.group = group;
}

// T5Attention._relative_position_bucket (bidirectional) for rel = key - query, in the fp32 arithmetic of the reference:
// log(n / max_exact) / log(max_distance / max_exact) * (nb - max_exact), truncated
int t5_bucket(int rel, int num_buckets, int max_distance) {
  const int nb = num_buckets / 2;
  int out = rel > 0 ? nb : 0;
  const int n = std::abs(rel), max_exact = nb / 2;
  if (n < max_exact) return out + n;
  const float q = std::log((float)n / (float)max_exact) / (float)std::log((double)max_distance / (double)max_exact);
  const int large = max_exact + (int)(q * (float)(nb - max_exact));
  return out + std::min(large, nb - 1);
}

int t5_upload_buckets(int* dev, int num_buckets, int max_distance, int Lmax) {
  std::vector<int> b(2 * Lmax - 1);
  for (int d = 0; d < 2 * Lmax - 1; ++d) b[d] = t5_bucket(d - (Lmax - 1), num_buckets, max_distance);
  LATTE_HIP(hipMemcpy(dev, b.data(), sizeof(int) * b.size(), hipMemcpyHostToDevice));
  return LATTE_OK;
}

size_t round256(size_t r) { return (r + 255) / 256 * 256; }

}  // namespace

extern "C" {

int latte_t5_create(const latte_t5_config_t* c, int max_batch, int max_len, latte_t5_t** out) {
  if (!c || !out) return fail(LATTE_ERR_INVALID, "t5_create: null argument");
  if (c->compute_dtype != LATTE_DTYPE_F16) return fail(LATTE_ERR_INVALID, "t5_create: compute_dtype must be LATTE_DTYPE_F16");
  if (c->d_kv != 64) return fail(LATTE_ERR_INVALID, "t5_create: d_kv must be 64");
  if (c->d_model <= 0 || c->d_model % 64 || c->d_ff <= 0 || c->d_ff % 64)
    return fail(LATTE_ERR_INVALID, "t5_create: d_model and d_ff must be multiples of 64");
  if (c->num_heads <= 0 || c->num_layers <= 0 || c->vocab_size <= 0) return fail(LATTE_ERR_INVALID, "t5_create: bad configuration");
  if (c->relative_attention_num_buckets < 4 || c->relative_attention_num_buckets % 4 || c->relative_attention_max_distance <= c->relative_attention_num_buckets / 4)
    return fail(LATTE_ERR_INVALID, "t5_create: relative_attention_num_buckets must be a multiple of 4 and max_distance above num_buckets / 4");
  if (max_batch <= 0 || max_len <= 0 || max_len > 512) return fail(LATTE_ERR_INVALID, "t5_create: max_batch >= 1 and 1 <= max_len <= 512");
  latte_t5* t = new latte_t5();
  t->cfg = *c;
  t->max_batch = max_batch;
  t->max_len = max_len;
  const int D = c->d_model, F = c->d_ff, inner = c->num_heads * c->d_kv, H = c->num_heads, nbk = c->relative_attention_num_buckets;
  t->inner = inner;
  int rc;
#define TRY(x) do { if ((rc = (x))) { latte_t5_destroy(t); return rc; } } while (0)
  TRY(t->arena.alloc(&t->emb, (size_t)c->vocab_size * D, false));
  t5_slot(t, "shared.weight", {c->vocab_size, D}, TP_F32, t->emb, nullptr, 0);
  t5_slot(t, "encoder.embed_tokens.weight", {c->vocab_size, D}, TP_F32, t->emb, nullptr, 0);
  TRY(t->arena.alloc(&t->rel, (size_t)nbk * H, false));
  TRY(t->arena.alloc(&t->table, (size_t)H * (2 * max_len - 1), false));
  TRY(t->arena.alloc(&t->bucket, (size_t)2 * max_len - 1, false));
  TRY(t5_upload_buckets(t->bucket, nbk, c->relative_attention_max_distance, max_len));
  t->layers.resize(c->num_layers);
  for (int i = 0; i < c->num_layers; ++i) {
    T5Layer& l = t->layers[i];
    const std::string a = "encoder.block." + std::to_string(i) + ".layer.0.", f = "encoder.block." + std::to_string(i) + ".layer.1.";
    TRY(t->arena.alloc(&l.qkv_hi, (size_t)3 * inner * D, false)); TRY(t->arena.alloc(&l.qkv_lo, (size_t)3 * inner * D, false));
    TRY(t->arena.alloc(&l.o_hi, (size_t)D * inner, false)); TRY(t->arena.alloc(&l.o_lo, (size_t)D * inner, false));
    TRY(t->arena.alloc(&l.wi_hi, (size_t)2 * F * D, false)); TRY(t->arena.alloc(&l.wi_lo, (size_t)2 * F * D, false));
    TRY(t->arena.alloc(&l.wo_hi, (size_t)D * F, false)); TRY(t->arena.alloc(&l.wo_lo, (size_t)D * F, false));
    TRY(t->arena.alloc(&l.ln0, D, false)); TRY(t->arena.alloc(&l.ln1, D, false));
    const char* qkv_names[3] = {"q", "k", "v"};
    for (int j = 0; j < 3; ++j)
      t5_slot(t, a + "SelfAttention." + qkv_names[j] + ".weight", {inner, D}, TP_SPLIT, l.qkv_hi + (size_t)j * inner * D,
              l.qkv_lo + (size_t)j * inner * D);
    t5_slot(t, a + "SelfAttention.o.weight", {D, inner}, TP_SPLIT, l.o_hi, l.o_lo);
    if (i == 0) t5_slot(t, a + "SelfAttention.relative_attention_bias.weight", {nbk, H}, TP_F32, t->rel);
    t5_slot(t, a + "layer_norm.weight", {D}, TP_F32, l.ln0);
    t5_slot(t, f + "DenseReluDense.wi_0.weight", {F, D}, TP_SPLIT, l.wi_hi, l.wi_lo);
    t5_slot(t, f + "DenseReluDense.wi_1.weight", {F, D}, TP_SPLIT, l.wi_hi + (size_t)F * D, l.wi_lo + (size_t)F * D);
    t5_slot(t, f + "DenseReluDense.wo.weight", {D, F}, TP_SPLIT, l.wo_hi, l.wo_lo);
    t5_slot(t, f + "layer_norm.weight", {D}, TP_F32, l.ln1);
  }
  TRY(t->arena.alloc(&t->final_ln, D, false));
  t5_slot(t, "encoder.final_layer_norm.weight", {D}, TP_F32, t->final_ln);
  // workspace: operand pairs in whole 256-row blocks (the projection stages rows past M, results of those rows are never stored)
  const size_t M = (size_t)max_batch * max_len, Mp = round256(M);
  TRY(t->arena.alloc(&t->x, M * D, false));
  TRY(t->arena.alloc(&t->n_hi, Mp * D)); TRY(t->arena.alloc(&t->n_lo, Mp * D));
  TRY(t->arena.alloc(&t->c_hi, Mp * inner)); TRY(t->arena.alloc(&t->c_lo, Mp * inner));
  TRY(t->arena.alloc(&t->a_hi, Mp * F)); TRY(t->arena.alloc(&t->a_lo, Mp * F));
  TRY(t->arena.alloc(&t->qkv, M * 3 * inner, false));
  size_t slab = 0;
  const int shapes[4][2] = {{3 * inner, D}, {D, inner}, {2 * F, D}, {D, F}};
  for (auto& s : shapes) slab = std::max(slab, (size_t)t5_proj_splits(s[0], s[1]) * M * s[0]);
  TRY(t->arena.alloc(&t->slabs, slab, false));
#undef TRY
  *out = t;
  return LATTE_OK;
}

void latte_t5_destroy(latte_t5_t* t) {
  delete t;   // the arena frees every device block
}

int latte_t5_num_keys(const latte_t5_t* t) { return t ? t->weights.size() : 0; }
const char* latte_t5_key(const latte_t5_t* t, int i) { return t ? t->weights.key(i) : nullptr; }

int latte_t5_load_weight(latte_t5_t* t, const char* key, const float* data, const int64_t* shape, int ndim, void* stream) {
  if (!t || !key || !data || !shape) return fail(LATTE_ERR_INVALID, "t5_load_weight: null argument");
  WeightSlot* slot = nullptr;
  if (int rc = t->weights.find("t5_load_weight", key, &slot)) return rc;
  WeightSlot& s = *slot;
  bool same = ndim == (int)s.shape.size();
  for (int i = 0; same && i < ndim; ++i) same = shape[i] == s.shape[i];
  if (!same) {
    auto str = [](const int64_t* p, size_t n) { std::string r = "("; for (size_t i = 0; i < n; ++i) r += (i ? ", " : "") + std::to_string(p[i]); return r + ")"; };
    return fail(LATTE_ERR_INVALID, std::string("t5_load_weight: size mismatch for '") + key + "': got shape " + str(shape, ndim) +
                                       ", expected " + str(s.shape.data(), s.shape.size()));
  }
  const size_t numel = (size_t)s.numel;
  hipStream_t st = (hipStream_t)stream;
  if (s.kind == TP_F32) {
    LATTE_HIP(hipMemcpyAsync(s.dst, data, sizeof(float) * numel, hipMemcpyDeviceToDevice, st));
  } else {
    int rc = launch_t5_pack_w(data, (half_t*)s.dst, (half_t*)s.dst_lo, numel, st);
    if (rc) return rc;
  }
  s.loaded = true;   // (a device source: nothing to drain)
  if (s.dst == t->rel) t->table_built = false;
  return LATTE_OK;
}

int latte_t5_check_weights(latte_t5_t* t) {
  if (!t) return fail(LATTE_ERR_INVALID, "t5_check_weights: null");
  return t->weights.check_loaded();
}

int latte_t5_forward(latte_t5_t* t, const int64_t* ids, const float* mask, int B, int L, float* out, void* stream) {
  if (!t || !ids || !out) return fail(LATTE_ERR_INVALID, "t5_forward: null argument");
  if (B <= 0 || B > t->max_batch || L <= 0 || L > t->max_len)
    return fail(LATTE_ERR_STATE, "t5_forward: batch " + std::to_string(B) + " x length " + std::to_string(L) + " exceeds the workspace (" +
                                     std::to_string(t->max_batch) + " x " + std::to_string(t->max_len) + ")");
  int rc = latte_t5_check_weights(t);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const latte_t5_config_t& c = t->cfg;
  const int D = c.d_model, F = c.d_ff, inner = t->inner, H = c.num_heads, M = B * L;
  const float eps = c.layer_norm_epsilon;
#define TRY(x) do { if ((rc = (x))) return rc; } while (0)
  if (!t->table_built) {
    TRY(launch_t5_bias_table(t->rel, t->bucket, t->table, H, 2 * t->max_len - 1, st));
    t->table_built = true;
  }
  TRY(launch_t5_embed(ids, t->emb, t->x, M, D, c.vocab_size, st));
  TRY(launch_t5_res_norm(t->x, nullptr, 0, 0, t->layers[0].ln0, t->n_hi, t->n_lo, nullptr, M, D, eps, st));
  for (int i = 0; i < c.num_layers; ++i) {
    const T5Layer& l = t->layers[i];
    size_t stride = (size_t)M * 3 * inner;
    TRY(launch_t5_proj(t->n_hi, t->n_lo, l.qkv_hi, l.qkv_lo, t->slabs, stride, M, 3 * inner, D, st));
    TRY(launch_t5_reduce_h16(t->slabs, t5_proj_splits(3 * inner, D), stride, t->qkv, stride, st));
    TRY(launch_t5_attention(t->qkv, t->table, mask, t->c_hi, t->c_lo, B, L, H, t->max_len, st));
    stride = (size_t)M * D;
    TRY(launch_t5_proj(t->c_hi, t->c_lo, l.o_hi, l.o_lo, t->slabs, stride, M, D, inner, st));
    TRY(launch_t5_res_norm(t->x, t->slabs, t5_proj_splits(D, inner), stride, l.ln1, t->n_hi, t->n_lo, nullptr, M, D, eps, st));
    stride = (size_t)M * 2 * F;
    TRY(launch_t5_proj(t->n_hi, t->n_lo, l.wi_hi, l.wi_lo, t->slabs, stride, M, 2 * F, D, st));
    TRY(launch_t5_gated_act(t->slabs, t5_proj_splits(2 * F, D), stride, t->a_hi, t->a_lo, M, F, st));
    stride = (size_t)M * D;
    TRY(launch_t5_proj(t->a_hi, t->a_lo, l.wo_hi, l.wo_lo, t->slabs, stride, M, D, F, st));
    const bool last = i + 1 == c.num_layers;
    TRY(launch_t5_res_norm(t->x, t->slabs, t5_proj_splits(D, F), stride, last ? t->final_ln : t->layers[i + 1].ln0, t->n_hi, t->n_lo,
                           last ? out : nullptr, M, D, eps, st));
  }
#undef TRY
  return LATTE_OK;
}

// ------------------------------------------------------------------ test hooks (include/latte_amd_debug.h)
int latte_debug_t5_embed(const int64_t* ids, const float* table, float* x, int M, int D, int vocab, void* stream) {
  return launch_t5_embed(ids, table, x, M, D, vocab, (hipStream_t)stream);
}
int latte_debug_t5_rmsnorm(float* x, const float* w, void* out_hi, void* out_lo, float* out_f32, int M, int D, float eps, void* stream) {
  return launch_t5_res_norm(x, nullptr, 0, 0, w, (half_t*)out_hi, (half_t*)out_lo, out_f32, M, D, eps, (hipStream_t)stream);
}
int latte_debug_t5_bucket(int rel, int num_buckets, int max_distance) { return t5_bucket(rel, num_buckets, max_distance); }
int latte_debug_t5_bias_table(const float* rel, int heads, int num_buckets, int max_distance, int max_len, float* table, void* stream) {
  if (!rel || !table || heads <= 0 || max_len <= 0) return fail(LATTE_ERR_INVALID, "debug_t5_bias_table: bad arguments");
  int* dev = nullptr;
  LATTE_HIP(hipMalloc((void**)&dev, sizeof(int) * (2 * max_len - 1)));
  int rc = t5_upload_buckets(dev, num_buckets, max_distance, max_len);
  if (!rc) rc = launch_t5_bias_table(rel, dev, table, heads, 2 * max_len - 1, (hipStream_t)stream);
  if (!rc && hipStreamSynchronize((hipStream_t)stream) != hipSuccess) rc = fail(LATTE_ERR_HIP, "debug_t5_bias_table: device error");
  (void)hipFree(dev);
  return rc;
}
int latte_debug_t5_attention(const void* qkv, const float* table, const float* mask, void* out_hi, void* out_lo, int B, int L, int heads,
                             int max_len, void* stream) {
  return launch_t5_attention((const half_t*)qkv, table, mask, (half_t*)out_hi, (half_t*)out_lo, B, L, heads, max_len, (hipStream_t)stream);
}
int latte_debug_t5_gated_act(const float* u, void* out_hi, void* out_lo, int M, int F, void* stream) {
  return launch_t5_gated_act(u, 1, 0, (half_t*)out_hi, (half_t*)out_lo, M, F, (hipStream_t)stream);
}
int latte_debug_t5_pack(const float* w, void* hi, void* lo, int64_t n, void* stream) {
  return launch_t5_pack_w(w, (half_t*)hi, (half_t*)lo, (size_t)n, (hipStream_t)stream);
}
int latte_debug_t5_proj_splits(int N, int K) { return (N > 0 && N % 64 == 0 && K > 0) ? t5_proj_splits(N, K) : 0; }
int latte_debug_t5_proj(const void* a_hi, const void* a_lo, const void* w_hi, const void* w_lo, float* slabs, float* out, int M, int N, int K,
                        void* stream) {
  if (!a_hi || !a_lo || !w_hi || !w_lo || !slabs || !out) return fail(LATTE_ERR_INVALID, "debug_t5_proj: null argument");
  const size_t stride = (size_t)M * N;
  int rc = launch_t5_proj((const half_t*)a_hi, (const half_t*)a_lo, (const half_t*)w_hi, (const half_t*)w_lo, slabs, stride, M, N, K,
                          (hipStream_t)stream);
  if (rc) return rc;
  return launch_t5_res_norm(out, slabs, t5_proj_splits(N, K), stride, nullptr, nullptr, nullptr, nullptr, M, N, 0.f, (hipStream_t)stream);
}

}  // extern "C"
