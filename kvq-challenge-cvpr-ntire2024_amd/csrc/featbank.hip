// The feature bank of head fine-tuning (gfx950): the cached features of a frozen trunk, K train-phase draws per video, stored once as
// [n_rows][L][C] in fp32, fp16 or bf16.  Two launches live here: the store that narrows a trunk output into its rows, and
// the gather that widens rows back into a dense fp32 batch (prediction, tests).  The training launches of headtrain.hip and
// simple_headtrain.hip read the rows in place (featbank.hpp).
#include "featbank.hpp"

namespace kvq {

// One element quad, narrowed.  bad: the quad held a NaN, or (fp16) a value past +-65504, which is stored as +-65504.
__device__ __forceinline__ void bank_store4(float* p, f32x4 v, bool& bad) {
#pragma unroll
  for (int k = 0; k < 4; ++k) bad |= v[k] != v[k];
  *reinterpret_cast<f32x4*>(p) = v;
}
__device__ __forceinline__ void bank_store4(_Float16* p, f32x4 v, bool& bad) {
  f16x4 h;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool past = fabsf(v[k]) > 65504.0f;                      // false for a NaN, which converts to a NaN
    bad |= past || v[k] != v[k];
    h[k] = (_Float16)(past ? copysignf(65504.0f, v[k]) : v[k]);    // v_cvt_f16_f32: round to nearest even
  }
  *reinterpret_cast<f16x4*>(p) = h;
}
__device__ __forceinline__ void bank_store4(__bf16* p, f32x4 v, bool& bad) {
#pragma unroll
  for (int k = 0; k < 4; ++k) bad |= v[k] != v[k];
  *reinterpret_cast<u32x2*>(p) = (u32x2){pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};   // v_cvt_pk_bf16_f32: round to nearest even
}

// grid ceil(n L C / 4 / 256), 256 threads: thread = one channel quad of one token.  C % 4 == 0, the strides are multiples of 4.
template <typename E>
__global__ __launch_bounds__(256) void feature_bank_store_kernel(const float* __restrict__ feat, long quads, int L, int C, long stride_n,
                                                                 long stride_l, E* __restrict__ rows, int32_t* __restrict__ flag) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= quads) return;
  const int cq = C / 4;
  const long tok = q / cq;
  const int c = (int)(q - tok * cq) * 4;
  const long i = tok / L;
  const int l = (int)(tok - i * L);
  const f32x4 v = *reinterpret_cast<const f32x4*>(feat + (size_t)i * stride_n + (size_t)l * stride_l + c);
  bool bad = false;
  bank_store4(rows + (size_t)tok * C + c, v, bad);
  if (bad && flag) *flag = 1;
}

// grid ceil(B L C / 4 / 256), 256 threads: thread = one channel quad of one output token.
template <typename E>
__global__ __launch_bounds__(256) void feature_bank_rows_kernel(const E* __restrict__ rows, const int32_t* __restrict__ index, long n_rows,
                                                                long quads, int L, int C, float* __restrict__ out) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= quads) return;
  const int cq = C / 4;
  const long tok = q / cq;
  const int c = (int)(q - tok * cq) * 4;
  const long b = tok / L;
  const long l = tok - b * L;
  const size_t src = ((size_t)bank_row(index, n_rows, b) * L + l) * C + c;
  *reinterpret_cast<f32x4*>(out + (size_t)tok * C + c) = bank_load4(rows + src);
}

static int bank_check(const KvqFeatureBank* bank, const char* who) {
  KVQ_REQUIRE(bank && bank->rows, KVQ_ERR_NULL, "%s: NULL pointer", who);
  KVQ_REQUIRE(bank_dtype_ok(bank->dtype), KVQ_ERR_UNSUPPORTED, "%s: bank dtype %d (fp32, fp16 or bf16)", who, bank->dtype);
  KVQ_REQUIRE(((uintptr_t)bank->rows & 15) == 0, KVQ_ERR_UNSUPPORTED, "%s: the bank's rows must be 16-byte aligned", who);
  KVQ_REQUIRE(bank->C >= 4 && bank->C % 4 == 0, KVQ_ERR_UNSUPPORTED, "%s: bank C %d is not a multiple of 4", who, bank->C);
  KVQ_REQUIRE(bank->n_rows >= 1 && bank->L >= 1, KVQ_ERR_SHAPE, "%s: bank of %lld rows, L %d", who, (long long)bank->n_rows, bank->L);
  return KVQ_OK;
}

int headtrain_bank_check(const KvqHeadTrainBankArgs* a, const char* who) {
  KVQ_REQUIRE(a && a->index, KVQ_ERR_NULL, "%s: NULL pointer", who);
  if (int rc = bank_check(&a->bank, who)) return rc;
  KVQ_REQUIRE(((uintptr_t)a->index & 3) == 0, KVQ_ERR_UNSUPPORTED, "%s: index must be 4-byte aligned", who);
  // a step's L (simpleVQAHead: T) below 1 cannot be the bank's, which is at least 1: refused by its own name, with the mismatch's status
  KVQ_REQUIRE(a->L >= 1, KVQ_ERR_SHAPE, "%s: the step's L | T %d below 1", who, a->L);
  KVQ_REQUIRE(a->bank.L == a->L && a->bank.C == a->C, KVQ_ERR_SHAPE, "%s: the bank's rows are (L %d, C %d), the step's (L %d, C %d)", who,
              a->bank.L, a->bank.C, a->L, a->C);
  KVQ_REQUIRE((double)a->B * a->L * a->C < 4294967296.0, KVQ_ERR_SHAPE, "%s: B*L*C = %g elements exceed the 32-bit batch position", who,
              (double)a->B * a->L * a->C);
  return KVQ_OK;
}

}  // namespace kvq

extern "C" int kvq_feature_bank_store(const float* feat, int64_t n, int64_t stride_n, int64_t stride_l, const KvqFeatureBank* bank,
                                      int64_t first_row, int32_t* flag, void* stream) {
  using namespace kvq;
  const char* who = "kvq_feature_bank_store";
  KVQ_REQUIRE(feat, KVQ_ERR_NULL, "%s: NULL pointer", who);
  if (int rc = bank_check(bank, who)) return rc;
  KVQ_REQUIRE(n >= 1 && first_row >= 0 && n <= bank->n_rows && first_row <= bank->n_rows - n, KVQ_ERR_SHAPE,
              "%s: rows %lld .. %lld + %lld of a bank of %lld", who, (long long)first_row, (long long)first_row, (long long)n,
              (long long)bank->n_rows);
  KVQ_REQUIRE(((uintptr_t)feat & 15) == 0 && ((uintptr_t)flag & 3) == 0 && stride_n % 4 == 0 && stride_l % 4 == 0, KVQ_ERR_UNSUPPORTED,
              "%s: feat must be 16-byte aligned with strides (%lld, %lld) that are multiples of 4, flag 4-byte aligned", who,
              (long long)stride_n, (long long)stride_l);
  KVQ_REQUIRE(stride_n >= 0 && stride_l >= bank->C, KVQ_ERR_SHAPE, "%s: token stride %lld below C %d", who, (long long)stride_l, bank->C);
  const long quads = (long)n * bank->L * (bank->C / 4);
  KVQ_REQUIRE((double)n * bank->L * (bank->C / 4) < 256.0 * 2147483647.0, KVQ_ERR_SHAPE, "%s: %lld samples are more than one launch covers",
              who, (long long)n);
  const size_t off = (size_t)first_row * bank->L * bank->C;
  return with_bank_elem(bank->dtype, [&](auto e) {
    using E = decltype(e);
    return launch("feature_bank_store_kernel", feature_bank_store_kernel<E>, grid_1d(quads), dim3(256), 0, stream, feat, quads, bank->L,
                  bank->C, (long)stride_n, (long)stride_l, static_cast<E*>(bank->rows) + off, flag);
  });
}

extern "C" int kvq_feature_bank_rows(const KvqFeatureBank* bank, const int32_t* index, int64_t B, float* out, void* stream) {
  using namespace kvq;
  const char* who = "kvq_feature_bank_rows";
  KVQ_REQUIRE(index && out, KVQ_ERR_NULL, "%s: NULL pointer", who);
  if (int rc = bank_check(bank, who)) return rc;
  KVQ_REQUIRE(((uintptr_t)out & 15) == 0 && ((uintptr_t)index & 3) == 0, KVQ_ERR_UNSUPPORTED,
              "%s: out must be 16-byte aligned, index 4-byte aligned", who);
  KVQ_REQUIRE(B >= 1 && (double)B * bank->L * (bank->C / 4) < 256.0 * 2147483647.0, KVQ_ERR_SHAPE, "%s: B %lld", who, (long long)B);
  const long quads = (long)B * bank->L * (bank->C / 4);
  return with_bank_elem(bank->dtype, [&](auto e) {
    using E = decltype(e);
    return launch("feature_bank_rows_kernel", feature_bank_rows_kernel<E>, grid_1d(quads), dim3(256), 0, stream,
                  static_cast<const E*>(bank->rows), index, (long)bank->n_rows, quads, bank->L, bank->C, out);
  });
}
