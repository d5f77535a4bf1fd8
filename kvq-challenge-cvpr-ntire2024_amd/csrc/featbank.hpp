// What csrc/featbank.hip, csrc/headtrain.hip and csrc/simple_headtrain.hip share: the element types of a feature bank, the widening
// quad load, the index clamp, and the one argument form behind the dense and the bank entries of the two training steps.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace kvq {

typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;

// ---- a bank row's elements: float, _Float16 or __bf16.  Widening to fp32 is exact for both 16-bit types.
// Four consecutive elements at p (16-byte aligned for float, 8-byte for the 16-bit types) as fp32.
__device__ __forceinline__ f32x4 bank_load4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 bank_load4(const _Float16* p) {
  const f16x4 v = *reinterpret_cast<const f16x4*>(p);
  return (f32x4){(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
__device__ __forceinline__ f32x4 bank_load4(const __bf16* p) {
  const u32x2 v = *reinterpret_cast<const u32x2*>(p);
  return (f32x4){__uint_as_float(v[0] << 16), __uint_as_float(v[0] & 0xffff0000u), __uint_as_float(v[1] << 16),
                 __uint_as_float(v[1] & 0xffff0000u)};
}

// The bank row of batch position b.  IDX = false: the dense entries, row b.  IDX = true: index[b] clamped into [0, n_rows), so that no
// index value can cause a read outside the bank.
template <bool IDX>
__device__ __forceinline__ long bank_row(const int32_t* __restrict__ index, long n_rows, long b) {
  if constexpr (!IDX) {
    return b;
  } else {
    const long r = index[b];
    return r < 0 ? 0 : (r < n_rows ? r : n_rows - 1);
  }
}

static inline bool bank_dtype_ok(int dtype) { return dtype == KVQ_DT_FP32 || dtype == KVQ_DT_FP16 || dtype == KVQ_DT_BF16; }
static inline size_t bank_elem_bytes(int dtype) { return dtype == KVQ_DT_FP32 ? 4 : 2; }

// f(float{}), f(_Float16{}) or f(__bf16{}) for a dtype that passed bank_dtype_ok: a launch site names its kernel once, as
// kernel<decltype(e), ...>
template <class F>
int with_bank_elem(int dtype, F&& f) {
  if (dtype == KVQ_DT_FP32) return f(float{});
  return dtype == KVQ_DT_FP16 ? f(_Float16{}) : f(__bf16{});
}

// ---- the features of one training step as its launches see them: dense fp32 [B][L][C] (index == NULL: KvqHeadTrainArgs), or B rows of a
// bank picked by a device index (KvqHeadTrainBankArgs)
struct HeadTrainFeat {
  const void* rows;
  int dtype;
  const int32_t* index;
  long n_rows;
};
struct HeadTrainCall {
  HeadTrainFeat feat;
  int B, L, C, hidden;
  const float* params;
  float p_drop;
  uint32_t seed, step;
  void* workspace;
  size_t workspace_bytes;
  float* score;
  const float* dscore;
  float* grads;
};

inline HeadTrainCall headtrain_call(const KvqHeadTrainArgs* a) {
  return {{a->feat, KVQ_DT_FP32, nullptr, a->B}, a->B, a->L, a->C, a->hidden, a->params, a->p_drop, a->seed, a->step, a->workspace,
          a->workspace_bytes, a->score, a->dscore, a->grads};
}
inline HeadTrainCall headtrain_call(const KvqHeadTrainBankArgs* a) {
  return {{a->bank.rows, a->bank.dtype, a->index, (long)a->bank.n_rows}, a->B, a->L, a->C, a->hidden, a->params, a->p_drop, a->seed,
          a->step, a->workspace, a->workspace_bytes, a->score, a->dscore, a->grads};
}

// The host checks a bank entry makes before the checks it shares with its dense entry (which then see the bank's rows as `feat`).
int headtrain_bank_check(const KvqHeadTrainBankArgs* a, const char* who);

// f(elem, std::true_type / std::false_type) for the element type and for whether the call has an index; the dense entries are
// (float, false)
template <class F>
int with_headtrain_feat(const HeadTrainFeat& ft, F&& f) {
  if (!ft.index) return f(float{}, std::false_type{});
  return with_bank_elem(ft.dtype, [&](auto e) { return f(e, std::true_type{}); });
}

}  // namespace kvq
