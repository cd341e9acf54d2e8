// extern "C" boundary (include/denoise_hip_data.h): the input side of the trainers, the device-resident
// patch sampler that stands in for finetune.py:100-150's DenoisePatchDataset + DataLoader.
#include <string>

#include "capi_common.h"
#include "denoise_hip_data.h"

using namespace dn;

extern "C" {

dn_status dn_patch_sample(const float* clean_pool, const float* noisy_pool, int64_t pool_elems,
                          const int64_t* table, int M, int C, const int32_t* img_idx, int N, int ps,
                          uint64_t seed, uint64_t offset, uint64_t item_base,
                          const int32_t* origins_in, float* clean_out, float* noisy_out,
                          int32_t* origins_out, void* stream) {
  return guarded([&] {
    if (N < 0 || M < 1 || C < 1 || ps < 1)
      return fail(DN_ERR_ARG, "need N >= 0 and M, C, ps >= 1");
    if (N == 0) return DN_OK;
    if (!clean_pool || !table || !img_idx || !clean_out || (noisy_pool && !noisy_out))
      return fail(DN_ERR_ARG, "null argument");
    if (pool_elems < 1) return fail(DN_ERR_ARG, "pool_elems >= 1 required");
    if ((int64_t)C * ps * ps > 0x7fffffffL)
      return fail(DN_ERR_ARG, "C * ps * ps too large (2^31 elements per patch)");
    if (((uintptr_t)clean_out | (uintptr_t)noisy_out) & 15)
      return fail(DN_ERR_ARG, "clean_out and noisy_out must be 16-byte aligned");
    return hip_status(launch_patch_sample(clean_pool, noisy_pool, pool_elems,
                                          reinterpret_cast<const long*>(table), M, C, img_idx, N,
                                          ps, seed, offset, item_base, origins_in, clean_out,
                                          noisy_out, origins_out, (hipStream_t)stream),
                      "dn_patch_sample");
  });
}

}  // extern "C"
