/*
 * denoise_hip_data.h — the input side of libdenoise_hip.so: what feeds the trainers.
 *
 * Same library, same conventions as denoise_hip.h (raw device pointers, a hipStream_t as void*,
 * no allocation, no host synchronisation, dn_status + dn_last_error).  Kept as its own header so
 * that denoise_hip.h stays the network / loss / optimiser / evaluation boundary it has been since
 * ABI revision 5; nothing here changes that revision (symbols are added, no argument list of
 * denoise_hip.h changes).  The Python binding is image_denoising_amd/_lib.py DATA_SIGNATURES.
 */
#ifndef DENOISE_HIP_DATA_H
#define DENOISE_HIP_DATA_H

#include "denoise_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- data: device-resident paired patch sampler (finetune.py:100-150) -------------- */
/* One gather launch in place of DenoisePatchDataset + DataLoader.  clean_pool / noisy_pool hold
   the M images back to back as fp32 pixel values (0..255), CHW per image, pool_elems floats each;
   table [M][3] (device int64) gives each image's element offset, H and W (sizes may differ).
   noisy_pool may be null (a clean-only set): then noisy_out is not written.  For item i of image
   img_idx[i] (device int32 [N]) the outputs [N, C, ps, ps] are the same ps x ps window of both
   pools, each value x / 255.0f by fp32 division.  The window's origin is origins_in[i] = (top,
   left) when origins_in (device int32 [N][2]) is given, else
     top  = (philox_u32(seed, offset, 2g)     * (H - ps + 1)) >> 32,
     left = (philox_u32(seed, offset, 2g + 1) * (W - ps + 1)) >> 32,   g = item_base + i,
   a pure function of the global ordinal g, so a rank's shard equals its slice of the whole batch.
   origins_out (nullable, device int32 [N][2]) receives the origins used.  An item whose img_idx is
   outside [0, M), whose image is smaller than ps or does not lie inside the pool, or whose explicit
   origin is outside the image gets zeros and the origin (-1, -1); nothing outside an image is
   read.  clean_out / noisy_out: 16-byte aligned.  N == 0: DN_OK, nothing launched.  DN_ERR_ARG: a
   null required pointer, N < 0, M < 1, C < 1, ps < 1, pool_elems < 1. */
dn_status dn_patch_sample(const float* clean_pool, const float* noisy_pool, int64_t pool_elems,
                          const int64_t* table, int M, int C, const int32_t* img_idx, int N, int ps,
                          uint64_t seed, uint64_t offset, uint64_t item_base,
                          const int32_t* origins_in, float* clean_out, float* noisy_out,
                          int32_t* origins_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DENOISE_HIP_DATA_H */
