// host entry point of vocab_logprob.hip (a header of its own: kernels.h belongs to the digest that keys the GEMM family's PMC traffic
// record, which these kernels are not part of)
#pragma once
#include <hip/hip_runtime.h>
// partials of one row: a pass-1 block writes one 16-byte record; include/vidi_hip.h sizes the caller's workspace from the product
#define TOKEN_LOGPROB_MAX_PARTS 128
#define TOKEN_LOGPROB_PART_BYTES 16
// idx / lse / logprob / rank of R rows of logits [R, V] (row stride ld); arguments already validated (capi.hip)
int vidi_token_logprob_dispatch(const void* logits, const long long* targets, long long* idx, float* lse, float* logprob, int* rank, int R, int V,
                                long long ld, float cap, int dtype, void* workspace, hipStream_t st);
