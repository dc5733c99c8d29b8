// persistent 4-wave GEMM, MODE_PLAIN instantiations, bf16 (see gemm_w4_launch.h)
#include "gemm_w4_launch.h"
int vidi_w4_plain_bf16(GemmKernel k, const GemmParams& p, int batch, hipStream_t st) { return w4_plain_launch<BF16>(k, p, batch, st); }
