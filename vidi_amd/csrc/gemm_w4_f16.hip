// persistent 4-wave GEMM, MODE_PLAIN instantiations, fp16 (see gemm_w4_launch.h)
#include "gemm_w4_launch.h"
int vidi_w4_plain_f16(GemmKernel k, const GemmParams& p, int batch, hipStream_t st) { return w4_plain_launch<F16>(k, p, batch, st); }
