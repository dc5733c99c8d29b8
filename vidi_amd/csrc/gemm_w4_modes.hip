// persistent 4-wave GEMM, fused-epilogue modes (GeGLU / QKV + V-transpose / K,V cache tiles), both dtypes (see gemm_w4_launch.h)
#include "gemm_w4_launch.h"
template <typename T>
static int modes(GemmKernel k, const GemmParams& p, int batch, hipStream_t st) {
    switch (k) { VIDI_W4_MODES_KERNELS(VIDI_W4_LAUNCH_CASE) default: return VIDI_ERR_ARG; }
}
int vidi_w4_modes(GemmKernel k, const GemmParams& p, int batch, int dtype, hipStream_t st) {
    return dtype == VIDI_DT_BF16 ? modes<BF16>(k, p, batch, st) : modes<F16>(k, p, batch, st);
}
