// persistent 4-wave GEMM, LayerNorm-folded epilogues of the encoder towers (see GemmParams::ln_stats and gemm_w4_launch.h):
//   SigLIP / Whisper  LayerNorm -> q/k/v projection (MODE_QKV_VT, or MODE_PLAIN head-major)  and  LayerNorm -> fc1 + GELU (MODE_PLAIN),
//   and the producer side: the bias + residual epilogue that also emits the rows' per-strip partial sums (GemmParams::stat_part)
#include "gemm_w4_launch.h"
template <typename T>
static int lnf(GemmKernel k, const GemmParams& p, int batch, hipStream_t st) {
    switch (k) { VIDI_W4_LNF_KERNELS(VIDI_W4_LAUNCH_CASE) default: return VIDI_ERR_ARG; }
}
int vidi_w4_lnf(GemmKernel k, const GemmParams& p, int batch, int dtype, hipStream_t st) {
    return dtype == VIDI_DT_BF16 ? lnf<BF16>(k, p, batch, st) : lnf<F16>(k, p, batch, st);
}
