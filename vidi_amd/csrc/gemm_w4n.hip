// persistent 4-wave GEMM, 288 x 224 tiles (gemm_w4n.h): the bias + residual (+ LayerNorm statistics) epilogues of the encoder towers'
// out_proj / fc2, and the LayerNorm-folded head-major q | k | v projection, at widths that are multiples of 288 but not of 256
// (SigLIP: N = 1 152, 3 456); gemm_route.h decides when they run
#include "gemm_w4n.h"
#include "gemm_w4_launch.h"
int vidi_w4n(GemmKernel k, const GemmParams& p, int dtype, hipStream_t st) {
#define VIDI_W4N_LAUNCH_CASE(name, MODE, REPKV, ...) \
    case name: return dtype == VIDI_DT_BF16 ? launch_w4n<BF16, Epi<__VA_ARGS__>>(p, st) : launch_w4n<F16, Epi<__VA_ARGS__>>(p, st);
    switch (k) { VIDI_W4N_KERNELS(VIDI_W4N_LAUNCH_CASE) default: return VIDI_ERR_ARG; }
}
