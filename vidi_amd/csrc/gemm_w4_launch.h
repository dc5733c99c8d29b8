// Host-side launch of the persistent 4-wave GEMM (gemm_w4.h).  The instantiations are spread over several translation units
// (gemm_w4_*.hip) so the library builds in parallel; each switches from the router's enumerator (gemm_route.h) to its own rows of
// the instantiation table and exports one plain launcher declared here.
#pragma once
#include "gemm_w4.h"
#include "gemm_route.h"

template <typename T, int MODE, bool REPKV, typename EPI, int PATCH = 0>
static int launch_w4(const GemmParams& p, int batch, hipStream_t st) {
    auto kern = gemm_w4_kernel<T, MODE, REPKV, true, EPI, LabNone, PATCH>;
    static bool attr_done = false;
    const hipError_t e = w4_set_lds_once(kern, W4Geom::LDS_BYTES, attr_done);
    if (e != hipSuccess) return (int)e;
    const long long tiles = (long long)((p.N + 255) / 256) * ((p.M + 255) / 256) * batch;
    const int ncu = w4_cu_count(), grid = (int)(tiles < ncu ? tiles : ncu);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), W4Geom::LDS_BYTES, st, p, batch);
    return (int)hipGetLastError();
}

// one row of VIDI_W4_*_KERNELS -> its launch, for a launcher templated on the dtype T
#define VIDI_W4_LAUNCH_CASE(name, MODE, REPKV, ...) case name: return launch_w4<T, MODE, REPKV, Epi<__VA_ARGS__>>(p, batch, st);

template <typename T>
static int w4_plain_launch(GemmKernel k, const GemmParams& p, int batch, hipStream_t st) {      // instantiated by gemm_w4_bf16.hip / gemm_w4_f16.hip
    switch (k) { VIDI_W4_PLAIN_KERNELS(VIDI_W4_LAUNCH_CASE) default: return VIDI_ERR_ARG; }
}

int vidi_w4_plain_bf16(GemmKernel k, const GemmParams& p, int batch, hipStream_t st);             // VIDI_W4_PLAIN_KERNELS
int vidi_w4_plain_f16(GemmKernel k, const GemmParams& p, int batch, hipStream_t st);
int vidi_w4_lnf(GemmKernel k, const GemmParams& p, int batch, int dtype, hipStream_t st);         // VIDI_W4_LNF_KERNELS
int vidi_w4_modes(GemmKernel k, const GemmParams& p, int batch, int dtype, hipStream_t st);       // VIDI_W4_MODES_KERNELS
int vidi_w4n(GemmKernel k, const GemmParams& p, int dtype, hipStream_t st);                       // VIDI_W4N_KERNELS (gemm_w4n.hip)
