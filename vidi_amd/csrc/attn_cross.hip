// Text -> multimodal cross-attention (T2V / T2A of Decomposed Attention): skinny Q (Lq ~ 40 at
// prefill, 1 at decode) against ~10^5 cached video/audio keys.  Replaces the reference's
// flash_attn_func / flash_attn_varlen_func call sites (Vidi1.5_9B/vidi/model/lmm/dattn/xattn.py:123,253
// via gemma.py:81-91) — non-causal, logits softcap, key-padding mask, GQA.
//
// HBM-bound: every K/V byte is read once per (layer, modality): algorithmic bytes =
// n_keys * 2 * n_kv_heads * head_dim * 2 B.  Design:
//   * GQA-native: the G query heads sharing a KV head are stacked as rows (row = (token, g)), so
//     K/V are never repeat_kv'ed (the reference doubles the bytes, gemma.py:77-78).
//   * K cache is tile-contiguous  Kc[kvh][tile64][64 keys][HD];  V cache is stored transposed in 32-key
//     sub-tiles  Vtc[kvh][tile32][HD][32 positions]  with the perm16 key order, both written
//     by the KV-projection GEMM epilogue.  A wave's 32-key sub-tile is 16 KB + 16 KB of perfectly
//     linear 16-byte global_load_lds DMA.
//   * split-KV at WAVE granularity: every wave owns a contiguous key range and its private 32 KB
//     LDS ring and runs its own online softmax (no block barriers in the loop); the 4 waves of a block are merged
//     in LDS and the block emits one partial (O, m, l); `attn_merge_kernel` combines the blocks' partials (exact:
//     the tanh softcap is per logit).
//   * swapped MFMAs (S^T = K Q^T, O^T = Vt P^T): per-lane softmax statistics, P stays in registers.
#include "kernels.h"
#include "attn_text_decode.h"
#include "attn_cross_body.h"
#include <stdlib.h>


template <typename T, int HD>
__global__ __launch_bounds__(256) void attn_cross_kernel(AttnCrossParams p) {
    attn_cross_body<T, HD>(p, blockIdx.z, gridDim.z, blockIdx.x, blockIdx.y, gridDim.y == 1, 0);
}

// T2V and T2A of one layer in ONE launch (decode: a launch of this kernel costs ~8 us on top of its bytes, measured from the two
// modalities' durations; the two key regions are disjoint slices of the same caches): the first `za` z-slices sweep set a's keys,
// the rest set b's.  Same per-slice arithmetic as two attn_cross_kernel launches with zsplit = za and gridDim.z - za.
template <typename T, int HD>
__global__ __launch_bounds__(256) void attn_cross2_kernel(AttnCrossParams a, AttnCrossParams b, int za) {
    const int bz = blockIdx.z;
    if (bz < za) attn_cross_body<T, HD>(a, bz, za, blockIdx.x, blockIdx.y, gridDim.y == 1, 0);
    else attn_cross_body<T, HD>(b, bz - za, (int)gridDim.z - za, blockIdx.x, blockIdx.y, gridDim.y == 1, 0);
}


template <typename T, int HD>
__device__ __forceinline__ void attn_merge_body(const AttnMergeParams& p) {
    __shared__ float s_m[256], s_l[256];
    attn_merge_row<T, HD>(p, blockIdx.x, blockIdx.y, threadIdx.x, s_m, s_l);
}

template <typename T, int HD>
__global__ __launch_bounds__(HD) void attn_merge_kernel(AttnMergeParams p) { attn_merge_body<T, HD>(p); }

// two independent merges (the T2V and the T2A partials of one layer) in one launch: blockIdx.z picks the set
template <typename T, int HD>
__global__ __launch_bounds__(HD) void attn_merge2_kernel(AttnMergeParams a, AttnMergeParams b) {
    const AttnMergeParams& p = blockIdx.z == 0 ? a : b;
    if (!p.Out && !p.OutF32) return;                        // absent set (a modality the sample does not have)
    attn_merge_body<T, HD>(p);
}

// The decode step's two small launches in ONE: the T2T of the new token (attn_text_decode_body, nkv * B blocks) and the merge of the
// T2V / T2A partials (attn_merge_row, 2 * nkv * R blocks).  Neither fills the chip, neither depends on the other (the cross-attention
// launch that produced the partials comes first; the o_proj that follows needs both): one launch of ≈9 us instead of 8.8 + 6.7 us and a gap.
template <typename T, int HD>
__global__ __launch_bounds__(256) void attn_text_decode_merge2_kernel(AttnTextDecodeParams tp, AttnMergeParams a, AttnMergeParams b, int nt) {
    if ((int)blockIdx.x < nt) {
        const int row = blockIdx.x / tp.nkv;
        attn_text_decode_body<T, HD>(tp, blockIdx.x % tp.nkv, row, row, tp.pos_dev ? *tp.pos_dev : tp.pos0);
        return;
    }
    // the merge role's (m, l) staging lives at the head of the launch's DYNAMIC allocation (sized for the T2T role, never below 2 KB):
    // a static array on top of it would push a T2T plan of exactly 64 KB over the limit
    extern __shared__ float s_mrg[];
    float* s_m = s_mrg;
    float* s_l = s_mrg + 256;
    const int mb = blockIdx.x - nt;
    const int r = mb % a.R, kvh = (mb / a.R) % a.nkv, set = mb / (a.R * a.nkv);
    const AttnMergeParams& p = set == 0 ? a : b;
    attn_merge_row<T, HD>(p, r, kvh, threadIdx.x, s_m, s_l);
}

int vidi_attn_text_decode_merge2_dispatch(const AttnTextDecodeParams& tp, size_t lds, const AttnMergeParams& a, const AttnMergeParams& b, int HD,
                                          int dtype, hipStream_t st) {
    if (a.R <= 0 || a.W <= 0 || b.W <= 0 || a.R != b.R || a.nkv != b.nkv || a.nkv != tp.nkv || !a.Out || !b.Out) return VIDI_ERR_SHAPE;
    if (HD != 256 && HD != 128) return VIDI_ERR_SHAPE;
    const int nt = tp.nkv * tp.B;
    const dim3 grid(nt + 2 * a.nkv * a.R);
    if (lds < 2 * 256 * sizeof(float)) lds = 2 * 256 * sizeof(float);       // the merge role's staging
    if (dtype == VIDI_DT_BF16) {
        if (HD == 256) hipLaunchKernelGGL((attn_text_decode_merge2_kernel<BF16, 256>), grid, dim3(256), lds, st, tp, a, b, nt);
        else hipLaunchKernelGGL((attn_text_decode_merge2_kernel<BF16, 128>), grid, dim3(256), lds, st, tp, a, b, nt);
    } else if (dtype == VIDI_DT_F16) {
        if (HD == 256) hipLaunchKernelGGL((attn_text_decode_merge2_kernel<F16, 256>), grid, dim3(256), lds, st, tp, a, b, nt);
        else hipLaunchKernelGGL((attn_text_decode_merge2_kernel<F16, 128>), grid, dim3(256), lds, st, tp, a, b, nt);
    } else return VIDI_ERR_DTYPE;
    return (int)hipGetLastError();
}

int vidi_attn_merge2_dispatch(const AttnMergeParams& a, const AttnMergeParams& b, int HD, int dtype, hipStream_t st) {
    // W == 0: a rank that holds no key of the modality emits the neutral partial (m = -inf, l = 0, numerator 0)
    if (a.R <= 0 || a.W < 0 || b.W < 0 || a.R != b.R || a.nkv != b.nkv) return VIDI_ERR_SHAPE;
    const dim3 grid(a.R, a.nkv, 2);
    if (dtype == VIDI_DT_BF16) {
        if (HD == 256) hipLaunchKernelGGL((attn_merge2_kernel<BF16, 256>), grid, dim3(256), 0, st, a, b);
        else if (HD == 128) hipLaunchKernelGGL((attn_merge2_kernel<BF16, 128>), grid, dim3(128), 0, st, a, b);
        else return VIDI_ERR_SHAPE;
    } else if (dtype == VIDI_DT_F16) {
        if (HD == 256) hipLaunchKernelGGL((attn_merge2_kernel<F16, 256>), grid, dim3(256), 0, st, a, b);
        else if (HD == 128) hipLaunchKernelGGL((attn_merge2_kernel<F16, 128>), grid, dim3(128), 0, st, a, b);
        else return VIDI_ERR_SHAPE;
    } else {
        return VIDI_ERR_DTYPE;
    }
    return (int)hipGetLastError();
}

// Row tiles (32 rows) a block of the cross-attention launch covers: 4 — the shared-stream kernel above — from two row tiles on
// (VIDI_XATTN_ROWS=0: never, the A/B arm), else 1.  Callers size the key split with it (blocks = nkv x ceil(row tiles / this) x slices).
int vidi_attn_cross_rtpb(int Rpad, float softcap, int dtype) {
    static const int on = [] { const char* e = getenv("VIDI_XATTN_ROWS"); return (e && atoi(e) == 0) ? 0 : 1; }();
    // every dtype / softcap has a form of the shared-stream kernel (attn_cross_rows.hip: the fixed-reference softmax for bf16 with a cap whose
    // VALUE admits it — softcap x log2(e) <= VIDI_XROWS_MAX_CAP2, not merely softcap > 0 —, a running reference otherwise)
    (void)softcap;
    return (on && Rpad > 32 && (dtype == VIDI_DT_BF16 || dtype == VIDI_DT_F16)) ? 4 : 1;
}

int vidi_attn_cross_rows_launch(const AttnCrossParams& a, const AttnCrossParams& b, int za, int zb, int HD, int dtype, hipStream_t st);      // attn_cross_rows.hip

int vidi_attn_cross_dispatch(const AttnCrossParams& p, int HD, int zsplit, int dtype, hipStream_t st) {
    if (p.R <= 0 || p.n_keys <= 0 || p.G <= 0 || p.nkv <= 0 || zsplit <= 0) return VIDI_ERR_SHAPE;
    if (p.key_start % 64 != 0 || p.Rpad % 32 != 0 || p.Rpad < p.R) return VIDI_ERR_SHAPE;
    if ((p.ldq % 8) || ((uintptr_t)p.Q & 15) || ((uintptr_t)p.Kc & 15) || ((uintptr_t)p.Vtc & 15)) return VIDI_ERR_ALIGN;
    if (HD != 256 && HD != 128) return VIDI_ERR_SHAPE;
    if (vidi_attn_cross_rtpb(p.Rpad, p.softcap, dtype) == 4) return vidi_attn_cross_rows_launch(p, p, zsplit, 0, HD, dtype, st);
    const dim3 grid(p.nkv, p.Rpad / 32, zsplit);
    const int lds = 32 * HD * 2 + 4 * (32 * HD * 2 + HD * 64);
#define LAUNCH(TT, HH)                                                                        \
    do {                                                                                      \
        auto kern = attn_cross_kernel<TT, HH>;                                                \
        static bool done = false;                                                             \
        if (!done) {                                                                          \
            hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds); \
            if (e != hipSuccess) return (int)e;                                               \
            done = true;                                                                      \
        }                                                                                     \
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, p);                                \
    } while (0)
    if (dtype == VIDI_DT_BF16) { if (HD == 256) LAUNCH(BF16, 256); else LAUNCH(BF16, 128); }
    else if (dtype == VIDI_DT_F16) { if (HD == 256) LAUNCH(F16, 256); else LAUNCH(F16, 128); }
    else return VIDI_ERR_DTYPE;
#undef LAUNCH
    return (int)hipGetLastError();
}

int vidi_attn_cross2_dispatch(const AttnCrossParams& a, const AttnCrossParams& b, int HD, int za, int zb, int dtype, hipStream_t st) {
    if (a.R <= 0 || a.n_keys <= 0 || b.n_keys <= 0 || a.G <= 0 || a.nkv <= 0 || za <= 0 || zb <= 0) return VIDI_ERR_SHAPE;
    if (a.key_start % 64 != 0 || b.key_start % 64 != 0 || a.Rpad % 32 != 0 || a.Rpad < a.R) return VIDI_ERR_SHAPE;
    if ((a.ldq % 8) || ((uintptr_t)a.Q & 15) || ((uintptr_t)a.Kc & 15) || ((uintptr_t)a.Vtc & 15)) return VIDI_ERR_ALIGN;
    if (HD != 256 && HD != 128) return VIDI_ERR_SHAPE;
    if (vidi_attn_cross_rtpb(a.Rpad, a.softcap, dtype) == 4) return vidi_attn_cross_rows_launch(a, b, za, zb, HD, dtype, st);
    const dim3 grid(a.nkv, a.Rpad / 32, za + zb);
    const int lds = 32 * HD * 2 + 4 * (32 * HD * 2 + HD * 64);
#define LAUNCH(TT, HH)                                                                        \
    do {                                                                                      \
        auto kern = attn_cross2_kernel<TT, HH>;                                               \
        static bool done = false;                                                             \
        if (!done) {                                                                          \
            hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds); \
            if (e != hipSuccess) return (int)e;                                               \
            done = true;                                                                      \
        }                                                                                     \
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, a, b, za);                         \
    } while (0)
    if (dtype == VIDI_DT_BF16) { if (HD == 256) LAUNCH(BF16, 256); else LAUNCH(BF16, 128); }
    else if (dtype == VIDI_DT_F16) { if (HD == 256) LAUNCH(F16, 256); else LAUNCH(F16, 128); }
    else return VIDI_ERR_DTYPE;
#undef LAUNCH
    return (int)hipGetLastError();
}

int vidi_attn_merge_dispatch(const AttnMergeParams& p, int HD, int dtype, hipStream_t st) {
    if (p.R <= 0 || p.W <= 0) return VIDI_ERR_SHAPE;
    const dim3 grid(p.R, p.nkv);
    if (dtype == VIDI_DT_BF16) {
        if (HD == 256) hipLaunchKernelGGL((attn_merge_kernel<BF16, 256>), grid, dim3(256), 0, st, p);
        else if (HD == 128) hipLaunchKernelGGL((attn_merge_kernel<BF16, 128>), grid, dim3(128), 0, st, p);
        else return VIDI_ERR_SHAPE;
    } else if (dtype == VIDI_DT_F16) {
        if (HD == 256) hipLaunchKernelGGL((attn_merge_kernel<F16, 256>), grid, dim3(256), 0, st, p);
        else if (HD == 128) hipLaunchKernelGGL((attn_merge_kernel<F16, 128>), grid, dim3(128), 0, st, p);
        else return VIDI_ERR_SHAPE;
    } else {
        return VIDI_ERR_DTYPE;
    }
    return (int)hipGetLastError();
}
