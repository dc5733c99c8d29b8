// Segmented text -> multimodal cross-attention: a BATCH OF DIFFERENT VIDEOS decoded together.  Replaces the reference's
// flash_attn_varlen_func call site for a batch with one video per row (Vidi1.5_9B/vidi/model/lmm/dattn/xattn.py:36-103, 123 via
// gemma.py:81-91; the batch comes from multimodal.py:156-252).
//
// A segment is one video: a contiguous range of query tokens [tok0, tok0 + ntok) of the packed text rows and, per modality, a key region
// [key_start, key_start + n_keys) of ONE shared cache pair (the tiled layouts of attn_cross.hip).  The launch is flat: every block
// reads one fixed-size record of a caller-owned int32 table — (segment, modality, 32-row tile, key slice z of zsplit) — and runs the
// per-tile body of attn_cross.hip on it, so a segment's partials are the ones vidi_attn_cross writes for that video alone (same
// operands in the same order: bit-identical).  The table is written by the host side only; the kernels read it with wave-uniform
// loads and never write to it.  A record that does not fit the buffers the caller declared is skipped (the block returns before any
// access): a bad table cannot reach memory outside them.
#include "kernels.h"
#include "attn_cross_body.h"

// int32 words of one record of either table (vidi_hip.h: VIDI_XSEG_*)
#define XSEG_REC 16

struct AttnCrossSegParams {
    const u16* Q; const u16* Kc; const u16* Vtc; const unsigned char* mask;
    float* Opart; float* ML;
    const int* items;
    long long mask_len, part_rows;   // bytes of `mask`; rows ([HD] / [2] floats each) of Opart / ML
    int n_tokens;                    // rows of Q
    int G, nkv, ldq, ntile64;
    float scale, softcap;
};

struct AttnMergeSegParams {
    const float* Opart; const float* ML;
    const int* segs;
    u16* OutA; u16* OutB;            // image / audio outputs [n_tokens, ldo]; null: no video of the batch has the modality
    long long part_rows;
    int n_tokens, nkv, G, ldo;
};

template <typename T, int HD>
__global__ __launch_bounds__(256) void attn_cross_seg_kernel(AttnCrossSegParams s) {
    const int item = blockIdx.x / s.nkv, kvh = blockIdx.x % s.nkv;
    const int* rec = s.items + (size_t)item * XSEG_REC;
    const int tok0 = __builtin_amdgcn_readfirstlane(rec[0]), R = __builtin_amdgcn_readfirstlane(rec[1]);
    const int rt = __builtin_amdgcn_readfirstlane(rec[2]), key_start = __builtin_amdgcn_readfirstlane(rec[3]);
    const int n_keys = __builtin_amdgcn_readfirstlane(rec[4]), mask_off = __builtin_amdgcn_readfirstlane(rec[5]);
    const int z = __builtin_amdgcn_readfirstlane(rec[6]), zsplit = __builtin_amdgcn_readfirstlane(rec[7]);
    const int base = __builtin_amdgcn_readfirstlane(rec[8]), Rpad = __builtin_amdgcn_readfirstlane(rec[9]);
    const int one_tile = __builtin_amdgcn_readfirstlane(rec[10]);
    // the record against the declared buffers (block-uniform: the whole block leaves)
    if (R <= 0 || Rpad < R || (Rpad & 31) || rt < 0 || rt * 32 >= Rpad || tok0 < 0 || (long long)tok0 + (R + s.G - 1) / s.G > s.n_tokens) return;
    if (n_keys <= 0 || key_start < 0 || (key_start & 63) || ((long long)key_start + n_keys + 63) / 64 > s.ntile64) return;
    if (z < 0 || z >= zsplit || base < 0 || (long long)base + (long long)zsplit * s.nkv * Rpad > s.part_rows) return;
    if (mask_off >= 0 && (!s.mask || (long long)mask_off + (n_keys + 63) / 64 * 64 > s.mask_len)) return;
    AttnCrossParams p;
    p.Q = s.Q; p.Kc = s.Kc; p.Vtc = s.Vtc;
    p.mask = mask_off >= 0 ? s.mask + mask_off : nullptr;
    p.Opart = s.Opart + (size_t)base * HD; p.ML = s.ML + (size_t)base * 2;
    p.R = R; p.Rpad = Rpad; p.G = s.G; p.nkv = s.nkv; p.ldq = s.ldq; p.ntile64 = s.ntile64;
    p.key_start = key_start; p.n_keys = n_keys; p.scale = s.scale; p.softcap = s.softcap;
    attn_cross_body<T, HD>(p, z, zsplit, kvh, rt, one_tile != 0, tok0);
}

// grid (max rows of a segment, nkv, 2 * segments): block (r, kvh, 2 * seg + modality) merges the W partials of that segment's row r
template <typename T, int HD>
__global__ __launch_bounds__(HD) void attn_merge_seg_kernel(AttnMergeSegParams s) {
    __shared__ float s_m[256], s_l[256];
    const int seg = blockIdx.z >> 1, mod = blockIdx.z & 1;
    u16* out = mod ? s.OutB : s.OutA;
    if (!out) return;
    const int* rec = s.segs + (size_t)seg * XSEG_REC;
    const int tok0 = __builtin_amdgcn_readfirstlane(rec[0]), R = __builtin_amdgcn_readfirstlane(rec[1]);
    const int Rpad = __builtin_amdgcn_readfirstlane(rec[2]);
    const int base = __builtin_amdgcn_readfirstlane(rec[3 + 3 * mod]), W = __builtin_amdgcn_readfirstlane(rec[4 + 3 * mod]);
    const int zero = __builtin_amdgcn_readfirstlane(rec[5 + 3 * mod]);
    const int r = blockIdx.x;
    if (r >= R || Rpad < R || tok0 < 0 || (long long)tok0 + (R + s.G - 1) / s.G > s.n_tokens) return;
    if (W < 0 || base < 0 || (long long)base + (long long)W * s.nkv * Rpad > s.part_rows) return;
    AttnMergeParams p;
    p.Opart = s.Opart + (size_t)base * HD; p.ML = s.ML + (size_t)base * 2;
    p.Out = out + (size_t)tok0 * s.ldo; p.OutF32 = nullptr; p.OutML = nullptr;
    p.W = W; p.nkv = s.nkv; p.R = R; p.Rpad = Rpad; p.G = s.G; p.ldo = s.ldo; p.zero_out = zero;       // W == 0 (no key of the modality): zeros
    p.wsO = (long long)s.nkv * Rpad * HD; p.wsML = (long long)s.nkv * Rpad * 2; p.rpo = Rpad;
    attn_merge_row<T, HD>(p, r, blockIdx.y, threadIdx.x, s_m, s_l);
}

int vidi_attn_cross_seg_dispatch(const void* Q, const void* Kc, const void* Vtc, const void* mask, long long mask_len, float* Opart, float* ML,
                                 long long part_rows, const int* items, int n_items, int n_tokens, int G, int nkv, int HD, int ldq, int ntile64,
                                 float scale, float softcap, int dtype, hipStream_t st) {
    if (n_items <= 0 || n_tokens <= 0 || G <= 0 || nkv <= 0 || ntile64 <= 0 || part_rows <= 0 || mask_len < 0) return VIDI_ERR_SHAPE;
    if (HD != 256 && HD != 128) return VIDI_ERR_SHAPE;
    if ((long long)n_items * nkv > 0x7fffffffLL) return VIDI_ERR_SHAPE;
    if ((ldq % 8) || ((uintptr_t)Q & 15) || ((uintptr_t)Kc & 15) || ((uintptr_t)Vtc & 15) || ((uintptr_t)Opart & 15) || ((uintptr_t)items & 3))
        return VIDI_ERR_ALIGN;
    AttnCrossSegParams s;
    s.Q = (const u16*)Q; s.Kc = (const u16*)Kc; s.Vtc = (const u16*)Vtc; s.mask = (const unsigned char*)mask;
    s.Opart = Opart; s.ML = ML; s.items = items; s.mask_len = mask ? mask_len : 0; s.part_rows = part_rows; s.n_tokens = n_tokens;
    s.G = G; s.nkv = nkv; s.ldq = ldq; s.ntile64 = ntile64; s.scale = scale; s.softcap = softcap;
    const dim3 grid((unsigned)(n_items * nkv));
    const int lds = 32 * HD * 2 + 4 * (32 * HD * 2 + HD * 64);
#define LAUNCH(TT, HH)                                                                        \
    do {                                                                                      \
        auto kern = attn_cross_seg_kernel<TT, HH>;                                            \
        static bool done = false;                                                             \
        if (!done) {                                                                          \
            hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds); \
            if (e != hipSuccess) return (int)e;                                               \
            done = true;                                                                      \
        }                                                                                     \
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, s);                                \
    } while (0)
    if (dtype == VIDI_DT_BF16) { if (HD == 256) LAUNCH(BF16, 256); else LAUNCH(BF16, 128); }
    else if (dtype == VIDI_DT_F16) { if (HD == 256) LAUNCH(F16, 256); else LAUNCH(F16, 128); }
    else return VIDI_ERR_DTYPE;
#undef LAUNCH
    return (int)hipGetLastError();
}

int vidi_attn_merge_seg_dispatch(const float* Opart, const float* ML, long long part_rows, const int* segs, int n_segs, int max_rows,
                                 void* OutImg, void* OutAud, int n_tokens, int nkv, int G, int HD, int ldo, int dtype, hipStream_t st) {
    if (n_segs <= 0 || n_segs > 32767 || max_rows <= 0 || n_tokens <= 0 || nkv <= 0 || nkv > 65535 || G <= 0 || ldo <= 0 || part_rows <= 0)
        return VIDI_ERR_SHAPE;
    AttnMergeSegParams s;
    s.Opart = Opart; s.ML = ML; s.segs = segs; s.OutA = (u16*)OutImg; s.OutB = (u16*)OutAud; s.part_rows = part_rows;
    s.n_tokens = n_tokens; s.nkv = nkv; s.G = G; s.ldo = ldo;
    const dim3 grid(max_rows, nkv, 2 * n_segs);
    if (dtype == VIDI_DT_BF16) {
        if (HD == 256) hipLaunchKernelGGL((attn_merge_seg_kernel<BF16, 256>), grid, dim3(256), 0, st, s);
        else if (HD == 128) hipLaunchKernelGGL((attn_merge_seg_kernel<BF16, 128>), grid, dim3(128), 0, st, s);
        else return VIDI_ERR_SHAPE;
    } else if (dtype == VIDI_DT_F16) {
        if (HD == 256) hipLaunchKernelGGL((attn_merge_seg_kernel<F16, 256>), grid, dim3(256), 0, st, s);
        else if (HD == 128) hipLaunchKernelGGL((attn_merge_seg_kernel<F16, 128>), grid, dim3(128), 0, st, s);
        else return VIDI_ERR_SHAPE;
    } else {
        return VIDI_ERR_DTYPE;
    }
    return (int)hipGetLastError();
}
