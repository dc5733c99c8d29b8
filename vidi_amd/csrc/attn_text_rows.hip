// The decode step's T2T for rows AT DIFFERENT LENGTHS: in-flight batching of many queries on one video.  Same call site as
// attn_text_decode_kernel (attn_text.hip; gemma.py:165-175 -> TP gemma2:146-168, 248-288 at q_len = 1), the same body
// (attn_text_decode.h: rope of q and k, K/V append, attention over the row's own cache), but the batch has no common position: packed
// row m of the step lives in cache row slots[m] and writes its token to position pos[m] of that row (= the number of tokens the slot
// already holds).  A slot that finished is handed to another prompt without the other rows moving.
//
// Grid (nkv, M): block (kvh, m) reads its two table words with wave-uniform loads and runs the body on (m, slots[m], pos[m]).  The
// tables are caller-owned int32 device memory, written by the host side only and never by the kernel.  A record that does not fit what
// the caller declared (slot outside [0, B), position outside [0, pos_max] or beyond the cache) is skipped before any access — the rule
// attn_cross_seg.hip applies to its records; slot < 0 is the documented "idle row" value: that row's output stays untouched.
// Slots are dense (keys 0 .. pos of a slot are all valid): there is no key mask, and the sliding window counts from pos.
// Two packed rows of one launch must not name the same slot (they would append to the same cache position).
#include "kernels.h"
#include "attn_text_decode.h"

template <typename T, int HD>
__global__ __launch_bounds__(256) void attn_text_decode_rows_kernel(AttnTextDecodeParams p, const int* __restrict__ slots,
                                                                    const int* __restrict__ pos, int pos_max) {
    const int m = blockIdx.y;
    const int slot = __builtin_amdgcn_readfirstlane(slots[m]), ps = __builtin_amdgcn_readfirstlane(pos[m]);
    // the record against the declared buffers (block-uniform: the whole block leaves); pos_max sized the LDS score area
    if (slot < 0 || slot >= p.B || ps < 0 || ps > pos_max || ps >= p.Lmax) return;
    attn_text_decode_body<T, HD>(p, blockIdx.x, m, slot, ps);
}

int vidi_attn_text_decode_rows_dispatch(const void* qkv, int ldqkv, void* Kc, void* Vc, const void* cs, const void* sn, void* O, int M,
                                        const int* slots, const int* pos, int pos_max, int B, int Lmax, int nq, int nkv, int HD, int window,
                                        float scale, float softcap, int dtype, hipStream_t st) {
    if (M <= 0 || M > 65535 || Lmax <= 0 || pos_max < 0) return VIDI_ERR_SHAPE;
    if (((uintptr_t)slots & 3) || ((uintptr_t)pos & 3)) return VIDI_ERR_ALIGN;
    if (pos_max > Lmax - 1) pos_max = Lmax - 1;                       // positions beyond the cache are skipped anyway
    AttnTextDecodeParams p;
    size_t lds;
    // the LDS plan of vidi_attn_text_decode at pos0 = pos_max: room for the scores of the longest row (B = cache rows, no key mask)
    const int rc = attn_text_decode_params(p, lds, qkv, ldqkv, Kc, Vc, nullptr, cs, sn, O, B, Lmax, nq, nkv, HD, pos_max, nullptr, window, scale,
                                           softcap);
    if (rc) return rc;
    const dim3 grid(nkv, M);
#define VIDI_ATR(TT, D) hipLaunchKernelGGL((attn_text_decode_rows_kernel<TT, D>), grid, dim3(256), lds, st, p, slots, pos, pos_max)
    if (dtype == VIDI_DT_BF16) {
        if (HD == 256) VIDI_ATR(BF16, 256); else if (HD == 128) VIDI_ATR(BF16, 128); else if (HD == 64) VIDI_ATR(BF16, 64); else return VIDI_ERR_SHAPE;
    } else if (dtype == VIDI_DT_F16) {
        if (HD == 256) VIDI_ATR(F16, 256); else if (HD == 128) VIDI_ATR(F16, 128); else if (HD == 64) VIDI_ATR(F16, 64); else return VIDI_ERR_SHAPE;
    } else return VIDI_ERR_DTYPE;
#undef VIDI_ATR
    return (int)hipGetLastError();
}
