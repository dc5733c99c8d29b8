// Per-token log-probabilities over the vocabulary: gemma.py:565-590 (final softcap, `logits.float()`, cross-entropy) for ONE chosen token per
// row, without ever holding an fp32 [rows, V] block.  x_i = softcap_value<T>(logits[r, i], cap) (cap > 0) or the raw value, upcast to fp32.
//   idx[r]     first index of max x (vidi_softcap_argmax's tie rule)
//   lse[r]     log sum_i exp(x_i), with a running maximum
//   logprob[r] x_t - lse[r], t = targets[r] (-1 or no table: t = idx[r]);  rank[r] = #{i : x_i > x_t, or x_i == x_t and i < t}
// The logits are read once and never written.  Two launches, and the kernel boundary is the only hand-off between blocks:
//   pass 1  grid (parts, rows), parts <= 128 from V alone: block j of a row reduces its slice to (max, sum of exp relative to that max, first
//           arg-max index, number of entries ranked in front of the target) and stores that 16-byte record in the caller's workspace;
//   pass 2  one wave per row folds the row's records (a lane takes j = lane, lane + 64 in that order, then a butterfly) and writes the outputs.
// No zeroed scratch, no atomics: a row's outputs are the same bits from run to run, and — parts, slices and fold order being functions of V
// only — whatever other rows share the launch.
#include "common.h"
#include "softcap.h"
#include "vocab_logprob_api.h"

struct LpPart { float m, s; int arg, gt; };            // running max, sum of exp(x - m), first index of m, entries in front of the target
static_assert(sizeof(LpPart) == TOKEN_LOGPROB_PART_BYTES, "workspace record size");

// fold one entry into (m, s, arg): one exp whichever way the maximum moves
__device__ __forceinline__ void lp_push(float& m, float& s, int& arg, float x, int i) {
    const bool up = x > m;
    if (up || (x == m && i < arg)) arg = i;
    const float nm = up ? x : m;
    if (nm > -INFINITY) {                                // (entries of -inf before any finite one: nothing to add, and -inf - -inf is no number)
        const float e = __expf((up ? m : x) - nm);
        s = up ? s * e + 1.f : s + e;
    }
    m = nm;
}

// fold two partial results; the smaller index wins a tie of the maxima
__device__ __forceinline__ void lp_merge(float& m, float& s, int& arg, int& gt, float om, float os, int oarg, int ogt) {
    if (om > m || (om == m && oarg < arg)) arg = oarg;
    const float nm = fmaxf(m, om);
    s = (m > -INFINITY ? s * expf(m - nm) : 0.f) + (om > -INFINITY ? os * expf(om - nm) : 0.f);
    m = nm;
    gt += ogt;
}

template <typename T>
__device__ __forceinline__ float lp_value(const u16* row, long long i, float cap) {
    const float x = T::to_f32(row[i]);
    return cap > 0.f ? softcap_value<T>(x, cap) : x;
}

template <typename T>
__global__ __launch_bounds__(256) void token_logprob_part_kernel(const u16* __restrict__ logits, const long long* __restrict__ targets, int V,
                                                                 long long ld, float cap, int vec, LpPart* __restrict__ ws) {
    __shared__ LpPart sp[4];
    const int r = blockIdx.y, tid = threadIdx.x;
    const u16* row = logits + (size_t)r * ld;
    const long long t = targets ? targets[r] : -1;
    const bool counted = t >= 0 && t < V;                // the greedy token (-1) has rank 0 by definition; anything else outside [0, V) is never read
    const float xt = counted ? lp_value<T>(row, t, cap) : 0.f;
    const int ti = counted ? (int)t : 0;
    float m = -INFINITY, s = 0.f;
    int arg = 0x7fffffff, gt = 0;
    if (vec) {                                           // V % 8 == 0 and 16-byte aligned rows
        for (int c = blockIdx.x * 256 + tid; c < V / 8; c += gridDim.x * 256) {
            float x[8];
            unpack8<T>(*(const u32x4*)(row + (size_t)c * 8), x);
            if (cap > 0.f) {
#pragma unroll
                for (int e = 0; e < 8; ++e) x[e] = softcap_value<T>(x[e], cap);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int i = c * 8 + e;
                lp_push(m, s, arg, x[e], i);
                gt += (counted && (x[e] > xt || (x[e] == xt && i < ti))) ? 1 : 0;
            }
        }
    } else {
        for (int i = blockIdx.x * 256 + tid; i < V; i += gridDim.x * 256) {
            const float x = lp_value<T>(row, i, cap);
            lp_push(m, s, arg, x, i);
            gt += (counted && (x > xt || (x == xt && i < ti))) ? 1 : 0;
        }
    }
    for (int o = 32; o > 0; o >>= 1)
        lp_merge(m, s, arg, gt, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64), __shfl_xor(arg, o, 64), __shfl_xor(gt, o, 64));
    const int wave = tid >> 6, lane = tid & 63;
    if (lane == 0) sp[wave] = LpPart{m, s, arg, gt};
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) lp_merge(m, s, arg, gt, sp[w].m, sp[w].s, sp[w].arg, sp[w].gt);
        u32x4 rec;
        rec[0] = __float_as_uint(m); rec[1] = __float_as_uint(s); rec[2] = (unsigned)arg; rec[3] = (unsigned)gt;
        *(u32x4*)(ws + (size_t)r * TOKEN_LOGPROB_MAX_PARTS + blockIdx.x) = rec;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void token_logprob_final_kernel(const u16* __restrict__ logits, const long long* __restrict__ targets,
                                                                  const LpPart* __restrict__ ws, int parts, int R, int V, long long ld, float cap,
                                                                  long long* __restrict__ idx, float* __restrict__ lse,
                                                                  float* __restrict__ logprob, int* __restrict__ rank) {
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);       // one wave per row
    const int lane = threadIdx.x & 63;
    if (r >= R) return;
    float m = -INFINITY, s = 0.f;
    int arg = 0x7fffffff, gt = 0;
    for (int j = lane; j < parts; j += 64) {
        const u32x4 rec = *(const u32x4*)(ws + (size_t)r * TOKEN_LOGPROB_MAX_PARTS + j);
        lp_merge(m, s, arg, gt, __uint_as_float(rec[0]), __uint_as_float(rec[1]), (int)rec[2], (int)rec[3]);
    }
    for (int o = 32; o > 0; o >>= 1)
        lp_merge(m, s, arg, gt, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64), __shfl_xor(arg, o, 64), __shfl_xor(gt, o, 64));
    if (lane) return;
    const float l = m + logf(s);
    const long long t = targets ? targets[r] : -1;
    idx[r] = arg;                                        // 0x7fffffff: a row of NaNs only, as vidi_softcap_argmax reports it
    lse[r] = l;
    if (t == -1) {
        logprob[r] = m - l;
        rank[r] = 0;
    } else if (t >= 0 && t < V) {
        logprob[r] = lp_value<T>(logits + (size_t)r * ld, t, cap) - l;
        rank[r] = gt;
    } else {                                             // skipped before any access
        logprob[r] = -INFINITY;
        rank[r] = -1;
    }
}

template <typename T>
static int token_logprob_T(const void* logits, const long long* targets, long long* idx, float* lse, float* logprob, int* rank, int R, int V,
                           long long ld, float cap, void* workspace, hipStream_t st) {
    const int vec = (V % 8 == 0) && (ld % 8 == 0) && (((uintptr_t)logits & 15) == 0);
    const int items = vec ? V / 8 : V;
    const int parts = max(1, min(TOKEN_LOGPROB_MAX_PARTS, (items + 255) / 256));      // from V (and the load path) alone: never from R
    const u16* lg = (const u16*)logits;
    LpPart* ws = (LpPart*)workspace;
    for (int r0 = 0; r0 < R; r0 += 32768)                 // gridDim.y limit
        hipLaunchKernelGGL(token_logprob_part_kernel<T>, dim3(parts, min(32768, R - r0)), dim3(256), 0, st, lg + (size_t)r0 * ld,
                           targets ? targets + r0 : nullptr, V, ld, cap, vec, ws + (size_t)r0 * TOKEN_LOGPROB_MAX_PARTS);
    hipLaunchKernelGGL(token_logprob_final_kernel<T>, dim3((R + 3) / 4), dim3(256), 0, st, lg, targets, (const LpPart*)ws, parts, R, V, ld, cap,
                       idx, lse, logprob, rank);
    return (int)hipGetLastError();
}

int vidi_token_logprob_dispatch(const void* logits, const long long* targets, long long* idx, float* lse, float* logprob, int* rank, int R, int V,
                                long long ld, float cap, int dtype, void* workspace, hipStream_t st) {
    if (dtype == VIDI_DT_BF16) return token_logprob_T<BF16>(logits, targets, idx, lse, logprob, rank, R, V, ld, cap, workspace, st);
    if (dtype == VIDI_DT_F16) return token_logprob_T<F16>(logits, targets, idx, lse, logprob, rank, R, V, ld, cap, workspace, st);
    return VIDI_ERR_DTYPE;
}
