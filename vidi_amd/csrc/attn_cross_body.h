// Device bodies shared by the cross-attention launches (attn_cross.hip: one video; attn_cross_seg.hip: a batch of videos, one segment
// table): the per-tile split-KV partial pass and the merge of one (row, kv head).  See attn_cross.hip for the design notes.
#pragma once
#include "kernels.h"

#ifndef VIDI_XATTN_INTERLEAVE
#define VIDI_XATTN_INTERLEAVE 1
#endif
#ifndef VIDI_XATTN_NT
#define VIDI_XATTN_NT 1
#endif


// z / zsplit: this block's key slice and the number of slices of ITS modality (the dual launch runs the slices of two
// modalities in one grid).  kvh / rt: the block's kv head and 32-row tile; one_tile: a single row tile sweeps these keys (the
// non-temporal load policy below); tok0: first query token of the rows (row r is token tok0 + r / G of Q) — blockIdx.x,
// blockIdx.y, gridDim.y == 1 and 0 in the one-video launches, table values in the segmented one.
template <typename T, int HD>
__device__ __forceinline__ void attn_cross_body(const AttnCrossParams& p, const int z, const int zsplit, const int kvh, const int rt,
                                                const bool one_tile, const int tok0) {
    constexpr int QROW = HD * 2;                 // bytes per row
    constexpr int CPR = HD / 8;                  // 16-byte chunks per K/Q row (32 for HD=256)
    constexpr int KST = HD / 16;                 // k16 steps of QK^T
    constexpr int DT = HD / 32;                  // output d tiles
    constexpr int KBYTES = 32 * QROW;            // K sub-tile (32 keys)
    constexpr int VBYTES = HD * 64;              // Vt sub-tile (HD rows x 32 positions x 2 B)
    constexpr int KLD = KBYTES / 1024;           // DMA instructions per K sub-tile
    constexpr int VLD = VBYTES / 1024;
    static_assert(CPR >= 16 && (CPR & (CPR - 1)) == 0, "HD must be 128 or 256");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sQ = smem;                             // [32 rows][QROW], chunk-swizzled
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    char* sK = smem + 32 * QROW + wave * (KBYTES + VBYTES);
    char* sV = sK + KBYTES;

    const int r0 = rt * 32;

    // ---- stage the 32-row Q tile (rows beyond R are zero) -------------------------------------
    for (int i = tid; i < 32 * CPR; i += 256) {
        const int row = i / CPR, c = i % CPR, r = r0 + row;
        u32x4 v = {0, 0, 0, 0};
        if (r < p.R) {
            const int tq = tok0 + r / p.G, g = r % p.G;
            v = *(const u32x4*)(p.Q + (size_t)tq * p.ldq + (kvh * p.G + g) * HD + c * 8);
        }
        *(u32x4*)(sQ + row * QROW + ((c ^ (row & 15)) << 4)) = v;
    }
    __syncthreads();

    // Q fragments stay in registers for the whole key sweep (B operand: column = row l31)
    u32x4 qf[KST];
#pragma unroll
    for (int ks = 0; ks < KST; ++ks)
        qf[ks] = *(const u32x4*)(sQ + l31 * QROW + (((2 * ks + hi) ^ (l31 & 15)) << 4));

    // ---- this wave's key range (32-key sub-tiles) ----------------------------------------------
    const int nsub = (p.n_keys + 31) / 32;
    const int wtot = zsplit * 4;
    const int wg = z * 4 + wave;
    // key slices INTERLEAVED over the waves (wave wg sweeps sub-tiles wg, wg + wtot, ...): at any moment the waves of a kv head read
    // one contiguous window of its K and of its V cache (wtot x 16 KB each) that slides through memory, instead of wtot separate
    // streams half a megabyte apart (VIDI_XATTN_INTERLEAVE=0: a contiguous range per wave, the round-1 form)
#if VIDI_XATTN_INTERLEAVE
    const int st_begin = min(wg, nsub), st_end = nsub, st_step = wtot;
#else
    const int per = (nsub + wtot - 1) / wtot;
    const int st_begin = min(wg * per, nsub), st_end = min(st_begin + per, nsub), st_step = 1;
#endif

    const u16* kc_head = p.Kc + (size_t)kvh * p.ntile64 * 64 * HD;
    const u16* vt_head = p.Vtc + (size_t)kvh * p.ntile64 * HD * 64;

    // streamed once: when a single row tile sweeps the keys (decode, short prompts) every K/V byte is read by exactly one CU, and the
    // non-temporal policy on the DMA shortens issued -> landed (MI355X_MICROARCH.md "nt-weights"); with several row tiles the later
    // tiles re-read the slice from L2 and the default policy is kept
    const bool nt = VIDI_XATTN_NT && one_tile;
    auto issue_k = [&](int st) {
        const int kb = p.key_start + st * 32;
        const u16* src = kc_head + (size_t)kb * HD;                 // 32 consecutive keys are contiguous
        if (nt) {
#pragma unroll
            for (int j = 0; j < KLD; ++j) {
                const int pidx = j * 64 + lane, row = pidx / CPR, cl = pidx % CPR;
                glds16<2>(src + row * HD + (cl ^ (row & 15)) * 8, sK + j * 1024);
            }
        } else {
#pragma unroll
            for (int j = 0; j < KLD; ++j) {
                const int pidx = j * 64 + lane, row = pidx / CPR, cl = pidx % CPR;
                glds16(src + row * HD + (cl ^ (row & 15)) * 8, sK + j * 1024);
            }
        }
    };
    auto issue_v = [&](int st) {
        const int kb = p.key_start + st * 32;
        const u16* src = vt_head + (size_t)(kb >> 5) * HD * 32;          // [HD][32 positions]: 16 KB of linear 64-byte rows
        if (nt) {
#pragma unroll
            for (int j = 0; j < VLD; ++j) {
                const int pidx = j * 64 + lane, d = pidx >> 2, cl = pidx & 3;
                glds16<2>(src + d * 32 + (cl ^ ((d >> 2) & 3)) * 8, sV + j * 1024);
            }
        } else {
#pragma unroll
            for (int j = 0; j < VLD; ++j) {
                const int pidx = j * 64 + lane, d = pidx >> 2, cl = pidx & 3;
                glds16(src + d * 32 + (cl ^ ((d >> 2) & 3)) * 8, sV + j * 1024);
            }
        }
    };

    f32x16 o[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[t][i] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const float L2E = 1.4426950408889634f;
    const bool use_cap = p.softcap > 0.f;
    const float pre = use_cap ? p.scale / p.softcap : p.scale * L2E;   // x/cap, or base-2 logits
    const float capl2 = p.softcap * L2E;

    if (st_begin < st_end) {
        issue_k(st_begin);
        issue_v(st_begin);
    }
    for (int st = st_begin; st < st_end; st += st_step) {
        const bool has_next = (st + st_step < st_end);
        // K(st) landed?  (V(st) may still be in flight)
        wait_vmcnt<VLD>();
        // ---- S^T = K Q^T : Q fragments are register-resident; K fragments stream from LDS in
        //      batches of 4 k16-steps, the next batch's reads issued ahead of this batch's MFMAs ----
        f32x16 s;
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = 0.f;
#ifdef VIDI_XATTN_DIAG_NOCOMPUTE                          // lab builds only (wrong results): the DMA / wait skeleton without MFMAs and softmax
        if (p.R < 0)
#endif
        {
            u32x4 kf[2][4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                kf[0][e] = *(const u32x4*)(sK + l31 * QROW + ((((2 * e + hi)) ^ (l31 & 15)) << 4));
#pragma unroll
            for (int kb4 = 0; kb4 < KST / 4; ++kb4) {
                if (kb4 + 1 < KST / 4) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        kf[(kb4 + 1) & 1][e] = *(const u32x4*)(sK + l31 * QROW + (((2 * ((kb4 + 1) * 4 + e) + hi) ^ (l31 & 15)) << 4));
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int e = 0; e < 4; ++e) s = T::mfma32(kf[kb4 & 1][e], qf[kb4 * 4 + e], s);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // all K-fragment reads are consumed by the MFMAs above -> the K ring slot is free
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (has_next) issue_k(st + st_step);

        // ---- logits: scale, softcap, mask; online softmax in base 2 --------------------------
        const int kb_local = st * 32;
        u32x4 pf0 = {0, 0, 0, 0}, pf1 = {0, 0, 0, 0};
#ifdef VIDI_XATTN_DIAG_NOCOMPUTE
        if (p.R < 0)
#endif
        {
        float mx = -INFINITY;
        if (use_cap) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                // cap*tanh(y) in base-2 units: tanh(y) = 1 - 2/(exp(2y)+1)
                const float e2 = __expf(2.0f * s[r] * pre);
                s[r] = capl2 * (1.0f - 2.0f / (e2 + 1.0f));
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] *= pre;
        }
        if (kb_local + 32 > p.n_keys) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (kb_local + krow32(r, hi) >= p.n_keys) s[r] = -INFINITY;
        }
        if (p.mask) {
            // 32 mask bytes of this sub-tile (the cache region is padded to 64 keys => in bounds)
            const unsigned char* mp = p.mask + kb_local + 4 * hi;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned mv = *(const unsigned*)(mp + 8 * j);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (((mv >> (8 * e)) & 0xffu) == 0) s[4 * j + e] = -INFINITY;
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
        const float alpha = (m_run == -INFINITY) ? 0.f : fast_exp2(m_run - m_use);
        m_run = m_new;
        float pv[16], psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            pv[r] = fast_exp2(s[r] - m_use);
            psum += pv[r];
        }
        l_run = l_run * alpha + psum;
        pf0 = pack8<T>(pv);
        pf1 = pack8<T>(pv + 8);
        if (!__all(alpha == 1.0f)) {
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                for (int i = 0; i < 16; ++i) o[dt][i] *= alpha;
        }
        }
        // V(st) landed?  (K(st+1) may be in flight)
        if (has_next) wait_vmcnt<KLD>(); else wait_vmcnt<0>();
        // ---- O^T += Vt P^T : 2 d-tiles (4 fragments) per batch, reads one batch ahead ----------
#ifdef VIDI_XATTN_DIAG_NOCOMPUTE
        if (p.R < 0)
#endif
        {
            u32x4 vf[2][4];
            auto read_v = [&](int buf, int dt0) {
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int d = (dt0 + e) * 32 + l31;
                    const int swz = (d >> 2) & 3;
                    vf[buf][2 * e] = *(const u32x4*)(sV + d * 64 + (((0 + hi) ^ swz) << 4));
                    vf[buf][2 * e + 1] = *(const u32x4*)(sV + d * 64 + (((2 + hi) ^ swz) << 4));
                }
            };
            read_v(0, 0);
#pragma unroll
            for (int b2 = 0; b2 < DT / 2; ++b2) {
                if (b2 + 1 < DT / 2) read_v((b2 + 1) & 1, (b2 + 1) * 2);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    o[b2 * 2 + e] = T::mfma32(vf[b2 & 1][2 * e], pf0, o[b2 * 2 + e]);
                    o[b2 * 2 + e] = T::mfma32(vf[b2 & 1][2 * e + 1], pf1, o[b2 * 2 + e]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (has_next) issue_v(st + st_step);
    }

    // ---- merge the block's 4 waves in LDS (their private K/V rings are free now) and emit ONE partial ---------
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    float* so = (float*)sK;                                   // [32 rows][HD] fp32 = exactly this wave's ring bytes
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x4 ov = {o[dt][4 * j], o[dt][4 * j + 1], o[dt][4 * j + 2], o[dt][4 * j + 3]};
            *(f32x4*)(so + l31 * HD + dt * 32 + 8 * j + 4 * hi) = ov;
        }
    float* sml = (float*)sQ;                                  // Q tile is dead (fragments live in registers)
    if (hi == 0) {
        sml[(wave * 32 + l31) * 2] = m_run;                   // base-2 logit units
        sml[(wave * 32 + l31) * 2 + 1] = l_tot;
    }
    __syncthreads();
    const float* so_all = (const float*)(smem + 32 * QROW);
    constexpr int WSTRIDE = (KBYTES + VBYTES) / 4;            // floats between two waves' tiles
    for (int idx = tid; idx < 32 * (HD / 4); idx += 256) {
        const int row = idx / (HD / 4), c4 = idx % (HD / 4);
        const int r = r0 + row;
        if (r >= p.R) continue;
        float mw[4], m = -INFINITY;
#pragma unroll
        for (int w = 0; w < 4; ++w) { mw[w] = sml[(w * 32 + row) * 2]; m = fmaxf(m, mw[w]); }
        f32x4 accv = {0.f, 0.f, 0.f, 0.f};
        float l = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (mw[w] == -INFINITY) continue;
            const float scw = fast_exp2(mw[w] - m);
            const f32x4 v = *(const f32x4*)(so_all + w * WSTRIDE + row * HD + c4 * 4);
            accv += v * scw;
            l += scw * sml[(w * 32 + row) * 2 + 1];
        }
        const size_t base = ((size_t)z * p.nkv + kvh) * p.Rpad + r;
        *(f32x4*)(p.Opart + base * HD + c4 * 4) = accv;
        if (c4 == 0) {
            p.ML[base * 2] = m;
            p.ML[base * 2 + 1] = l;
        }
    }
}

// Combine W partials per (row, kv head): O = sum_w 2^(m_w-m) O_w / sum_w 2^(m_w-m) l_w.
// Optionally emits the merged result in PARTIAL form (numerator, m, l) for a further cross-GPU merge.

// One (row r, kv head) merged by threads d = 0 .. HD-1 of the block; threads with d >= HD (a 256-thread caller at HD = 128) only take
// part in the barriers.
template <typename T, int HD>
__device__ __forceinline__ void attn_merge_row(const AttnMergeParams& p, const int r, const int kvh, const int d, float* s_m, float* s_l) {
    // the W (m, l) pairs of this (row, kv head) are fetched by W threads at once and shared through LDS; the weights
    // 2^(m_w - m) are then uniform values and the numerator loads of all partials are independent of each other
    const bool act = d < HD;
    float m = -INFINITY;
    for (int w0 = 0; w0 < p.W; w0 += 256) {
        __syncthreads();
        const int nw = min(256, p.W - w0);
        for (int w = d; act && w < nw; w += HD) {
            const size_t base = (size_t)(w0 + w) * p.wsML + ((size_t)kvh * p.Rpad + r) * 2;
            s_m[w] = p.ML[base];
            s_l[w] = p.ML[base + 1];
        }
        __syncthreads();
        for (int w = 0; w < nw; ++w) m = fmaxf(m, s_m[w]);
    }
    float num = 0.f, den = 0.f;
    if (m != -INFINITY) {
        for (int w0 = 0; w0 < p.W; w0 += 256) {
            const int nw = min(256, p.W - w0);
            if (p.W > 256) {                                            // re-stage this window (single window: still resident)
                __syncthreads();
                for (int w = d; act && w < nw; w += HD) {
                    const size_t base = (size_t)(w0 + w) * p.wsML + ((size_t)kvh * p.Rpad + r) * 2;
                    s_m[w] = p.ML[base];
                    s_l[w] = p.ML[base + 1];
                }
                __syncthreads();
            }
#pragma unroll 8
            for (int w = 0; w < nw; ++w) {
                const float mw = s_m[w];
                const float sc = (mw == -INFINITY) ? 0.f : fast_exp2(mw - m);
                den += sc * s_l[w];
                const float v = p.Opart[(size_t)(w0 + w) * p.wsO + ((size_t)kvh * p.Rpad + r) * HD + (act ? d : 0)];
                num += (mw == -INFINITY) ? 0.f : sc * v;                // a skipped partial may hold stale (even non-finite) data
            }
        }
    }
    if (!act) return;
    const int tq = r / p.G, g = r % p.G;
    const size_t oidx = (size_t)tq * p.ldo + (kvh * p.G + g) * HD + d;
    float out = (den > 0.f && !p.zero_out) ? num / den : 0.f;
    if (p.Out) p.Out[oidx] = T::from_f32(out);
    // partial form (same layout as one slice of Opart/ML): lets a second merge combine per-GPU results
    const size_t pbase = (size_t)kvh * p.rpo + r;
    if (p.OutF32) p.OutF32[pbase * HD + d] = num;
    if (p.OutML && d == 0) {
        p.OutML[pbase * 2] = m;
        p.OutML[pbase * 2 + 1] = den;
    }
}
