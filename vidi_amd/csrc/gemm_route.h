// Which GEMM kernel runs: the ONE place that decides.  gemm_route() maps a call (shape, epilogue, tile_cfg, dtype, the three
// environment switches) to the exact kernel instantiation or to an error code — pure integer logic, no HIP call, no getenv, no
// pointer dereferenced — so tools/gemm_route_dump.hip prints it and tests/test_gemm_route.py pins it without a GPU.  The launchers
// (gemm.hip, gemm_w4_*.hip, gemm_w4n.hip) only switch from the enumerator to their own instantiations.
#pragma once
#include "kernels.h"
#include <stdlib.h>

// ---- thresholds ----------------------------------------------------------------------------------------------------------------
// measured (tools/lab): the 256 x 256 tile wins from ~1 wave of blocks up, also with masked edge tiles; smaller problems take the 128 x 128 tile
constexpr long long GEMM_BIG_MIN_TILES = 192;
constexpr int W4_MIN_K = 192;          // the persistent kernels' K loop needs >= 3 slices of 64
constexpr int W4_REPKV_HD = 64;        // ... and with REPKV a K slice must lie inside one head
constexpr int W4N_BN = 288;            // n tile of the 288 x 224 geometry (gemm_w4n.h)
// the widths the 288 x 224 geometry takes over from the 256-wide kernel (SigLIP: N = 1 152, q | k | v = 3 456)
__host__ __device__ inline bool w4n_takes(int N) { return N >= W4N_BN && N % W4N_BN == 0 && N % 256 != 0; }
// partial-sum entries per row that the statistics epilogue of that geometry writes for an output width N
__host__ __device__ inline int w4n_stat_strips(int N) { return 4 * ((N + W4N_BN - 1) / W4N_BN); }

// ---- environment switches (A/B arms; every setting computes the same results) ------------------------------------------------
struct GemmEnv {
    int big_cfg = 5;                   // VIDI_GEMM_CFG: 4 or 5, the large-tile kernel of the automatic route
    bool w4n = true;                   // VIDI_W4N=0: the 256-wide kernel everywhere (the partial-sum layout follows the switch)
    bool w4n_qkv = true;               // VIDI_W4N_QKV=0: the 256-wide kernel for the LayerNorm-folded head-major q | k | v projection
};
inline const GemmEnv& gemm_env() {     // read once per process
    static const GemmEnv env = [] {
        const char *c = getenv("VIDI_GEMM_CFG"), *n = getenv("VIDI_W4N"), *q = getenv("VIDI_W4N_QKV");
        return GemmEnv{c && atoi(c) == 4 ? 4 : 5, !(n && n[0] == '0'), !(q && q[0] == '0')};
    }();
    return env;
}

// ---- the instantiations ----------------------------------------------------------------------------------------------------------
// Tile kernels (gemm_tile.h), gemm.hip, each for every MODE (x REPKV) and dtype:
//   X(enumerator, tile_cfg, BN, BM, WN, WM, STAGES, SCHED, MFMA size, MODE_PLAIN only)
#define VIDI_TILE_KERNELS(X)                                                                                                        \
    X(GK_TILE_128x128, 0, 128, 128, 2, 2, 2, SCHED_RING, 32, false)     /* small problems; the only tile with the folded LayerNorm */ \
    X(GK_TILE_128x256, 1, 128, 256, 2, 4, 3, SCHED_RING, 32, false)                                                                 \
    X(GK_TILE_256x256, 2, 256, 256, 2, 4, 2, SCHED_RING, 32, false)                                                                 \
    X(GK_TILE_256x256_LATE, 4, 256, 256, 2, 4, 2, SCHED_LATE, 16, false)  /* 8 waves x (128x64), 16x16x32 MFMA */                     \
    X(GK_TILE_192x256_LATE, 11, 192, 256, 2, 4, 2, SCHED_LATE, 16, true)  /* 192-wide n tile (N = 1152: 6 exact tiles instead of 4.5) */
// Persistent 4-wave kernel, 256 x 256 tiles (gemm_w4.h), each for both dtypes:
//   X(enumerator, MODE, REPKV, Epi<BIAS, ACT, RES, LNF, STATS, HEADS>)       RES: 0 none, 1 row m, 2 row m % rmod
#define VIDI_W4_PLAIN_KERNELS(X)           /* gemm_w4_bf16.hip, gemm_w4_f16.hip */                                                   \
    X(GK_W4_REPKV_RES, MODE_PLAIN, true, false, ACT_NONE, 1, 0, false, false)                                                        \
    X(GK_W4_REPKV, MODE_PLAIN, true, false, ACT_NONE, 0, 0, false, false)                                                            \
    X(GK_W4_RES, MODE_PLAIN, false, false, ACT_NONE, 1, 0, false, false)            /* x += proj(...)  (mistral.py:219-221, :135) */   \
    X(GK_W4, MODE_PLAIN, false, false, ACT_NONE, 0, 0, false, false)                /* bias-free projections */                      \
    X(GK_W4_BIAS, MODE_PLAIN, false, true, ACT_NONE, 0, 0, false, false)            /* projector second linear */                    \
    X(GK_W4_BIAS_RES, MODE_PLAIN, false, true, ACT_NONE, 1, 0, false, false)        /* encoder out_proj / fc2 + residual */          \
    X(GK_W4_BIAS_RMOD, MODE_PLAIN, false, true, ACT_NONE, 2, 0, false, false)       /* patch embedding + position table */           \
    X(GK_W4_BIAS_TANH, MODE_PLAIN, false, true, ACT_GELU_TANH, 0, 0, false, false)  /* SigLIP fc1 */                                 \
    X(GK_W4_BIAS_ERF, MODE_PLAIN, false, true, ACT_GELU_ERF, 0, 0, false, false)    /* Whisper fc1 / conv1, projector first linear */ \
    X(GK_W4_BIAS_ERF_RES, MODE_PLAIN, false, true, ACT_GELU_ERF, 1, 0, false, false) /* Whisper conv2 + embed_positions (one window per batch entry) */ \
    X(GK_W4_BIAS_ERF_RMOD, MODE_PLAIN, false, true, ACT_GELU_ERF, 2, 0, false, false) /* the same with the table repeating inside M */
#define VIDI_W4_LNF_KERNELS(X)             /* gemm_w4_lnf.hip: LayerNorm folded into the encoder towers' projections, and its producer */ \
    X(GK_W4_BIAS_RES_STATS, MODE_PLAIN, false, true, ACT_NONE, 1, 0, true, false)   /* out_proj / fc2 + residual, emits the rows' per-strip partial sums */ \
    X(GK_W4_QKV_VT_LNF, MODE_QKV_VT, false, true, ACT_NONE, 0, 1, false, false)     /* LayerNorm -> q/k/v projection, V transposed */ \
    X(GK_W4_LNF_HEADS, MODE_PLAIN, false, true, ACT_NONE, 0, 1, false, true)        /* LayerNorm -> q/k/v projection, head-major */  \
    X(GK_W4_LNF, MODE_PLAIN, false, true, ACT_NONE, 0, 1, false, false)                                                              \
    X(GK_W4_LNF_TANH, MODE_PLAIN, false, true, ACT_GELU_TANH, 0, 1, false, false)   /* SigLIP LayerNorm -> fc1 */                    \
    X(GK_W4_LNF_ERF, MODE_PLAIN, false, true, ACT_GELU_ERF, 0, 1, false, false)     /* Whisper LayerNorm -> fc1 */
#define VIDI_W4_MODES_KERNELS(X)           /* gemm_w4_modes.hip: GeGLU / QKV + V-transpose / K,V cache tiles */                      \
    X(GK_W4_GEGLU, MODE_GEGLU, false, false, ACT_NONE, 0, 0, false, false)                                                           \
    X(GK_W4_QKV_VT_BIAS, MODE_QKV_VT, false, true, ACT_NONE, 0, 0, false, false)                                                     \
    X(GK_W4_QKV_VT, MODE_QKV_VT, false, false, ACT_NONE, 0, 0, false, false)                                                         \
    X(GK_W4_KV_CACHE, MODE_KV_CACHE, false, false, ACT_NONE, 0, 0, false, false)
// Persistent 4-wave kernel, 288 x 224 tiles (gemm_w4n.h), gemm_w4n.hip: takes these epilogues over at the w4n_takes() widths, batch 1
#define VIDI_W4N_KERNELS(X)                                                                                                         \
    X(GK_W4N_BIAS_RES_STATS, MODE_PLAIN, false, true, ACT_NONE, 1, 0, true, false)                                                   \
    X(GK_W4N_BIAS_RES, MODE_PLAIN, false, true, ACT_NONE, 1, 0, false, false)       /* SigLIP out_proj / fc2 (N = 1 152) */           \
    X(GK_W4N_LNF_HEADS, MODE_PLAIN, false, true, ACT_NONE, 0, 1, false, true)       /* SigLIP q | k | v (N = 3 456 = 12 x 288) */

#define VIDI_GK_ENUM(name, ...) name,
enum GemmKernel {
    GK_REGSTAGE,                       // tile_cfg 3: register-staged 128 x 128 (global_load -> ds_write), MODE_PLAIN with the bias epilogue (gemm.hip)
    VIDI_TILE_KERNELS(VIDI_GK_ENUM) GK_TILE_END,
    VIDI_W4_PLAIN_KERNELS(VIDI_GK_ENUM) GK_W4_PLAIN_END,
    VIDI_W4_LNF_KERNELS(VIDI_GK_ENUM) GK_W4_LNF_END,
    VIDI_W4_MODES_KERNELS(VIDI_GK_ENUM) GK_W4_MODES_END,
    VIDI_W4N_KERNELS(VIDI_GK_ENUM)
};

struct GemmEpi { int mode; bool repkv, bias; int act, res, lnf; bool stats, heads; };
struct GemmEpiRow { GemmKernel kernel; GemmEpi e; };
#define VIDI_GK_ROW(name, ...) {name, {__VA_ARGS__}},
constexpr GemmEpiRow W4_KERNELS[] = {VIDI_W4_PLAIN_KERNELS(VIDI_GK_ROW) VIDI_W4_LNF_KERNELS(VIDI_GK_ROW) VIDI_W4_MODES_KERNELS(VIDI_GK_ROW)};
constexpr GemmEpiRow W4N_KERNELS[] = {VIDI_W4N_KERNELS(VIDI_GK_ROW)};

template <int COUNT>
inline const GemmEpiRow* gemm_find(const GemmEpiRow (&rows)[COUNT], const GemmEpi& e) {
    for (const GemmEpiRow& r : rows)
        if (r.e.mode == e.mode && r.e.repkv == e.repkv && r.e.bias == e.bias && r.e.act == e.act && r.e.res == e.res && r.e.lnf == e.lnf &&
            r.e.stats == e.stats && r.e.heads == e.heads) return &r;
    return nullptr;
}

// ---- the statistics layout -------------------------------------------------------------------------------------------------------
// (sum, sum^2) entries per row of GemmParams::stat_part: the 288-wide kernel's layout exactly where gemm_w4n_width() lets it run (a function
// of N and VIDI_W4N alone); the unfused pass (vidi_row_partials_dispatch) writes whichever layout it is told
inline bool gemm_w4n_width(int N, const GemmEnv& env) { return env.w4n && w4n_takes(N); }
inline int gemm_stat_strips(int N, const GemmEnv& env) { return gemm_w4n_width(N, env) ? w4n_stat_strips(N) : (N + 127) / 128; }

// ---- the route -----------------------------------------------------------------------------------------------------------------
struct GemmRoute {
    int err = 0;                       // VIDI_ERR_*: nothing is launched
    GemmKernel kernel = GK_REGSTAGE;
    bool row_partials = false;         // a call with stat_part: the kernel does not emit the partial sums, vidi_row_partials_dispatch follows it
    int strips = 0;                    // ... and the entries per row of stat_part
};

// tile_cfg (include/vidi_hip.h): < 0 automatic, 0 1 2 4 11 a tile kernel, 3 register-staged, 5 the persistent kernel.  A call with
// p.stat_part (vidi_gemm_res_stats) gets the fused statistics where the persistent kernel runs, otherwise tile_cfg's kernel + row partials.
inline GemmRoute gemm_route(const GemmParams& p, int batch, int mode, int repkv, int tile_cfg, int dtype, const GemmEnv& env) {
    GemmRoute r;
    const auto fail = [&r](int code) { r.err = code; return r; };
    if (tile_cfg == 3 && (mode != MODE_PLAIN || p.ln_stats)) return fail(VIDI_ERR_ARG);      // the register-staged kernel has the bias epilogue only
    if (p.M <= 0 || p.N <= 0 || p.K <= 0 || batch <= 0 || p.K % 64 != 0 || p.N % 32 != 0 || (mode == MODE_GEGLU && p.N % 64 != 0)) return fail(VIDI_ERR_SHAPE);
    const uintptr_t ptrs = (uintptr_t)p.X | (uintptr_t)p.W | (uintptr_t)p.Y | (uintptr_t)p.R | (mode == MODE_KV_CACHE ? (uintptr_t)p.Kc | (uintptr_t)p.Vrow : 0);
    if ((ptrs & 15) || ((p.ldx | p.ldw | p.ldy | (p.R ? p.ldr : 0) | (mode == MODE_KV_CACHE ? p.hd : 0)) & 7)) return fail(VIDI_ERR_ALIGN);      // 16-byte pieces
    if (dtype != VIDI_DT_BF16 && dtype != VIDI_DT_F16) return fail(VIDI_ERR_DTYPE);
    if (mode != MODE_PLAIN && mode != MODE_GEGLU && mode != MODE_QKV_VT && mode != MODE_KV_CACHE) return fail(VIDI_ERR_ARG);

    // the epilogue asked for, in the terms of the tables above (GEGLU / KV_CACHE have one; QKV_VT has bias or the folded LayerNorm)
    const bool lnf = p.ln_stats != nullptr;
    GemmEpi e = {mode, false, false, ACT_NONE, 0, 0, false, false};
    if (mode == MODE_PLAIN) e = {mode, repkv != 0, p.bias || lnf, p.act, p.R ? (p.rmod < p.M ? 2 : 1) : 0, lnf, false, p.hm_seq != 0};
    if (mode == MODE_QKV_VT) { e.bias = p.bias || lnf; e.lnf = lnf; }
    const bool big = (long long)((p.N + 255) / 256) * ((p.M + 255) / 256) * batch >= GEMM_BIG_MIN_TILES;
    const bool w4_fits = p.K >= W4_MIN_K && !(e.repkv && p.rep_hd % W4_REPKV_HD);
    if (p.stat_part) {
        r.strips = gemm_stat_strips(p.N, env);
        e.stats = (tile_cfg < 0 || tile_cfg == 5) && big && w4_fits;
        r.row_partials = !e.stats;
        tile_cfg = e.stats ? 5 : tile_cfg == 5 ? -1 : tile_cfg;
    }

    if (tile_cfg == 3) { r.kernel = GK_REGSTAGE; return r; }
    if (tile_cfg == 5 || (tile_cfg < 0 && big && (env.big_cfg == 5 || lnf))) {
        // persistent kernel; on the automatic route the 8-wave tile kernel covers the plain epilogue combinations it lacks
        const GemmEpiRow* row = w4_fits ? gemm_find(W4_KERNELS, e) : nullptr;
        // the LayerNorm fold and its producer exist on this kernel only (and the 128x128 tile, when asked for by number): no fall-back
        if (w4_fits && (e.lnf || e.stats) && (!row || batch != 1 || (e.lnf && (!p.ln_s || !p.ln_c)))) return fail(VIDI_ERR_ARG);
        if (row) {
            const GemmEpiRow* n = (batch == 1 && gemm_w4n_width(p.N, env)) ? gemm_find(W4N_KERNELS, e) : nullptr;
            if (n && e.heads && !(env.w4n_qkv && p.hm_hd % 8 == 0)) n = nullptr;          // a 16-byte chunk lies inside one head
            r.kernel = n ? n->kernel : row->kernel;
            return r;
        }
        if (tile_cfg == 5) return fail(VIDI_ERR_ARG);
    }
    if (tile_cfg < 0) tile_cfg = (big && !lnf) ? 4 : 0;
    if ((lnf || p.hm_seq) && tile_cfg != 0) return fail(VIDI_ERR_ARG);                     // folded LayerNorm: persistent kernel or the 128x128 tile
#define VIDI_GK_ROUTE_TILE(name, cfg, BN, BM, WN, WM, ST, SCHED, MI, PLAIN_ONLY) \
    if (tile_cfg == cfg && !(PLAIN_ONLY && mode != MODE_PLAIN)) { r.kernel = name; return r; }
    VIDI_TILE_KERNELS(VIDI_GK_ROUTE_TILE)
    return fail(VIDI_ERR_ARG);
}
