// Which GEMM kernel runs for a call: prints what gemm_route() (vidi_amd/csrc/gemm_route.h) decides, without a GPU.
//
//   hipcc --cuda-host-only -std=c++17 tools/gemm_route_dump.hip -o gemm_route_dump      (add -fsanitize=address,undefined for a checked run)
//   echo "gemm M=16384 N=1152 K=4352 bias=1 res=1" | ./gemm_route_dump
//       -> w4n<Epi<true,ACT_NONE,1,0,false,false>> bf16
//
// One case per line on stdin: the C entry point (vidi_<kind> of include/vidi_hip.h) and key=value pairs; one line per case on stdout:
// the instantiation's template arguments and dtype (a tile kernel: also MODE and REPKV), or `err <code>`; a vidi_gemm_res_stats call adds
// `+row_partials` when the statistics are not fused into the kernel, and the partial-sum entries per row.
//   kinds   gemm geglu glu qkv_vt res_stats gemm_ln ln_heads qkv_vt_ln kv_cache
//   keys    M N K (N: the GEMM's output width, 2 * I for geglu / glu, 2 * kvd for kv_cache)   ldx ldw ldy ldr (default: dense)   batch
//           bias res (0 / 1: pointer given)   rmod act   rep_hd rep_g   seq hd (ln_heads)   cfg (tile_cfg)   dtype
//           env_cfg w4n w4n_qkv (VIDI_GEMM_CFG, VIDI_W4N, VIDI_W4N_QKV; default 5 1 1)
// tests/test_gemm_route.py feeds it tests/golden/gemm_routes.json.
#include "../vidi_amd/csrc/gemm_route.h"
#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

// an instantiation's template arguments, spelled from its row of the tables in gemm_route.h (dtype, and MODE / REPKV of a tile kernel, follow)
static const char* gemm_kernel_name(GemmKernel k) {
    switch (k) {
        case GK_REGSTAGE: return "regstage<128x128>";
#define VIDI_GK_NAME_TILE(name, cfg, BN, BM, WN, WM, ST, SCHED, MI, PO) case name: return "tile<" #BN "x" #BM ",waves=" #WN "x" #WM ",stages=" #ST "," #SCHED ",mfma" #MI ">";
        VIDI_TILE_KERNELS(VIDI_GK_NAME_TILE)
#define VIDI_GK_NAME_W4(name, MODE, REPKV, B, A, R, L, S, H) case name: return "w4<" #MODE ",repkv=" #REPKV ",Epi<" #B "," #A "," #R "," #L "," #S "," #H ">>";
        VIDI_W4_PLAIN_KERNELS(VIDI_GK_NAME_W4) VIDI_W4_LNF_KERNELS(VIDI_GK_NAME_W4) VIDI_W4_MODES_KERNELS(VIDI_GK_NAME_W4)
#define VIDI_GK_NAME_W4N(name, MODE, REPKV, B, A, R, L, S, H) case name: return "w4n<Epi<" #B "," #A "," #R "," #L "," #S "," #H ">>";
        VIDI_W4N_KERNELS(VIDI_GK_NAME_W4N)
        default: return "?";
    }
}

int main() {
    static const char* const MODES[] = {"MODE_PLAIN", "MODE_GEGLU", "MODE_QKV_VT", "MODE_KV_CACHE"};
    u16* const ptr = (u16*)0x1000;                    // never dereferenced: only null-ness and alignment matter to the route
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind, tok;
        if (!(in >> kind)) continue;
        std::map<std::string, int> v;
        while (in >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "bad token '%s'\n", tok.c_str()); return 2; }
            v[tok.substr(0, eq)] = atoi(tok.c_str() + eq + 1);
        }
        const auto get = [&v](const char* key, int dflt) { const auto it = v.find(key); return it == v.end() ? dflt : it->second; };
        GemmParams p = {};
        p.M = get("M", 0); p.N = get("N", 0); p.K = get("K", 0);
        p.X = ptr; p.W = ptr; p.Y = ptr;
        p.ldx = get("ldx", p.K); p.ldw = get("ldw", p.K); p.ldy = get("ldy", p.N); p.ldr = get("ldr", p.N);
        p.rmod = 0x7fffffff;
        int mode = MODE_PLAIN, batch = 1, repkv = 0;
        const bool ln = kind == "gemm_ln" || kind == "ln_heads" || kind == "qkv_vt_ln";
        if (ln) { p.ln_stats = (const float*)ptr; p.ln_s = (const float*)ptr; p.ln_c = (const float*)ptr; }
        if (kind == "gemm") {
            batch = get("batch", 1); p.act = get("act", 0);
            if (get("bias", 0)) p.bias = ptr;
            if (get("res", 0)) p.R = ptr;
            if (get("rmod", 0) > 0) p.rmod = get("rmod", 0);
            repkv = get("rep_hd", 0) > 0 && get("rep_g", 0) > 1;
            if (repkv) { p.rep_hd = get("rep_hd", 0); p.rep_g = get("rep_g", 0); }
        } else if (kind == "geglu" || kind == "glu") {
            mode = MODE_GEGLU; p.act = get("act", 0);
        } else if (kind == "qkv_vt" || kind == "qkv_vt_ln") {
            mode = MODE_QKV_VT;
            if (get("bias", 0) && !ln) p.bias = ptr;
        } else if (kind == "res_stats") {
            p.bias = ptr; p.R = ptr; p.stat_part = (float*)ptr;
        } else if (kind == "gemm_ln") {
            p.act = get("act", 0);
        } else if (kind == "ln_heads") {
            p.ldy = p.N; p.hm_seq = get("seq", 0); p.hm_hd = get("hd", 0);
        } else if (kind == "kv_cache") {
            mode = MODE_KV_CACHE; p.ldy = p.N / 2; p.hd = get("hd", 0); p.Kc = ptr; p.Vrow = ptr;
        } else {
            fprintf(stderr, "unknown kind '%s'\n", kind.c_str());
            return 2;
        }
        GemmEnv env;
        env.big_cfg = get("env_cfg", 5); env.w4n = get("w4n", 1) != 0; env.w4n_qkv = get("w4n_qkv", 1) != 0;
        const int dtype = get("dtype", VIDI_DT_BF16);
        const GemmRoute r = gemm_route(p, batch, mode, repkv, get("cfg", -1), dtype, env);
        if (r.err) { printf("err %d\n", r.err); continue; }
        printf("%s %s", gemm_kernel_name(r.kernel), dtype == VIDI_DT_BF16 ? "bf16" : "f16");
        if (r.kernel < GK_TILE_END) printf(" %s repkv=%d", MODES[mode], repkv);
        if (p.stat_part) printf("%s strips=%d", r.row_partials ? " +row_partials" : "", r.strips);
        printf("\n");
    }
    return 0;
}
